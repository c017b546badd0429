"""Frames and masks for the tests of the bad-pixel masks of apply (``mask=``, ``fill_nonfinite=``; DESIGN.md 3.8, "Bad-pixel masks"), their
reference and the preconditions, shared between the emulator tests (tests/test_mask_host.py) and the GPU tests (tests/test_gpu_mask.py).

The definition, on the 2N-padded frame ``P = np.pad(image, 2N, pad_mode)``::

    hot = P > threshold;  M = binary_dilation(hot, iterations=dilation) if hot.any() else hot
    E   = pad(mask) through the pad mode's index map (False in the pad of 'constant');  if fill_nonfinite: E |= ~isfinite(P)
    M2  = M | E;  P[M2] = nan;  raster-order nan-mean fill of M2;  out = correct(P);  out[M2] = raw[M2];  crop

The reference of the filled padded frame is ``rpsf_saturation_fill`` (the host route's fill, no GPU involved) on the float32 frame padded
by NumPy with M2 from NumPy / SciPy.  What a case is there for is asserted by ``precondition`` from NumPy / SciPy alone, before anything
under test runs.
"""

from __future__ import annotations

import functools
import pathlib

import numpy as np

from regularizepsf_amd import _native
from tests import saturation_cases as sc

N = 16
THRESHOLD = sc.THRESHOLD
HOT = sc.HOT
ODD, QUADS = (37, 51), (40, 48)  # padded 101 x 115 (an odd pixel count: F1's scalar tail runs) and 104 x 112 (all quads)
INDEX_MAP_MODES = ("symmetric", "reflect", "edge", "wrap")


# ---------------------------------------------------------------------------------------------------------------- frames and masks
def _plain(shape, seed):
    return sc.background(*shape, seed), np.zeros(shape, bool)


def _pixel_first(shape):
    im, m = _plain(shape, 21)
    m[0, 0] = True
    return im, m


def _pixel_last(shape):
    im, m = _plain(shape, 22)
    m[-1, -1] = True
    im[shape[0] // 2, shape[1] // 2] = HOT  # a saturated pixel elsewhere: M and E both at work
    return im, m


def _block(shape):
    im, m = _plain(shape, 23)
    m[14:18, 20:25] = True
    return im, m


def _row(shape):
    im, m = _plain(shape, 24)
    m[18, :] = True
    # but for the pixels that 'wrap' brings into the first columns of the padded frame, where the window [j - h, j + h) is empty (h = 4):
    # the row stays one fill group, since the grown mask bridges a gap of four
    m[18, [(c - 2 * N) % shape[1] for c in range(4)]] = False
    return im, m


def _overlap(shape):
    im, m = _plain(shape, 25)
    im[20:23, 20:23] = HOT
    m[21:27, 22:30] = True  # covers part of the blob, part of its dilation and pixels beyond it
    return im, m


def _nan_under(shape):
    im, m = _plain(shape, 26)
    m[8:11, 20:24] = True  # (its mirror images stay clear of the padded frame's first columns, where a window is empty)
    im[9, 21] = np.nan
    im[9, 22] = np.inf
    im[shape[0] // 2, 5] = HOT
    return im, m


def _nonfinite(shape):
    im, m = _plain(shape, 27)
    m[5:7, 5:8] = True
    im[20, 20] = np.nan
    im[20, 21] = np.nan
    im[28, 40] = np.inf  # above any finite threshold as well: hot, so dilated
    im[12, 33] = -np.inf
    im[0, 25] = np.nan  # on the rim
    return im, m


# name -> (maker, (H, W), pad mode, (dilation, width), threshold, fill_nonfinite, mask storage)
CASES = {
    "pixel_first": (_pixel_first, ODD, "symmetric", (1, 7), np.inf, False, "dense"),
    "pixel_last": (_pixel_last, QUADS, "reflect", (2, 5), THRESHOLD, False, "dense"),
    "block": (_block, ODD, "edge", (1, 3), np.inf, False, "dense"),
    "row_wrap": (_row, ODD, "wrap", (1, 9), THRESHOLD, False, "dense"),
    "overlap_blob": (_overlap, QUADS, "constant", (3, 2), THRESHOLD, False, "dense"),
    "nan_under": (_nan_under, ODD, "symmetric", (2, 5), THRESHOLD, False, "dense"),
    "nonfinite": (_nonfinite, ODD, "constant", (1, 7), THRESHOLD, True, "dense"),
    "nonfinite_only": (_nonfinite, QUADS, "reflect", (1, 7), np.inf, True, "none"),
    "strided": (_block, QUADS, "wrap", (1, 9), THRESHOLD, False, "strided"),
    "empty_mask": (lambda shape: _plain(shape, 28), ODD, "symmetric", (1, 7), np.inf, False, "dense"),
}
assert {c[3] for c in CASES.values()} == set(sc.PARAMS)
assert {c[2] for c in CASES.values()} == set(_native.PAD_MODES)
assert {c[1] for c in CASES.values()} == {ODD, QUADS}

# one batch of three ODD frames: busy, idle (empty mask, nothing hot), busy
BATCH = ("block", "empty_mask", "pixel_first")
BATCH_SETTINGS = ("symmetric", (1, 7), THRESHOLD, False)


@functools.cache
def _made(name: str):
    make, shape = CASES[name][:2]
    im, m = make(shape)
    im.flags.writeable = m.flags.writeable = False
    return im, m


def frame(name: str) -> np.ndarray:
    return _made(name)[0]


def mask(name: str) -> np.ndarray | None:
    """The caller's mask as a bool array (None: the case gives none)."""
    return None if CASES[name][6] == "none" else _made(name)[1]


def stored(m: np.ndarray | None, storage: str) -> np.ndarray | None:
    """``m`` as the uint8 array the entry points take: dense, or a view with a row pitch and a column stride of 2 whose other bytes are 1."""
    if m is None:
        return None
    if storage != "strided":
        return np.ascontiguousarray(m, np.uint8)
    h, w = m.shape
    store = np.ones((h, 2 * w + 6), np.uint8)
    view = store[:, 3 : 3 + 2 * w : 2]
    view[...] = m
    assert view.strides == (2 * w + 6, 2) and np.array_equal(view.astype(bool), m)
    return view


# ---------------------------------------------------------------------------------------------------------------- reference
def pad_mask(m: np.ndarray | None, shape, n: int, pad_mode: str) -> np.ndarray:
    if m is None:
        return np.zeros((shape[0] + 4 * n, shape[1] + 4 * n), bool)
    if pad_mode in INDEX_MAP_MODES:
        return np.pad(m, 2 * n, mode=pad_mode)
    return np.pad(m, 2 * n, mode="constant", constant_values=False)


def reference_fill(image, m, n, pad_mode, dilation, width, threshold, fill_nonfinite):
    """(filled padded frame as float64, M2, hot, E, raw padded frame) by NumPy, SciPy and the host route's fill on the float32 frame."""
    from scipy.ndimage import binary_dilation

    assert image.dtype == np.float32
    padded = np.pad(image.astype(np.float64), ((2 * n, 2 * n), (2 * n, 2 * n)), mode=pad_mode)
    raw = padded.copy()
    hot = padded > threshold
    dilated = binary_dilation(hot, iterations=dilation) if hot.any() else hot.copy()
    exact = pad_mask(m, image.shape, n, pad_mode)
    if fill_nonfinite:
        exact |= ~np.isfinite(padded)
    m2 = dilated | exact
    if m2.any():
        padded[m2] = np.nan
        _native.saturation_fill(padded, m2, width)
    return padded, m2, hot, exact, raw


@functools.cache
def reference(name: str):
    """Computed once per case and shared; callers must not write to it."""
    _, _, pad_mode, (dilation, width), threshold, fill_nonfinite, _ = CASES[name]
    out = reference_fill(frame(name), mask(name), N, pad_mode, dilation, width, threshold, fill_nonfinite)
    for a in out:
        a.flags.writeable = False
    return out


@functools.cache
def batch_reference():
    pad_mode, (dilation, width), threshold, fill_nonfinite = BATCH_SETTINGS
    out = [reference_fill(frame(name), mask(name), N, pad_mode, dilation, width, threshold, fill_nonfinite) for name in BATCH]
    for a in (x for o in out for x in o):
        a.flags.writeable = False
    return out


def every_window_has_a_value(filled: np.ndarray, m2: np.ndarray) -> bool:
    """Every fill window held a finite unmasked or already-filled pixel: the sequential fill left no NaN on M2."""
    return bool(np.isfinite(filled[m2]).all())


def precondition(name: str) -> None:
    """The case contains what it is named for - from the frame, the mask, NumPy and SciPy alone."""
    make, (h, w), pad_mode, (dilation, width), threshold, fill_nonfinite, storage = CASES[name]
    image, m = frame(name), mask(name)
    filled, m2, hot, exact, raw = reference(name)
    inner = (slice(2 * N, 2 * N + h), slice(2 * N, 2 * N + w))
    assert image.shape == (h, w) and m2.shape == (h + 4 * N, w + 4 * N)
    assert ((h + 4 * N) * (w + 4 * N)) % 4 == (3 if (h, w) == ODD else 0), "F1's scalar tail runs on the odd shape only"
    assert every_window_has_a_value(filled, m2), "no pixel of M2 may stay NaN: nothing is left out of the comparisons"
    assert np.isfinite(filled[~m2]).all(), "the reference is finite off M2 too"
    if m is not None:
        assert (m2[inner] >= (hot[inner] | m)).all(), "M2 holds the hot pixels and the caller's mask"
    if name == "pixel_first":
        assert m[0, 0] and m.sum() == 1 and not hot.any() and m2.sum() > 1, "mirror images in the pad are masked too"
    elif name == "pixel_last":
        assert m[h - 1, w - 1] and m.sum() == 1 and hot[inner].sum() == 1
    elif name in ("block", "strided"):
        assert m.sum() == 20 and m[14:18, 20:25].all()
        if storage == "strided":
            assert stored(m, storage).strides == (2 * w + 6, 2)
    elif name == "row_wrap":
        from scipy.ndimage import binary_dilation, label

        reach = (width // 2) // 2  # F3's box growth
        labels, _ = label(binary_dilation(m2, structure=np.ones((2 * reach + 1, 2 * reach + 1))), structure=np.ones((3, 3)))
        row = 2 * N + 18
        assert pad_mode == "wrap" and m.sum() == w - 4 and m2[row].sum() > 64 and len(set(labels[row][m2[row]])) == 1, \
            "one fill group with more than 64 masked pixels in one row of the padded frame"
        assert m2[[row - h, row + h]].sum(axis=1).min() > 64, "and its images above and below"
    elif name == "overlap_blob":
        from scipy.ndimage import binary_dilation

        dilated = binary_dilation(hot, iterations=dilation)
        assert (dilated & exact).any() and (dilated & ~exact).any() and (exact & ~dilated).any() and (hot & exact).any()
    elif name == "nan_under":
        bad = ~np.isfinite(image)
        assert bad.sum() == 2 and m[bad].all() and not fill_nonfinite
    elif name.startswith("nonfinite"):
        bad = ~np.isfinite(image)
        assert fill_nonfinite and np.isnan(image).any() and np.isposinf(image).any() and (m is None or not (m & bad).any())
        assert m2[~np.isfinite(raw)].all()
        if np.isfinite(threshold):
            r, c = np.argwhere(np.isposinf(image))[0]
            assert m2[2 * N + r + 1, 2 * N + c] and not m2[2 * N + 21, 2 * N + 20], "+Inf is hot and dilated, NaN is masked as it is"
        else:
            assert m2.sum() == (~np.isfinite(raw)).sum(), "nothing is dilated"
    elif name == "empty_mask":
        assert m is not None and not m.any() and not m2.any()
    if pad_mode in INDEX_MAP_MODES and m is not None and m.any() and name != "pixel_last":
        outside = exact.copy()
        outside[inner] = False
        assert outside.any() or name in ("block", "nan_under"), "the mask follows the image into the pad"
    if pad_mode == "constant" and m is not None:
        outside = pad_mask(m, (h, w), N, pad_mode)
        outside[inner] = False
        assert not outside.any()


def batch_precondition() -> None:
    refs = batch_reference()
    assert all(frame(name).shape == ODD for name in BATCH)
    assert refs[0][1].any() and refs[2][1].any() and not refs[1][1].any() and not refs[1][2].any(), "an idle frame between two busy ones"
    for filled, m2, *_ in refs:
        assert every_window_has_a_value(filled, m2) and np.isfinite(filled).all()


# ---------------------------------------------------------------------------------------------------------------- emulator
@functools.cache
def emulator():
    """tests/emu/libemu_mask.so: the masked drivers of kernels F1 - F5 on the CPU.  __graft_entry__.build() compiles it; it is compiled
    here when it is missing or older than its sources.  Without a compiler that is an error, not a skip."""
    import ctypes
    import os
    import shutil
    import subprocess

    root = pathlib.Path(__file__).resolve().parent.parent
    src, out = root / "tests" / "emu" / "emu_mask.cpp", root / "tests" / "emu" / "libemu_mask.so"
    cores = [root / "regularizepsf_amd" / "csrc" / n for n in ("rpsf_core_saturation.hpp", "rpsf_core_saturation_batch.hpp", "rpsf_core_stars.hpp")]
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, *(c.stat().st_mtime for c in cores)):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++") or shutil.which("hipcc")
        assert clang is not None, "no clang++ to build tests/emu/emu_mask.cpp"
        fresh = out.with_name(f"libemu_mask.{os.getpid()}.so")  # written aside and moved into place: test processes may run side by side
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(fresh), str(src)], check=True)
        os.replace(fresh, out)
    lib = ctypes.CDLL(str(out))
    p, i, d, z, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.c_long
    lib.emumask_fill.argtypes = [p, i, i, i, i, d, i, i, p, l, l, i, p, p, p]
    lib.emumask_fill_batch.argtypes = [p, i, z, i, i, i, i, d, i, i, i, p, i, z, l, l, i, p, p, p]
    lib.emumask_restore_batch.argtypes = [p, i, z, i, i, i, i, d, i, i, p, i, z, l, l, i, p, z, i, p, z, p, p]
    return lib


def _mask_args(masks):
    """(pointer, n_masks, frame bytes, row stride, column stride, keep-alive) of a uint8 array (n_masks, H, W) or None."""
    if masks is None:
        return None, 0, 0, 0, 0, None
    assert masks.dtype == np.uint8 and masks.ndim == 3
    return masks.ctypes.data, masks.shape[0], masks.strides[0], masks.strides[1], masks.strides[2], masks


def emu_fill(image, m, n, pad_mode, dilation, width, threshold, fill_nonfinite):
    """F1 - F4 of one frame by the single-frame functions: (filled padded float32 frame, M2, (hot, exact, masked, groups)).
    ``m``: None or a uint8 array at any positive strides."""
    image = np.ascontiguousarray(image, np.float32)
    shape = (image.shape[0] + 4 * n, image.shape[1] + 4 * n)
    padded, out_mask, counts = np.full(shape, -3.0, np.float32), np.full(shape, 7, np.uint8), np.full(4, -1, np.int32)
    assert emulator().emumask_fill(image.ctypes.data, *image.shape, n, _native.PAD_MODES[pad_mode], threshold, dilation, width,
                                   None if m is None else m.ctypes.data, *((0, 0) if m is None else m.strides), int(fill_nonfinite),
                                   padded.ctypes.data, out_mask.ctypes.data, counts.ctypes.data) == 0
    return padded, out_mask.astype(bool), tuple(int(c) for c in counts)


def emu_fill_batch(images, masks, n, pad_mode, dilation, width, threshold, fill_nonfinite, order=0):
    """F1 - F4 of a frame-group through the batch drivers: (padded frames, M2 per frame, counts (frames, 4)).
    ``masks``: None or a uint8 array (1 or frames, H, W) at any positive strides."""
    stack = np.ascontiguousarray(np.stack([np.asarray(im, np.float32) for im in images]))
    f, h, w = stack.shape
    shape = (f, h + 4 * n, w + 4 * n)
    padded, out_masks, counts = np.full(shape, -3.0, np.float32), np.full(shape, 7, np.uint8), np.full((f, 4), -1, np.int32)
    ptr, n_masks, fb, rs, cs, _keep = _mask_args(masks)
    assert emulator().emumask_fill_batch(stack.ctypes.data, f, h * w, h, w, n, _native.PAD_MODES[pad_mode], threshold, dilation, width, order,
                                         ptr, n_masks, fb, rs, cs, int(fill_nonfinite), padded.ctypes.data, out_masks.ctypes.data,
                                         counts.ctypes.data) == 0
    return padded, out_masks.astype(bool), counts


def emu_restore_batch(images, masks, n, pad_mode, dilation, width, threshold, fill_nonfinite, corrected, out_row0):
    """F5 behind F1 - F4 of a frame-group: (results (frames, H, W), per frame the sorted list of its masked in-frame pixels)."""
    stack = np.ascontiguousarray(np.stack([np.asarray(im, np.float32) for im in images]))
    corrected = np.ascontiguousarray(corrected, np.float32)
    f, h, w = stack.shape
    outs, lists, n_lists = np.full(stack.shape, -3.0, np.float32), np.full((f, h * w), -1, np.int32), np.full(f, -1, np.int32)
    ptr, n_masks, fb, rs, cs, _keep = _mask_args(masks)
    assert emulator().emumask_restore_batch(stack.ctypes.data, f, h * w, h, w, n, _native.PAD_MODES[pad_mode], threshold, dilation, width, ptr,
                                            n_masks, fb, rs, cs, int(fill_nonfinite), corrected.ctypes.data, corrected[0].size, out_row0,
                                            outs.ctypes.data, h * w, lists.ctypes.data, n_lists.ctypes.data) == 0
    return outs, [np.sort(lists[i, : n_lists[i]]) for i in range(f)]


@functools.cache
def emulated(name: str):
    """The single-frame emulator's result of a case, computed once and shared (read only)."""
    _, _, pad_mode, (dilation, width), threshold, fill_nonfinite, storage = CASES[name]
    out = emu_fill(frame(name), stored(mask(name), storage), N, pad_mode, dilation, width, threshold, fill_nonfinite)
    out[0].flags.writeable = out[1].flags.writeable = False
    return out


assert_same_bits = sc.assert_same_bits
