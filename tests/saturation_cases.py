"""Frames for the tests of the saturation branch on the device (kernels F1 - F5, csrc/rpsf_core_saturation.hpp), their reference and
the preconditions, shared between the emulator tests (tests/test_saturation_host.py) and the GPU tests (tests/test_gpu_saturation.py).

The reference of the filled padded frame is ``rpsf_saturation_fill`` (the host route's fill, no GPU involved) on the float32 frame
padded by NumPy, with the mask from ``scipy.ndimage.binary_dilation``.  What a case is there for is asserted by ``precondition`` from
NumPy / SciPy alone, before anything under test runs.
"""

from __future__ import annotations

import functools
import pathlib

import numpy as np

from regularizepsf_amd import _native

THRESHOLD = 1000.0
HOT = 5000.0
TILE = 32  # the labeller's tile (rpsf_core_stars.hpp, TILE_R = TILE_C)
PARAMS = ((1, 7), (2, 5), (3, 2), (1, 3), (1, 9))  # (dilation, neighborhood_width); the last has h = 4, a window of 64


# ---------------------------------------------------------------------------------------------------------------- frames
def background(h: int, w: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).uniform(100.0, 200.0, (h, w)).astype(np.float32)


def _isolated(h, w, hh):
    im = background(h, w, 1)
    im[h // 2, w // 2] = HOT
    return im


def _blob(h, w, hh):
    im = background(h, w, 2)
    im[h // 3 : h // 3 + 4, w // 3 : w // 3 + 5] = HOT  # the blob of tests/test_gpu_edge.py
    return im


def _corners_edges(h, w, hh):
    im = background(h, w, 3)
    for r, c in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)):
        im[r, c] = HOT
    return im


def _pair(gap):
    def make(h, w, hh, first=True):
        # dilation 1: the diamonds around (10, 10) and (10 + x, 10 + x) come as close as x - 1 rows and x - 1 columns
        im = background(h, w, 4)
        x = hh + gap + 1
        if first:
            im[10, 10] = HOT
        im[10 + x, 10 + x] = HOT
        return im

    return make


def _column70(h, w, hh):
    im = background(h, w, 5)
    im[10:80, w // 2 - 3] = HOT
    return im


def _row70(h, w, hh):
    im = background(h, w, 6)
    im[h // 2 + 1, 20:90] = HOT
    return im


def _nan_beside(h, w, hh):
    im = background(h, w, 7)
    im[20:23, 20:23] = HOT
    im[21, 18] = np.nan  # left of the dilated blob: unmasked, inside the window [j - h, j + h) of its first pixel in that row
    return im


def _wrap_top(h, w, hh):
    im = background(h, w, 8)
    im[(-2 * 16) % h, w // 2] = HOT  # with N = 16 and 'wrap' this image row is padded row 0
    return im


def _nothing(h, w, hh):
    return background(h, w, 9)


def _fully_hot(h, w, hh):
    return np.full((h, w), HOT, np.float32)


def _mixed(h, w, hh):
    rng = np.random.default_rng(10)
    im = background(h, w, 10)
    for r, c in zip(rng.integers(0, h, 25), rng.integers(0, w, 25)):
        im[r, c] = HOT + r
    im[h // 3 : h // 3 + 4, w // 3 : w // 3 + 5] = HOT
    im[100:170, 150] = HOT
    im[150, 30:100] = HOT
    im[0, 0] = im[h - 1, w - 1] = HOT
    im[60, 61] = np.nan
    return im


# name -> (frame maker, N, (H, W), pad mode, (dilation, width))
CASES = {
    "isolated": (_isolated, 16, (40, 48), "symmetric", (1, 7)),
    "blob": (_blob, 16, (40, 48), "reflect", (2, 5)),
    "corners_edges": (_corners_edges, 16, (40, 48), "symmetric", (1, 3)),
    "corners_edges_wrap": (_corners_edges, 16, (40, 48), "wrap", (1, 7)),
    "pair_h": (_pair(0), 16, (40, 48), "constant", (1, 7)),
    "pair_h_wide": (_pair(0), 16, (40, 48), "constant", (1, 9)),
    "pair_h_plus_1": (_pair(1), 16, (40, 48), "constant", (1, 7)),
    "column70": (_column70, 32, (96, 128), "symmetric", (1, 9)),
    "row70": (_row70, 32, (96, 128), "symmetric", (3, 2)),
    "nan_beside": (_nan_beside, 16, (40, 48), "edge", (1, 3)),
    "wrap_top": (_wrap_top, 16, (40, 48), "wrap", (1, 7)),
    "nothing_hot": (_nothing, 16, (40, 48), "symmetric", (1, 7)),
    "fully_hot": (_fully_hot, 16, (24, 24), "symmetric", (1, 9)),
    "mixed": (_mixed, 64, (200, 192), "symmetric", (2, 5)),
    "mixed_edge": (_mixed, 64, (200, 192), "edge", (3, 2)),
}
assert {c[4] for c in CASES.values()} == set(PARAMS)
assert {c[3] for c in CASES.values() if c[1] == 16 and c[2] == (40, 48)} == set(_native.PAD_MODES)


def frame(name: str) -> np.ndarray:
    make, _, (h, w), _, (_, width) = CASES[name]
    return make(h, w, width // 2)


# ---------------------------------------------------------------------------------------------------------------- reference
def reference_fill(image: np.ndarray, n: int, pad_mode: str, dilation: int, width: int, threshold: float = THRESHOLD):
    """(filled padded frame as float32, mask, hot) by NumPy, SciPy and the host route's fill on the float32 frame."""
    from scipy.ndimage import binary_dilation

    assert image.dtype == np.float32
    padded = np.pad(image.astype(np.float64), ((2 * n, 2 * n), (2 * n, 2 * n)), mode=pad_mode)
    hot = padded > threshold
    mask = binary_dilation(hot, iterations=dilation) if hot.any() else hot.copy()
    padded[mask] = np.nan
    if mask.any():
        _native.saturation_fill(padded, mask, width)
    return padded.astype(np.float32), mask, hot


@functools.cache
def reference(name: str):
    """Computed once per case and shared; callers must not write to it."""
    _, n, _, pad_mode, (dilation, width) = CASES[name]
    out = reference_fill(frame(name), n, pad_mode, dilation, width)
    for a in out:
        a.flags.writeable = False
    return out


def chebyshev_gap(a: np.ndarray, b: np.ndarray) -> int:
    """Smallest max(|row difference|, |column difference|) between a pixel of mask a and one of mask b."""
    pa, pb = np.argwhere(a), np.argwhere(b)
    return int(np.abs(pa[:, None, :] - pb[None, :, :]).max(-1).min())


def precondition(name: str) -> None:
    """The case contains what it is named for - from the frame, NumPy and SciPy alone."""
    from scipy.ndimage import label

    make, n, (h, w), pad_mode, (dilation, width) = CASES[name]
    image = frame(name)
    hh = width // 2
    want, mask, hot = reference(name)
    inner = (slice(2 * n, 2 * n + h), slice(2 * n, 2 * n + w))
    assert image.shape == (h, w) and mask.shape == (h + 4 * n, w + 4 * n)
    assert np.array_equal(np.isnan(want), np.isnan(want) & (mask | np.isnan(np.pad(image, 2 * n, mode=pad_mode)))), "NaN only on the mask or from the frame"
    if name == "isolated":
        assert hot[inner].sum() == 1 and mask[inner].sum() == 2 * dilation * (dilation + 1) + 1
    elif name == "blob":
        assert hot[inner].sum() == 20
        once = np.pad(image.astype(np.float64), 2 * n, mode=pad_mode)
        once[mask] = np.nan
        frozen = once.copy()
        with np.errstate(all="ignore"):
            for i, j in np.argwhere(mask):  # every pixel from the NaN-ed frame alone: no fill sees another
                win = frozen[max(i - hh, 0) : i + hh, max(j - hh, 0) : j + hh]
                once[i, j] = np.nanmean(win) if np.isfinite(win).any() else np.nan
        assert not np.array_equal(once.astype(np.float32)[mask], want[mask], equal_nan=True), "later fills must see earlier ones"
    elif name.startswith("corners_edges"):
        for r, c in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)):
            assert hot[2 * n + r, 2 * n + c]
        outside = mask.copy()
        outside[inner] = False
        assert outside[: 2 * n].any() and outside[-2 * n :].any() and outside[:, : 2 * n].any() and outside[:, -2 * n :].any()
        raw = np.pad(image, 2 * n, mode=pad_mode)
        assert (want[outside] != raw[outside]).all(), "the mirror images in the pad are filled"
        if pad_mode == "wrap":
            assert label(mask, structure=np.ones((3, 3)))[1] > label(mask[inner], structure=np.ones((3, 3)))[1], "images far from their originals"
    elif name.startswith("pair_h"):
        gap = 1 if name.endswith("plus_1") else 0
        labels, count = label(mask)
        assert count == 2
        first, second = labels == labels[2 * n + 10, 2 * n + 10], labels != labels[2 * n + 10, 2 * n + 10]
        second &= mask
        assert chebyshev_gap(first, second) == hh + gap
        alone, alone_mask, _ = reference_fill(make(h, w, hh, first=False), n, pad_mode, dilation, width)
        assert np.array_equal(alone_mask, second)
        same = np.array_equal(alone[second], want[second], equal_nan=True)
        assert same == bool(gap), "exactly h apart: the second blob's fill depends on the first; h + 1 apart: it does not"
    elif name == "column70":
        cols = np.flatnonzero(hot[inner].any(0))
        assert len(cols) == 1 and hot[inner][:, cols[0]].sum() == 70 > 64 > TILE
    elif name == "row70":
        rows = np.flatnonzero(hot[inner].any(1))
        assert len(rows) == 1 and hot[inner][rows[0]].sum() == 70
        cols = 2 * n + np.flatnonzero(hot[inner][rows[0]])
        assert len({int(c) // TILE for c in cols}) >= 3 and len({int(c) // 64 for c in cols}) >= 2, "crosses tile seams and a 64-pixel segment"
    elif name == "nan_beside":
        r, c = np.argwhere(np.isnan(image))[0]
        assert not mask[2 * n + r, 2 * n + c]
        near = mask[2 * n + r - hh + 1 : 2 * n + r + hh + 1, 2 * n + c - hh + 1 : 2 * n + c + hh + 1]  # the pixels whose window holds (r, c)
        assert near.any()
    elif name == "wrap_top":
        assert mask[:hh].any() and np.isnan(want[:hh][mask[:hh]]).all(), "an empty window gives NaN"
    elif name == "nothing_hot":
        assert not hot.any() and not mask.any()
    elif name == "fully_hot":
        assert mask.all()
    elif name.startswith("mixed"):
        assert label(mask, structure=np.ones((3, 3)))[1] >= 10 and np.isnan(image).sum() == 1


# ---------------------------------------------------------------------------------------------------------------- emulator
@functools.cache
def emulator():
    """tests/emu/libemu_saturation.so: the drivers of kernels F1 - F5 on the CPU.  __graft_entry__.build() compiles it; it is compiled
    here when it is missing or older than its sources.  Without a compiler that is an error, not a skip."""
    import ctypes
    import os
    import shutil
    import subprocess

    root = pathlib.Path(__file__).resolve().parent.parent
    src, out = root / "tests" / "emu" / "emu_saturation.cpp", root / "tests" / "emu" / "libemu_saturation.so"
    cores = [root / "regularizepsf_amd" / "csrc" / n for n in ("rpsf_core_saturation.hpp", "rpsf_core_stars.hpp")]
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, *(c.stat().st_mtime for c in cores)):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++") or shutil.which("hipcc")
        assert clang is not None, "no clang++ to build tests/emu/emu_saturation.cpp"
        fresh = out.with_name(f"libemu_saturation.{os.getpid()}.so")  # written aside and moved into place: test processes may run side by side
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(fresh), str(src)], check=True)
        os.replace(fresh, out)
    lib = ctypes.CDLL(str(out))
    p, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emusat_fill.argtypes = [p, i, i, i, i, d, i, i, i, p, p, p]
    lib.emusat_restore.argtypes = [p, i, i, i, i, d, i, i, p, i, p, p, p]
    return lib


def emu_fill(image: np.ndarray, n: int, pad_mode: str, dilation: int, width: int, reverse: bool = False, threshold: float = THRESHOLD):
    """Kernels F1 - F4 on the emulator: (filled padded float32 frame, mask, groups)."""
    import ctypes

    image = np.ascontiguousarray(image, np.float32)
    shape = (image.shape[0] + 4 * n, image.shape[1] + 4 * n)
    padded, mask, groups = np.full(shape, -3.0, np.float32), np.full(shape, 7, np.uint8), ctypes.c_int(-1)
    assert emulator().emusat_fill(image.ctypes.data, *image.shape, n, _native.PAD_MODES[pad_mode], threshold, dilation, width, int(reverse),
                                  padded.ctypes.data, mask.ctypes.data, ctypes.byref(groups)) == 0
    return padded, mask.astype(bool), groups.value


def emu_restore(image: np.ndarray, n: int, pad_mode: str, dilation: int, width: int, corrected: np.ndarray, out_row0: int,
                threshold: float = THRESHOLD):
    """Kernel F5 behind F1 - F4 on the emulator: (H x W result, sorted list of the masked in-frame pixels)."""
    import ctypes

    image = np.ascontiguousarray(image, np.float32)
    corrected = np.ascontiguousarray(corrected, np.float32)
    out, listed, count = np.full(image.shape, -3.0, np.float32), np.full(image.size, -1, np.int32), ctypes.c_int(-1)
    assert emulator().emusat_restore(image.ctypes.data, *image.shape, n, _native.PAD_MODES[pad_mode], threshold, dilation, width,
                                     corrected.ctypes.data, out_row0, out.ctypes.data, listed.ctypes.data, ctypes.byref(count)) == 0
    return out, np.sort(listed[: count.value])


def assert_same_bits(got: np.ndarray, want: np.ndarray, what: str) -> None:
    """Bit-equal float32 frames; every NaN counts as the same NaN (its payload is not part of the definition)."""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    a, b = np.where(np.isnan(got), 0, got).view(np.uint32), np.where(np.isnan(want), 0, want).view(np.uint32)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
