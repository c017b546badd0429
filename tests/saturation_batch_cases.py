"""Stacks of frames for the tests of the batched device saturation route (csrc/rpsf_core_saturation_batch.hpp), their reference and
preconditions, shared between the emulator tests (tests/test_saturation_batch_host.py) and the GPU tests
(tests/test_gpu_saturation_batch.py).

Every expected value is ``saturation_cases.reference_fill`` of the single frame: a batch may change nothing of any frame.  The frames
come from the makers of ``saturation_cases.CASES``.  What a stack is there for is asserted by ``precondition`` from NumPy / SciPy alone,
before anything under test runs.  A *runner* is ``run(frames, n, pad_mode, dilation, width, order=0, group=0)`` ->
``(filled padded frames, masks, groups per frame, info)``: the emulator's here, the GPU's in the GPU tests - the checks are the same.
"""

from __future__ import annotations

import functools
import pathlib

import numpy as np

from regularizepsf_amd import _native
from tests import saturation_cases as sc

ORDER_LONGEST_FIRST, ORDER_REVERSED, ORDER_FRAMES = 0, 1, 2
KINDS = ("isolated", "blob", "corners_edges", "nothing_hot", "pair_h", "nan_beside", "wrap_top")  # the issue's order


def _maker(name):
    return sc.CASES[name][0]


def _seam_pair(h, w, n, pad_mode):
    """Two frames: in the first the LAST pixel of the padded frame is hot, in the second the FIRST - neighbours in memory when the
    frames lie one behind the other."""
    index = np.pad(np.arange(h * w).reshape(h, w), 2 * n, mode=pad_mode)
    first, second = sc.background(h, w, 31), sc.background(h, w, 32)
    first.flat[index[-1, -1]] = sc.HOT
    second.flat[index[0, 0]] = sc.HOT
    return [first, second]


def _kinds(h, w, n, pad_mode, hh):
    # (the seam pair goes last: none of the seven kinds has the padded frame's first or last pixel on its mask in every pad mode)
    return [_maker(k)(h, w, hh) for k in KINDS] + _seam_pair(h, w, n, pad_mode)


def _blobs(h, w, n, pad_mode, hh):
    blob = _maker("blob")(h, w, hh)
    return [blob, np.roll(blob, (3, 5), axis=(0, 1)), np.roll(blob, (-7, 11), axis=(0, 1))]


def _same_layout(h, w, n, pad_mode, hh):
    hot = _maker("corners_edges")(h, w, hh) > sc.THRESHOLD
    hot[h // 2 : h // 2 + 3, w // 2 : w // 2 + 4] = True
    first, third = sc.background(h, w, 21), (3.0 * sc.background(h, w, 22)).astype(np.float32)
    first[hot] = sc.HOT
    third[hot] = sc.HOT
    return [first, sc.background(h, w, 23), third]


def _around_fully_hot(h, w, n, pad_mode, hh):
    return [_maker("isolated")(h, w, hh), _maker("fully_hot")(h, w, hh), _maker("blob")(h, w, hh)]


def _nothing(h, w, n, pad_mode, hh):
    return [sc.background(h, w, seed) for seed in (41, 42, 43)]


def _kinds_and_column(h, w, n, pad_mode, hh):
    return _kinds(h, w, n, pad_mode, hh) + [_maker("column70")(h, w, hh)]


# name -> (frames maker, N, (H, W), pad mode, (dilation, width))
STACKS = {
    "kinds_wrap": (_kinds, 16, (40, 48), "wrap", (1, 7)),
    "kinds_edge": (_kinds, 16, (40, 48), "edge", (2, 5)),
    "odd_stride": (_blobs, 16, (41, 47), "symmetric", (1, 7)),
    "same_layout": (_same_layout, 16, (40, 48), "symmetric", (1, 7)),
    "around_fully_hot": (_around_fully_hot, 16, (24, 24), "symmetric", (1, 9)),
    "nothing_hot": (_nothing, 16, (40, 48), "symmetric", (1, 7)),
    "the_cut": (lambda h, w, n, m, hh: _kinds(h, w, n, m, hh)[:5], 16, (40, 48), "wrap", (1, 7)),
    "order": (_kinds_and_column, 32, (96, 128), "symmetric", (1, 9)),
}


@functools.cache
def stack(name: str):
    """The frames of a stack, made once and shared; callers must not write to them."""
    make, n, (h, w), pad_mode, (_, width) = STACKS[name]
    frames = make(h, w, n, pad_mode, width // 2)
    for f in frames:
        assert f.dtype == np.float32 and f.shape == (h, w)
        f.flags.writeable = False
    return frames


@functools.cache
def reference(name: str):
    """Per frame (filled padded float32 frame, mask, hot) of ``saturation_cases.reference_fill``; computed once, read-only."""
    _, n, _, pad_mode, (dilation, width) = STACKS[name]
    out = []
    for f in stack(name):
        one = sc.reference_fill(f, n, pad_mode, dilation, width)
        for a in one:
            a.flags.writeable = False
        out.append(one)
    return out


def precondition(name: str) -> None:
    make, n, (h, w), pad_mode, (dilation, width) = STACKS[name]
    frames, ref = stack(name), reference(name)
    ph, pw = h + 4 * n, w + 4 * n
    if name.startswith("kinds") or name == "order":
        assert len(frames) >= len(KINDS) + 2
        for kind, (_, mask, _) in zip(KINDS, ref):
            assert mask.any() == (kind != "nothing_hot"), kind
        seams = [f for f in range(len(frames) - 1) if ref[f][1][ph - 1, pw - 1] and ref[f + 1][1][0, 0]]
        assert seams, "a consecutive pair with the last padded pixel of frame f and the first of frame f + 1 on the mask"
        f = seams[0]
        assert not ref[f][1][0, 0] and not ref[f + 1][1][ph - 1, pw - 1], "a union across the seam would change a mask or a group"
    if name == "order":
        from scipy.ndimage import label

        column = ref[-1][2]
        cols = np.flatnonzero(column[2 * n : 2 * n + h, 2 * n : 2 * n + w].any(0))
        assert len(cols) == 1 and column[2 * n : 2 * n + h, 2 * n + cols[0]].sum() == 70

        def longest(mask):  # masked pixels of the largest 8-connected piece (a group holds at least that many)
            lab, cnt = label(mask, structure=np.ones((3, 3)))
            return max((int((lab == k).sum()) for k in range(1, cnt + 1)), default=0)

        others = max(longest(m) for _, m, _ in ref[:-1])
        assert longest(ref[-1][1]) > 2 * others >= 2, "the longest group is the LAST frame's: in frame order it would start last"
    if name == "odd_stride":
        assert (ph * pw) % 4 != 0 and (ph * pw) % 2 == 1 and len(frames) == 3
        assert all(m.any() for _, m, _ in ref)
    if name == "same_layout":
        assert np.array_equal(ref[0][1], ref[2][1]) and ref[0][1].any() and not ref[1][1].any()
        m = ref[0][1]
        assert not np.array_equal(ref[0][0][m], ref[2][0][m], equal_nan=True), "the same pixels get different fills"
    if name == "around_fully_hot":
        assert ref[1][1].all() and 0 < ref[0][1].sum() < ref[0][1].size and 0 < ref[2][1].sum() < ref[2][1].size
    if name == "nothing_hot":
        assert not any(m.any() or hot.any() for _, m, hot in ref)
    if name == "the_cut":
        assert len(frames) == 5 and sum(bool(m.any()) for _, m, _ in ref) >= 3


# ---------------------------------------------------------------------------------------------------------------- emulator
@functools.cache
def emulator():
    """tests/emu/libemu_saturation_batch.so: the batch drivers of kernels F1 - F5 on the CPU.  __graft_entry__.build() compiles it; it is
    compiled here when it is missing or older than its sources.  Without a compiler that is an error, not a skip."""
    import ctypes
    import os
    import shutil
    import subprocess

    root = pathlib.Path(__file__).resolve().parent.parent
    src, out = root / "tests" / "emu" / "emu_saturation_batch.cpp", root / "tests" / "emu" / "libemu_saturation_batch.so"
    cores = [root / "regularizepsf_amd" / "csrc" / n for n in ("rpsf_core_saturation_batch.hpp", "rpsf_core_saturation.hpp", "rpsf_core_stars.hpp")]
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, *(c.stat().st_mtime for c in cores)):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++") or shutil.which("hipcc")
        assert clang is not None, "no clang++ to build tests/emu/emu_saturation_batch.cpp"
        fresh = out.with_name(f"libemu_saturation_batch.{os.getpid()}.so")  # written aside and moved into place
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(fresh), str(src)], check=True)
        os.replace(fresh, out)
    lib = ctypes.CDLL(str(out))
    p, i, d, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
    lib.emusatb_fill.argtypes = [p, i, z, i, i, i, i, d, i, i, i, i, p, p, p, p]
    lib.emusatb_restore.argtypes = [p, i, z, i, i, i, i, d, i, i, p, z, i, p, z, p, p]
    return lib


def _strided(frames, filler: int):
    """The frames laid `H * W + filler` floats apart, as a resident caller may hold them."""
    h, w = frames[0].shape
    stride = h * w + filler
    flat = np.full(len(frames) * stride, -11.0, np.float32)
    for f, im in enumerate(frames):
        flat[f * stride : f * stride + h * w] = np.ascontiguousarray(im, np.float32).ravel()
    return flat, stride


def emu_fill_batch(frames, n: int, pad_mode: str, dilation: int, width: int, order: int = 0, group: int = 0, threshold: float = sc.THRESHOLD):
    """Kernels F1 - F4 of a stack on the emulator (frames H * W + 3 floats apart): (filled padded frames, masks, groups per frame, info)."""
    h, w = frames[0].shape
    flat, stride = _strided(frames, 3)
    shape = (len(frames), h + 4 * n, w + 4 * n)
    padded, masks = np.full(shape, -3.0, np.float32), np.full(shape, 7, np.uint8)
    groups, info = np.full(len(frames), -1, np.int32), np.full(4, -1, np.int32)
    rc = emulator().emusatb_fill(flat.ctypes.data, len(frames), stride, h, w, n, _native.PAD_MODES[pad_mode], threshold, dilation, width, order,
                                 group, padded.ctypes.data, masks.ctypes.data, groups.ctypes.data, info.ctypes.data)
    if rc == -1:
        msg = "bad argument"
        raise ValueError(msg)
    assert rc == 0, f"emusatb_fill: {rc}"
    return padded, masks.astype(bool), groups, tuple(int(v) for v in info)


def emu_restore_batch(frames, n: int, pad_mode: str, dilation: int, width: int, corrected: np.ndarray, out_row0: int,
                      threshold: float = sc.THRESHOLD):
    """Kernel F5 behind F1 - F4 of one frame-group on the emulator: (results H x W per frame, per frame the sorted list of masked pixels)."""
    h, w = frames[0].shape
    flat, stride = _strided(frames, 3)
    corrected = np.ascontiguousarray(corrected, np.float32)
    out_stride = h * w + 5
    outs = np.full(len(frames) * out_stride, -3.0, np.float32)
    lists, counts = np.full((len(frames), h * w), -1, np.int32), np.full(len(frames), -1, np.int32)
    rc = emulator().emusatb_restore(flat.ctypes.data, len(frames), stride, h, w, n, _native.PAD_MODES[pad_mode], threshold, dilation, width,
                                    corrected.ctypes.data, corrected[0].size, out_row0, outs.ctypes.data, out_stride, lists.ctypes.data,
                                    counts.ctypes.data)
    assert rc == 0, f"emusatb_restore: {rc}"
    rows = outs.reshape(len(frames), out_stride)
    assert (rows[:, h * w :] == -3.0).all(), "the floats between two results are untouched"
    return rows[:, : h * w].reshape(len(frames), h, w).copy(), [np.sort(lists[f, : counts[f]]) for f in range(len(frames))]


# ---------------------------------------------------------------------------------------------------------------- the checks
def run_stack(run, name: str, order: int = 0, group: int = 0):
    _, n, _, pad_mode, (dilation, width) = STACKS[name]
    return run(stack(name), n, pad_mode, dilation, width, order=order, group=group)


def check_against_reference(got, name: str, single_groups=None) -> None:
    """Every frame of the batch has the bits and the mask of its own single-frame reference (and the single entry's group count)."""
    padded, masks, groups, info = got
    ref = reference(name)
    assert len(padded) == len(masks) == len(groups) == len(ref)
    for f, (want, mask, _) in enumerate(ref):
        assert np.array_equal(masks[f], mask), f"{name}, frame {f}: mask"
        sc.assert_same_bits(np.ascontiguousarray(padded[f]), want, f"{name}, frame {f}")
        assert (groups[f] == 0) == (not mask.any()), f"{name}, frame {f}: groups"
        if single_groups is not None:
            assert groups[f] == single_groups(f), f"{name}, frame {f}: groups of the single-frame entry"
    assert info[0] == len(ref) and info[2] == int(np.sum(groups)) and info[3] == sum(int(m.sum()) for _, m, _ in ref)


def check_same_results(a, b, what: str) -> None:
    for f in range(len(a[0])):
        assert np.array_equal(a[1][f], b[1][f]), f"{what}, frame {f}: mask"
        sc.assert_same_bits(np.ascontiguousarray(a[0][f]), np.ascontiguousarray(b[0][f]), f"{what}, frame {f}")
    assert np.array_equal(a[2], b[2]), f"{what}: groups"


def emu_single_groups(name: str):
    _, n, _, pad_mode, (dilation, width) = STACKS[name]
    return lambda f: sc.emu_fill(stack(name)[f], n, pad_mode, dilation, width)[2]
