"""Cases of the device-array views (DeviceArray, rpsf_view, the conversion kernels C1 / C2 of csrc/convert.hip), shared between the
emulator tests (tests/test_device_array_host.py) and the GPU tests (tests/test_gpu_device_array.py).

A view is described over one flat buffer of its dtype: element (r, c) is flat element ``off + r * pitch + c * step``.  The buffer is
filled with a sentinel (NaN for float inputs) and has at least 64 elements before the view, behind it and - for every view that is not
dense - between two rows, so that an indexing mistake shows as a changed sentinel or a NaN in the result, inside the allocation.
The reference of every conversion is NumPy's ``astype``; NaN is compared by position (its payload is no part of the definition).
"""

from __future__ import annotations

import ctypes
import functools
import pathlib

import numpy as np

from regularizepsf_amd import _native

MARGIN = 64
#: tail, vector and wave boundaries of the chunking (rpsf_core_convert.hpp: 4, 8 or 16 elements per thread, 64 threads per wave)
SHAPES = ((1, 1), (1, 3), (3, 5), (2, 63), (2, 64), (3, 65), (5, 67), (1, 257), (70, 131))
IN_DTYPES = (np.float32, np.float64, np.float16, np.uint8, np.int16, np.uint16, np.int32)
OUT_DTYPES = (np.float32, np.float64, np.float16)
#: name -> (extra base offset in elements, extra row pitch in elements, column step)
VIEWS = {"dense": (0, None, 1), "off1": (1, None, 1), "off2": (2, None, 1), "off3": (3, None, 1), "pitch1": (0, 1, 1), "pitch5": (0, 5, 1),
         "col2": (0, 0, 2), "col3": (0, 0, 3), "off1pitch3": (1, 3, 1)}


def layout(shape, view):
    """(flat length, off, pitch, step) in elements."""
    rows, cols = shape
    extra_off, extra_pitch, step = VIEWS[view]
    pitch = cols if extra_pitch is None else cols * step + MARGIN + extra_pitch
    off = MARGIN + extra_off
    return off + (rows - 1) * pitch + (cols - 1) * step + 1 + MARGIN, off, pitch, step


def aligned_flat(length, dtype, fill):
    """A 1-D array of ``length`` elements that starts on a 16-byte boundary (what hipMalloc gives the device side)."""
    dtype = np.dtype(dtype)
    raw = np.empty(length * dtype.itemsize + 16, np.uint8)
    start = (-raw.ctypes.data) % 16
    flat = raw[start : start + length * dtype.itemsize].view(dtype)
    flat[...] = fill
    return flat


def sentinel(dtype):
    dtype = np.dtype(dtype)
    return np.nan if dtype.kind == "f" else (201 if dtype.itemsize == 1 else 12345)


def host_view(flat, shape, view):
    """The strided NumPy view of ``flat`` for (shape, view), and the flat indices of its elements."""
    _, off, pitch, step = layout(shape, view)
    isz = flat.dtype.itemsize
    v = np.lib.stride_tricks.as_strided(flat[off:], shape, (pitch * isz, step * isz))
    index = (off + np.arange(shape[0])[:, None] * pitch + np.arange(shape[1])[None, :] * step).reshape(-1)
    return v, index


def device_view(big, shape, view):
    """The same view of a 1-D DeviceArray holding the flat buffer."""
    from regularizepsf_amd.device_array import DeviceArray

    _, off, pitch, step = layout(shape, view)
    isz = big.dtype.itemsize
    return DeviceArray._from_parts(big.ptr + off * isz, shape, big.dtype, (pitch * isz, step * isz), big, big.device, big._pending)


# ---------------------------------------------------------------------------------------------------------------- values
def special_values(dtype) -> np.ndarray:
    dtype = np.dtype(dtype)
    if dtype == np.int32:
        return np.array([2**24 + 1, 2**31 - 1, -(2**31), -(2**24) - 1, 2**24 + 3, 0, -1, 2**31 - 65], dtype)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return np.array([info.min, info.max, 0, 1, info.max - 1], dtype)
    if dtype == np.float64:
        tiny = 2.0**-149  # the smallest float32 denormal
        return np.array([1e-40, -1e-40, tiny * 1.5, tiny * 2.5, tiny * 0.5, tiny * 0.5000001, 1e39, -1e39, 3.4028235677973366e38, 3.4028235677973362e38,
                         1 + 2.0**-24, 1 + 3 * 2.0**-24, 1 + 2.0**-24 + 2.0**-50, np.nan, np.inf, -np.inf, -0.0, 1e-320, 1.7976931348623157e308], dtype)
    if dtype == np.float32:
        return np.array([1e-40, -1e-45, np.nan, np.inf, -np.inf, -0.0, 3.4028235e38, 1.17549435e-38], dtype)
    return np.array([6e-8, -6e-8, 6.1e-5, 65504, -65504, np.nan, np.inf, -np.inf, -0.0, 1.0009766], dtype)  # float16


def input_values(dtype, shape, seed=0) -> np.ndarray:
    """Random values of ``dtype`` over its range with the special values first (as many as fit)."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(1000 + seed + 7 * shape[0] + shape[1])
    count = shape[0] * shape[1]
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        flat = rng.integers(info.min, info.max, count, dtype=np.int64, endpoint=True).astype(dtype)
    else:
        with np.errstate(over="ignore"):
            flat = (rng.standard_normal(count) * 10.0 ** rng.uniform(-6, 4, count)).astype(dtype)
    special = special_values(dtype)[:count]
    flat[: len(special)] = special
    return flat.reshape(shape)


def dense_values(shape, out_dtype, seed=0) -> np.ndarray:
    """float32 values for C2: random over the output type's range, with halfway cases, overflow and the denormal range of float16 first."""
    rng = np.random.default_rng(2000 + seed + 7 * shape[0] + shape[1])
    count = shape[0] * shape[1]
    flat = (rng.standard_normal(count) * 10.0 ** rng.uniform(-9, 5, count)).astype(np.float32)
    u = 2.0**-24  # float16's smallest denormal
    special = np.array([1 + 2.0**-11, 1 + 3 * 2.0**-11, 1 + 2.0**-11 + 2.0**-20, 65504, 65519.996, 65520, 1e5, -1e5, u, u / 2, u / 2 * 1.0000002, 3 * u / 2, 5 * u / 2,
                        1023.5 * u, 2.0**-14 - u / 2, 2.0**-14, 6e-8, 1e-7, -3e-8, -0.0, np.nan, np.inf, -np.inf, 1e-40, -1e-45, 3.4028235e38, 2049, 2051],
                       np.float32)[:count]
    flat[: len(special)] = special
    return flat.reshape(shape)


def same_bits(got: np.ndarray, want: np.ndarray, what: str = "") -> None:
    """Bit-equal arrays of one dtype and shape; every NaN counts as the same NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
        got, want = np.where(np.isnan(got), 0, got), np.where(np.isnan(want), 0, want)
    word = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    a, b = np.ascontiguousarray(got).view(word), np.ascontiguousarray(want).view(word)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


def to_float32(view: np.ndarray) -> np.ndarray:
    """What C1 must produce."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(view).astype(np.float32)


def from_float32(dense: np.ndarray, dtype) -> np.ndarray:
    """What C2 must produce."""
    with np.errstate(over="ignore", invalid="ignore"):
        return dense.astype(dtype)


def untouched(flat: np.ndarray, index: np.ndarray, fill) -> bool:
    """Every element of ``flat`` outside ``index`` still holds ``fill``."""
    rest = np.ones(flat.size, bool)
    rest[index] = False
    return bool(np.all(np.isnan(flat[rest]))) if isinstance(fill, float) and np.isnan(fill) else bool(np.all(flat[rest] == fill))


# ---------------------------------------------------------------------------------------------------------------- rpsf_view
def view_of(array: np.ndarray, data: int | None = None) -> _native.View:
    """rpsf_view of a 2-D NumPy array (``data``: a pointer to put in place of the array's own)."""
    return _native.View(array.ctypes.data if data is None else data, _native.DTYPES[array.dtype.str], array.shape[0], array.shape[1],
                        array.strides[0], array.strides[1])


# ---------------------------------------------------------------------------------------------------------------- emulator
@functools.cache
def emulator():
    """tests/emu/libemu_convert.so: the thread bodies of C1 and C2 on the CPU.  __graft_entry__.build() compiles it; it is compiled here
    when it is missing or older than its sources.  Without a compiler that is an error, not a skip."""
    import os
    import shutil
    import subprocess

    root = pathlib.Path(__file__).resolve().parent.parent
    src, out = root / "tests" / "emu" / "emu_convert.cpp", root / "tests" / "emu" / "libemu_convert.so"
    core = root / "regularizepsf_amd" / "csrc" / "rpsf_core_convert.hpp"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, core.stat().st_mtime):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++") or shutil.which("hipcc")
        assert clang is not None, "no clang++ to build tests/emu/emu_convert.cpp"
        fresh = out.with_name(f"libemu_convert.{os.getpid()}.so")  # written aside and moved into place: test processes may run side by side
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(fresh), str(src)], check=True)
        os.replace(fresh, out)
    lib = ctypes.CDLL(str(out))
    lib.emu_convert.argtypes = [ctypes.POINTER(_native.View), ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return lib


def emu_gather(view: np.ndarray, workgroups: int = 0):
    """C1 on the emulator: (dense float32 frame, bit 0: the strided side moved by 16-byte accesses | bit 1: the dense side did)."""
    dense = aligned_flat(view.size + 1, np.float32, -3.0)
    vec = ctypes.c_int(0)
    assert emulator().emu_convert(ctypes.byref(view_of(view)), dense.ctypes.data, 1, workgroups, ctypes.byref(vec)) == 0
    assert dense[-1] == -3.0
    return dense[:-1].reshape(view.shape), vec.value


def emu_scatter(dense: np.ndarray, view: np.ndarray, workgroups: int = 0) -> int:
    """C2 on the emulator, into ``view``; returns the access bits as emu_gather."""
    assert dense.dtype == np.float32 and dense.flags.c_contiguous and dense.ctypes.data % 16 == 0
    vec = ctypes.c_int(0)
    assert emulator().emu_convert(ctypes.byref(view_of(view)), dense.ctypes.data, 0, workgroups, ctypes.byref(vec)) == 0
    return vec.value


# ---------------------------------------------------------------------------------------------------------------- apply cases (GPU)
#: patch size -> frame shape: one plan of every compiled size
APPLY_SHAPES = {16: (40, 56), 32: (72, 88), 64: (136, 152), 128: (256, 384), 256: (512, 512)}
CONVERTED_SIZES = (32, 128)


@functools.cache
def apply_case(n: int):
    """(corner list, random complex64 K - nothing like an identity -, float32 frame) of the plan size's shape."""
    from tests.helpers import random_transfer

    shape = APPLY_SHAPES[n]
    coords, k = random_transfer(shape, n, 4100 + n)
    frame = (np.random.default_rng(4200 + n).standard_normal(shape) * 10 + 30).astype(np.float32)
    return coords, k, frame


def frame_as(frame: np.ndarray, dtype) -> np.ndarray:
    """The apply frame in another input dtype, with values that dtype holds (integers: scaled into its range)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return (frame.astype(np.float64) * (1 + 2.0**-30)).astype(dtype) if dtype == np.float64 else frame.astype(dtype)
    info = np.iinfo(dtype)
    scale = 500.0 if dtype == np.uint16 else 2e7  # (30 +- 10 lands in the middle of the type's range)
    return np.clip(np.rint(frame.astype(np.float64) * scale), info.min, info.max).astype(dtype)
