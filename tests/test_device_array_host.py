"""Device arrays without a GPU: the conversion kernels C1 / C2 on the CPU emulator (tests/emu/emu_convert.cpp runs the thread bodies of
csrc/rpsf_core_convert.hpp, the code the GPU runs), the zero-copy predicate through ``rpsf_view_route``, the view arithmetic of
``DeviceArray`` and the Python surface.  tests/test_gpu_device_array.py holds the GPU to the same conversion cases.
"""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, device_array
from regularizepsf_amd.device_array import DeviceArray
from tests import device_array_cases as dc


# ---------------------------------------------------------------------------------------------------------------- C1 on the emulator
@pytest.mark.parametrize("view", sorted(dc.VIEWS))
@pytest.mark.parametrize("dtype", dc.IN_DTYPES, ids=lambda d: np.dtype(d).name)
def test_c1_has_the_bits_of_astype_float32(dtype, view):
    for shape in dc.SHAPES:
        values = dc.input_values(dtype, shape)
        flat = dc.aligned_flat(dc.layout(shape, view)[0], dtype, dc.sentinel(dtype))
        v, index = dc.host_view(flat, shape, view)
        v[...] = values
        before = flat.copy()
        got, _ = dc.emu_gather(v)
        dc.same_bits(got, dc.to_float32(values), f"{np.dtype(dtype).name} {shape} {view}")
        dc.same_bits(flat, before, "the input")  # (read only)


def test_c1_special_values_are_all_exercised_and_a_small_grid_strides():
    for dtype in dc.IN_DTYPES:
        special = dc.special_values(dtype)
        assert len(special) <= 70 * 131 and np.array_equal(dc.input_values(dtype, (70, 131)).reshape(-1)[: len(special)], special, equal_nan=True)
        values = dc.input_values(dtype, (70, 131), seed=5)
        got, _ = dc.emu_gather(values, workgroups=1)  # 256 threads for 2293 chunks (573 of uint8): every thread takes several
        dc.same_bits(got, dc.to_float32(values), np.dtype(dtype).name)
    # what the float64 specials are there for: float32 denormals, both infinities, ties to even
    f = dc.to_float32(dc.special_values(np.float64))
    assert (np.abs(f[np.isfinite(f) & (f != 0)]) < 1.1754944e-38).sum() >= 4 and np.isposinf(f).sum() >= 3 and np.isneginf(f).sum() >= 2
    assert f[10] == 1.0 and f[11] == np.float32(1 + 2.0**-22) and f[12] == np.float32(1 + 2.0**-23) and f[4] == 0 and f[5] > 0
    i = dc.to_float32(dc.special_values(np.int32))
    assert i[0] == 2.0**24 and i[1] == 2.0**31 and i[4] == 2.0**24 + 4


def test_both_access_forms_run():
    """16-byte accesses where the view allows them, element accesses elsewhere (make_args, rpsf_core_convert.hpp)."""
    for dtype, elems in ((np.float32, 4), (np.float64, 4), (np.int32, 4), (np.float16, 8), (np.int16, 8), (np.uint16, 8), (np.uint8, 16)):
        for shape, view, want in (((2, 64), "dense", 3), ((2, 64), "pitch1", 2), ((2, 64), "col2", 2), ((3, 65), "dense", 2), ((2, 64), "off1", 2),
                                  ((2, 64), "pitch5", 2)):
            flat = dc.aligned_flat(dc.layout(shape, view)[0], dtype, 0)
            v, _ = dc.host_view(flat, shape, view)
            assert dc.emu_gather(v)[1] == want, (dtype, shape, view)
        # a pitched view whose base and pitch are multiples of 16 bytes and whose width is a multiple of the chunk
        big = dc.aligned_flat(4 * 96, dtype, 0).reshape(4, 96)
        assert dc.emu_gather(big[1:3, 16:16 + 4 * elems])[1] == 3
        assert dc.emu_gather(big[1:3, 16:16 + 4 * elems + 1])[1] == 2


def test_views_that_are_not_aligned_to_their_item_size_are_served():
    """What the zero-copy predicate turns away for its pointer or row stride (aligned to 2, a stride of 4 cols + 2) is a view all the same."""
    for dtype in (np.float32, np.float64, np.int32, np.uint16):
        isz = np.dtype(dtype).itemsize
        shape = (5, 67)
        values = dc.input_values(dtype, shape, seed=3)
        raw = dc.aligned_flat(isz // 2 + shape[0] * (shape[1] * isz + isz // 2) + 64, np.uint8, 0xEE)
        v = np.lib.stride_tricks.as_strided(raw[isz // 2:].view(np.uint8), shape + (isz,), (shape[1] * isz + isz // 2, isz, 1))
        v[...] = np.ascontiguousarray(values).view(np.uint8).reshape(shape + (isz,))
        view = _native.View(raw.ctypes.data + isz // 2, _native.DTYPES[np.dtype(dtype).str], shape[0], shape[1], shape[1] * isz + isz // 2, isz)
        dense = dc.aligned_flat(values.size, np.float32, -3.0)
        vec = ctypes.c_int(-1)
        assert dc.emulator().emu_convert(ctypes.byref(view), dense.ctypes.data, 1, 0, ctypes.byref(vec)) == 0 and vec.value == 2
        dc.same_bits(dense.reshape(shape), dc.to_float32(values), np.dtype(dtype).name)
        if dtype in dc.OUT_DTYPES:  # and back out through C2, into the same misaligned view
            v[...] = 0
            assert dc.emulator().emu_convert(ctypes.byref(view), dense.ctypes.data, 0, 0, None) == 0
            got = np.ascontiguousarray(v).reshape(shape[0], -1).view(dtype)
            dc.same_bits(got, dc.from_float32(dc.to_float32(values), dtype), np.dtype(dtype).name)
            v[...] = 0xEE
            assert np.all(raw == 0xEE)  # not a byte beside the elements


# ---------------------------------------------------------------------------------------------------------------- C2 on the emulator
@pytest.mark.parametrize("view", sorted(dc.VIEWS))
@pytest.mark.parametrize("dtype", dc.OUT_DTYPES, ids=lambda d: np.dtype(d).name)
def test_c2_has_the_bits_of_astype_and_writes_nothing_else(dtype, view):
    for shape in dc.SHAPES:
        values = dc.dense_values(shape, dtype)
        dense = dc.aligned_flat(values.size, np.float32, 0).reshape(shape)
        dense[...] = values
        fill = dc.sentinel(dtype)
        flat = dc.aligned_flat(dc.layout(shape, view)[0], dtype, fill)
        v, index = dc.host_view(flat, shape, view)
        dc.emu_scatter(dense, v)
        dc.same_bits(np.ascontiguousarray(v), dc.from_float32(values, dtype), f"{np.dtype(dtype).name} {shape} {view}")
        assert dc.untouched(flat, index, fill)  # rows x cols elements were written and nothing before, behind or between them


def test_c2_float16_cases_are_what_they_are_there_for():
    values = dc.dense_values((70, 131), np.float16)
    dense = dc.aligned_flat(values.size, np.float32, 0).reshape(values.shape)
    dense[...] = values
    out = np.zeros(values.shape, np.float16)
    dc.emu_scatter(dense, out, workgroups=1)
    want = dc.from_float32(values, np.float16)
    dc.same_bits(out, want, "float16")
    h = want.reshape(-1)
    assert h[0] == 1.0 and h[1] == np.float16(1 + 2.0**-9) and h[2] == np.float16(1 + 2.0**-10)  # ties to even, just above a tie
    assert h[3] == 65504 and h[4] == 65504 and np.isposinf(h[5]) and np.isposinf(h[6]) and np.isneginf(h[7])  # overflow
    u = np.float16(2.0**-24)
    assert h[8] == u and h[9] == 0 and h[10] == u and h[11] == 2 * u and h[12] == 2 * u and h[13] == 1024 * u and h[14] == np.float16(2.0**-14)  # denormals
    assert h[23] == 0 and np.signbit(h[24]) and h[24] == 0 and np.isposinf(h[25]) and h[26] == 2048 and h[27] == 2052
    denormal = (np.abs(want) > 0) & (np.abs(want) < 2.0**-14)
    assert denormal.sum() > 100  # the random part reaches the denormal range too


# ---------------------------------------------------------------------------------------------------------------- the zero-copy predicate
def _view(data=4096, dtype=0, rows=8, cols=10, row_stride=40, col_stride=4):
    return _native.View(data, dtype, rows, cols, row_stride, col_stride)


ROUTE_TABLE = [  # (what, view, zero copy?) - one case on each side of every clause
    ("dense float32", {}, True),
    ("float64", {"dtype": 1, "row_stride": 80, "col_stride": 8}, False),
    ("float16", {"dtype": 2, "row_stride": 20, "col_stride": 2}, False),
    ("col_stride 8", {"col_stride": 8, "row_stride": 80}, False),
    ("row_stride == 4 cols", {"row_stride": 40}, True),
    ("row_stride larger", {"row_stride": 44}, True),
    ("row_stride much larger", {"row_stride": 4 * 1000}, True),
    ("row_stride not a multiple of 4", {"row_stride": 42}, False),
    ("row_stride smaller than a row", {"row_stride": 36}, False),
    ("pointer aligned to 4, not to 16", {"data": 4096 + 4}, True),
    ("pointer aligned to 2", {"data": 4096 + 2}, False),
    ("ld == INT_MAX", {"row_stride": 4 * (2**31 - 1)}, True),
    ("ld overflows an int", {"row_stride": 4 * 2**31}, False),
]


@pytest.mark.parametrize("what,fields,zero_copy", ROUTE_TABLE, ids=[r[0] for r in ROUTE_TABLE])
def test_view_route_truth_table(what, fields, zero_copy):
    v, dense = _view(**fields), _view()
    assert _native.view_route(v, dense) == (0 if zero_copy else _native.ROUTE_C1)
    assert _native.view_route(dense, v) == (0 if zero_copy else _native.ROUTE_C2)
    assert _native.view_route(v, v) == (0 if zero_copy else _native.ROUTE_C1 | _native.ROUTE_C2)


def test_view_route_refuses_bad_views_and_writes_nothing():
    lib = _native.lib()
    good = _view()
    bad = {
        "null data": _view(data=None),
        "zero row stride": _view(row_stride=0),
        "negative column stride": _view(col_stride=-4),
        "negative rows": _view(rows=-1),
        "negative cols": _view(cols=-1),
        "unknown dtype": _view(dtype=7),
        "negative dtype": _view(dtype=-1),
    }
    for what, v in bad.items():
        for image, out in ((v, good), (good, v)):
            route = ctypes.c_int(77)
            assert lib.rpsf_view_route(ctypes.byref(image), ctypes.byref(out), ctypes.byref(route)) == _native.E_BADARG, what
            assert route.value == 77 and lib.rpsf_last_error()
    for dtype, item in ((3, 1), (4, 2), (5, 2), (6, 4)):  # integers are inputs only
        v = _view(dtype=dtype, row_stride=10 * item, col_stride=item)
        route = ctypes.c_int(77)
        assert lib.rpsf_view_route(ctypes.byref(v), ctypes.byref(good), ctypes.byref(route)) == 0 and route.value == _native.ROUTE_C1
        assert lib.rpsf_view_route(ctypes.byref(good), ctypes.byref(v), ctypes.byref(route)) == _native.E_BADARG
    assert lib.rpsf_view_route(None, ctypes.byref(good), ctypes.byref(ctypes.c_int())) == _native.E_BADARG
    assert lib.rpsf_view_route(ctypes.byref(good), ctypes.byref(good), None) == _native.E_BADARG
    # empty views: nothing to do, no pointer needed
    empty = _view(data=None, rows=0)
    assert _native.view_route(empty, empty) == 0
    assert lib.rpsf_convert_view(0, ctypes.byref(empty), ctypes.byref(empty), None) == 0
    # the calls that would touch memory refuse the same views before they touch a device
    for what, v in bad.items():
        assert lib.rpsf_convert_view(0, ctypes.byref(v), ctypes.byref(good), None) == _native.E_BADARG, what
        assert lib.rpsf_apply_view(None, ctypes.byref(v), ctypes.byref(good), 1, 0.0, float("inf"), 1, 7, None, None) == _native.E_BADARG
    two_shapes = _view(rows=7)
    assert lib.rpsf_convert_view(0, ctypes.byref(two_shapes), ctypes.byref(good), None) == _native.E_BADARG
    neither_dense = _view(row_stride=44)
    assert lib.rpsf_convert_view(0, ctypes.byref(neither_dense), ctypes.byref(neither_dense), None) == _native.E_BADARG


def test_header_and_ctypes_declare_the_view_entry_points():
    import pathlib
    import re

    header = (pathlib.Path(__file__).resolve().parent.parent / "include" / "rpsf.h").read_text()
    for name in ("rpsf_view_route", "rpsf_convert_view", "rpsf_apply_view", "rpsf_apply_batch_view", "rpsf_stream_synchronize"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _native._PROTOTYPES and hasattr(_native.lib(), name)
    assert ctypes.sizeof(_native.View) == 40
    for code, name in enumerate(("FLOAT32", "FLOAT64", "FLOAT16", "UINT8", "INT16", "UINT16", "INT32")):
        assert re.search(rf"#define RPSF_DTYPE_{name} {code}\b", header)
    assert sorted(_native.DTYPES.values()) == list(range(7))
    from regularizepsf_amd import build as hip_build

    assert hip_build.CSRC / "convert.hip" in hip_build.SOURCES and hip_build.CSRC / "rpsf_core_convert.hpp" in hip_build.HEADERS


# ---------------------------------------------------------------------------------------------------------------- DeviceArray views
BASE = 1 << 20
INDEX_CASES = [
    (slice(None),), (slice(2, 9),), (slice(1, None, 2),), (3,), (-1,), (slice(None), slice(None)), (slice(2, 7), slice(3, 11)),
    (slice(None, None, 2), slice(1, None, 3)), (4, slice(None)), (slice(None), 5), (slice(1, 6), -2), (slice(-5, -1), slice(-7, None, 2)),
    (slice(100, 200), slice(0, 3)), (slice(0, 4, 7), slice(0, 1)),
]


@pytest.mark.parametrize("dtype", (np.float32, np.float64, np.uint8, np.int16), ids=lambda d: np.dtype(d).name)
def test_slices_and_integers_give_numpys_pointer_and_strides(dtype):
    for shape in ((12, 17), (5, 12, 17), (40,)):
        host = np.zeros(shape, dtype)
        dev = DeviceArray._from_parts(BASE, shape, dtype, None, owner=host)
        assert dev.strides == host.strides and dev.nbytes == host.nbytes and dev.ptr == BASE and dev.device == 0
        for index in INDEX_CASES:
            if len(index) > len(shape) or all(isinstance(i, int) for i in index) and len(index) == len(shape):
                continue
            h, d = host[index], dev[index]
            assert d.shape == h.shape and d.dtype == h.dtype, index
            if h.size:
                assert d.ptr - BASE == h.ctypes.data - host.ctypes.data, index
                assert all(ds == hs for ds, hs, n in zip(d.strides, h.strides, h.shape) if n > 1), index
            assert d._owner is host and d._pending is dev._pending  # a view keeps the buffer alive and shares what is pending on it
            if len(index) == 1 and h.ndim >= 2 and h.size:  # views of views
                h2, d2 = h[1:, ::2], d[1:, ::2]
                assert d2.shape == h2.shape and d2.strides == h2.strides and d2.ptr - BASE == h2.ctypes.data - host.ctypes.data


def test_what_a_device_array_refuses():
    dev = DeviceArray._from_parts(BASE, (6, 8), np.float32)
    for index in ((slice(None, None, -1),), (slice(None), slice(5, 1, -2)), (slice(None, None, 0),)):
        with pytest.raises(ValueError, match="positive step"):
            dev[index]
    with pytest.raises(IndexError):
        dev[6]
    with pytest.raises(IndexError):
        dev[0, 0, 0]
    with pytest.raises(IndexError):
        dev[1, 2]
    with pytest.raises(TypeError):
        dev[[1, 2]]
    with pytest.raises(TypeError):
        DeviceArray(BASE, (6, 8))
    with pytest.raises(ValueError, match="not supported"):
        DeviceArray._from_parts(BASE, (6, 8), np.complex64)
    with pytest.raises(ValueError, match="negative strides"):
        DeviceArray._from_parts(BASE, (6, 8), np.float32, (-32, 4))
    with pytest.raises(ValueError, match="multiples of the item size"):
        DeviceArray._from_parts(BASE, (6, 8), np.float32, (34, 4))
    with pytest.raises(ValueError, match="dimensions"):
        DeviceArray._from_parts(BASE, (2, 2, 2, 2), np.float32)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
class Protocol:
    """A foreign array: nothing but the dict (and, where a test wants one, the device it says it lives on)."""

    def __init__(self, array, **changes):
        self.__cuda_array_interface__ = {**array.__cuda_array_interface__, **changes}


def test_names_are_exported():
    for name in ("DeviceArray", "to_device", "device_empty"):
        assert name in rp.__all__ and hasattr(rp, name)
    assert rp.DeviceArray is DeviceArray
    import sys

    assert "torch" not in device_array.__dict__ and "cupy" not in sys.modules


def test_cuda_array_interface_of_contiguous_and_strided_arrays():
    dev = DeviceArray._from_parts(BASE, (6, 8), np.float64)
    assert dev.__cuda_array_interface__ == {"shape": (6, 8), "typestr": "<f8", "data": (BASE, False), "version": 3, "strides": None, "stream": None}
    v = dev[1:5, ::2]
    assert v.__cuda_array_interface__ == {"shape": (4, 4), "typestr": "<f8", "data": (BASE + 64, False), "version": 3, "strides": (64, 16),
                                          "stream": None}
    assert dev[2:4].__cuda_array_interface__["strides"] is None and dev[:, 0:1].__cuda_array_interface__["strides"] == (64, 8)
    dev._pending.stream = 0xABC0  # a write was enqueued on that stream: every view of the buffer says so
    assert v.__cuda_array_interface__["stream"] == 0xABC0
    # and back in: the dict alone describes the same array
    back = device_array.as_device_array(Protocol(v), 0)
    assert (back.ptr, back.shape, back.dtype, back.strides, back._pending.stream) == (v.ptr, v.shape, v.dtype, v.strides, 0xABC0)
    assert device_array.as_device_array(Protocol(dev), 0).strides == (64, 8)
    assert device_array.as_device_array(dev, 0) is dev
    assert device_array.stream_handle(None) is None and device_array.stream_handle(5) == 5 and device_array.stream_handle(ctypes.c_void_p(7)) == 7

    class Torchish:
        cuda_stream = 9

    assert device_array.stream_handle(Torchish()) == 9
    with pytest.raises(TypeError):
        device_array.stream_handle("s")


def _transform():
    return rp.ArrayPSFTransform(rp.IndexedCube([(0, 0)], np.ones((1, 16, 16), np.complex64)))


def test_protocol_objects_that_are_refused():
    t = _transform()
    dev = DeviceArray._from_parts(BASE, (16, 16), np.float32)
    with pytest.raises(ValueError, match="negative strides"):
        t.apply(Protocol(dev, strides=(-64, 4)))
    with pytest.raises(ValueError, match="multiples of the item size"):
        t.apply(Protocol(dev, strides=(66, 4)))
    elsewhere = Protocol(dev)
    elsewhere.device = 1
    with pytest.raises(ValueError, match="device 1"):
        t.apply(elsewhere)
    with pytest.raises(ValueError, match="device 3"):
        t.apply(DeviceArray._from_parts(BASE, (16, 16), np.float32, device=3))
    with pytest.raises(ValueError, match="device 1"):
        t.apply_batch([elsewhere])
    with pytest.raises(ValueError, match="read-only"):
        device_array.as_device_array(Protocol(dev, data=(BASE, True)), 0, writeable=True, what="out")
    assert device_array.as_device_array(Protocol(dev, data=(BASE, True)), 0).ptr == BASE  # as an input it is fine
    with pytest.raises(ValueError, match="two dimensional"):
        t.apply(DeviceArray._from_parts(BASE, (2, 16, 16), np.float32))
    empty = rp.ArrayPSFTransform(rp.IndexedCube([], np.zeros((0, 16, 16), np.complex64)))
    with pytest.raises(ValueError, match="need at least one array to stack"):
        empty.apply(dev)


def test_mixing_host_and_device_frames_is_refused():
    t = _transform()
    dev = DeviceArray._from_parts(BASE, (16, 16), np.float32)
    with pytest.raises(ValueError, match="mixes host and device"):
        t.apply_batch([dev, np.zeros((16, 16), np.float32)])
    with pytest.raises(ValueError, match="mixes host and device"):
        t.apply_batch((np.zeros((16, 16), np.float32), Protocol(dev)))
    with pytest.raises(ValueError, match=r"\(frames, H, W\)"):
        t.apply_batch(dev)
    with pytest.raises(ValueError, match="one shape"):
        t.apply_batch([dev, dev[:8]])
    with pytest.raises(ValueError, match="stream"):
        t.apply(np.zeros((16, 16), np.float32), stream=5)
