"""Device arrays on the GPU: the conversion kernels C1 / C2 against the emulator and NumPy, and ``apply`` / ``apply_batch`` on
``DeviceArray`` views against the host route of the same transform, bit for bit (cases: tests/device_array_cases.py).

Every view under test is carved out of a larger DeviceArray that is filled with NaN (inputs) or a sentinel (outputs) and has at least 64
elements before the view, behind it and between two of its rows: an indexing mistake shows as a changed sentinel or a NaN in the result,
inside the test's own allocation.  No torch or cupy tensor is made here: the protocol is exercised with DeviceArray and with a bare object
that carries nothing but a ``__cuda_array_interface__`` dict.
"""

import functools

import numpy as np
import pytest

import regularizepsf_amd as rp
from oracle import regpsf_oracle as orc
from regularizepsf_amd import _native
from regularizepsf_amd.device_array import DeviceArray
from tests import device_array_cases as dc
from tests import saturation_cases as sc
from tests.helpers import random_transfer, rel_errors

pytestmark = pytest.mark.gpu
TOL = 1e-5  # of the frame's peak (and of its norm), against the oracle
C1, C2, SAT, STAGED = _native.ROUTE_C1, _native.ROUTE_C2, _native.ROUTE_SATURATED, _native.ROUTE_STAGED


class Protocol:
    """A foreign array: nothing but the dict (it keeps the DeviceArray it describes alive, as a foreign library keeps its tensor)."""

    def __init__(self, array, **changes):
        self._keep = array
        self.__cuda_array_interface__ = {**array.__cuda_array_interface__, **changes}


# ---------------------------------------------------------------------------------------------------------------- carving
def carve(values: np.ndarray, view: str):
    """``values`` as the view ``view`` of a NaN- (integers: sentinel-) filled device buffer: (view, buffer, host copy of the buffer, index)."""
    flat = dc.aligned_flat(dc.layout(values.shape, view)[0], values.dtype, dc.sentinel(values.dtype))
    v, index = dc.host_view(flat, values.shape, view)
    v[...] = values
    big = rp.to_device(flat)
    return dc.device_view(big, values.shape, view), big, flat, index


def carve_out(shape, dtype, view: str):
    """An output view of a sentinel-filled device buffer: (view, check) - check(want) asserts the view's bits and the sentinels."""
    fill = dc.sentinel(dtype)
    flat = dc.aligned_flat(dc.layout(shape, view)[0], dtype, fill)
    _, index = dc.host_view(flat, shape, view)
    big = rp.to_device(flat)
    out = dc.device_view(big, shape, view)

    def check(want, what=""):
        after = big.to_host()
        assert dc.untouched(after, index, fill), f"{what}: a sentinel outside the {view} view changed"
        dc.same_bits(after[index].reshape(shape), np.ascontiguousarray(want), what)
        dc.same_bits(out.to_host(), np.ascontiguousarray(want), what)

    return out, check


# ---------------------------------------------------------------------------------------------------------------- the conversion kernels
@pytest.mark.parametrize("dtype", dc.IN_DTYPES, ids=lambda d: np.dtype(d).name)
def test_c1_equals_the_emulator_and_numpy(dtype):
    for view in sorted(dc.VIEWS):
        for shape in dc.SHAPES:
            values = dc.input_values(dtype, shape)
            what = f"C1 {np.dtype(dtype).name} {shape} {view}"
            src, big, flat, _ = carve(values, view)
            dense, check = carve_out(shape, np.float32, "dense")
            _native.convert_view(src._view2d(), dense._view2d())
            check(dc.to_float32(values), what)
            check(dc.emu_gather(dc.host_view(flat, shape, view)[0])[0], what + " (emulator)")
            dc.same_bits(big.to_host(), flat, what + ": the input")


@pytest.mark.parametrize("dtype", dc.OUT_DTYPES, ids=lambda d: np.dtype(d).name)
def test_c2_equals_the_emulator_and_numpy_and_writes_nothing_else(dtype):
    for view in sorted(dc.VIEWS):
        for shape in dc.SHAPES:
            values = dc.dense_values(shape, dtype)
            what = f"C2 {np.dtype(dtype).name} {shape} {view}"
            src, _, _, _ = carve(values, "dense")
            out, check = carve_out(shape, dtype, view)
            _native.convert_view(src._view2d(), out._view2d())
            check(dc.from_float32(values, dtype), what)
            emu = np.zeros(shape, dtype)
            dense = dc.aligned_flat(values.size, np.float32, 0).reshape(shape)
            dense[...] = values
            dc.emu_scatter(dense, emu)
            check(emu, what + " (emulator)")


@pytest.mark.parametrize("dtype", dc.IN_DTYPES, ids=lambda d: np.dtype(d).name)
def test_to_device_and_to_host_round_trip(dtype):
    values = dc.input_values(dtype, (70, 131), seed=9)
    dev = rp.to_device(values)
    assert isinstance(dev, DeviceArray) and dev.dtype == values.dtype and dev.shape == values.shape and dev.strides == values.strides
    assert dev.nbytes == values.nbytes and dev.device == 0 and dev.ptr
    dc.same_bits(dev.to_host(), values)
    dc.same_bits(np.asarray(dev), values)
    for index in ((slice(3, 60, 2), slice(5, None, 3)), (slice(10, 20),), (7,), (slice(None), 4)):
        dc.same_bits(dev[index].to_host(), np.ascontiguousarray(values[index]), str(index))
    out = np.zeros((70, 131), dtype)
    assert dev.to_host(out=out) is out
    dc.same_bits(out, values)
    stack = rp.to_device(np.stack([values, values[::-1]]))
    dc.same_bits(stack[1, 2:5].to_host(), values[::-1][2:5])
    # writing into a strided view leaves everything around it as it was
    dev[1:9:3, 2:40:5]._assign(np.ones((3, 8), dtype))
    want = values.copy()
    want[1:9:3, 2:40:5] = 1
    dc.same_bits(dev.to_host(), want)
    empty = rp.device_empty((4, 6), dtype)
    assert empty.shape == (4, 6) and empty.dtype == np.dtype(dtype) and empty.c_contiguous and empty.to_host().shape == (4, 6)
    assert rp.to_device(np.zeros((0, 5), dtype)).to_host().shape == (0, 5)


# ---------------------------------------------------------------------------------------------------------------- apply
@functools.cache
def transform(n):
    coords, k, _ = dc.apply_case(n)
    return rp.ArrayPSFTransform(rp.IndexedCube(coords, k))


@functools.cache
def host_result(n, dtype=np.float32, view=None):
    """The host route on the case's frame as ``dtype`` (a column view: every ``view``-th column), narrowed to float32 first: float32 out."""
    frame = dc.frame_as(dc.apply_case(n)[2], dtype)
    frame = frame if view is None else frame[:, ::view]
    t = transform(n) if view is None else column_transform(n, view)
    result = t.apply(np.ascontiguousarray(frame).astype(np.float32), out=np.empty(frame.shape, np.float32))
    result.flags.writeable = False
    return result


@functools.cache
def column_transform(n, step):
    """A transform for the frame of every ``step``-th column (its own covering)."""
    shape = dc.apply_case(n)[2][:, ::step].shape
    coords, k = random_transfer(shape, n, 4300 + n)
    return rp.ArrayPSFTransform(rp.IndexedCube(coords, k))


@pytest.mark.parametrize("n", sorted(dc.APPLY_SHAPES))
def test_apply_on_the_zero_copy_route_has_the_host_routes_bits(n):
    coords, k, frame = dc.apply_case(n)
    t, want = transform(n), host_result(n)
    dev = rp.to_device(frame)
    got = t.apply(dev)
    assert isinstance(got, DeviceArray) and got.dtype == np.float32 and got.shape == frame.shape and t.last_route == 0
    assert got.__cuda_array_interface__["stream"] is None  # the safe mode has waited
    dc.same_bits(got.to_host(), want, f"N = {n}, dense")
    # the suite's bar against the oracle, so that this file stands on its own
    ref = orc.apply_transfer(frame, coords, k)
    assert max(rel_errors(got.to_host(), ref)) <= TOL
    # pitched and offset views on both sides: in place (route 0), nothing but the view written
    for view_in, view_out in (("off1pitch3", "pitch5"), ("pitch1", "off1pitch3"), ("off3", "dense")):
        src, big, flat, _ = carve(frame, view_in)
        out, check = carve_out(frame.shape, np.float32, view_out)
        assert t.apply(src, out=out) is out and t.last_route == 0
        check(want, f"N = {n}, {view_in} -> {view_out}")
        dc.same_bits(big.to_host(), flat, "the input")


@pytest.mark.parametrize("n", dc.CONVERTED_SIZES)
def test_converted_routes_have_the_host_routes_bits(n):
    _, _, frame = dc.apply_case(n)
    t = transform(n)
    for dtype in (np.float64, np.float16, np.uint16, np.int32):
        values = dc.frame_as(frame, dtype)
        for view in ("dense", "off1pitch3", "col2"):
            src, _, _, _ = carve(values, view)
            got = t.apply(src)
            assert t.last_route == C1 and got.dtype == np.float32
            dc.same_bits(got.to_host(), host_result(n, dtype), f"N = {n}, {np.dtype(dtype).name} {view}")
    # a float32 view of every second column: C1 gathers it
    wide = np.full((frame.shape[0], frame.shape[1] * 2), np.nan, np.float32)
    wide[:, ::2] = frame
    got = t.apply(rp.to_device(wide)[:, ::2])
    assert t.last_route == C1
    dc.same_bits(got.to_host(), host_result(n), f"N = {n}, column step 2")
    half = column_transform(n, 2)
    got = half.apply(rp.to_device(frame)[:, ::2])
    assert half.last_route == C1
    dc.same_bits(got.to_host(), host_result(n, np.float32, 2), f"N = {n}, every second column of the frame")
    # outputs
    dev = rp.to_device(frame)
    for dtype in (np.float64, np.float16):
        want = dc.from_float32(host_result(n), dtype)
        for view in ("dense", "off1pitch3", "col2"):
            out, check = carve_out(frame.shape, dtype, view)
            assert t.apply(dev, out=out) is out and t.last_route == C2
            check(want, f"N = {n}, out {np.dtype(dtype).name} {view}")
    src, _, _, _ = carve(dc.frame_as(frame, np.float64), "pitch1")
    out, check = carve_out(frame.shape, np.float64, "pitch5")
    t.apply(src, out=out)
    assert t.last_route == C1 | C2
    check(dc.from_float32(host_result(n, np.float64), np.float64), "float64 -> float64")
    out, check = carve_out(frame.shape, np.float32, "col3")  # a float32 output that is not contiguous along its rows
    t.apply(dev, out=out)
    assert t.last_route == C2
    check(host_result(n), "float32 column step 3")


# ---------------------------------------------------------------------------------------------------------------- batches
def stack_view(frames: np.ndarray, gap: int):
    """(frames, H, W) as a device stack whose planes lie ``gap`` elements apart: (stack view, buffer, host copy of the buffer)."""
    count, h, w = frames.shape
    stride = h * w + gap
    flat = dc.aligned_flat(dc.MARGIN + count * stride + dc.MARGIN, frames.dtype, dc.sentinel(frames.dtype))
    for f in range(count):
        flat[dc.MARGIN + f * stride : dc.MARGIN + f * stride + h * w] = frames[f].reshape(-1)
    big = rp.to_device(flat)
    isz = frames.dtype.itemsize
    return DeviceArray._from_parts(big.ptr + dc.MARGIN * isz, frames.shape, frames.dtype, (stride * isz, w * isz, isz), big, 0, big._pending), big, flat


@pytest.mark.parametrize("n", dc.CONVERTED_SIZES)
def test_batches_have_the_bits_of_the_loop_over_apply(n):
    _, _, frame = dc.apply_case(n)
    t = transform(n)
    frames = np.stack([frame, frame[::-1] * 0.5, frame + 3]).astype(np.float32)
    loop = [t.apply(rp.to_device(f)).to_host() for f in frames]
    # a float32 stack with a padded frame stride: in place
    stack, big, flat = stack_view(frames, 68)
    got = t.apply_batch(stack, dtype=np.float32)
    assert isinstance(got, DeviceArray) and got.shape == frames.shape and got.dtype == np.float32 and t.last_route == 0
    for f in range(3):
        dc.same_bits(got[f].to_host(), loop[f], f"N = {n}, frame {f}")
    out, out_big, out_flat = stack_view(np.full(frames.shape, np.nan, np.float32), 132)
    assert t.apply_batch(stack, out=out) is out and t.last_route == 0
    after = out_big.to_host()
    for f in range(3):
        dc.same_bits(out[f].to_host(), loop[f], f"N = {n}, frame {f} with out=")
    dc.same_bits(big.to_host(), flat, "the input stack")
    touched = np.isnan(out_flat) & ~np.isnan(after)
    assert touched.sum() == frames.size  # as many elements written as the frames have, the gaps and margins still NaN
    assert t.apply_batch(stack).dtype == np.float64 and t.last_route == C2  # the default dtype of apply_batch: converted on the way out
    # a uint16 stack and a list of three separate frames: gathered into the plan's staging stack
    ints = np.stack([dc.frame_as(f, np.uint16) for f in frames])
    int_loop = [t.apply(rp.to_device(f)).to_host() for f in ints]
    got = t.apply_batch(stack_view(ints, 70)[0], dtype=np.float32)
    assert t.last_route == C1 | STAGED
    for f in range(3):
        dc.same_bits(got[f].to_host(), int_loop[f], f"N = {n}, uint16 frame {f}")
    order = (2, 0, 1)  # not evenly spaced: nothing a frame stride describes
    out = rp.device_empty(frames.shape, np.float32)
    assert t.apply_batch([stack[f] for f in order], out=out) is out and t.last_route == C1 | STAGED
    for i, f in enumerate(order):
        dc.same_bits(out[i].to_host(), loop[f], f"N = {n}, list frame {f}")
    got = t.apply_batch([Protocol(stack[f]) for f in order], dtype=np.float16)
    assert t.last_route == C1 | C2 | STAGED and got.dtype == np.float16
    for i, f in enumerate(order):
        dc.same_bits(got[i].to_host(), dc.from_float32(loop[f], np.float16), f"N = {n}, list frame {f} as float16")


# ---------------------------------------------------------------------------------------------------------------- saturation
SATURATION_CASES = ("isolated", "nothing_hot", "corners_edges")  # the smallest frames: something hot, nothing hot, a hot pad edge


@functools.cache
def saturation_transforms():
    coords, k = random_transfer((40, 48), 32, 4432)
    cube = rp.IndexedCube(coords, k)
    return rp.ArrayPSFTransform(cube), rp.ArrayPSFTransform(rp.IndexedCube(coords, k.copy()), saturation="device")


@pytest.mark.parametrize("name", SATURATION_CASES)
def test_saturation_on_device_frames_has_the_device_routes_bits(name):
    _, _, shape, pad_mode, (dilation, width) = sc.CASES[name]
    assert shape == (40, 48)
    frame = sc.frame(name)
    t, t_device = saturation_transforms()
    args = dict(pad_mode=pad_mode, saturation_threshold=sc.THRESHOLD, saturation_dilation=dilation, neighborhood_width=width)
    want = t_device.apply(frame, **args)
    assert want.dtype == np.float64 and np.array_equal(want.astype(np.float32).astype(np.float64), want, equal_nan=True)
    want = want.astype(np.float32)
    got = t.apply(rp.to_device(frame), **args)  # saturation="host": a device frame takes the device kernels all the same
    assert t.last_route == SAT
    dc.same_bits(got.to_host(), want, name)
    src, _, _, _ = carve(frame, "off1pitch3")  # the saturation entry points take dense frames: a pitched one is gathered first
    out, check = carve_out(shape, np.float64, "pitch1")
    t.apply(src, out=out, **args)
    assert t.last_route == SAT | C1 | C2
    check(want.astype(np.float64), name + ", views")


def test_saturation_batch_equals_the_loop_and_the_fallbacks_equal_the_host_route():
    t, _ = saturation_transforms()
    frames = [sc.frame(name) for name in SATURATION_CASES]
    args = dict(pad_mode="symmetric", saturation_threshold=sc.THRESHOLD, saturation_dilation=1, neighborhood_width=7)
    loop = [t.apply(rp.to_device(f), **args).to_host() for f in frames]
    got = t.apply_batch(rp.to_device(np.stack(frames)), dtype=np.float32, **args)
    assert t.last_route == SAT
    for f in range(3):
        dc.same_bits(got[f].to_host(), loop[f], f"frame {f}")
    got = t.apply_batch([rp.to_device(f) for f in frames[::-1]], dtype=np.float32, **args)
    assert t.last_route & SAT
    for f in range(3):
        dc.same_bits(got[f].to_host(), loop[2 - f], f"list frame {f}")
    # what the device routes do not cover: down, the host route, up
    frame = frames[0]
    for changes in ({"pad_mode": "mean"}, {"neighborhood_width": 1}):
        fallback = {**args, **changes}
        t.last_route = -1
        got = t.apply(rp.to_device(frame), **fallback)
        assert t.last_route == -1 and got.dtype == np.float32  # no device route ran
        dc.same_bits(got.to_host(), t.apply(frame, **fallback).astype(np.float32), str(changes))
    out, check = carve_out(frame.shape, np.float64, "off1pitch3")
    assert t.apply(rp.to_device(frame), pad_mode="mean", out=out) is out
    check(t.apply(frame, pad_mode="mean"), "pad_mode='mean' without a threshold")
    got = t.apply_batch(rp.to_device(np.stack(frames)), pad_mode="linear_ramp")
    assert got.dtype == np.float64
    dc.same_bits(got.to_host(), t.apply_batch(np.stack(frames), pad_mode="linear_ramp"), "batch fallback")


# ---------------------------------------------------------------------------------------------------------------- streams
def test_applies_on_a_callers_stream_queue_up_without_a_host_wait():
    n = 32
    _, _, frame = dc.apply_case(n)
    t = transform(n)
    other = np.ascontiguousarray(frame[::-1])
    first, second = host_result(n), t.apply(other, out=np.empty(frame.shape, np.float32))
    third = t.apply(first, out=np.empty(frame.shape, np.float32))
    a, b = rp.to_device(frame), rp.to_device(other)
    o1, o2, o3 = (rp.device_empty(frame.shape) for _ in range(3))
    s = _native.Stream()
    handle = s.ptr.value
    assert t.apply(a, out=o1, stream=s) is o1
    assert t.apply(b, out=o2, stream=handle) is o2
    assert t.apply(o1, out=o3, stream=s) is o3  # consumes the first result, still pending on the same stream
    for o in (o1, o2, o3, o1[2:5]):
        assert o.__cuda_array_interface__["stream"] == handle
    dc.same_bits(o3.to_host(), third, "third")
    assert o3.__cuda_array_interface__["stream"] is None
    dc.same_bits(o1.to_host(), first, "first")
    dc.same_bits(o2.to_host(), second, "second")
    assert o1.__cuda_array_interface__["stream"] is None and o2.__cuda_array_interface__["stream"] is None
    # a result pending on one stream is waited for by an apply on another one (an event, no host wait), and by the safe mode
    s2 = _native.Stream()
    t.apply(a, out=o1, stream=s)
    t.apply(o1, out=o3, stream=s2)
    assert o1.__cuda_array_interface__["stream"] == handle and o3.__cuda_array_interface__["stream"] == s2.ptr.value
    dc.same_bits(o3.to_host(), third, "third, across streams")
    t.apply(b, out=o1, stream=s)
    got = t.apply(o1)
    assert o1.__cuda_array_interface__["stream"] is None
    dc.same_bits(got.to_host(), t.apply(second, out=np.empty(frame.shape, np.float32)), "safe mode behind a stream")
    # converted sides on a stream: the staging is the plan's
    src, _, _, _ = carve(dc.frame_as(frame, np.uint16), "col2")
    out64 = rp.device_empty(frame.shape, np.float64)
    t.apply(src, out=out64, stream=s)
    assert t.last_route == C1 | C2 and out64.__cuda_array_interface__["stream"] == handle
    dc.same_bits(out64.to_host(), host_result(n, np.uint16).astype(np.float64), "uint16 -> float64 on a stream")
    _native.check(_native.lib().rpsf_device_synchronize(0))
    s.close()
    s2.close()


# ---------------------------------------------------------------------------------------------------------------- the protocol
def test_a_bare_protocol_object_gives_the_bits_of_the_device_array_it_wraps():
    n = 32
    _, _, frame = dc.apply_case(n)
    t = transform(n)
    src, _, _, _ = carve(frame, "off1pitch3")
    got = t.apply(Protocol(src))
    assert isinstance(got, DeviceArray) and t.last_route == 0
    dc.same_bits(got.to_host(), host_result(n), "as input")
    out, check = carve_out(frame.shape, np.float32, "pitch5")
    wrapped = t.apply(Protocol(src), out=Protocol(out))
    assert isinstance(wrapped, DeviceArray) and wrapped is not out and t.last_route == 0
    assert (wrapped.ptr, wrapped.shape, wrapped.strides, wrapped.dtype) == (out.ptr, out.shape, out.strides, out.dtype)
    check(host_result(n), "as out")
    dc.same_bits(wrapped.to_host(), host_result(n), "the wrapping view")
    values = dc.frame_as(frame, np.float64)
    got = t.apply(Protocol(carve(values, "col2")[0]))
    assert t.last_route == C1
    dc.same_bits(got.to_host(), host_result(n, np.float64), "float64, column step 2")
    with pytest.raises(ValueError, match="read-only"):
        t.apply(src, out=Protocol(out, data=(out.ptr, True)))
    check(host_result(n), "a refused out")


# ---------------------------------------------------------------------------------------------------------------- exceptions
def test_the_host_routes_exceptions_are_raised_for_device_frames_and_nothing_is_written():
    n = 32
    coords, k, frame = dc.apply_case(n)
    t = transform(n)
    dev = rp.to_device(frame)
    out, check = carve_out(frame.shape, np.float32, "off1pitch3")
    untouched = np.full(frame.shape, np.nan, np.float32)
    with pytest.raises(ValueError, match="image must be two dimensional"):
        t.apply(rp.to_device(np.stack([frame, frame])), out=out)
    with pytest.raises(ValueError, match="need at least one array to stack"):
        rp.ArrayPSFTransform(rp.IndexedCube([], np.zeros((0, n, n), np.complex64))).apply(dev, out=out)
    far = rp.ArrayPSFTransform(rp.IndexedCube([*coords[:-1], (frame.shape[0] + n + 1, 0)], k))
    with pytest.raises(ValueError, match="lies outside the padded image"):
        far.apply(dev, out=out)
    with pytest.raises(ValueError, match="lies outside the padded image"):
        far.apply(frame)  # the host route says the same
    with pytest.raises(TypeError, match="patch coordinates must be integral"):
        rp.ArrayPSFTransform(rp.IndexedCube([(0.5, 0)], k[:1])).apply(dev, out=out)
    with pytest.raises(ValueError, match="out must have the image's shape"):
        t.apply(dev[1:], out=out)
    with pytest.raises(ValueError, match="float32, float64 or float16"):
        t.apply(dev, out=rp.device_empty(frame.shape, np.int32))
    with pytest.raises(ValueError, match=r"out must have shape \(frames, H, W\)"):
        t.apply_batch([dev, dev], out=rp.device_empty((3, *frame.shape)))
    check(untouched, "after the refusals")
    # the library refuses what the Python layer cannot see, and writes nothing either
    plan = t._device_plan()
    bad = out._view2d()
    bad.col_stride = 0
    with pytest.raises(_native.NativeError):
        plan.apply_view(dev._view2d(), bad, 1)
    bad = dev._view2d()
    bad.dtype = 9
    with pytest.raises(_native.NativeError):
        plan.apply_view(bad, out._view2d(), 1)
    with pytest.raises(_native.NativeError):
        plan.apply_view(dev._view2d(), out._view2d(), 7)  # no such pad mode
    with pytest.raises(_native.NativeError):
        plan.apply_view(dev._view2d(), out._view2d(), 1, threshold=10.0, neighborhood_width=1)
    _native.check(_native.lib().rpsf_device_synchronize(0))
    check(untouched, "after the library's refusals")
