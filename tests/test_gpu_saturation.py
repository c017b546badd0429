"""The saturation branch of apply on the GPU (kernels F1 - F5, csrc/saturation.hip).

On float32 frames the device route has exactly one result per step, so everything here is compared as bits: the filled padded frame
against the host route's fill and against the CPU emulator, the whole route against ``saturation="host"``, the device entry against
the class route.  The oracle bar (1e-5 of the peak) is checked on top, and for the frames the device rounds to float32.
"""

import numpy as np
import pytest

import regularizepsf_amd as rp
from oracle import regpsf_oracle as orc
from regularizepsf_amd import _native
from tests import saturation_cases as sc

pytestmark = pytest.mark.gpu
TOL = 1e-5
THRESHOLD = 2.0e4
ROUTE = [(16, (40, 48), "wrap", 1, 7), (32, (96, 128), "reflect", 2, 5), (64, (200, 192), "edge", 3, 2), (128, (300, 260), "constant", 1, 3),
         (256, (512, 640), "reflect", 1, 9)]


def _fill_plan(n):
    return _native.Plan(n, [(0, 0)])


def _frame(n, shape, seed=0):
    """tests/test_gpu_edge.py's saturated frame: hot pixels in the corners, on the rim, in a cluster, at random, and the 4 x 5 blob."""
    h, w = shape
    rng = np.random.default_rng(n + seed)
    image = orc.starfield(h, w, seed=3 * n + seed).astype(np.float64)
    hot = [(0, 0), (h - 1, w - 1), (1, w // 2), (h // 2, 0), (h // 2, w // 2), (h // 2, w // 2 + 1), (h // 2 + 1, w // 2)]
    hot += [(int(r), int(c)) for r, c in zip(rng.integers(0, h, 12), rng.integers(0, w, 12))]
    for r, c in hot:
        image[r, c] = 5.0e4 + r + c
    image[h // 3 : h // 3 + 4, w // 3 : w // 3 + 5] = 7.0e4
    return image, hot


def _within_the_bar(out, ref):
    bad = ~np.isfinite(ref)
    assert np.array_equal(~np.isfinite(out), bad), "non-finite pattern differs"
    good = ~bad
    d = out[good] - ref[good]
    print(f"max|d|/max|ref| = {np.abs(d).max() / np.abs(ref[good]).max():.3e}, rel-L2 = {np.linalg.norm(d) / np.linalg.norm(ref[good]):.3e}")
    assert np.abs(d).max() <= TOL * np.abs(ref[good]).max()
    assert np.linalg.norm(d) <= TOL * np.linalg.norm(ref[good])


def _same_bits(a, b, what):
    sc.assert_same_bits(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32), what)


# ------------------------------------------------------------------------------------------------ 1: F1 - F4 alone
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_filled_padded_frame_and_mask_have_the_host_fills_bits(name):
    sc.precondition(name)
    _, n, _, pad_mode, (dilation, width) = sc.CASES[name]
    want, mask, _ = sc.reference(name)
    got, got_mask, groups = _fill_plan(n).saturation_fill_device(sc.frame(name), _native.PAD_MODES[pad_mode], sc.THRESHOLD, dilation, width)
    assert np.array_equal(got_mask, mask)
    sc.assert_same_bits(got, want, name)
    assert (groups == 0) == (not mask.any())


# ------------------------------------------------------------------------------------------------ 2: the whole route
@pytest.mark.parametrize(("n", "shape", "other_mode", "dilation", "width"), ROUTE)
def test_device_route_has_the_host_routes_bits_on_float32_frames(n, shape, other_mode, dilation, width):
    coords, k = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)
    image, hot = _frame(n, shape)
    image = image.astype(np.float32)
    before = image.copy()
    host = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    device = rp.ArrayPSFTransform(rp.IndexedCube(coords, k), saturation="device")
    for pad_mode in ("symmetric", other_mode):
        kwargs = dict(pad_mode=pad_mode, saturation_threshold=THRESHOLD, saturation_dilation=dilation, neighborhood_width=width)
        out = device.apply(image, **kwargs)
        assert out.dtype == np.float64 and np.array_equal(image, before)  # the input is never modified
        want = host.apply(image, **kwargs)
        assert np.array_equal(out, want, equal_nan=True) and np.array_equal(np.isnan(out), np.isnan(want))
        _same_bits(out, want, f"N = {n}, {pad_mode}")
        for r, c in hot:
            assert out[r, c] == float(image[r, c])
    _within_the_bar(out, orc.apply_transfer(image, coords, k, **kwargs))


@pytest.mark.parametrize(("n", "shape", "pad_mode", "dtype"), [(32, (96, 128), "symmetric", np.float64), (64, (192, 192), "symmetric", np.int32),
                                                               (128, (300, 260), "reflect", np.float64)])
def test_float64_and_integer_frames_meet_the_oracle_and_get_their_own_values_back(n, shape, pad_mode, dtype):
    coords, k = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)
    image, hot = _frame(n, shape)
    if dtype == np.float64:
        image += 1.0 / 3.0  # no pixel is a float32 number
        image[shape[0] // 4, shape[1] // 4] = np.nan
        assert not np.array_equal(image, image.astype(np.float32).astype(np.float64))
    image = image.astype(dtype)
    before = image.copy()
    kwargs = dict(pad_mode=pad_mode, saturation_threshold=THRESHOLD, saturation_dilation=2, neighborhood_width=5)
    out = rp.ArrayPSFTransform(rp.IndexedCube(coords, k), saturation="device").apply(image, **kwargs)
    assert np.array_equal(image, before, equal_nan=True)
    _within_the_bar(out, orc.apply_transfer(image, coords, k, **kwargs))
    from scipy.ndimage import binary_dilation

    mask = binary_dilation(np.nan_to_num(image.astype(np.float64)) > THRESHOLD, iterations=2)  # at least these (mirror images may add more)
    assert mask.sum() >= len(hot) and np.array_equal(out[mask], image.astype(np.float64)[mask])
    for r, c in hot:
        assert out[r, c] == float(image[r, c])


def test_generic_patch_size_meets_the_oracle():
    n, shape = 24, (96, 120)
    coords, k = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)
    image, hot = _frame(n, shape)
    image = image.astype(np.float32)
    kwargs = dict(saturation_threshold=THRESHOLD, saturation_dilation=1, neighborhood_width=7)
    out = rp.ArrayPSFTransform(rp.IndexedCube(coords, k), saturation="device").apply(image, **kwargs)
    _within_the_bar(out, orc.apply_transfer(image, coords, k, **kwargs))
    for r, c in hot:
        assert out[r, c] == float(image[r, c])


def test_apply_batch_is_the_loop_bit_for_bit():
    n, shape = 32, (96, 128)
    coords, k = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)
    stack = [_frame(n, shape, seed=s)[0].astype(np.float32) for s in (1, 2, 3)]
    stack[1] = np.minimum(stack[1], 1.0e4)  # nothing above the threshold
    assert stack[0].max() > THRESHOLD > stack[1].max()
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k), saturation="device")
    kwargs = dict(saturation_threshold=THRESHOLD, saturation_dilation=2, neighborhood_width=5)
    loop = np.stack([t.apply(im, **kwargs) for im in stack])
    assert np.array_equal(t.apply_batch(stack, **kwargs), loop, equal_nan=True)
    assert np.array_equal(t.apply_batch(np.stack(stack), dtype=np.float32, **kwargs), loop.astype(np.float32), equal_nan=True)
    t.saturation = "host"
    assert np.array_equal(t.apply_batch(stack, **kwargs), loop, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 3: the device entry
def _resident_apply(plan, image, pad_mode, dilation, width):
    img = _native.DeviceBuffer(image.nbytes).upload(image)
    out = _native.DeviceBuffer(image.nbytes)
    try:
        masked = plan.apply_device_saturated(img.ptr, out.ptr, *image.shape, _native.PAD_MODES[pad_mode], THRESHOLD, dilation, width)
        plan.synchronize()
        return out.download(image.shape), masked
    finally:
        img.free()
        out.free()


def test_device_entry_equals_the_class_route_and_reuses_and_grows_its_scratch():
    n, shape, other = 32, (96, 128), (112, 152)
    coords, k = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)  # (its corners are valid for the larger frame too)
    image = _frame(n, shape)[0].astype(np.float32)
    larger = _frame(n, other, seed=4)[0].astype(np.float32)
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k), saturation="device")
    kwargs = dict(saturation_threshold=THRESHOLD, saturation_dilation=2, neighborhood_width=5)
    want, want_larger = t.apply(image, **kwargs).astype(np.float32), t.apply(larger, **kwargs).astype(np.float32)
    plan = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))._device_plan()
    first, masked = _resident_apply(plan, image, "symmetric", 2, 5)
    assert masked > 20
    _same_bits(first, want, "first call")
    _same_bits(_resident_apply(plan, image, "symmetric", 2, 5)[0], want, "second call on the same scratch")
    _same_bits(_resident_apply(plan, larger, "symmetric", 2, 5)[0], want_larger, "a larger frame: the scratch grows")
    _same_bits(_resident_apply(plan, image, "symmetric", 2, 5)[0], want, "the first frame again, on the grown scratch")
    fresh = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))._device_plan()
    _same_bits(_resident_apply(fresh, image, "symmetric", 2, 5)[0], want, "a fresh plan")
    calm = np.minimum(image, 1.0e4)
    out, masked = _resident_apply(plan, calm, "symmetric", 2, 5)
    assert masked == 0
    _same_bits(out, t.apply(calm, **kwargs).astype(np.float32), "nothing hot: the padded frame is corrected as it is")
    ms = plan.saturation_kernel_ms()
    assert ms.shape == (5,) and ms[0] > 0 and ms[4] > 0 and (ms[1:4] == 0).all()


# ------------------------------------------------------------------------------------------------ 4: hardware-only hazards, as bits
@pytest.mark.parametrize("name", ["mixed", "mixed_edge", "pair_h_plus_1", "column70"])
def test_group_order_earlier_frames_and_the_emulator_give_the_same_bits(name):
    _, n, _, pad_mode, (dilation, width) = sc.CASES[name]
    mode = _native.PAD_MODES[pad_mode]
    plan = _fill_plan(n)
    forward, mask, groups = plan.saturation_fill_device(sc.frame(name), mode, sc.THRESHOLD, dilation, width)
    assert groups >= 2 or name == "column70"
    backward, _, _ = plan.saturation_fill_device(sc.frame(name), mode, sc.THRESHOLD, dilation, width, reverse_groups=True)
    sc.assert_same_bits(backward, forward, "groups taken last first")
    full = np.full_like(sc.frame(name), sc.HOT)  # every pixel hot: one group, every label, fill slot and list entry used
    filled, full_mask, full_groups = plan.saturation_fill_device(full, mode, sc.THRESHOLD, dilation, width)
    full_want, full_want_mask, _ = sc.reference_fill(full, n, pad_mode, dilation, width)
    assert np.array_equal(full_mask, full_want_mask) and full_groups == 1 and (full_mask.all() or pad_mode == "constant")
    sc.assert_same_bits(filled, full_want, "every pixel hot")
    after, after_mask, _ = plan.saturation_fill_device(sc.frame(name), mode, sc.THRESHOLD, dilation, width)
    assert np.array_equal(after_mask, mask)
    sc.assert_same_bits(after, forward, "after a fully hot frame on the same scratch")
    sc.assert_same_bits(_fill_plan(n).saturation_fill_device(sc.frame(name), mode, sc.THRESHOLD, dilation, width)[0], forward, "a fresh plan")
    emulated, emu_mask, emu_groups = sc.emu_fill(sc.frame(name), n, pad_mode, dilation, width)
    assert np.array_equal(emu_mask, mask) and emu_groups == groups
    sc.assert_same_bits(forward, emulated, "GPU against the emulator")


# ------------------------------------------------------------------------------------------------ 5: API
def test_windows_that_are_always_empty_and_dilations_below_one_stay_with_the_host_route():
    n, shape = 32, (96, 128)
    coords, k = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)
    image = _frame(n, shape)[0].astype(np.float32)
    host = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    device = rp.ArrayPSFTransform(rp.IndexedCube(coords, k), saturation="device")
    assert host.saturation == "host" and device.saturation == "device"
    for dilation, width in ((1, 0), (1, 1), (0, 7), (-1, 7)):
        kwargs = dict(saturation_threshold=THRESHOLD, saturation_dilation=dilation, neighborhood_width=width)
        assert np.array_equal(device.apply(image, **kwargs), host.apply(image, **kwargs), equal_nan=True), (dilation, width)
    plan = device._device_plan()
    buf = _native.DeviceBuffer(image.nbytes).upload(image)
    with pytest.raises(_native.NativeError, match="neighborhood_width"):
        plan.apply_device_saturated(buf.ptr, buf.ptr, *shape, 1, THRESHOLD, 1, 1)
    with pytest.raises(_native.NativeError, match="dilation"):
        plan.apply_device_saturated(buf.ptr, buf.ptr, *shape, 1, THRESHOLD, 0, 7)
    buf.free()
