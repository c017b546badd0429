"""Bad-pixel masks of apply on the GPU (``mask=``, ``fill_nonfinite=``; DESIGN.md 3.8, "Bad-pixel masks").

The filled padded frame, the mask M2 and the counts of the masked fill are compared as bits with the CPU emulator, which
tests/test_mask_host.py holds against the NumPy / SciPy definition.  The whole route is held against the float64 oracle on the filled
frame with the project's bar (max and 2-norm within 1e-5 of the reference's) on every pixel off M2 - no pixel is left out
for another reason: ``precondition`` asserts that the reference is finite there - and as exact equality with the input on M2.
"""

import math

import numpy as np
import pytest

import regularizepsf_amd as rp
from oracle import regpsf_oracle as orc
from regularizepsf_amd import _native
from tests import mask_cases as mc

pytestmark = pytest.mark.gpu
TOL = 1e-5
N = mc.N


def _transfer(shape):
    return orc.synthetic_transfer(*shape, N, alpha=1.0, epsilon=0.1)


def _definition(image32, m, pad_mode, dilation, width, threshold, fill_nonfinite, coords, k):
    """(H x W float64 result, M2 on the frame) of the definition: NumPy / SciPy mask, the host fill, the oracle on the filled padded frame."""
    h, w = image32.shape
    filled, m2, _, _, raw = mc.reference_fill(image32, m, N, pad_mode, dilation, width, threshold, fill_nonfinite)
    out = orc.apply_transfer(filled, [(r + 2 * N, c + 2 * N) for r, c in coords], k, pad_mode="constant").copy()
    assert out.shape == m2.shape
    out[m2] = raw[m2]
    inner = (slice(2 * N, 2 * N + h), slice(2 * N, 2 * N + w))
    return out[inner], m2[inner]


def _check(out, ref, inner, image, what):
    """The bar off M2, the input itself on M2."""
    out = np.asarray(out, np.float64)
    assert np.isfinite(ref[~inner]).all(), "the reference leaves no pixel out"
    d = out[~inner] - ref[~inner]
    rel_max, rel_l2 = np.abs(d).max() / np.abs(ref[~inner]).max(), np.linalg.norm(d) / np.linalg.norm(ref[~inner])
    print(f"{what}: max|d|/max|ref| = {rel_max:.3e}, rel-L2 = {rel_l2:.3e}, {inner.sum()} masked in-frame pixels")
    assert rel_max <= TOL and rel_l2 <= TOL
    assert np.array_equal(out[inner], np.asarray(image, np.float64)[inner], equal_nan=True), f"{what}: M2 must carry the input"


def _kwargs(name):
    _, _, pad_mode, (dilation, width), threshold, fill_nonfinite, _ = mc.CASES[name]
    return dict(pad_mode=pad_mode, saturation_threshold=threshold, saturation_dilation=dilation, neighborhood_width=width,
                fill_nonfinite=fill_nonfinite)


def _device_mask(m, storage):
    """The mask as a uint8 device array; 'strided': a view with a row pitch and a column stride of 2 into a buffer of ones."""
    if m is None:
        return None
    if storage != "strided":
        return rp.to_device(np.ascontiguousarray(m, np.uint8))
    view = mc.stored(m, storage)
    h, w = m.shape
    base = rp.to_device(np.ascontiguousarray(view.base))
    dev = base[:, 3 : 3 + 2 * w : 2]
    assert dev.shape == (h, w) and dev.strides == (2 * w + 6, 2)
    return dev


# ------------------------------------------------------------------------------------------------ 2: F1 - F4, bitwise
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_masked_fill_has_the_emulators_bits(name):
    mc.precondition(name)
    _, _, pad_mode, (dilation, width), threshold, fill_nonfinite, storage = mc.CASES[name]
    want, want_mask, (_, _, n_masked, groups) = mc.emulated(name)
    m = mc.stored(mc.mask(name), storage)
    plan = _native.Plan(N, [(0, 0)])
    for order in (2, 0):
        got, got_mask, got_groups, got_masked = plan.saturation_fill_masked_device([mc.frame(name)], _native.PAD_MODES[pad_mode], threshold, dilation,
                                                                                   width, None if m is None else m[None], fill_nonfinite, order)
        assert np.array_equal(got_mask[0], want_mask) and got_groups[0] == groups and got_masked[0] == n_masked
        mc.assert_same_bits(got[0], want, f"{name}, order {order}")
    assert np.array_equal(want_mask, mc.reference(name)[1])


def test_masked_fill_of_a_batch_with_an_idle_frame_has_the_emulators_bits():
    mc.batch_precondition()
    pad_mode, (dilation, width), threshold, fill_nonfinite = mc.BATCH_SETTINGS
    frames = [mc.frame(name) for name in mc.BATCH]
    masks = np.stack([mc.stored(mc.mask(name), "dense") for name in mc.BATCH])
    want, want_masks, counts = mc.emu_fill_batch(frames, masks, N, pad_mode, dilation, width, threshold, fill_nonfinite)
    plan = _native.Plan(N, [(0, 0)])
    first = None
    for _ in range(2):  # twice: two runs give the same bits, on scratch the first run left dirty
        got, got_masks, groups, masked = plan.saturation_fill_masked_device(frames, _native.PAD_MODES[pad_mode], threshold, dilation, width, masks,
                                                                            fill_nonfinite)
        assert np.array_equal(got_masks, want_masks) and np.array_equal(groups, counts[:, 3]) and np.array_equal(masked, counts[:, 2])
        for f in range(3):
            mc.assert_same_bits(got[f], want[f], mc.BATCH[f])
        first = got if first is None else first
        assert np.array_equal(got.view(np.uint32), first.view(np.uint32))
    assert masked[1] == 0 and groups[1] == 0 and not got_masks[1].any()
    for f, (_, m2, *_) in enumerate(mc.batch_reference()):
        assert np.array_equal(got_masks[f], m2)
    # one shared mask for all three frames
    shared = masks[0][None]
    got, got_masks, _, _ = plan.saturation_fill_masked_device(frames, _native.PAD_MODES[pad_mode], threshold, dilation, width, shared, fill_nonfinite)
    want, want_masks, _ = mc.emu_fill_batch(frames, shared, N, pad_mode, dilation, width, threshold, fill_nonfinite)
    assert np.array_equal(got_masks, want_masks)
    for f in range(3):
        mc.assert_same_bits(got[f], want[f], f"shared mask, frame {f}")


# ------------------------------------------------------------------------------------------------ 3: the whole route against the oracle
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_masked_apply_meets_the_bar_off_m2_and_returns_the_input_on_it(name):
    mc.precondition(name)
    _, shape, pad_mode, (dilation, width), threshold, fill_nonfinite, storage = mc.CASES[name]
    coords, k = _transfer(shape)
    image, m = mc.frame(name), mc.mask(name)
    before = image.copy()
    ref, inner = _definition(image, m, pad_mode, dilation, width, threshold, fill_nonfinite, coords, k)
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    out = t.apply(image, mask=m, **_kwargs(name))
    assert out.dtype == np.float64 and np.array_equal(image, before, equal_nan=True)
    _check(out, ref, inner, image, f"{name}, host frame")
    # a device frame with a device mask (for 'strided': row pitch and a column stride of 2) has the host frame's bits
    dev = t.apply(rp.to_device(image), mask=_device_mask(m, storage), **_kwargs(name))
    assert isinstance(dev, rp.DeviceArray) and dev.dtype == np.float32 and t.last_route & _native.ROUTE_SATURATED
    mc.assert_same_bits(dev.to_host(), out.astype(np.float32), f"{name}, device frame")
    # ... and so has a device frame with the host mask, which is uploaded
    up = t.apply(rp.to_device(image), mask=None if m is None else m.astype(np.int16) * 3, **_kwargs(name))
    mc.assert_same_bits(up.to_host(), out.astype(np.float32), f"{name}, device frame, host mask")


@pytest.mark.parametrize("name", ["nan_under", "pixel_last", "nonfinite"])
def test_float64_host_frames_get_their_own_bits_back_on_m2(name):
    _, shape, pad_mode, (dilation, width), threshold, fill_nonfinite, _ = mc.CASES[name]
    coords, k = _transfer(shape)
    image = mc.frame(name).astype(np.float64) + 1.0 / 3.0  # no finite pixel is a float32 number
    m = mc.mask(name)
    assert not np.array_equal(image, image.astype(np.float32).astype(np.float64), equal_nan=True)
    ref, inner = _definition(image.astype(np.float32), m, pad_mode, dilation, width, threshold, fill_nonfinite, coords, k)
    out = rp.ArrayPSFTransform(rp.IndexedCube(coords, k)).apply(image, mask=m, **_kwargs(name))
    _check(out, ref, inner, image, f"{name}, float64")
    finite = inner & np.isfinite(image)
    assert finite.any() and np.array_equal(out[finite].view(np.uint64), image[finite].view(np.uint64))


def test_apply_batch_with_masks_is_the_loop_bit_for_bit():
    mc.batch_precondition()
    pad_mode, (dilation, width), threshold, fill_nonfinite = mc.BATCH_SETTINGS
    coords, k = _transfer(mc.ODD)
    frames = [mc.frame(name) for name in mc.BATCH]
    masks = [mc.mask(name) for name in mc.BATCH]
    kwargs = dict(pad_mode=pad_mode, saturation_threshold=threshold, saturation_dilation=dilation, neighborhood_width=width)
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    loop = np.stack([t.apply(im, mask=m, **kwargs) for im, m in zip(frames, masks)])
    for f, (im, m) in enumerate(zip(frames, masks)):
        ref, inner = _definition(im, m, pad_mode, dilation, width, threshold, fill_nonfinite, coords, k)
        _check(loop[f], ref, inner, im, f"batch frame {f}")
    assert np.array_equal(t.apply_batch(frames, mask=masks, **kwargs), loop, equal_nan=True)
    assert np.array_equal(t.apply_batch(np.stack(frames), mask=np.stack(masks), dtype=np.float32, **kwargs), loop.astype(np.float32), equal_nan=True)
    shared = np.stack([t.apply(im, mask=masks[0], **kwargs) for im in frames])
    assert np.array_equal(t.apply_batch(frames, mask=masks[0], **kwargs), shared, equal_nan=True)
    stack = rp.to_device(np.stack(frames))
    dev = t.apply_batch(stack, mask=rp.to_device(np.stack(masks).astype(np.uint8)), dtype=np.float32, **kwargs)
    assert t.last_route & _native.ROUTE_SATURATED
    assert np.array_equal(dev.to_host(), loop.astype(np.float32), equal_nan=True)
    dev = t.apply_batch(stack, mask=[rp.to_device(m.astype(np.uint8)) for m in masks], dtype=np.float32, **kwargs)
    assert np.array_equal(dev.to_host(), loop.astype(np.float32), equal_nan=True)
    dev = t.apply_batch(stack, mask=masks[0], dtype=np.float32, **kwargs)
    assert np.array_equal(dev.to_host(), shared.astype(np.float32), equal_nan=True)


# ------------------------------------------------------------------------------------------------ 4: what users care about
def test_one_nan_no_longer_poisons_its_patches():
    h, w = mc.ODD
    coords, k = _transfer(mc.ODD)
    image = mc.sc.background(h, w, 31)
    image[h // 2, w // 2] = np.nan
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    poisoned = t.apply(image)
    assert np.isnan(poisoned).sum() > N * N / 4, "today's behaviour: a block of NaN"
    out = t.apply(image, fill_nonfinite=True)
    bad = ~np.isfinite(out)
    assert bad.sum() == 1 and bad[h // 2, w // 2] and np.isnan(out[h // 2, w // 2])
    for frames in ([image, image], rp.to_device(np.stack([image, image]))):
        batch = np.asarray(t.apply_batch(frames, fill_nonfinite=True))
        assert np.array_equal(~np.isfinite(batch), np.stack([bad, bad]))


# ------------------------------------------------------------------------------------------------ 5: a mask equal to the dilated hot mask
@pytest.mark.parametrize("pad_mode", mc.INDEX_MAP_MODES)
@pytest.mark.parametrize("dilation", [1, 2])
def test_a_threshold_and_the_mask_it_makes_give_the_same_bits(pad_mode, dilation):
    from scipy.ndimage import binary_dilation

    h, w = mc.ODD
    coords, k = _transfer(mc.ODD)
    image = mc.sc.background(h, w, 32)
    for r, c in ((9, 11), (18, 25), (27, 38)):
        image[r, c] = mc.HOT
    image[20:23, 30:34] = mc.HOT
    hot = image > mc.THRESHOLD
    m = binary_dilation(hot, iterations=dilation)
    assert np.array_equal(np.pad(m, 2 * N, mode=pad_mode), binary_dilation(np.pad(hot, 2 * N, mode=pad_mode), iterations=dilation)), \
        "padding the dilated mask is dilating the padded mask"
    for saturation in ("device", "host"):
        t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k), saturation=saturation)
        want = t.apply(image, pad_mode=pad_mode, saturation_threshold=mc.THRESHOLD, saturation_dilation=dilation)
        got = t.apply(image, pad_mode=pad_mode, saturation_threshold=math.inf, saturation_dilation=dilation, mask=m)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), saturation
        assert np.array_equal(got[m], image[m].astype(np.float64))


# ------------------------------------------------------------------------------------------------ 6: the defaults change nothing
@pytest.mark.parametrize("threshold", [math.inf, mc.THRESHOLD])
@pytest.mark.parametrize("saturation", ["host", "device"])
def test_explicit_defaults_take_the_same_route_and_give_the_same_bits(threshold, saturation):
    h, w = mc.QUADS
    coords, k = _transfer(mc.QUADS)
    image = mc.sc.background(h, w, 33)
    image[h // 2, w // 2] = image[3, 4] = mc.HOT
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k), saturation=saturation)
    kwargs = dict(saturation_threshold=threshold, saturation_dilation=2, neighborhood_width=5)
    off = dict(mask=None, fill_nonfinite=False)
    stack = np.stack([image, image[::-1].copy(), np.minimum(image, 500.0)])
    for frame in (image, image.astype(np.float64) + 1.0 / 3.0):
        t.last_route = -1
        want = t.apply(frame, **kwargs)
        route = t.last_route
        t.last_route = -1
        got = t.apply(frame, **kwargs, **off)
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint64), want.view(np.uint64)) and t.last_route == route
    dev = rp.to_device(image)
    want = t.apply(dev, **kwargs)
    route = t.last_route
    t.last_route = -1
    got = t.apply(dev, **kwargs, **off)
    assert t.last_route == route and bool(route & _native.ROUTE_SATURATED) == math.isfinite(threshold)
    assert np.array_equal(got.to_host().view(np.uint32), want.to_host().view(np.uint32))
    want = t.apply_batch(stack, **kwargs)
    info = t._device_plan().saturation_batch_info()
    got = t.apply_batch(stack, **kwargs, **off)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and t._device_plan().saturation_batch_info() == info
    want = t.apply_batch(rp.to_device(stack), dtype=np.float32, **kwargs)
    route = t.last_route
    t.last_route = -1
    got = t.apply_batch(rp.to_device(stack), dtype=np.float32, **kwargs, **off)
    assert t.last_route == route and np.array_equal(got.to_host().view(np.uint32), want.to_host().view(np.uint32))


def test_a_null_mask_at_the_c_abi_is_the_unmasked_entry_point():
    name = "pixel_last"
    _, shape, pad_mode, (dilation, width), threshold, _, _ = mc.CASES[name]
    plan = _native.Plan(N, [(0, 0)])
    mode = _native.PAD_MODES[pad_mode]
    want, want_mask, want_groups = plan.saturation_fill_batch_device([mc.frame(name)], mode, threshold, dilation, width, 2)
    got, got_mask, groups, _ = plan.saturation_fill_masked_device([mc.frame(name)], mode, threshold, dilation, width, None, False, 2)
    assert np.array_equal(got_mask, want_mask) and np.array_equal(groups, want_groups)
    mc.assert_same_bits(got[0], want[0], "no mask, no flag")


# ------------------------------------------------------------------------------------------------ 7: what the kernels do not cover
@pytest.mark.parametrize(("pad_mode", "dilation"), [("linear_ramp", 1), ("symmetric", 0)])
def test_other_pad_modes_and_dilations_take_the_numpy_steps_of_the_definition(pad_mode, dilation):
    name = "pixel_last"  # one masked pixel, one saturated pixel
    shape = mc.CASES[name][1]
    coords, k = _transfer(shape)
    image, m = mc.frame(name), mc.mask(name)
    ref, inner = _definition(image, m, pad_mode, dilation, 7, mc.THRESHOLD, False, coords, k) if dilation else (image.astype(np.float64), np.ones(shape, bool))
    if dilation == 0:  # scipy dilates until nothing changes: everything is masked and comes back as it went in
        from scipy.ndimage import binary_dilation

        assert binary_dilation(np.pad(image, 2 * N, mode=pad_mode) > mc.THRESHOLD, iterations=0).all()
    else:
        assert inner[-1, -1] and inner.sum() == 1 + 5, "the masked pixel and the dilated saturated one; no pad pixel is masked"
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    kwargs = dict(pad_mode=pad_mode, saturation_threshold=mc.THRESHOLD, saturation_dilation=dilation, mask=m)
    out = t.apply(image, **kwargs)
    if dilation:
        _check(out, ref, inner, image, f"{pad_mode}, dilation {dilation}")
    else:
        assert np.array_equal(out, ref)
    dev = t.apply(rp.to_device(image), **kwargs)
    assert isinstance(dev, rp.DeviceArray) and np.array_equal(dev.to_host(), out.astype(np.float32), equal_nan=True)
    dev = t.apply(rp.to_device(image), **{**kwargs, "mask": rp.to_device(m.astype(np.uint8))})
    assert np.array_equal(dev.to_host(), out.astype(np.float32), equal_nan=True)
