"""Bad-pixel masks of apply without a GPU ("Bad-pixel masks"): the masked variants of kernel F1 and of F2's last pass
on the CPU lane emulator (tests/emu/emu_mask.cpp) against the NumPy / SciPy definition and the host route's fill, the batch drivers
against the single-frame functions, F5 behind them, and the argument checks of ``mask=`` / ``fill_nonfinite=``, which run before any
GPU work.
"""

import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, transform
from regularizepsf_amd.device_array import DeviceArray
from tests import mask_cases as mc

BASE = 0x7F0000000000  # a device address nobody dereferences: these tests stop before the GPU


# ------------------------------------------------------------------------------------------------ 1: the emulator against the definition
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_emulator_gives_m2_the_reference_fill_and_the_counts(name):
    mc.precondition(name)
    want, m2, hot, exact, _ = mc.reference(name)
    got, got_mask, (n_hot, n_exact, n_masked, groups) = mc.emulated(name)
    assert np.array_equal(got_mask, m2)
    mc.assert_same_bits(got, want.astype(np.float32), name)
    assert (n_hot, n_exact) == (hot.sum(), exact.sum())
    assert n_masked == (m2.sum() if m2.any() else 0) and (groups == 0) == (not m2.any())


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_batch_drivers_give_the_single_frame_bits(name):
    _, _, pad_mode, (dilation, width), threshold, fill_nonfinite, storage = mc.CASES[name]
    m = mc.stored(mc.mask(name), storage)
    one, one_mask, one_counts = mc.emulated(name)
    # the frame three times: a per-frame stack of masks, then one shared mask, in two orders of F4
    frames = [mc.frame(name)] * 3
    for masks, order in ((None if m is None else np.stack([m] * 3), 0), (None if m is None else m[None], 2)):
        padded, masks_out, counts = mc.emu_fill_batch(frames, masks, mc.N, pad_mode, dilation, width, threshold, fill_nonfinite, order)
        for f in range(3):
            assert np.array_equal(masks_out[f], one_mask) and tuple(counts[f]) == one_counts
            mc.assert_same_bits(padded[f], one, f"{name}, frame {f}")


def test_an_idle_frame_between_two_busy_ones():
    mc.batch_precondition()
    pad_mode, (dilation, width), threshold, fill_nonfinite = mc.BATCH_SETTINGS
    frames = [mc.frame(name) for name in mc.BATCH]
    masks = np.stack([mc.stored(mc.mask(name), "dense") for name in mc.BATCH])
    padded, masks_out, counts = mc.emu_fill_batch(frames, masks, mc.N, pad_mode, dilation, width, threshold, fill_nonfinite)
    for f, (want, m2, hot, exact, _) in enumerate(mc.batch_reference()):
        assert np.array_equal(masks_out[f], m2)
        mc.assert_same_bits(padded[f], want.astype(np.float32), mc.BATCH[f])
        assert tuple(counts[f][:3]) == (hot.sum(), exact.sum(), m2.sum())
        single, single_mask, single_counts = mc.emu_fill(frames[f], masks[f], mc.N, pad_mode, dilation, width, threshold, fill_nonfinite)
        assert np.array_equal(single_mask, m2) and single_counts == tuple(counts[f])
        mc.assert_same_bits(padded[f], single, f"{mc.BATCH[f]} alone")
    assert tuple(counts[1]) == (0, 0, 0, 0)


def test_restore_puts_the_raw_values_on_m2_and_lists_them():
    pad_mode, (dilation, width), threshold, fill_nonfinite = mc.BATCH_SETTINGS
    frames = [mc.frame(name) for name in mc.BATCH]
    masks = np.stack([mc.stored(mc.mask(name), "dense") for name in mc.BATCH])
    h, w = mc.ODD
    rng = np.random.default_rng(5)
    corrected = rng.normal(size=(3, h, w + 4 * mc.N)).astype(np.float32)  # rows 2N ... 2N + H of the padded frame
    outs, lists = mc.emu_restore_batch(frames, masks, mc.N, pad_mode, dilation, width, threshold, fill_nonfinite, corrected, 2 * mc.N)
    for f, (_, m2, *_) in enumerate(mc.batch_reference()):
        inner = m2[2 * mc.N : 2 * mc.N + h, 2 * mc.N : 2 * mc.N + w]
        want = np.where(inner, frames[f], corrected[f][:, 2 * mc.N : 2 * mc.N + w])
        assert np.array_equal(outs[f], want)
        assert np.array_equal(lists[f], np.flatnonzero(inner))


def test_a_null_mask_without_fill_nonfinite_is_the_unmasked_fill():
    from tests import saturation_cases as sc

    name = "corners_edges"
    _, n, _, pad_mode, (dilation, width) = sc.CASES[name]
    want, want_mask, groups = sc.emu_fill(sc.frame(name), n, pad_mode, dilation, width)
    got, got_mask, counts = mc.emu_fill(sc.frame(name), None, n, pad_mode, dilation, width, sc.THRESHOLD, False)
    assert np.array_equal(got_mask, want_mask) and counts[3] == groups and counts[1] == 0
    mc.assert_same_bits(got, want, name)


# ------------------------------------------------------------------------------------------------ 8: arguments, before the GPU
def _transform():
    k = np.ones((1, 16, 16), np.complex64)
    return rp.ArrayPSFTransform(rp.IndexedCube([(0, 0)], k))


def test_the_keywords_exist_are_keyword_only_and_default_to_off():
    for method in (rp.ArrayPSFTransform.apply, rp.ArrayPSFTransform.apply_batch):
        params = inspect.signature(method).parameters
        assert params["mask"].default is None and params["mask"].kind is inspect.Parameter.KEYWORD_ONLY
        assert params["fill_nonfinite"].default is False and params["fill_nonfinite"].kind is inspect.Parameter.KEYWORD_ONLY
    for symbol in ("rpsf_apply_batch_device_masked", "rpsf_apply_view_masked", "rpsf_apply_batch_view_masked",
                   "rpsf_apply_frames_host_masked_device", "rpsf_saturation_fill_masked_device"):
        assert hasattr(_native.lib(), symbol)


def test_shape_count_dtype_and_mixed_errors_are_raised_before_the_gpu_is_touched():
    t = _transform()
    host = np.zeros((40, 48), np.float32)
    dev = DeviceArray._from_parts(BASE, (40, 48), np.float32)
    dev_stack = DeviceArray._from_parts(BASE, (3, 40, 48), np.float32)
    good = DeviceArray._from_parts(BASE, (40, 48), np.uint8)
    for frame in (host, dev):
        with pytest.raises(ValueError, match="mask must have the frame's shape"):
            t.apply(frame, mask=np.zeros((40, 47), bool))
        with pytest.raises(ValueError, match="mask must have the frame's shape"):
            t.apply(frame, mask=np.zeros((1, 40, 48), bool))
    with pytest.raises(ValueError, match="mask must have the frame's shape"):
        t.apply(dev, mask=DeviceArray._from_parts(BASE, (40, 50), np.uint8))
    for frames in ([host] * 3, np.zeros((3, 40, 48), np.float32), dev_stack, [dev] * 3):
        with pytest.raises(ValueError, match="2 masks for 3 frames"):
            t.apply_batch(frames, mask=np.zeros((2, 40, 48), bool))
        with pytest.raises(ValueError, match="mask must have the frame's shape"):
            t.apply_batch(frames, mask=np.zeros((3, 41, 48), bool))
    with pytest.raises(ValueError, match="2 masks for 3 frames"):
        t.apply_batch(dev_stack, mask=[good, good])
    for bad in (np.float32, np.int32, np.uint16):
        with pytest.raises(ValueError, match="a device mask must be uint8"):
            t.apply(dev, mask=DeviceArray._from_parts(BASE, (40, 48), bad))
        with pytest.raises(ValueError, match="a device mask must be uint8"):
            t.apply_batch(dev_stack, mask=DeviceArray._from_parts(BASE, (3, 40, 48), bad))
    with pytest.raises(ValueError, match="lives on device 3"):
        t.apply(dev, mask=DeviceArray._from_parts(BASE, (40, 48), np.uint8, device=3))
    for call in (lambda: t.apply(host, mask=good), lambda: t.apply_batch([host, host], mask=good), lambda: t.apply_batch([host, host], mask=[good, good]),
                 lambda: t.apply_batch(np.zeros((2, 40, 48)), mask=DeviceArray._from_parts(BASE, (2, 40, 48), np.uint8))):
        with pytest.raises(TypeError, match="a device mask goes with device frames"):
            call()
    with pytest.raises(ValueError, match="mixes host and device"):
        t.apply_batch([dev, dev], mask=[good, np.zeros((40, 48), bool)])


def test_masks_are_normalised_to_one_or_one_per_frame():
    shape = (40, 48)
    on_device, items = transform._check_masks(np.eye(40, 48, dtype=np.int16) * 7, shape, None, 0, False)
    assert not on_device and len(items) == 1 and items[0].dtype == bool and items[0].sum() == 40
    _, items = transform._check_masks([np.zeros(shape), np.ones(shape)], shape, 2, 0, False)
    assert len(items) == 2 and not items[0].any() and items[1].all()
    _, items = transform._check_masks(np.zeros(shape, np.uint8), shape, 5, 0, True)
    assert len(items) == 1
    pitched = DeviceArray._from_parts(BASE, (3, 40, 48), np.uint8, strides=(40 * 128, 128, 2))
    on_device, items = transform._check_masks(pitched, shape, 3, 0, True)
    assert on_device and [m.ptr for m in items] == [BASE + i * 40 * 128 for i in range(3)] and all(m.strides == (128, 2) for m in items)
    view = transform._mask_view(items[1])
    assert (view.data, view.dtype, view.rows, view.cols, view.row_stride, view.col_stride) == (BASE + 40 * 128, _native.DTYPES["|u1"], 40, 48, 128, 2)
    assert transform._check_masks(None, shape, None, 0, False) == (False, None)


def test_the_mask_follows_the_index_map_and_stays_out_of_other_pads():
    m = np.zeros((5, 6), bool)
    m[0, 0] = m[4, 2] = True
    for mode in ("symmetric", "reflect", "edge", "wrap"):
        assert np.array_equal(transform._pad_mask(m, m.shape, 2, mode), np.pad(m, 4, mode=mode))
    for mode in ("constant", "linear_ramp", "mean", "maximum"):
        padded = transform._pad_mask(m, m.shape, 2, mode)
        assert np.array_equal(padded[4:-4, 4:-4], m) and padded.sum() == 2
    assert not transform._pad_mask(None, m.shape, 2, "wrap").any()
