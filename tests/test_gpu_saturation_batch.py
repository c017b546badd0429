"""The device saturation route for batches of frames on the GPU (csrc/saturation.hip, csrc/rpsf_core_saturation_batch.hpp; DESIGN.md
3.8 "Frame batches").

A batch shares launches, never data: every frame must come out with the bits the single-frame entry gives it (a frame-group of one on
the same driver, so the comparisons that decide are the independent ones).  The stacks of
tests/saturation_batch_cases.py are held against ``saturation_cases.reference_fill`` per frame and against the CPU emulator; the whole
route against ``rpsf_apply_device_saturated`` on a fresh plan, against ``saturation="host"`` and against the loop over ``apply``.
"""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from oracle import regpsf_oracle as orc
from regularizepsf_amd import _native
from tests import saturation_batch_cases as bc
from tests import saturation_cases as sc

pytestmark = pytest.mark.gpu
THRESHOLD = 2.0e4
FILLER = -11.0
ROUTE = [(16, (40, 48), "wrap", 1, 7), (32, (96, 128), "reflect", 2, 5), (64, (200, 192), "edge", 3, 2), (128, (300, 260), "constant", 1, 3),
         (256, (512, 640), "reflect", 1, 9), (24, (96, 120), "edge", 1, 7)]


def gpu_fill_batch(frames, n, pad_mode, dilation, width, order=0, group=0, plan=None):
    plan = plan or _native.Plan(n, [(0, 0)])
    plan.set_option("sat_group", group)
    padded, masks, groups = plan.saturation_fill_batch_device(frames, _native.PAD_MODES[pad_mode], sc.THRESHOLD, dilation, width, order=order)
    return padded, masks, groups, plan.saturation_batch_info()


def _gpu_single_groups(name):
    _, n, _, pad_mode, (dilation, width) = bc.STACKS[name]
    plan = _native.Plan(n, [(0, 0)])
    return lambda f: plan.saturation_fill_device(bc.stack(name)[f], _native.PAD_MODES[pad_mode], sc.THRESHOLD, dilation, width)[2]


def _frame(n, shape, seed=0):
    """tests/test_gpu_saturation.py's saturated frame: hot pixels in the corners, on the rim, in a cluster, at random, and the 4 x 5 blob."""
    h, w = shape
    rng = np.random.default_rng(n + seed)
    image = orc.starfield(h, w, seed=3 * n + seed).astype(np.float64)
    hot = [(0, 0), (h - 1, w - 1), (1, w // 2), (h // 2, 0), (h // 2, w // 2), (h // 2, w // 2 + 1), (h // 2 + 1, w // 2)]
    hot += [(int(r), int(c)) for r, c in zip(rng.integers(0, h, 12), rng.integers(0, w, 12))]
    for r, c in hot:
        image[r, c] = 5.0e4 + r + c
    image[h // 3 : h // 3 + 4, w // 3 : w // 3 + 5] = 7.0e4
    return image, hot


def _three_frames(n, shape, seed=0):
    """Three float32 frames, the middle one clipped below the threshold; and the hot pixels of the outer ones."""
    made = [_frame(n, shape, seed=seed + s) for s in (1, 2, 3)]
    frames = [m[0].astype(np.float32) for m in made]
    frames[1] = np.minimum(frames[1], np.float32(1.0e4))
    assert frames[0].max() > THRESHOLD > frames[1].max() and frames[2].max() > THRESHOLD
    return frames, [made[0][1], [], made[2][1]]


def _same_bits(a, b, what):
    sc.assert_same_bits(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32), what)


def _resident_single(plan, image, pad_mode, dilation, width):
    img = _native.DeviceBuffer(image.nbytes).upload(image)
    out = _native.DeviceBuffer(image.nbytes)
    try:
        masked = plan.apply_device_saturated(img.ptr, out.ptr, *image.shape, _native.PAD_MODES[pad_mode], THRESHOLD, dilation, width)
        plan.synchronize()
        return out.download(image.shape), masked
    finally:
        img.free()
        out.free()


def _resident_batch(plan, frames, pad_mode, dilation, width, in_filler=3, out_filler=5):
    """Frames H * W + 3 floats apart in, results H * W + 5 apart out: (results, masked counts); the floats between results must survive."""
    h, w = frames[0].shape
    flat, stride = bc._strided(frames, in_filler)
    out_stride = h * w + out_filler
    outs = np.full(len(frames) * out_stride, FILLER, np.float32)
    img = _native.DeviceBuffer(flat.nbytes).upload(flat)
    out = _native.DeviceBuffer(outs.nbytes).upload(outs)
    try:
        masked = plan.apply_batch_device_saturated(img.ptr, out.ptr, len(frames), stride, out_stride, h, w, _native.PAD_MODES[pad_mode], THRESHOLD,
                                                   dilation, width)
        plan.synchronize()
        rows = out.download((len(frames), out_stride))
    finally:
        img.free()
        out.free()
    assert (rows[:, h * w :] == FILLER).all(), "the filler words between two frames of outs_dev are untouched"
    return rows[:, : h * w].reshape(len(frames), h, w).copy(), masked


# ------------------------------------------------------------------------------------------------ 1 - 4, 6: F1 - F4 of a stack
@pytest.mark.parametrize("name", ["kinds_wrap", "kinds_edge", "odd_stride", "same_layout", "around_fully_hot"])
def test_every_frame_of_a_stack_has_the_bits_of_its_own_reference_and_of_the_emulator(name):
    bc.precondition(name)
    got = bc.run_stack(gpu_fill_batch, name)
    bc.check_against_reference(got, name, single_groups=_gpu_single_groups(name))
    assert got[3][1] == 1
    bc.check_same_results(got, bc.run_stack(bc.emu_fill_batch, name), "GPU against the emulator")


def test_a_batch_in_which_nothing_is_hot_has_no_groups_and_launches_no_fill():
    bc.precondition("nothing_hot")
    _, n, _, pad_mode, (dilation, width) = bc.STACKS["nothing_hot"]
    plan = _native.Plan(n, [(0, 0)])
    got = gpu_fill_batch(bc.stack("nothing_hot"), n, pad_mode, dilation, width, plan=plan)
    bc.check_against_reference(got, "nothing_hot")
    assert got[3] == (3, 1, 0, 0)
    ms = plan.saturation_kernel_ms()
    assert ms[0] > 0 and (ms[1:4] == 0).all(), "F4 is not launched"


def test_the_cut_into_frame_groups_changes_no_bit():
    bc.precondition("the_cut")
    whole = bc.run_stack(gpu_fill_batch, "the_cut", group=0)
    bc.check_against_reference(whole, "the_cut")
    assert whole[3][1] == 1
    for group, frame_groups in ((1, 5), (2, 3)):
        cut = bc.run_stack(gpu_fill_batch, "the_cut", group=group)
        bc.check_same_results(cut, whole, f"frame-groups of {group}")
        assert cut[3] == (5, frame_groups, whole[3][2], whole[3][3])
    bc.check_same_results(whole, bc.run_stack(bc.emu_fill_batch, "the_cut", group=2), "GPU against the emulator")
    plan = _native.Plan(16, [(0, 0)])
    for bad in (-1, 65536):
        with pytest.raises(_native.NativeError, match="RPSF_OPT_SAT_GROUP") as err:
            plan.set_option("sat_group", bad)
        assert err.value.code == _native.E_BADARG


def test_the_order_in_which_f4_takes_the_groups_changes_no_bit():
    bc.precondition("order")
    longest_first = bc.run_stack(gpu_fill_batch, "order")
    bc.check_against_reference(longest_first, "order")
    for order in (bc.ORDER_REVERSED, bc.ORDER_FRAMES):
        bc.check_same_results(bc.run_stack(gpu_fill_batch, "order", order=order), longest_first, f"order {order}")
    bc.check_same_results(longest_first, bc.run_stack(bc.emu_fill_batch, "order"), "GPU against the emulator")


# ------------------------------------------------------------------------------------------------ 7: the whole route, resident
@pytest.mark.parametrize(("n", "shape", "other_mode", "dilation", "width"), ROUTE)
def test_resident_batch_has_the_single_entrys_and_the_host_routes_bits(n, shape, other_mode, dilation, width):
    coords, k = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)
    frames, hots = _three_frames(n, shape)
    host = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    single = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))._device_plan()  # (never sees a batch)
    batch = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))._device_plan()
    for pad_mode in ("symmetric", other_mode):
        outs, masked = _resident_batch(batch, frames, pad_mode, dilation, width)
        assert batch.saturation_batch_info()[:2] == (3, 1)
        kwargs = dict(pad_mode=pad_mode, saturation_threshold=THRESHOLD, saturation_dilation=dilation, neighborhood_width=width)
        for f, image in enumerate(frames):
            what = f"N = {n}, {pad_mode}, frame {f}"
            want, want_masked = _resident_single(single, image, pad_mode, dilation, width)
            _same_bits(outs[f], want, what + ": the single entry")
            assert masked[f] == want_masked, what
            _same_bits(outs[f], host.apply(image, **kwargs), what + ': saturation="host"')
            for r, c in hots[f]:
                assert outs[f][r, c] == image[r, c]
        assert masked[0] > 20 and masked[1] == 0 and masked[2] > 20


# ------------------------------------------------------------------------------------------------ 8: apply_batch
def test_apply_batch_takes_the_batch_route_and_is_the_loop_bit_for_bit():
    n, shape = 32, (96, 128)
    coords, k = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)
    stack32, _ = _three_frames(n, shape)
    stack64 = [_frame(n, shape, seed=s)[0] + 1.0 / 3.0 for s in (1, 2, 3)]  # no pixel is a float32 number
    stack64[1] = np.minimum(stack64[1], 1.0e4)
    stack64[2][shape[0] // 4, shape[1] // 4] = np.nan
    assert all(not np.array_equal(f, f.astype(np.float32).astype(np.float64)) for f in stack64)
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k), saturation="device")
    kwargs = dict(saturation_threshold=THRESHOLD, saturation_dilation=2, neighborhood_width=5)
    from scipy.ndimage import binary_dilation

    for stack in (stack32, stack64):
        before = [f.copy() for f in stack]
        loop = np.stack([t.apply(im, **kwargs) for im in stack])
        t._device_plan().apply_frames_host_saturated_device([], 1, THRESHOLD, 2, 5)  # zero frames: the info is cleared
        assert t._device_plan().saturation_batch_info() == (0, 0, 0, 0)
        got = t.apply_batch(stack, **kwargs)
        info = t._device_plan().saturation_batch_info()
        assert info[0] == len(stack) and info[1] == 1, "one host wait for all frames: the loop has gone"
        assert got.dtype == np.float64 and np.array_equal(got, loop, equal_nan=True)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(stack, before))
        assert np.array_equal(t.apply_batch(np.stack(stack), dtype=np.float32, **kwargs), loop.astype(np.float32), equal_nan=True)
        for f, im in enumerate(stack):
            mask = binary_dilation(np.nan_to_num(np.asarray(im, np.float64)) > THRESHOLD, iterations=2)  # at least these
            assert np.array_equal(got[f][mask], np.asarray(im, np.float64)[mask]), "masked pixels carry the caller's own values"
        assert got[0][shape[0] // 3, shape[1] // 3] == stack[0][shape[0] // 3, shape[1] // 3]
    # always-empty windows and dilations below one: today's routes, untouched by the batch entry
    host = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    for dilation, width in ((1, 1), (0, 7)):
        kw = dict(saturation_threshold=THRESHOLD, saturation_dilation=dilation, neighborhood_width=width)
        assert np.array_equal(t.apply_batch(stack32[:2], **kw), host.apply_batch(stack32[:2], **kw), equal_nan=True), (dilation, width)
        assert t._device_plan().saturation_batch_info()[0] == 3, "no batch call was made"


# ------------------------------------------------------------------------------------------------ 9: reuse
def test_batches_and_single_frames_share_one_plans_scratch():
    n, shape, larger = 32, (96, 128), (112, 152)
    coords, k = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)  # (its corners are valid for the larger frame too)
    two = _three_frames(n, shape)[0][:2][::-1]
    five = [_frame(n, larger, seed=s)[0].astype(np.float32) for s in (4, 5, 6, 7, 8)]
    five[3] = np.minimum(five[3], np.float32(1.0e4))

    def fresh():
        return rp.ArrayPSFTransform(rp.IndexedCube(coords, k))._device_plan()

    want_two = _resident_batch(fresh(), two, "symmetric", 2, 5)
    want_five = _resident_batch(fresh(), five, "reflect", 1, 7)
    want_one = _resident_single(fresh(), five[0], "reflect", 1, 7)
    plan = fresh()
    steps = [("a batch of 2", two, "symmetric", 2, 5, want_two), ("a batch of 5 of a larger shape", five, "reflect", 1, 7, want_five),
             ("the first batch again", two, "symmetric", 2, 5, want_two), None, ("the first batch once more", two, "symmetric", 2, 5, want_two)]
    for step in steps:
        if step is None:
            got, masked = _resident_single(plan, five[0], "reflect", 1, 7)
            _same_bits(got, want_one[0], "a single frame between batches")
            assert masked == want_one[1] and plan.saturation_batch_info()[0] == 2, "the single entry leaves the batch info alone"
            continue
        what, frames, pad_mode, dilation, width, want = step
        got, masked = _resident_batch(plan, frames, pad_mode, dilation, width)
        for f in range(len(frames)):
            _same_bits(got[f], want[0][f], f"{what}, frame {f}")
        assert np.array_equal(masked, want[1]), what
        assert plan.saturation_batch_info()[:2] == (len(frames), 1)
    for f, image in enumerate(five):  # and the batch of 5 is the single entry five times
        _same_bits(want_five[0][f], _resident_single(plan, image, "reflect", 1, 7)[0], f"frame {f} alone")


# ------------------------------------------------------------------------------------------------ 10: one frame, no frame, bad arguments
def test_one_frame_no_frame_and_bad_arguments():
    n, shape = 32, (96, 128)
    coords, k = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)
    image = _frame(n, shape)[0].astype(np.float32)
    plan = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))._device_plan()
    want, want_masked = _resident_single(rp.ArrayPSFTransform(rp.IndexedCube(coords, k))._device_plan(), image, "symmetric", 1, 7)
    got, masked = _resident_batch(plan, [image], "symmetric", 1, 7, in_filler=0, out_filler=1)
    _same_bits(got[0], want, "n_frames = 1")
    assert list(masked) == [want_masked] and plan.saturation_batch_info()[:2] == (1, 1)
    lib, handle = _native.lib(), plan._handle
    buf = _native.DeviceBuffer(image.nbytes).upload(image)
    out = _native.DeviceBuffer(image.nbytes).upload(np.full(shape, FILLER, np.float32))
    h, w = shape
    try:
        def call(images, outs, frames, stride=h * w, dilation=1, width=7, pad_mode=1, height=h, handle=handle):
            return lib.rpsf_apply_batch_device_saturated(handle, images, outs, frames, stride, stride, height, w, pad_mode, THRESHOLD, dilation, width,
                                                         None, None)

        assert call(buf.ptr, out.ptr, 0) == 0 and call(None, None, 0) == 0
        plan.synchronize()
        assert plan.saturation_batch_info() == (0, 0, 0, 0)
        assert (out.download(shape) == FILLER).all(), "n_frames = 0 does nothing"
        assert call(None, out.ptr, 1) == _native.E_BADARG and call(buf.ptr, None, 1) == _native.E_BADARG
        assert call(buf.ptr, out.ptr, 1, handle=None) == _native.E_BADARG and call(buf.ptr, out.ptr, 0, handle=None) == _native.E_BADARG
        assert call(buf.ptr, out.ptr, -1) == _native.E_BADARG
        assert call(buf.ptr, out.ptr, 2, stride=h * w - 1) == _native.E_BADARG
        assert call(buf.ptr, out.ptr, 1, width=1) == _native.E_BADARG and call(buf.ptr, out.ptr, 1, dilation=0) == _native.E_BADARG
        assert call(buf.ptr, out.ptr, 1, pad_mode=5) == _native.E_BADARG and call(buf.ptr, out.ptr, 1, height=0) == _native.E_BADARG
        bare = _native.Plan(n, coords)  # no transfer kernel yet
        assert call(buf.ptr, out.ptr, 1, handle=bare._handle) == _native.E_STATE
        info = (ctypes.c_int * 4)()
        assert lib.rpsf_saturation_batch_info(None, info) == _native.E_BADARG and lib.rpsf_saturation_batch_info(handle, None) == _native.E_BADARG
        ptrs = (ctypes.c_void_p * 1)(image.ctypes.data)
        assert lib.rpsf_apply_frames_host_saturated_device(handle, ptrs, 0, 0, h, w, 1, THRESHOLD, 1, 7, ptrs, 0) == 0
        assert lib.rpsf_apply_frames_host_saturated_device(handle, None, 0, 1, h, w, 1, THRESHOLD, 1, 7, ptrs, 0) == _native.E_BADARG
        assert lib.rpsf_apply_frames_host_saturated_device(handle, ptrs, 0, 1, h, w, 1, THRESHOLD, 1, 1, ptrs, 0) == _native.E_BADARG
        null = (ctypes.c_void_p * 1)(None)
        assert lib.rpsf_apply_frames_host_saturated_device(handle, null, 0, 1, h, w, 1, THRESHOLD, 1, 7, ptrs, 0) == _native.E_BADARG
        assert (out.download(shape) == FILLER).all(), "a refused call writes nothing"
    finally:
        buf.free()
        out.free()


# ------------------------------------------------------------------------------------------------ 11: a single frame is a frame-group of one
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_the_single_frame_entry_is_a_frame_group_of_one_in_table_order(name):
    _, n, _, pad_mode, (dilation, width) = sc.CASES[name]
    mode = _native.PAD_MODES[pad_mode]
    plan = _native.Plan(n, [(0, 0)])
    single, mask, groups = plan.saturation_fill_device(sc.frame(name), mode, sc.THRESHOLD, dilation, width)
    padded, masks, per_frame = plan.saturation_fill_batch_device([sc.frame(name)], mode, sc.THRESHOLD, dilation, width, order=bc.ORDER_FRAMES)
    assert np.array_equal(masks[0].astype(bool), mask) and list(per_frame) == [groups]
    sc.assert_same_bits(np.ascontiguousarray(padded[0]), single, f"{name}: a batch of one in table order")
    backward, backward_mask, backward_groups = plan.saturation_fill_device(sc.frame(name), mode, sc.THRESHOLD, dilation, width, reverse_groups=True)
    assert np.array_equal(backward_mask, mask) and backward_groups == groups
    sc.assert_same_bits(backward, single, f"{name}: groups taken last first")


def test_single_frame_calls_leave_the_batch_info_as_it_was():
    n, shape = 16, (40, 48)
    coords, k = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)
    frames, _ = _three_frames(n, shape)
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k), saturation="device")
    plan = t._device_plan()
    _resident_batch(plan, frames, "symmetric", 1, 7)
    info = plan.saturation_batch_info()
    assert info[:2] == (3, 1) and info[2] > 0 and info[3] > 20
    plan.saturation_fill_device(frames[0], _native.PAD_MODES["symmetric"], THRESHOLD, 1, 7)
    assert plan.saturation_batch_info() == info, "saturation_fill_device"
    _resident_single(plan, frames[2], "symmetric", 1, 7)
    assert plan.saturation_batch_info() == info, "apply_device_saturated"
    t.apply(frames[0], saturation_threshold=THRESHOLD, saturation_dilation=1, neighborhood_width=7)
    assert t._device_plan() is plan and plan.saturation_batch_info() == info, 'apply(..., saturation="device")'
