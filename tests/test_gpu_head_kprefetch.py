"""RPSF_OPT_HEAD_KPREFETCH: the head summing workgroups of a persistent 256-pixel launch touch the transfer kernel of the first round's
patches before they sum (csrc/rpsf_kernels2.hpp, prefetch_first_round_k), and a plan that lives on one stream records no event between its
applies (csrc/rpsf.hip, launch_apply).  Neither may change a bit of any result.

A launch has head summing workgroups from 512 patch-frames on (rpsf.hip, sum_first_for).  The 1024^2 and 2048^2 cases below (81 and 289
patches) stay under that: there the option must be inert.  The 2816^2 frame (529 patches: 8 head workgroups, 31 patch workgroups per XCD,
chunks of 67 slots, the last one of 60) and the batch of seven 1024^2 frames (567 patch-frames: chunks of 11 slots, the last one of 4,
against 31 queue positions = 5 slots per XCD in the first round) are the launches in which the phase really runs - more than one round in
the first, a slot list clipped by the chunk in the second."""

import numpy as np
import pytest

import regularizepsf_amd as rp
from oracle import regpsf_oracle as orc
from regularizepsf_amd import _native
from tests.helpers import rel_errors

pytestmark = pytest.mark.gpu
TOL = 1e-5
N = 256


def random_case(shape, seed):
    rng = np.random.default_rng(seed)
    coords = [tuple(int(v) for v in c) for c in rp.calculate_covering(shape, N)]
    k = np.empty((len(coords), N, N), np.complex64)
    k.real = rng.standard_normal(k.shape, dtype=np.float32)
    k.imag = rng.standard_normal(k.shape, dtype=np.float32)
    image = (rng.standard_normal(shape, dtype=np.float32) * 10 + 30).astype(np.float32)
    return coords, k, image


def plan_for(coords, k, option=None):
    plan = _native.Plan(N, coords)
    plan.set_transfer(k)
    if option is not None:
        plan.set_option("head_kprefetch", option)
    return plan


@pytest.fixture(scope="module")
def running():
    """The single frame in which the phase runs (2816^2, 529 patches), its plan and its result with the option off."""
    coords, k, image = random_case((2816, 2816), 31)
    plan = plan_for(coords, k, 0)
    return plan, image, plan.apply(image, 1)


def test_option_is_validated_and_ignored_by_other_plans():
    coords = [tuple(int(v) for v in c) for c in rp.calculate_covering((512, 512), 128)]
    plan = _native.Plan(128, coords)
    plan.set_option("head_kprefetch", 1)
    plan.set_option("head_kprefetch", 0)
    with pytest.raises(_native.NativeError):
        plan.set_option("head_kprefetch", 3)


def test_fewer_patches_than_resident_workgroups():
    h = w = 1024
    coords, k = orc.synthetic_transfer(h, w, N, alpha=3.0, epsilon=0.1)
    assert len(coords) == 81
    image = orc.starfield(h, w, seed=3)
    on = plan_for(coords, k, 1).apply(image, 1)
    off = plan_for(coords, k, 0).apply(image, 1)
    assert np.array_equal(on, off)
    rel_max, rel_l2 = rel_errors(on, orc.apply_transfer(image, coords, k))
    print(f"1024^2, option on against the oracle: max|d|/max|ref| = {rel_max:.3e}, rel-L2 = {rel_l2:.3e}")
    assert rel_max <= TOL and rel_l2 <= TOL


def test_more_than_one_round():
    coords, k, image = random_case((2048, 2048), 5)
    assert len(coords) == 289
    plan = plan_for(coords, k)  # (the default: off)
    off = plan.apply(image, 1)
    plan.set_option("head_kprefetch", 1)
    assert np.array_equal(plan.apply(image, 1), off)
    plan.set_option("head_kprefetch", 0)
    assert np.array_equal(plan.apply(image, 1), off)


def test_more_than_one_round_with_head_workgroups(running):
    plan, image, off = running
    assert plan.n_patches == 529
    plan.set_option("head_kprefetch", 1)
    on = plan.apply(image, 1)
    plan.set_option("head_kprefetch", 0)
    assert np.array_equal(on, off)


@pytest.mark.parametrize("overlap", [False, True])
def test_row_bands(overlap):
    """Two bands of a 2048^2 frame as ShardedApply cuts them: the second one starts neither at image row 0 nor at output row 0; with
    overlap=True every band with spill rows is two plans (its last lattice row on a stream of its own)."""
    from regularizepsf_amd.sharding import ShardedApply

    h = w = 2048
    coords, k, image = random_case((h, w), 9)
    got = {}
    for option in (1, 0):
        for rank in range(2):
            sh = ShardedApply(coords, lambda idx: k[idx], N, h, w, rank, 2, 0, None, overlap=overlap)
            b = sh.band
            if rank == 1:
                assert b.image_row0 > 0 and b.out_row0 > 0
            for plan in (sh.plan, sh.seam_plan):
                if plan is not None:
                    plan.set_option("head_kprefetch", option)
            sh.upload_rows(image[b.image_row0 : b.image_row0 + b.image_rows])
            sh.step()
            got[option, rank] = (sh.owned_rows(), sh.spill_rows())
    for rank in range(2):
        assert np.array_equal(got[1, rank][0], got[0, rank][0]) and np.array_equal(got[1, rank][1], got[0, rank][1])


@pytest.mark.parametrize("frames", [2, 7])
def test_batch(frames):
    """apply_batch_device, 1024^2 frames sharing one K: two frames (the issue's case; no head workgroups) and seven (567 patch-frames: the
    phase runs, on the position-to-slot rule of frames side by side)."""
    h = w = 1024
    coords, k, _ = random_case((h, w), 13)
    rng = np.random.default_rng(14)
    stack = (rng.standard_normal((frames, h, w), dtype=np.float32) * 10 + 30).astype(np.float32)
    d_in = _native.DeviceBuffer(stack.nbytes).upload(stack)
    d_out = _native.DeviceBuffer(stack.nbytes)
    geom = _native.Geometry.whole(h, w, 1)
    outs = []
    for option in (1, 0):
        plan = plan_for(coords, k, option)
        plan.apply_batch_device(d_in.ptr, d_out.ptr, frames, h * w, h * w, geom)
        plan.synchronize()
        outs.append(d_out.download((frames, h, w)))
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0][frames - 1], plan_for(coords, k, 0).apply(stack[frames - 1], 1))


def test_counters_survive_the_option_being_flipped(running):
    """Five applies back to back on one plan, the option on, off, on, on, off: a prefetch pass that drew from a queue or moved an epoch
    would leave the never-reset counters (slot queues, tile queue, tile counters) out of step with the host's accounting for the next one."""
    plan, image, off = running
    for option in (1, 0, 1, 1, 0):
        plan.set_option("head_kprefetch", option)
        assert np.array_equal(plan.apply(image, 1), off)


def test_two_streams():
    """One plan applied alternately on two streams of the caller's, twenty times, two frames in turn, nothing waited for in between: an apply
    on another stream than the previous one waits for that one (include/rpsf.h) - the plan's scratch serves one apply at a time.  Then one
    more on the plan's own stream."""
    h = w = 1024
    coords, k, image = random_case((h, w), 21)
    images = [image, image[::-1].copy() + 3]
    plan = plan_for(coords, k)
    want = [plan.apply(im, 1) for im in images]  # (single stream)
    geom = _native.Geometry.whole(h, w, 1)
    d_in = [_native.DeviceBuffer(im.nbytes).upload(im) for im in images]
    d_out = [_native.DeviceBuffer(image.nbytes) for _ in range(21)]
    streams = [_native.Stream(), _native.Stream()]
    for i in range(20):
        plan.apply_device(d_in[i & 1].ptr, d_out[i].ptr, geom, streams[i & 1].ptr)
    plan.apply_device(d_in[0].ptr, d_out[20].ptr, geom)
    plan.synchronize()
    for i in range(21):
        assert np.array_equal(d_out[i].download((h, w)), want[i & 1]), f"apply {i}"
    for s in streams:
        s.close()
