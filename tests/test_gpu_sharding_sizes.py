"""The sharded row-band step (regularizepsf_amd/sharding.py, ShardedApply) at every patch size, pad mode and seam form, on one GPU.

Every case of tests/sharding_cases.py runs as `world` ShardedApply objects in one process, in the four forms: two plans on two streams with
the seam patches run once (`overlap=True`), apply -> exchange -> add on one stream (`overlap=False`), the exchange of step k beside the launch
of step k + 1 (`overlap="pipeline"`), and `seam="recompute"`.  The transport is LocalSeam (a host mailbox); every add is K4
(`add_rows_kernel`) on the pointers the step hands it, `rows x width x 4` bytes into their allocations.  The stitched result is held to

  * the bound per neighbourhood of tests/test_gpu_local_parity.py (local error <= MARGIN = 4 x the float32 yardstick on six-decade frames, of
    which the rows a band receives are dim for a quarter at least) beside the global 1e-5 bar: a spill row added one row off, or a seam
    patch's upper rows dropped in a dim region, passes the global bar and not this one;
  * exact scaling: the steps f, 1024 f, f / 1024, f on the same objects go through both slots of every double buffer, and a seam or output
    buffer left over from two steps back is off by 2^20, with no tolerance to hide in;
  * fresh objects: three unrelated frames in a row give, bit for bit, what new ShardedApply objects give for each alone;
  * the whole-frame apply: `recompute` bands of the sweep kernel (N <= 64, coverings) equal one plan over the whole frame bit for bit.  The
    sweep kernel adds a pixel's contributions lattice row by lattice row top-down, even columns before odd ones (rpsf_plan3.hpp), whichever
    regions the lattice is cut into; a band's plan holds whole lattice rows of the same columns and every patch that reaches its own rows, so
    its order at those rows is the frame's.

The case of corners every 8 rows is no half-overlap lattice and adds with float atomics, in no fixed order: its four steps are each held to
the bound (a stale buffer is off by 2^10 at least there), not to bit-identity, as the atomic paths of tests/test_gpu_local_parity.py are.

What this does not show: LocalSeam waits for the whole device at every exchange (as bench.GlooSeam does), so an ordering race between
streams that nothing synchronizes stays with the two-process tests of tests/test_gpu_sharding.py and test_two_persistent_plans_on_two_streams;
and `rpsf_comm_seam_exchange` with a real RCCL peer is not run here at all.

K4 itself is run at counts 1 ... 4 x 256 x 64 + 5, on 1, 3, 64 and all workgroups, with `accum` and `src` each 0 ... 3 floats into their
allocations: the 16-byte body where both are aligned, the scalar loop elsewhere, against NumPy float32 bit for bit.

Measured on an MI355X (result / yardstick, min ... max over the cases of a patch size and the five pad modes; log:
profiles/sharding_sizes_gpu.log):

    form (coverings)             N = 16         32             64             128            256
    overlap (two plans, once)    0.72 ... 2.08  0.95 ... 1.46  1.10 ... 1.71  1.03 ... 1.62  0.91 ... 1.58
    sequence                     0.58 ... 1.90  0.90 ... 1.68  1.07 ... 1.54  1.03 ... 1.62  0.91 ... 1.58
    pipeline                     0.58 ... 1.90  0.90 ... 1.68  1.07 ... 1.54  1.03 ... 1.62  0.91 ... 1.58
    recompute                    0.58 ... 1.90  0.90 ... 1.68  1.07 ... 1.70  1.03 ... 1.62  0.91 ... 1.58
    corners every 8 rows, N = 32 (float atomics): overlap, sequence, pipeline 0.77 ... 1.58, recompute 0.77 ... 1.61
    covering with a hole, N = 32 (colour planes): overlap 1.00 ... 1.29, sequence, pipeline 0.96 ... 1.68, recompute 0.96 ... 1.29

Yardstick 8.7e-8 ... 3.3e-7, global max|d| / max|ref| 1.2e-7 ... 3.9e-7.  The stitched result carries one float32 addition more than a
whole-frame apply (partial sum + partial sum at the seam rows); the largest figure, 2.08 at N = 16 with two plans, is where it shows, and
it stays at half of MARGIN = 4.  Scaling, fresh-object and whole-frame identities hold bit for bit in every case they are asserted for.

Wrong versions of the step were run against this module once each (all in bounds).  Caught by the first test, in all 70 cases of each form
named: the K4 add of the seam patches' upper rows skipped (overlap); received rows added one row down with one row fewer (overlap, pipeline);
the spill sent from one row early (sequence, pipeline); `a.w += b.z` in K4 (overlap, sequence, pipeline, and 20 of the 28 K4 cases: every
count above 3); the upper-row add, or the pipelined send, reading slot 0 whatever the step wrote (overlap / pipeline, and the frame-by-frame
test).  The resident window of 'wrap' computed as for 'edge' is caught without a GPU by tests/test_sharding_cases.py (all 14 cases) and was
not run here: the kernels would read rows that are not resident.  NOT caught, and not catchable here: `d_seam[slot]` -> `d_seam[0]`
everywhere, and the pipeline's `slot = 0` always - with the device idle at every exchange one buffer is as good as two; what the second
buffer buys is freedom from a race (above).
"""

import functools

import numpy as np
import pytest

from tests.helpers import KERNEL_PAD_MODES, MARGIN, rel_errors
from tests.sharding_cases import CASES, FORMS, FRAME_CASES, band_plans, expected_branches, local_case, run_sharded, transfer

pytestmark = pytest.mark.gpu
TOL = 1e-5  # the global bar of the other modules, kept beside the local one
SCALES = (np.float32(1024.0), np.float32(1.0 / 1024.0))
CASE_IDS = [c.name for c in CASES]


def _pad(mode):
    from regularizepsf_amd import _native

    return _native.PAD_MODES[mode]


def _bound(lc, out, path):
    """Print the figures, then assert the global bar and the local bound."""
    out = np.asarray(out, np.float64)
    rel_max, rel_l2 = rel_errors(out, lc.ref)
    ratio = lc.ratio(out)
    print(f"LOCAL-RATIO | {path} | N={lc.n} {lc.shape[0]}x{lc.shape[1]} {lc.pad_mode} | dim share {lc.share:.2f} | "
          f"yardstick {lc.yardstick:.2e} | ratio {ratio:.2f} | global {rel_max:.1e}")
    assert rel_max <= TOL and rel_l2 <= TOL, (path, rel_max, rel_l2)
    lc.check(out, MARGIN, path)
    return ratio


def _where(out, expect):
    """Rows, columns and count of the pixels that differ (for the failure message)."""
    rows, cols = np.where(out != expect)
    if rows.size == 0:
        return "no pixel differs"
    return f"{rows.size} pixels differ, rows {rows.min()}..{rows.max()}, columns {cols.min()}..{cols.max()}"


@functools.lru_cache(maxsize=8)
def _whole_frame(case, mode):
    """The frame through one plan over the whole lattice (a fresh one), for the recompute bands of the sweep kernel."""
    from regularizepsf_amd import _native

    coords, k = transfer(case)
    plan = _native.Plan(case.n, coords)
    try:
        plan.set_transfer(k)
        assert plan.sweep_info()["regions"] > 0
        return plan.apply(local_case(case, mode).image, _pad(mode))
    finally:
        plan.close()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("mode", KERNEL_PAD_MODES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_bound_per_neighbourhood_and_exact_scaling(case, mode, form):
    lc = local_case(case, mode)
    f = lc.image
    outs, branches = run_sharded(case, mode, form, (f, SCALES[0] * f, SCALES[1] * f, f))
    path = f"sharded {form}, world {case.world}{'' if case.lattice == 'covering' else ', ' + case.lattice}"
    assert all(np.isfinite(o).all() for o in outs), path  # every owned row was written
    _bound(lc, outs[0], path)
    if case.ordered:
        for s, out in zip(SCALES, outs[1:3]):
            assert np.array_equal(out, s * outs[0]), (path, mode, float(s), _where(out, s * outs[0]))
        assert np.array_equal(outs[3], outs[0]), (path, mode, "the frame again", _where(outs[3], outs[0]))
    else:  # float atomics: the scaled steps brought back by the power of two (exact), each held to the bound
        for s, out in zip((*SCALES, np.float32(1.0)), outs[1:]):
            lc.check(np.asarray(out / s, np.float64), MARGIN, f"{path}, step scaled by {float(s)}")
    if form == "recompute" and case.n <= 64 and case.lattice == "covering":
        whole = _whole_frame(case, mode)
        assert np.array_equal(outs[0], whole), (path, mode, "whole-frame apply", _where(outs[0], whole))
    assert branches == expected_branches(case, mode, form), (path, mode)


@pytest.mark.parametrize("form", ["overlap", "pipeline"])
@pytest.mark.parametrize("case", FRAME_CASES, ids=[c.name for c in FRAME_CASES])
def test_unrelated_frames_step_after_step(case, form):
    """The HDR frame, its vertical flip, and a frame 10^6 times brighter in the top band only, one step each on the same objects: every result
    is what fresh objects give for that frame alone, bit for bit."""
    mode = "symmetric"
    f = local_case(case, mode).image
    top = f.copy()
    top[: band_plans(case, mode, "exchange")[0].own_rows] *= np.float32(1e6)
    frames = (f, np.ascontiguousarray(f[::-1]), top)
    outs, _ = run_sharded(case, mode, form, frames)
    for step, frame in enumerate(frames):
        fresh = run_sharded(case, mode, form, (frame,))[0][0]
        assert np.isfinite(fresh).all()
        assert np.array_equal(outs[step], fresh), (form, step, _where(outs[step], fresh))
    assert not np.array_equal(outs[0], outs[2])


# ---- K4 on its own ----------------------------------------------------------------------------------------------------------------------------
K4_COUNTS = (1, 3, 4, 5, 1023, 4 * 256 * 64 - 1, 4 * 256 * 64 + 5)
LEAD = 4  # floats in front of `accum` that must stay as they were


@pytest.mark.parametrize("max_workgroups", [0, 1, 3, 64])
@pytest.mark.parametrize("count", K4_COUNTS)
def test_add_rows_at_every_alignment(count, max_workgroups):
    """accum[0:count] += src[0:count] with accum and src 0 ... 3 floats past a 16-byte boundary each (16 combinations): bit-identical to NumPy
    float32, nothing written outside accum[0:count], src unchanged.  max_workgroups 0 is rpsf_add_rows (a workgroup per 1024 floats); 1, 3
    and 64 are rpsf_add_rows_narrow, whose grid-stride loop then takes 65, 22 and 2 trips at the largest count."""
    from regularizepsf_amd import _native

    rng = np.random.default_rng(count * 7 + max_workgroups)
    size = LEAD + 3 + count + 4
    a0 = (rng.standard_normal(size) * 10.0 ** rng.integers(-3, 4, size)).astype(np.float32)
    b0 = (rng.standard_normal(size) * 10.0 ** rng.integers(-3, 4, size)).astype(np.float32)
    da, db = _native.DeviceBuffer(a0.nbytes), _native.DeviceBuffer(b0.nbytes)
    try:
        for off_a in range(4):
            for off_b in range(4):
                da.upload(a0)
                db.upload(b0)
                lo = LEAD + off_a
                _native.add_rows(da.at(lo * 4), db.at(off_b * 4), count, max_workgroups=max_workgroups)
                _native.check(_native.lib().rpsf_device_synchronize(0))
                want = a0.copy()
                want[lo : lo + count] = a0[lo : lo + count] + b0[off_b : off_b + count]
                got = da.download((size,))
                assert np.array_equal(got[lo : lo + count], want[lo : lo + count]), (off_a, off_b)
                assert np.array_equal(got, want), ("written outside accum", off_a, off_b)  # the sentinels on either side included
                assert np.array_equal(db.download((size,)), b0), ("src changed", off_a, off_b)
    finally:
        da.free()
        db.free()


def test_add_rows_refuses_no_workgroups_and_adds_nothing_at_count_0():
    from regularizepsf_amd import _native

    a0 = np.arange(16, dtype=np.float32)
    da, db = _native.DeviceBuffer(a0.nbytes).upload(a0), _native.DeviceBuffer(a0.nbytes).upload(a0)
    try:
        lib = _native.lib()
        assert lib.rpsf_add_rows_narrow(0, da.ptr, db.ptr, 16, 0, None) == _native.E_BADARG
        assert lib.rpsf_add_rows_narrow(0, da.ptr, db.ptr, 16, -1, None) == _native.E_BADARG
        assert lib.rpsf_add_rows(0, da.ptr, db.ptr, 0, None) == 0
        assert lib.rpsf_add_rows_narrow(0, da.at(4), db.at(8), 0, 3, None) == 0
        _native.check(lib.rpsf_device_synchronize(0))
        assert np.array_equal(da.download((16,)), a0) and np.array_equal(db.download((16,)), a0)
    finally:
        da.free()
        db.free()
