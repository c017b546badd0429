"""The conditions that tests/test_gpu_sharding_sizes.py relies on, proven from NumPy and the float64 oracle alone (no GPU), for every case of
tests/sharding_cases.py, both seams and the five pad modes the kernels evaluate: the band plans are accepted, partition the patches and tile
the image; every band owns rows; every row a band's patches read is resident under the pad mode in use; enough of the frame, and of the rows
each band receives, is dim for the bound per neighbourhood to see a seam; the branches of ShardedApply's constructor are the ones the table
names; and the band buffers, emulated in float64, stitch to the whole-frame oracle."""

import numpy as np
import pytest

from regularizepsf_amd.sharding import make_band_plans
from oracle import regpsf_oracle as orc
from tests.helpers import KERNEL_PAD_MODES
from tests.sharding_cases import (CASES, FORMS, FRAME_CASES, NO_ROWS, SEAM_ROWS_DIM, SEAM_ROWS_DIM_SMALL, SEAMS, SERVED, band_buffer, band_plans, expected_branches, local_case,
                                  patch_terms, resident_window_holds, seam_patches, seam_rows_dim_share, transfer)

CASE_IDS = [c.name for c in CASES]


def test_the_table_spans_sizes_widths_and_lattices():
    generations = {"sweep": (16, 32, 64), "second": (128, 256)}
    for sizes in generations.values():
        widths = {c.shape[1] % 4 for c in CASES if c.n in sizes and c.lattice == "covering"}
        assert widths >= {0, 1, 2}, (sizes, widths)  # the seam rows start at every alignment
    assert {c.n for c in CASES} == {16, 32, 64, 128, 256}
    for n in (16, 32, 64, 128):
        assert any(c.n == n and c.single for c in CASES) and any(c.n == n and not c.single for c in CASES)
    assert any(c.n == 128 and c.shape[1] % 32 == 0 for c in CASES)  # persistent + fused in bands
    assert {c.lattice for c in CASES} == {"covering", "rows8", "hole"}
    assert {c.n for c in FRAME_CASES} == {16, 32, 64, 128, 256} and all(c.ordered for c in FRAME_CASES)
    assert len(set(CASE_IDS)) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_band_plans_of_every_case(case):
    """Accepted, a partition of the patches, owned rows that tile the image, no empty band, resident windows, for 2 seams x 5 pad modes."""
    coords = transfer(case)[0]
    h = case.shape[0]
    for mode in KERNEL_PAD_MODES:
        for seam in SEAMS:
            plans = band_plans(case, mode, seam)
            assert len(plans) == case.world
            assert all(p.own_rows >= 1 and p.image_rows >= 1 and len(p.patch_index) >= 1 for p in plans), (mode, seam)
            assert [p.out_row0 for p in plans] == list(np.cumsum([0] + [p.own_rows for p in plans[:-1]])) and sum(p.own_rows for p in plans) == h
            assert all(resident_window_holds(case, p, mode) for p in plans), (mode, seam)
            assert all(0 <= p.image_row0 and p.image_row0 + p.image_rows <= h for p in plans)
            if mode == "wrap" and coords[0][0] < 0:  # the first lattice row reads the frame's last rows, the last one its first
                assert (plans[0].image_row0, plans[0].image_rows) == (0, h) and (plans[-1].image_row0, plans[-1].image_rows) == (0, h)
            if seam == "exchange":
                assert sorted(i for p in plans for i in p.patch_index) == list(range(len(coords)))
                assert plans[0].recv_rows == 0 and plans[-1].send_rows == 0
                assert all(p.send_rows >= 1 for p in plans[:-1]) and [p.recv_rows for p in plans[1:]] == [p.send_rows for p in plans[:-1]]
                assert all(p.send_offset_rows == p.own_rows >= 1 and p.out_rows == p.own_rows + p.send_rows for p in plans[:-1])  # (e): one row early is in bounds
                assert all(p.recv_rows <= p.own_rows for p in plans)
            else:
                assert set(range(len(coords))) == {i for p in plans for i in p.patch_index}
                assert all(p.send_rows == 0 and p.recv_rows == 0 and p.out_rows == p.own_rows for p in plans)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_branches_are_the_tables(case):
    """`once`: some band's seam patches run once, beside a main plan of the others; `single`: some sending band is a single lattice row, so
    it has no others and takes the spill-buffer branch.  The same under every pad mode; the other forms have one branch each."""
    coords = transfer(case)[0]
    for mode in KERNEL_PAD_MODES:
        branches = expected_branches(case, mode, "overlap")
        assert len(branches) == case.world and all(overlap and not pipeline for _, _, pipeline, overlap in branches)
        assert any(once for _, once, _, _ in branches) == case.once
        senders = [b for b in band_plans(case, mode, "exchange") if b.send_rows]
        single = [len({coords[i][0] for i in b.patch_index}) == 1 for b in senders]
        assert any(single) == case.single
        for b, alone in zip(senders, single):
            seam, rest = seam_patches(case, b)
            assert seam and bool(rest) != alone
            assert ((b.rank, not alone, False, True) in branches)
        assert (case.world - 1, False, False, True) in branches  # the last band only receives: no seam plan
        assert expected_branches(case, mode, "pipeline") == {(r, False, True, False) for r in range(case.world)}
        for form in ("sequence", "recompute"):
            assert expected_branches(case, mode, form) == {(r, False, False, False) for r in range(case.world)}
    if case.lattice == "rows8":  # the patches that reach below a band's line span three lattice rows
        for b in band_plans(case, "symmetric", "exchange")[:-1]:
            assert len({coords[i][0] for i in seam_patches(case, b)[0]}) == 3
    assert set(FORMS) == {"overlap", "sequence", "pipeline", "recompute"}


@pytest.mark.parametrize("mode", KERNEL_PAD_MODES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_dim_shares_and_float64_stitching(case, mode):
    """LocalCase asserts the 10 % dim share itself; the rows every band receives are dim for a quarter at least; the band buffers of both seams,
    summed in float64 from the band's own patches, stitch to the oracle at 1e-9."""
    lc = local_case(case, mode)
    assert lc.share >= 0.10
    share = seam_rows_dim_share(case, mode)
    assert share >= (SEAM_ROWS_DIM if case.n > 64 else SEAM_ROWS_DIM_SMALL), share
    terms = patch_terms(case, mode)
    tol = 1e-9 * np.abs(lc.ref).max()
    plans = band_plans(case, mode, "exchange")
    bufs = [band_buffer(case, p, terms) for p in plans]
    for g in range(1, case.world):
        send = bufs[g - 1][plans[g - 1].send_offset_rows : plans[g - 1].send_offset_rows + plans[g - 1].send_rows]
        bufs[g][: plans[g].recv_rows] += send
    got = np.concatenate([b[: p.own_rows] for b, p in zip(bufs, plans)])
    assert got.shape == lc.ref.shape and np.abs(got - lc.ref).max() <= tol
    got = np.concatenate([band_buffer(case, p, terms) for p in band_plans(case, mode, "recompute")])
    assert got.shape == lc.ref.shape and np.abs(got - lc.ref).max() <= tol


@pytest.mark.parametrize(("n", "shape", "world", "seam"), NO_ROWS)
def test_a_band_without_rows_is_refused(n, shape, world, seam):
    """Band 0 would be the covering's first lattice row alone, at -N/2: every output row its patches reach belongs to the next band."""
    coords = [tuple(int(v) for v in c) for c in orc.calculate_covering(shape, n)]
    with pytest.raises(ValueError, match="own no output rows"):
        make_band_plans(coords, n, shape[0], world, seam=seam)


@pytest.mark.parametrize(("n", "shape", "world", "seam"), SERVED)
def test_the_neighbouring_splits_are_served(n, shape, world, seam):
    coords = [tuple(int(v) for v in c) for c in orc.calculate_covering(shape, n)]
    plans = make_band_plans(coords, n, shape[0], world, seam=seam)
    assert all(p.own_rows >= 1 for p in plans) and sum(p.own_rows for p in plans) == shape[0]
