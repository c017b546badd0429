"""The star kernels at the product's model sizes, radii and frames (tests/wide_cases.py) without a GPU: every case on the CPU emulators of
the kernels' per-thread source against the float64 restatements, by each kernel's own comparison, and the conditions the case table must
hold - a case that reaches nothing must fail, not pass.  tests/test_gpu_wide.py runs the same cases on the GPU."""

import numpy as np
import pytest

from tests import builder_sub_cases as bc
from tests import fit_cases as fc
from tests import wide_cases as wc

EMU = (wc.EmuFinder, wc.EmuModel)


def test_the_frame_has_a_mesh_of_four_by_four_with_partial_last_boxes():
    finder = wc.EmuFinder(wc.SHAPE, wc.BOX)
    try:
        level, rms = finder.background(wc.field()["frame"], None)
    finally:
        finder.close()
    assert level.shape == rms.shape == (4, 4) and wc.SHAPE[0] % wc.BOX == 8 and wc.SHAPE[1] % wc.BOX == 40
    assert np.isfinite(level).all() and wc.field()["frame"].dtype == np.float64
    assert np.array_equal(wc.field()["frame"], wc.field()["frame"].astype(np.float32))  # rounded to float32 once
    m = wc.masked_field()
    assert np.isnan(m["frame"]).sum() == 1 and np.isinf(m["frame"]).sum() == 2 and m["mask"].sum() >= 2 * 30 * 30
    p = wc.positions()
    assert np.all(p[:5] - 64.0 >= 0) and np.all(p[:5] + 64.0 <= np.array(wc.SHAPE))  # every star's disc of R = 64 is on the frame
    assert np.all(np.abs(p) < 2.0 ** 20) and np.abs(p).max() == 2.0 ** 20 - 0.5
    big = wc.cube(256)[wc.NARROW]
    assert (big == 0.0).any() and ((big > 0.0) & (big < np.finfo(np.float64).tiny)).any()  # far values denormal and zero


@pytest.mark.parametrize("name", tuple(wc.PHOT_CASES))
def test_apertures_to_64(name):
    wc.check_photometry(wc.EmuFinder, name)


@pytest.mark.parametrize("name", tuple(wc.REFINE_CASES))
def test_windows_of_sigma_16(name):
    wc.check_refine(wc.EmuFinder, name)


def test_fits_at_every_model_size_and_every_flag():
    rows = {name: wc.check_fit(*EMU, name) for name in wc.FIT_CASES}
    wc.check_fit_flags(rows)
    nothing = rows["no valid mesh node"]
    assert np.all(nothing[:, fc.FLAGS].astype(int) & fc.NO_MESH)


def test_fitted_positions_at_every_model_size():
    steps = {name: wc.check_fitpos(*EMU, name)[0] for name in wc.FITPOS_CASES}
    wc.check_fitpos_ends(steps)


def test_the_render_lists_have_three_chunks_an_empty_tile_and_a_partial_column():
    wc.check_render_lists()


@pytest.mark.parametrize("name", tuple(wc.RENDER_CASES))
def test_model_and_residual_frames(name):
    wc.check_render(*EMU, name)


@pytest.mark.parametrize("name", tuple(wc.GROUP_CASES))
def test_group_fits(name):
    wc.check_group(*EMU, name)


def test_neighbour_subtracted_patches_of_64_with_a_model_of_130():
    case = wc.builder_case()
    brute, lists = bc.brute_lists(case), bc.emu_lists(case)
    assert all(np.array_equal(a, b) for a, b in zip(brute, lists))
    patches, flags = bc.emu_patches(case, lists)
    want_patches, want_flags = wc.builder_expected()
    print(f"B1n: {len(flags)} patches of 64, lists of {[len(l) for l in lists]} neighbours, flags {flags.tolist()}")
    assert flags.tolist() == want_flags.tolist() and bc.same_bits(patches, want_patches)
    assert (flags == bc.ACCEPTED).sum() >= 3
