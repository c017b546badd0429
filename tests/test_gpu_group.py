"""Group fits (DESIGN.md 3.7 "Group fits", kernel S11) on the GPU, through the C ABI (regularizepsf_amd.stars._Finder and ._Model) and
through fit_groups, against the float64 restatement bit for bit and against the CPU emulator of the same per-thread source byte for byte
(tests/group_cases.py) - the cases and checks of tests/test_group_host.py.

Measured on an MI355X: see profiles/star_group_gpu.log (every check prints its figures before it asserts)."""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import fit_cases as fc
from tests import group_cases as gc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tuple(gc.CROWD_CASES) + tuple(gc.MASKED_CASES) + tuple(gc.OTHER_CASES) + tuple(gc.COUNT_CASES))
def test_the_group_fit_matches_the_restatement_and_the_emulator(name):
    rows = gc.check_case(stars._Finder, stars._Model, name)
    _, emu_rows = gc.run(gc.EmuFinder, gc.EmuModel, gc.case(name))
    for radius, got in rows.items():
        assert got.tobytes() == emu_rows[radius].tobytes(), (name, radius)  # the same per-thread source on the CPU: the same bytes


def test_the_crowd_is_grouped_as_laid_out():
    gc.check_crowd_groups(stars._Finder, stars._Model)


def test_every_flag_fires():
    gc.check_every_flag_fires(stars._Finder, stars._Model)


def test_group_counts_around_a_workgroup():
    columns, max_group, per_workgroup = stars.fit_groups_info()
    assert (columns, max_group) == (gc.COLUMNS, gc.MAX_GROUP) and per_workgroup == gc.emulator_info()[0]
    gc.check_group_counts(stars._Finder, stars._Model, per_workgroup)


def test_the_members_sums_are_fit_stars_and_stars_alone_are_its_rows():
    gc.check_against_fit(stars._Finder, stars._Model)


def test_the_residual_is_subtract_stars():
    gc.check_against_render(stars._Finder, stars._Model)


def test_the_fluxes_against_an_independent_solve():
    assert gc.check_against_lstsq(stars._Finder, stars._Model, tuple(gc.CROWD_CASES)[:4] + tuple(gc.MASKED_CASES)[:1]) <= 1.0


@pytest.mark.parametrize("name", ("crowd, N = 16, mesh, flux and background", "masked crowd, mesh, flux alone", "9 groups"))
def test_repeats_are_bit_equal(name):
    gc.check_reproducible(stars._Finder, stars._Model, name)


def test_the_other_kernels_are_untouched_and_a_model_serves_two_finders():
    gc.check_isolation(stars._Finder, stars._Model)


def test_state_and_argument_errors():
    gc.check_errors(stars._Finder, stars._Model, _native.NativeError)


def test_return_codes_on_a_live_handle():
    """RPSF_E_STATE and RPSF_E_BADARG write nothing; n = 0 launches nothing and needs no pointers; a model of another device is refused."""
    lib = _native.lib()
    c = gc.case("crowd, N = 9, mesh, flux and background")
    finder, model = stars._Finder(c["frame"].shape, c["box"]), stars._Model(c["cube"])
    try:
        out, ms = np.full((4, gc.COLUMNS), -1.0), ctypes.c_double(-1.0)
        pos, cells = np.ascontiguousarray(c["positions"][:4]), np.zeros(4, np.int32)
        args = lambda radius=3.5, fb=1, link=7.0, g=8: (finder._handle, model._handle, 4, _native._ptr(pos), _native._ptr(cells), radius, fb, 1,
                                                        link, g, _native._ptr(out))
        assert lib.rpsf_stars_fit_groups(*args()) == _native.E_STATE and b"before" in lib.rpsf_last_error()
        assert lib.rpsf_stars_fit_groups(finder._handle, model._handle, 0, None, None, 3.5, 1, 1, 7.0, 8, None) == _native.E_STATE
        assert np.all(out == -1.0)
        finder.background_device(c["frame"], None)
        rows = finder.detect_device(3.0, 5, None)
        before = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(before)) == 0
        assert lib.rpsf_stars_fit_groups(*args()) == 0 and not np.any(out == -1.0)
        assert lib.rpsf_stars_fit_groups_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value > 0.0
        after = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(after)) == 0
        assert after.tobytes() == before.tobytes() == rows.tobytes()
        assert lib.rpsf_stars_fit_groups(finder._handle, model._handle, 0, None, None, 3.5, 1, 1, 7.0, 8, None) == 0  # nothing to launch
        assert lib.rpsf_stars_fit_groups_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value == 0.0
        kept = out.copy()
        assert lib.rpsf_stars_fit_groups(*args(radius=3.75)) == _native.E_BADARG and b"N / 2 - 1" in lib.rpsf_last_error()
        assert lib.rpsf_stars_fit_groups(*args(fb=2)) == _native.E_BADARG
        assert lib.rpsf_stars_fit_groups(*args(link=7.5)) == _native.E_BADARG and b"link" in lib.rpsf_last_error()
        assert lib.rpsf_stars_fit_groups(*args(g=9)) == _native.E_BADARG and b"max_group" in lib.rpsf_last_error()
        assert out.tobytes() == kept.tobytes()
        if _native.device_count() > 1:
            elsewhere = stars._Model(c["cube"], device=1)
            try:
                assert lib.rpsf_stars_fit_groups(finder._handle, elsewhere._handle, 4, _native._ptr(pos), _native._ptr(cells), 3.5, 1, 1, 7.0, 8,
                                                 _native._ptr(out)) == _native.E_BADARG and b"another device" in lib.rpsf_last_error()
            finally:
                elsewhere.close()
    finally:
        model.close()
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ composition
def test_fit_groups_on_host_and_device_frames():
    frame = fc.field()["frame"].astype(np.float32)
    masked = fc.masked_field()
    positions, cells = gc.crowd()
    coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering(fc.SHAPE, 9)]
    cube = np.stack([fc.model(9)[fc.LOBES if k % 3 == 1 else fc.GAUSSIAN] for k in range(len(coordinates))])
    psf = rp.IndexedCube(coordinates, cube)
    host = rp.fit_groups(frame, positions, psf, 2.3, box=16)
    assert host[0].dtype == stars.group_fit_dtype() and host[0].shape == (len(positions),)
    emu_finder, emu_model = gc.EmuFinder(frame.shape, 16), gc.EmuModel(cube)
    emu_finder.background_device(frame, None)
    nearest = stars.nearest_cells(positions, coordinates, 9)
    assert host[0].tobytes() == stars.group_fit_from_sums(emu_finder.fit_groups(emu_model, positions, nearest, 2.3)).tobytes()
    emu_finder.close()
    for options in ({}, {"background": "none"}, {"fit_background": False}, {"max_group": 2}, {"link": 3.0}):  # a DeviceArray frame
        on_host = rp.fit_groups(frame, positions, psf, 2.3, box=16, **options)
        on_device = rp.fit_groups(rp.to_device(frame), positions, psf, 2.3, box=16, **options)
        assert on_host[0].tobytes() == on_device[0].tobytes(), options
    frames = np.stack([frame, masked["frame"].astype(np.float32)])
    masks = [np.zeros(fc.SHAPE, bool), masked["mask"]]
    on_host = rp.fit_groups(frames, [positions, positions[:7]], psf, 2.3, masks, box=16)
    on_device = rp.fit_groups(rp.to_device(frames), [positions, positions[:7]], psf, 2.3, masks, box=16)
    assert [len(r) for r in on_host] == [len(positions), 7] and all(a.tobytes() == b.tobytes() for a, b in zip(on_host, on_device))
    assert on_host[0].tobytes() == host[0].tobytes()
    nothing = rp.fit_groups(rp.to_device(np.full(fc.SHAPE, np.nan, np.float32)), [positions], psf, 2.3, box=16)[0]
    assert np.all(nothing["no_mesh"]) and np.isnan(nothing["flux"]).all() and np.all(nothing["group_size"] == 1)
    flat = rp.fit_groups(frame, positions[:21], psf, 2.3, box=16, background="none", fit_background=False)
    residual = rp.subtract_stars(frame, flat, psf, 2.3, dtype=np.float64)[0]  # subtract_stars takes the new array as it is
    assert fc.same_bits(residual[flat[0]["peak_row"].astype(int), flat[0]["peak_col"].astype(int)], flat[0]["peak_e"])
    assert rp.cell_fit_summary(host, psf)["count"].sum() == int((host[0]["flags"] == 0).sum())


def test_the_joint_fit_recovers_what_the_single_fit_does_not():
    gc.check_truth(rp.fit_groups, rp.fit_stars, "fit_groups on the GPU")
