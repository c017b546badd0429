"""Weighted fits (DESIGN.md 3.7 "Weighted fits", kernel S12) on the GPU, through the C ABI (regularizepsf_amd.stars._Finder and ._Model)
and through fit_stars_weighted, against the float64 restatement bit for bit and against the CPU emulator of the same per-thread source
byte for byte (tests/fitw_cases.py) - the cases and checks of tests/test_fitw_host.py.

Measured on an MI355X: see profiles/star_fitw_gpu.log (every check prints its figures before it asserts)."""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import fit_cases as fc
from tests import fitw_cases as fw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tuple(fw.TABLE_CASES))
def test_the_weighted_fit_matches_the_restatement_and_the_emulator(name):
    rows = fw.check_case(stars._Finder, stars._Model, name)
    _, emu_rows = fw.run(fw.EmuFinder, fw.EmuModel, fw.case(name))
    for radius, got in rows.items():
        assert got.tobytes() == emu_rows[radius].tobytes(), (name, radius)  # the same per-thread source on the CPU: the same bytes


def test_every_flag_fires():
    fw.check_every_flag_fires(stars._Finder, stars._Model)


def test_each_bad_variance_takes_out_its_pixel():
    fw.check_bad_variances(stars._Finder, stars._Model)


def test_unit_and_power_of_two_variances_against_the_gpus_own_unweighted_fit():
    fw.check_power_of_two(stars._Finder, stars._Model)


def test_row_counts_around_a_workgroup():
    fw.check_row_counts(stars._Finder, stars._Model, fw.emulator_info()[0])


@pytest.mark.parametrize("name", ("N = 16, mesh, flux and background, map", "noise model, gain 2.5", "9 rows"))
def test_repeats_are_bit_equal(name):
    fw.check_reproducible(stars._Finder, stars._Model, name)


def test_the_other_kernels_are_untouched():
    fw.check_isolation(stars._Finder, stars._Model)


def test_state_and_argument_errors():
    fw.check_errors(stars._Finder, stars._Model, _native.NativeError)


def test_return_codes_and_times_on_a_live_handle():
    """RPSF_E_STATE before a frame and, in map mode, before a variance frame; RPSF_E_STATE and RPSF_E_BADARG write nothing; the device time
    is positive after a launch and 0.0 after n = 0, which needs no pointers; a variance view of another shape and a model of another device
    are refused."""
    lib = _native.lib()
    c = fw.case("N = 9, mesh, flux and background, map")
    finder, model = stars._Finder(c["frame"].shape, c["box"]), stars._Model(c["cube"])
    try:
        out, ms = np.full((2, fw.COLUMNS), -1.0), ctypes.c_double(-1.0)
        pos, cells = np.ascontiguousarray(c["positions"][:2]), np.array([0, 2], np.int32)
        common = (finder._handle, model._handle, 2, _native._ptr(pos), _native._ptr(cells), 3.5, 1, 1)
        by_map, by_model = (*common, stars.VARIANCE_MAP, 0.0, 1.0, _native._ptr(out)), (*common, stars.VARIANCE_MODEL, 0.3, 2.0, _native._ptr(out))
        nothing = (finder._handle, model._handle, 0, None, None, 3.5, 1, 1)
        assert lib.rpsf_stars_fit_weighted(*by_map) == _native.E_STATE and b"before" in lib.rpsf_last_error()  # no frame yet
        assert lib.rpsf_stars_fit_weighted(*by_model) == _native.E_STATE
        assert lib.rpsf_stars_fit_weighted(*nothing, stars.VARIANCE_MODEL, 0.3, 2.0, None) == _native.E_STATE
        finder.background_device(c["frame"], None)
        rows = finder.detect_device(3.0, 5, None)
        assert lib.rpsf_stars_fit_weighted(*by_map) == _native.E_STATE and b"rpsf_stars_variance" in lib.rpsf_last_error()  # no variance yet
        assert lib.rpsf_stars_fit_weighted(*nothing, stars.VARIANCE_MAP, 0.0, 1.0, None) == _native.E_STATE
        assert np.all(out == -1.0)
        assert lib.rpsf_stars_fit_weighted_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value == 0.0
        assert lib.rpsf_stars_fit_weighted(*by_model) == 0 and not np.any(out == -1.0)
        assert lib.rpsf_stars_fit_weighted_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value > 0.0
        assert lib.rpsf_stars_fit_weighted(*nothing, stars.VARIANCE_MODEL, 0.3, 2.0, None) == 0  # nothing to launch
        assert lib.rpsf_stars_fit_weighted_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value == 0.0
        finder.variance(c["variance"])
        assert lib.rpsf_stars_fit_weighted(*by_map) == 0
        assert lib.rpsf_stars_fit_weighted_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value > 0.0
        assert lib.rpsf_stars_fit_weighted(*nothing, stars.VARIANCE_MAP, 0.0, 1.0, None) == 0
        assert lib.rpsf_stars_fit_weighted_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value == 0.0
        kept = out.copy()
        assert lib.rpsf_stars_fit_weighted(finder._handle, model._handle, 2, _native._ptr(pos), _native._ptr(cells), 3.75, 1, 1, 0, 0.0, 1.0,
                                           _native._ptr(out)) == _native.E_BADARG and b"N / 2 - 1" in lib.rpsf_last_error()
        assert lib.rpsf_stars_fit_weighted(*common, stars.VARIANCE_MODEL, 0.0, np.inf, _native._ptr(out)) == _native.E_BADARG
        assert lib.rpsf_stars_fit_weighted(*common, 2, 0.3, 2.0, _native._ptr(out)) == _native.E_BADARG
        assert out.tobytes() == kept.tobytes()
        after = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(after)) == 0 and after.tobytes() == rows.tobytes()
        small = rp.to_device(np.ones((c["frame"].shape[0], c["frame"].shape[1] - 1), np.float32))
        view = small._view2d()
        assert lib.rpsf_stars_variance_view(finder._handle, ctypes.byref(view)) == _native.E_BADARG and b"the finder's frame" in lib.rpsf_last_error()
        assert lib.rpsf_stars_fit_weighted(*by_map) == 0 and out.tobytes() == kept.tobytes()  # the variance frame is still the last good one
        if _native.device_count() > 1:
            elsewhere = stars._Model(c["cube"], device=1)
            try:
                assert lib.rpsf_stars_fit_weighted(finder._handle, elsewhere._handle, 2, _native._ptr(pos), _native._ptr(cells), 3.5, 1, 1, 1, 0.3, 2.0,
                                                   _native._ptr(out)) == _native.E_BADARG and b"another device" in lib.rpsf_last_error()
            finally:
                elsewhere.close()
    finally:
        model.close()
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ composition
def test_fit_stars_weighted_on_host_and_device_frames_and_variances():
    frame, truth = fc.field()["frame"].astype(np.float32), fc.field()["truth"]
    masked = fc.masked_field()
    coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering(fc.SHAPE, 9)]
    cube = np.stack([fc.model(9)[k % 4 if k % 4 != fc.ZERO else fc.GAUSSIAN] for k in range(len(coordinates))])
    psf = rp.IndexedCube(coordinates, cube)
    variance, bad = fw.smooth_map(), fw.bad_map()
    host = rp.fit_stars_weighted(frame, truth, psf, 3.5, variance=variance, box=16)
    assert host[0].dtype == stars.weighted_fit_dtype() and host[0].shape == (5,) and (host[0]["flags"] == 0).sum() >= 4  # (one star has a constant cell)
    emu_finder, emu_model = fw.EmuFinder(frame.shape, 16), fw.EmuModel(cube)
    emu_finder.background_device(frame, None)
    emu_finder.variance(variance)
    cells = stars.nearest_cells(truth, coordinates, 9)
    assert host[0].tobytes() == stars.weighted_fit_from_sums(emu_finder.fit_weighted(emu_model, truth, cells, 3.5)).tobytes()
    emu_finder.close()
    for options in ({}, {"background": "none"}, {"fit_background": False}, {"cells": [np.array([0, -1, 3, 2, 400])]}):
        on_host = rp.fit_stars_weighted(frame, truth, psf, 2.5, variance=bad, box=16, **options)
        on_device = rp.fit_stars_weighted(rp.to_device(frame), truth, psf, 2.5, variance=rp.to_device(bad), box=16, **options)
        assert on_host[0].tobytes() == on_device[0].tobytes(), options
        by_model = rp.fit_stars_weighted(frame, truth, psf, 2.5, sky_variance=0.2, gain=3.0, box=16, **options)
        assert by_model[0].tobytes() == rp.fit_stars_weighted(rp.to_device(frame), truth, psf, 2.5, sky_variance=0.2, gain=3.0, box=16, **options)[0].tobytes()
    # a float64 map on the device is rounded once by kernel C1, as the host route rounds it; a strided view is read through its strides
    wide64 = fw.float64_map()
    on_host = rp.fit_stars_weighted(frame, truth, psf, 3.5, variance=wide64, box=16)[0]
    assert on_host.tobytes() == rp.fit_stars_weighted(rp.to_device(frame), truth, psf, 3.5, variance=rp.to_device(wide64), box=16)[0].tobytes()
    assert on_host.tobytes() == rp.fit_stars_weighted(frame, truth, psf, 3.5, variance=wide64.astype(np.float32), box=16)[0].tobytes()
    padded = np.full((fc.SHAPE[0], fc.SHAPE[1] + 3), np.nan, np.float32)
    padded[:, :fc.SHAPE[1]] = variance
    strided = rp.to_device(padded)[:, :fc.SHAPE[1]]
    assert rp.fit_stars_weighted(rp.to_device(frame), truth, psf, 3.5, variance=strided, box=16)[0].tobytes() == host[0].tobytes()
    # one map per frame and one for all, host and device
    frames = np.stack([frame, masked["frame"].astype(np.float32)])
    masks = [np.zeros(fc.SHAPE, bool), masked["mask"]]
    maps = [variance, bad]
    on_host = rp.fit_stars_weighted(frames, [truth, truth[:3]], psf, 3.5, masks, variance=maps, box=16)
    on_device = rp.fit_stars_weighted(rp.to_device(frames), [truth, truth[:3]], psf, 3.5, masks, variance=rp.to_device(np.stack(maps)), box=16)
    listed = rp.fit_stars_weighted(rp.to_device(frames), [truth, truth[:3]], psf, 3.5, masks, variance=[rp.to_device(m) for m in maps], box=16)
    assert [len(r) for r in on_host] == [5, 3] and all(a.tobytes() == b.tobytes() == c.tobytes() for a, b, c in zip(on_host, on_device, listed))
    assert on_host[0].tobytes() == host[0].tobytes() and np.all(on_host[1]["coverage"] < 1.0)
    shared = rp.fit_stars_weighted(rp.to_device(frames), [truth, truth[:3]], psf, 3.5, masks, variance=rp.to_device(variance), box=16)
    assert shared[0].tobytes() == host[0].tobytes() and shared[1].tobytes() != on_host[1].tobytes()
    with pytest.raises(TypeError, match="variance and images must live in the same place"):
        rp.fit_stars_weighted(rp.to_device(frame), truth, psf, 3.5, variance=variance, box=16)
    with pytest.raises(TypeError, match="variance and images must live in the same place"):
        rp.fit_stars_weighted(frame, truth, psf, 3.5, variance=rp.to_device(variance), box=16)
    with pytest.raises(rp.IncorrectShapeError, match="A variance frame of shape"):
        rp.fit_stars_weighted(rp.to_device(frame), truth, psf, 3.5, variance=rp.to_device(padded), box=16)
    nothing = rp.fit_stars_weighted(rp.to_device(np.full(fc.SHAPE, np.nan, np.float32)), [truth], psf, 3.5, sky_variance=1.0, box=16)[0]
    assert np.all(nothing["no_mesh"]) and np.isnan(nothing["flux_err"]).all() and nothing["row"].tobytes() == truth[:, 0].tobytes()


def test_build_fit_weighted_and_rebuild_with_the_faint_stars_left_out():
    """build -> fit_stars_weighted -> build_subtracted(keep=[f["snr"] > 5 for f in fits]) on a small frame of five bright stars, noise of
    variance 4 and two positions on bare noise: the chain runs, the two are not cut, and the result is the composition written out - the
    same call on plain positions, fluxes and cells, and per kept star the patch build cuts from subtract_stars' frame without that star."""
    from regularizepsf_amd.device_array import device_empty

    t = fc.truth_case()
    rng = np.random.default_rng([17, 67])
    frame = (t["frames"][0] + rng.normal(0.0, 2.0, fc.TRUTH_SHAPE)).astype(np.float32)
    positions = np.concatenate([t["truth"][0], [(31.3, 33.8), (34.4, 12.6)]])
    assert np.linalg.norm(positions[5:, None] - positions[None, :5], axis=2).min() > 10.0  # bare noise under the two
    builder = rp.ArrayPSFBuilder(fc.TRUTH_N)
    psf, counts = builder.build(frame, stars=[positions[:5]])  # the model is the bright stars'; the two borrow the first star's cell
    cells = stars.nearest_cells(positions, *stars.model_cube(psf)[:1], fc.TRUTH_N)
    cells[5:] = cells[0]
    fits = rp.fit_stars_weighted(frame, [positions], psf, fc.TRUTH_RADIUS, sky_variance=4.0, background="none", box=fc.BOX, cells=[cells])
    keep = [f["snr"] > 5 for f in fits]
    print(f"snr {fits[0]['snr'].round(1).tolist()}, flux_err {fits[0]['flux_err'].round(1).tolist()}, chi2_reduced {fits[0]['chi2_reduced'].round(2).tolist()}")
    assert np.all(fits[0]["flags"] == 0) and keep[0].tolist() == [True] * 5 + [False] * 2 and np.all(fits[0]["snr"][:5] > 100)
    got_psf, got_counts, got_patches = rp.build_subtracted(frame, fits, psf, fc.TRUTH_RADIUS, keep=keep, return_patches=True)
    want_psf, want_counts, want_patches = builder.build_subtracted(frame, [positions], psf, fc.TRUTH_RADIUS, flux=[fits[0]["flux"]],
                                                                    cells=[fits[0]["cell"]], keep=keep, return_patches=True)
    assert got_counts == want_counts and sum(got_counts.values()) > 0 and list(got_patches) == list(want_patches) and len(got_patches) == 5
    assert got_psf.coordinates == want_psf.coordinates and fc.same_bits(np.asarray(got_psf.values), np.asarray(want_psf.values))
    out = device_empty(frame.shape, np.float32, 0)
    for i in np.flatnonzero(keep[0]):
        flux = fits[0]["flux"].copy()
        flux[i] = np.nan
        rp.subtract_stars(frame, [positions], psf, fc.TRUTH_RADIUS, flux=[flux], cells=[fits[0]["cell"]], out=out)
        (key, patch), = builder.build(out, stars=[positions[i:i + 1]], return_patches=True)[2].items()
        assert np.asarray(got_patches[key]).tobytes() == np.asarray(patch).tobytes(), i
    everything = rp.build_subtracted(frame, fits, psf, fc.TRUTH_RADIUS, return_patches=True)[2]
    assert len(everything) == 7 and set(got_patches) < set(everything)  # without keep the two are cut as well
