"""Model fits (DESIGN.md 3.7 "Model fits", kernel S8) on the GPU, through the C ABI (regularizepsf_amd.stars._Finder and ._Model) and
through fit_stars, against the float64 restatement bit for bit and against the CPU emulator of the same per-thread source byte for byte
(tests/fit_cases.py) - the cases and checks of tests/test_fit_host.py.

Measured on an MI355X: see profiles/star_fit_gpu.log (every check prints its figures before it asserts)."""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import fit_cases as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tuple(fc.GRID_CASES) + tuple(fc.MASKED_CASES) + tuple(fc.OTHER_CASES))
def test_the_fit_matches_the_restatement_and_the_emulator(name):
    rows = fc.check_case(stars._Finder, stars._Model, name)
    emu_level_f, emu_rows = fc.run(fc.EmuFinder, fc.EmuModel, fc.case(name))
    for radius, got in rows.items():
        assert got.tobytes() == emu_rows[radius].tobytes(), (name, radius)  # the same per-thread source on the CPU: the same bytes


def test_every_flag_fires():
    fc.check_every_flag_fires(stars._Finder, stars._Model)


def test_hard_positions():
    fc.check_hard_positions(stars._Finder, stars._Model)


def test_row_counts_around_a_workgroup():
    fc.check_row_counts(stars._Finder, stars._Model, fc.emulator_info()[0])


@pytest.mark.parametrize("name", ("N = 16, mesh, flux and background", "masked, mesh, flux alone", "9 rows"))
def test_repeats_are_bit_equal(name):
    fc.check_reproducible(stars._Finder, stars._Model, name)


def test_detect_measure_photometry_and_refine_are_untouched():
    fc.check_isolation(stars._Finder, stars._Model)


def test_state_and_argument_errors():
    fc.check_errors(stars._Finder, stars._Model, _native.NativeError)


def test_positions_and_return_codes_on_a_live_handle():
    """rpsf_stars_positions after a fit gives the bits it gave before; RPSF_E_STATE and RPSF_E_BADARG write nothing; n = 0 launches nothing
    and needs no pointers; one model serves two finders, and a model of another device is refused."""
    lib = _native.lib()
    c = fc.case("N = 9, mesh, flux and background")
    finder, model = stars._Finder(c["frame"].shape, c["box"]), stars._Model(c["cube"])
    try:
        out, ms = np.full((2, fc.COLUMNS), -1.0), ctypes.c_double(-1.0)
        pos, cells = np.ascontiguousarray(c["positions"][:2]), np.array([0, 2], np.int32)
        args = (finder._handle, model._handle, 2, _native._ptr(pos), _native._ptr(cells), 3.5, 1, 1, _native._ptr(out))
        assert lib.rpsf_stars_fit(*args) == _native.E_STATE and b"before" in lib.rpsf_last_error()
        assert lib.rpsf_stars_fit(finder._handle, model._handle, 0, None, None, 3.5, 1, 1, None) == _native.E_STATE
        assert np.all(out == -1.0)
        finder.background_device(c["frame"], None)
        rows = finder.detect_device(3.0, 5, None)
        before = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(before)) == 0
        assert lib.rpsf_stars_fit(*args) == 0 and not np.any(out == -1.0)
        assert lib.rpsf_stars_fit_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value > 0.0
        after = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(after)) == 0
        assert after.tobytes() == before.tobytes() == rows.tobytes()
        assert lib.rpsf_stars_fit(finder._handle, model._handle, 0, None, None, 3.5, 1, 1, None) == 0  # nothing to launch
        assert lib.rpsf_stars_fit_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value == 0.0
        kept = out.copy()
        assert lib.rpsf_stars_fit(finder._handle, model._handle, 2, _native._ptr(pos), _native._ptr(cells), 3.75, 1, 1,
                                  _native._ptr(out)) == _native.E_BADARG and b"N / 2 - 1" in lib.rpsf_last_error()
        assert lib.rpsf_stars_fit(finder._handle, model._handle, 2, _native._ptr(pos), _native._ptr(cells), 3.5, 2, 1,
                                  _native._ptr(out)) == _native.E_BADARG
        assert out.tobytes() == kept.tobytes()
        other = stars._Finder((40, 56), 8)  # the model outlives a finder and serves another
        try:
            other.background_device(np.ascontiguousarray(c["frame"][:40, :40].repeat(2, axis=1)[:, :56]), None)
            assert other.fit(model, pos, cells, 2.0).shape == (2, fc.COLUMNS)
        finally:
            other.close()
        assert lib.rpsf_stars_fit(*args) == 0 and out.tobytes() == kept.tobytes()
        if _native.device_count() > 1:
            elsewhere = stars._Model(c["cube"], device=1)
            try:
                assert lib.rpsf_stars_fit(finder._handle, elsewhere._handle, 2, _native._ptr(pos), _native._ptr(cells), 3.5, 1, 1,
                                          _native._ptr(out)) == _native.E_BADARG and b"another device" in lib.rpsf_last_error()
            finally:
                elsewhere.close()
    finally:
        model.close()
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ composition
def test_fit_stars_on_host_and_device_frames():
    frame, truth = fc.field()["frame"].astype(np.float32), fc.field()["truth"]
    masked = fc.masked_field()
    coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering(fc.SHAPE, 9)]
    cube = np.stack([fc.model(9)[k % 4 if k % 4 != fc.ZERO else fc.GAUSSIAN] for k in range(len(coordinates))])
    psf = rp.IndexedCube(coordinates, cube)
    host = rp.fit_stars(frame, truth, psf, 3.5, box=16)
    assert host[0].dtype == stars.fit_dtype() and host[0].shape == (5,)
    emu_finder, emu_model = fc.EmuFinder(frame.shape, 16), fc.EmuModel(cube)
    emu_finder.background_device(frame, None)
    cells = stars.nearest_cells(truth, coordinates, 9)
    assert host[0].tobytes() == stars.fit_from_sums(emu_finder.fit(emu_model, truth, cells, 3.5)).tobytes()
    emu_finder.close()
    for options in ({}, {"background": "none"}, {"fit_background": False}, {"cells": [np.array([0, -1, 3, 2, 400])]}):  # a DeviceArray frame
        on_host = rp.fit_stars(frame, truth, psf, 2.5, box=16, **options)
        on_device = rp.fit_stars(rp.to_device(frame), truth, psf, 2.5, box=16, **options)
        assert on_host[0].tobytes() == on_device[0].tobytes(), options
    frames = np.stack([frame, masked["frame"].astype(np.float32)])
    masks = [np.zeros(fc.SHAPE, bool), masked["mask"]]
    on_host = rp.fit_stars(frames, [truth, truth[:3]], psf, 3.5, masks, box=16)
    on_device = rp.fit_stars(rp.to_device(frames), [truth, truth[:3]], psf, 3.5, masks, box=16)
    assert [len(r) for r in on_host] == [5, 3] and all(a.tobytes() == b.tobytes() for a, b in zip(on_host, on_device))
    assert on_host[0].tobytes() == host[0].tobytes() and np.all(on_host[1]["coverage"] < 1.0)
    nothing = rp.fit_stars(rp.to_device(np.full(fc.SHAPE, np.nan, np.float32)), [truth], psf, 3.5, box=16)[0]
    assert np.all(nothing["no_mesh"]) and np.isnan(nothing["flux"]).all() and nothing["row"].tobytes() == truth[:, 0].tobytes()
    refined = rp.refine_stars(frame, np.rint(truth), 1.3, box=16)
    assert rp.fit_stars(frame, refined, psf, 3.5, box=16)[0]["row"].tobytes() == refined[0]["row"].tobytes()


def test_fit_stars_end_to_end_on_a_built_model():
    """One 64 x 64 frame of the truth case: the model ArrayPSFBuilder builds from it at the true positions, fitted to the same stars.  The
    rows are the restatement's on that model bit for bit, and the model describes its stars as well as the float64 oracle's does - the
    bound is fit_cases.MEASURED_RESIDUAL times TRUTH_MARGIN, fixed on the CPU; kernel B1's float32 patches move the figure in the seventh
    place."""
    t = fc.truth_case()
    frame, truth = t["frames"][0].astype(np.float32), t["truth"][0]
    psf, counts = rp.ArrayPSFBuilder(fc.TRUTH_N).build(frame, stars=[truth])
    assert sum(counts.values()) > 0
    got = rp.fit_stars(frame, truth, psf, fc.TRUTH_RADIUS, background="none", box=fc.BOX)[0]
    coordinates, values = stars.model_cube(psf)
    cells = stars.nearest_cells(truth, coordinates, fc.TRUTH_N)
    want = stars.fit_from_sums(fc.ref_fit(frame, None, fc.BOX, None, values, truth, cells, fc.TRUTH_RADIUS, True, "none"))
    median = float(np.median(got["residual_fraction"]))
    displaced = [float(np.median(rp.fit_stars(frame, truth + o, psf, fc.TRUTH_RADIUS, background="none", box=fc.BOX, cells=cells)[0]["residual_fraction"]))
                 for o in (0.5, -0.5)]
    print(f"end to end: {len(got)} stars in cells {got['cell'].tolist()}, median residual_fraction {median:.4g} (the oracle's model: "
          f"{fc.MEASURED_RESIDUAL}), half a pixel off {displaced[0]:.4g} and {displaced[1]:.4g}; flux {got['flux'].round(1).tolist()}")
    assert np.all(got["flags"] == 0) and got["cell"].tolist() == cells.tolist() and np.all(got["coverage"] == 1.0)
    assert all(fc.same_bits(got[name].astype(np.float64), want[name].astype(np.float64)) for name in got.dtype.names)
    assert median <= fc.TRUTH_MARGIN * fc.MEASURED_RESIDUAL and min(displaced) >= fc.DISPLACED_FACTOR * median
    summary = rp.cell_fit_summary([got], psf)
    assert summary["count"].sum() == len(got) and set(np.flatnonzero(summary["count"]).tolist()) == set(cells.tolist())
