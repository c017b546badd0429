"""Fitted positions (DESIGN.md 3.7 "Fitted positions", kernel S9) on the GPU, through the C ABI (regularizepsf_amd.stars._Finder and
._Model) and through fit_positions, against the float64 restatement bit for bit and against the CPU emulator of the same per-thread source
byte for byte (tests/fitpos_cases.py) - the cases and checks of tests/test_fitpos_host.py.

Measured on an MI355X: see profiles/star_fitpos_gpu.log (every check prints its figures before it asserts)."""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import fit_cases as fc
from tests import fitpos_cases as fp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tuple(fp.GRID_CASES) + tuple(fp.MASKED_CASES) + tuple(fp.OTHER_CASES))
def test_the_iteration_matches_the_restatement_and_the_emulator(name):
    rows = fp.check_case(stars._Finder, stars._Model, name)
    _, emu_rows = fp.run(fp.EmuFinder, fp.EmuModel, fp.case(name))
    for radius, (steps, fits) in rows.items():  # the same per-thread source on the CPU: the same bytes
        assert steps.tobytes() == emu_rows[radius][0].tobytes() and fits.tobytes() == emu_rows[radius][1].tobytes(), (name, radius)


def test_without_iterations_both_outputs_are_the_plain_fit():
    fp.check_no_iteration(stars._Finder, stars._Model)


def test_every_stop_rule():
    fp.check_every_stop_rule(stars._Finder, stars._Model)


def test_row_counts_around_a_workgroup():
    fp.check_row_counts(stars._Finder, stars._Model, fp.emulator_info()[0])


@pytest.mark.parametrize("name", ("N = 16, mesh, flux and background", "masked, mesh, flux alone", "9 rows"))
def test_repeats_are_bit_equal(name):
    fp.check_reproducible(stars._Finder, stars._Model, name)


def test_the_other_kernels_are_untouched_and_a_model_serves_two_finders():
    fp.check_isolation(stars._Finder, stars._Model)


def test_state_and_argument_errors():
    fp.check_errors(stars._Finder, stars._Model, _native.NativeError)


def test_positions_and_return_codes_on_a_live_handle():
    """rpsf_stars_positions after a fit_positions gives the bits it gave before; RPSF_E_STATE and RPSF_E_BADARG write nothing; n = 0
    launches nothing and needs no pointers; a model of another device is refused."""
    lib = _native.lib()
    c = fp.case("N = 9, mesh, flux and background")
    finder, model = stars._Finder(c["frame"].shape, c["box"]), stars._Model(c["cube"])
    try:
        steps, fits, ms = np.full((2, fp.COLUMNS), -1.0), np.full((2, fc.COLUMNS), -1.0), ctypes.c_double(-1.0)
        pos, cells = np.ascontiguousarray(c["positions"][:2]), np.array([0, 2], np.int32)
        tail = (16, 1e-4, 2.0, 0.5, 1)
        args = (finder._handle, model._handle, 2, _native._ptr(pos), _native._ptr(cells), 3.5, 1, *tail, _native._ptr(steps), _native._ptr(fits))
        call = lib.rpsf_stars_fit_positions
        assert call(*args) == _native.E_STATE and b"before" in lib.rpsf_last_error()
        assert call(finder._handle, model._handle, 0, None, None, 3.5, 1, *tail, None, None) == _native.E_STATE
        assert np.all(steps == -1.0) and np.all(fits == -1.0)
        finder.background_device(c["frame"], None)
        rows = finder.detect_device(3.0, 5, None)
        before = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(before)) == 0
        assert call(*args) == 0 and not np.any(steps == -1.0) and not np.any(fits[:, :fc.N_ALL + 1] == -1.0)
        assert lib.rpsf_stars_fit_positions_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value > 0.0
        after = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(after)) == 0
        assert after.tobytes() == before.tobytes() == rows.tobytes()
        assert call(finder._handle, model._handle, 0, None, None, 3.5, 1, *tail, None, None) == 0  # nothing to launch
        assert lib.rpsf_stars_fit_positions_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value == 0.0
        kept = steps.copy(), fits.copy()
        bad = [(3.75, 1, *tail), (3.5, 2, *tail), (3.5, 1, -1, 1e-4, 2.0, 0.5, 1), (3.5, 1, 16, 0.0, 2.0, 0.5, 1), (3.5, 1, 16, 1e-4, np.nan, 0.5, 1),
               (3.5, 1, 16, 1e-4, 2.0, 0.0, 1)]
        for rest in bad:
            assert call(finder._handle, model._handle, 2, _native._ptr(pos), _native._ptr(cells), *rest, _native._ptr(steps),
                        _native._ptr(fits)) == _native.E_BADARG, rest
        assert steps.tobytes() == kept[0].tobytes() and fits.tobytes() == kept[1].tobytes()
        assert call(*args) == 0 and steps.tobytes() == kept[0].tobytes() and fits.tobytes() == kept[1].tobytes()
        if _native.device_count() > 1:
            elsewhere = stars._Model(c["cube"], device=1)
            try:
                assert call(finder._handle, elsewhere._handle, 2, _native._ptr(pos), _native._ptr(cells), 3.5, 1, *tail, _native._ptr(steps),
                            _native._ptr(fits)) == _native.E_BADARG and b"another device" in lib.rpsf_last_error()
            finally:
                elsewhere.close()
    finally:
        model.close()
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ the truth, composition
def test_the_truth_with_the_oracles_model():
    """fit_positions on the GPU with the float64 oracle's model: the restatement's result byte for byte, and the bounds."""
    coordinates, values = fc.oracle_model()
    for offset in fp.TRUTH_STARTS:
        got = fp.truth_rows(values, coordinates, offset, rp.fit_positions)
        want = fp.truth_rows(values, coordinates, offset)
        assert np.concatenate(got).tobytes() == np.concatenate(want).tobytes()
    fp.check_truth(what="the oracle's model, the GPU", fit_positions=rp.fit_positions)


def test_the_truth_with_the_model_build_makes():
    """The truth case with the model ArrayPSFBuilder builds from its three frames at the true positions: the same bounds (kernel B1's
    float32 patches move the figures in the seventh place), the rows the restatement's on that model, and fit_stars at the fitted positions
    gives the fit fields bit for bit."""
    t = fc.truth_case()
    frames = t["frames"].astype(np.float32)
    psf, counts = rp.ArrayPSFBuilder(fc.TRUTH_N).build(frames, stars=list(t["truth"]))
    assert sum(counts.values()) > 0
    coordinates, values = stars.model_cube(psf)
    displaced = np.median(np.concatenate(rp.fit_stars(frames, [p + np.asarray(fp.TRUTH_STARTS[0]) for p in t["truth"]], psf, fc.TRUTH_RADIUS,
                                                      background="none", box=fc.BOX,
                                                      cells=[stars.nearest_cells(p, coordinates, fc.TRUTH_N) for p in t["truth"]]))["residual_fraction"])
    fp.check_truth(values, coordinates, "the model build makes", rp.fit_positions, float(displaced))
    got = fp.truth_rows(values, coordinates, fp.TRUTH_STARTS[1], rp.fit_positions)
    want = fp.truth_rows(values, coordinates, fp.TRUTH_STARTS[1])
    assert all(fc.same_bits(g[name].astype(np.float64), w[name].astype(np.float64)) for g, w in zip(got, want) for name in g.dtype.names)
    again = rp.fit_stars(frames, got, psf, fc.TRUTH_RADIUS, background="none", box=fc.BOX)
    for one, fit in zip(got, again):
        assert all(one["fit_flags" if n == "flags" else n].tobytes() == fit[n].tobytes() for n in fit.dtype.names)
    rebuilt, counts = rp.ArrayPSFBuilder(fc.TRUTH_N).build(frames, stars=got)  # the other half of the loop takes the result as it is
    assert sum(counts.values()) > 0 and stars.model_cube(rebuilt)[1].shape == values.shape


def test_fit_positions_on_host_and_device_frames():
    frame, truth = fc.field()["frame"].astype(np.float32), fc.field()["truth"]
    start = truth + (0.3, -0.2)
    masked = fc.masked_field()
    coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering(fc.SHAPE, 9)]
    cube = np.stack([fc.model(9)[k % 4 if k % 4 != fc.ZERO else fc.GAUSSIAN] for k in range(len(coordinates))])
    psf = rp.IndexedCube(coordinates, cube)
    host = rp.fit_positions(frame, start, psf, 3.5, box=16)
    assert host[0].dtype == stars.fitpos_dtype() and host[0].shape == (5,)
    emu_finder, emu_model = fp.EmuFinder(frame.shape, 16), fp.EmuModel(cube)
    emu_finder.background_device(frame, None)
    cells = stars.nearest_cells(start, coordinates, 9)
    assert host[0].tobytes() == stars.fitpos_from_sums(*emu_finder.fit_positions(emu_model, start, cells, 3.5)).tobytes()
    emu_finder.close()
    for options in ({}, {"background": "none"}, {"fit_background": False}, {"cells": [np.array([0, -1, 3, 2, 400])]}, {"max_iter": 0},
                    {"max_iter": 2, "max_step": 0.125, "max_shift": 0.2, "eps": 1e-2}):  # a DeviceArray frame
        on_host = rp.fit_positions(frame, start, psf, 2.5, box=16, **options)
        on_device = rp.fit_positions(rp.to_device(frame), start, psf, 2.5, box=16, **options)
        assert on_host[0].tobytes() == on_device[0].tobytes(), options
    frames = np.stack([frame, masked["frame"].astype(np.float32)])
    masks = [np.zeros(fc.SHAPE, bool), masked["mask"]]
    on_host = rp.fit_positions(frames, [start, start[:3]], psf, 3.5, masks, box=16)
    on_device = rp.fit_positions(rp.to_device(frames), [start, start[:3]], psf, 3.5, masks, box=16)
    assert [len(r) for r in on_host] == [5, 3] and all(a.tobytes() == b.tobytes() for a, b in zip(on_host, on_device))
    assert on_host[0].tobytes() == host[0].tobytes() and np.all(on_host[1]["coverage"] < 1.0)
    nothing = rp.fit_positions(rp.to_device(np.full(fc.SHAPE, np.nan, np.float32)), [start], psf, 3.5, box=16)[0]
    assert np.all(nothing["skipped"]) and np.all(nothing["no_mesh"]) and nothing["row"].tobytes() == start[:, 0].tobytes()
    again = rp.fit_stars(frame, host, psf, 3.5, box=16, cells=[host[0]["cell"]])[0]
    assert all(host[0]["fit_flags" if n == "flags" else n].tobytes() == again[n].tobytes() for n in again.dtype.names)
    assert rp.star_photometry(frame, host, [2.0, 3.0], box=16)[0]["row"].tobytes() == host[0]["row"].tobytes()
    assert rp.refine_stars(frame, host, 1.3, box=16)[0]["row0"].tobytes() == host[0]["row"].tobytes()
