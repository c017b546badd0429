"""Model fits (DESIGN.md 3.7 "Model fits", kernel S8) without a GPU: the kernel's driver (csrc/rpsf_core_stars_fit.hpp) on the CPU
emulator against the float64 restatement (tests/fit_cases.py), bit for bit - the cases and checks tests/test_gpu_fit.py runs on the GPU -
plus what is host code in the product: fit_stars, the cell choice, the derived fields, cell_fit_summary and the C ABI's return codes."""

import ctypes
import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import fit_cases as fc

NEW_SYMBOLS = ("rpsf_stars_model_create", "rpsf_stars_model_destroy", "rpsf_stars_fit", "rpsf_stars_fit_ms")
FAKE = 0x7F0000000000  # a handle nobody dereferences


@pytest.mark.parametrize("name", tuple(fc.GRID_CASES) + tuple(fc.MASKED_CASES) + tuple(fc.OTHER_CASES))
def test_the_fit_matches_the_restatement_bit_for_bit(name):
    fc.check_case(fc.EmuFinder, fc.EmuModel, name)


def test_every_flag_fires():
    fc.check_every_flag_fires(fc.EmuFinder, fc.EmuModel)


def test_hard_positions():
    fc.check_hard_positions(fc.EmuFinder, fc.EmuModel)


def test_row_counts_around_a_workgroup():
    fc.check_row_counts(fc.EmuFinder, fc.EmuModel, fc.emulator_info()[0])


@pytest.mark.parametrize("name", ("N = 16, mesh, flux and background", "masked, mesh, flux alone", "9 rows"))
def test_repeats_are_bit_equal(name):
    fc.check_reproducible(fc.EmuFinder, fc.EmuModel, name)


def test_detect_measure_photometry_and_refine_are_untouched():
    fc.check_isolation(fc.EmuFinder, fc.EmuModel)


def test_state_and_argument_errors():
    fc.check_errors(fc.EmuFinder, fc.EmuModel, fc.EmuError)


def test_the_records_fit_the_lds_of_a_plain_launch():
    """s8_lds_bytes(): what the kernel carves, the launch asks for and the emulator allocates.  256 lane records and 32 group records of
    six doubles, one 64-bit index and two ints, then two doubles and one int of state for each of the four waves, rounded up to 16 bytes."""
    waves, _, size = fc.emulator_info()
    assert waves == 4
    state = (waves * (2 * 8 + 4) + 15) // 16 * 16
    assert size == (256 + 8 * waves) * (6 * 8 + 8 + 2 * 4) + state == 18512 and size % 16 == 0 and size <= 64 * 1024


def test_the_ordered_sum_is_not_numpys():
    """The restatement's sums follow the kernel's order: on terms of mixed magnitude they differ from np.sum's pairwise order in the last
    places, and on a single lane they are the running sum."""
    rng = np.random.default_rng([10, 67])
    terms = rng.normal(0.0, 1.0, 700) * 10.0 ** rng.uniform(-8, 8, 700)
    ours = fc.ordered_sum(terms)
    assert abs(ours - np.sum(terms)) <= 700 * 2.0 ** -53 * np.abs(terms).sum()
    lane = np.zeros(64 * 5)
    lane[3::64] = terms[:5]
    running = np.float64(0.0)
    for t in terms[:5]:
        running = running + t
    assert fc.ordered_sum(lane) == running and fc.ordered_sum(np.zeros(0)) == 0.0


def test_the_definition_describes_the_stars_the_model_was_built_from():
    """The truth test: it pins h = N / 2 - 0.5, the builder's centre."""
    median, factor = fc.check_truth()
    # the figure the bound was fixed from (fit_cases.MEASURED_RESIDUAL), to its printed precision
    assert median <= fc.MEASURED_RESIDUAL and factor >= fc.DISPLACED_FACTOR


def test_the_truth_on_the_emulator_is_the_restatement(monkeypatch):
    """fit_stars on the truth's frames and model, the emulator behind it: the restatement's result, bit for bit."""
    monkeypatch.setattr(stars, "_Finder", fc.EmuFinder)
    monkeypatch.setattr(stars, "_Model", fc.EmuModel)
    t = fc.truth_case()
    coordinates, values = fc.oracle_model()
    got = rp.fit_stars(t["frames"], t["truth"], rp.IndexedCube(coordinates, values), fc.TRUTH_RADIUS, background="none", box=fc.BOX)
    want = fc.truth_fits(values, coordinates, 0.0)
    assert [len(g) for g in got] == [5, 5, 5] and np.concatenate(got).tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------------------------ host derivations
def _row(y, x, cell, flags, n, n_all, sums, f, bg, chi2, abs_res, peak):
    return np.array([[y, x, cell, flags, n, n_all, *sums, f, bg, chi2, abs_res, *peak]])


def test_derived_fields_on_hand_made_rows():
    # n = 6, Sm = 0.5, Sm_all = 0.625, f = -8, chi2 = 16, abs_res = 2: coverage 0.8, dof 4, rms 2, residual_fraction 2 / (8 * 0.5) = 0.5
    rows = _row(10.0, 20.0, 3, 0, 6, 9, [0.5, 0.625, 0.0625, 30.0, 4.0, 200.0], -8.0, 1.5, 16.0, 2.0, [1.25, -1.25, 11.0, 19.0])
    fit = stars.fit_from_sums(rows)
    assert fit.dtype == stars.fit_dtype() and fit.shape == (1,)
    row = fit[0]
    assert (row["row"], row["col"], row["cell"], row["flags"], row["n_use"], row["n_all"]) == (10.0, 20.0, 3, 0, 6, 9)
    assert (row["flux"], row["background"], row["coverage"], row["dof"], row["chi2"], row["rms"]) == (-8.0, 1.5, 0.8, 4, 16.0, 2.0)
    assert (row["abs_res"], row["residual_fraction"], row["peak_res"], row["peak_e"], row["peak_row"], row["peak_col"]) == (2.0, 0.5, 1.25, -1.25,
                                                                                                                       11.0, 19.0)
    assert (row["sm"], row["sm_all"], row["smm"], row["sd"], row["sdm"], row["sdd"]) == (0.5, 0.625, 0.0625, 30.0, 4.0, 200.0)
    assert not (row["no_mesh"] or row["too_few"] or row["degenerate"] or row["bad_cell"])
    alone = stars.fit_from_sums(rows, fit_background=False)[0]
    assert alone["dof"] == 5 and alone["rms"] == np.sqrt(16.0 / 5.0)
    nan = np.nan
    for n, with_background, dof in ((2, True, 0), (1, True, -1), (1, False, 0), (0, False, -1)):  # dof <= 0: rms NaN
        one = stars.fit_from_sums(_row(1.0, 1.0, 0, 0, n, 5, [1.0] * 6, 1.0, 0.0, 0.0, 0.0, [0.0, 0.0, 1.0, 1.0]), with_background)[0]
        assert one["dof"] == dof and np.isnan(one["rms"])
    for flags, names in ((1, ["no_mesh"]), (2, ["too_few"]), (4, ["degenerate"]), (8, ["bad_cell"]), (9, ["no_mesh", "bad_cell"])):
        one = stars.fit_from_sums(_row(1.0, 1.0, -1, flags, 0, 5, [nan] * 6, nan, nan, nan, nan, [nan, nan, -1.0, -1.0]))[0]
        assert [k for k in ("no_mesh", "too_few", "degenerate", "bad_cell") if one[k]] == names
        assert np.isnan(one["coverage"]) and np.isnan(one["rms"]) and np.isnan(one["residual_fraction"]) and one["peak_row"] == -1.0
    empty = stars.fit_from_sums(np.zeros((0, len(stars.FIT_COLUMNS))))
    assert empty.shape == (0,) and empty.dtype == stars.fit_dtype()


def test_the_cell_choice_against_a_brute_force_loop():
    rng = np.random.default_rng([11, 67])
    for shape, size in (((48, 40), 8), ((40, 48), 9), ((33, 70), 16)):
        coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering(shape, size)]
        positions = np.concatenate([rng.uniform(-10, max(shape) + 10, (300, 2)), np.array(coordinates[:40], np.float64) + size / 2,
                                    np.array(coordinates[5:25], np.float64) + size / 2 + [size / 4, 0.0]])  # on centres and between two
        got = stars.nearest_cells(positions, coordinates, size)
        assert got.dtype == np.int32 and got.shape == (len(positions),)
        ties = 0
        for (y, x), cell in zip(positions, got):
            best, best_d = -1, np.inf
            for k, (r, c) in enumerate(coordinates):
                cy, cx = np.float64(r) + size / 2, np.float64(c) + size / 2
                d = (y - cy) * (y - cy) + (x - cx) * (x - cx)
                ties += d == best_d
                if d < best_d:
                    best, best_d = k, d
            assert cell == best
        assert ties > 0
    # a star equidistant from two cell centres: the first cell in the cube's coordinate order wins, whichever that is
    for coordinates in ([(0, 0), (0, 8)], [(0, 8), (0, 0)]):
        assert stars.nearest_cells([(4.0, 8.0)], coordinates, 8).tolist() == [0]
    four = [(8, 0), (0, 0), (0, 8), (8, 8)]  # (8, 8) is equidistant from all four centres, (4, 8) from the second and the third
    assert stars.nearest_cells([(8.0, 8.0), (4.0, 8.0), (12.0, 8.0)], four, 8).tolist() == [0, 1, 0]
    assert stars.nearest_cells(np.zeros((0, 2)), [(0, 0)], 8).shape == (0,)
    many = stars.nearest_cells(rng.uniform(0, 4096, (5000, 2)), rp.calculate_covering((4096, 4096), 32), 32)  # in chunks
    assert many.shape == (5000,) and many.min() >= 0


def test_cell_fit_summary_on_hand_made_rows():
    psf = rp.IndexedCube([(0, 0), (0, 8), (8, 0), (8, 8)], np.zeros((4, 8, 8)))

    def fits(cells, flags, flux, rms, fraction):
        out = np.zeros(len(cells), stars.fit_dtype())
        out["cell"], out["flags"], out["flux"], out["rms"], out["residual_fraction"] = cells, flags, flux, rms, fraction
        return out

    one = fits([0, 0, 0, 2, 2, 3, 5, -1], [0, 0, 0, 0, 4, 2, 0, 8], [10.0, -20.0, 40.0, 8.0, 1.0, 1.0, 1.0, 1.0], [1.0, 4.0, 2.0, 2.0, 9.0, 9.0, 9.0, 9.0],
               [0.1, 0.3, 0.2, 0.5, 9.0, 9.0, 9.0, 9.0])
    got = stars.cell_fit_summary([one], psf)
    assert got.dtype == stars.CELL_FIT_DTYPE and got.shape == (4,) and rp.cell_fit_summary is stars.cell_fit_summary
    assert got["count"].tolist() == [3, 0, 1, 0]  # flagged stars and stars of no cell of the model do not count
    assert got["residual_fraction"][[0, 2]].tolist() == [0.2, 0.5] and got["flux"][[0, 2]].tolist() == [10.0, 8.0]
    assert got["relative_rms"][[0, 2]].tolist() == [0.1, 0.25]  # the median of 1 / 10, 4 / 20, 2 / 40
    for name in ("residual_fraction", "relative_rms", "flux"):
        assert np.isnan(got[name][[1, 3]]).all()
    two = stars.cell_fit_summary([one[:3], one[3:], one[:0]], psf)  # the frames are pooled
    assert two.tobytes() == got.tobytes() and stars.cell_fit_summary(one, psf).tobytes() == got.tobytes()
    nothing = stars.cell_fit_summary([], psf)
    assert nothing["count"].tolist() == [0] * 4 and np.isnan(nothing["flux"]).all()


# ------------------------------------------------------------------------------------------------------------------ Python surface
def test_fit_stars_is_exported_and_says_what_it_is_not():
    assert "fit_stars" in rp.__all__ and rp.fit_stars is stars.fit_stars and "cell_fit_summary" in rp.__all__
    parameters = inspect.signature(rp.fit_stars).parameters
    assert list(parameters) == ["images", "stars", "psf", "radius", "mask", "background", "box", "fit_background", "cells", "device"]
    assert [parameters[n].default for n in ("mask", "background", "box", "fit_background", "cells", "device")] == [None, "mesh", 64, True, None, 0]
    assert all(parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("background", "box", "fit_background", "cells", "device"))
    for text in (stars.fit_stars.__doc__, stars.__doc__):
        assert "NOT a PSF-photometry" in text and "uniform" in text and "no error column" in text and "variance weighting" in text
        assert "not fitted" in text and "bilinear" in text and "does not conserve flux" in text and "not corrected for" in text
    dtype = stars.fit_dtype()
    assert dtype.names == stars.FIT_FIELDS and dtype.names[:6] == ("row", "col", "cell", "flags", "flux", "background")
    assert all(dtype[n] == np.int32 for n in ("cell", "flags", "n_use", "n_all", "dof"))
    assert all(dtype[n] == np.bool_ for n in ("no_mesh", "too_few", "degenerate", "bad_cell"))
    assert len(stars.FIT_COLUMNS) == fc.COLUMNS and (stars.NO_MESH, stars.TOO_FEW, stars.DEGENERATE, stars.BAD_CELL) == (1, 2, 4, 8)


def test_fit_stars_on_the_emulator(monkeypatch):
    """fit_stars with the emulator behind it: stars as positions and as catalogues, the forms of psf and cells, and its place after
    refine_stars."""
    monkeypatch.setattr(stars, "_Finder", fc.EmuFinder)
    monkeypatch.setattr(stars, "_Model", fc.EmuModel)
    frame, truth = fc.field()["frame"], fc.field()["truth"]
    coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering(fc.SHAPE, 8)]
    cube = np.broadcast_to(fc.model(8)[fc.GAUSSIAN], (len(coordinates), 8, 8)).copy()
    psf = rp.IndexedCube(coordinates, cube)
    one = rp.fit_stars(frame, truth, psf, 3.0, box=16)
    assert isinstance(one, list) and len(one) == 1 and one[0].dtype == stars.fit_dtype() and one[0].shape == (5,)
    cells = stars.nearest_cells(truth, coordinates, 8)
    assert one[0]["cell"].tolist() == cells.tolist() and np.all(one[0]["flags"] == 0) and np.all(one[0]["coverage"] == 1.0)
    finder, model = fc.EmuFinder(frame.shape, 16), fc.EmuModel(cube)
    finder.background_device(frame, None)
    assert one[0].tobytes() == stars.fit_from_sums(finder.fit(model, truth, cells, 3.0)).tobytes()
    finder.close()
    # sigma 1.3 on both sides; the model is cut at 8 x 8 and bilinear interpolation flattens its peak, by up to 1 / (8 sigma^2) = 7 % per
    # axis at the worst phase, which the flux makes up for: a sanity check of the composition, not a bound on the kernel
    assert np.all(np.abs(one[0]["flux"] / (2 * np.pi * 1.3 ** 2 * np.array([400.0, 250.0, 300.0, 150.0, 500.0])) - 1) < 0.25)
    assert np.all(one[0]["residual_fraction"] < 0.1) and np.all(one[0]["dof"] == one[0]["n_use"] - 2)
    for form in ([truth], [truth.tolist()], np.ascontiguousarray(truth)):
        assert rp.fit_stars(frame, form, psf, 3.0, box=16)[0].tobytes() == one[0].tobytes()
    assert rp.fit_stars(frame, truth, rp.ArrayPSF(psf), 3.0, box=16)[0].tobytes() == one[0].tobytes()  # an ArrayPSF
    assert rp.fit_stars(frame, truth, rp.IndexedCube(coordinates, cube.astype(np.float32)), 3.0, box=16)[0]["cell"].tolist() == cells.tolist()
    for form in (cells, [cells], [cells.astype(np.int64)], [cells.tolist()]):
        assert rp.fit_stars(frame, truth, psf, 3.0, box=16, cells=form)[0].tobytes() == one[0].tobytes()
    other = rp.fit_stars(frame, truth, psf, 3.0, box=16, cells=[[0, -1, len(coordinates), 1, 2]])[0]
    assert other["cell"].tolist() == [0, -1, len(coordinates), 1, 2] and other["bad_cell"].tolist() == [False, True, True, False, False]
    refined = rp.refine_stars(frame, np.rint(truth), 1.3, box=16)  # refine_stars' output is taken by row / col
    after = rp.fit_stars(frame, refined, psf, 3.0, box=16)[0]
    assert after["row"].tobytes() == refined[0]["row"].tobytes() and np.all(after["residual_fraction"] < 0.1)
    cat = rp.star_catalog(frame, box=16)
    assert rp.fit_stars(frame, cat, psf, 3.0, box=16)[0]["row"].tobytes() == cat[0]["row"].tobytes()
    alone = rp.fit_stars(frame, truth, psf, 3.0, box=16, fit_background=False)[0]
    assert np.all(alone["background"] == 0.0) and np.all(alone["dof"] == alone["n_use"] - 1) and alone["flux"].tobytes() != one[0]["flux"].tobytes()
    none = rp.fit_stars(frame, truth, psf, 3.0, box=16, background="none")[0]
    assert np.all(none["background"] > one[0]["background"] + 5.0)  # the background of 10 is still in, and the constant takes it
    masked = fc.masked_field()
    both = rp.fit_stars([frame, masked["frame"]], [truth, truth[:3]], psf, 3.0, [np.zeros(fc.SHAPE, bool), masked["mask"]], box=16)
    assert [len(b) for b in both] == [5, 3] and both[0].tobytes() == one[0].tobytes() and np.all(both[1]["coverage"] < 1.0)
    stack = rp.fit_stars(np.stack([frame, frame]), [truth, truth[:0]], psf, 3.0, box=16)
    assert stack[0].tobytes() == one[0].tobytes() and stack[1].shape == (0,) and stack[1].dtype == stars.fit_dtype()
    off = rp.fit_stars(frame, [[(-50.0, -50.0)]], psf, 3.0, box=16)[0]
    assert off["too_few"][0] and off["coverage"][0] == 0.0 and np.isnan(off["flux"][0]) and off["cell"][0] >= 0
    summary = rp.cell_fit_summary(both, psf)
    assert summary.shape == (len(coordinates),) and summary["count"].sum() == int((np.concatenate(both)["flags"] == 0).sum())
    assert np.isnan(summary["flux"][summary["count"] == 0]).all() and np.all(summary["residual_fraction"][summary["count"] > 0] > 0)


def test_argument_errors():
    frame, stars_ = np.zeros((40, 48), np.float32), [np.array([[10.0, 12.0]])]
    psf = rp.IndexedCube([(0, 0)], np.ones((1, 8, 8)))
    for radius in (0.0, -1.0, 3.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="radius must lie in 0 < R <= min\\(64, N / 2 - 1\\) = 3 for cells of 8"):
            rp.fit_stars(frame, stars_, psf, radius)
    with pytest.raises(ValueError, match="= 64 for cells of 256"):
        rp.fit_stars(frame, stars_, rp.IndexedCube([(0, 0)], np.ones((1, 256, 256))), 64.5)
    with pytest.raises(TypeError, match="radius must be a number"):
        rp.fit_stars(frame, stars_, psf, "wide")
    for bad in (rp.IndexedCube([(0, 0)], np.ones((1, 3, 3))), rp.IndexedCube([(0, 0)], np.ones((1, 8, 9))),
                rp.IndexedCube([(0, 0)], np.ones((1, 257, 257))), rp.IndexedCube([], np.ones((0, 8, 8)))):
        with pytest.raises(rp.IncorrectShapeError, match="the model must be a cube"):
            rp.fit_stars(frame, stars_, bad, 1.0)
    with pytest.raises(TypeError, match="the model's values must be real"):
        rp.fit_stars(frame, stars_, rp.IndexedCube([(0, 0)], np.ones((1, 8, 8), np.complex128)), 1.0)
    with pytest.raises(TypeError, match="psf must be an ArrayPSF or an IndexedCube"):
        rp.fit_stars(frame, stars_, np.ones((1, 8, 8)), 1.0)
    for fit_background in (1, "yes", None):
        with pytest.raises(TypeError, match="fit_background must be True or False"):
            rp.fit_stars(frame, stars_, psf, 1.0, fit_background=fit_background)
    with pytest.raises(ValueError, match='background must be "mesh" or "none"'):
        rp.fit_stars(frame, stars_, psf, 1.0, background="annulus")
    with pytest.raises(ValueError, match="box must lie in 8 ... 128"):
        rp.fit_stars(frame, stars_, psf, 1.0, box=4)
    with pytest.raises(ValueError, match="stars has 2 entries for 1 frames"):
        rp.fit_stars(frame, stars_ * 2, psf, 1.0)
    for bad in (np.nan, np.inf, 2.0 ** 20, -2.0 ** 20):
        with pytest.raises(ValueError, match="not finite or not inside"):
            rp.fit_stars(frame, [np.array([[10.0, bad]])], psf, 1.0)
    with pytest.raises(ValueError, match="cells has 2 entries for 1 frames"):
        rp.fit_stars(frame, stars_, psf, 1.0, cells=[[0], [0]])
    with pytest.raises(ValueError, match="cells\\[0\\] has shape \\(2,\\) for the 1 stars"):
        rp.fit_stars(frame, stars_, psf, 1.0, cells=[[0, 0]])
    with pytest.raises(TypeError, match="cells\\[0\\] must be integers"):
        rp.fit_stars(frame, stars_, psf, 1.0, cells=[[0.5]])
    with pytest.raises(ValueError, match="outside int32"):
        rp.fit_stars(frame, stars_, psf, 1.0, cells=[[2 ** 40]])


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_exist_and_are_in_the_table():
    lib = _native.lib()
    header = (fc.ROOT / "include" / "rpsf.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in _native._PROTOTYPES and getattr(lib, name).argtypes is not None
        assert f" {name}(" in header
    assert "#define RPSF_STARS_FIT_COLUMNS 20\n" in header
    for name, value in (("NO_MESH", 1), ("TOO_FEW", 2), ("DEGENERATE", 4), ("BAD_CELL", 8)):
        assert f"#define RPSF_STARS_FIT_{name} {value}\n" in header


def test_new_entry_points_check_their_arguments_before_the_handles():
    lib = _native.lib()
    fake, fake_model = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + 4096)  # must not be looked at before the other arguments are
    pos, cells, out, ms = np.array([[3.0, 4.0]]), np.array([0], np.int32), np.full(fc.COLUMNS, -1.0), ctypes.c_double(-1.0)
    p, c, o = _native._ptr(pos), _native._ptr(cells), _native._ptr(out)
    cube, handle = np.ones((1, 8, 8)), ctypes.c_void_p()
    calls = [
        lib.rpsf_stars_fit(None, fake_model, 1, p, c, 2.0, 1, 1, o),
        lib.rpsf_stars_fit(fake, None, 1, p, c, 2.0, 1, 1, o),
        lib.rpsf_stars_fit(None, None, 0, None, None, 2.0, 1, 1, None),
        lib.rpsf_stars_fit(fake, fake_model, 1, None, c, 2.0, 1, 1, o),
        lib.rpsf_stars_fit(fake, fake_model, 1, p, None, 2.0, 1, 1, o),
        lib.rpsf_stars_fit(fake, fake_model, 1, p, c, 2.0, 1, 1, None),
        *(lib.rpsf_stars_fit(fake, fake_model, 1, p, c, radius, 1, 1, o) for radius in (0.0, -2.0, 64.5, np.nan, np.inf)),
        lib.rpsf_stars_fit(fake, fake_model, 0, None, None, 0.0, 1, 1, None),
        *(lib.rpsf_stars_fit(fake, fake_model, 1, p, c, 2.0, fit_background, 1, o) for fit_background in (2, -1)),
        *(lib.rpsf_stars_fit(fake, fake_model, 1, _native._ptr(np.array([[3.0, bad]])), c, 2.0, 0, 0, o)
          for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20)),
        lib.rpsf_stars_fit_ms(None, ctypes.byref(ms)),
        lib.rpsf_stars_fit_ms(fake, None),
        lib.rpsf_stars_model_create(0, 1, 8, _native._ptr(cube), None),
        lib.rpsf_stars_model_create(0, 1, 8, None, ctypes.byref(handle)),
        lib.rpsf_stars_model_create(0, 0, 8, _native._ptr(cube), ctypes.byref(handle)),
        lib.rpsf_stars_model_create(0, 2 ** 24 + 1, 8, _native._ptr(cube), ctypes.byref(handle)),
        *(lib.rpsf_stars_model_create(0, 1, n, _native._ptr(cube), ctypes.byref(handle)) for n in (3, 257, 0, -8)),
    ]
    assert calls == [_native.E_BADARG] * len(calls)
    assert np.all(out == -1.0) and ms.value == -1.0 and not handle.value
    lib.rpsf_stars_model_destroy(None)  # nothing to destroy is not an error
