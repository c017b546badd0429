"""Fitted positions (DESIGN.md 3.7 "Fitted positions", kernel S9) without a GPU: the kernel's driver (csrc/rpsf_core_stars_fitpos.hpp) on
the CPU emulator against the float64 restatement (tests/fitpos_cases.py), bit for bit - the cases and checks tests/test_gpu_fitpos.py runs
on the GPU - plus what is host code in the product: fit_positions, the derived fields and the C ABI's return codes."""

import ctypes
import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import fit_cases as fc
from tests import fitpos_cases as fp

NEW_SYMBOLS = ("rpsf_stars_fit_positions", "rpsf_stars_fit_positions_ms")
FAKE = 0x7F0000000000  # a handle nobody dereferences


@pytest.mark.parametrize("name", tuple(fp.GRID_CASES) + tuple(fp.MASKED_CASES) + tuple(fp.OTHER_CASES))
def test_the_iteration_matches_the_restatement_and_the_fit_row_is_s8s(name):
    fp.check_case(fp.EmuFinder, fp.EmuModel, name)


def test_without_iterations_both_outputs_are_the_plain_fit():
    fp.check_no_iteration(fp.EmuFinder, fp.EmuModel)


def test_every_stop_rule():
    fp.check_every_stop_rule(fp.EmuFinder, fp.EmuModel)


def test_row_counts_around_a_workgroup():
    fp.check_row_counts(fp.EmuFinder, fp.EmuModel, fp.emulator_info()[0])


@pytest.mark.parametrize("name", ("N = 16, mesh, flux and background", "masked, mesh, flux alone", "9 rows"))
def test_repeats_are_bit_equal(name):
    fp.check_reproducible(fp.EmuFinder, fp.EmuModel, name)


def test_the_other_kernels_are_untouched_and_a_model_serves_two_finders():
    fp.check_isolation(fp.EmuFinder, fp.EmuModel)


def test_state_and_argument_errors():
    fp.check_errors(fp.EmuFinder, fp.EmuModel, fp.EmuError)


def test_the_records_fit_the_lds_of_a_plain_launch():
    """s9_lds_bytes(): what the kernel carves, the launch asks for and the emulator allocates.  256 lane records and 32 group records of
    thirteen doubles and one int, then four doubles and three ints of state for each of the four waves, rounded up to 16 bytes."""
    waves, _, size = fp.emulator_info()
    assert waves == 4
    state = (waves * (4 * 8 + 3 * 4) + 15) // 16 * 16
    assert size == (256 + 8 * waves) * (13 * 8 + 4) + state == 31280 and size % 16 == 0 and size <= 64 * 1024


def test_the_elimination_against_numpy():
    """ref_solve is the definition's elimination: on well-conditioned symmetric positive definite systems it agrees with numpy.linalg.solve
    to rounding, and it refuses a pivot that is zero, negative or not finite."""
    rng = np.random.default_rng([12, 67])
    for k in (3, 4):
        for _ in range(20):
            m = rng.normal(size=(k + 3, k))
            a, b = m.T @ m, rng.normal(size=k)
            upper = [[a[i, j] if j >= i else None for j in range(k)] for i in range(k)]
            got = np.array(fp.ref_solve(upper, list(b)))
            assert np.allclose(got, np.linalg.solve(a, b), rtol=1e-9, atol=1e-12)
    assert fp.ref_solve([[0.0, 1.0, 1.0], [None, 1.0, 0.0], [None, None, 1.0]], [1.0, 1.0, 1.0]) is None
    assert fp.ref_solve([[1.0, 2.0, 0.0], [None, 1.0, 0.0], [None, None, 1.0]], [1.0, 1.0, 1.0]) is None  # the second pivot is 1 - 4
    assert fp.ref_solve([[np.nan, 0.0, 0.0], [None, 1.0, 0.0], [None, None, 1.0]], [1.0, 1.0, 1.0]) is None
    assert fp.ref_solve([[np.inf, 0.0, 0.0], [None, 1.0, 0.0], [None, None, 1.0]], [1.0, 1.0, 1.0]) is None


def test_the_gradient_is_the_interpolants_derivative():
    """g_u and g_v against central differences of fit_cases.ref_model inside one cell of the grid, where the interpolant is bilinear:
    (m(u + e) - m(u - e)) / 2 e is its derivative up to rounding."""
    cell = fc.model(9)[fc.LOBES]
    pr, pc_ = np.array([-2.3, -0.75, 0.2, 1.6]), np.array([-1.4, 0.3, 2.45])
    inside = np.ones((4, 3), bool)
    m, gu, gv = fp.ref_sample(cell, pr, pc_, inside)
    assert fc.same_bits(m, fc.ref_model(cell, pr, pc_, inside))
    e = 2.0 ** -12
    du = (fc.ref_model(cell, pr + e, pc_, inside) - fc.ref_model(cell, pr - e, pc_, inside)) / (2 * e)
    dv = (fc.ref_model(cell, pr, pc_ + e, inside) - fc.ref_model(cell, pr, pc_ - e, inside)) / (2 * e)
    assert np.allclose(gu, du, rtol=0, atol=1e-10) and np.allclose(gv, dv, rtol=0, atol=1e-10)


def test_the_definition_finds_the_stars_the_model_was_built_from():
    """The truth test on the restatement alone."""
    figures = fp.check_truth()
    # the figures the bounds were fixed from (fitpos_cases.MEASURED_*), to their printed precision
    assert figures["worst"] <= fp.MEASURED_WORST_DISTANCE and figures["median"] <= fp.MEASURED_MEDIAN_DISTANCE
    assert figures["residual"] <= fp.MEASURED_RESIDUAL and figures["niter"] == fp.MEASURED_NITER


def test_the_truth_on_the_emulator_is_the_restatement(monkeypatch):
    """fit_positions on the truth's frames and model, the emulator behind it: the restatement's result, byte for byte, and the bounds."""
    monkeypatch.setattr(stars, "_Finder", fp.EmuFinder)
    monkeypatch.setattr(stars, "_Model", fp.EmuModel)
    coordinates, values = fc.oracle_model()
    for offset in fp.TRUTH_STARTS:
        got = fp.truth_rows(values, coordinates, offset, rp.fit_positions)
        want = fp.truth_rows(values, coordinates, offset)
        assert [len(g) for g in got] == [5, 5, 5] and np.concatenate(got).tobytes() == np.concatenate(want).tobytes()
    fp.check_truth(what="the oracle's model, the emulator", fit_positions=rp.fit_positions)


# ------------------------------------------------------------------------------------------------------------------ host derivations
def test_derived_fields_on_hand_made_rows():
    steps = np.array([[10.5, 20.5, 10.25, 20.75, 3, 0, -1e-5, 2e-5], [1.0, 2.0, 1.0, 2.0, 0, 8, np.nan, np.nan], [1.0, 2.0, 1.5, 2.0, 1, 1, 0.5, 0.1],
                      [1.0, 2.0, 1.0, 2.0, 0, 4, np.nan, np.nan], [1.0, 2.0, 1.1, 2.1, 2, 2, 0.01, 0.01], [1.0, 2.0, 1.0, 2.0, 0, 0, np.nan, np.nan]])
    fits = np.zeros((6, fc.COLUMNS))
    fits[:, fc.Y:fc.X + 1], fits[:, fc.CELL], fits[:, fc.FLAGS], fits[:, fc.N_USE], fits[:, fc.F] = steps[:, 2:4], 3, [0, 8, 0, 4, 0, 0], 9, 7.0
    got = stars.fitpos_from_sums(steps, fits)
    assert got.dtype == stars.fitpos_dtype() and got.shape == (6,) and got.dtype.names == stars.FITPOS_FIELDS
    assert got.dtype.names[:13] == ("row", "col", "row0", "col0", "niter", "flags", "converged", "step_row", "step_col", "ran_away", "not_converged",
                                    "singular", "skipped")
    assert got.dtype.names[13:] == tuple("fit_flags" if n == "flags" else n for n in stars.FIT_FIELDS if n not in ("row", "col"))
    assert all(got.dtype[n] == np.int32 for n in ("niter", "flags", "fit_flags", "cell", "n_use", "dof"))
    assert all(got.dtype[n] == np.bool_ for n in ("converged", "ran_away", "not_converged", "singular", "skipped", "no_mesh", "bad_cell"))
    assert (got["row"][0], got["col"][0], got["row0"][0], got["col0"][0], got["niter"][0], got["step_row"][0]) == (10.25, 20.75, 10.5, 20.5, 3, -1e-5)
    assert got["converged"].tolist() == [True, False, False, False, False, False]  # (max_iter = 0 leaves no flag and no step: not converged)
    assert got["skipped"].tolist() == [False, True, False, False, False, False] and got["ran_away"].tolist() == [False, False, True, False, False, False]
    assert got["singular"].tolist() == [False, False, False, True, False, False] and got["not_converged"].tolist() == [False] * 4 + [True, False]
    assert got["fit_flags"].tolist() == [0, 8, 0, 4, 0, 0] and got["bad_cell"].tolist() == [False, True] + [False] * 4 and np.all(got["flux"] == 7.0)
    fit = stars.fit_from_sums(fits)
    assert all(got["fit_flags" if n == "flags" else n].tobytes() == fit[n].tobytes() for n in fit.dtype.names)
    assert np.all(stars.fitpos_from_sums(steps, fits, fit_background=False)["dof"] == 8)
    empty = stars.fitpos_from_sums(np.zeros((0, len(stars.FITPOS_COLUMNS))), np.zeros((0, fc.COLUMNS)))
    assert empty.shape == (0,) and empty.dtype == stars.fitpos_dtype()
    with pytest.raises(ValueError, match="5 fit rows for 6 iteration rows"):
        stars.fitpos_from_sums(steps, fits[:5])


# ------------------------------------------------------------------------------------------------------------------ Python surface
def test_fit_positions_is_exported_and_says_what_it_is_not():
    assert "fit_positions" in rp.__all__ and rp.fit_positions is stars.fit_positions
    parameters = inspect.signature(rp.fit_positions).parameters
    assert list(parameters) == ["images", "stars", "psf", "radius", "mask", "background", "box", "fit_background", "cells", "max_iter", "eps",
                                "max_shift", "max_step", "device"]
    names = ("mask", "background", "box", "fit_background", "cells", "max_iter", "eps", "max_shift", "max_step", "device")
    assert [parameters[n].default for n in names] == [None, "mesh", 64, True, None, 16, 1e-4, 2.0, 0.5, 0]
    assert all(parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[1:])
    fit_stars = inspect.signature(rp.fit_stars).parameters  # it takes exactly what fit_stars takes, and the iteration's four
    assert [n for n in parameters if n not in ("max_iter", "eps", "max_shift", "max_step")] == list(fit_stars)
    text = stars.fit_positions.__doc__
    for words in ("NOT a PSF-photometry", "uniform", "no error column", "bilinear", "cell is fixed", "one star is fitted at a time",
                  "neighbours are not fitted together", "not corrected for"):
        assert words in text, words
    assert "fit_positions" in stars.__doc__ and "one star is fitted at a time" in stars.__doc__
    assert len(stars.FITPOS_COLUMNS) == fp.COLUMNS
    assert (stars.FITPOS_RAN_AWAY, stars.FITPOS_NOT_CONVERGED, stars.FITPOS_SINGULAR, stars.FITPOS_SKIPPED) == (1, 2, 4, 8)


def test_fit_positions_on_the_emulator_and_what_takes_its_result(monkeypatch):
    """fit_positions with the emulator behind it: the forms of stars, psf and cells, and its result in fit_stars, refine_stars,
    star_photometry and the builder's star list."""
    from regularizepsf_amd import builder as bld

    monkeypatch.setattr(stars, "_Finder", fp.EmuFinder)
    monkeypatch.setattr(stars, "_Model", fp.EmuModel)
    frame, truth = fc.field()["frame"], fc.field()["truth"]
    start = truth + (0.3, -0.2)
    coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering(fc.SHAPE, 8)]
    cube = np.broadcast_to(fc.model(8)[fc.GAUSSIAN], (len(coordinates), 8, 8)).copy()
    psf = rp.IndexedCube(coordinates, cube)
    one = rp.fit_positions(frame, start, psf, 3.0, box=16)
    assert isinstance(one, list) and len(one) == 1 and one[0].dtype == stars.fitpos_dtype() and one[0].shape == (5,)
    cells = stars.nearest_cells(start, coordinates, 8)  # chosen once, at the input
    assert one[0]["cell"].tolist() == cells.tolist() and np.all(one[0]["converged"]) and np.all(one[0]["fit_flags"] == 0)
    assert one[0]["row0"].tobytes() == start[:, 0].tobytes() and one[0]["col0"].tobytes() == start[:, 1].tobytes()
    # sigma 1.3 on both sides and noise of 0.3 under amplitudes of 150 ... 500: a sanity check of the composition, not a bound on the kernel
    assert np.all(np.hypot(one[0]["row"] - truth[:, 0], one[0]["col"] - truth[:, 1]) < 0.05)
    finder, model = fp.EmuFinder(frame.shape, 16), fp.EmuModel(cube)
    finder.background_device(frame, None)
    assert one[0].tobytes() == stars.fitpos_from_sums(*finder.fit_positions(model, start, cells, 3.0)).tobytes()
    finder.close()
    for form in ([start], [start.tolist()], np.ascontiguousarray(start)):
        assert rp.fit_positions(frame, form, psf, 3.0, box=16)[0].tobytes() == one[0].tobytes()
    assert rp.fit_positions(frame, start, rp.ArrayPSF(psf), 3.0, box=16)[0].tobytes() == one[0].tobytes()
    for form in (cells, [cells], [cells.astype(np.int64)], [cells.tolist()]):
        assert rp.fit_positions(frame, start, psf, 3.0, box=16, cells=form)[0].tobytes() == one[0].tobytes()
    other = rp.fit_positions(frame, start, psf, 3.0, box=16, cells=[[0, -1, len(coordinates), 1, 2]])[0]
    assert other["skipped"].tolist() == [False, True, True, False, False] and other["bad_cell"].tolist() == other["skipped"].tolist()
    still = rp.fit_positions(frame, start, psf, 3.0, box=16, max_iter=0)[0]
    assert still["row"].tobytes() == start[:, 0].tobytes() and not still["converged"].any() and np.all(still["flags"] == 0)
    plain = rp.fit_stars(frame, start, psf, 3.0, box=16)[0]
    assert all(still["fit_flags" if n == "flags" else n].tobytes() == plain[n].tobytes() for n in plain.dtype.names)
    capped = rp.fit_positions(frame, start, psf, 3.0, box=16, max_iter=1, max_step=0.125)[0]
    assert np.all(capped["not_converged"]) and np.all(capped["niter"] == 1) and np.all(np.abs(capped["step_row"]) <= 0.125)
    alone = rp.fit_positions(frame, start, psf, 3.0, box=16, fit_background=False)[0]
    assert np.all(alone["background"] == 0.0) and np.all(alone["dof"] == alone["n_use"] - 1)
    # (the star on a pixel centre may end in a cycle of a few thousandths of a pixel across a kink of the interpolant: DESIGN.md 3.7)
    assert np.all(alone["flags"] & ~stars.FITPOS_NOT_CONVERGED == 0) and alone["converged"].sum() >= 4
    assert np.all(np.hypot(alone["row"] - one[0]["row"], alone["col"] - one[0]["col"]) < 0.02)
    # composition: fit_stars at the fitted positions gives the fit fields bit for bit
    again = rp.fit_stars(frame, one, psf, 3.0, box=16)[0]
    assert again["cell"].tolist() == cells.tolist()  # (no star crossed into another cell: the default choice is the same)
    assert all(one[0]["fit_flags" if n == "flags" else n].tobytes() == again[n].tobytes() for n in again.dtype.names)
    again = rp.fit_stars(frame, one[0], psf, 3.0, box=16, cells=one[0]["cell"])[0]
    assert all(one[0]["fit_flags" if n == "flags" else n].tobytes() == again[n].tobytes() for n in again.dtype.names)
    assert rp.refine_stars(frame, one, 1.3, box=16)[0]["row0"].tobytes() == one[0]["row"].tobytes()
    assert rp.star_photometry(frame, one, [2.0, 3.0], box=16)[0]["row"].tobytes() == one[0]["row"].tobytes()
    assert rp.fit_positions(frame, one, psf, 3.0, box=16)[0]["row0"].tobytes() == one[0]["row"].tobytes()
    # the builder's star list takes the result by row / col
    assert bld.star_positions(one[0]).tobytes() == np.stack([one[0]["row"], one[0]["col"]], axis=-1).tobytes()
    masked = fc.masked_field()
    both = rp.fit_positions([frame, masked["frame"]], [start, start[:3]], psf, 3.0, [np.zeros(fc.SHAPE, bool), masked["mask"]], box=16)
    assert [len(b) for b in both] == [5, 3] and both[0].tobytes() == one[0].tobytes() and np.all(both[1]["coverage"] < 1.0)
    stack = rp.fit_positions(np.stack([frame, frame]), [start, start[:0]], psf, 3.0, box=16)
    assert stack[0].tobytes() == one[0].tobytes() and stack[1].shape == (0,) and stack[1].dtype == stars.fitpos_dtype()
    off = rp.fit_positions(frame, [[(-50.0, -50.0)]], psf, 3.0, box=16)[0]
    assert off["singular"][0] and off["too_few"][0] and off["niter"][0] == 0 and off["row"][0] == -50.0


def test_argument_errors():
    frame, stars_ = np.zeros((40, 48), np.float32), [np.array([[10.0, 12.0]])]
    psf = rp.IndexedCube([(0, 0)], np.ones((1, 8, 8)))
    # fit_stars' own, word for word
    for radius in (0.0, -1.0, 3.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="radius must lie in 0 < R <= min\\(64, N / 2 - 1\\) = 3 for cells of 8"):
            rp.fit_positions(frame, stars_, psf, radius)
    with pytest.raises(TypeError, match="radius must be a number"):
        rp.fit_positions(frame, stars_, psf, "wide")
    with pytest.raises(rp.IncorrectShapeError, match="the model must be a cube"):
        rp.fit_positions(frame, stars_, rp.IndexedCube([(0, 0)], np.ones((1, 3, 3))), 1.0)
    with pytest.raises(TypeError, match="the model's values must be real"):
        rp.fit_positions(frame, stars_, rp.IndexedCube([(0, 0)], np.ones((1, 8, 8), np.complex128)), 1.0)
    with pytest.raises(TypeError, match="psf must be an ArrayPSF or an IndexedCube"):
        rp.fit_positions(frame, stars_, np.ones((1, 8, 8)), 1.0)
    for fit_background in (1, "yes", None):
        with pytest.raises(TypeError, match="fit_background must be True or False"):
            rp.fit_positions(frame, stars_, psf, 1.0, fit_background=fit_background)
    with pytest.raises(ValueError, match='background must be "mesh" or "none"'):
        rp.fit_positions(frame, stars_, psf, 1.0, background="annulus")
    with pytest.raises(ValueError, match="box must lie in 8 ... 128"):
        rp.fit_positions(frame, stars_, psf, 1.0, box=4)
    with pytest.raises(ValueError, match="stars has 2 entries for 1 frames"):
        rp.fit_positions(frame, stars_ * 2, psf, 1.0)
    for bad in (np.nan, np.inf, 2.0 ** 20, -2.0 ** 20):
        with pytest.raises(ValueError, match="not finite or not inside"):
            rp.fit_positions(frame, [np.array([[10.0, bad]])], psf, 1.0)
    with pytest.raises(ValueError, match="cells has 2 entries for 1 frames"):
        rp.fit_positions(frame, stars_, psf, 1.0, cells=[[0], [0]])
    with pytest.raises(ValueError, match="cells\\[0\\] has shape \\(2,\\) for the 1 stars"):
        rp.fit_positions(frame, stars_, psf, 1.0, cells=[[0, 0]])
    with pytest.raises(TypeError, match="cells\\[0\\] must be integers"):
        rp.fit_positions(frame, stars_, psf, 1.0, cells=[[0.5]])
    with pytest.raises(ValueError, match="outside int32"):
        rp.fit_positions(frame, stars_, psf, 1.0, cells=[[2 ** 40]])
    # the iteration's, as refine_stars says them
    for max_iter in (1.0, True, "3", None):
        with pytest.raises(TypeError, match="max_iter must be an integer"):
            rp.fit_positions(frame, stars_, psf, 1.0, max_iter=max_iter)
    for max_iter in (-1, 65):
        with pytest.raises(ValueError, match="max_iter must lie in 0 ... 64"):
            rp.fit_positions(frame, stars_, psf, 1.0, max_iter=max_iter)
    for eps in (0.0, -1e-4, np.nan, np.inf):
        with pytest.raises(ValueError, match="eps must be positive and finite"):
            rp.fit_positions(frame, stars_, psf, 1.0, eps=eps)
    for name in ("max_shift", "max_step"):
        for value in (0.0, -1.0, 64.5, np.nan, np.inf):
            with pytest.raises(ValueError, match=f"{name} must lie in 0 < {name} <= 64"):
                rp.fit_positions(frame, stars_, psf, 1.0, **{name: value})


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_exist_and_are_in_the_table():
    lib = _native.lib()
    header = (fc.ROOT / "include" / "rpsf.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in _native._PROTOTYPES and getattr(lib, name).argtypes is not None
        assert f" {name}(" in header
    assert "#define RPSF_STARS_FITPOS_COLUMNS 8\n" in header and "#define RPSF_STARS_FIT_COLUMNS 20\n" in header
    for name, value in (("RAN_AWAY", 1), ("NOT_CONVERGED", 2), ("SINGULAR", 4), ("SKIPPED", 8)):
        assert f"#define RPSF_STARS_FITPOS_{name} {value}\n" in header


def test_new_entry_points_check_their_arguments_before_the_handles():
    lib = _native.lib()
    fake, fake_model = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + 4096)  # must not be looked at before the other arguments are
    pos, cells, ms = np.array([[3.0, 4.0]]), np.array([0], np.int32), ctypes.c_double(-1.0)
    steps, fits = np.full(fp.COLUMNS, -1.0), np.full(fc.COLUMNS, -1.0)
    p, c, o, f = _native._ptr(pos), _native._ptr(cells), _native._ptr(steps), _native._ptr(fits)
    call = lib.rpsf_stars_fit_positions
    calls = [
        call(None, fake_model, 1, p, c, 2.0, 1, 16, 1e-4, 2.0, 0.5, 1, o, f),
        call(fake, None, 1, p, c, 2.0, 1, 16, 1e-4, 2.0, 0.5, 1, o, f),
        call(None, None, 0, None, None, 2.0, 1, 16, 1e-4, 2.0, 0.5, 1, None, None),
        call(fake, fake_model, 1, None, c, 2.0, 1, 16, 1e-4, 2.0, 0.5, 1, o, f),
        call(fake, fake_model, 1, p, None, 2.0, 1, 16, 1e-4, 2.0, 0.5, 1, o, f),
        call(fake, fake_model, 1, p, c, 2.0, 1, 16, 1e-4, 2.0, 0.5, 1, None, f),
        call(fake, fake_model, 1, p, c, 2.0, 1, 16, 1e-4, 2.0, 0.5, 1, o, None),
        *(call(fake, fake_model, 1, p, c, radius, 1, 16, 1e-4, 2.0, 0.5, 1, o, f) for radius in (0.0, -2.0, 64.5, np.nan, np.inf)),
        call(fake, fake_model, 0, None, None, 0.0, 1, 16, 1e-4, 2.0, 0.5, 1, None, None),
        *(call(fake, fake_model, 1, p, c, 2.0, fit_background, 16, 1e-4, 2.0, 0.5, 1, o, f) for fit_background in (2, -1)),
        *(call(fake, fake_model, 1, p, c, 2.0, 1, max_iter, 1e-4, 2.0, 0.5, 1, o, f) for max_iter in (-1, 65)),
        *(call(fake, fake_model, 1, p, c, 2.0, 1, 16, eps, 2.0, 0.5, 1, o, f) for eps in (0.0, -1.0, np.nan, np.inf)),
        *(call(fake, fake_model, 1, p, c, 2.0, 1, 16, 1e-4, shift, 0.5, 1, o, f) for shift in (0.0, -1.0, np.nan, 64.5)),
        *(call(fake, fake_model, 1, p, c, 2.0, 1, 16, 1e-4, 2.0, step, 1, o, f) for step in (0.0, -1.0, np.nan, 64.5)),
        call(fake, fake_model, 0, None, None, 2.0, 1, 16, 1e-4, 2.0, 0.0, 1, None, None),
        *(call(fake, fake_model, 1, _native._ptr(np.array([[3.0, bad]])), c, 2.0, 0, 16, 1e-4, 2.0, 0.5, 0, o, f)
          for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20)),
        lib.rpsf_stars_fit_positions_ms(None, ctypes.byref(ms)),
        lib.rpsf_stars_fit_positions_ms(fake, None),
    ]
    assert calls == [_native.E_BADARG] * len(calls)
    assert np.all(steps == -1.0) and np.all(fits == -1.0) and ms.value == -1.0
