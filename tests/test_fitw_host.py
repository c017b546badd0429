"""Weighted fits (DESIGN.md 3.7 "Weighted fits", kernel S12) without a GPU: the kernel's driver (csrc/rpsf_core_stars_fit_weighted.hpp) on
the CPU emulator against the float64 restatement (tests/fitw_cases.py), bit for bit - the cases and checks tests/test_gpu_fitw.py runs on
the GPU - the statistics of the formal errors on the restatement, and what is host code in the product: fit_stars_weighted, the derived
fields and the C ABI's return codes."""

import ctypes
import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import fit_cases as fc
from tests import fitw_cases as fw

NEW_SYMBOLS = ("rpsf_stars_variance_host", "rpsf_stars_variance_view", "rpsf_stars_fit_weighted", "rpsf_stars_fit_weighted_ms")
FAKE = 0x7F0000000000  # a handle nobody dereferences


@pytest.mark.parametrize("name", tuple(fw.TABLE_CASES))
def test_the_weighted_fit_matches_the_restatement_bit_for_bit(name):
    fw.check_case(fw.EmuFinder, fw.EmuModel, name)


def test_the_table_covers_what_it_claims():
    names = set(fw.TABLE_CASES)
    for n, radii in ((8, (3.0,)), (9, (3.5,)), (16, (3.5, 7.0))):
        for b in ("mesh", "none"):
            for fb in ("flux and background", "flux alone"):
                for how in ("map", "model"):
                    assert fw.case(f"N = {n}, {b}, {fb}, {how}")["radii"] == radii
    assert {f"{k} rows" for k in (0, 3, 4, 5)} <= names and fw.emulator_info()[0] == 4
    wide = fw.case("wide: N = 130, R = 64, three stars")
    assert wide["frame"].shape == (200, 232) and wide["cube"].shape[1:] == (130, 130) and wide["radii"] == (64.0,) and len(wide["positions"]) == 3
    assert fw.case("a float64 map")["variance"].dtype == np.float64 and np.isinf(fw.case("noise model, gain inf")["gain"])
    bad = fw.bad_map()
    assert np.isnan(bad[20, 17]) and bad[21, 17] == 0.0 and bad[19, 18] < 0.0 and np.isposinf(bad[20, 19]) and 0.0 < bad[22, 18] < 1.2e-38
    for r, c in (*fw.BAD_PIXELS, fw.SUBNORMAL_PIXEL):  # inside the disc of R = 3.5 around the first star
        assert (r - fw.STAR[0]) ** 2 + (c - fw.STAR[1]) ** 2 <= 3.5 ** 2


def test_every_flag_fires():
    fw.check_every_flag_fires(fw.EmuFinder, fw.EmuModel)


def test_each_bad_variance_takes_out_its_pixel():
    fw.check_bad_variances(fw.EmuFinder, fw.EmuModel)


def test_unit_and_power_of_two_variances_against_the_unweighted_fit():
    fw.check_power_of_two(fw.EmuFinder, fw.EmuModel)


def test_row_counts_around_a_workgroup():
    fw.check_row_counts(fw.EmuFinder, fw.EmuModel, fw.emulator_info()[0])


@pytest.mark.parametrize("name", ("N = 16, mesh, flux and background, map", "noise model, gain 2.5", "9 rows"))
def test_repeats_are_bit_equal(name):
    fw.check_reproducible(fw.EmuFinder, fw.EmuModel, name)


def test_the_other_kernels_are_untouched():
    fw.check_isolation(fw.EmuFinder, fw.EmuModel)


def test_state_and_argument_errors():
    fw.check_errors(fw.EmuFinder, fw.EmuModel, fw.EmuError)


def test_the_records_fit_the_lds_of_a_plain_launch():
    """s12_lds_bytes(): 256 lane records and 32 group records of eight doubles, one 64-bit index and two ints, then S8's state."""
    waves, _, size = fw.emulator_info()
    state = (waves * (2 * 8 + 4) + 15) // 16 * 16
    assert waves == 4 and size == (256 + 8 * waves) * (8 * 8 + 8 + 2 * 4) + state == 23120 and size % 16 == 0 and size <= 64 * 1024


def test_the_core_header_calls_s8s_functions_and_keeps_contraction_off():
    text = (fw.ROOT / "regularizepsf_amd" / "csrc" / "rpsf_core_stars_fit_weighted.hpp").read_text()
    assert '#include "rpsf_core_stars_fit.hpp"' in text and "#pragma clang fp contract(off)" in text and "namespace rpsfw" in text
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    # S12 is S8's driver with a weight policy: the header calls fit_disc and defines no walk, fold or pass 2 of its own, and that driver
    # and the walk under it call S8's functions
    assert "fit_disc(" in code and "finite_d(" in code and "each(" not in code and "for (" not in code
    csrc = fw.ROOT / "regularizepsf_amd" / "csrc"
    shared = "\n".join(line.split("//")[0] for n in ("rpsf_core_stars_fit.hpp", "rpsf_core_stars_disc.hpp") for line in (csrc / n).read_text().splitlines())
    assert "void fit_disc(" in shared and "void fit_disc(" not in code
    for name in ("model_at(", "see_residual(", "usable(", "background_at(", "finite_d("):
        assert name in shared, name
    for definition in ("double model_at(", "void see_residual(", "double peak_key(", "bool usable(", "double background_at(", "bool finite_d(", "sqrt"):
        assert definition not in code, definition


# ------------------------------------------------------------------------------------------------------------------ the statistics
def test_the_formal_errors_describe_the_scatter():
    """256 isolated stars, noise drawn from a variance map that runs through a factor of 30 inside every disc, the map given to the fit.
    For 256 independent unit-normal pulls, at 5 sigma: |mean| <= 5 / sqrt(256), the sample variance within 1 +- 5 sqrt(2 / 255), the mean
    chi2_reduced within 1 +- 5 sqrt(2 / (dof 256)) with the largest dof of the field (the narrowest bound).
    Measured: mean pull -0.0676, variance 1.0977, mean chi2_reduced 1.0011 (bound 1 +- 0.0708) at dof 33 ... 39."""
    f = fw.pull_field()
    assert fw.disc_variance_ratio(f).min() > 10.0
    fits = fw.stat_fits(f, weighted=True)
    assert len(fits) == 256 and np.all(fits["flags"] == 0) and np.all(fits["coverage"] == 1.0)
    pulls = (fits["flux"] - f["flux"]) / fits["flux_err"]
    dof = fits["dof"].astype(np.float64)
    mean, variance, chi2 = float(pulls.mean()), float(pulls.var(ddof=1)), float(fits["chi2_reduced"].mean())
    print(f"pulls of 256 stars: mean {mean:.4f} (|.| <= 0.3125), variance {variance:.4f} (1 +- 0.443), mean chi2_reduced {chi2:.4f} "
          f"(1 +- {5 * np.sqrt(2 / (dof.max() * 256)):.4f}), dof {int(dof.min())} ... {int(dof.max())}, flux_err {fits['flux_err'].min():.3g} ... "
          f"{fits['flux_err'].max():.3g}, snr {fits['snr'].min():.3g} ... {fits['snr'].max():.3g}")
    assert abs(mean) <= 5.0 / np.sqrt(256.0)
    assert abs(variance - 1.0) <= 5.0 * np.sqrt(2.0 / 255.0)
    assert abs(chi2 - 1.0) <= 5.0 * np.sqrt(2.0 / (dof.max() * 256.0))


def test_weights_tame_pixels_of_large_variance():
    """Every disc holds three pixels of 10^4 times the variance of the others, next to the star's own pixel, with matching noise: the
    scatter of the weighted flux is below half the scatter of the unweighted fit's.
    Measured on the restatement: weighted 8.449, unweighted 325.9, ratio 0.0259."""
    f = fw.outlier_field()
    weighted, plain = fw.stat_fits(f, weighted=True), fw.stat_fits(f, weighted=False)
    assert np.all(weighted["flags"] == 0) and np.all(plain["flags"] == 0) and np.all(weighted["n_use"] == plain["n_use"])
    inside = [int((f["variance"][int(np.floor(y)) - 4:int(np.floor(y)) + 6, int(np.floor(x)) - 4:int(np.floor(x)) + 6] > 1.0).sum()) for y, x in f["truth"]]
    assert set(inside) == {3}
    scatter_w = float(np.sqrt(np.mean((weighted["flux"] - f["flux"]) ** 2)))
    scatter_p = float(np.sqrt(np.mean((plain["flux"] - f["flux"]) ** 2)))
    print(f"flux scatter of 256 stars: weighted {scatter_w:.4g}, unweighted {scatter_p:.4g}, ratio {scatter_w / scatter_p:.4g} (< 0.5); "
          f"median flux_err {np.median(weighted['flux_err']):.4g}")
    assert scatter_w < 0.5 * scatter_p


# ------------------------------------------------------------------------------------------------------------------ host derivations
def _row(n, sums, f, bg, variances, chi2, abs_res, peak, flags=0):
    return np.array([[10.0, 20.0, 3, flags, n, 9, *sums, f, bg, *variances, chi2, abs_res, *peak]])


def test_derived_fields_on_hand_made_rows():
    # n = 6, Sm = 0.5, Sm_all = 0.625, f = -8, var_f = 4, var_bg = 0.25, chi2 = 16, abs_res = 2
    rows = _row(6, [0.5, 0.625, 12.0, 1.5, 0.25, 30.0, 4.0, 200.0], -8.0, 1.5, [4.0, 0.25, -0.5], 16.0, 2.0, [1.25, -1.25, 11.0, 19.0])
    fit = stars.weighted_fit_from_sums(rows)
    assert fit.dtype == stars.weighted_fit_dtype() and fit.shape == (1,)
    row = fit[0]
    assert (row["row"], row["col"], row["cell"], row["flags"], row["n_use"], row["n_all"]) == (10.0, 20.0, 3, 0, 6, 9)
    assert (row["flux"], row["background"], row["coverage"], row["dof"], row["chi2"], row["chi2_reduced"], row["rms"]) == (-8.0, 1.5, 0.8, 4, 16.0, 4.0, 2.0)
    assert (row["flux_err"], row["background_err"], row["flux_background_cov"], row["snr"]) == (2.0, 0.5, -0.5, -4.0)
    assert (row["sm"], row["sm_all"], row["sw"], row["swm"], row["smm"], row["sd"], row["sdm"], row["sdd"]) == (0.5, 0.625, 12.0, 1.5, 0.25, 30.0, 4.0, 200.0)
    assert (row["abs_res"], row["residual_fraction"], row["peak_res"], row["peak_e"], row["peak_row"], row["peak_col"]) == (2.0, 0.5, 1.25, -1.25, 11.0, 19.0)
    alone = stars.weighted_fit_from_sums(rows, fit_background=False)[0]
    assert alone["dof"] == 5 and alone["chi2_reduced"] == 16.0 / 5.0 and alone["rms"] == np.sqrt(16.0 / 5.0)
    for n, with_background, dof in ((2, True, 0), (1, True, -1), (1, False, 0), (0, False, -1)):  # dof <= 0: chi2_reduced and rms NaN
        one = stars.weighted_fit_from_sums(_row(n, [1.0] * 8, 1.0, 0.0, [1.0, 1.0, 0.0], 0.0, 0.0, [0.0, 0.0, 1.0, 1.0]), with_background)[0]
        assert one["dof"] == dof and np.isnan(one["chi2_reduced"]) and np.isnan(one["rms"]) and one["flux_err"] == 1.0
    nan = np.nan
    for flags, names in ((1, ["no_mesh"]), (2, ["too_few"]), (4, ["degenerate"]), (8, ["bad_cell"]), (9, ["no_mesh", "bad_cell"])):
        one = stars.weighted_fit_from_sums(_row(0, [nan] * 8, nan, nan, [nan] * 3, nan, nan, [nan, nan, -1.0, -1.0], flags))[0]
        assert [k for k in ("no_mesh", "too_few", "degenerate", "bad_cell") if one[k]] == names
        assert all(np.isnan(one[k]) for k in ("coverage", "rms", "chi2_reduced", "flux_err", "background_err", "snr", "flux_background_cov"))
    empty = stars.weighted_fit_from_sums(np.zeros((0, len(stars.FITW_COLUMNS))))
    assert empty.shape == (0,) and empty.dtype == stars.weighted_fit_dtype()


# ------------------------------------------------------------------------------------------------------------------ Python surface
def test_fit_stars_weighted_is_exported_and_says_what_it_is_not():
    assert "fit_stars_weighted" in rp.__all__ and rp.fit_stars_weighted is stars.fit_stars_weighted
    parameters = inspect.signature(rp.fit_stars_weighted).parameters
    assert list(parameters) == ["images", "stars", "psf", "radius", "mask", "variance", "sky_variance", "gain", "background", "box", "fit_background",
                                "cells", "device"]
    keywords = ("variance", "sky_variance", "gain", "background", "box", "fit_background", "cells", "device")
    assert [parameters[n].default for n in ("mask", *keywords)] == [None, None, None, None, "mesh", 64, True, None, 0]
    assert all(parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in keywords)
    text = " ".join(stars.fit_stars_weighted.__doc__.split())
    for phrase in ("positions are fixed", "bilinear and cut at", "errors are formal", "``fit_positions`` and ``fit_groups`` stay unweighted",
                   "w = 1 / v", "sum w e^2", "bit for bit", "2^k"):
        assert phrase in text, phrase
    dtype, plain = stars.weighted_fit_dtype(), stars.fit_dtype()
    assert dtype.names[:len(plain.names)] == plain.names and all(dtype[n] == plain[n] for n in plain.names)  # a superset by name
    assert dtype.names[len(plain.names):] == ("sw", "swm", "flux_err", "background_err", "flux_background_cov", "snr", "chi2_reduced")
    assert len(stars.FITW_COLUMNS) == fw.COLUMNS == 25 and (stars.VARIANCE_MAP, stars.VARIANCE_MODEL) == (0, 1)
    assert stars.FITW_COLUMNS[:6] == stars.FIT_COLUMNS[:6] and stars.FITW_COLUMNS[-6:] == stars.FIT_COLUMNS[-6:]


def test_fit_stars_weighted_on_the_emulator(monkeypatch):
    """fit_stars_weighted with the emulator behind it: the forms of variance, the noise model, and its place before cell_fit_summary."""
    monkeypatch.setattr(stars, "_Finder", fw.EmuFinder)
    monkeypatch.setattr(stars, "_Model", fw.EmuModel)
    frame, truth = fc.field()["frame"], fc.field()["truth"]
    coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering(fc.SHAPE, 8)]
    cube = np.broadcast_to(fc.model(8)[fc.GAUSSIAN], (len(coordinates), 8, 8)).copy()
    psf = rp.IndexedCube(coordinates, cube)
    variance = fw.smooth_map()
    one = rp.fit_stars_weighted(frame, truth, psf, 3.0, variance=variance, box=16)
    assert isinstance(one, list) and len(one) == 1 and one[0].dtype == stars.weighted_fit_dtype() and one[0].shape == (5,)
    cells = stars.nearest_cells(truth, coordinates, 8)
    finder, model = fw.EmuFinder(frame.shape, 16), fw.EmuModel(cube)
    finder.background_device(frame, None)
    finder.variance(variance)
    assert one[0].tobytes() == stars.weighted_fit_from_sums(finder.fit_weighted(model, truth, cells, 3.0)).tobytes()
    by_model = stars.weighted_fit_from_sums(finder.fit_weighted(model, truth, cells, 3.0, True, True, 0.09, 4.0))
    finder.close()
    assert np.all(one[0]["flags"] == 0) and np.all(one[0]["coverage"] == 1.0) and np.all(one[0]["flux_err"] > 0) and np.all(one[0]["snr"] > 50)
    assert np.allclose(one[0]["snr"], one[0]["flux"] / one[0]["flux_err"], rtol=0, atol=0)
    for form in (variance.astype(np.float64), [variance], (variance,), variance[None]):
        assert rp.fit_stars_weighted(frame, truth, psf, 3.0, variance=form, box=16)[0].tobytes() == one[0].tobytes()
    assert rp.fit_stars_weighted(frame, truth, psf, 3.0, sky_variance=0.09, gain=4.0, box=16)[0].tobytes() == by_model.tobytes()
    unit = rp.fit_stars_weighted(frame, truth, psf, 3.0, sky_variance=1.0, box=16)[0]  # gain None: +inf
    plain = rp.fit_stars(frame, truth, psf, 3.0, box=16)[0]
    for name in ("flux", "background", "chi2", "rms", "abs_res", "residual_fraction", "peak_res", "peak_e", "peak_row", "peak_col", "coverage", "sm",
                 "smm", "sd", "sdm", "sdd", "dof", "n_use", "flags", "cell"):
        assert unit[name].tobytes() == plain[name].tobytes(), name
    assert unit["sw"].tolist() == plain["n_use"].tolist() and np.all(unit["chi2_reduced"] == plain["chi2"] / plain["dof"])
    both = rp.fit_stars_weighted([frame, frame], [truth, truth[:3]], psf, 3.0, variance=[variance, np.ones(fc.SHAPE)], box=16)
    assert [len(b) for b in both] == [5, 3] and both[0].tobytes() == one[0].tobytes() and both[1]["flux"].tobytes() == plain["flux"][:3].tobytes()
    shared = rp.fit_stars_weighted(np.stack([frame, frame]), [truth, truth[:0]], psf, 3.0, variance=variance, box=16)
    assert shared[0].tobytes() == one[0].tobytes() and shared[1].shape == (0,) and shared[1].dtype == stars.weighted_fit_dtype()
    summary = rp.cell_fit_summary(both, psf)  # the wider rows are taken by name
    assert summary["count"].sum() == 8 and np.all(summary["residual_fraction"][summary["count"] > 0] > 0)
    keep = [f["snr"] > 5 for f in both]
    assert [k.dtype for k in keep] == [np.bool_, np.bool_] and all(k.all() for k in keep)


def test_argument_errors():
    frame, stars_ = np.zeros((40, 48), np.float32), [np.array([[10.0, 12.0]])]
    psf = rp.IndexedCube([(0, 0)], np.ones((1, 8, 8)))
    ones = np.ones((40, 48), np.float32)
    with pytest.raises(ValueError, match="either as a map .* or as a noise model"):
        rp.fit_stars_weighted(frame, stars_, psf, 2.0)
    with pytest.raises(ValueError, match="either as a map .* or as a noise model"):
        rp.fit_stars_weighted(frame, stars_, psf, 2.0, variance=ones, sky_variance=1.0)
    with pytest.raises(ValueError, match="gain belongs to the noise model"):
        rp.fit_stars_weighted(frame, stars_, psf, 2.0, variance=ones, gain=2.0)
    for sky in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="sky_variance must be finite and not negative"):
            rp.fit_stars_weighted(frame, stars_, psf, 2.0, sky_variance=sky)
    for gain in (0.0, -2.0, np.nan):
        with pytest.raises(ValueError, match="gain must be positive"):
            rp.fit_stars_weighted(frame, stars_, psf, 2.0, sky_variance=1.0, gain=gain)
    for gain in (None, np.inf):
        with pytest.raises(ValueError, match="leaves no variance at all"):
            rp.fit_stars_weighted(frame, stars_, psf, 2.0, sky_variance=0.0, gain=gain)
    with pytest.raises(ValueError, match="must be numbers"):
        rp.fit_stars_weighted(frame, stars_, psf, 2.0, sky_variance="dark")
    for bad in (np.ones((40, 47)), np.ones((1, 40, 47)), [np.ones((48, 40))]):
        with pytest.raises(rp.IncorrectShapeError, match="A variance frame of shape"):
            rp.fit_stars_weighted(frame, stars_, psf, 2.0, variance=bad)
    with pytest.raises(ValueError, match="variance has 2 entries for 1 frames"):
        rp.fit_stars_weighted(frame, stars_, psf, 2.0, variance=[ones, ones])
    with pytest.raises(ValueError, match="variance has 3 entries for 1 frames"):
        rp.fit_stars_weighted(frame, stars_, psf, 2.0, variance=np.ones((3, 40, 48)))
    with pytest.raises(TypeError, match="variance must hold real numbers"):
        rp.fit_stars_weighted(frame, stars_, psf, 2.0, variance=ones.astype(np.complex64))

    class OnDevice:  # what is_device_array takes for a device array; nothing here looks inside it
        __cuda_array_interface__ = {"shape": (40, 48), "typestr": "<f4", "data": (FAKE, False), "version": 3, "strides": None}

    with pytest.raises(TypeError, match="variance and images must live in the same place"):
        rp.fit_stars_weighted(frame, stars_, psf, 2.0, variance=OnDevice())
    with pytest.raises(TypeError, match="variance and images must live in the same place"):
        rp.fit_stars_weighted(frame, stars_, psf, 2.0, variance=[OnDevice()])
    # fit_stars' own checks come through _fit_inputs unchanged
    with pytest.raises(ValueError, match="radius must lie in 0 < R <= min\\(64, N / 2 - 1\\) = 3 for cells of 8"):
        rp.fit_stars_weighted(frame, stars_, psf, 3.5, variance=ones)
    with pytest.raises(TypeError, match="fit_background must be True or False"):
        rp.fit_stars_weighted(frame, stars_, psf, 2.0, variance=ones, fit_background=1)
    with pytest.raises(ValueError, match='background must be "mesh" or "none"'):
        rp.fit_stars_weighted(frame, stars_, psf, 2.0, sky_variance=1.0, background="annulus")
    with pytest.raises(ValueError, match="stars has 2 entries for 1 frames"):
        rp.fit_stars_weighted(frame, stars_ * 2, psf, 2.0, sky_variance=1.0)


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_exist_and_are_in_the_table():
    lib = _native.lib()
    header = (fw.ROOT / "include" / "rpsf.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in _native._PROTOTYPES and getattr(lib, name).argtypes is not None
        assert f" {name}(" in header
    assert "#define RPSF_STARS_FIT_WEIGHTED_COLUMNS 25\n" in header
    assert "#define RPSF_STARS_VARIANCE_MAP 0\n" in header and "#define RPSF_STARS_VARIANCE_MODEL 1\n" in header


def test_new_entry_points_check_their_arguments_before_the_handles():
    lib = _native.lib()
    fake, fake_model = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + 4096)  # must not be looked at before the other arguments are
    pos, cells, out, ms = np.array([[3.0, 4.0]]), np.array([0], np.int32), np.full(fw.COLUMNS, -1.0), ctypes.c_double(-1.0)
    p, c, o = _native._ptr(pos), _native._ptr(cells), _native._ptr(out)
    view = _native.View(None, 0, 40, 48, 48 * 4, 4)
    fit = lib.rpsf_stars_fit_weighted
    calls = [
        fit(None, fake_model, 1, p, c, 2.0, 1, 1, 1, 1.0, 2.0, o),
        fit(fake, None, 1, p, c, 2.0, 1, 1, 1, 1.0, 2.0, o),
        fit(None, None, 0, None, None, 2.0, 1, 1, 1, 1.0, 2.0, None),
        fit(fake, fake_model, 1, None, c, 2.0, 1, 1, 1, 1.0, 2.0, o),
        fit(fake, fake_model, 1, p, None, 2.0, 1, 1, 1, 1.0, 2.0, o),
        fit(fake, fake_model, 1, p, c, 2.0, 1, 1, 1, 1.0, 2.0, None),
        *(fit(fake, fake_model, 1, p, c, radius, 1, 1, 0, 0.0, 1.0, o) for radius in (0.0, -2.0, 64.5, np.nan, np.inf)),
        fit(fake, fake_model, 0, None, None, 0.0, 1, 1, 0, 0.0, 1.0, None),
        *(fit(fake, fake_model, 1, p, c, 2.0, fit_background, 1, 0, 0.0, 1.0, o) for fit_background in (2, -1)),
        *(fit(fake, fake_model, 1, p, c, 2.0, 1, 1, mode, 1.0, 2.0, o) for mode in (2, -1)),
        *(fit(fake, fake_model, 1, p, c, 2.0, 1, 1, 1, sky, gain, o)
          for sky, gain in ((-1.0, 2.0), (np.nan, 2.0), (np.inf, 2.0), (1.0, 0.0), (1.0, -2.0), (1.0, np.nan), (0.0, np.inf))),
        *(fit(fake, fake_model, 1, _native._ptr(np.array([[3.0, bad]])), c, 2.0, 0, 0, 0, 0.0, 1.0, o)
          for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20)),
        lib.rpsf_stars_fit_weighted_ms(None, ctypes.byref(ms)),
        lib.rpsf_stars_fit_weighted_ms(fake, None),
        lib.rpsf_stars_variance_host(None, p, 1),
        lib.rpsf_stars_variance_host(fake, None, 0),
        lib.rpsf_stars_variance_view(None, ctypes.byref(view)),
        lib.rpsf_stars_variance_view(fake, None),
        lib.rpsf_stars_variance_view(fake, ctypes.byref(view)),  # a view without data
    ]
    assert calls == [_native.E_BADARG] * len(calls)
    assert np.all(out == -1.0) and ms.value == -1.0
