"""Gaussian-windowed positions (DESIGN.md 3.7 "Windowed positions", kernel S7) without a GPU: the kernel's driver
(csrc/rpsf_core_stars_refine.hpp) on the CPU emulator against the float64 restatement (tests/refine_cases.py) - the cases and checks
tests/test_gpu_refine.py runs on the GPU - plus what is host code in the product: refine_stars, the builder's refine_sigma option, the derived fields
and the C ABI's return codes."""

import ctypes
import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, builder, stars
from tests import refine_cases as rc

NEW_SYMBOLS = ("rpsf_stars_refine", "rpsf_stars_refine_ms")
FAKE = 0x7F0000000000  # a handle nobody dereferences


@pytest.mark.parametrize("name", tuple(rc.WALK_CASES))
def test_the_walk_matches_the_restatement(name):
    rc.check_walk(rc.EmuFinder, name)


def test_hard_positions():
    rc.check_hard_positions(rc.EmuFinder)


@pytest.mark.parametrize("name", tuple(rc.CHAIN_CASES))
def test_the_chain_follows_the_rules_bit_for_bit(name):
    rc.check_chain_case(rc.EmuFinder, name)


def test_every_stop_rule_fires():
    rc.check_stop_rules(rc.EmuFinder)


def test_row_counts_around_a_workgroup():
    rc.check_row_counts(rc.EmuFinder, rc.emulator_info()[0])


@pytest.mark.parametrize("name", ("chain, sigma 2.5", "walk, masked, mesh", "one workgroup, three ends"))
def test_repeats_are_bit_equal(name):
    rc.check_reproducible(rc.EmuFinder, name)


def test_detect_measure_and_photometry_are_untouched():
    rc.check_isolation(rc.EmuFinder)


def test_state_and_argument_errors():
    rc.check_errors(rc.EmuFinder, rc.EmuError)


def test_the_window_function_against_long_double():
    worst = rc.check_g()
    assert worst < rc.G_BOUND / rc.U


def test_the_records_fit_the_lds_of_a_plain_launch():
    """s7_lds_bytes(): what the kernel carves, the launch asks for and the emulator allocates.  256 lane records and 32 group records of
    seven doubles and two ints, then four doubles and three ints of state for each of the four waves, rounded up to 16 bytes."""
    waves, _, size = rc.emulator_info()
    assert waves == 4
    state = (waves * (4 * 8 + 3 * 4) + 15) // 16 * 16
    assert size == (256 + 8 * waves) * (7 * 8 + 2 * 4) + state == 18608 and size % 16 == 0 and size <= 64 * 1024


def test_the_definition_recovers_gaussians():
    position, moments = rc.check_truth()
    # the figures the bounds were fixed from (refine_cases.MEASURED_*), to their printed precision
    assert position <= rc.MEASURED_POSITION and moments <= rc.MEASURED_MOMENTS


# ------------------------------------------------------------------------------------------------------------------ host derivations
def _row(y0, x0, y, x, sigma, niter, flags, dy, dx, n_use, n_all, sums):
    return np.array([[y0, x0, y, x, sigma, niter, flags, dy, dx, n_use, n_all, *sums]])


def test_derived_fields_on_hand_made_sums():
    # S = 8, A = 12, mr = 2, mc = -4, mrr = 4.5, mcc = 6, mrc = -1: drow = 0.25, dcol = -0.5, M_w = [[0.5, 0], [0, 0.5]]
    rows = _row(10.0, 20.0, 10.5, 19.75, 1.0, 3, 0, 0.125, -0.25, 30.0, 40.0, [8.0, 12.0, 2.0, -4.0, 4.5, 6.0, -1.0])
    cat = stars.refine_from_sums(rows)
    assert cat.dtype == stars.refine_dtype() and cat.shape == (1,)
    row = cat[0]
    assert (row["row"], row["col"], row["row0"], row["col0"], row["sigma"]) == (10.5, 19.75, 10.0, 20.0, 1.0)
    assert (row["niter"], row["flags"], bool(row["converged"]), row["step_row"], row["step_col"]) == (3, 0, True, 0.125, -0.25)
    assert (row["flux"], row["abs_flux"], row["coverage"], row["drow"], row["dcol"]) == (8.0, 12.0, 0.75, 0.25, -0.5)
    assert (row["wrr"], row["wcc"], row["wrc"]) == (0.5, 0.5, 0.0)
    assert (row["rr"], row["cc"], row["rc"]) == (1.0, 1.0, 0.0)  # a unit Gaussian under a unit window: 1 / (1 / 0.5 - 1)
    a, b, theta, elongation = stars.ellipse(row["rr"], row["cc"], row["rc"])
    assert (row["a"], row["b"], row["theta"], row["elongation"]) == (a, b, theta, elongation) and (a, b) == (1.0, 1.0)
    for niter, flags, converged in ((0, 0, False), (16, stars.NOT_CONVERGED, False), (2, stars.NO_FLUX, False), (1, stars.RAN_AWAY, False),
                                    (1, 0, True)):
        one = stars.refine_from_sums(_row(1.0, 1.0, 1.0, 1.0, 2.0, niter, flags, np.nan, np.nan, 0.0, 0.0, [0.0] * 7))[0]
        assert bool(one["converged"]) is converged and np.isnan(one["coverage"]) and np.isnan(one["rr"])  # 0 / 0
    empty = stars.refine_from_sums(np.zeros((0, len(stars.REFINE_COLUMNS))))
    assert empty.shape == (0,) and empty.dtype == stars.refine_dtype()


def test_the_window_correction():
    # M_w = [[0.8, 0.2], [0.2, 0.5]] under sigma = 2: M_w^-1 = [[0.5, -0.2], [-0.2, 0.8]] / 0.36, minus I / 4, inverted
    rr, cc, rc = stars.window_corrected(0.8, 0.5, 0.2, 2.0)
    want = np.linalg.inv(np.linalg.inv(np.array([[0.8, 0.2], [0.2, 0.5]])) - np.eye(2) / 4.0)
    assert np.allclose([rr, cc, rc], [want[0, 0], want[1, 1], want[0, 1]], rtol=1e-14, atol=0)
    sigma, true = 1.5, np.array([[1.9, -0.4], [-0.4, 1.1]])  # a Gaussian of covariance `true` seen through the window
    seen = np.linalg.inv(np.linalg.inv(true) + np.eye(2) / sigma ** 2)
    assert np.allclose(stars.window_corrected(seen[0, 0], seen[1, 1], seen[0, 1], sigma), [1.9, 1.1, -0.4], rtol=1e-12, atol=0)
    # not positive definite: as wide as the window (M_w = sigma^2 I), wider, a negative or singular M_w, NaN
    for wrr, wcc, wrc in ((4.0, 4.0, 0.0), (5.0, 1.0, 0.0), (1.0, 5.0, 0.0), (-1.0, 1.0, 0.0), (1.0, 1.0, 1.0), (1.0, 1.0, 2.0), (np.nan, 1.0, 0.0),
                          (0.0, 0.0, 0.0)):
        assert np.isnan(stars.window_corrected(wrr, wcc, wrc, 2.0)).all(), (wrr, wcc, wrc)
    many = stars.window_corrected(np.array([0.5, 4.0]), np.array([0.5, 4.0]), np.zeros(2), np.array([1.0, 2.0]))
    assert many[0].tolist()[0] == 1.0 and np.isnan(many[0][1]) and many[2][0] == 0.0


def test_refined_positions_keep_the_detection_on_failure():
    positions = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0], [9.0, 10.0]])
    rows = np.zeros((5, len(stars.REFINE_COLUMNS)))
    rows[:, 2:4] = positions + 0.25
    rows[:, 6] = [0, stars.NOT_CONVERGED, stars.NO_FLUX, stars.RAN_AWAY, stars.RAN_AWAY | stars.NOT_CONVERGED]
    got = stars.refined_positions(positions, rows)
    assert got.tolist() == [[1.25, 2.25], [3.25, 4.25], [5.0, 6.0], [7.0, 8.0], [9.0, 10.0]] and got.flags.c_contiguous
    assert stars.refined_positions(np.zeros((0, 2)), np.zeros((0, 18))).shape == (0, 2)


# ------------------------------------------------------------------------------------------------------------------ Python surface
def test_refine_stars_is_exported_and_says_what_it_is_not():
    assert "refine_stars" in rp.__all__ and rp.refine_stars is stars.refine_stars
    parameters = inspect.signature(rp.refine_stars).parameters
    assert list(parameters) == ["images", "stars", "sigma", "mask", "background", "box", "max_iter", "eps", "max_shift", "device"]
    assert [parameters[n].default for n in ("mask", "background", "box", "max_iter", "eps", "max_shift", "device")] == [None, "mesh", 64, 16, 1e-4,
                                                                                                                      2.0, 0]
    assert all(parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("background", "box", "max_iter", "eps", "max_shift", "device"))
    for text in (stars.refine_stars.__doc__, stars.__doc__):
        assert "NOT ``sep``" in text and "winpos" in text and "<=" in text and "error column" in text and "not corrected for" in text
        assert "sub-pixel sampling" in text
    assert "exact for a Gaussian" in stars.refine_stars.__doc__ and "untruncated" in stars.refine_stars.__doc__
    dtype = stars.refine_dtype()
    assert dtype.names == ("row", "col", "row0", "col0", "sigma", "niter", "flags", "converged", "step_row", "step_col", "flux", "abs_flux",
                           "coverage", "drow", "dcol", "wrr", "wcc", "wrc", "rr", "cc", "rc", "a", "b", "theta", "elongation")
    assert dtype["niter"] == np.int32 and dtype["flags"] == np.int32 and dtype["converged"] == np.bool_
    assert all(dtype[n] == np.float64 for n in dtype.names if n not in ("niter", "flags", "converged"))
    assert len(stars.REFINE_COLUMNS) == rc.COLUMNS and (stars.NO_FLUX, stars.RAN_AWAY, stars.NOT_CONVERGED) == (1, 2, 4)
    # the option lives in the builder's finder_options alone: find_stars and star_catalog keep their parameters, and FINDER_OPTIONS,
    # find_stars's defaults, still goes into find_stars as it is
    assert "refine_sigma" not in builder.FINDER_OPTIONS and builder.REFINE_OPTIONS == {"refine_sigma": None}
    assert list(builder.FINDER_OPTIONS)[:3] == ["box", "min_area", "max_area"]
    for function in (rp.find_stars, rp.star_catalog):
        assert set(builder.FINDER_OPTIONS) <= set(inspect.signature(function).parameters)


def test_refine_stars_on_the_emulator(monkeypatch):
    """refine_stars with the emulator behind it: stars as positions and as catalogues, the forms of sigma, and what takes its output."""
    monkeypatch.setattr(stars, "_Finder", rc.EmuFinder)
    frame, truth = rc.field()["frame"], rc.field()["truth"]
    starts = rc.whole_pixel_starts()
    one = rp.refine_stars(frame, starts, 1.5, box=32)
    assert isinstance(one, list) and len(one) == 1 and one[0].dtype == stars.refine_dtype() and one[0].shape == (8,)
    _, rows = rc.run(rc.EmuFinder, rc.case("chain, sigma 1.5"))
    assert one[0].tobytes() == stars.refine_from_sums(rows).tobytes()
    assert np.all(one[0]["converged"]) and one[0]["row0"].tobytes() == starts[:, 0].tobytes() and one[0]["col0"].tobytes() == starts[:, 1].tobytes()
    assert np.all(np.hypot(one[0]["row"] - truth[:, 0], one[0]["col"] - truth[:, 1]) < 0.02) and np.all(one[0]["coverage"] == 1.0)
    assert np.all(np.hypot(one[0]["drow"], one[0]["dcol"]) < 1e-4) and np.all(one[0]["elongation"] < 1.3)
    for form in ([starts], [starts.tolist()], np.ascontiguousarray(starts)):
        assert rp.refine_stars(frame, form, 1.5, box=32)[0].tobytes() == one[0].tobytes()
    for sigma in (np.full(8, 1.5), [np.full(8, 1.5)], np.float64(1.5), [1.5] * 8):
        assert rp.refine_stars(frame, starts, sigma, box=32)[0].tobytes() == one[0].tobytes()
    cat = rp.star_catalog(frame, box=32)
    again = rp.refine_stars(frame, cat, 1.5, box=32)[0]  # a star_catalog array, and refine_stars' own output
    assert again["row0"].tobytes() == cat[0]["row"].tobytes() and np.all(again["converged"])
    nearest = np.hypot(again["row"][:, None] - one[0]["row"][None, :], again["col"][:, None] - one[0]["col"][None, :]).min(axis=1)
    assert np.all(nearest < 1e-3)  # the same stars from another start (the catalogue is in raster order)
    twice = rp.refine_stars(frame, [again], 1.5, box=32)[0]
    assert twice["row0"].tobytes() == again["row"].tobytes() and np.all(twice["niter"] <= 2)
    phot = rp.star_photometry(frame, [again], (2.0, 4.0), box=32)[0]  # star_photometry takes it as it is
    assert phot["row"].tobytes() == again["row"].tobytes() and phot["col"].tobytes() == again["col"].tobytes()
    assert builder.star_positions(again).tobytes() == np.stack([again["row"], again["col"]], axis=-1).tobytes()
    forced = rp.refine_stars(frame, starts, 1.5, box=32, max_iter=0)[0]
    assert forced["row"].tobytes() == starts[:, 0].tobytes() and not forced["converged"].any() and np.all(forced["flags"] == 0)
    none = rp.refine_stars(frame, starts, 1.5, box=32, background="none")[0]
    assert np.all(none["flux"] > one[0]["flux"])  # the background of 10 is still in
    masked = rc.case("walk, masked, mesh")
    both = rp.refine_stars([frame, masked["frame"]], [starts, starts[:3]], [np.full(8, 1.5), np.array([1.0, 1.5, 2.5])],
                           [np.zeros(rc.SHAPE, bool), masked["mask"]], box=32)
    assert [len(b) for b in both] == [8, 3] and both[0].tobytes() == one[0].tobytes() and np.all(both[1]["coverage"] < 1.0)
    stack = rp.refine_stars(np.stack([frame, frame]), [starts, starts[:0]], 1.5, box=32)
    assert stack[0].tobytes() == one[0].tobytes() and stack[1].shape == (0,) and stack[1].dtype == stars.refine_dtype()
    off = rp.refine_stars(frame, [[(-50.0, -50.0)]], 2.0, box=32)[0]
    assert off["flags"][0] == stars.NO_FLUX and off["coverage"][0] == 0.0 and off["flux"][0] == 0.0 and not off["converged"][0]


def test_refined_positions_on_the_emulator(monkeypatch):
    """What the builder's refine_sigma does to a star list, composed from the public calls: refine_stars on find_stars' detections, the
    detection kept where the iteration fails."""
    monkeypatch.setattr(stars, "_Finder", rc.EmuFinder)
    frame = rc.field()["frame"]
    found = rp.find_stars(frame, box=32)
    assert rp.find_stars(**{"images": frame, **builder.FINDER_OPTIONS, "box": 32})[0].tobytes() == found[0].tobytes()
    rows = rp.refine_stars(frame, found, 1.5, box=32)[0]
    refined = stars.refined_positions(found[0], rows)
    assert np.all(rows["converged"]) and refined.tobytes() == np.stack([rows["row"], rows["col"]], axis=-1).tobytes()
    assert refined.shape == (8, 2) and refined.dtype == np.float64 and refined.flags.c_contiguous and refined.tobytes() != found[0].tobytes()
    finder = rc.EmuFinder(frame.shape, 32)  # the builder's own call, on a finder that holds the frame
    finder.background_device(frame, None)
    assert stars.refine_detections(finder, finder.detect_device(3.0, 5, None)[:, :2], 1.5).tobytes() == refined.tobytes()
    assert stars.refine_detections(finder, np.zeros((0, 2)), 1.5).shape == (0, 2) and finder.refine_ms() > 0.0  # (nothing launched for none)
    finder.close()
    # two stars six pixels apart come out as one detection between them, whose iteration runs away: it keeps its position
    stop = rc.case("between two stars")["frame"]
    found = rp.find_stars(stop, box=32)
    rows = rp.refine_stars(stop, found, 1.5, box=32)[0]
    failed = (rows["flags"] & (stars.NO_FLUX | stars.RAN_AWAY)) != 0
    assert len(found[0]) == 3 and failed.tolist() == [False, False, True]
    refined = stars.refined_positions(found[0], rows)
    assert refined[2].tobytes() == found[0][2].tobytes() and refined[:2].tobytes() == np.stack([rows["row"], rows["col"]], axis=-1)[:2].tobytes()


def test_argument_errors():
    frame, stars_ = np.zeros((40, 48), np.float32), [np.array([[10.0, 12.0]])]
    for sigma in (0.4, 16.5, np.nan, -1.0, [0.3], [[1.0, 0.2]]):
        with pytest.raises(ValueError, match="sigma must lie in 0.5 ... 16"):
            rp.refine_stars(frame, [np.array([[10.0, 12.0], [11.0, 13.0]])] if np.ndim(sigma) == 2 else stars_, sigma)
    with pytest.raises(TypeError, match="sigma must be numbers"):
        rp.refine_stars(frame, stars_, "wide")
    with pytest.raises(ValueError, match="a scalar or one value per star"):
        rp.refine_stars(frame, stars_, [1.0, 2.0])
    with pytest.raises(ValueError, match="sigma has 2 entries for 1 frames"):
        rp.refine_stars(frame, stars_, [np.array([1.0]), np.array([1.0])])
    for max_iter in (-1, 65):
        with pytest.raises(ValueError, match="max_iter must lie in 0 ... 64"):
            rp.refine_stars(frame, stars_, 1.5, max_iter=max_iter)
    for max_iter in (2.5, True, "5", None):
        with pytest.raises(TypeError, match="max_iter must be an integer"):
            rp.refine_stars(frame, stars_, 1.5, max_iter=max_iter)
    for eps in (0.0, -1e-4, np.nan, np.inf):
        with pytest.raises(ValueError, match="eps must be positive and finite"):
            rp.refine_stars(frame, stars_, 1.5, eps=eps)
    for max_shift in (0.0, -1.0, 64.5, np.nan):
        with pytest.raises(ValueError, match="max_shift must lie in 0 < max_shift <= 64"):
            rp.refine_stars(frame, stars_, 1.5, max_shift=max_shift)
    with pytest.raises(ValueError, match='background must be "mesh" or "none"'):
        rp.refine_stars(frame, stars_, 1.5, background="annulus")
    with pytest.raises(ValueError, match="box must lie in 8 ... 128"):
        rp.refine_stars(frame, stars_, 1.5, box=4)
    with pytest.raises(ValueError, match="stars has 2 entries for 1 frames"):
        rp.refine_stars(frame, stars_ * 2, 1.5)
    for bad in (np.nan, np.inf, 2.0 ** 20, -2.0 ** 20):
        with pytest.raises(ValueError, match="not finite or not inside"):
            rp.refine_stars(frame, [np.array([[10.0, bad]])], 1.5)
    for function in (rp.find_stars, rp.star_catalog):  # the option is the builder's
        with pytest.raises(TypeError, match="refine_sigma"):
            function(frame, refine_sigma=1.5)
    for bad in (17.0, np.nan):
        with pytest.raises(ValueError, match="refine_sigma must lie in 0.5 ... 16"):
            rp.ArrayPSFBuilder(16, finder="device", finder_options={"refine_sigma": bad})
    for bad in ("1.5", True, [1.5]):
        with pytest.raises(TypeError, match="refine_sigma must be None or a number"):
            rp.ArrayPSFBuilder(16, finder="device", finder_options={"refine_sigma": bad})
    with pytest.raises(ValueError, match="finder_options is a dict with any of .*'deblend_prominence', 'refine_sigma'\\), not"):
        rp.ArrayPSFBuilder(16, finder="device", finder_options={"refine": 1.5})
    with pytest.raises(ValueError, match="refine_sigma must lie in 0.5 ... 16"):
        rp.ArrayPSFBuilder(16, finder="device", finder_options={"refine_sigma": 0.1})
    with pytest.raises(ValueError, match='finder_options may only be given with finder="device"'):
        rp.ArrayPSFBuilder(16, finder_options={"refine_sigma": 1.5})
    assert rp.ArrayPSFBuilder(16, finder="device", finder_options={"refine_sigma": 2})._refine_sigma == 2.0
    assert rp.ArrayPSFBuilder(16, finder="device")._refine_sigma is None and rp.ArrayPSFBuilder(16)._refine_sigma is None


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_exist_and_are_in_the_table():
    lib = _native.lib()
    header = (rc.ROOT / "include" / "rpsf.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in _native._PROTOTYPES and getattr(lib, name).argtypes is not None
        assert f"int {name}(" in header
    assert "#define RPSF_STARS_REFINE_COLUMNS 18\n" in header
    for name, value in (("NO_FLUX", 1), ("RAN_AWAY", 2), ("NOT_CONVERGED", 4)):
        assert f"#define RPSF_STARS_REFINE_{name} {value}\n" in header


def test_new_entry_points_check_their_arguments_before_the_handle():
    lib = _native.lib()
    fake = ctypes.c_void_p(FAKE)  # must not be looked at before the other arguments are
    pos, sigma, out, ms = np.array([[3.0, 4.0]]), np.array([1.5]), np.full(rc.COLUMNS, -1.0), ctypes.c_double(-1.0)
    p, s, o = _native._ptr(pos), _native._ptr(sigma), _native._ptr(out)

    def one(value):
        return _native._ptr(np.array([value], np.float64))

    calls = [
        lib.rpsf_stars_refine(None, 1, p, s, 16, 1e-4, 2.0, 1, o),
        lib.rpsf_stars_refine(None, 0, None, None, 16, 1e-4, 2.0, 1, None),
        lib.rpsf_stars_refine(fake, 1, None, s, 16, 1e-4, 2.0, 1, o),
        lib.rpsf_stars_refine(fake, 1, p, None, 16, 1e-4, 2.0, 1, o),
        lib.rpsf_stars_refine(fake, 1, p, s, 16, 1e-4, 2.0, 1, None),
        lib.rpsf_stars_refine(fake, 1, p, s, -1, 1e-4, 2.0, 1, o),
        lib.rpsf_stars_refine(fake, 1, p, s, 65, 1e-4, 2.0, 1, o),
        lib.rpsf_stars_refine(fake, 0, None, None, 65, 1e-4, 2.0, 1, None),
        *(lib.rpsf_stars_refine(fake, 1, p, s, 16, eps, 2.0, 1, o) for eps in (0.0, -1.0, np.nan, np.inf)),
        *(lib.rpsf_stars_refine(fake, 1, p, s, 16, 1e-4, shift, 1, o) for shift in (0.0, -2.0, 64.5, np.nan, np.inf)),
        *(lib.rpsf_stars_refine(fake, 1, p, one(bad), 16, 1e-4, 2.0, 0, o) for bad in (0.49, 16.5, 0.0, -1.5, np.nan, np.inf)),
        *(lib.rpsf_stars_refine(fake, 1, _native._ptr(np.array([[3.0, bad]])), s, 16, 1e-4, 2.0, 0, o)
          for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20)),
        lib.rpsf_stars_refine_ms(None, ctypes.byref(ms)),
        lib.rpsf_stars_refine_ms(fake, None),
    ]
    assert calls == [_native.E_BADARG] * len(calls)
    assert np.all(out == -1.0) and ms.value == -1.0
