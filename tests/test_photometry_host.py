"""Forced aperture photometry (DESIGN.md 3.7 "Apertures", kernel S6) without a GPU: the kernel's driver
(csrc/rpsf_core_stars_photometry.hpp) on the CPU emulator against the float64 restatement (tests/photometry_cases.py) - the cases and checks
tests/test_gpu_photometry.py runs on the GPU - plus what is host code in the product: star_photometry, the derived fields and the C ABI's
return codes."""

import ctypes
import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import photometry_cases as pc

NEW_SYMBOLS = ("rpsf_stars_photometry", "rpsf_stars_photometry_ms")
FAKE = 0x7F0000000000  # a handle nobody dereferences


@pytest.mark.parametrize("name", tuple(n for n in pc.CASES if not n.endswith(" rows")))
def test_sums_and_counts_match_the_restatement(name):
    pc.check_case(pc.EmuFinder, name)


def test_hard_positions():
    pc.check_hard_positions(pc.EmuFinder)


def test_exact_cases():
    pc.check_exact(pc.EmuFinder)


def test_a_frame_without_a_usable_pixel():
    pc.check_unusable(pc.EmuFinder)


def test_row_counts_around_a_workgroup():
    pc.check_row_counts(pc.EmuFinder, pc.emulator_info()[0])


@pytest.mark.parametrize("name", ("field, mesh", "masked, none", "eight radii, s = 8"))
def test_repeats_are_bit_equal(name):
    pc.check_reproducible(pc.EmuFinder, name)


def test_detect_and_measure_are_untouched():
    pc.check_isolation(pc.EmuFinder)


def test_state_and_argument_errors():
    pc.check_errors(pc.EmuFinder, pc.EmuError)


def test_the_records_fit_the_lds_of_a_plain_launch():
    """s6_lds_bytes(m): what the kernel carves, the launch asks for and the emulator allocates - below 64 KiB for every m."""
    sizes = [pc.emulator_info(m)[2] for m in range(1, 9)]
    assert sizes == [592 + 288 * (16 * m + 64) for m in range(1, 9)] and sizes[-1] <= 64 * 1024 and all(s % 16 == 0 for s in sizes)


def test_the_definition_recovers_gaussians():
    half, centroid = pc.check_truth()
    # the figures the bounds were fixed from (photometry_cases.MEASURED_*), to their printed precision
    assert half <= pc.MEASURED_HALF_LIGHT and centroid <= pc.MEASURED_CENTROID


# ------------------------------------------------------------------------------------------------------------------ host derivations
def _rows(m, flux, n_use, n_all, sums):
    return np.concatenate([[1.5, 2.5], flux, n_use, n_all, sums]).reshape(1, pc.columns(m))


def test_derived_fields_on_hand_made_sums():
    sums = [12.0, 2.0, -4.0, 10.0, 18.0, -3.0, 7.0, 3.0, 4.0]  # abs, mr, mc, mrr, mcc, mrc, peak, peak_row, peak_col
    cat = stars.photometry_from_sums(_rows(3, [2.0, 6.0, 8.0], [25.0, 50.0, 0.0], [25.0, 100.0, 0.0], sums), (1.0, 2.0, 4.0), 5)
    assert cat.dtype == stars.photometry_dtype(3) and cat.shape == (1,)
    assert cat["flux"].shape == cat["area"].shape == cat["coverage"].shape == (1, 3)
    row = cat[0]
    assert (row["row"], row["col"], row["abs_flux"], row["peak"], row["peak_row"], row["peak_col"]) == (1.5, 2.5, 12.0, 7.0, 3.0, 4.0)
    assert row["area"].tolist() == [1.0, 2.0, 0.0] and row["coverage"][:2].tolist() == [1.0, 0.5] and np.isnan(row["coverage"][2])  # 0 / 0
    assert (row["drow"], row["dcol"]) == (0.25, -0.5)
    assert (row["rr"], row["cc"], row["rc"]) == (10.0 / 8 - 0.0625, 18.0 / 8 - 0.25, -3.0 / 8 + 0.125)
    a, b, theta, elongation = stars.ellipse(row["rr"], row["cc"], row["rc"])
    assert (row["a"], row["b"], row["theta"], row["elongation"]) == (a, b, theta, elongation)
    assert row["half_light_radius"] == 1.5  # half of 8 is 4: halfway between (1, 2) and (2, 6)


def test_half_light_radius_interpolation():
    radii = (1.0, 2.0, 4.0)
    flux = np.array([[8.0, 9.0, 10.0],  # reached inside the first segment, from (0, 0): 5 / 8
                     [1.0, 2.0, 10.0],  # in the last: 2 + 3 / 8 * 2
                     [5.0, 7.0, 10.0],  # exactly at a radius
                     [6.0, 3.0, 10.0],  # not monotone: the FIRST crossing, in the first segment
                     [1.0, 2.0, 0.0], [1.0, 2.0, -3.0], [1.0, 2.0, np.nan], [1.0, 2.0, np.inf],  # F <= 0 or not finite
                     [-2.0, -1.0, 4.0]])  # negative on the way: crosses in the last segment, (2 + 1) / 5 of it
    got = stars.half_light_radius(radii, flux)
    assert got[:4].tolist() == [0.625, 2.75, 1.0, 5.0 / 6.0] and np.isnan(got[4:8]).all() and got[8] == 2.0 + 3.0 / 5.0 * 2.0
    assert stars.half_light_radius((3.0,), [[2.0]]).tolist() == [1.5] and stars.half_light_radius(radii, np.zeros((0, 3))).shape == (0,)


def test_dtype_and_shapes_for_one_and_three_radii():
    for m in (1, 3):
        dtype = stars.photometry_dtype(m)
        assert dtype.names == ("row", "col", "flux", "area", "coverage", "abs_flux", "peak", "peak_row", "peak_col", "drow", "dcol", "rr",
                               "cc", "rc", "a", "b", "theta", "elongation", "half_light_radius")
        assert all(dtype[n].shape == (m,) for n in ("flux", "area", "coverage")) and dtype.itemsize == 8 * (16 + 3 * m)
        assert all(dtype[n] == np.float64 for n in dtype.names if n not in ("flux", "area", "coverage"))
        assert stars.photometry_columns(m) == pc.columns(m)
        empty = stars.photometry_from_sums(np.zeros((0, pc.columns(m))), np.arange(1.0, m + 1), 5)
        assert empty.shape == (0,) and empty.dtype == dtype and empty["flux"].shape == (0, m)


# ------------------------------------------------------------------------------------------------------------------ Python surface
def test_star_photometry_is_exported_and_says_what_it_is_not():
    assert "star_photometry" in rp.__all__ and rp.star_photometry is stars.star_photometry
    parameters = inspect.signature(rp.star_photometry).parameters
    assert list(parameters) == ["images", "stars", "radii", "mask", "background", "box", "subpix", "device"]
    assert [parameters[n].default for n in ("mask", "background", "box", "subpix", "device")] == [None, "mesh", 64, 5, 0]
    assert all(parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("background", "box", "subpix", "device"))
    for text in (stars.star_photometry.__doc__, stars.__doc__):
        assert "NOT ``sep``" in text and "sum_circle" in text and "flux_radius" in text and "<=" in text and "1 / 12" in text
        assert "error column" in text and "coverage" in text and "not corrected for" in text


def test_star_photometry_on_the_emulator(monkeypatch):
    """star_photometry with the emulator behind it: stars as positions and as a star_catalog array, frame and mask forms, both backgrounds."""
    monkeypatch.setattr(stars, "_Finder", pc.EmuFinder)
    c, masked = pc.case("field, mesh"), pc.case("masked, mesh")
    frame, radii = c["frame"], (2.0, 4.0, 8.0)
    cat = rp.star_catalog(frame, box=32)
    assert len(cat) == 1 and len(cat[0]) == 8
    one = rp.star_photometry(frame, cat, radii, box=32)
    assert isinstance(one, list) and len(one) == 1 and one[0].dtype == stars.photometry_dtype(3) and one[0].shape == (8,)
    assert one[0]["row"].tobytes() == cat[0]["row"].tobytes() and one[0]["col"].tobytes() == cat[0]["col"].tobytes()
    plain = np.stack([cat[0]["row"], cat[0]["col"]], axis=-1)
    for form in ([plain], plain, cat[0], [plain.tolist()]):
        assert rp.star_photometry(frame, form, radii, box=32)[0].tobytes() == one[0].tobytes()
    case_like = {**c, "positions": plain}
    level_f, rows = pc.run(pc.EmuFinder, case_like)
    assert one[0].tobytes() == stars.photometry_from_sums(rows, radii, 5).tobytes()
    # round stars at the detector's centroids: centred, round, all the area there, and half the light well inside R = 4
    assert np.all(np.hypot(one[0]["drow"], one[0]["dcol"]) < 0.05) and np.all(one[0]["elongation"] < 1.3)
    assert np.all(one[0]["coverage"] == 1.0) and np.all((one[0]["half_light_radius"] > 1.0) & (one[0]["half_light_radius"] < 2.5))
    keep = cat[0][cat[0]["elongation"] < np.median(cat[0]["elongation"])]  # a filtered catalogue
    assert rp.star_photometry(frame, [keep], radii, box=32)[0].tobytes() == one[0][cat[0]["elongation"] < np.median(cat[0]["elongation"])].tobytes()
    none = rp.star_photometry(frame, cat, radii, box=32, background="none")[0]
    assert np.all(none["flux"] > one[0]["flux"]) and none["area"].tobytes() == one[0]["area"].tobytes()  # the background of 10 is still in
    frames = [frame, masked["frame"]]
    both = rp.star_photometry(frames, [plain, plain[:3]], radii, [np.zeros(pc.SHAPE, bool), masked["mask"]], box=32, subpix=3)
    assert [len(b) for b in both] == [8, 3] and np.all(both[0]["coverage"] == 1.0)
    hidden = rp.star_photometry(masked["frame"], plain[:3], radii, masked["mask"], box=32, subpix=3)
    assert hidden[0].tobytes() == both[1].tobytes()
    stack = rp.star_photometry(np.stack(frames), [plain, plain[:0]], (3.0,), box=32)
    assert stack[0]["flux"].shape == (8, 1) and stack[1].shape == (0,) and stack[1].dtype == stars.photometry_dtype(1)
    off = rp.star_photometry(frame, [[(-50.0, -50.0)]], radii, box=32)[0]
    assert np.all(off["flux"] == 0.0) and np.all(off["coverage"] == 0.0) and np.all(off["area"] == 0.0) and np.isnan(off["half_light_radius"][0])


def test_star_photometry_argument_errors():
    frame, stars_ = np.zeros((40, 48), np.float32), [np.array([[10.0, 12.0]])]
    for radii, text in (((), "1 ... 8 values"), (np.arange(1.0, 10.0), "1 ... 8 values"), ((2.0, 2.0), "ascend strictly"),
                        ((3.0, 2.0), "ascend strictly"), ((0.0, 2.0), "0 < R <= 64"), ((2.0, 65.0), "0 < R <= 64"), ((np.nan,), "0 < R <= 64"),
                        (((1.0, 2.0),), "1 ... 8 values")):
        with pytest.raises(ValueError, match=text):
            rp.star_photometry(frame, stars_, radii)
    with pytest.raises(TypeError, match="radii must be numbers"):
        rp.star_photometry(frame, stars_, "wide")
    for subpix in (0, 9, -1):
        with pytest.raises(ValueError, match="subpix must lie in 1 ... 8"):
            rp.star_photometry(frame, stars_, (2.0,), subpix=subpix)
    for subpix in (2.5, True, "5", None):
        with pytest.raises(TypeError, match="subpix must be an integer"):
            rp.star_photometry(frame, stars_, (2.0,), subpix=subpix)
    with pytest.raises(ValueError, match='background must be "mesh" or "none"'):
        rp.star_photometry(frame, stars_, (2.0,), background="annulus")
    with pytest.raises(ValueError, match="box must lie in 8 ... 128"):
        rp.star_photometry(frame, stars_, (2.0,), box=4)
    with pytest.raises(ValueError, match="stars has 2 entries for 1 frames"):
        rp.star_photometry(frame, stars_ * 2, (2.0,))
    with pytest.raises(ValueError, match="needs the fields 'row' and 'col'"):
        rp.star_photometry(frame, [np.zeros(2, [("y", np.float64), ("x", np.float64)])], (2.0,))
    for bad in (np.nan, np.inf, 2.0 ** 20, -2.0 ** 20):
        with pytest.raises(ValueError, match="not finite or not inside"):
            rp.star_photometry(frame, [np.array([[10.0, bad]])], (2.0,))


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_exist_and_are_in_the_table():
    lib = _native.lib()
    header = (pc.ROOT / "include" / "rpsf.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in _native._PROTOTYPES and getattr(lib, name).argtypes is not None
        assert f"int {name}(" in header
    assert "#define RPSF_STARS_PHOTOMETRY_COLUMNS(m) (2 + 3 * (m) + 9)\n" in header


def test_new_entry_points_check_their_arguments_before_the_handle():
    lib = _native.lib()
    fake = ctypes.c_void_p(FAKE)  # must not be looked at before the other arguments are
    pos, out, ms = np.array([[3.0, 4.0]]), np.full(pc.columns(8), -1.0), ctypes.c_double(-1.0)
    p, o = _native._ptr(pos), _native._ptr(out)

    def radii(*values):
        return _native._ptr(np.array(values, np.float64))

    calls = [
        lib.rpsf_stars_photometry(None, 1, p, 1, radii(2.0), 5, 1, o),
        lib.rpsf_stars_photometry(None, 0, None, 1, radii(2.0), 5, 1, None),
        lib.rpsf_stars_photometry(fake, 1, None, 1, radii(2.0), 5, 1, o),
        lib.rpsf_stars_photometry(fake, 1, p, 1, radii(2.0), 5, 1, None),
        lib.rpsf_stars_photometry(fake, 1, p, 1, None, 5, 1, o),
        lib.rpsf_stars_photometry(fake, 1, p, 0, radii(2.0), 5, 1, o),
        lib.rpsf_stars_photometry(fake, 1, p, 9, radii(*range(1, 10)), 5, 1, o),
        lib.rpsf_stars_photometry(fake, 1, p, 1, radii(2.0), 0, 1, o),
        lib.rpsf_stars_photometry(fake, 1, p, 1, radii(2.0), 9, 1, o),
        lib.rpsf_stars_photometry(fake, 1, p, 2, radii(2.0, 2.0), 5, 1, o),
        lib.rpsf_stars_photometry(fake, 1, p, 2, radii(3.0, 2.0), 5, 1, o),
        lib.rpsf_stars_photometry(fake, 1, p, 1, radii(0.0), 5, 1, o),
        lib.rpsf_stars_photometry(fake, 1, p, 1, radii(64.5), 5, 1, o),
        lib.rpsf_stars_photometry(fake, 1, p, 1, radii(np.nan), 5, 1, o),
        lib.rpsf_stars_photometry(fake, 0, None, 1, radii(-1.0), 5, 1, None),
        *(lib.rpsf_stars_photometry(fake, 1, _native._ptr(np.array([[3.0, bad]])), 1, radii(2.0), 5, 0, o)
          for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20)),
        lib.rpsf_stars_photometry_ms(None, ctypes.byref(ms)),
        lib.rpsf_stars_photometry_ms(fake, None),
    ]
    assert calls == [_native.E_BADARG] * len(calls)
    assert np.all(out == -1.0) and ms.value == -1.0
