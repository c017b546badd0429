"""Second moments and shape per detection (kernel S5) without a GPU: the kernel's driver (csrc/rpsf_core_stars_shape.hpp)
on the CPU emulator against the float64 restatement (tests/shape_cases.py) - the cases and checks tests/test_gpu_shapes.py runs on the
GPU - plus what is host code in the product: star_catalog, the derived fields, build(stars=catalogue) and the C ABI's return codes."""

import ctypes
import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, builder, stars
from tests import shape_cases as shc

NEW_SYMBOLS = ("rpsf_stars_measure", "rpsf_stars_shapes", "rpsf_stars_shape_ms")
FAKE = 0x7F0000000000  # a handle nobody dereferences


@pytest.mark.parametrize("name", tuple(n for n in shc.CASES if n != "background"))
def test_shapes_match_the_restatement(name):
    shc.check_shapes(shc.EmuFinder, name)


def test_pure_background_gives_no_rows_and_no_launch():
    shc.check_empty(shc.EmuFinder)


def test_single_pixels_have_zero_moments_exactly():
    shc.check_single_pixels(shc.EmuFinder)


def test_objects_inside_one_anothers_boxes_keep_their_own_pixels():
    shc.check_enclosure(shc.EmuFinder)


def test_row_counts_around_a_workgroup():
    walk_waves, columns, _ = shc.emulator_info()
    assert columns == len(shc.COLUMNS)
    shc.check_row_counts(shc.EmuFinder, walk_waves)


@pytest.mark.parametrize("name", ("wide", "masked", "pairs 6", "one component, split"))
def test_repeats_are_bit_equal_and_detect_is_untouched(name):
    shc.check_reproducible(shc.EmuFinder, name)


def test_measure_needs_a_detect_of_the_present_frame():
    shc.check_state_errors(shc.EmuFinder, shc.EmuStateError)


def test_the_definition_recovers_the_angles_of_elliptical_stars():
    worst, elongation = shc.check_ellipse_truth()
    # the figures the bound was fixed from (shape_cases.MEASURED_*), to their printed precision
    assert worst <= shc.MEASURED_THETA and elongation >= shc.MEASURED_ELONGATION


def test_the_emulator_detects_what_the_deblend_emulator_detects():
    """The shape emulator runs the detect itself: its rows are deblend_cases.EmuFinder's bit for bit, option on and off."""
    from tests import deblend_cases as dc

    for name in ("wide", "edge", "pairs 5", "masked member"):
        case = shc.reference(name)
        o = case["options"]
        other = dc.run(dc.EmuFinder, case, deblend=o["deblend"], threshold=o["threshold"], min_area=o["min_area"], max_area=o["max_area"])
        assert shc.run(shc.EmuFinder, case)[0].tobytes() == other.tobytes()


# ------------------------------------------------------------------------------------------------------------------ Python surface
def test_star_catalog_is_exported_with_find_stars_signature():
    assert "star_catalog" in rp.__all__ and rp.star_catalog is stars.star_catalog
    assert str(inspect.signature(rp.star_catalog).parameters.keys()) == str(inspect.signature(rp.find_stars).parameters.keys())
    for (_, a), (_, b) in zip(inspect.signature(rp.star_catalog).parameters.items(), inspect.signature(rp.find_stars).parameters.items()):
        assert (a.kind, a.default) == (b.kind, b.default)
    assert stars.SHAPE_COLUMNS == shc.COLUMNS and stars.CATALOG_FIELDS == shc.FIELDS
    assert stars.CATALOG_DTYPE.names == shc.FIELDS and stars.CATALOG_DTYPE.itemsize == 8 * len(shc.FIELDS)
    for text in (stars.star_catalog.__doc__, stars.__doc__):
        assert "NOT ``sep``" in text and "1 / 12" in text and "clamp" in text and "footprint" in text


def test_derived_fields_follow_ieee_rules():
    rr, cc, rc = np.array([4.0, 1.0, 2.0, 0.0, 1.0, -1.0]), np.array([1.0, 4.0, 2.0, 0.0, 1.0, 2.0]), np.array([0.0, 0.0, 1.0, 0.0, 2.0, 0.0])
    a, b, theta, elongation = stars.ellipse(rr, cc, rc)
    assert np.array_equal(a[:4], [2.0, 2.0, np.sqrt(3.0), 0.0]) and np.array_equal(b[:4], [1.0, 1.0, 1.0, 0.0])
    assert np.array_equal(theta[:4], [np.pi / 2, 0.0, np.pi / 4, 0.0])  # along the rows, along the columns, the diagonal, nothing
    assert np.array_equal(elongation[:3], [2.0, 2.0, np.sqrt(3.0)]) and np.isnan(elongation[3])  # 0 / 0
    assert a[4] == np.sqrt(3.0) and np.isnan(b[4]) and np.isnan(elongation[4])  # lambda- = -1
    assert a[5] == np.sqrt(2.0) and np.isnan(b[5])


def test_star_catalog_on_the_emulator(monkeypatch):
    """star_catalog with the emulator behind it: frame and mask forms, a list equal to single calls, dtype and field names."""
    monkeypatch.setattr(stars, "_Finder", shc.EmuFinder)
    wide, masked = shc.reference("wide"), shc.reference("masked")
    one = rp.star_catalog(wide["frame"])
    assert isinstance(one, list) and len(one) == 1 and one[0].dtype == stars.CATALOG_DTYPE and one[0].dtype.names == shc.FIELDS
    assert one[0].shape == (20,)
    want = stars.catalog_from_shapes(shc.run(shc.EmuFinder, wide)[1])
    assert one[0].tobytes() == want.tobytes()
    found = rp.find_stars(wide["frame"])
    assert np.stack([one[0]["row"], one[0]["col"]], axis=-1).tobytes() == found[0].tobytes()
    hidden = rp.star_catalog(masked["frame"], mask=masked["mask"])
    assert hidden[0].tobytes() == stars.catalog_from_shapes(shc.run(shc.EmuFinder, masked)[1]).tobytes() and len(hidden[0]) == 17
    frames = [wide["frame"], masked["frame"]]
    both = rp.star_catalog(frames, 3.0, [np.zeros(wide["frame"].shape, bool), masked["mask"]])
    assert [c.tobytes() for c in both] == [one[0].tobytes(), hidden[0].tobytes()]
    stack = rp.star_catalog(np.stack(frames), mask=masked["mask"])  # one mask for all frames
    assert len(stack) == 2 and stack[1].tobytes() == hidden[0].tobytes() and len(stack[0]) < 20
    pairs = shc.reference("pairs 6")
    assert len(rp.star_catalog(pairs["frame"])[0]) == 12
    split = rp.star_catalog(pairs["frame"], deblend=True)[0]
    assert split.tobytes() == stars.catalog_from_shapes(shc.run(shc.EmuFinder, pairs)[1]).tobytes() and len(split) == 24
    empty = rp.star_catalog(shc.reference("background")["frame"], box=32)
    assert empty[0].shape == (0,) and empty[0].dtype == stars.CATALOG_DTYPE
    nothing = rp.star_catalog(np.full((40, 48), np.nan), box=32)  # no usable pixel: no detect at all
    assert nothing[0].shape == (0,) and nothing[0].dtype == stars.CATALOG_DTYPE
    small = rp.star_catalog(shc.reference("single pixels")["frame"], box=32, min_area=1)[0]
    assert len(small) == 7 and np.all(small["area"] == 1)
    with pytest.raises(ValueError, match="box must lie in 8 ... 128"):
        rp.star_catalog(wide["frame"], box=4)
    with pytest.raises(ValueError, match="deblend must be True or False"):
        rp.star_catalog(wide["frame"], deblend=1)


def test_the_selection_idiom():
    """cat[cat["elongation"] < 1.5] on the restatement's ellipses and round stars: the elongated ones go, the round ones stay."""
    round_stars = stars.catalog_from_shapes(shc.reference("wide")["ref"]["columns"])
    ellipses = stars.catalog_from_shapes(shc.reference("ellipses")["ref"]["columns"])
    assert len(round_stars[round_stars["elongation"] < 1.5]) == 20 and len(ellipses[ellipses["elongation"] < 1.5]) == 0


# ------------------------------------------------------------------------------------------------------------------ build(stars=)
def test_star_positions_of_catalogues_and_plain_arrays():
    catalog = stars.catalog_from_shapes(shc.reference("wide")["ref"]["columns"])
    plain = np.stack([catalog["row"], catalog["col"]], axis=-1)
    got = builder.star_positions(catalog)
    assert got.dtype == np.float64 and got.shape == (20, 2) and got.tobytes() == plain.tobytes()
    keep = catalog["elongation"] < np.median(catalog["elongation"])
    assert builder.star_positions(catalog[keep]).tobytes() == plain[keep].tobytes()
    assert builder.star_positions(catalog[:0]).shape == (0, 2)
    assert builder.star_positions(plain).tobytes() == plain.tobytes()  # plain arrays as before
    assert builder.star_positions([(1, 2), (3, 4)]).tolist() == [[1.0, 2.0], [3.0, 4.0]]
    assert builder.star_positions(np.zeros((0, 2))).shape == (0, 2) and builder.star_positions([]).shape == (0, 2)
    narrow = np.zeros(3, [("row", np.float32), ("col", np.int16), ("flux", np.float64)])
    assert builder.star_positions(narrow).dtype == np.float64 and builder.star_positions(narrow).shape == (3, 2)
    with pytest.raises(ValueError, match="needs the fields 'row' and 'col'"):
        builder.star_positions(np.zeros(3, [("y", np.float64), ("x", np.float64)]))


def test_build_checks_catalogues_before_the_gpu_is_touched():
    frame = np.zeros((40, 48), np.float32)
    catalog = stars.catalog_from_shapes(np.zeros((0, len(shc.COLUMNS))))
    with pytest.raises(ValueError, match="stars has 2 entries for 1 frames"):
        rp.ArrayPSFBuilder(16).build(frame, stars=[catalog, catalog])
    with pytest.raises(ValueError, match="needs the fields 'row' and 'col'"):
        rp.ArrayPSFBuilder(16).build(frame, stars=[np.zeros(2, [("y", np.float64), ("x", np.float64)])])


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_exist_and_are_in_the_table():
    lib = _native.lib()
    header = (shc.ROOT / "include" / "rpsf.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in _native._PROTOTYPES and getattr(lib, name).argtypes is not None
        assert f"int {name}(" in header
    assert f"#define RPSF_STARS_SHAPE_COLUMNS {len(shc.COLUMNS)}\n" in header


def test_new_entry_points_refuse_null_arguments_without_a_gpu():
    lib = _native.lib()
    n, ms, out = ctypes.c_size_t(7), ctypes.c_double(-1.0), np.zeros(len(shc.COLUMNS))
    fake = ctypes.c_void_p(FAKE)  # must not be looked at before the other arguments are
    calls = [
        lib.rpsf_stars_measure(None, ctypes.byref(n)),
        lib.rpsf_stars_measure(fake, None),
        lib.rpsf_stars_shapes(None, 0, 1, _native._ptr(out)),
        lib.rpsf_stars_shapes(fake, 0, 1, None),
        lib.rpsf_stars_shape_ms(None, ctypes.byref(ms)),
        lib.rpsf_stars_shape_ms(fake, None),
    ]
    assert calls == [_native.E_BADARG] * len(calls)
    assert n.value == 7 and ms.value == -1.0 and not out.any()
