"""Second moments and shape per detection (kernel S5) on the GPU, through the C ABI (regularizepsf_amd.stars._Finder)
and through star_catalog and ArrayPSFBuilder, against the float64 restatement and against the CPU emulator of the same per-thread source
(tests/shape_cases.py) - the cases and checks of tests/test_shapes_host.py.

Measured on an MI355X: see profiles/star_shapes_gpu.log (every check prints its figures before it asserts)."""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import shape_cases as shc
from tests import stars_fused_cases as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tuple(n for n in shc.CASES if n != "background"))
def test_shapes_match_the_restatement_and_the_emulator(name):
    shc.check_shapes(stars._Finder, name)
    case = shc.reference(name)
    rows, shapes = shc.run(stars._Finder, case)
    emu_rows, emu_shapes = shc.run(shc.EmuFinder, case)
    assert rows.tobytes() == emu_rows.tobytes()
    assert shapes.tobytes() == emu_shapes.tobytes()  # the same per-thread source on the CPU: the same bits


def test_pure_background_gives_no_rows_and_no_launch():
    shc.check_empty(stars._Finder)


def test_single_pixels_have_zero_moments_exactly():
    shc.check_single_pixels(stars._Finder)


def test_objects_inside_one_anothers_boxes_keep_their_own_pixels():
    shc.check_enclosure(stars._Finder)


def test_row_counts_around_a_workgroup():
    shc.check_row_counts(stars._Finder, shc.emulator_info()[0])


@pytest.mark.parametrize("name", ("wide", "masked", "pairs 6", "one component, split"))
def test_repeats_are_bit_equal_and_detect_is_untouched(name):
    shc.check_reproducible(stars._Finder, name)


def test_measure_needs_a_detect_of_the_present_frame():
    shc.check_state_errors(stars._Finder, _native.NativeError)


def test_return_codes_on_a_live_handle():
    """No detect yet, a replaced mesh, replaced labels, and ranges outside the rows: RPSF_E_BADARG each, and nothing is written."""
    lib = _native.lib()
    case = shc.reference("one_box")
    finder = stars._Finder(case["frame"].shape, case["box"])
    try:
        count, out = ctypes.c_size_t(9), np.full((5, len(shc.COLUMNS)), -1.0)
        assert lib.rpsf_stars_measure(finder._handle, ctypes.byref(count)) == _native.E_BADARG and b"before" in lib.rpsf_last_error()
        assert lib.rpsf_stars_shapes(finder._handle, 0, 0, None) == 0  # no rows, none asked for
        assert lib.rpsf_stars_shapes(finder._handle, 0, 1, _native._ptr(out)) == _native.E_BADARG
        rows = stars.frame_stars(finder, case["frame"], None, 3.0, 5, None)
        assert len(rows) == 4 and lib.rpsf_stars_shapes(finder._handle, 0, 1, _native._ptr(out)) == _native.E_BADARG  # detected, not measured
        shapes = finder.measure()
        assert finder.shape_ms() > 0.0
        for first, n in ((0, 5), (1, 4), (4, 1), (5, 0), (2, ctypes.c_size_t(-1).value)):
            assert lib.rpsf_stars_shapes(finder._handle, first, n, _native._ptr(out)) == _native.E_BADARG, (first, n)
        assert np.all(out == -1.0)
        assert lib.rpsf_stars_shapes(finder._handle, 4, 0, _native._ptr(out)) == 0
        assert lib.rpsf_stars_shapes(finder._handle, 1, 2, _native._ptr(out)) == 0 and out[:2].tobytes() == shapes[1:3].tobytes()
        assert np.all(out[2:] == -1.0)
        level, rms = np.full(finder.mesh_shape, 10.0), np.full(finder.mesh_shape, 0.3)
        finder.filter_mesh(level, rms, 3.0)  # S1b on the caller's meshes: the finder's meshes are replaced
        assert lib.rpsf_stars_measure(finder._handle, ctypes.byref(count)) == _native.E_BADARG and b"replaced" in lib.rpsf_last_error()
        stars.frame_stars(finder, case["frame"], None, 3.0, 5, None)
        assert finder.measure().tobytes() == shapes.tobytes()
        finder.label(np.ones(finder.shape, bool))  # S3 alone: the labels are replaced
        assert lib.rpsf_stars_measure(finder._handle, ctypes.byref(count)) == _native.E_BADARG
        assert count.value == 9
        finder.background_device(case["frame"], None)  # the fused route: measure after detect_device
        assert lib.rpsf_stars_measure(finder._handle, ctypes.byref(count)) == _native.E_BADARG
        fused = finder.detect_device(3.0, 5, None)
        assert fused.tobytes() == rows.tobytes() and finder.measure().tobytes() == shapes.tobytes()
    finally:
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ star_catalog
def test_star_catalog_on_host_and_device_frames():
    wide, pairs = shc.reference("wide"), shc.reference("pairs 6")
    host = rp.star_catalog(wide["frame"].astype(np.float32))
    assert host[0].dtype == stars.CATALOG_DTYPE and host[0].shape == (20,)
    assert host[0].tobytes() == stars.catalog_from_shapes(shc.run(stars._Finder, wide)[1]).tobytes()
    found = rp.find_stars(wide["frame"].astype(np.float32))
    assert np.stack([host[0]["row"], host[0]["col"]], axis=-1).tobytes() == found[0].tobytes()
    device = rp.star_catalog(rp.to_device(wide["frame"].astype(np.float32)))
    assert device[0].tobytes() == host[0].tobytes()
    frames = np.stack([wide["frame"], pairs["frame"]]).astype(np.float32)
    for options in ({}, {"deblend": True}):
        on_host, on_device = rp.star_catalog(frames, **options), rp.star_catalog(rp.to_device(frames), **options)
        assert [len(c) for c in on_host] == ([20, 24] if options else [20, 12])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(on_host, on_device))
        positions = rp.find_stars(frames, **options)
        assert all(np.stack([c["row"], c["col"]], axis=-1).tobytes() == p.tobytes() for c, p in zip(on_host, positions))
    masked = shc.reference("masked")
    hidden = rp.star_catalog(masked["frame"], mask=masked["mask"])
    assert hidden[0].tobytes() == rp.star_catalog(rp.to_device(masked["frame"]), mask=masked["mask"])[0].tobytes() and len(hidden[0]) == 17
    empty = rp.star_catalog(shc.reference("background")["frame"], box=32)
    assert empty[0].shape == (0,) and empty[0].dtype == stars.CATALOG_DTYPE
    nothing = rp.star_catalog(rp.to_device(np.full((40, 48), np.nan, np.float32)), box=32)  # no usable box: T = +inf on the device
    assert nothing[0].shape == (0,) and nothing[0].dtype == stars.CATALOG_DTYPE


# ------------------------------------------------------------------------------------------------------------------ the build
def test_build_takes_catalogues():
    frames = [shc.reference("wide")["frame"], shc._frame((150, 200), 32, shc._ellipses, 4)["frame"]]  # round stars, elliptical stars
    catalogs, found = rp.star_catalog(frames, box=32), rp.find_stars(frames, box=32)
    assert [len(c) for c in catalogs] == [20, 8]
    want = rp.ArrayPSFBuilder(16).build(frames, stars=found, return_patches=True)
    got = rp.ArrayPSFBuilder(16).build(frames, stars=catalogs, return_patches=True)
    fc.assert_same_build(got, want, "catalogues")
    assert [sum(key[0] == i for key in got[2]) for i in (0, 1)] == [20, 8]  # every star gave a patch
    # the selection idiom: the ellipses go, and exactly their stars leave the patches and the counts
    chosen = [c[c["elongation"] < 1.5] for c in catalogs]
    assert [len(c) for c in chosen] == [20, 0]
    fewer = rp.ArrayPSFBuilder(16).build(frames, stars=chosen, return_patches=True)
    fc.assert_same_build(fewer, rp.ArrayPSFBuilder(16).build(frames, stars=[found[0], found[1][:0]], return_patches=True), "filtered")
    assert list(fewer[2]) == [key for key in got[2] if key[0] == 0]
    only_first = rp.ArrayPSFBuilder(16).build(frames[:1], stars=found[:1])[1]
    assert fewer[1] == only_first and fewer[1] != got[1]  # the counts of the round stars alone
    assert all(fewer[1][corner] <= got[1][corner] for corner in got[1])
