"""The deblend option of the star finder on the GPU, through the C ABI (regularizepsf_amd.stars._Finder) and through find_stars and
ArrayPSFBuilder, against the float64 restatement of D1 - D4 and against the CPU emulator of the same per-thread source
(tests/deblend_cases.py) - the cases and checks of tests/test_deblend_host.py.

Measured on an MI355X: see profiles/deblend_gpu.log (every check prints its figures before it asserts)."""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import deblend_cases as dc
from tests import star_cases as sc
from tests import stars_fused_cases as fc

pytestmark = pytest.mark.gpu


def test_basins_equal_the_restatement():
    dc.check_basins(stars._Finder)


@pytest.mark.parametrize("name", tuple(dc.CASES))
def test_detections_match_the_restatement_and_the_emulator(name):
    dc.check_detect(stars._Finder, name)  # rows, the counts of rpsf_stars_deblend_info, and on blend-free frames on == off bit for bit
    case = dc.CASES[name]()
    first, second = dc.run(stars._Finder, case), dc.run(stars._Finder, case)
    assert first.tobytes() == second.tobytes()  # two runs agree
    assert first.tobytes() == dc.run(dc.EmuFinder, case).tobytes()  # the same per-thread source on the CPU: the same bits


def test_single_component_with_two_cores_is_split():
    dc.check_one_component(stars._Finder)
    case = dc.one_component_case()
    assert dc.run(stars._Finder, case, **dc.ONE_COMPONENT).tobytes() == dc.run(dc.EmuFinder, case, **dc.ONE_COMPONENT).tobytes()


@pytest.mark.parametrize("name", ("wide", "pairs 6", "masked member"))
def test_contrast_one_and_huge_prominence_are_off_and_zero_keeps_every_basin(name):
    dc.check_limits(stars._Finder, name)


def test_off_after_on_leaves_nothing_behind():
    case = dc.pair_case("pairs 6")
    finder = stars._Finder(case["frame"].shape, case["box"])
    try:
        plain = stars.frame_stars(finder, case["frame"], None, 3.0, 5, None)
        assert finder.deblend_info() == (12, 0, 0) and finder.deblend_ms() == 0.0
        assert plain.tobytes() == sc.run(stars._Finder, case).tobytes()  # a finder that was never configured
        finder.set_deblend(True)
        split = stars.frame_stars(finder, case["frame"], None, 3.0, 5, None)
        assert len(split) == 24 and finder.deblend_info() == (12, 24, 12) and finder.deblend_ms() > 0.0
        finder.set_deblend(False)
        assert stars.frame_stars(finder, case["frame"], None, 3.0, 5, None).tobytes() == plain.tobytes()
        assert finder.deblend_info() == (12, 0, 0) and finder.deblend_ms() == 0.0
        assert len(finder.kernel_ms()) == 4 and all(ms > 0 for ms in finder.kernel_ms())
    finally:
        finder.close()


def test_return_codes_on_a_live_handle():
    lib = _native.lib()
    finder = stars._Finder((40, 48), 32)
    try:
        for contrast, prominence in ((-0.1, 1.0), (1.1, 1.0), (float("nan"), 1.0), (0.5, -1.0), (0.5, float("inf"))):
            assert lib.rpsf_stars_set_deblend(finder._handle, 1, contrast, prominence) == _native.E_BADARG
        assert lib.rpsf_stars_set_deblend(finder._handle, 1, 0.0, 0.0) == 0 and lib.rpsf_stars_set_deblend(finder._handle, 1, 1.0, 1e300) == 0
        count = ctypes.c_size_t(5)
        level = np.zeros(finder.mesh_shape)
        assert lib.rpsf_stars_detect(finder._handle, _native._ptr(level), 1.0, 5, -1, ctypes.byref(count)) == _native.E_STATE  # no frame yet
        assert lib.rpsf_stars_detect_device(finder._handle, 3.0, 5, -1, ctypes.byref(count)) == _native.E_STATE
        with pytest.raises(rp.IncorrectShapeError):
            finder.basins(np.zeros((3, 3)), np.ones((3, 3), bool))
    finally:
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ find_stars
def test_device_frames_equal_host_frames():
    case = dc.pair_case("pairs 6")
    frame = case["frame"]
    h, w = frame.shape
    want = rp.find_stars(frame.astype(np.float32), deblend=True)
    assert want[0].shape == (24, 2) and np.allclose(want[0], case["ref"]["rows"][:, :2], rtol=0, atol=1e-9)
    got = rp.find_stars(rp.to_device(frame.astype(np.float32)), deblend=True)
    assert got[0].tobytes() == want[0].tobytes()
    wide = frame * (1 + 1e-9 * np.random.default_rng(5).standard_normal(frame.shape))  # float64 values that are not float32 values
    big = np.full((h + 6, w + 12), np.nan)
    big[3:3 + h, 5:5 + w] = wide
    view = rp.to_device(big)[3:3 + h, 5:5 + w]  # a pitched float64 view
    assert rp.find_stars(view, deblend=True)[0].tobytes() == rp.find_stars(wide, deblend=True)[0].tobytes()
    stack = rp.find_stars(rp.to_device(np.stack([frame, dc.pair_case("pairs 8")["frame"]]).astype(np.float32)), deblend=True)
    assert stack[0].tobytes() == want[0].tobytes() and len(stack[1]) == 24
    assert len(rp.find_stars(rp.to_device(frame.astype(np.float32)))[0]) == 12  # the default is off


# ------------------------------------------------------------------------------------------------------------------ the fused build
def test_fused_build_equals_the_composition():
    frames = [dc.pair_case("pairs 8")["frame"], dc.pair_case("pairs 6")["frame"]]
    found = rp.find_stars(frames, deblend=True)
    assert [len(s) for s in found] == [24, 24]
    want = rp.ArrayPSFBuilder(16).build(frames, stars=found, return_patches=True)
    builder = rp.ArrayPSFBuilder(16, finder="device", finder_options={"deblend": True})
    got = builder.build(frames, return_patches=True)
    fc.assert_same_build(got, want, "deblend")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(builder.found_stars, found))  # the split positions
    plain = rp.ArrayPSFBuilder(16, finder="device")
    counts = plain.build(frames)[1]
    assert [len(s) for s in plain.found_stars] == [12, 12]
    assert sum(got[1].values()) > sum(counts.values()) > 0
    other = rp.ArrayPSFBuilder(16, finder="device", finder_options={"deblend": True, "deblend_contrast": 1.0})  # the options arrive
    other.build(frames)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(other.found_stars, plain.found_stars))


def test_scaled_fused_build_equals_the_composition():
    rng = np.random.default_rng([9, 43])
    frame = dc.blend_frame((40, 50), np.array([(15.2, 15.3), (15.6, 20.4), (30.1, 35.2)]), np.array([300.0, 250.0, 280.0]), rng)
    scaled = rp.scale_image([frame], 2)
    found, plain = rp.find_stars(scaled, box=32, deblend=True), rp.find_stars(scaled, box=32)
    print(f"scaled: {len(plain[0])} detections, {len(found[0])} with the option")
    assert len(plain[0]) == 2 and len(found[0]) == 3  # the pair is one component of the scaled frame and two objects
    want = rp.ArrayPSFBuilder(8, interpolation="device").build([frame], interpolation_scale=2, stars=found, return_patches=True)
    builder = rp.ArrayPSFBuilder(8, interpolation="device", finder="device", finder_options={"box": 32, "deblend": True})
    got = builder.build([frame], interpolation_scale=2, return_patches=True)
    assert builder.found_stars[0].tobytes() == found[0].tobytes()
    fc.assert_same_build(got, want, "scaled, deblend")
