"""The fused star finding and build on the GPU.  The reference of every check is the composition of calls that existed
before it - ``find_stars`` on host frames (S1, the host's filter_mesh, S2 - S4) and ``build(frames, stars=...)`` - and equality is of
bytes: the fused route moves no arithmetic, it only keeps the frame and the mesh on the device.

1. S1b through rpsf_stars_filter_mesh against stars.filter_mesh: the table of the CPU test, and a mesh above the switch to many workgroups.
2. detection: found_stars of a fused build equals find_stars, per case of tests/star_cases.py, a fully masked frame, box = 8 meshes.
3. build: fused against build(frames, stars=find_stars(frames)) - methods, sizes, clean-ups, patches, rejections, the edge frame.
4. interpolation_scale = 2.
5. device frames of every layout and dtype in find_stars and in build; the source buffers stay as they were.
6. repeatability and isolation.  7. errors.
"""

import functools

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import stars
from tests import star_cases as sc
from tests import stars_fused_cases as fc

pytestmark = pytest.mark.gpu


def _same_stars(got, want, what=""):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        assert a.dtype == np.float64 and a.ndim == 2 and a.shape == b.shape and a.tobytes() == b.tobytes(), what


# ------------------------------------------------------------------------------------------------------------------ 1. S1b
def _gpu_filter_mesh():
    finders = {}

    def run(level, rms, threshold):
        finder = finders.get(level.shape)
        if finder is None:  # a finder whose mesh has the table's shape: boxes of 8 pixels
            finder = finders[level.shape] = stars._Finder((8 * level.shape[0], 8 * level.shape[1]), 8)
        return finder.filter_mesh(level, rms, threshold)

    return run, finders


def test_s1b_equals_filter_mesh_bit_for_bit():
    run, finders = _gpu_filter_mesh()
    fc.check_filter_mesh(run)
    for finder in finders.values():
        finder.close()


def test_s1b_on_many_workgroups_equals_filter_mesh_bit_for_bit():
    run, finders = _gpu_filter_mesh()
    table = fc.mesh_table((fc.LARGE_MESH_SHAPE,))
    fc.check_filter_mesh(run, tuple(case for case in table if case[0].split()[1] in ("0%", "30%", "100%") and case[0].split()[2] in ("plain", "both", "ties")))
    for finder in finders.values():
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ 2. detection
@pytest.mark.parametrize("name", list(fc.detection_cases()))
def test_found_stars_equal_find_stars(name):
    frame, mask, box = fc.detection_cases()[name]
    want = rp.find_stars(frame, mask=mask, box=box)
    print(f"{name}: mesh {-(-frame.shape[0] // box)} x {-(-frame.shape[1] // box)}, {len(want[0])} stars")
    # find_stars on a device frame takes the fused route
    _same_stars(rp.find_stars(rp.to_device(frame.astype(np.float32)), mask=mask, box=box), want, name)
    if name.startswith("box 8"):
        assert len(want[0]) >= 10
    if name == "box 8 large":  # (a model of 17 000 cells adds nothing to the comparison of the stars)
        return
    builder = rp.ArrayPSFBuilder(16, cleanup="device", finder="device", finder_options={"box": box})
    psf, counts = builder.build(frame, sep_mask=mask)
    _same_stars(builder.found_stars, want, name)
    if name in ("background", "fully masked"):
        assert want[0].shape == (0, 2) and sum(counts.values()) == 0
    else:
        assert len(want[0]) > 0 and sum(counts.values()) > 0


def test_finder_options_reach_the_detector():
    frame = sc.frame_case("wide")["frame"]
    areas = sc.frame_case("wide")["ref"]["rows"][:, 3]
    options = {"box": 64, "min_area": int(areas.min()) + 1, "max_area": int(areas.max()) - 1}
    want = rp.find_stars(frame, 2.5, **options)
    assert 0 < len(want[0]) < len(areas) - 1
    builder = rp.ArrayPSFBuilder(16, finder="device", finder_options=options)
    builder.build(frame, star_threshold=2.5)
    _same_stars(builder.found_stars, want)


# ------------------------------------------------------------------------------------------------------------------ 3. build
@functools.cache
def _stars_of_build_frames():
    return rp.find_stars(list(fc.build_frames()), box=64)


BUILDS = {
    "n16 mean": (16, {"average_method": "mean"}, "host"),
    "n16 median": (16, {"average_method": "median"}, "host"),
    "n16 percentile 30": (16, {"average_method": "percentile", "percentile": 30}, "host"),
    "n16 median, device clean-up": (16, {"average_method": "median"}, "device"),
    "n15": (15, {}, "host"),
    "n128": (128, {}, "host"),
    "n128, device clean-up": (128, {}, "device"),
    "n16 patches": (16, {"return_patches": True}, "host"),
    "n16 rejections": (16, {"return_patches": True, "star_minimum": 150.0, "star_maximum": 330.0, "saturation_threshold": 380.0}, "device"),
}


@pytest.mark.parametrize("name", list(BUILDS))
def test_fused_build_equals_the_composition(name):
    size, kwargs, cleanup = BUILDS[name]
    frames = list(fc.build_frames())
    found = _stars_of_build_frames()
    assert len(found[0]) > 0 and found[1].shape == (0, 2) and len(found[2]) > 0  # a starless frame between two with stars
    want = rp.ArrayPSFBuilder(size, cleanup=cleanup).build(frames, stars=found, **kwargs)
    builder = rp.ArrayPSFBuilder(size, cleanup=cleanup, finder="device")
    got = builder.build(frames, **kwargs)
    fc.assert_same_build(got, want, name)
    _same_stars(builder.found_stars, found, name)
    total = sum(want[1].values())
    assert total > 0
    if "patches" in name or "rejections" in name:
        assert {key[0] for key in want[2]} == {0, 2}  # frame indices survive the starless frame
    if "rejections" in name:
        kept_all = rp.ArrayPSFBuilder(size).build(frames, stars=found, return_patches=True)[2]
        assert 0 < len(want[2]) < len(kept_all)


def test_fused_build_of_the_edge_frame_equals_the_composition():
    """Stars on a corner and on two edges: their corners reach outside the frame, through the reflect map of the gather."""
    case = sc.edge_case()
    found = rp.find_stars(case["frame"], box=case["box"])
    assert len(found[0]) == 4 and found[0].min() < 1.0
    want = rp.ArrayPSFBuilder(16).build(case["frame"], stars=found, return_patches=True)
    builder = rp.ArrayPSFBuilder(16, finder="device", finder_options={"box": case["box"]})
    fc.assert_same_build(builder.build(case["frame"], return_patches=True), want, "edge")
    assert any(key[1] < 0 and key[2] < 0 for key in want[2])


def test_build_with_stars_ignores_the_finder_and_clears_found_stars():
    frames = list(fc.build_frames())
    found = _stars_of_build_frames()
    builder = rp.ArrayPSFBuilder(16, finder="device")
    builder.build(frames)
    assert builder.found_stars is not None
    got = builder.build(frames, stars=found)
    assert builder.found_stars is None
    fc.assert_same_build(got, rp.ArrayPSFBuilder(16).build(frames, stars=found), "stars given")


# ------------------------------------------------------------------------------------------------------------------ 4. scaled
def test_scaled_fused_build_equals_the_composition():
    frames = list(fc.scaled_frames())
    found = rp.find_stars(rp.scale_image(frames, 2), box=32)
    assert [len(s) for s in found] == [3, 3]
    want = rp.ArrayPSFBuilder(8, interpolation="device").build(frames, interpolation_scale=2, stars=found, return_patches=True)
    builder = rp.ArrayPSFBuilder(8, interpolation="device", finder="device", finder_options={"box": 32})
    got = builder.build(frames, interpolation_scale=2, return_patches=True)
    _same_stars(builder.found_stars, found, "scaled")
    fc.assert_same_build(got, want, "scaled")
    assert len(want[2]) == 6 and next(iter(want[2].values())).shape == (16, 16)
    # float32 frames and a mask of the scaled shape
    narrow = [f.astype(np.float32) for f in frames]
    mask = np.zeros((79, 99), bool)
    mask[:40, :50] = True
    found = rp.find_stars(rp.scale_image(narrow, 2), mask=mask, box=32)
    assert [len(s) for s in found] == [2, 2]
    want = rp.ArrayPSFBuilder(8, interpolation="device").build(narrow, interpolation_scale=2, stars=found)
    fc.assert_same_build(builder.build(narrow, sep_mask=mask, interpolation_scale=2), want, "scaled, masked")
    _same_stars(builder.found_stars, found, "scaled, masked")


# ------------------------------------------------------------------------------------------------------------------ 5. device frames
def _device_layouts():
    """name -> (host values the device frame holds, make() -> (device frame, device source array, its host bytes))."""
    frame = sc.frame_case("wide")["frame"]
    h, w = frame.shape
    rng = np.random.default_rng(5)
    out = {}

    def dense(values):
        def make():
            dev = rp.to_device(values)
            return dev, dev, values
        return make

    def pitched(values, fill):
        def make():
            big = np.full((h + 6, w + 12), fill, values.dtype)
            big[3:3 + h, 5:5 + w] = values
            dev = rp.to_device(big)
            return dev[3:3 + h, 5:5 + w], dev, big
        return make

    def strided(values, fill):
        def make():
            big = np.full((h, 2 * w + 3), fill, values.dtype)
            big[:, 1:1 + 2 * w:2] = values
            dev = rp.to_device(big)
            return dev[:, 1:1 + 2 * w:2], dev, big
        return make

    f32 = frame.astype(np.float32)
    f64 = frame * (1 + 1e-9 * rng.standard_normal(frame.shape))  # float64 values that are no float32 values
    assert not np.array_equal(f64, f64.astype(np.float32))
    u16 = np.rint(frame * 50).astype(np.uint16)
    out["dense float32"] = (f32, dense(f32))
    out["pitched float32"] = (f32, pitched(f32, np.nan))
    out["column-strided float32"] = (f32, strided(f32, np.nan))
    out["float64"] = (f64, pitched(f64, np.nan))
    out["uint16"] = (u16, pitched(u16, 65535))
    return out


@pytest.mark.parametrize("name", list(_device_layouts()))
def test_device_frames_equal_host_frames(name):
    values, make = _device_layouts()[name]
    dev, source, source_host = make()
    if name != "dense float32":
        assert not dev.c_contiguous or dev.dtype != np.float32
    want_stars = rp.find_stars(values)
    assert len(want_stars[0]) >= 15
    _same_stars(rp.find_stars(dev), want_stars, name)
    want = rp.ArrayPSFBuilder(16).build(values, stars=want_stars, return_patches=True)
    builder = rp.ArrayPSFBuilder(16, finder="device")
    fc.assert_same_build(builder.build(dev, return_patches=True), want, f"{name}: fused")
    _same_stars(builder.found_stars, want_stars, name)
    fc.assert_same_build(rp.ArrayPSFBuilder(16).build(dev, stars=want_stars, return_patches=True), want, f"{name}: stars given")
    fc.assert_same_build(builder.build([dev], return_patches=True), want, f"{name}: list")
    assert source.to_host().tobytes() == source_host.tobytes(), f"{name}: the source buffer changed"


def test_device_stack_equals_the_list_of_its_frames():
    frames = np.stack([f.astype(np.float32) for f in fc.build_frames()])
    found = _stars_of_build_frames()
    big = np.full((3, frames.shape[1] + 2, frames.shape[2] + 4), np.nan, np.float32)
    big[:, 1:-1, 3:-1] = frames
    dev = rp.to_device(big)
    stack = dev[:, 1:-1, 3:-1]
    _same_stars(rp.find_stars(stack), found, "3-D device stack")
    _same_stars(rp.find_stars([stack[i] for i in range(3)]), found, "list of device frames")
    want = rp.ArrayPSFBuilder(16).build(list(frames), stars=found, return_patches=True)
    builder = rp.ArrayPSFBuilder(16, finder="device")
    fc.assert_same_build(builder.build(stack, return_patches=True), want, "3-D device stack")
    fc.assert_same_build(builder.build([stack[i] for i in range(3)], return_patches=True), want, "list of device frames")
    fc.assert_same_build(rp.ArrayPSFBuilder(16).build(stack, stars=found, return_patches=True), want, "3-D device stack, stars given")
    assert dev.to_host().tobytes() == big.tobytes()


def test_cuda_array_interface_objects_are_device_frames():
    class Foreign:
        def __init__(self, array):
            self._array, self.__cuda_array_interface__ = array, array.__cuda_array_interface__

    frame = sc.frame_case("wide")["frame"].astype(np.float32)
    dev = rp.to_device(frame)
    _same_stars(rp.find_stars([Foreign(dev)]), rp.find_stars(frame))


# ------------------------------------------------------------------------------------------------------------------ 6. repeatability
def test_fused_build_is_repeatable_and_isolated():
    frames = list(fc.build_frames())
    host_stars_before = rp.find_stars(frames)
    host_build_before = rp.ArrayPSFBuilder(16).build(frames, stars=host_stars_before, return_patches=True)
    builder = rp.ArrayPSFBuilder(16, finder="device")
    first = builder.build(frames, return_patches=True)
    first_stars = builder.found_stars
    second = builder.build(frames, return_patches=True)
    fc.assert_same_build(second, first, "the same build twice")
    _same_stars(builder.found_stars, first_stars)
    # another frame shape and box in between
    case = sc.frame_case("tall")
    other = rp.ArrayPSFBuilder(16, finder="device", finder_options={"box": case["box"]})
    other.build(case["frame"])
    assert len(other.found_stars[0]) == 6
    fc.assert_same_build(builder.build(frames, return_patches=True), first, "after another shape")
    # the host route is what it was
    _same_stars(rp.find_stars(frames), host_stars_before, "host find_stars after a fused build")
    fc.assert_same_build(rp.ArrayPSFBuilder(16).build(frames, stars=host_stars_before, return_patches=True), host_build_before,
                         "host build after a fused build")
    fc.assert_same_build(first, host_build_before, "fused")


def test_one_finder_serves_the_host_steps_after_the_fused_ones():
    """rpsf_stars_background / rpsf_stars_detect on a handle that ran the fused route, and back: neither leaves the other anything."""
    case = sc.frame_case("wide")
    finder = stars._Finder(case["frame"].shape, case["box"])
    host = stars.frame_stars(finder, case["frame"], None, 3.0, 5, None)
    fused = stars.frame_stars_device(finder, case["frame"], None, 3.0, 5, None)
    again = stars.frame_stars(finder, case["frame"], None, 3.0, 5, None)
    fused_again = stars.frame_stars_device(finder, rp.to_device(case["frame"].astype(np.float32)), None, 3.0, 5, None)
    assert len(host) == 20 and host.tobytes() == fused.tobytes() == again.tobytes() == fused_again.tobytes()
    assert finder.mesh_ms() > 0
    finder.close()


# ------------------------------------------------------------------------------------------------------------------ 7. errors
def test_degenerate_ring_raises_the_composition_s_error():
    frame = fc.crater_frame()
    found = rp.find_stars(frame, box=32)
    assert len(found[0]) == 1 and np.abs(found[0][0] - (32.3, 31.6)).max() < 1.0
    with pytest.raises(rp.PSFBuilderError) as composed:
        rp.ArrayPSFBuilder(16).build(frame, stars=found)
    assert "no background plane can be fitted" in str(composed.value)
    with pytest.raises(rp.PSFBuilderError) as fused:
        rp.ArrayPSFBuilder(16, finder="device", finder_options={"box": 32}).build(frame)
    assert str(fused.value) == str(composed.value)
    with pytest.raises(rp.PSFBuilderError) as on_device:
        rp.ArrayPSFBuilder(16, finder="device", finder_options={"box": 32}).build(rp.to_device(frame.astype(np.float32)))
    assert str(on_device.value) == str(composed.value)


def test_detect_device_before_a_frame_is_a_state_error():
    from regularizepsf_amd import _native

    finder = stars._Finder((64, 64), 32)
    with pytest.raises(_native.NativeError, match="before"):
        finder.detect_device(3.0, 5, None)
    with pytest.raises(_native.NativeError, match="before"):
        finder.frame_ptr()
    finder.close()
