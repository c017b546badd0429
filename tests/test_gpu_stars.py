"""The star finder on the GPU, through the C ABI (regularizepsf_amd.stars._Finder is a thin ctypes wrapper of rpsf_stars_*) and through
find_stars, against the float64 restatement of its definition in tests/star_cases.py - the cases and checks of the emulator tests
(tests/test_stars_host.py), and the end-to-end comparison with ArrayPSFBuilder.build.

Measured on an MI355X: see profiles/star_finder_gpu.log (every check prints its figures before it asserts)."""

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import stars
from regularizepsf_amd.builder import star_geometry
from tests import star_cases as sc

pytestmark = pytest.mark.gpu
FRAMES = tuple(sc.FRAMES)


def test_labels_equal_scipy_with_smallest_index():
    sc.check_labels(stars._Finder)


def test_tile_is_the_emulators():
    finder = stars._Finder((10, 10), 64)
    assert finder.info() == sc.EmuFinder((10, 10), 64).info()
    finder.close()


@pytest.mark.parametrize("name", tuple(sc.CASES))
def test_mesh_matches_the_restatement(name):
    sc.check_mesh(stars._Finder, name)


@pytest.mark.parametrize("name", tuple(sc.CASES))
def test_detections_match_the_restatement(name):
    sc.check_detect(stars._Finder, name)
    if name in sc.FRAMES:
        sc.check_truth(name)


@pytest.mark.parametrize("name", FRAMES)
def test_area_limits_drop_exactly_the_extreme_component(name):
    sc.check_area_limits(stars._Finder, name)


def test_masked_star_pure_background_and_single_component():
    sc.check_special_frames(stars._Finder)


@pytest.mark.parametrize("name", FRAMES)
def test_runs_are_bit_reproducible_and_float64_is_rounded_once(name):
    sc.check_reproducible(stars._Finder, name)


def test_gpu_and_emulator_agree_bit_for_bit():
    """Same phases, same order of every addition: the GPU's rows are the emulator's."""
    for name in sc.CASES:
        case = sc.CASES[name]()
        assert sc.run(stars._Finder, case).tobytes() == sc.run(sc.EmuFinder, case).tobytes(), name


def test_mesh_at_the_largest_and_smallest_box():
    """box = 128 (70 KiB of LDS, 64 samples per thread) and box = 8 (fewer samples than threads) against the restatement."""
    frame = sc.frame_case("wide")["frame"]
    for box in (128, 8):
        want_level, want_rms, gap = sc.ref_mesh(frame, None, box)
        assert gap >= sc.GAP_CLIP, (box, gap)
        finder = stars._Finder(frame.shape, box)
        level, rms = finder.background(frame, None)
        finder.close()
        err = max(np.max(np.abs(level - want_level) / np.abs(want_level)), np.max(np.abs(rms - want_rms) / want_rms))
        print(f"box {box}: mesh {level.shape}, clip gap {gap:.1e} sd, relative error {err:.1e}")
        assert err <= sc.MESH_TOLERANCE


def test_find_stars_takes_what_build_takes():
    frames = [sc.frame_case("tall", offset)["frame"] for offset in (0, 10, 20)]
    together = rp.find_stars(frames, box=32)
    assert [s.shape for s in together] == [(6, 2)] * 3 and all(s.dtype == np.float64 for s in together)
    for frame, found in zip(frames, together):  # a list of three frames equals three single calls
        assert rp.find_stars(frame, box=32)[0].tobytes() == found.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rp.find_stars(np.stack(frames), box=32), together))
    assert rp.find_stars(sc.background_case()["frame"], box=32)[0].shape == (0, 2)
    truth = sc.frame_case("tall")["truth"]
    r, c = np.rint(truth[0]).astype(int)
    mask = np.zeros(frames[0].shape, bool)
    mask[r - 10:r + 11, c - 10:c + 11] = True
    assert [len(s) for s in rp.find_stars(frames, mask=[mask, np.zeros_like(mask), np.zeros_like(mask)], box=32)] == [5, 6, 6]


def test_detect_needs_a_frame_first():
    import ctypes

    from regularizepsf_amd import _native

    finder = stars._Finder((40, 40), 32)
    count = ctypes.c_size_t(0)
    level = np.zeros(finder.mesh_shape)
    rc = _native.lib().rpsf_stars_detect(finder._handle, _native._ptr(level), 1.0, 5, -1, ctypes.byref(count))
    assert rc == _native.E_STATE and b"rpsf_stars_background" in _native.lib().rpsf_last_error()
    level[0, 0] = np.nan
    finder.background(np.zeros((40, 40), np.float32), None)
    assert _native.lib().rpsf_stars_detect(finder._handle, _native._ptr(level), 1.0, 5, -1, ctypes.byref(count)) == _native.E_BADARG
    assert _native.lib().rpsf_stars_positions(finder._handle, 0, 1, _native._ptr(level)) == _native.E_BADARG  # nothing was detected
    finder.close()


def test_build_from_found_stars_equals_build_from_the_restatements():
    """frames -> find_stars -> build against the same build on the restatement's positions."""
    n = 16
    cases = [sc.frame_case("wide", offset) for offset in (0, 10)]
    frames = np.stack([case["frame"] for case in cases])
    found = rp.find_stars(frames)
    want = [case["ref"]["rows"][:, :2] for case in cases]
    for got_pos, case in zip(found, cases):
        rows = case["ref"]["rows"]
        assert got_pos.shape == (len(rows), 2)
        bound = 8 * rows[:, 3] * 2.0 ** -53 * (case["ref"]["abs_flux"] / rows[:, 2]) * max(frames.shape[1:])
        assert np.all(np.abs(got_pos - rows[:, :2]).max(axis=1) <= bound)
        corner_got, rounded_got, _ = star_geometry(got_pos, n)
        corner_want, rounded_want, _ = star_geometry(rows[:, :2], n)
        assert np.all(np.abs(corner_want - np.floor(corner_want) - 0.5) > 1e-6)  # no corner next to a half-integer
        assert np.array_equal(rounded_got, rounded_want)
        assert np.all(np.abs(corner_got - corner_want).max(axis=1) <= bound)  # the patch keys
    psf_a, counts_a, patches_a = rp.ArrayPSFBuilder(n).build(frames, stars=found, return_patches=True)
    psf_b, counts_b, patches_b = rp.ArrayPSFBuilder(n).build(frames, stars=want, return_patches=True)
    assert counts_a == counts_b and sum(counts_a.values()) > 0
    assert len(patches_a) == len(patches_b) > 0
    worst = 0.0
    for (key_a, patch_a), (key_b, patch_b) in zip(patches_a.items(), patches_b.items()):
        assert key_a[0] == key_b[0] and np.allclose(key_a[1:], key_b[1:], rtol=0, atol=1e-9)
        worst = max(worst, float(np.abs(patch_a - patch_b).max() / np.abs(patch_b).max()))
    print(f"{len(patches_a)} patches, worst difference {worst:.2e} of the patch maximum")
    assert worst <= 4 * 2.0 ** -24  # 4 float32 ulp of each patch's maximum
