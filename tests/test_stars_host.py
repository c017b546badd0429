"""The star finder without a GPU: the kernels' drivers (csrc/rpsf_core_stars.hpp) on the CPU emulator, through the same cases and
checks as tests/test_gpu_stars.py (tests/star_cases.py), plus what is host code in the product: the mesh filter, the argument
checks of find_stars and the C ABI's return codes."""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import star_cases as sc

FRAMES = tuple(sc.FRAMES)


def test_labels_equal_scipy_with_smallest_index():
    sc.check_labels(sc.EmuFinder)


@pytest.mark.parametrize("name", tuple(sc.CASES))
def test_mesh_matches_the_restatement(name):
    sc.check_mesh(sc.EmuFinder, name)


@pytest.mark.parametrize("name", tuple(sc.CASES))
def test_detections_match_the_restatement(name):
    sc.check_detect(sc.EmuFinder, name)


@pytest.mark.parametrize("name", FRAMES)
def test_the_definition_finds_the_generated_stars(name):
    sc.check_truth(name)


@pytest.mark.parametrize("name", FRAMES)
def test_area_limits_drop_exactly_the_extreme_component(name):
    sc.check_area_limits(sc.EmuFinder, name)


def test_masked_star_pure_background_and_single_component():
    sc.check_special_frames(sc.EmuFinder)


@pytest.mark.parametrize("name", FRAMES)
def test_runs_are_bit_reproducible_and_float64_is_rounded_once(name):
    sc.check_reproducible(sc.EmuFinder, name)


def test_find_stars_on_the_emulator(monkeypatch):
    """find_stars itself with the emulator behind it: the frame and mask forms it takes, one (k, 2) array per frame, a list of
    frames equal to single calls."""
    monkeypatch.setattr(stars, "_Finder", sc.EmuFinder)
    frames = [sc.frame_case("tall", offset)["frame"] for offset in (0, 10, 20)]
    together = rp.find_stars(frames, box=32)
    assert [s.shape for s in together] == [(6, 2)] * 3 and all(s.dtype == np.float64 for s in together)
    for frame, found, offset in zip(frames, together, (0, 10, 20)):
        assert np.array_equal(rp.find_stars(frame, box=32)[0], found)
        assert np.allclose(found, sc.frame_case("tall", offset)["ref"]["rows"][:, :2], rtol=0, atol=1e-10)
    assert all(np.array_equal(a, b) for a, b in zip(rp.find_stars(np.stack(frames), box=32), together))
    assert all(np.array_equal(a, b) for a, b in zip(rp.find_stars((f for f in frames), box=32), together))
    # a mask for all frames, and one per frame: the star under it disappears
    truth = sc.frame_case("tall")["truth"]
    r, c = np.rint(truth[0]).astype(int)
    mask = np.zeros(frames[0].shape, bool)
    mask[r - 10:r + 11, c - 10:c + 11] = True
    assert len(rp.find_stars(frames[0], mask=mask, box=32)[0]) == 5
    per_frame = rp.find_stars(frames, mask=[mask, np.zeros_like(mask), np.zeros_like(mask)], box=32)
    assert [len(s) for s in per_frame] == [5, 6, 6]
    assert rp.find_stars(sc.background_case()["frame"], box=32)[0].shape == (0, 2)
    assert rp.find_stars(np.full((40, 40), np.nan), box=32)[0].shape == (0, 2)  # no usable pixel at all


def test_mesh_filter_fills_and_filters():
    level = np.arange(12, dtype=np.float64).reshape(3, 4)
    rms = np.ones((3, 4))
    level[1, 2], rms[1, 2] = np.nan, np.nan
    got_level, got_rms, global_rms = stars.filter_mesh(level, rms)
    want = sc.ref_filter_mesh(level, rms)
    assert np.array_equal(got_level, want[0]) and np.array_equal(got_rms, want[1]) and global_rms == want[2] == 1.0
    assert stars.filter_mesh(np.full((2, 2), np.nan), np.full((2, 2), np.nan)) is None


def test_bad_arguments_raise_before_anything_runs(monkeypatch):
    monkeypatch.setattr(stars, "_Finder", sc.EmuFinder)
    frame = np.zeros((40, 40), np.float32)
    for box in (7, 129, 0):
        with pytest.raises(ValueError, match="box"):
            rp.find_stars(frame, box=box)
    with pytest.raises(rp.IncorrectShapeError):
        rp.find_stars(np.zeros((2, 3, 4, 5)))
    with pytest.raises(rp.IncorrectShapeError):
        rp.find_stars([np.zeros(5)])
    with pytest.raises(rp.IncorrectShapeError):
        rp.find_stars(frame, mask=np.zeros((40, 41), bool))
    with pytest.raises(ValueError, match="mask"):
        rp.find_stars([frame, frame], mask=[np.zeros((40, 40), bool)])


def test_c_abi_returns_codes_for_bad_arguments():
    """Null handles, null outputs and an unsupported box are return codes with a message, with or without a GPU."""
    lib = _native.lib()
    handle = ctypes.c_void_p()
    assert lib.rpsf_stars_create(None, 0, 10, 10, 64) == _native.E_BADARG and b"null" in lib.rpsf_last_error()
    for box in (7, 129):
        assert lib.rpsf_stars_create(ctypes.byref(handle), 0, 10, 10, box) == _native.E_UNSUPPORTED
        assert str(box).encode() in lib.rpsf_last_error() and not handle.value
    for height, width in ((0, 10), (10, -1)):
        assert lib.rpsf_stars_create(ctypes.byref(handle), 0, height, width, 64) == _native.E_BADARG
    buf = np.zeros(16)
    count, rows, cols, ms = ctypes.c_size_t(7), ctypes.c_int(-1), ctypes.c_int(-1), (ctypes.c_double * 4)()
    assert lib.rpsf_stars_background(None, _native._ptr(buf), 1, None, _native._ptr(buf), _native._ptr(buf)) == _native.E_BADARG
    assert lib.rpsf_stars_detect(None, _native._ptr(buf), 1.0, 5, -1, ctypes.byref(count)) == _native.E_BADARG and count.value == 7
    assert lib.rpsf_stars_positions(None, 0, 0, None) == _native.E_BADARG
    assert lib.rpsf_stars_label(None, _native._ptr(buf), _native._ptr(buf)) == _native.E_BADARG
    assert lib.rpsf_stars_info(None, ctypes.byref(rows), ctypes.byref(cols)) == _native.E_BADARG and rows.value == -1
    assert lib.rpsf_stars_kernel_ms(None, ms) == _native.E_BADARG
    lib.rpsf_stars_destroy(None)  # like free(NULL)
