"""Gaussian-windowed positions (DESIGN.md 3.7 "Windowed positions", kernel S7) on the GPU, through the C ABI
(regularizepsf_amd.stars._Finder), through refine_stars and through the refine_sigma option of the fused build, against the float64 restatement and against the CPU emulator of the same per-thread source (tests/refine_cases.py) - the cases and
checks of tests/test_refine_host.py.

Measured on an MI355X: see profiles/star_refine_gpu.log (every check prints its figures before it asserts)."""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import refine_cases as rc
from tests import stars_fused_cases as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tuple(rc.WALK_CASES))
def test_the_walk_matches_the_restatement_and_the_emulator(name):
    rc.check_walk(stars._Finder, name)
    c = rc.case(name)
    level_f, rows = rc.run(stars._Finder, c)
    emu_level_f, emu_rows = rc.run(rc.EmuFinder, c)
    assert (level_f is None) == (emu_level_f is None) and (level_f is None or level_f.tobytes() == emu_level_f.tobytes())
    assert rows.tobytes() == emu_rows.tobytes()  # the same per-thread source on the CPU: the same bits


def test_hard_positions():
    rc.check_hard_positions(stars._Finder)


@pytest.mark.parametrize("name", tuple(rc.CHAIN_CASES))
def test_the_chain_follows_the_rules_bit_for_bit(name):
    rc.check_chain_case(stars._Finder, name)
    c = rc.case(name)
    assert rc.run(stars._Finder, c)[1].tobytes() == rc.run(rc.EmuFinder, c)[1].tobytes()


def test_every_stop_rule_fires():
    rc.check_stop_rules(stars._Finder)


def test_row_counts_around_a_workgroup():
    rc.check_row_counts(stars._Finder, rc.emulator_info()[0])


@pytest.mark.parametrize("name", ("chain, sigma 2.5", "walk, masked, mesh", "one workgroup, three ends"))
def test_repeats_are_bit_equal(name):
    rc.check_reproducible(stars._Finder, name)


def test_detect_measure_and_photometry_are_untouched():
    rc.check_isolation(stars._Finder)


def test_state_and_argument_errors():
    rc.check_errors(stars._Finder, _native.NativeError)


def test_positions_and_return_codes_on_a_live_handle():
    """rpsf_stars_positions after a refine gives the bits it gave before; RPSF_E_STATE and RPSF_E_BADARG write nothing; n = 0 launches
    nothing and needs no pointers."""
    lib = _native.lib()
    c = rc.case("chain, sigma 1.5")
    finder = stars._Finder(c["frame"].shape, c["box"])
    try:
        out, ms = np.full((2, rc.COLUMNS), -1.0), ctypes.c_double(-1.0)
        pos, sigma = np.ascontiguousarray(c["positions"][:2]), np.array([1.5, 2.5])
        args = (finder._handle, 2, _native._ptr(pos), _native._ptr(sigma), 16, 1e-4, 2.0, 1, _native._ptr(out))
        assert lib.rpsf_stars_refine(*args) == _native.E_STATE and b"before" in lib.rpsf_last_error()
        assert lib.rpsf_stars_refine(finder._handle, 0, None, None, 16, 1e-4, 2.0, 1, None) == _native.E_STATE
        assert np.all(out == -1.0)
        finder.background_device(c["frame"], None)
        rows = finder.detect_device(3.0, 5, None)
        before = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(before)) == 0
        assert lib.rpsf_stars_refine(*args) == 0 and not np.any(out == -1.0)
        assert lib.rpsf_stars_refine_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value > 0.0
        after = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(after)) == 0
        assert after.tobytes() == before.tobytes() == rows.tobytes()
        assert lib.rpsf_stars_refine(finder._handle, 0, None, None, 16, 1e-4, 2.0, 1, None) == 0  # nothing to launch
        assert lib.rpsf_stars_refine_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value == 0.0
        kept = out.copy()
        assert lib.rpsf_stars_refine(finder._handle, 2, _native._ptr(pos), _native._ptr(np.array([1.5, 0.25])), 16, 1e-4, 2.0, 1,
                                     _native._ptr(out)) == _native.E_BADARG
        assert out.tobytes() == kept.tobytes()
    finally:
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ composition
def _failed(rows) -> np.ndarray:
    return (rows["flags"] & (stars.NO_FLUX | stars.RAN_AWAY)) != 0


def test_refine_stars_on_host_and_device_frames():
    field, masked = rc.field(), rc.case("walk, masked, mesh")
    frame, starts = field["frame"].astype(np.float32), rc.whole_pixel_starts()
    host = rp.refine_stars(frame, starts, 1.5, box=32)
    assert host[0].dtype == stars.refine_dtype() and host[0].shape == (8,) and np.all(host[0]["converged"])
    _, rows = rc.run(stars._Finder, rc.case("chain, sigma 1.5"))
    assert host[0].tobytes() == stars.refine_from_sums(rows).tobytes()
    for options in ({}, {"background": "none"}, {"max_iter": 0}, {"max_shift": 0.25, "eps": 1e-2}):  # a DeviceArray frame gives the host frame's bits
        on_host = rp.refine_stars(frame, starts, 2.5, box=32, **options)
        on_device = rp.refine_stars(rp.to_device(frame), starts, 2.5, box=32, **options)
        assert on_host[0].tobytes() == on_device[0].tobytes(), options
    frames = np.stack([frame, masked["frame"].astype(np.float32)])
    masks, sigmas = [np.zeros(rc.SHAPE, bool), masked["mask"]], [np.full(8, 1.5), np.array([1.0, 1.5, 2.5])]
    on_host = rp.refine_stars(frames, [starts, starts[:3]], sigmas, masks, box=32)
    on_device = rp.refine_stars(rp.to_device(frames), [starts, starts[:3]], sigmas, masks, box=32)
    assert [len(r) for r in on_host] == [8, 3] and all(a.tobytes() == b.tobytes() for a, b in zip(on_host, on_device))
    assert on_host[0].tobytes() == host[0].tobytes()
    nothing = rp.refine_stars(rp.to_device(np.full(rc.SHAPE, np.nan, np.float32)), [starts], 1.5, box=32)[0]
    assert np.all(nothing["flags"] == stars.NO_FLUX) and np.isnan(nothing["flux"]).all() and nothing["row"].tobytes() == starts[:, 0].tobytes()
    phot = rp.star_photometry(frame, host, (2.0, 4.0), box=32)[0]
    assert phot["row"].tobytes() == host[0]["row"].tobytes() and np.all(np.hypot(phot["drow"], phot["dcol"]) < 0.05)


def _composed(frames, sigma, mask=None, box=32):
    """What the builder's refine_sigma does, from the public calls: (find_stars' detections, the star list the build must equal)."""
    found = rp.find_stars(frames, 3, mask, box=box)
    rows = rp.refine_stars(frames, found, sigma, mask, box=box)
    kept = sum(int(_failed(r).sum()) for r in rows)
    print(f"refine_sigma = {sigma}: {kept} of {sum(len(f) for f in found)} detections keep their detected position")
    return found, [stars.refined_positions(f, r) for f, r in zip(found, rows)], kept


@pytest.mark.parametrize("sigma", (1.5, 0.5))
def test_the_fused_build_with_refine_sigma_is_the_build_on_the_refined_detections(sigma):
    """The second frame holds two stars six pixels apart, one detection whose iteration runs away: it keeps its detected position."""
    frames = np.stack([rc.field()["frame"], rc.case("between two stars")["frame"]]).astype(np.float32)
    found, refined, kept = _composed(frames, sigma)
    assert [len(f) for f in found] == [8, 3] and kept >= 1 and refined[1][2].tobytes() == found[1][2].tobytes()
    assert all(a.tobytes() != b.tobytes() and a.dtype == np.float64 and a.flags.c_contiguous for a, b in zip(refined, found))
    fused = rp.ArrayPSFBuilder(16, finder="device", finder_options={"box": 32, "refine_sigma": sigma})
    got = fused.build(frames, star_threshold=3)
    assert len(fused.found_stars) == 2 and all(a.tobytes() == b.tobytes() for a, b in zip(fused.found_stars, refined))
    want = rp.ArrayPSFBuilder(16).build(frames, stars=refined)
    fc.assert_same_build(got, want, "refine_sigma")
    assert sum(got[1].values()) > 0
    fc.assert_same_build(fused.build(rp.to_device(frames), star_threshold=3), want, "refine_sigma, device frames")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fused.found_stars, refined))
    plain = rp.ArrayPSFBuilder(16, finder="device", finder_options={"box": 32, "refine_sigma": None})  # None: the detections as they are
    plain.build(frames, star_threshold=3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain.found_stars, found))


def test_the_fused_build_with_refine_sigma_under_a_mask_and_with_deblend():
    frames = np.stack([rc.field()["frame"], rc.case("between two stars")["frame"]]).astype(np.float32)
    mask = np.zeros(rc.SHAPE, bool)
    mask[:48, :48] = True
    found, refined, _ = _composed(frames, 1.5, mask)
    fused = rp.ArrayPSFBuilder(16, finder="device", finder_options={"box": 32, "refine_sigma": 1.5})
    fc.assert_same_build(fused.build(frames, sep_mask=mask, star_threshold=3), rp.ArrayPSFBuilder(16).build(frames, stars=refined), "masked")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fused.found_stars, refined)) and 0 < len(found[0]) < 8
    split = rp.find_stars(frames, 3, box=32, deblend=True)  # the pair comes out as two detections, and both converge
    rows = rp.refine_stars(frames, split, 1.5, box=32)
    assert len(split[1]) == 4 and not _failed(rows[1]).any()
    fused = rp.ArrayPSFBuilder(16, finder="device", finder_options={"box": 32, "deblend": True, "refine_sigma": 1.5})
    fused.build(frames, star_threshold=3)
    assert all(a.tobytes() == stars.refined_positions(f, r).tobytes() for a, f, r in zip(fused.found_stars, split, rows))


def test_the_scaled_fused_build_with_refine_sigma_is_the_build_on_the_refined_detections():
    """interpolation_scale = 2: S7 runs on the finder's scaled frame, and the stars are positions in it."""
    frames = list(fc.scaled_frames())
    found, refined, _ = _composed(rp.scale_image(frames, 2), 2.5)
    assert [len(s) for s in found] == [3, 3] and refined[0].tobytes() != found[0].tobytes()
    want = rp.ArrayPSFBuilder(8, interpolation="device").build(frames, interpolation_scale=2, stars=refined, return_patches=True)
    fused = rp.ArrayPSFBuilder(8, interpolation="device", finder="device", finder_options={"box": 32, "refine_sigma": 2.5})
    fc.assert_same_build(fused.build(frames, interpolation_scale=2, return_patches=True), want, "scaled, refine_sigma")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fused.found_stars, refined))
