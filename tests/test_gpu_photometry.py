"""Forced aperture photometry (DESIGN.md 3.7 "Apertures", kernel S6) on the GPU, through the C ABI (regularizepsf_amd.stars._Finder) and
through star_photometry, against the float64 restatement and against the CPU emulator of the same per-thread source
(tests/photometry_cases.py) - the cases and checks of tests/test_photometry_host.py.

Measured on an MI355X: see profiles/star_photometry_gpu.log (every check prints its figures before it asserts)."""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import photometry_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tuple(n for n in pc.CASES if not n.endswith(" rows")))
def test_sums_and_counts_match_the_restatement_and_the_emulator(name):
    pc.check_case(stars._Finder, name)
    c = pc.case(name)
    level_f, rows = pc.run(stars._Finder, c)
    emu_level_f, emu_rows = pc.run(pc.EmuFinder, c)
    assert (level_f is None) == (emu_level_f is None) and (level_f is None or level_f.tobytes() == emu_level_f.tobytes())
    assert rows.tobytes() == emu_rows.tobytes()  # the same per-thread source on the CPU: the same bits


def test_hard_positions():
    pc.check_hard_positions(stars._Finder)


def test_exact_cases():
    pc.check_exact(stars._Finder)


def test_a_frame_without_a_usable_pixel():
    pc.check_unusable(stars._Finder)


def test_row_counts_around_a_workgroup():
    pc.check_row_counts(stars._Finder, pc.emulator_info()[0])


@pytest.mark.parametrize("name", ("field, mesh", "masked, none", "eight radii, s = 8"))
def test_repeats_are_bit_equal(name):
    pc.check_reproducible(stars._Finder, name)


def test_detect_and_measure_are_untouched():
    pc.check_isolation(stars._Finder)


def test_state_and_argument_errors():
    pc.check_errors(stars._Finder, _native.NativeError)


def test_positions_and_return_codes_on_a_live_handle():
    """rpsf_stars_positions after a photometry gives the bits it gave before; RPSF_E_STATE and RPSF_E_BADARG write nothing; n = 0 launches
    nothing and needs no pointers."""
    lib = _native.lib()
    c = pc.case("field, mesh")
    finder = stars._Finder(c["frame"].shape, c["box"])
    try:
        radii, out, ms = np.array([2.0, 4.0]), np.full((2, pc.columns(2)), -1.0), ctypes.c_double(-1.0)
        pos = np.ascontiguousarray(c["positions"][:2])
        args = (finder._handle, 2, _native._ptr(pos), 2, _native._ptr(radii), 5, 1, _native._ptr(out))
        assert lib.rpsf_stars_photometry(*args) == _native.E_STATE and b"before" in lib.rpsf_last_error()
        assert lib.rpsf_stars_photometry(finder._handle, 0, None, 2, _native._ptr(radii), 5, 1, None) == _native.E_STATE
        finder.background_device(c["frame"], None)
        rows = finder.detect_device(3.0, 5, None)
        before = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(before)) == 0
        assert lib.rpsf_stars_photometry(*args) == 0 and not np.any(out == -1.0)
        assert lib.rpsf_stars_photometry_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value > 0.0
        after = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(after)) == 0
        assert after.tobytes() == before.tobytes() == rows.tobytes()
        assert lib.rpsf_stars_photometry(finder._handle, 0, None, 2, _native._ptr(radii), 5, 1, None) == 0  # nothing to launch
        assert lib.rpsf_stars_photometry_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value == 0.0
        kept = out.copy()
        assert lib.rpsf_stars_photometry(finder._handle, 2, _native._ptr(pos), 2, _native._ptr(radii[::-1].copy()), 5, 1,
                                         _native._ptr(out)) == _native.E_BADARG
        assert out.tobytes() == kept.tobytes()
    finally:
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ star_photometry
def test_star_photometry_on_host_and_device_frames():
    c, masked = pc.case("field, mesh"), pc.case("masked, mesh")
    frame, radii = c["frame"].astype(np.float32), (2.0, 4.0, 8.0)
    cat = rp.star_catalog(frame, box=32)
    assert len(cat[0]) == 8
    host = rp.star_photometry(frame, cat, radii, box=32)
    assert host[0].dtype == stars.photometry_dtype(3) and host[0].shape == (8,)
    plain = np.stack([cat[0]["row"], cat[0]["col"]], axis=-1)
    _, rows = pc.run(stars._Finder, {**c, "positions": plain})
    assert host[0].tobytes() == stars.photometry_from_sums(rows, radii, 5).tobytes()
    assert np.all(np.hypot(host[0]["drow"], host[0]["dcol"]) < 0.05) and np.all(host[0]["coverage"] == 1.0)
    for options in ({}, {"background": "none"}, {"subpix": 8}):  # a DeviceArray frame gives the host frame's bits
        on_host = rp.star_photometry(frame, cat, radii, box=32, **options)
        on_device = rp.star_photometry(rp.to_device(frame), cat, radii, box=32, **options)
        assert on_host[0].tobytes() == on_device[0].tobytes(), options
    frames = np.stack([frame, masked["frame"].astype(np.float32)])
    masks = [np.zeros(pc.SHAPE, bool), masked["mask"]]
    on_host = rp.star_photometry(frames, [plain, plain[:3]], radii, masks, box=32)
    on_device = rp.star_photometry(rp.to_device(frames), [plain, plain[:3]], radii, masks, box=32)
    assert [len(r) for r in on_host] == [8, 3] and all(a.tobytes() == b.tobytes() for a, b in zip(on_host, on_device))
    assert on_host[0].tobytes() == host[0].tobytes()
    nothing = rp.star_photometry(rp.to_device(np.full(pc.SHAPE, np.nan, np.float32)), [plain], radii, box=32)[0]
    assert np.isnan(nothing["flux"]).all() and np.all(nothing["area"] == 0.0) and np.isnan(nothing["half_light_radius"]).all()
