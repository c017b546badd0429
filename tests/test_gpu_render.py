"""Model and residual frames (DESIGN.md 3.7 "Model and residual frames", kernel S10) on the GPU, through the C ABI
(regularizepsf_amd.stars._Finder and ._Model) and through subtract_stars and render_stars, against the float64 restatement bit for bit
and against the CPU emulator of the same per-thread source bit for bit, NaN by position (tests/render_cases.py) - the cases and checks of
tests/test_render_host.py.

Measured on an MI355X: see profiles/star_render_gpu.log (every check prints its figures before it asserts)."""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import fit_cases as fc
from tests import render_cases as rd

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tuple(rd.CASES))
def test_the_frames_match_the_restatement_and_the_emulator(name):
    frames = rd.check_case(stars._Finder, stars._Model, name)
    _, emulated = rd.run(rd.EmuFinder, rd.EmuModel, rd.case(name))
    for key, got in frames.items():  # the same per-thread source on the CPU: the same bits; a NaN the arithmetic makes has the hardware's sign
        assert rd.same_frame(got, emulated[key][0]), (name, key)


def test_the_library_and_the_emulator_share_the_tile_and_the_chunk():
    assert stars.render_info() == rd.emulator_info()[:3]


def test_a_cell_of_nan_fills_its_disc_and_nothing_else():
    rd.check_nan_cell(stars._Finder, stars._Model)


def test_skipped_stars_are_counted_out_and_touch_no_pixel():
    rd.check_skipped(stars._Finder, stars._Model)


def test_list_lengths_around_a_chunk():
    rd.check_chunks(stars._Finder, stars._Model)


def test_a_pixel_adds_its_stars_in_ascending_index():
    rd.check_order(stars._Finder, stars._Model)


def test_the_residual_is_the_fits_own():
    rd.check_tie_to_fit(stars._Finder, stars._Model)


def test_the_round_trip_on_the_finder():
    rd.check_round_trip(stars._Finder, stars._Model)


def test_the_round_trip_through_the_package():
    rd.check_public_round_trip(rp.render_stars, rp.fit_stars, rp.subtract_stars)


def test_fit_positions_then_subtract_stars():
    rd.check_composition(rp.fit_positions, rp.subtract_stars)


@pytest.mark.parametrize("name", ("N = 9", "two chunks and one"))
def test_repeats_are_bit_equal(name):
    rd.check_reproducible(stars._Finder, stars._Model, name)


def test_the_other_kernels_are_untouched_and_a_model_serves_two_finders():
    rd.check_isolation(stars._Finder, stars._Model)


def test_state_and_argument_errors():
    rd.check_errors(stars._Finder, stars._Model, _native.NativeError)


def test_python_argument_errors():
    rd.check_python_errors(rp.subtract_stars, rp.render_stars)


def test_return_codes_and_sentinels_on_a_live_handle():
    """RPSF_E_STATE and RPSF_E_BADARG write nothing - the output and the count keep their sentinels -, rpsf_stars_positions after a render
    gives the bits it gave before, rpsf_stars_render_ms is positive after a launch, n = 0 needs no star pointers (MODEL: zeros, RESIDUAL:
    the frame), and a model of another device is refused."""
    lib = _native.lib()
    c = rd.case("N = 9")
    shape = c["frame"].shape
    finder, model = stars._Finder(shape, c["box"]), stars._Model(c["cube"])
    try:
        out, count, ms = np.full(shape, -7.0), ctypes.c_size_t(77), ctypes.c_double(-1.0)
        pos, flux, cells = np.ascontiguousarray(c["positions"][:4]), np.ascontiguousarray(c["flux"][:4]), np.ascontiguousarray(c["cells"][:4])
        stars_ = (4, _native._ptr(pos), _native._ptr(flux), _native._ptr(cells))
        tail = (1, 0, _native._ptr(out), ctypes.byref(count))  # float64, on the host
        call = lib.rpsf_stars_render
        for mode in (rd.RESIDUAL, rd.RESIDUAL_MESH):
            assert call(finder._handle, model._handle, *stars_, 3.5, mode, *tail) == _native.E_STATE and b"before" in lib.rpsf_last_error()
            assert call(finder._handle, model._handle, 0, None, None, None, 3.5, mode, *tail) == _native.E_STATE
        assert np.all(out == -7.0) and count.value == 77
        finder.background_device(c["frame"], None)
        rows = finder.detect_device(3.0, 5, None)
        before = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(before)) == 0
        assert call(finder._handle, model._handle, *stars_, 3.5, rd.RESIDUAL, *tail) == 0 and not np.any(out == -7.0) and count.value == 4
        assert lib.rpsf_stars_render_ms(finder._handle, ctypes.byref(ms)) == 0 and ms.value > 0.0
        after = np.empty_like(rows)
        assert lib.rpsf_stars_positions(finder._handle, 0, len(rows), _native._ptr(after)) == 0
        assert after.tobytes() == before.tobytes() == rows.tobytes()
        kept = out.copy()
        count.value = 77
        for radius, mode in ((3.75, 1), (0.0, 1), (np.nan, 0), (3.5, 3), (3.5, -1)):
            assert call(finder._handle, model._handle, *stars_, radius, mode, *tail) == _native.E_BADARG, (radius, mode)
        far = np.array([[1.0, 2.0 ** 20]])
        assert call(finder._handle, model._handle, 1, _native._ptr(far), _native._ptr(flux), _native._ptr(cells), 3.5, 0, *tail) == _native.E_BADARG
        assert out.tobytes() == kept.tobytes() and count.value == 77
        assert call(finder._handle, model._handle, 0, None, None, None, 3.5, rd.MODEL, *tail) == 0 and count.value == 0
        assert out.tobytes() == np.zeros(shape).tobytes()
        assert call(finder._handle, model._handle, 0, None, None, None, 3.5, rd.RESIDUAL, 1, 0, _native._ptr(out), None) == 0
        assert rd.same_frame(out, c["frame"].astype(np.float64))
        empty = np.full(shape, np.nan, np.float32)
        finder.background_device(empty, None)  # no usable pixel: RESIDUAL_MESH has nothing to subtract and writes nothing
        out[...] = -7.0
        assert call(finder._handle, model._handle, *stars_, 3.5, rd.RESIDUAL_MESH, *tail) == _native.E_STATE and np.all(out == -7.0)
        if _native.device_count() > 1:
            elsewhere = stars._Model(c["cube"], device=1)
            try:
                assert call(finder._handle, elsewhere._handle, *stars_, 3.5, rd.MODEL, *tail) == _native.E_BADARG
                assert b"another device" in lib.rpsf_last_error() and np.all(out == -7.0)
            finally:
                elsewhere.close()
    finally:
        model.close()
        finder.close()


def test_a_device_out_holds_the_host_results_bytes_and_a_wrong_one_is_refused():
    """Check 7: the kernel writes a DeviceArray given as out=, which is returned, and its bytes are the host result's; a wrong shape,
    dtype, layout or device, or anything that is no DeviceArray, is refused before anything runs (the array keeps its contents)."""
    t = rd.isolated()
    frame, shape = t["frame"], t["frame"].shape
    psf = rp.IndexedCube([(0, 0), (0, 20), (20, 0), (20, 20)], np.ascontiguousarray(t["cube"]))
    flux = [rd.ROUND_TRIP_FLUX]
    for dtype in rd.DTYPES:
        for background in ("none", "mesh"):
            host = rp.subtract_stars(frame, t["positions"], psf, t["radius"], flux=flux, cells=[t["cells"]], background=background, box=t["box"],
                                     dtype=dtype)
            target = rp.to_device(np.full(shape, -7.0, dtype))
            got = rp.subtract_stars(rp.to_device(frame), t["positions"], psf, t["radius"], flux=flux, cells=[t["cells"]], background=background,
                                    box=t["box"], dtype=dtype, out=target)
            assert got[0] is target and target.to_host().tobytes() == host[0].tobytes() and host[0].dtype == dtype
        drawn = rp.render_stars(shape, t["positions"], flux, psf, t["radius"], cells=[t["cells"]], dtype=dtype)
        target = rp.to_device(np.full(shape, -7.0, dtype))
        assert rp.render_stars(shape, t["positions"], flux, psf, t["radius"], cells=[t["cells"]], dtype=dtype, out=[target])[0] is target
        assert target.to_host().tobytes() == drawn[0].tobytes()
    kept = rp.to_device(np.full(shape, -7.0, np.float32))
    wide = rp.to_device(np.full((shape[0], 2 * shape[1]), -7.0, np.float32))
    wrong = [(rp.device_empty((shape[0], shape[1] + 1), np.float32), rp.IncorrectShapeError), (rp.device_empty(shape, np.float64), TypeError),
             (wide[:, ::2], ValueError), (wide[:, :shape[1]], ValueError), (np.zeros(shape, np.float32), TypeError), ([kept, kept], ValueError)]
    for out, error in wrong:
        with pytest.raises(error):
            rp.subtract_stars(frame, t["positions"], psf, t["radius"], flux=flux, cells=[t["cells"]], out=out)
    with pytest.raises(ValueError, match="device"):
        rp.subtract_stars(frame, t["positions"], psf, t["radius"], flux=flux, cells=[t["cells"]], out=kept, device=1)
    assert np.all(kept.to_host() == -7.0) and np.all(wide.to_host() == -7.0)


def test_the_timed_device_copy_copies():
    """rpsf_memcpy_d2d, the yardstick of scripts/render_timing.py: the bytes arrive, and the device time is positive when it is asked for."""
    lib = _native.lib()
    src = rp.to_device(rd.frame())
    dst, ms = rp.device_empty(rd.SHAPE, np.float32), ctypes.c_double(-1.0)
    assert lib.rpsf_memcpy_d2d(0, ctypes.c_void_p(dst.ptr), ctypes.c_void_p(src.ptr), src.nbytes, ctypes.byref(ms)) == 0 and ms.value > 0.0
    assert dst.to_host().tobytes() == rd.frame().tobytes()
    again = rp.device_empty(rd.SHAPE, np.float32)
    assert lib.rpsf_memcpy_d2d(0, ctypes.c_void_p(again.ptr), ctypes.c_void_p(dst.ptr), src.nbytes, None) == 0
    assert again.to_host().tobytes() == rd.frame().tobytes()


def test_a_tile_row_past_the_frames_first_two_to_the_31_bytes():
    """A frame whose float64 output is larger than 2^31 bytes: the pixel index is a size_t.  A star at the far corner lands where the
    restatement puts it, and the first and last rows come back."""
    shape = (16400, 16400)  # 268 960 000 pixels, 2.15e9 bytes of float64
    cube = fc.model(9)
    positions = np.array([(3.25, 4.5), (shape[0] - 4.5, shape[1] - 3.75)])
    flux, cells = np.array([100.0, -50.0]), np.array([rd.GAUSSIAN, rd.LOBES], np.int32)
    finder, model = stars._Finder(shape, 64), stars._Model(cube)
    try:
        target = rp.device_empty(shape, np.float64)
        _, count = finder.render(model, positions, flux, cells, 3.5, rd.MODEL, np.float64, target)
        assert count == 2
        for rows in (slice(0, 8), slice(shape[0] - 9, shape[0])):
            got = target[rows].to_host()
            offset = np.array([rows.start, 0.0])
            want, _ = rd.ref_sum((got.shape[0], shape[1]), cube, positions - offset, flux, cells, 3.5)
            assert rd.same_frame(got, want) and np.count_nonzero(got) > 30
    finally:
        model.close()
        finder.close()
