"""Model and residual frames (DESIGN.md 3.7 "Model and residual frames", kernel S10) without a GPU: the kernel's driver and the host's
tile lists (csrc/rpsf_core_stars_render.hpp) on the CPU emulator against the float64 restatement (tests/render_cases.py), bit for bit -
the cases and checks tests/test_gpu_render.py runs on the GPU - plus what is host code in the product: subtract_stars, render_stars and
the C ABI's declarations."""

import ctypes
import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, build, stars
from tests import render_cases as rd

FAKE = 0x7F0000000000  # a handle nobody dereferences
NEW_SYMBOLS = ("rpsf_stars_render", "rpsf_stars_render_ms", "rpsf_stars_render_info", "rpsf_memcpy_d2d")
PLAIN_CASES = tuple(n for n in rd.CASES if n not in ("skipped stars", "a cell of NaN", "the order of the sum") and "chunk" not in n)


@pytest.mark.parametrize("name", PLAIN_CASES)
def test_the_frames_match_the_restatement(name):
    rd.check_case(rd.EmuFinder, rd.EmuModel, name)


@pytest.mark.parametrize("name", tuple(rd.CASES))
def test_the_tile_lists(name):
    rd.check_lists(name)


def test_a_cell_of_nan_fills_its_disc_and_nothing_else():
    rd.check_nan_cell(rd.EmuFinder, rd.EmuModel)


def test_skipped_stars_are_counted_out_and_touch_no_pixel():
    rd.check_skipped(rd.EmuFinder, rd.EmuModel)


def test_list_lengths_around_a_chunk():
    rd.check_chunks(rd.EmuFinder, rd.EmuModel)


def test_a_pixel_adds_its_stars_in_ascending_index():
    rd.check_order(rd.EmuFinder, rd.EmuModel)


def test_the_residual_is_the_fits_own():
    rd.check_tie_to_fit(rd.EmuFinder, rd.EmuModel)


def test_the_round_trip_on_the_finder():
    rd.check_round_trip(rd.EmuFinder, rd.EmuModel)


@pytest.mark.parametrize("name", ("N = 9", "two chunks and one"))
def test_repeats_are_bit_equal(name):
    rd.check_reproducible(rd.EmuFinder, rd.EmuModel, name)


def test_the_other_kernels_are_untouched_and_a_model_serves_two_finders():
    rd.check_isolation(rd.EmuFinder, rd.EmuModel)


def test_state_and_argument_errors():
    rd.check_errors(rd.EmuFinder, rd.EmuModel, rd.EmuError)


def test_the_tile_the_chunk_and_the_lds():
    """One pixel per thread of a workgroup of 256, and a chunk of records of three doubles and one int."""
    tile_r, tile_c, chunk, _, lds = rd.emulator_info()
    assert tile_r * tile_c == 256 and 1 <= chunk <= 256
    assert lds == chunk * (3 * 8 + 4) and lds % 16 == 0 and lds <= 64 * 1024


# ------------------------------------------------------------------------------------------------------------------ the package on the emulator
@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(stars, "_Finder", rd.EmuFinder)
    monkeypatch.setattr(stars, "_Model", rd.EmuModel)


def test_the_round_trip_through_the_package(emulated):
    rd.check_public_round_trip(rp.render_stars, rp.fit_stars, rp.subtract_stars)


def test_fit_positions_then_subtract_stars(emulated):
    rd.check_composition(rp.fit_positions, rp.subtract_stars)


def test_python_argument_errors():
    rd.check_python_errors(rp.subtract_stars, rp.render_stars)


# ------------------------------------------------------------------------------------------------------------------ surface
def test_the_functions_are_exported_and_say_what_they_are_not():
    for name in ("subtract_stars", "render_stars"):
        assert name in rp.__all__ and getattr(rp, name) is getattr(stars, name)
    parameters = inspect.signature(rp.subtract_stars).parameters
    assert list(parameters) == ["images", "fits", "psf", "radius", "mask", "flux", "cells", "background", "box", "dtype", "out", "return_model",
                                "return_counts", "device"]
    assert parameters["background"].default == "none" and parameters["box"].default == 64 and parameters["dtype"].default is np.float32
    assert all(parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(parameters)[5:])
    assert list(inspect.signature(rp.render_stars).parameters) == ["shape", "stars", "flux", "psf", "radius", "cells", "dtype", "out", "device"]
    text = " ".join(rp.subtract_stars.__doc__.split())
    for phrase in ("NOT a PSF-photometry package's subtraction", "bilinear", "does not conserve flux below the pixel scale",
                   "the disc cuts the model at", "is not subtracted"):
        assert phrase in text, phrase


def test_the_c_abi_declares_binds_and_lists_the_new_calls():
    lib = _native.lib()
    header = (build.PKG.parent / "include" / "rpsf.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in _native._PROTOTYPES and getattr(lib, name).argtypes is not None
        assert f"int {name}(" in header
    assert build.CSRC / "rpsf_core_stars_render.hpp" in build.HEADERS
    assert (stars.RENDER_MODEL, stars.RENDER_RESIDUAL, stars.RENDER_RESIDUAL_MESH) == (rd.MODEL, rd.RESIDUAL, rd.RESIDUAL_MESH)
    for name, value in (("MODEL", 0), ("RESIDUAL", 1), ("RESIDUAL_MESH", 2)):
        assert f"#define RPSF_STARS_RENDER_{name} {value}\n" in header
    assert stars.render_info() == rd.emulator_info()[:3]  # the library's tile and chunk are the emulator's: one header


def test_the_entry_points_check_their_arguments_before_the_handles():
    lib = _native.lib()
    fake, fake_model = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + 4096)  # must not be looked at before the other arguments are
    pos, flux, cells, ms = np.array([[3.0, 4.0]]), np.array([1.0]), np.array([0], np.int32), ctypes.c_double(-1.0)
    out, count = np.full(12, -1.0), ctypes.c_size_t(77)
    p, f, c, o, n = _native._ptr(pos), _native._ptr(flux), _native._ptr(cells), _native._ptr(out), ctypes.byref(count)
    call = lib.rpsf_stars_render
    calls = [
        call(None, fake_model, 1, p, f, c, 2.0, 0, 1, 0, o, n),
        call(fake, None, 1, p, f, c, 2.0, 0, 1, 0, o, n),
        call(fake, fake_model, 1, None, f, c, 2.0, 0, 1, 0, o, n),
        call(fake, fake_model, 1, p, None, c, 2.0, 0, 1, 0, o, n),
        call(fake, fake_model, 1, p, f, None, 2.0, 0, 1, 0, o, n),
        call(fake, fake_model, 1, p, f, c, 2.0, 0, 1, 0, None, n),
        call(fake, fake_model, 0, None, None, None, 2.0, 0, 1, 0, None, None),
        *(call(fake, fake_model, 1, p, f, c, radius, 0, 1, 0, o, n) for radius in (0.0, -2.0, 64.5, np.nan, np.inf)),
        *(call(fake, fake_model, 1, p, f, c, 2.0, mode, 1, 0, o, n) for mode in (-1, 3, 7)),
        call(fake, fake_model, 0, None, None, None, 2.0, 3, 1, 0, o, None),
        *(call(fake, fake_model, 1, _native._ptr(np.array([[3.0, bad]])), f, c, 2.0, 1, 0, 0, o, n)
          for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20)),
        lib.rpsf_stars_render_ms(None, ctypes.byref(ms)),
        lib.rpsf_stars_render_ms(fake, None),
    ]
    assert calls == [_native.E_BADARG] * len(calls)
    assert np.all(out == -1.0) and count.value == 77 and ms.value == -1.0
    assert lib.rpsf_stars_render_info(None, None, None) == 0
