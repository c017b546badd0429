"""The deblend option of the star finder without a GPU: the kernels' drivers (csrc/rpsf_core_stars_deblend.hpp) on the CPU emulator
against the float64 restatement of D1 - D4 (tests/deblend_cases.py) - the cases and checks tests/test_gpu_deblend.py runs on the GPU -
plus what is host code in the product: the option checks of find_stars and ArrayPSFBuilder and the C ABI's return codes."""

import ctypes
import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from regularizepsf_amd.builder import FINDER_OPTIONS
from tests import deblend_cases as dc
from tests import star_cases as sc

NEW_SYMBOLS = ("rpsf_stars_set_deblend", "rpsf_stars_basins", "rpsf_stars_deblend_info", "rpsf_stars_deblend_ms")
FAKE = 0x7F0000000000  # a handle nobody dereferences


def test_basins_equal_the_restatement():
    dc.check_basins(dc.EmuFinder)


@pytest.mark.parametrize("name", tuple(dc.CASES))
def test_detections_match_the_restatement(name):
    dc.check_detect(dc.EmuFinder, name)


def test_single_component_with_two_cores_is_split():
    dc.check_one_component(dc.EmuFinder)


@pytest.mark.parametrize("name", ("wide", "pairs 6", "faint pairs 6", "triple", "masked member"))
def test_contrast_one_and_huge_prominence_are_off_and_zero_keeps_every_basin(name):
    dc.check_limits(dc.EmuFinder, name)


@pytest.mark.parametrize("name", tuple(dc.MEASURED))
def test_the_definition_finds_both_members_of_every_pair(name):
    dc.check_truth(name)


def test_the_emulator_without_the_option_is_the_star_emulator():
    """Off, nothing of D1 - D4 runs: the rows are star_cases.EmuFinder's bit for bit, on blended frames too."""
    for name in ("wide", "pairs 5", "frame edge"):
        case = dc.CASES[name]()
        assert dc.run(dc.EmuFinder, case, deblend=False).tobytes() == sc.run(sc.EmuFinder, case).tobytes()


def test_off_after_on_leaves_nothing_behind():
    case = dc.pair_case("pairs 6")
    finder = dc.EmuFinder(case["frame"].shape, case["box"])
    plain = stars.frame_stars(finder, case["frame"], None, 3.0, 5, None)
    finder.set_deblend(True)
    split = stars.frame_stars(finder, case["frame"], None, 3.0, 5, None)
    finder.set_deblend(False)
    assert len(split) == 2 * len(plain) and stars.frame_stars(finder, case["frame"], None, 3.0, 5, None).tobytes() == plain.tobytes()


# ------------------------------------------------------------------------------------------------------------------ Python surface
def test_find_stars_keywords_and_defaults():
    parameters = inspect.signature(rp.find_stars).parameters
    assert list(parameters) == ["images", "threshold", "mask", "box", "min_area", "max_area", "deblend", "deblend_contrast",
                                "deblend_prominence", "device"]
    new = ("deblend", "deblend_contrast", "deblend_prominence")
    assert all(parameters[name].kind is inspect.Parameter.KEYWORD_ONLY for name in new)
    assert [parameters[name].default for name in new] == [False, 0.005, 1.0]
    assert {name: FINDER_OPTIONS[name] for name in new} == stars.DEBLEND_OPTIONS == dict(zip(new, (False, 0.005, 1.0)))
    assert list(FINDER_OPTIONS)[:3] == ["box", "min_area", "max_area"]


@pytest.mark.parametrize("options, text", [
    ({"deblend": 1}, "deblend must be True or False, not 1"),
    ({"deblend": True, "deblend_contrast": -0.1}, "deblend_contrast must lie in 0 ... 1, got -0.1"),
    ({"deblend_contrast": 1.5}, "deblend_contrast must lie in 0 ... 1, got 1.5"),
    ({"deblend_contrast": float("nan")}, "deblend_contrast must lie in 0 ... 1, got nan"),
    ({"deblend_prominence": -1.0}, "deblend_prominence must be finite and not negative, got -1.0"),
    ({"deblend_prominence": float("inf")}, "deblend_prominence must be finite and not negative, got inf"),
])
def test_options_are_validated_before_the_gpu_is_touched(options, text):
    frame = np.zeros((40, 48), np.float32)
    with pytest.raises(ValueError) as caught:
        rp.find_stars(frame, **options)
    assert str(caught.value) == text
    with pytest.raises(ValueError) as caught:
        rp.ArrayPSFBuilder(16, finder="device", finder_options=options)
    assert str(caught.value) == text


def test_finder_options_accept_the_new_keys_only_with_the_device_finder():
    builder = rp.ArrayPSFBuilder(16, finder="device", finder_options={"deblend": True, "deblend_contrast": 0.0, "deblend_prominence": 2})
    assert builder._finder_options == {"box": 64, "min_area": 5, "max_area": None, "deblend": True, "deblend_contrast": 0.0,
                                       "deblend_prominence": 2.0}
    assert rp.ArrayPSFBuilder(16, finder="device")._finder_options["deblend"] is False
    with pytest.raises(ValueError, match='only be given with finder="device"'):
        rp.ArrayPSFBuilder(16, finder_options={"deblend": True})


def test_find_stars_on_the_emulator(monkeypatch):
    """find_stars with the emulator behind it: the option reaches the finder, the default is off, the old calls give what they gave."""
    monkeypatch.setattr(stars, "_Finder", dc.EmuFinder)
    case = dc.pair_case("pairs 8")
    frame, want = case["frame"], case["ref"]["rows"][:, :2]
    split = rp.find_stars(frame, deblend=True)
    assert len(split) == 1 and split[0].shape == (24, 2) and np.allclose(split[0], want, rtol=0, atol=1e-10)
    plain = rp.find_stars(frame)
    assert plain[0].shape == (12, 2) and np.allclose(plain[0], case["plain"]["rows"][:, :2], rtol=0, atol=1e-10)
    for old in (rp.find_stars(frame, 3.0), rp.find_stars(frame, 3.0, None), rp.find_stars(frame, threshold=3.0, mask=None, box=64, min_area=5,
                                                                                            max_area=None, device=0),
                rp.find_stars(frame, deblend=False, deblend_contrast=0.5, deblend_prominence=7.0)):
        assert old[0].tobytes() == plain[0].tobytes()
    both = rp.find_stars([frame, frame], deblend=True, deblend_contrast=1.0)  # no basin holds the component's whole flux but the only one
    assert len(both) == 2 and all(found.tobytes() == plain[0].tobytes() for found in both)
    monkeypatch.setattr(stars, "_Finder", sc.EmuFinder)  # a finder that knows nothing of the option serves the default
    assert rp.find_stars(frame)[0].tobytes() == plain[0].tobytes()


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_exist_and_are_in_the_table():
    lib = _native.lib()
    header = (dc.ROOT / "include" / "rpsf.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in _native._PROTOTYPES and getattr(lib, name).argtypes is not None
        assert f"int {name}(" in header


def test_new_entry_points_refuse_null_and_bad_arguments_without_a_gpu():
    lib = _native.lib()
    buf, flags, peak = np.zeros(16), np.zeros(16, np.uint8), np.zeros(16, np.int32)
    n, ms = ctypes.c_size_t(7), ctypes.c_double(-1.0)
    fake = ctypes.c_void_p(FAKE)  # must not be looked at before the other arguments are
    inf, nan = float("inf"), float("nan")
    calls = [
        lib.rpsf_stars_set_deblend(None, 1, 0.005, 1.0),
        *(lib.rpsf_stars_set_deblend(fake, 1, contrast, 1.0) for contrast in (-1e-9, 1.0 + 1e-9, inf, -inf, nan)),
        *(lib.rpsf_stars_set_deblend(fake, 1, 0.005, prominence) for prominence in (-1e-9, inf, -inf, nan)),
        lib.rpsf_stars_basins(None, _native._ptr(buf), _native._ptr(flags), _native._ptr(peak)),
        lib.rpsf_stars_basins(fake, None, _native._ptr(flags), _native._ptr(peak)),
        lib.rpsf_stars_basins(fake, _native._ptr(buf), None, _native._ptr(peak)),
        lib.rpsf_stars_basins(fake, _native._ptr(buf), _native._ptr(flags), None),
        lib.rpsf_stars_deblend_info(None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)),
        lib.rpsf_stars_deblend_ms(None, ctypes.byref(ms)),
        lib.rpsf_stars_deblend_ms(fake, None),
    ]
    assert calls == [_native.E_BADARG] * len(calls)
    assert n.value == 7 and ms.value == -1.0 and not peak.any()
