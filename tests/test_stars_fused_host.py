"""The fused star finding without a GPU: kernel S1b on the CPU emulator against stars.filter_mesh bit for bit, the
Python surface of ``ArrayPSFBuilder(..., finder=...)`` and of device frames, and the new C entry points' argument checks."""

import ctypes
import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from regularizepsf_amd.device_array import DeviceArray
from tests import stars_fused_cases as fc

BASE = 0x7F0000000000  # an address nobody dereferences


# ------------------------------------------------------------------------------------------------------------------ S1b
@pytest.mark.parametrize("many", [0, 1], ids=["one workgroup", "many workgroups"])
def test_s1b_equals_filter_mesh_bit_for_bit(many):
    """Every shape, invalid share and kind of the table at both thresholds, on either route of the kernel."""
    fc.check_filter_mesh(lambda level, rms, threshold: fc.emu_filter_mesh(level, rms, threshold, many))


def test_s1b_above_the_switch_takes_the_many_workgroup_route():
    """A mesh above the switch, on the route the library picks for its size."""
    threads, many_nodes, lds_bytes = ctypes.c_int(0), ctypes.c_long(0), ctypes.c_long(0)
    fc.emulator().emusm_info(ctypes.byref(threads), ctypes.byref(many_nodes), ctypes.byref(lds_bytes))
    assert fc.LARGE_MESH_SHAPE[0] * fc.LARGE_MESH_SHAPE[1] > many_nodes.value >= 4096  # 4096^2 / 64 stays with the one workgroup
    assert 40 * 50 > threads.value and lds_bytes.value <= 8192
    fc.check_filter_mesh(lambda level, rms, threshold: fc.emu_filter_mesh(level, rms, threshold, -1), fc.mesh_table((fc.LARGE_MESH_SHAPE,)))


def test_s1b_table_covers_what_it_claims():
    fc.emulator()  # (the table is the kernel's: no kernel, no table)
    names = [name for name, _, _ in fc.mesh_table()]
    assert len(names) == len(set(names)) == len(fc.MESH_SHAPES) * (2 + 5 * 3)
    for name, level, rms in fc.mesh_table():
        bad_level, bad_rms = ~np.isfinite(level), ~np.isfinite(rms)
        if " level" in name:
            assert bad_level.any() or level.size < 12
            assert not bad_rms.any()
        if " rms" in name:
            assert not bad_level.any()
        if "100%" in name:
            assert (bad_level | bad_rms).all()
    assert any(np.isinf(level).any() or np.isinf(rms).any() for name, level, rms in fc.mesh_table() if "inf" in name)
    ties = [level for name, level, _ in fc.mesh_table() if name == "16x16 0% ties"][0]
    assert len(np.unique(ties)) < ties.size // 4


def test_s1b_result_does_not_depend_on_the_threshold_except_T():
    _, level, rms = [c for c in fc.mesh_table() if c[0] == "9x13 30% both"][0]
    a, b = fc.emu_filter_mesh(level, rms, 3.0), fc.emu_filter_mesh(level, rms, 0.1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    assert a[3] == 3.0 * a[2] and b[3] == 0.1 * b[2]


# ------------------------------------------------------------------------------------------------------------------ Python surface
def test_finder_keyword_is_validated():
    assert rp.ArrayPSFBuilder(16).finder == "sep"
    assert rp.ArrayPSFBuilder(16, finder="device").finder == "device"
    with pytest.raises(ValueError, match=r"finder must be one of \('sep', 'device'\), not 'gpu'"):
        rp.ArrayPSFBuilder(16, finder="gpu")
    parameters = inspect.signature(rp.ArrayPSFBuilder.__init__).parameters
    assert list(parameters) == ["self", "psf_size", "device", "finder", "finder_options", "interpolation", "cleanup"]
    assert all(parameters[name].kind is inspect.Parameter.KEYWORD_ONLY for name in ("interpolation", "cleanup", "finder", "finder_options"))
    assert "finder" not in inspect.signature(rp.ArrayPSFBuilder.build).parameters


def test_finder_options_are_validated():
    rp.ArrayPSFBuilder(16, finder="device", finder_options={"box": 8, "min_area": 3, "max_area": 100})
    rp.ArrayPSFBuilder(16, finder="device", finder_options={})
    with pytest.raises(ValueError, match='only be given with finder="device"'):
        rp.ArrayPSFBuilder(16, finder_options={"box": 32})
    with pytest.raises(ValueError, match="finder_options is a dict"):
        rp.ArrayPSFBuilder(16, finder="device", finder_options={"threshold": 3})
    with pytest.raises(ValueError, match="finder_options is a dict"):
        rp.ArrayPSFBuilder(16, finder="device", finder_options=[("box", 32)])
    for box in (7, 129):
        with pytest.raises(ValueError, match=f"box must lie in 8 ... 128, got {box}"):
            rp.ArrayPSFBuilder(16, finder="device", finder_options={"box": box})


def test_default_finder_still_needs_sep():
    frame = np.zeros((40, 40))
    with pytest.raises(ImportError, match="stars="):
        rp.ArrayPSFBuilder(16).build([frame])
    with pytest.raises(ImportError, match="stars="):
        rp.ArrayPSFBuilder(16, finder="sep").build([frame])


def test_found_stars_is_none_before_a_build():
    assert rp.ArrayPSFBuilder(16, finder="device").found_stars is None
    assert rp.ArrayPSFBuilder(16).found_stars is None


def test_mixed_and_device_mask_inputs_are_type_errors():
    dev = DeviceArray._from_parts(BASE, (40, 48), np.float32)
    host = np.zeros((40, 48), np.float32)
    builder = rp.ArrayPSFBuilder(16, finder="device")
    for call in (lambda: rp.find_stars([dev, host]), lambda: rp.find_stars([host, dev]), lambda: builder.build([dev, host]),
                 lambda: builder.build([host, dev], stars=[np.zeros((0, 2))] * 2)):
        with pytest.raises(TypeError, match="mixes host and device frames"):
            call()
    mask = DeviceArray._from_parts(BASE, (40, 48), np.uint8)
    for call in (lambda: rp.find_stars(host, mask=mask), lambda: rp.find_stars([host], mask=[mask]), lambda: rp.find_stars(dev, mask=mask),
                 lambda: builder.build([host], sep_mask=mask), lambda: builder.build(dev, sep_mask=[mask])):
        with pytest.raises(TypeError, match="masks are host arrays"):
            call()
    with pytest.raises(TypeError, match="scale_image takes host frames"):
        rp.scale_image(dev, 2)
    with pytest.raises(TypeError, match="takes host frames"):
        rp.ArrayPSFBuilder(8, interpolation="device", finder="device").build(dev, interpolation_scale=2)
    with pytest.raises(TypeError, match="sep"):
        rp.ArrayPSFBuilder(16).build(dev)


def test_device_frames_are_validated_before_the_gpu_is_touched():
    with pytest.raises(ValueError, match="lives on device 3"):
        rp.find_stars(DeviceArray._from_parts(BASE, (40, 48), np.float32, device=3))
    with pytest.raises(rp.PSFBuilderError, match="same shape"):
        rp.find_stars([DeviceArray._from_parts(BASE, (40, 48), np.float32), DeviceArray._from_parts(BASE, (40, 50), np.float32)])
    with pytest.raises(rp.IncorrectShapeError):
        rp.find_stars([DeviceArray._from_parts(BASE, (3, 40, 48), np.float32)])
    with pytest.raises(rp.IncorrectShapeError):
        rp.find_stars(DeviceArray._from_parts(BASE, (48,), np.float32))


# ------------------------------------------------------------------------------------------------------------------ C ABI
NEW_SYMBOLS = ("rpsf_stars_background_view", "rpsf_stars_background_host", "rpsf_stars_background_scaled", "rpsf_stars_filter_mesh",
               "rpsf_stars_detect_device", "rpsf_stars_frame", "rpsf_stars_mesh_ms", "rpsf_builder_add_frame_device")


def test_new_symbols_exist_and_are_in_the_table():
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert name in _native._PROTOTYPES and getattr(lib, name).argtypes is not None
    header = (fc.ROOT / "include" / "rpsf.h").read_text()
    assert all(f"int {name}(" in header for name in NEW_SYMBOLS)


def test_new_entry_points_refuse_null_arguments_without_a_gpu():
    lib = _native.lib()
    buf, bytes_ = np.zeros(16), np.zeros(16, np.uint8)
    view = _native.View(BASE, 0, 4, 4, 16, 4)
    count, ptr, ms = ctypes.c_size_t(7), ctypes.c_void_p(), ctypes.c_double(-1.0)
    grms, T, none = ctypes.c_double(-1.0), ctypes.c_double(-1.0), ctypes.c_int(-1)
    fake = ctypes.c_void_p(BASE)  # a handle that must not be looked at before the other arguments are
    calls = [
        lib.rpsf_stars_background_view(None, ctypes.byref(view), None),
        lib.rpsf_stars_background_view(fake, None, None),
        lib.rpsf_stars_background_host(None, _native._ptr(buf), 1, None),
        lib.rpsf_stars_background_host(fake, None, 1, None),
        lib.rpsf_stars_background_scaled(None, _native._ptr(buf), 1, 4, 4, 2, None),
        lib.rpsf_stars_background_scaled(fake, None, 1, 4, 4, 2, None),
        lib.rpsf_stars_filter_mesh(None, _native._ptr(buf), _native._ptr(buf), 3.0, _native._ptr(buf), _native._ptr(buf), ctypes.byref(grms),
                                   ctypes.byref(T), ctypes.byref(none)),
        lib.rpsf_stars_filter_mesh(fake, None, _native._ptr(buf), 3.0, _native._ptr(buf), _native._ptr(buf), ctypes.byref(grms),
                                   ctypes.byref(T), ctypes.byref(none)),
        lib.rpsf_stars_filter_mesh(fake, _native._ptr(buf), _native._ptr(buf), 3.0, _native._ptr(buf), _native._ptr(buf), None,
                                   ctypes.byref(T), ctypes.byref(none)),
        lib.rpsf_stars_detect_device(None, 3.0, 5, -1, ctypes.byref(count)),
        lib.rpsf_stars_detect_device(fake, 3.0, 5, -1, None),
        lib.rpsf_stars_frame(None, ctypes.byref(ptr), None, None),
        lib.rpsf_stars_frame(fake, None, None, None),
        lib.rpsf_stars_mesh_ms(None, ctypes.byref(ms)),
        lib.rpsf_stars_mesh_ms(fake, None),
        lib.rpsf_builder_add_frame_device(None, fake, 10, 10, 1, _native._ptr(buf), _native._ptr(buf), np.inf, 0.0, np.inf, _native._ptr(bytes_)),
        lib.rpsf_builder_add_frame_device(fake, None, 10, 10, 1, _native._ptr(buf), _native._ptr(buf), np.inf, 0.0, np.inf, _native._ptr(bytes_)),
    ]
    assert calls == [_native.E_BADARG] * len(calls)
    assert b"null" in lib.rpsf_last_error()
    assert count.value == 7 and not ptr.value and ms.value == -1.0 and none.value == -1
    # inconsistent arguments, checked before the handle is used
    assert lib.rpsf_builder_add_frame_device(fake, fake, 1, 10, 1, _native._ptr(buf), _native._ptr(buf), np.inf, 0.0, np.inf,
                                             _native._ptr(bytes_)) == _native.E_BADARG and b"2 x 2" in lib.rpsf_last_error()
    assert lib.rpsf_builder_add_frame_device(fake, fake, 10, 10, -1, _native._ptr(buf), _native._ptr(buf), np.inf, 0.0, np.inf,
                                             _native._ptr(bytes_)) == _native.E_BADARG
    assert lib.rpsf_builder_add_frame_device(fake, fake, 10, 10, 1, None, _native._ptr(buf), np.inf, 0.0, np.inf,
                                             _native._ptr(bytes_)) == _native.E_BADARG
    assert lib.rpsf_stars_background_scaled(fake, _native._ptr(buf), 1, 4, 4, 1, None) == _native.E_BADARG and b"scale" in lib.rpsf_last_error()
    assert lib.rpsf_stars_background_scaled(fake, _native._ptr(buf), 1, 3, 4, 2, None) == _native.E_BADARG and b"4 x 4" in lib.rpsf_last_error()


def test_finder_methods_of_the_fused_route_exist():
    for name in ("background_device", "background_scaled", "detect_device", "filter_mesh", "frame_ptr", "mesh_ms"):
        assert callable(getattr(stars._Finder, name))
    assert callable(stars.frame_stars_device)
