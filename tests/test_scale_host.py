"""``interpolation_scale`` without a GPU: the upscale's launches (U1 / U2) and the block mean (B4) of csrc/rpsf_core_scale.hpp on the
CPU lane emulator (tests/emu/emu_scale.cpp) against the float64 oracle and with the checks of tests/scale_cases.py - the ones
tests/test_gpu_scale.py runs on the device -, the pivot table against a dense solve, the host side of ``scale_image`` and of
``ArrayPSFBuilder(..., interpolation=...)``, the new entry points' argument checks, and a scaled ``build`` on emulator stand-ins
(``scale_cases.ScaledEmulatedStack`` in place of ``builder._Stack``) against the fixtures the real reference wrote.
"""

import ctypes
import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native
from regularizepsf_amd import builder as bld
from tests import builder_cases as bc
from tests import scale_cases as sc


# ------------------------------------------------------------------------------------------------ kernels on the emulator
@pytest.mark.parametrize("name", sc.case_names())
def test_emulated_upscale_against_the_oracle(name):
    case = sc.case(name)
    got = sc.emu_upscale(case["frame"], case["scale"])
    sc.check_upscale(name, got)
    narrow = sc.emu_upscale(case["frame"], case["scale"], np.float32)  # the builder's route: the same values rounded once
    assert np.array_equal(narrow.view(np.int32), got.astype(np.float32).view(np.int32))


def test_cases_cover_both_input_types_the_pedestal_and_every_boundary():
    names = sc.case_names()
    assert any(n.endswith("_f32") for n in names) and any(n.endswith("_pedestal") for n in names)
    assert sc.case(names[-1])["peak"] > 1e7
    scaled = {sc.scaled_shape(sc.case(n)["frame"].shape, sc.case(n)["scale"]) + sc.case(n)["frame"].shape for n in names}
    hs, ws = {v[0] for v in scaled}, {v[1] for v in scaled}
    w = {v[3] for v in scaled}
    for values, edge in ((hs, 32), (w, 32), (ws, 64), (w, 256), (hs, 256)):  # one size on each side of a tile / a workgroup
        assert any(v in (edge - 1, edge) for v in values) and any(v in (edge + 1, edge + 2) for v in values), (sorted(values), edge)


@pytest.mark.parametrize("m", (4, 5, 6, 7, 40, 257))
def test_pivot_table_against_a_dense_solve(m):
    """The table drives a Thomas elimination of the (1, 4, 1) system of m - 4 unknowns; with it, the second derivatives of a random
    line equal the dense solve of the full m x m not-a-knot system (interior rows 1 4 1, end rows 1 -2 1)."""
    ip = sc.emu_pivots(m)
    assert ip.shape == (m - 4,)
    rng = np.random.default_rng(m)
    y = rng.normal(size=m)
    d = np.zeros(m)
    d[1:-1] = y[2:] - 2 * y[1:-1] + y[:-2]
    full = np.zeros((m, m))
    for i in range(1, m - 1):
        full[i, i - 1:i + 2] = (1, 4, 1)
    full[0, :3] = full[-1, -3:] = (1, -2, 1)
    want = np.linalg.solve(full, 6 * d)
    got = np.zeros(m)
    got[1], got[m - 2] = d[1], d[m - 2]
    n = m - 4
    if n:
        rhs = 6 * d[2:m - 2].copy()
        rhs[0] -= d[1]
        rhs[-1] -= d[m - 2]
        r = np.zeros(n)
        for k in range(n):
            r[k] = (rhs[k] - (r[k - 1] if k else 0.0)) * ip[k]
        for k in range(n - 1, -1, -1):
            got[k + 2] = r[k] - (ip[k] * got[k + 3] if k < n - 1 else 0.0)
        dense = np.linalg.solve(np.diag(np.full(n, 4.0)) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1), rhs)
        assert np.abs(got[2:m - 2] - dense).max() <= 1e-13 * np.abs(dense).max()
    got[0], got[-1] = 2 * got[1] - got[2], 2 * got[-2] - got[-3]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert sc.emulator().emus_pivots(3, None) != 0


@pytest.mark.parametrize(("n", "scale"), sc.BLOCK_CASES)
def test_emulated_block_mean_against_numpy(n, scale):
    sc.check_block_mean(n, scale, sc.emu_block_mean(sc.block_case(n, scale)["cells"], scale))


# ------------------------------------------------------------------------------------------------ host API
def test_scale_image_is_exported_and_validates():
    assert "scale_image" in rp.__all__ and rp.scale_image is bld.scale_image
    sig = inspect.signature(rp.scale_image)
    assert [(p.name, p.kind) for p in sig.parameters.values()] == [
        ("images", inspect.Parameter.POSITIONAL_OR_KEYWORD), ("interpolation_scale", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("device", inspect.Parameter.KEYWORD_ONLY)]
    frame = np.arange(30.0).reshape(5, 6)
    for bad in (0, -2, 1.5, "2", None):
        with pytest.raises(ValueError, match="interpolation_scale"):
            rp.scale_image(frame, bad)
    for small in (np.zeros((3, 9)), np.zeros((9, 3))):
        with pytest.raises(ValueError, match="4 x 4"):
            rp.scale_image(small, 2)
    with pytest.raises(rp.IncorrectShapeError):
        rp.scale_image(np.zeros(7), 2)
    with pytest.raises(TypeError, match="Unsupported type"):
        rp.scale_image("frame.fits", 2)


def test_scale_one_is_a_copy_in_every_form():
    frame = np.arange(30, dtype=np.float32).reshape(5, 6)
    one = rp.scale_image(frame, 1)
    assert one.dtype == np.float64 and one.shape == (5, 6) and np.array_equal(one, frame) and one is not frame
    stack = rp.scale_image(np.stack([frame, 2 * frame]), 1)
    assert stack.shape == (2, 5, 6) and np.array_equal(stack[1], 2 * frame)
    listed = rp.scale_image([frame.astype(np.float64), frame.astype(np.int16)], np.int64(1))
    assert isinstance(listed, list) and len(listed) == 2 and all(a.dtype == np.float64 and np.array_equal(a, frame) for a in listed)
    out = np.full((5, 6), np.nan)
    assert _native.lib().rpsf_scale_image(0, _native._ptr(frame), 0, 5, 6, 1, _native._ptr(out)) == 0 and np.array_equal(out, frame)


def test_interpolation_argument():
    params = list(inspect.signature(rp.ArrayPSFBuilder).parameters.values())
    assert [(p.name, p.default, p.kind) for p in params[-2:]] == [("interpolation", "off", inspect.Parameter.KEYWORD_ONLY),
                                                                  ("cleanup", "host", inspect.Parameter.KEYWORD_ONLY)]
    assert "interpolation" not in inspect.signature(rp.ArrayPSFBuilder.build).parameters
    assert rp.ArrayPSFBuilder(16).interpolation == "off" and rp.ArrayPSFBuilder(16, interpolation="device").interpolation == "device"
    for bad in ("gpu", "Device", "host", None, 1):
        with pytest.raises(ValueError, match="interpolation"):
            rp.ArrayPSFBuilder(16, interpolation=bad)


def test_refusals():
    frames, one = np.zeros((1, 40, 40)), [np.zeros((0, 2))]
    # the default still refuses, and now says how to switch the feature on instead of blaming scikit-image
    with pytest.raises(NotImplementedError, match="interpolation_scale") as info:
        rp.ArrayPSFBuilder(16).build(frames, interpolation_scale=2, stars=one)
    assert 'interpolation="device"' in str(info.value) and "scikit" not in str(info.value)
    on = rp.ArrayPSFBuilder(16, interpolation="device")
    with pytest.raises(NotImplementedError, match="128"):
        on.build(frames, interpolation_scale=9, stars=one)
    for bad in (0, -1, 2.5, "2"):
        for builder in (on, rp.ArrayPSFBuilder(16)):
            with pytest.raises(ValueError, match="interpolation_scale"):
                builder.build(frames, interpolation_scale=bad, stars=one)
    with pytest.raises(ValueError, match="4 x 4"):
        on.build(np.zeros((1, 3, 40)), interpolation_scale=2, stars=one)


def test_new_entry_points_return_codes_for_bad_arguments():
    lib = _native.lib()
    handle = ctypes.c_void_p()
    ms = ctypes.c_double(7.0)
    buf = np.zeros(64)
    assert lib.rpsf_scale_image(0, None, 0, 8, 8, 2, None) == _native.E_BADARG and b"null" in lib.rpsf_last_error()
    assert lib.rpsf_scale_image(0, _native._ptr(buf), 1, 3, 8, 2, _native._ptr(buf)) == _native.E_BADARG  # m < 4
    assert lib.rpsf_scale_image(0, _native._ptr(buf), 1, 8, 8, 0, _native._ptr(buf)) == _native.E_BADARG  # scale < 1
    assert lib.rpsf_scale_kernel_ms(None, None) == _native.E_BADARG
    assert lib.rpsf_scale_kernel_ms(ctypes.byref(ms), None) == 0
    assert lib.rpsf_builder_create_scaled(None, 0, 16, 2, 8) == _native.E_BADARG
    for size, scale in ((3, 2), (16, 9), (65, 2), (128, 2)):  # the model's size or P outside 4..128
        assert lib.rpsf_builder_create_scaled(ctypes.byref(handle), 0, size, scale, 8) == _native.E_UNSUPPORTED and not handle.value
    assert lib.rpsf_builder_create_scaled(ctypes.byref(handle), 0, 16, 0, 8) == _native.E_BADARG and not handle.value
    assert lib.rpsf_builder_add_frame_scaled(None, None, 0, 8, 8, 2, 0, None, None, 1.0, 0.0, 1.0, None) == _native.E_BADARG
    assert lib.rpsf_builder_downscale(None, 1, None, None) == _native.E_BADARG


# ------------------------------------------------------------------------------------------------ a scaled build on the emulators
BUILDS = list(sc.BUILD_CASES)


@pytest.mark.parametrize("name", BUILDS)
def test_host_bookkeeping_of_a_scaled_build_equals_the_reference_exactly(name):
    g = sc.load_build(name)
    p, s = g["p"], g["scale"]
    keys = []
    for i, (pos, rounded, shift, accepted) in enumerate(zip(g["stars"], sc.per_frame(g, "rounded"), sc.per_frame(g, "shift"),
                                                            sc.per_frame(g, "accepted"))):
        corner, got_rounded, got_shift = bld.star_geometry(pos, p)
        assert np.array_equal(got_rounded, rounded) and np.array_equal(got_shift.view(np.int64), shift.view(np.int64))
        keys += [(float(i), r, c) for (r, c), a in zip(corner.tolist(), accepted) if a]
    assert np.array_equal(np.array(keys), g["patch_keys"])
    scaled = bld.scaled_shape(g["frames"][0].shape, s)
    assert scaled == tuple(g["scaled_shape"])
    corners = rp.calculate_covering((scaled[0] * s, scaled[1] * s), p)  # the reference's quirk: the scaled shape times the scale
    assert np.array_equal(corners, g["corners"])
    offsets, members = bld.cell_membership(g["patch_keys"][:, 1:], corners, p)
    assert np.array_equal(offsets, g["offsets"]) and np.array_equal(members, g["members"])
    assert (g["counts"] == 0).any() and (g["counts"] > 1).any()


@pytest.mark.parametrize("name", BUILDS)
def test_emulated_scaled_stack_against_the_reference_patches_and_cells(name):
    g = sc.load_build(name)
    stack = sc.ScaledEmulatedStack(g["n"], 0, 1, g["scale"])
    flags = [stack.add_frame(frame, rounded, shift, np.inf, 0.0, np.inf)
             for frame, rounded, shift in zip(g["frames"], sc.per_frame(g, "rounded"), sc.per_frame(g, "shift"))]
    sc.check_patches(g, stack.patches(), np.concatenate(flags))
    for method, q in bc.METHODS:
        sc.check_cells(stack.average(method, q, g["offsets"], g["members"]), g[f"cells_{method}"], f"{name} {method}")


@pytest.mark.parametrize("cleanup", bld.CLEANUPS)
@pytest.mark.parametrize("name", BUILDS)
def test_scaled_build_on_the_emulators_against_the_fixtures(name, cleanup, monkeypatch):
    monkeypatch.setattr(bld, "_Stack", sc.ScaledEmulatedStack)
    for method, q in bc.METHODS:
        sc.check_build(name, cleanup, method, q)


def test_emulated_stack_with_128_pixel_patches_and_a_64_pixel_model():
    sc.check_large_patch_small_model(sc.ScaledEmulatedStack(64, 0, 4, 2))


def test_scale_one_is_the_same_build_with_either_setting(monkeypatch):
    monkeypatch.setattr(bld, "_Stack", sc.ScaledEmulatedStack)
    g = bc.load("n15")
    kw = dict(stars=g["stars"], return_patches=True, **bc.thresholds("n15"))
    off, off_counts, off_patches = rp.ArrayPSFBuilder(15).build(g["frames"], **kw)
    on, on_counts, on_patches = rp.ArrayPSFBuilder(15, interpolation="device").build(g["frames"], interpolation_scale=1, **kw)
    assert off_counts == on_counts and list(off_patches) == list(on_patches)
    assert np.array_equal(off.values.view(np.int64), on.values.view(np.int64))
    assert all(np.array_equal(off_patches[k], on_patches[k]) for k in off_patches)
