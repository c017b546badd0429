"""``interpolation_scale`` on the GPU: the upscale kernels U1 / U2 and the block mean B4 of csrc/scale.hip, and scaled builds.

Cases, oracle and criteria are those of tests/scale_cases.py, shared with the emulator tests (tests/test_scale_host.py):
1. ``rpsf_scale_image`` per case within 1e-12 max|frame| of ``RectBivariateSpline`` called as the reference calls it, the data points
   returned exactly (``out[::s, ::s]`` is the input), two runs the same bits.
2. the builder's float32 route (``rpsf_builder_add_frame_scaled``: upscaled on the device into the frame buffer B1 reads) gives the
   patches of the float64 route narrowed once on the host, bit for bit.
3. B4 alone within s^2 2^-53 of each block's largest sample of NumPy's reshape-mean.
4. ``build(..., interpolation_scale=2 and 3)`` for the three averaging methods and both clean-ups against the fixtures of the real
   reference and against the float64 oracle chain, with the builder criteria of tests/test_gpu_builder.py.
5. N = 64, s = 2: the 1024-thread B1 next to the 256-thread B3 in one builder.
"""

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import builder as bld
from tests import builder_cases as bc
from tests import cleanup_cases as cc
from tests import scale_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sc.case_names())
def test_scale_image_against_the_oracle(name):
    case = sc.case(name)
    got = rp.scale_image(case["frame"], case["scale"])
    sc.check_upscale(name, got)
    again = rp.scale_image(case["frame"], case["scale"])
    assert np.array_equal(got.view(np.int64), again.view(np.int64))


def test_scale_image_takes_a_stack_and_a_list_and_reports_its_kernel_times():
    import ctypes

    from regularizepsf_amd import _native

    a, b = sc.case("17x33_s2_f64")["frame"], sc.case("17x33_s3_f64")["frame"]
    stack = rp.scale_image(np.stack([a, b]), 2)
    assert stack.shape == (2, 33, 65) and np.array_equal(stack[0], rp.scale_image(a, 2))
    listed = rp.scale_image([a, b.astype(np.float32)], 3)
    assert isinstance(listed, list) and listed[0].shape == (49, 97) and listed[1].dtype == np.float64
    u1, u2 = ctypes.c_double(-1), ctypes.c_double(-1)
    _native.check(_native.lib().rpsf_scale_kernel_ms(ctypes.byref(u1), ctypes.byref(u2)))
    assert 0 < u1.value < 1000 and 0 < u2.value < 1000


@pytest.mark.parametrize("kind", (np.float32, np.float64))
@pytest.mark.parametrize("name", list(sc.BUILD_CASES))
def test_device_float32_route_is_the_float64_route_narrowed_once(name, kind):
    g = sc.load_build(name)
    scaled_stack = bld._Stack(g["n"], 0, len(g["accepted"]), g["scale"])
    plain_stack = bld._Stack(g["p"], 0, len(g["accepted"]))
    for frame, rounded, shift in zip(g["frames"].astype(kind), sc.per_frame(g, "rounded"), sc.per_frame(g, "shift")):
        on_device = scaled_stack.add_frame(frame, rounded, shift, np.inf, 0.0, np.inf)
        narrowed = rp.scale_image(frame, g["scale"]).astype(np.float32)
        assert np.array_equal(on_device, plain_stack.add_frame(narrowed, rounded, shift, np.inf, 0.0, np.inf))
    got, want = scaled_stack.patches(), plain_stack.patches()
    assert got.shape == want.shape == g["patches"].shape and np.array_equal(got.view(np.int32), want.view(np.int32))
    scaled_stack.close()
    plain_stack.close()


@pytest.mark.parametrize(("n", "scale"), sc.BLOCK_CASES)
def test_block_mean_alone_against_numpy(n, scale):
    stack = bld._Stack(n, 0, 1, scale)
    cells = sc.block_case(n, scale)["cells"]
    got = stack.downscale(cells)
    sc.check_block_mean(n, scale, got)
    assert np.array_equal(got.view(np.int64), stack.downscale(cells).view(np.int64))
    stack.close()


@pytest.mark.parametrize("name", list(sc.BUILD_CASES))
def test_scaled_stack_against_the_reference_patches_and_cells(name):
    g = sc.load_build(name)
    stack = bld._Stack(g["n"], 0, 1, g["scale"])  # smaller than the fill: the stack grows
    flags = [stack.add_frame(frame, rounded, shift, np.inf, 0.0, np.inf)
             for frame, rounded, shift in zip(g["frames"], sc.per_frame(g, "rounded"), sc.per_frame(g, "shift"))]
    sc.check_patches(g, stack.patches(), np.concatenate(flags))
    for method, q in bc.METHODS:
        cells = stack.average(method, q, g["offsets"], g["members"])
        sc.check_cells(cells, g[f"cells_{method}"], f"{name} {method}")
        fused, flags_b3 = stack.model(method, q, g["offsets"], g["members"])  # B2, B4, B3 is B3 on what B2, B4 delivered
        separate, separate_flags = stack.clean(cells)
        assert np.array_equal(flags_b3, separate_flags) and cc.same_bits(fused, separate)
    stack.close()


@pytest.mark.parametrize(("method", "q"), bc.METHODS)
@pytest.mark.parametrize("cleanup", bld.CLEANUPS)
@pytest.mark.parametrize("name", list(sc.BUILD_CASES))
def test_scaled_build_against_the_fixtures_and_the_oracle_chain(name, cleanup, method, q):
    sc.check_build(name, cleanup, method, q)


def test_two_scaled_builds_agree_bit_for_bit_and_scale_one_is_the_plain_build():
    g = sc.load_build("n8s2")
    builder = rp.ArrayPSFBuilder(g["n"], interpolation="device", cleanup="device")
    first, _ = builder.build(g["frames"], interpolation_scale=2, stars=g["stars"], average_method="mean")
    again, _ = builder.build(g["frames"], interpolation_scale=2, stars=g["stars"], average_method="mean")
    assert cc.same_bits(first.values, again.values)
    h = bc.load("n15")
    kw = dict(stars=h["stars"], **bc.thresholds("n15"))
    off, off_counts = rp.ArrayPSFBuilder(15).build(h["frames"], **kw)
    on, on_counts = rp.ArrayPSFBuilder(15, interpolation="device").build(h["frames"], interpolation_scale=1, **kw)
    assert off_counts == on_counts and cc.same_bits(off.values, on.values)


def test_n64_scale_2_runs_the_1024_thread_patch_kernel_with_the_256_thread_clean_up():
    """P = 128 needs B1's 141 KiB of LDS, the model's 64 x 64 cells B3's small launch: one builder sets both up (the
    case and its criteria: scale_cases.check_large_patch_small_model)."""
    stack = bld._Stack(64, 0, 4, 2)
    sc.check_large_patch_small_model(stack)
    stack.close()
