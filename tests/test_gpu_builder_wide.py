"""The PSF builder at the wide sizes 129 ... 256 on the GPU (kernels B1w and B3w, a handle of rpsf_builder_create_wide): the cases and
checks of tests/builder_wide_cases.py, which tests/test_builder_wide_host.py runs on the emulators.

1. / 2. B1w per case against float64 SciPy (flags, 1e-5 per patch) and bit for bit against the emulator;
3. isolation: one launch, one launch per star and reversed stars give the same bits; a launch of 2 slots + 3 stars equals the
   emulator, so a slot's second and third star are covered;
4. three handles in turn (wide 256, narrow 128, narrow 16) equal their solo results;
5. B2 alone at N = 129 and 256; 6. frames -> cells; 7. B3w per size and per labelling case, and model = average then clean;
8. the public call on every route; 9. frames -> model -> transform -> corrected frame at 256 pixels.
"""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native
from regularizepsf_amd import builder as bld
from tests import builder_cases as bc
from tests import builder_wide_cases as wc
from tests import cleanup_cases as cc

pytestmark = pytest.mark.gpu


def _bits(a):
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _fill(case, capacity=32, frames=None):
    """The device stack of a case: its frames (or the first `frames` of them) through kernel B1, flags of every star."""
    stack = bld._Stack(case["n"], 0, capacity)
    flags = [stack.add_frame(frame, rounded, shift, *case["thresholds"])
             for frame, rounded, shift in list(zip(case["frames"], case["rounded"], case["shift"]))[:frames]]
    return stack, np.concatenate(flags)


def _one_launch(case):
    stack, flags = _fill(case, frames=1)
    patches = stack.patches()
    stack.close()
    assert 1 < len(patches)
    return patches, flags


# ------------------------------------------------------------------------------------------------ 1. / 2. B1w per case
@pytest.mark.parametrize("name", list(wc.WIDE_CASES))
def test_wide_patches_against_scipy_and_the_emulator(name):
    case = wc.wide_case(name)
    bc.well_posed(case)
    stack, flags = _fill(case)
    got = stack.patches()
    b1_ms, _ = stack.kernel_ms()
    stack.close()
    assert len(got) == int((flags == 1).sum()) and b1_ms > 0.0
    wc.check_patches(name, got, flags)
    emulated, emulated_flags = wc.emu_case(case)
    assert np.array_equal(flags, emulated_flags) and _same_bits(got, emulated[emulated_flags == 1])


# ------------------------------------------------------------------------------------------------ 3. isolation
@pytest.mark.parametrize("name", wc.ISOLATION)
def test_one_launch_per_star_and_reversed_stars_give_the_same_bits(name):
    case = wc.wide_case(name)
    frame, rounded, shift = case["frames"][0], case["rounded"][0], case["shift"][0]
    patches, flags = _one_launch(case)
    alone = bld._Stack(case["n"], 0, 16)  # every star in a launch of its own: always slot 0
    alone_flags = np.concatenate([alone.add_frame(frame, rounded[j:j + 1], shift[j:j + 1], *case["thresholds"]) for j in range(len(rounded))])
    assert np.array_equal(alone_flags, flags) and _same_bits(alone.patches(), patches)
    alone.close()
    back = bld._Stack(case["n"], 0, 16)  # the stars in reversed order: other slots, other neighbours
    back_flags = back.add_frame(frame, rounded[::-1], shift[::-1], *case["thresholds"])
    assert np.array_equal(back_flags[::-1], flags) and _same_bits(back.patches()[::-1], patches)
    back.close()


def test_a_launch_beyond_the_slots_equals_the_emulator():
    case = wc.slot_case()
    stack = bld._Stack(case["n"], 0, len(case["rounded"]))
    slots = ctypes.c_int(0)
    _native.check(_native.lib().rpsf_builder_wide_slots(stack._handle, ctypes.byref(slots)))
    assert slots.value == wc.slots(case["n"]) and len(case["rounded"]) == 2 * slots.value + 3
    flags = stack.add_frame(case["frame"], case["rounded"], case["shift"], np.inf, 0.0, np.inf)
    got = stack.patches()
    stack.close()
    emulated, emulated_flags = wc.emu_patches(case["frame"], case["n"], case["rounded"], case["shift"])
    assert np.array_equal(flags, emulated_flags) and (flags == 1).sum() > 2 * slots.value
    assert (flags[slots.value:] == 1).any() and (flags[2 * slots.value:] == 1).any()  # second and third stars of a slot among them
    assert _same_bits(got, emulated[emulated_flags == 1])


# ------------------------------------------------------------------------------------------------ 4. three handles in turn
def test_three_handles_used_in_turn_equal_their_solo_results():
    cases = [wc.wide_case("n256"), bc.size_case("n128"), bc.size_case("n16")]
    solo = [_one_launch(case) for case in cases]
    stacks = [bld._Stack(case["n"], 0, 4) for case in cases]
    got = [[] for _ in cases]
    for j in range(0, 10, 2):  # two stars of each kernel, then the next handle
        for k, (case, stack) in enumerate(zip(cases, stacks)):
            got[k].append(stack.add_frame(case["frames"][0], case["rounded"][0][j:j + 2], case["shift"][0][j:j + 2], *case["thresholds"]))
    for (want, want_flags), stack, flags in zip(solo, stacks, got):
        assert len(want_flags) == 10 and np.array_equal(np.concatenate(flags), want_flags) and _same_bits(stack.patches(), want)
        stack.close()


# ------------------------------------------------------------------------------------------------ 5. B2 alone
@pytest.mark.parametrize("n", (129, 256))
def test_averaging_at_the_wide_sizes_against_numpy_and_twice_the_same(n):
    case = bc.b2_size_case(n)  # (the grid is cells x ceil(N^2 / 256): 5 x 256 at N = 256)
    stack = bld._Stack(n, 0, 12)
    stack.load(case["stack"])
    assert len(stack) == len(case["stack"])

    def average(method, q):
        return stack.average(method, q, case["offsets"], case["members"])

    first = bc.check_b2(case, average)
    again = bc.check_b2(case, average)
    assert all(_same_bits(first[key], again[key]) for key in first)
    stack.close()


# ------------------------------------------------------------------------------------------------ 6. frames -> cells
@pytest.mark.parametrize("name", wc.END_TO_END)
def test_frames_to_cells_against_the_oracle(name):
    case = wc.wide_case(name)
    stack, flags = _fill(case)
    assert np.array_equal(flags, np.concatenate(case["flags"]))
    wc.check_end_to_end(name, stack.average)
    stack.close()


# ------------------------------------------------------------------------------------------------ 7. B3w
def _clean_checked(case, label):
    stack = bld._Stack(case["cells"].shape[-1], 0, 1)
    out, flags = stack.clean(case["cells"])
    again, flags_again = stack.clean(case["cells"])
    assert stack.clean_ms() > 0.0
    stack.close()
    cc.check(case, out, flags, label)
    emulated, emulated_flags = wc.emu_clean(case["cells"])
    assert np.array_equal(flags, emulated_flags) and cc.same_bits(out, emulated)
    assert np.array_equal(flags, flags_again) and cc.same_bits(out, again)


@pytest.mark.parametrize("n", wc.CLEAN_SIZES)
def test_wide_cleanup_per_size(n):
    _clean_checked(cc.size_case(n), f"GPU N = {n}")


@pytest.mark.parametrize("n", wc.CLEAN_SIZES)
def test_wide_cleanup_on_the_labelling_cells(n):
    _clean_checked(wc.label_case(n), f"GPU labelling N = {n}")


def test_wide_cleanup_beyond_the_slots_and_in_reversed_order():
    cells = np.concatenate([cc.size_case(129)["cells"], wc.label_case(129)["cells"]])
    many = np.concatenate([cells] * (2 * wc.slots(129) // len(cells) + 1))[:2 * wc.slots(129) + 3]
    stack = bld._Stack(129, 0, 1)
    together, flags = stack.clean(many)
    backwards, flags_backwards = stack.clean(many[::-1])
    few, few_flags = stack.clean(cells)
    stack.close()
    assert cc.same_bits(together, backwards[::-1]) and np.array_equal(flags, flags_backwards[::-1])
    for k in range(len(many)):  # whatever the slot and the cell before it in the slot
        assert cc.same_bits(together[k], few[k % len(cells)]) and flags[k] == few_flags[k % len(cells)], k


@pytest.mark.parametrize("name", wc.END_TO_END)
def test_model_is_average_then_clean(name):
    case, want = wc.wide_case(name), wc.end_to_end_case(name)
    stack, _ = _fill(case)
    for method, q in bc.METHODS:
        cells = stack.average(method, q, want["offsets"], want["members"])
        separate, separate_flags = stack.clean(cells)
        fused, fused_flags = stack.model(method, q, want["offsets"], want["members"])
        assert np.array_equal(fused_flags, separate_flags) and cc.same_bits(fused, separate)
        assert cc.same_bits(fused[fused_flags == cc.DEGENERATE], cells[fused_flags == cc.DEGENERATE])
        final = bld.model_on_device(stack, method, q, want["offsets"], want["members"])
        cc.compare_models(final, np.stack([bld.clean_cell(c) for c in cells]), f"{name} {method}")
    stack.close()


def test_a_wide_handle_refuses_the_scaled_entry_points():
    lib, ptr = _native.lib(), _native._ptr
    stack = bld._Stack(129, 0, 1)
    frame, corners, frac, flags = np.zeros((8, 8), np.float32), np.zeros((1, 2), np.int32), np.zeros((1, 2)), np.full(1, 77, np.uint8)
    assert lib.rpsf_builder_add_frame_scaled(stack._handle, ptr(frame), 0, 8, 8, 1, 1, ptr(corners), ptr(frac), np.inf, 0.0, np.inf,
                                             ptr(flags)) == _native.E_UNSUPPORTED
    cells, out = np.ones((1, 129, 129)), np.full((1, 129, 129), 7.0)
    assert lib.rpsf_builder_downscale(stack._handle, 1, ptr(cells), ptr(out)) == _native.E_UNSUPPORTED
    assert flags[0] == 77 and np.all(out == 7.0) and len(stack) == 0
    stack.close()
    with pytest.raises(_native.NativeError) as info:
        bld._Stack(257, 0, 1)
    assert info.value.code == _native.E_UNSUPPORTED and "257" in str(info.value)


# ------------------------------------------------------------------------------------------------ 8. the public call
@pytest.mark.parametrize("name", wc.END_TO_END)
def test_build_with_host_and_device_cleanup(name):
    case = wc.wide_case(name)
    n, frames, stars = case["n"], case["frames"], case["stars"]
    saturation, minimum, maximum = case["thresholds"]
    kw = dict(stars=stars, return_patches=True, saturation_threshold=saturation, star_minimum=minimum, star_maximum=maximum)
    want_keys = [(f, r, c) for f, (corner, flags) in enumerate(zip(case["corner"], case["flags"])) for r, c in corner[flags == 1].tolist()]
    covering = [tuple(c) for c in rp.calculate_covering(frames[0].shape, n)]
    results = {}
    for method, q in bc.METHODS if name == "n129" else bc.METHODS[1:2]:
        for cleanup in bld.CLEANUPS:
            psf, counts, patches = rp.ArrayPSFBuilder(n, cleanup=cleanup).build(frames, average_method=method, percentile=q, **kw)
            assert list(patches) == want_keys and [tuple(c) for c in psf.coordinates] == covering == list(counts)
            stack = np.stack([patches[k] for k in want_keys])
            assert stack.dtype == np.float64 and np.array_equal(stack, stack.astype(np.float32))
            offsets, members = bld.cell_membership(np.array([k[1:] for k in want_keys]), np.array(covering), n)
            assert list(counts.values()) == np.diff(offsets).tolist()
            # the oracle's cells of the patches the build kept, cleaned by clean_cell
            cells = bc.oracle_cells(stack.astype(np.float32), offsets, members, method, q)
            cc.compare_models(psf.values, np.stack([bld.clean_cell(c) for c in cells]), f"build {name} {method} cleanup={cleanup}")
            results[method, cleanup] = (psf.values, stack)
        assert _same_bits(results[method, "host"][1], results[method, "device"][1])
    # the same frames on the device give the bits of the host call
    method, q = bc.METHODS[1]
    on_device = rp.ArrayPSFBuilder(n, cleanup="device").build(rp.to_device(frames.astype(np.float32)), average_method=method, percentile=q, **kw)
    assert _same_bits(on_device[0].values, results[method, "device"][0])
    assert _same_bits(np.stack([on_device[2][k] for k in want_keys]), results[method, "device"][1])


def test_the_fused_route_at_a_wide_size():
    frames = wc.wide_case("n129")["frames"].astype(np.float32)
    builder = rp.ArrayPSFBuilder(129, finder="device")
    fused, fused_counts, fused_patches = builder.build(frames, return_patches=True)
    found = rp.find_stars(frames)
    assert sum(len(f) for f in found) > 3 and all(np.array_equal(a, b) for a, b in zip(found, builder.found_stars))
    plain, counts, patches = rp.ArrayPSFBuilder(129).build(frames, stars=found, return_patches=True)
    assert sum(counts.values()) > 0 and counts == fused_counts and list(patches) == list(fused_patches)
    assert _same_bits(fused.values, plain.values) and all(_same_bits(patches[k], fused_patches[k]) for k in patches)


# ------------------------------------------------------------------------------------------------ 9. frames -> model -> transform -> frame
def test_a_256_pixel_model_corrects_a_frame():
    n, shape = 256, (512, 512)
    frames, stars = bc.make_size_case(shape, n, 1, 1)
    model, counts = rp.ArrayPSFBuilder(n, cleanup="device").build(frames, stars=stars, average_method="mean")
    values = model.values.copy()
    empty = np.isnan(values).all(axis=(1, 2))
    assert values.shape == (len(counts), n, n) and 0 < empty.sum() < len(values) and np.isfinite(values[~empty]).all()
    values[empty] = values[~empty].mean(axis=0)  # a cell without a star takes the mean model, as a caller would have it
    source = rp.ArrayPSF(rp.IndexedCube(model.coordinates, values))
    rows, cols = np.mgrid[0:n, 0:n].astype(np.float64)
    gauss = np.exp(-0.5 * (((rows - n // 2) / 1.2) ** 2 + ((cols - n // 2) / 1.2) ** 2))
    target = rp.ArrayPSF(rp.IndexedCube(model.coordinates, np.broadcast_to(gauss / gauss.sum(), values.shape).copy()))
    transform = rp.ArrayPSFTransform.construct(source, target, 3.0, 0.1)
    assert transform.psf_shape == (n, n) and len(transform) == len(counts)
    out = transform.apply(frames[0])
    assert out.shape == shape and out.dtype == np.float64 and np.isfinite(out).all()
    assert np.abs(out - frames[0]).max() > 0.0  # and it is not the input handed back
