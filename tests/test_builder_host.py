"""ArrayPSFBuilder without a GPU: the host API and its errors, the host bookkeeping (corners, shifts, cell membership, counts)
against the reference's exactly, the clean-up stage against the reference's final values, and both kernels' per-thread phases
on the CPU lane emulator (tests/emu/emu_builder.cpp) with the bounds of the GPU tests (tests/test_gpu_builder.py).

Fixtures: tests/golden/builder_*.npz, written by tests/golden/make_builder_golden.py from the real reference with sep replaced
by a lookup of given star positions.
"""

import ctypes
import inspect
import sys

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native
from regularizepsf_amd import builder as bld
from tests import builder_cases as bc

CASES = list(bc.CASES)
TOL = 1e-5  # the project's parity bound, applied per patch and per cell


def _per_frame(g, key):
    return np.split(g[key], np.cumsum(g["stars_per_frame"])[:-1])


# ------------------------------------------------------------------------------------------------ host API
def test_signature_is_the_reference_one_plus_stars():
    sig = inspect.signature(rp.ArrayPSFBuilder.build)
    names = [(p.name, p.default, p.kind) for p in sig.parameters.values()][1:]
    pos = inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert names == [("images", inspect.Parameter.empty, pos), ("sep_mask", None, pos), ("hdu_choice", 0, pos), ("num_workers", None, pos),
                     ("interpolation_scale", 1, pos), ("star_threshold", 3, pos), ("average_method", "median", pos), ("percentile", 50, pos),
                     ("saturation_threshold", np.inf, pos), ("image_mask", None, pos), ("star_minimum", 0, pos),
                     ("star_maximum", np.inf, pos), ("sqrt_compressed", False, pos), ("return_patches", False, pos),
                     ("stars", None, inspect.Parameter.KEYWORD_ONLY)]
    assert rp.ArrayPSFBuilder(24).psf_size == 24
    assert "ArrayPSFBuilder" in rp.__all__


def test_image_argument_errors():
    b = rp.ArrayPSFBuilder(16)
    one = [np.zeros((0, 2))]
    with pytest.raises(rp.IncorrectShapeError, match="must be 3D"):
        b.build(np.zeros(10), stars=one)
    with pytest.raises(rp.IncorrectShapeError, match="must be 3D"):
        b.build(np.zeros((2, 2, 40, 40)), stars=one)
    for bad in ("frame.fits", 3, {"a": 1}, [1, 2], []):
        with pytest.raises(TypeError, match="Unsupported type"):
            b.build(bad, stars=one)
    with pytest.raises(NotImplementedError, match="astropy"):
        b.build(["a.fits", "b.fits"], stars=one * 2)
    with pytest.raises(rp.PSFBuilderError, match=r"Images must all be the same shape\.Found both \(40, 40\) and \(40, 41\)\."):
        b.build([np.zeros((40, 40)), np.zeros((40, 41))], stars=one * 2)
    with pytest.raises(rp.PSFBuilderError, match="same shape"):
        b.build((f for f in [np.zeros((40, 40)), np.zeros((41, 40))]), stars=one * 2)
    # a single 2-D array is one frame (the reference yields it without end)
    frame = np.zeros((40, 40))
    assert len(bld._frames(frame)) == 1 and bld._frames(frame)[0] is frame
    assert len(bld._frames(np.zeros((3, 40, 40)))) == 3


def test_out_of_scope_options_say_so():
    b = rp.ArrayPSFBuilder(16)
    frames = np.zeros((1, 40, 40))
    one = [np.zeros((0, 2))]
    with pytest.raises(NotImplementedError, match="interpolation_scale"):
        b.build(frames, interpolation_scale=2, stars=one)
    with pytest.raises(NotImplementedError, match="image_mask"):
        b.build(frames, image_mask=np.zeros((40, 40), bool), stars=one)
    with pytest.raises(NotImplementedError, match="sqrt_compressed"):
        b.build(frames, sqrt_compressed=True, stars=one)
    with pytest.raises(rp.PSFBuilderError, match="Unknown method mode"):
        b.build(frames, average_method="mode", stars=one)
    with pytest.raises(ValueError, match="2 entries for 1 frames"):
        b.build(frames, stars=one * 2)


def test_star_finding_without_sep_names_the_stars_argument(monkeypatch):
    monkeypatch.setitem(sys.modules, "sep", None)  # import sep -> ImportError, whether or not it is installed
    with pytest.raises(ImportError, match="stars="):
        rp.ArrayPSFBuilder(16).build(np.zeros((1, 40, 40)))


def test_builder_entry_points_return_codes_for_bad_arguments():
    lib = _native.lib()
    handle = ctypes.c_void_p()
    assert lib.rpsf_builder_create(None, 0, 16, 8) == _native.E_BADARG and b"null" in lib.rpsf_last_error()
    for size in (3, 129, -16):
        assert lib.rpsf_builder_create(ctypes.byref(handle), 0, size, 8) == _native.E_UNSUPPORTED
        assert str(size).encode() in lib.rpsf_last_error() and not handle.value
    count = ctypes.c_size_t(7)
    assert lib.rpsf_builder_count(None, ctypes.byref(count)) == _native.E_BADARG and count.value == 7
    assert lib.rpsf_builder_add_frame(None, None, 0, 8, 8, 0, None, None, 1.0, 0.0, 1.0, None) == _native.E_BADARG
    assert lib.rpsf_builder_patches(None, 0, 0, None) == _native.E_BADARG
    assert lib.rpsf_builder_load_patches(None, 0, None) == _native.E_BADARG
    assert lib.rpsf_builder_average(None, 0, 50.0, 1, None, None, None) == _native.E_BADARG
    assert lib.rpsf_builder_kernel_ms(None, None, None) == _native.E_BADARG
    lib.rpsf_builder_destroy(None)


# ------------------------------------------------------------------------------------------------ host bookkeeping
@pytest.mark.parametrize("name", CASES)
def test_corners_shifts_membership_and_counts_equal_the_reference_exactly(name):
    g = bc.load(name)
    n = g["n"]
    keys = []
    for i, (pos, rounded, shift, accepted) in enumerate(zip(g["stars"], _per_frame(g, "rounded"), _per_frame(g, "shift"),
                                                            _per_frame(g, "accepted"))):
        corner, got_rounded, got_shift = bld.star_geometry(pos, n)
        assert got_rounded.dtype == np.int64 and np.array_equal(got_rounded, rounded)
        assert np.array_equal(got_shift.view(np.int64), shift.view(np.int64))
        keys += [(float(i), r, c) for (r, c), a in zip(corner.tolist(), accepted) if a]
    assert np.array_equal(np.array(keys), g["patch_keys"])  # the dict keys, in insertion order
    corners = rp.calculate_covering(g["frames"][0].shape, n)
    assert np.array_equal(corners, g["corners"])
    offsets, members = bld.cell_membership(g["patch_keys"][:, 1:], corners, n)
    assert offsets.dtype == np.int64 and members.dtype == np.int32
    assert np.array_equal(offsets, g["offsets"]) and np.array_equal(members, g["members"])
    assert np.array_equal(np.diff(offsets), g["counts"])
    if name != "n16":
        assert (g["counts"] == 0).any()  # a covering cell without a star


def test_round_half_to_even_corners():
    # position - N / 2 = k + 0.5: Python's round goes to the even neighbour, and the shift amount follows
    _, rounded, shift = bld.star_geometry(np.array([[20.5, 21.5], [8.5, 9.5], [7.5, 0.5]]), 16)
    assert rounded.tolist() == [[12, 14], [0, 2], [0, -8]]
    assert shift.tolist() == [[-1.0, 0.0], [-1.0, 0.0], [0.0, -1.0]]


@pytest.mark.parametrize("name", CASES)
def test_clean_up_reproduces_the_reference_final_values(name):
    """Fed the reference's own averaged cells, the clean-up gives the reference's ArrayPSF.values to 1e-12 relative: both sides
    make the same SciPy calls in float64, only the order of a few reductions may differ.  A cell without stars is all NaN in the
    reference (0 / 0 at the unit-sum step), and here."""
    g = bc.load(name)
    for method, _ in bc.METHODS:
        cells, want = g[f"cells_{method}"], g[f"values_{method}"]
        before = cells.copy()
        got = np.stack([bld.clean_cell(c) for c in cells])
        assert np.array_equal(cells, before)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        for a, b, count in zip(got, want, g["counts"]):
            if count == 0:
                assert np.isnan(b).all()
                continue
            assert np.isfinite(b).all() and np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
            assert abs(a.sum() - 1.0) < 1e-12


# ------------------------------------------------------------------------------------------------ kernel phases on the emulator
@pytest.mark.parametrize("name", CASES)
def test_emulated_patch_kernel_against_the_reference_patches(name):
    g = bc.load(name)
    n, kw = g["n"], bc.thresholds(name)
    next_patch, worst = 0, 0.0
    for frame, rounded, shift, accepted in zip(g["frames"], _per_frame(g, "rounded"), _per_frame(g, "shift"), _per_frame(g, "accepted")):
        patches, flags = bc.emu_patches(frame, n, rounded, shift, kw.get("saturation_threshold", np.inf), kw.get("star_minimum", 0.0),
                                        kw.get("star_maximum", np.inf))
        assert np.array_equal(flags, accepted)
        for j in np.flatnonzero(flags == 1):
            ref = g["patches"][next_patch]
            next_patch += 1
            assert np.isfinite(patches[j]).all()
            err = np.abs(patches[j] - ref).max() / np.abs(ref).max()
            worst = max(worst, err)
            assert err <= TOL
    assert next_patch == len(g["patches"])
    print(f"{name}: max per-patch error {worst:.3e}")
    if name == "n16":
        assert (g["accepted"] == 0).any()  # the NaN pixel rejected somebody
    else:
        assert 0 < g["accepted"].sum() < len(g["accepted"])  # the thresholds rejected somebody


def test_emulated_patch_kernel_flags():
    # no border pixel below the centre: no plane
    _, rounded, shift = bld.star_geometry(np.array([[20.3, 17.6]]), 16)
    _, flags = bc.emu_patches(bc.bowl_frame((40, 36), (20.3, 17.6)), 16, rounded, shift)
    assert flags.tolist() == [bld.DEGENERATE_RING]
    # a frame of zeros: every pixel of the shifted patch is an exact zero -> rejected, not an error
    _, flags = bc.emu_patches(np.zeros((40, 36), np.float32), 16, rounded, shift)
    assert flags.tolist() == [bld.REJECTED]
    # odd and extreme sizes run (4 and 128 are the limits of the C ABI)
    rng = np.random.default_rng(4)
    for n, shape in ((4, (9, 7)), (5, (11, 8)), (128, (140, 131))):
        frame = rng.random(shape).astype(np.float32) + 1
        centre = np.array([[shape[0] / 2 + 0.2, shape[1] / 2 - 0.3]])
        frame[tuple(np.rint(centre[0]).astype(int))] = 50
        _, rounded, shift = bld.star_geometry(centre, n)
        patches, flags = bc.emu_patches(frame, n, rounded, shift)
        assert flags.tolist() == [bld.ACCEPTED] and np.isfinite(patches).all()
        want, want_flags = bc.oracle_patches(frame, n, rounded, shift)  # ... and give what float64 SciPy gives
        assert want_flags.tolist() == [bld.ACCEPTED]
        assert np.abs(patches - want).max() <= TOL * np.abs(want).max()


def test_emulated_average_kernel_against_numpy():
    case = bc.average_case()
    got = {"mean": bc.emu_average(case["stack"], 0, 50.0, case["offsets"], case["members"]),
           "median": bc.emu_average(case["stack"], 1, 50.0, case["offsets"], case["members"])}
    for q in bc.AVERAGE_PERCENTILES:
        got[q] = bc.emu_average(case["stack"], 2, q, case["offsets"], case["members"])
    bc.check_average(got)
    assert all(np.all(v[-1] == 0) for v in got.values())  # the empty cell


@pytest.mark.parametrize("name", CASES)
def test_emulated_kernels_end_to_end_against_the_reference_cells(name):
    g = bc.load(name)
    stack = g["patches"].astype(np.float32)  # what B1 stores, to within its own bound (checked above)
    for index, (method, q) in enumerate(bc.METHODS):
        cells = bc.emu_average(stack, index, q, g["offsets"], g["members"])
        for got, want in zip(cells, g[f"cells_{method}"]):
            assert np.abs(got - want).max() <= TOL * np.abs(want).max()


# ------------------------------------------------------------------------------------------------ every patch-size path (float64 SciPy oracle)
# The cases and criteria of tests/test_gpu_builder_sizes.py, shared through tests/builder_cases.py.  The emulator runs the threads one
# after another and clears its LDS between stars, so this side checks the arithmetic and the index algebra of each size path; barriers,
# the LDS carve and the launch itself are the GPU side's.
SIZES = list(bc.SIZE_CASES)


def _emulated_stack(name):
    """Kernel B1 on the emulator over every frame of a size case: (the accepted float32 patches in star order, all flags)."""
    case = bc.size_case(name)
    kept, flags = [], []
    for frame, rounded, shift in zip(case["frames"], case["rounded"], case["shift"]):
        patches, accepted = bc.emu_patches(frame, case["n"], rounded, shift, *case["thresholds"])
        kept.append(patches[accepted == 1])
        flags.append(accepted)
    return np.concatenate(kept), np.concatenate(flags)


@pytest.mark.parametrize("name", SIZES)
def test_size_cases_are_well_posed(name):
    case = bc.size_case(name)
    bc.well_posed(case)
    assert all(8 <= len(pos) <= 12 for pos in case["stars"])
    # the star whose corner is k + 0.5 on both axes
    assert all(np.array_equal(np.abs(corner[-1] - np.rint(corner[-1])), [0.5, 0.5]) for corner in case["corner"])
    if case["n"] == 4:  # a corner that is an exact integer (shift -0.5) makes a ring pixel equal the centre there: none in this case
        assert not np.any(np.concatenate(case["shift"]) == -0.5)


@pytest.mark.parametrize("name", SIZES)
def test_emulated_patch_kernel_per_size_against_scipy(name):
    bc.check_size_patches(name, *_emulated_stack(name))


def _emulated_average(case):
    return lambda method, q: bc.emu_average(case["stack"], bld.AVERAGE_METHODS[method], q, case["offsets"], case["members"])


def test_emulated_average_kernel_with_ties_and_percentile_ends():
    bc.check_b2(bc.tie_case(), _emulated_average(bc.tie_case()))


@pytest.mark.parametrize("n", bc.B2_SIZES)
def test_emulated_average_kernel_per_size(n):
    bc.check_b2(bc.b2_size_case(n), _emulated_average(bc.b2_size_case(n)))


@pytest.mark.parametrize("name", bc.END_TO_END)
def test_emulated_kernels_frames_to_cells_per_size(name):
    stack, flags = _emulated_stack(name)
    assert np.array_equal(flags, np.concatenate(bc.size_case(name)["flags"]))
    bc.check_end_to_end(name, lambda method, q, offsets, members: bc.emu_average(stack, bld.AVERAGE_METHODS[method], q, offsets, members))


def test_emulated_patch_kernel_on_the_growth_frames_and_beyond_float32():
    """The two remaining inputs of the GPU tests' storage section, arithmetic only."""
    case = bc.growth_case()
    bc.well_posed(case)
    for frame, rounded, shift, want, want_flags in zip(case["frames"], case["rounded"], case["shift"], case["patches"], case["flags"]):
        patches, flags = bc.emu_patches(frame, case["n"], rounded, shift)
        assert np.array_equal(flags, want_flags) and want_flags.all()
        assert np.all(np.abs(patches - want).max(axis=(1, 2)) <= TOL * np.abs(want).max(axis=(1, 2)))
    bright = bc.near_float32_max_case()
    kept = bright["patches"][0][0]  # float64 keeps the patch: finite, but its maximum does not fit float32 ...
    assert np.isfinite(kept).all() and kept.max() > 1.1 * float(np.finfo(np.float32).max) and bright["flags"][0].tolist() == [bld.ACCEPTED]
    _, flags = bc.emu_patches(bright["frames"][0], 16, bright["rounded"][0], bright["shift"][0])
    assert flags.tolist() == [bld.REJECTED]  # ... so the kernel, whose stack is float32 and finite, does not
