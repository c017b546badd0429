"""The PSF builder on the GPU at every patch-size path, against float64 NumPy / SciPy (the oracle, cases and criteria of
tests/builder_cases.py, which the emulator tests of tests/test_builder_host.py share).

The fixtures of tests/test_gpu_builder.py stop at N = 32: one pixel to four per thread of the 256-thread kernel.  Here:
1. kernel B1 per size path - N = 4, 5, 16, 33, 63, 64 (256 threads, up to 16 pixels per thread), 65, 127, 128 (1024 threads, the
   141 KiB LDS carve), and frames smaller than the patch: flags equal the oracle's, per accepted patch max|d| <= 1e-5 max|ref patch|;
2. workgroup isolation, which only the hardware can show: the patches of one launch over all stars, of one launch per star, of the
   stars in reversed order, and of two handles of different kernels used in turn are the same bits;
3. kernel B2 alone: heavy ties of both signs with every percentile end, and N = 4, 5, 33, 128 (partial last block, 64 blocks);
4. frames -> cells at N = 33, 64, 128;
5. device storage (stack and buffer growth on later frames), builds with few or no stars, duplicate stars, frame dtypes and
   layouts, values near the float32 maximum;
6. every refusal of rpsf_builder_* on a live handle (each returns before any HIP call; nothing here launches with bad arguments).
"""

import ctypes

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native
from regularizepsf_amd import builder as bld
from tests import builder_cases as bc

pytestmark = pytest.mark.gpu
SIZES = list(bc.SIZE_CASES)
ISOLATION = ("n16", "n64", "n128")


def _bits(a):
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _fill(case, capacity=64, frames=None):
    """The device stack of a case: its frames (or the given ones in their place) through kernel B1, flags of every star."""
    stack = bld._Stack(case["n"], 0, capacity)
    flags = [stack.add_frame(frame, rounded, shift, *case["thresholds"])
             for frame, rounded, shift in zip(case["frames"] if frames is None else frames, case["rounded"], case["shift"])]
    return stack, np.concatenate(flags)


# ------------------------------------------------------------------------------------------------ 1. B1 per size path
@pytest.mark.parametrize("name", SIZES)
def test_patches_per_size_against_scipy(name):
    case = bc.size_case(name)
    bc.well_posed(case)
    stack, flags = _fill(case)
    assert len(stack) == int(flags.sum())
    bc.check_size_patches(name, stack.patches(), flags)
    stack.close()


# ------------------------------------------------------------------------------------------------ 2. workgroup isolation
def _one_launch(case):
    stack, flags = _fill(case, frames=case["frames"][:1])
    patches = stack.patches()
    stack.close()
    assert 1 < len(patches)
    return patches, flags


@pytest.mark.parametrize("name", ISOLATION)
def test_one_launch_per_star_and_reversed_stars_give_the_same_bits(name):
    case = bc.size_case(name)
    frame, rounded, shift = case["frames"][0], case["rounded"][0], case["shift"][0]
    patches, flags = _one_launch(case)
    # every star in a launch of its own: no workgroup before it, none beside it
    alone = bld._Stack(case["n"], 0, 64)
    alone_flags = np.concatenate([alone.add_frame(frame, rounded[j:j + 1], shift[j:j + 1], *case["thresholds"]) for j in range(len(rounded))])
    assert np.array_equal(alone_flags, flags) and _same_bits(alone.patches(), patches)
    alone.close()
    # the stars in reversed order: other neighbours, other predecessors on the same compute unit
    back = bld._Stack(case["n"], 0, 64)
    back_flags = back.add_frame(frame, rounded[::-1], shift[::-1], *case["thresholds"])
    assert np.array_equal(back_flags[::-1], flags) and _same_bits(back.patches()[::-1], patches)
    back.close()


def test_two_handles_used_in_turn_equal_their_solo_results():
    big, small = bc.size_case("n128"), bc.size_case("n16")
    want_big, flags_big = _one_launch(big)
    want_small, flags_small = _one_launch(small)
    a, b = bld._Stack(128, 0, 4), bld._Stack(16, 0, 4)
    got_big, got_small = [], []
    for j in range(0, len(flags_big), 2):  # two stars of the 1024-thread kernel, then one and one of the 256-thread kernel
        got_big.append(a.add_frame(big["frames"][0], big["rounded"][0][j:j + 2], big["shift"][0][j:j + 2], *big["thresholds"]))
        for i in (j, j + 1):
            got_small.append(b.add_frame(small["frames"][0], small["rounded"][0][i:i + 1], small["shift"][0][i:i + 1], *small["thresholds"]))
    assert len(flags_big) == len(flags_small) == 10
    assert np.array_equal(np.concatenate(got_big), flags_big) and np.array_equal(np.concatenate(got_small), flags_small)
    assert _same_bits(a.patches(), want_big) and _same_bits(b.patches(), want_small)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 3. B2 alone
def _loaded(case, capacity):
    stack = bld._Stack(case["stack"].shape[-1], 0, capacity)
    stack.load(case["stack"])
    assert len(stack) == len(case["stack"])
    return stack, lambda method, q: stack.average(method, q, case["offsets"], case["members"])


def test_averaging_with_ties_and_percentile_ends_against_numpy():
    case = bc.tie_case()
    stack, average = _loaded(case, len(case["stack"]))
    bc.check_b2(case, average)
    stack.close()


@pytest.mark.parametrize("n", bc.B2_SIZES)
def test_averaging_per_size_against_numpy_and_twice_the_same(n):
    case = bc.b2_size_case(n)
    stack, average = _loaded(case, 12)
    first = bc.check_b2(case, average)
    again = bc.check_b2(case, average)
    for key in first:
        assert _same_bits(first[key], again[key])
    stack.close()


# ------------------------------------------------------------------------------------------------ 4. frames -> cells
@pytest.mark.parametrize("name", bc.END_TO_END)
def test_frames_to_cells_per_size_against_the_oracle(name):
    case = bc.size_case(name)
    stack, flags = _fill(case)
    assert np.array_equal(flags, np.concatenate(case["flags"]))
    bc.check_end_to_end(name, stack.average)
    stack.close()


# ------------------------------------------------------------------------------------------------ 5. device storage and build paths
def test_the_stack_grows_through_add_frame_while_it_holds_patches():
    case = bc.growth_case()
    tight, tight_flags = _fill(case, capacity=1)  # 3, then 9, then 20 stars: doubles from 1 to 32 with patches in it
    ample, ample_flags = _fill(case, capacity=64)
    assert len(tight) == len(ample) == int(ample_flags.sum()) > 16
    assert np.array_equal(tight_flags, ample_flags) and _same_bits(tight.patches(), ample.patches())
    tight.close()
    ample.close()


def test_buffers_grow_on_later_frames_with_more_stars():
    case = bc.growth_case()
    bc.well_posed(case)
    assert tuple(len(pos) for pos in case["stars"]) == bc.GROWTH_STARS
    stack, flags = _fill(case)
    got = stack.patches()
    stack.close()
    want_flags = np.concatenate(case["flags"])
    want = np.concatenate(case["patches"])[want_flags == 1]
    assert np.array_equal(flags, want_flags) and got.shape == want.shape
    err = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
    print(f"frames of {bc.GROWTH_STARS} stars: max per-patch error {err.max():.3e}")
    assert np.all(err <= bc.TOL)
    separate = []
    for frame, rounded, shift in zip(case["frames"], case["rounded"], case["shift"]):  # every frame in a handle of its own: nothing grows
        one = bld._Stack(case["n"], 0, len(rounded))
        one.add_frame(frame, rounded, shift, *case["thresholds"])
        separate.append(one.patches())
        one.close()
    assert _same_bits(np.concatenate(separate), got)


def _model_bits(result):
    psf, counts = result[:2]
    return _bits(psf.values), [tuple(c) for c in psf.coordinates], counts


def test_builds_with_few_or_no_stars():
    case = bc.growth_case()
    n, frames, stars = case["n"], case["frames"], case["stars"]
    builder = rp.ArrayPSFBuilder(n)
    none = np.zeros((0, 2))
    # a middle frame without a star adds nothing: the model of the two other frames
    values, coordinates, counts = _model_bits(builder.build(frames, stars=[stars[0], none, stars[2]], average_method="mean"))
    want_values, want_coordinates, want_counts = _model_bits(builder.build(frames[[0, 2]], stars=[stars[0], stars[2]], average_method="mean"))
    assert sum(counts.values()) > 0 and counts == want_counts and coordinates == want_coordinates and np.array_equal(values, want_values)
    # every star rejected by star_maximum (every centre of the oracle is far above 1), and no star at all
    assert min(patches[:, n // 2, n // 2].min() for patches in case["patches"]) > 2.0
    for kwargs in ({"stars": stars, "star_maximum": 1.0}, {"stars": [none] * 3}):
        for method in ("mean", "median", "percentile"):
            psf, counts, patches = builder.build(frames, average_method=method, percentile=30, return_patches=True, **kwargs)
            assert patches == {}
            assert [tuple(c) for c in psf.coordinates] == [tuple(c) for c in rp.calculate_covering(frames[0].shape, n)]
            assert list(counts.values()) == [0] * len(psf.coordinates)
            assert psf.values.shape == (len(counts), n, n) and np.isnan(psf.values).all()


def test_a_star_listed_twice_counts_once():
    case = bc.growth_case()
    n, frames, stars = case["n"], case["frames"], case["stars"]
    # the copies come after the first listing: which patch is kept, and the order of the stack, stay as they are
    twice = [np.concatenate([stars[0], stars[0][1:2]]), stars[1], np.concatenate([stars[2], stars[2][4:5], stars[2][4:5]])]
    builder = rp.ArrayPSFBuilder(n)
    for method in ("mean", "median"):
        values, coordinates, counts = _model_bits(builder.build(frames, stars=twice, average_method=method))
        want_values, want_coordinates, want_counts = _model_bits(builder.build(frames, stars=stars, average_method=method))
        assert counts == want_counts and coordinates == want_coordinates and np.array_equal(values, want_values)


def test_frame_dtypes_and_layouts_give_the_same_bits():
    case = bc.size_case("n33")
    whole = np.rint(case["frames"][0]).astype(np.uint16)  # the same values in every dtype below
    assert whole.max() > 300 and np.array_equal(whole, whole.astype(np.float32))
    wide = whole.astype(np.float64)
    room = np.zeros((2 * whole.shape[0] + 1, 2 * whole.shape[1] + 3))
    room[1::2, 3::2] = wide
    variants = {"uint16": whole, "int64": whole.astype(np.int64), "float32": whole.astype(np.float32), "Fortran float64": np.asfortranarray(wide),
                "Fortran float32": np.asfortranarray(whole.astype(np.float32)), "sliced": room[1::2, 3::2]}
    assert not variants["sliced"].flags.c_contiguous and not variants["Fortran float64"].flags.c_contiguous
    want_stack, want_flags = _fill(case, frames=[wide])
    want = want_stack.patches()
    assert want_flags.sum() > 1
    for label, frame in variants.items():
        assert np.array_equal(frame, wide), label
        stack, flags = _fill(case, frames=[frame])
        assert np.array_equal(flags, want_flags) and _same_bits(stack.patches(), want), label
        stack.close()
    want_stack.close()


def test_a_value_beyond_float32_rejects_the_star_and_leaves_the_stack_finite():
    bright, ordinary = bc.near_float32_max_case(), bc.size_case("n16")
    kept = bright["patches"][0][0]  # float64 keeps it: finite, above the float32 maximum by far more than any rounding
    assert np.isfinite(kept).all() and kept.max() > 1.1 * float(np.finfo(np.float32).max) and bright["flags"][0].tolist() == [1]
    frame = bright["frames"][0].astype(np.float32)
    assert np.isfinite(frame).all() and frame.max() > 3e38
    want, want_flags = _one_launch(ordinary)
    stack = bld._Stack(16, 0, 4)
    assert stack.add_frame(frame, bright["rounded"][0], bright["shift"][0], np.inf, 0.0, np.inf).tolist() == [bld.REJECTED]
    assert len(stack) == 0
    flags = stack.add_frame(ordinary["frames"][0], ordinary["rounded"][0], ordinary["shift"][0], *ordinary["thresholds"])
    got = stack.patches()
    assert np.array_equal(flags, want_flags) and np.isfinite(got).all() and _same_bits(got, want)
    stack.close()


# ------------------------------------------------------------------------------------------------ 6. refusals on a live handle
def _refused(code):
    return code == _native.E_BADARG and len(_native.lib().rpsf_last_error()) > 0


def test_add_frame_and_patches_refuse_bad_arguments_on_a_live_handle():
    lib, ptr = _native.lib(), _native._ptr
    case = bc.size_case("n16")
    n, frame = 16, np.ascontiguousarray(case["frames"][0], np.float32)
    h, w = frame.shape
    corners, frac = np.ascontiguousarray(case["rounded"][0], np.int32), np.ascontiguousarray(case["shift"][0], np.float64)
    want, want_flags = _one_launch(case)
    stack = bld._Stack(n, 0, 4)
    stack.add_frame(frame, corners[:3], frac[:3], np.inf, 0.0, np.inf)
    count = len(stack)
    assert count == 3
    flags = np.full(len(corners), 77, np.uint8)

    def add(height=h, width=w, stars=len(corners), where=corners, amount=frac):
        return lib.rpsf_builder_add_frame(stack._handle, ptr(frame), 0, height, width, stars, ptr(where), ptr(amount), np.inf, 0.0, np.inf, ptr(flags))

    def moved(array, index, value):
        out = array.copy()
        out[index] = value
        return out

    assert _refused(add(height=1)) and _refused(add(width=1))
    assert _refused(add(stars=-1))
    for index, value in (((2, 0), 2 * h + 1), ((2, 1), 2 * w + 1), ((9, 0), -n - h - 1), ((0, 1), -n - w - 1)):
        assert _refused(add(where=moved(corners, index, value)))
    for value in (2.5, -2.5, np.nan):
        assert _refused(add(amount=moved(frac, (4, 1), value)))
    assert len(stack) == count and np.all(flags == 77)  # nothing was added, nothing was written
    # the limits themselves are taken (the mirror map brings any such corner back into the frame), and a good frame still works
    assert add(where=moved(moved(corners, (2, 0), 2 * h), (0, 1), -n - w), amount=moved(frac, (4, 1), 2.0)) == 0
    assert len(stack) > count and np.isfinite(stack.patches()).all()
    stack.close()
    stack = bld._Stack(n, 0, 4)
    assert _refused(lib.rpsf_builder_add_frame(stack._handle, ptr(frame), 0, 1, w, len(corners), ptr(corners), ptr(frac), np.inf, 0.0, np.inf, ptr(flags)))
    assert np.array_equal(stack.add_frame(frame, corners, frac, *case["thresholds"]), want_flags) and _same_bits(stack.patches(), want)
    # rpsf_builder_patches: a range outside the stack
    count = len(stack)
    out = np.zeros((count + 1, n, n), np.float32)
    for first, many in ((count + 1, 0), (0, count + 1), (count, 1), (1, np.iinfo(np.uint64).max)):
        assert _refused(lib.rpsf_builder_patches(stack._handle, ctypes.c_size_t(first), ctypes.c_size_t(many), ptr(out)))
    assert not out.any()
    assert lib.rpsf_builder_patches(stack._handle, count, 0, ptr(out)) == 0  # the empty range at the end is a range
    stack.close()


def test_average_refuses_bad_arguments_on_a_live_handle():
    lib, ptr = _native.lib(), _native._ptr
    case = bc.b2_size_case(5)
    stack, average = _loaded(case, 12)
    offsets, members = np.ascontiguousarray(case["offsets"], np.int64), np.ascontiguousarray(case["members"], np.int32)
    cells = np.full((len(offsets) - 1, 5, 5), 7.0)

    def run(method=2, q=30.0, n_cells=len(offsets) - 1, where=offsets, who=members):
        return lib.rpsf_builder_average(stack._handle, method, q, n_cells, ptr(where), ptr(who), ptr(cells))

    for method in (3, -1, 7):
        assert _refused(run(method=method))
    for q in (-1.0, 100.5, np.nan):
        assert _refused(run(q=q))
    assert _refused(run(n_cells=0)) and _refused(run(n_cells=-2))
    first_is_one = offsets.copy()
    first_is_one[0] = 1
    assert _refused(run(where=first_is_one))
    decreasing = offsets.copy()
    decreasing[2] = decreasing[1] - 1
    assert _refused(run(where=decreasing))
    negative = members.copy()
    negative[3] = -1
    assert _refused(run(who=negative))
    assert np.all(cells == 7.0)  # nothing was written
    assert run() == 0 and _same_bits(cells, average("percentile", 30.0))  # and the good call still works
    stack.close()
