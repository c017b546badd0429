"""ArrayPSFBuilder on the GPU against the reference builder (fixtures of tests/golden/make_builder_golden.py: the real
reference downstream of a given star list, frames rounded to float32 before it saw them).

1. patches: accept flags exact; per accepted patch max|d| <= 1e-5 max|ref patch| (SURVEY.md 8d's bound, per patch: a faint
   star with a bright neighbour must not hide behind the frame's maximum).  The arithmetic is float64, so what is left is the
   float32 rounding of the stored patch, about 6e-8.
2. averaging alone, on a loaded stack with 1 ... 2500 members per cell: mean and median bit-identical to NumPy, percentiles to
   1e-12; twice the same call, the same bits.
3. frames -> patches -> averaged cells against the reference's averaged cells, per cell 1e-5 of the cell's maximum.
4. the final model against the reference's ArrayPSF.values, per cell 1e-5, counts equal.  The clean-up cuts at 0.005 x centre;
   a pixel within 1e-5 x centre of the cut may legitimately fall on the other side, which changes the labelled component and
   the normalisation of the whole cell - such cells (flagged by the generator from the reference's own data, at most 10 %) are
   left out here and stay covered by 3.
5. behaviour: errors, return_patches, the model feeds construct / apply.
"""

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import builder as bld
from tests import builder_cases as bc

pytestmark = pytest.mark.gpu
CASES = list(bc.CASES)
TOL = 1e-5


def _per_frame(g, key):
    return np.split(g[key], np.cumsum(g["stars_per_frame"])[:-1])


def _fill(g, name):
    """The device stack of a case: frames through kernel B1, flags per frame."""
    kw = bc.thresholds(name)
    stack = bld._Stack(g["n"], 0, len(g["accepted"]))
    flags = [stack.add_frame(frame, rounded, shift, kw.get("saturation_threshold", np.inf), kw.get("star_minimum", 0.0),
                             kw.get("star_maximum", np.inf))
             for frame, rounded, shift in zip(g["frames"], _per_frame(g, "rounded"), _per_frame(g, "shift"))]
    return stack, np.concatenate(flags)


@pytest.mark.parametrize("name", CASES)
def test_patches_against_the_reference(name):
    g = bc.load(name)
    stack, flags = _fill(g, name)
    assert np.array_equal(flags, g["accepted"])
    got = stack.patches()
    assert got.dtype == np.float32 and got.shape == g["patches"].shape and np.isfinite(got).all()
    err = np.abs(got - g["patches"]).max(axis=(1, 2)) / np.abs(g["patches"]).max(axis=(1, 2))
    print(f"{name}: {len(got)} patches, max per-patch error {err.max():.3e}")
    assert np.all(err <= TOL)
    stack.close()


def test_float32_and_float64_frames_give_the_same_patches():
    g = bc.load("n15")
    a, _ = _fill(g, "n15")
    narrow = dict(g, frames=g["frames"].astype(np.float32))
    b, _ = _fill(narrow, "n15")
    assert np.array_equal(a.patches().view(np.int32), b.patches().view(np.int32))


def _average_all(stack, offsets, members):
    got = {"mean": stack.average("mean", 50.0, offsets, members), "median": stack.average("median", 50.0, offsets, members)}
    for q in bc.AVERAGE_PERCENTILES:
        got[q] = stack.average("percentile", q, offsets, members)
    return got


def test_averaging_alone_against_numpy_and_twice_the_same():
    case = bc.average_case()
    stack = bld._Stack(16, 0, 8)  # smaller than the load: the stack grows
    stack.load(case["stack"])
    assert len(stack) == len(case["stack"]) and np.array_equal(stack.patches(2490, 10), case["stack"][2490:])
    first = _average_all(stack, case["offsets"], case["members"])
    bc.check_average(first)
    assert all(np.all(v[-1] == 0) for v in first.values())  # the empty cell
    again = _average_all(stack, case["offsets"], case["members"])
    for key in first:
        assert np.array_equal(first[key].view(np.int64), again[key].view(np.int64))
    stack.close()


def test_load_patches_refuses_what_the_averaging_cannot_take():
    from regularizepsf_amd import _native

    stack = bld._Stack(16, 0, 4)
    good = np.ones((2, 16, 16), np.float32)
    for value, where in ((np.nan, (1, 3, 4)), (np.inf, (0, 0, 0)), (0.0, (1, 8, 8))):
        bad = good.copy()
        bad[where] = value
        with pytest.raises(_native.NativeError) as info:
            stack.load(bad)
        assert info.value.code == _native.E_BADARG
    assert len(stack) == 0
    stack.load(good)
    with pytest.raises(_native.NativeError) as info:  # a member that is not in the stack
        stack.average("mean", 50.0, np.array([0, 1]), np.array([2]))
    assert info.value.code == _native.E_BADARG
    stack.close()


@pytest.mark.parametrize("name", CASES)
def test_averaged_cells_end_to_end_against_the_reference(name):
    g = bc.load(name)
    stack, _ = _fill(g, name)
    for method, q in bc.METHODS:
        cells = stack.average(method, q, g["offsets"], g["members"])
        want = g[f"cells_{method}"]
        err = np.abs(cells - want).max(axis=(1, 2))
        scale = np.abs(want).max(axis=(1, 2))
        print(f"{name} {method}: max per-cell error {np.max(err[scale > 0] / scale[scale > 0]):.3e}")
        assert np.all(err <= TOL * scale)  # a cell without a star is all zeros on both sides
    stack.close()


@pytest.mark.parametrize("name", CASES)
def test_final_model_against_the_reference(name):
    g = bc.load(name)
    for method, q in bc.METHODS:
        psf, counts = rp.ArrayPSFBuilder(g["n"]).build(g["frames"], average_method=method, percentile=q, stars=g["stars"],
                                                       **bc.thresholds(name))
        assert isinstance(psf, rp.ArrayPSF)
        assert [tuple(c) for c in psf.coordinates] == [tuple(c) for c in g["corners"]]
        assert list(counts) == [tuple(c) for c in g["corners"]] and list(counts.values()) == g["counts"].tolist()
        want, excluded = g[f"values_{method}"], g[f"excluded_{method}"]
        assert excluded.mean() <= 0.10
        got = psf.values
        assert got.dtype == np.float64 and got.shape == want.shape
        compared = 0
        for a, b, skip in zip(got, want, excluded):
            if skip:
                continue
            assert np.array_equal(np.isnan(a), np.isnan(b))
            if np.isnan(b).all():  # no star in the cell: 0 / 0 at the unit-sum step, in the reference too
                continue
            assert np.abs(a - b).max() <= TOL * np.abs(b).max()
            compared += 1
        assert compared == ((g["counts"] > 0) & ~excluded).sum() > 0  # every cell with a star that is not near the cut


def test_behaviour():
    g = bc.load("n15")
    n = g["n"]
    builder = rp.ArrayPSFBuilder(n)
    # frames of different shapes
    with pytest.raises(rp.PSFBuilderError, match="same shape"):
        builder.build([g["frames"][0], g["frames"][1][:, :-1]], stars=g["stars"])
    # a 'star' that is the minimum of its patch: no border pixel below the centre, no background plane
    with pytest.raises(rp.PSFBuilderError, match="fewer than three border pixels"):
        builder.build(bc.bowl_frame((50, 44), (20.3, 17.6)), stars=[np.array([[20.3, 17.6]])])
    # return_patches: keys (frame, row - N / 2, col - N / 2) as Python numbers, float64 N x N copies of the device's float32 patches
    psf, counts, patches = builder.build(g["frames"], stars=g["stars"], return_patches=True, **bc.thresholds("n15"))
    assert [tuple(k) for k in g["patch_keys"]] == list(patches)
    for key, value in patches.items():
        assert type(key[0]) is int and type(key[1]) is float and type(key[2]) is float
        assert value.dtype == np.float64 and value.shape == (n, n)
        assert np.array_equal(value, value.astype(np.float32).astype(np.float64))
    assert sum(counts.values()) == len(g["members"])
    # a single 2-D frame is one frame, a list of frames works like a stack, num_workers is ignored
    one, _ = builder.build(g["frames"][0], stars=g["stars"][:1], num_workers=3, **bc.thresholds("n15"))
    two, _ = builder.build([g["frames"][0]], stars=g["stars"][:1], **bc.thresholds("n15"))
    assert np.array_equal(one.values.view(np.int64), two.values.view(np.int64))
    # two builds of one input agree bit for bit
    again, _ = builder.build(g["frames"], stars=g["stars"], **bc.thresholds("n15"))
    assert np.array_equal(psf.values.view(np.int64), again.values.view(np.int64))


def test_the_model_feeds_construct_and_apply():
    g = bc.load("n16")
    psf, counts = rp.ArrayPSFBuilder(16).build(g["frames"], stars=g["stars"], average_method="mean")
    empty = np.array(list(counts.values())) == 0  # cells without a star are 0 / 0 in the reference and here: give them the mean model
    assert empty.any() and np.isnan(psf.values[empty]).all() and np.isfinite(psf.values[~empty]).all()
    values = psf.values.copy()
    values[empty] = values[~empty].mean(axis=0)
    source = rp.ArrayPSF(rp.IndexedCube(psf.coordinates, values))
    transform = rp.ArrayPSFTransform.construct(source, source, 3.0, 0.1)
    out = transform.apply(np.nan_to_num(g["frames"][0]))
    assert out.shape == g["frames"][0].shape and np.isfinite(out).all()
