"""Parity per patch neighbourhood, exact homogeneity, and isolation between the applies of one plan.

The other GPU modules bound the error by 1e-5 of the brightest pixel of the frame.  The reference treats every patch on its own, so a
correct float32 implementation errs at a pixel by ~2e-7 of what the (at most four) patches over that pixel carry, however bright the
rest of the frame is.  Here (tests/helpers.py):

    local scale(pixel) = sum over the patches covering it of max|patch result after the second window|     (float64 oracle)
    local error(out)   = max |out - oracle| / local scale
    yardstick          = local error of the oracle's own steps carried out in float32 (scipy.fft on complex64), same inputs
    bound              = local error(kernel) <= MARGIN x yardstick,  MARGIN = 4

on frames whose amplitude steps through six decades in blocks of 2 N pixels (hdr_frame); a case counts only if at least 10 % of its
pixels have a local scale <= 1e-3 of the frame's largest (asserted from the float64 oracle alone, LocalCase).  The global 1e-5 bar is
asserted beside it, unchanged.

Two properties that need no tolerance ride on the same plans:
  * homogeneity: apply(2^10 f) == 2^10 apply(f) and the same for 2^-10, bit for bit, on ONE plan in the sequence f, 1024 f, f / 1024, f
    (true of anything made of multiplies, adds and FMAs in a fixed order; false of anything additive that does not come from the frame);
  * isolation: whatever a plan was applied to before - a frame 10^6 times brighter, another shape, a frame with NaN and Inf - every result
    is bit-identical to what a freshly created plan gives for that frame alone.

Measured on an MI355X (kernel / yardstick, min ... max over the cases and pad modes of this module; log: profiles/local_parity_gpu.log;
the whole module takes 13 s there, most of it the float64 oracle on the host).  The rows of N = 128 / 256 are named after the launch that
the geometry selects (launch() of tests/local_parity_cases.py; the forms are bit-identical, so no figure can show which one ran):

    path                                                   N = 16        32            64            128           256
    sweep kernel, region targets 1 and 1000                0.66 ... 1.38 1.16          1.02 ... 1.25
    same corner lists forced to colour planes              0.68 ... 1.21 0.92 ... 1.52 0.97 ... 1.22
    same corner lists forced to float atomics              0.65 ... 1.21 0.92 ... 1.52 0.97 ... 1.15
    persistent + fused (width % 32 == 0; constant, symmetric, wrap)                                  1.22          1.09 ... 1.24
    fused, one patch per workgroup (reflect, edge; persist = 0)                                      1.22          1.09 ... 1.24
    separate plane sum (odd width with rim patches; fuse = 0)                                        0.85 ... 1.22 0.86 ... 1.24
    direct overlap-add                                                                               0.85 ... 1.22 0.88 ... 1.24
    apply_batch_device, streamed apply_batch, 3 row bands, class API
      float32 / float64 in (= single apply, bitwise): persistent + fused 1.16 (sweep)                1.36          1.12
      the same routes, separate plane sum (520 x 650, reflect)                                       1.21
    isolation sequence and mixed batches, dim frame: persistent + fused  1.16          1.02 (sweep)  1.36          1.12
      the same, separate plane sum (520 x 770)                                                                     1.13
    hipFFT fallback, N = 24, on a covering                 0.95 ... 1.10
    BASELINE config 1 star field (512 x 512 / 32)                        1.10

Yardstick 1.6e-7 ... 2.8e-7, global max|d| / max|ref| 1.5e-7 ... 3.6e-7.  No path comes near MARGIN = 4, so float atomics and hipFFT keep
the common margin.  Homogeneity and isolation hold bit for bit on every path.
"""

import functools

import numpy as np
import pytest

import regularizepsf_amd as rp
from oracle import regpsf_oracle as orc
from tests.helpers import KERNEL_PAD_MODES, MARGIN, LocalCase, hdr_frame, local_error, per_patch_reference, random_transfer, rel_errors
from tests.local_parity_cases import ISOLATION_CASES, ROUTE_CASES, SECOND_CASES, SWEEP_CASES
from tests.local_parity_cases import launch as _launch

pytestmark = pytest.mark.gpu
TOL = 1e-5  # the global bar of the other modules, kept beside the local one
#: float atomics add a pixel's four contributions in the order the hardware serves them; hipFFT runs its own algorithm at sizes that are
#: no power of two.  Both get the common margin unless a measurement (module docstring) says otherwise.
MARGIN_ATOMIC = MARGIN
MARGIN_HIPFFT = MARGIN
SCALES = (np.float32(1024.0), np.float32(1.0 / 1024.0))

@functools.lru_cache(maxsize=4)
def _case(shape, n, seed, mode):
    return LocalCase(shape, n, seed, mode)


def _pad(mode):
    from regularizepsf_amd import _native

    return _native.PAD_MODES[mode]


def _plan(case, overlap=None, **options):
    from regularizepsf_amd import _native

    plan = _native.Plan(case.n, case.coords)
    plan.set_transfer(case.k)
    if overlap is not None:
        plan.set_overlap_mode(overlap)
    for name, value in options.items():
        plan.set_option(name, value)
    return plan


def _bound(case, out, path, margin=MARGIN):
    """Print the figures, then assert the global bar and the local bound."""
    out = np.asarray(out, np.float64)
    rel_max, rel_l2 = rel_errors(out, case.ref)
    ratio = case.ratio(out)
    print(f"LOCAL-RATIO | {path} | N={case.n} {case.shape[0]}x{case.shape[1]} {case.pad_mode} | dim share {case.share:.2f} | "
          f"yardstick {case.yardstick:.2e} | ratio {ratio:.2f} | global {rel_max:.1e}")
    assert rel_max <= TOL and rel_l2 <= TOL, (path, rel_max, rel_l2)
    case.check(out, margin, path)
    return ratio


def _bound_and_homogeneity(case, apply, path, margin=MARGIN):
    """f, 1024 f, f / 1024, f on whatever ``apply`` closes over: the bound on the first, exact scaling of the next two, the first again."""
    base = apply(case.image)
    _bound(case, base, path, margin)
    for s in SCALES:
        assert np.array_equal(apply(s * case.image), s.astype(base.dtype) * base), (path, case.pad_mode, float(s))
    assert np.array_equal(apply(case.image), base), (path, case.pad_mode, "the frame again")
    return base


@pytest.mark.parametrize(("n", "shape", "seed"), SWEEP_CASES)
def test_sweep_kernel_and_its_forced_overlap_modes(n, shape, seed):
    """N = 16 / 32 / 64: the sweep kernel cut into as few regions as its LDS ring allows (target 1) and into many (target 1000), the same corner list forced to the
    colour planes and to float atomics (bound only: their add order is not fixed), the five pad modes the kernels evaluate."""
    first = _case(shape, n, seed, KERNEL_PAD_MODES[0])
    sweep, planes, atomic = _plan(first), _plan(first, "planes"), _plan(first, "atomic")
    assert sweep.sweep_info()["regions"] > 0
    cuts = []
    for mode in KERNEL_PAD_MODES:
        case = _case(shape, n, seed, mode)
        outs = []
        for target in (1, 1000):
            sweep.set_sweep_regions(target)
            cuts.append(sweep.sweep_info()["regions"])
            outs.append(_bound_and_homogeneity(case, lambda f: sweep.apply(f, _pad(mode)), f"sweep, region target {target}"))
        assert np.array_equal(outs[0], outs[1])
        assert 1 <= cuts[-2] < cuts[-1], cuts  # the fewest regions the LDS ring's width allows (one on the narrow lattices), and many
        _bound_and_homogeneity(case, lambda f: planes.apply(f, _pad(mode)), "planes (N <= 64)")
        _bound(case, atomic.apply(case.image, _pad(mode)), "atomic (N <= 64)", MARGIN_ATOMIC)


@pytest.mark.parametrize(("n", "shape", "seed"), SECOND_CASES)
def test_second_generation_plans_every_launch_form(n, shape, seed):
    """N = 128 / 256, five pad modes: the default plan (persistent + fused, fused, or the separate sum kernel: _launch() says which the
    geometry selects), `persist` 0, `fuse` 0, and direct accumulation; bit-identical to each other where the colour order is the same."""
    modes = KERNEL_PAD_MODES
    first = _case(shape, n, seed, modes[0])
    plans = {"default": _plan(first), "persist=0": _plan(first, persist=0), "fuse=0": _plan(first, fuse=0), "direct": _plan(first, "direct")}
    if shape[1] % 32 == 0:
        assert {_launch(n, shape, m) for m in modes} == {"persistent + fused", "fused, one patch per workgroup"}
    else:
        assert {_launch(n, shape, m) for m in modes} == {"separate plane sum"}
    for mode in modes:
        case = _case(shape, n, seed, mode)
        label = {"default": _launch(n, shape, mode), "persist=0": "persist=0: " + _launch(n, shape, mode, persist=False),
                 "fuse=0": "fuse=0: " + _launch(n, shape, mode, fuse=False), "direct": "direct overlap-add"}
        outs = {name: _bound_and_homogeneity(case, lambda f, plan=plan: plan.apply(f, _pad(mode)), label[name]) for name, plan in plans.items()}
        assert np.array_equal(outs["default"], outs["persist=0"]) and np.array_equal(outs["default"], outs["fuse=0"]), mode


@pytest.mark.parametrize(("n", "shape", "seed"), [(24, (100, 130), 24)])
def test_hipfft_fallback_on_a_covering(n, shape, seed):
    """A patch size without a hand-written plan: gather -> hipFFT -> x K -> hipFFT -> overlap-add colour class by colour class (fixed order
    on a covering, so homogeneity is exact there too)."""
    for mode in KERNEL_PAD_MODES:
        case = _case(shape, n, seed, mode)
        plan = _plan(case)
        _bound_and_homogeneity(case, lambda f: plan.apply(f, _pad(mode)), "hipFFT fallback", MARGIN_HIPFFT)


@pytest.mark.parametrize(("n", "shape", "seed", "mode"), ROUTE_CASES)
def test_batch_streamed_banded_and_class_api_routes(n, shape, seed, mode):
    """The frames f, 1024 f, f / 1024, f as ONE batch on the device and as one streamed host batch; a single host frame cut into three row
    bands; ArrayPSFTransform.apply with a float64 and a float32 frame.  Same bound, same exact scaling, every route the same bits."""
    from regularizepsf_amd import _native

    case = _case(shape, n, seed, mode)
    h, w = shape
    launch = _launch(n, shape, mode)
    stack = np.ascontiguousarray(np.stack([case.image, SCALES[0] * case.image, SCALES[1] * case.image, case.image]))
    single = _plan(case).apply(case.image, _pad(mode))

    def scaled(outs, path):
        _bound(case, outs[0], path)
        assert np.array_equal(outs[0], single.astype(outs.dtype)), path
        assert np.array_equal(outs[1], SCALES[0].astype(outs.dtype) * outs[0]), path
        assert np.array_equal(outs[2], SCALES[1].astype(outs.dtype) * outs[0]), path
        assert np.array_equal(outs[3], outs[0]), path

    plan = _plan(case)
    d_in = _native.DeviceBuffer(stack.nbytes).upload(stack)
    d_out = _native.DeviceBuffer(stack.nbytes)
    try:
        plan.apply_batch_device(d_in.ptr, d_out.ptr, 4, h * w, h * w, _native.Geometry.whole(h, w, _pad(mode)))
        plan.synchronize()
        scaled(d_out.download((4, h, w)), f"apply_batch_device ({launch})")
    finally:
        d_in.free()
        d_out.free()

    t = rp.ArrayPSFTransform(rp.IndexedCube(case.coords, case.k))
    scaled(t.apply_batch(stack, pad_mode=mode), f"ArrayPSFTransform.apply_batch ({launch})")
    base = _bound_and_homogeneity(case, lambda f: t.apply(f, pad_mode=mode), f"ArrayPSFTransform.apply float32 in ({launch})")
    assert base.dtype == np.float64 and np.array_equal(base, single.astype(np.float64))
    wide = _bound_and_homogeneity(case, lambda f: t.apply(f.astype(np.float64), pad_mode=mode), f"ArrayPSFTransform.apply float64 in ({launch})")
    assert np.array_equal(wide, base)
    t._device_plan().set_option("host_bands", 3)
    banded = _bound_and_homogeneity(case, lambda f: t.apply(f, pad_mode=mode), "host row bands = 3")
    assert t._device_plan().host_bands() == 3
    assert np.array_equal(banded, base)


def _poisoned(frame):
    """A masked block (as a detector mask would be) and one Inf pixel, both off the frame's border."""
    bad = frame.copy()
    h, w = bad.shape
    bad[h // 3 : h // 3 + 9, w // 4 : w // 4 + 17] = np.nan
    bad[h - h // 5, w - w // 3] = np.inf
    return bad


def _non_finite_pattern_is_the_oracles(out, frame, case):
    with np.errstate(invalid="ignore"):
        ref = orc.apply_transfer(frame, case.coords, case.k, pad_mode=case.pad_mode)
    assert np.array_equal(np.isfinite(out), np.isfinite(ref))
    assert not np.isfinite(ref).all() and np.isfinite(ref).any()


@pytest.mark.parametrize(("n", "shape", "seed"), ISOLATION_CASES)
def test_isolation_between_applies_on_one_plan(n, shape, seed):
    """bright (x 1e6) -> dim -> another shape under the same corner list (fewer rows and columns, width parity changed) -> NaN block and
    Inf pixel -> dim again -> bright again, on one library plan and on one ArrayPSFTransform: each result is what a fresh plan gives for
    that frame alone, bit for bit; the dim frame meets the local bound; the non-finite pattern is the oracle's."""
    mode = "symmetric"
    case = _case(shape, n, seed, mode)
    h, w = shape
    dim = case.image
    bright = np.float32(1e6) * dim
    other = np.ascontiguousarray(hdr_frame(shape, n, seed + 1)[: h - 3, : w - 5])
    sequence = [("bright", bright), ("dim", dim), ("other shape", other), ("NaN / Inf", _poisoned(dim)), ("dim again", dim), ("bright again", bright)]
    fresh = {}
    for name, frame in sequence[:4]:
        fresh[name] = _plan(case).apply(frame, _pad(mode))
    fresh["dim again"], fresh["bright again"] = fresh["dim"], fresh["bright"]
    launch = _launch(n, shape, mode)
    if n >= 128:  # what the sequence is for: the launch with state of its own before and after a launch without
        assert _launch(n, other.shape, mode) == "separate plane sum"
    _bound(case, fresh["dim"], f"fresh plan, dim frame ({launch})")
    assert np.isfinite(fresh["bright"]).all() and np.isfinite(fresh["other shape"]).all()
    _non_finite_pattern_is_the_oracles(fresh["NaN / Inf"], sequence[3][1], case)
    other_ref, other_scale = per_patch_reference(other, case.coords, case.k, mode, np.float64)
    other_yard = local_error(per_patch_reference(other, case.coords, case.k, mode, np.float32)[0], other_ref, other_scale)
    assert local_error(fresh["other shape"], other_ref, other_scale) <= MARGIN * other_yard

    plan = _plan(case)
    t = rp.ArrayPSFTransform(rp.IndexedCube(case.coords, case.k))
    for step, (name, frame) in enumerate(sequence):
        out = plan.apply(frame, _pad(mode))
        assert np.array_equal(out, fresh[name], equal_nan=True), ("library plan", step, name, _where(out, fresh[name]))
        out = t.apply(frame, pad_mode=mode)
        assert out.dtype == np.float64
        assert np.array_equal(out, fresh[name].astype(np.float64), equal_nan=True), ("class API", step, name, _where(out, fresh[name]))
    _bound(case, plan.apply(dim, _pad(mode)), f"dim frame after bright, NaN / Inf and another shape ({launch})")


def _where(out, expect):
    """Bounding box, count and largest size of the pixels that differ (for the failure message)."""
    bad = ~((out == expect) | (np.isnan(out) & np.isnan(expect)))
    rows, cols = np.where(bad)
    if rows.size == 0:
        return "no pixel differs"
    with np.errstate(invalid="ignore"):
        worst = np.nanmax(np.abs(out[bad].astype(np.float64) - expect[bad]))
    return f"{rows.size} pixels differ, rows {rows.min()}..{rows.max()}, columns {cols.min()}..{cols.max()}, largest |d| {worst:.3e}"


@pytest.mark.parametrize(("n", "shape", "seed"), ISOLATION_CASES)
def test_isolation_between_the_frames_of_a_batch(n, shape, seed):
    """Frames of amplitude 1e6, 1, 1e-3 and a NaN-masked one in one apply_batch_device and in one streamed apply_batch: each frame equals
    its single apply on a fresh plan bit for bit, clean frames stay finite, the masked frame has the oracle's non-finite pattern.  Then, on
    the same plan, batch(4) -> single apply -> batch(2) -> batch(4): the fused launches count finished patches on per-(frame, tile)
    counters that restart when the frame count changes, and nothing of the NaN frame or the bright one may survive that."""
    from regularizepsf_amd import _native

    mode = "symmetric"
    case = _case(shape, n, seed, mode)
    h, w = shape
    stack = np.ascontiguousarray(np.stack([np.float32(1e6) * case.image, case.image, np.float32(1e-3) * case.image, _poisoned(case.image)]))
    fresh = [_plan(case).apply(frame, _pad(mode)) for frame in stack]
    assert all(np.isfinite(f).all() for f in fresh[:3])
    _non_finite_pattern_is_the_oracles(fresh[3], stack[3], case)

    plan = _plan(case)
    d_in = _native.DeviceBuffer(stack.nbytes).upload(stack)
    d_out = _native.DeviceBuffer(stack.nbytes)

    def batch(count):
        d_out.upload(np.zeros_like(stack))
        plan.apply_batch_device(d_in.ptr, d_out.ptr, count, h * w, h * w, _native.Geometry.whole(h, w, _pad(mode)))
        plan.synchronize()
        return d_out.download((4, h, w))[:count]

    try:
        got = batch(4)
        for step, count in enumerate((1, 2, 4, 1, 4)):
            if count == 1:  # the dim frame, straight after a batch whose last frame is the NaN-masked one
                out = plan.apply(stack[2], _pad(mode))
                assert np.array_equal(out, fresh[2]), ("single apply after a batch", step, _where(out, fresh[2]))
            else:
                again = batch(count)
                for f in range(count):
                    assert np.array_equal(again[f], fresh[f], equal_nan=True), ("batch again", step, count, f, _where(again[f], fresh[f]))
    finally:
        d_in.free()
        d_out.free()
    streamed = rp.ArrayPSFTransform(rp.IndexedCube(case.coords, case.k)).apply_batch(stack, pad_mode=mode)
    for f in range(4):
        assert np.array_equal(got[f], fresh[f], equal_nan=True), ("apply_batch_device", f, _where(got[f], fresh[f]))
        assert np.array_equal(streamed[f], fresh[f].astype(np.float64), equal_nan=True), ("apply_batch", f, _where(streamed[f], fresh[f]))
    launch = _launch(n, shape, mode)
    _bound(case, got[1], f"unit frame of a mixed batch, device ({launch})")
    _bound(case, streamed[1], f"unit frame of a mixed batch, streamed ({launch})")


def test_config1_starfield_local_bound():
    """BASELINE config 1 (512 x 512, 32-pixel patches, orc.starfield seed 1, orc.synthetic_transfer): a star field is the real HDR input.
    Its background is ~100 under peaks of ~9e4, so the dim-share condition is taken at 1e-2 of the largest scale here."""
    h = w = 512
    coords, k = orc.synthetic_transfer(h, w, 32)
    case = LocalCase((h, w), 32, 1, "symmetric", image=orc.starfield(h, w, 1), coords=coords, k=k, dim=1e-2)
    assert case.share >= 0.10
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    _bound_and_homogeneity(case, lambda f: t.apply(f), "config 1 star field, class API")
