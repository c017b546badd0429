"""Non-finite pixels and large pedestals on the default (no saturation) path.

The reference poisons exactly the patches that contain a NaN / Inf pixel: `fft2(w * patch)` of such a patch is non-finite in every bin,
so after `ifft2(. * K)` the whole patch is non-finite and the overlap-add (regularizepsf/transform.py:163-169) spreads it over the four
patches that cover the pixel - and, through np.pad's mirror, over the patches that read its reflection (transform.py:119-123).  Real PUNCH
frames carry NaN masks; the kernels' window tables, rim selects and fused tile sums must reproduce that pattern, not launder it.

What is compared: the SET of non-finite output pixels must be the reference's, always; for NaN pixels (the mask value in practice) the
output is NaN exactly where the reference's is; everything else meets the usual tolerance.  For a +-Inf pixel WHICH of the poisoned
pixels read +-Inf instead of NaN is an artefact of the FFT algorithm: where the pixel sits on patch-local row / column 0 or N/2 it meets
only trivial twiddles, pocketfft hands that one pixel back as +-Inf (NaN around it), and a radix-2 network leaves +-Inf in a few other
places of the same patches - every one of them inside the reference's poisoned set.
"""

import numpy as np
import pytest

import regularizepsf_amd as rp
from oracle import regpsf_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-5  # north_star: 1e-5 relative float32, on the finite pixels (SURVEY 8d metric)


def _setup(n, shape, seed):
    h, w = shape
    coords, k = orc.synthetic_transfer(h, w, n, alpha=3.0, epsilon=0.1)
    return coords, k, orc.starfield(h, w, seed)


def _compare(out, ref, nan_exact=True):
    assert out.dtype == np.float64 and out.shape == ref.shape
    bad_ref, bad_out = ~np.isfinite(ref), ~np.isfinite(out)
    assert np.array_equal(bad_out, bad_ref), f"non-finite pattern differs: {bad_out.sum()} vs {bad_ref.sum()} pixels"
    if nan_exact:
        assert np.array_equal(np.isnan(out), np.isnan(ref))
    good = ~bad_ref
    assert good.any()
    d = out[good] - ref[good]
    assert np.abs(d).max() <= TOL * np.abs(ref[good]).max()
    assert np.linalg.norm(d) <= TOL * np.linalg.norm(ref[good])
    return int(bad_ref.sum())


CASES = [(32, (160, 192)), (64, (256, 320)), (128, (512, 640)), (256, (1024, 1280))]
SPOTS = {  # where the bad pixel sits: inside, on the rim (np.pad mirrors it), in the image corner
    "interior": lambda h, w, n: (h // 2 + 3, w // 2 - 5),
    "rim": lambda h, w, n: (1, w // 2 + 1),
    "corner": lambda h, w, n: (h - 1, w - 1),
    "patch_seam": lambda h, w, n: (n // 2, n),
}


@pytest.mark.parametrize(("n", "shape"), CASES)
@pytest.mark.parametrize("spot", sorted(SPOTS))
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_non_finite_pixel_poisons_exactly_the_patches_the_reference_poisons(n, shape, spot, value):
    coords, k, image = _setup(n, shape, 7 + n)
    r, c = SPOTS[spot](*shape, n)
    image[r, c] = value
    ref = orc.apply_transfer(image, coords, k)
    out = rp.ArrayPSFTransform(rp.IndexedCube(coords, k)).apply(image)
    poisoned = _compare(out, ref, nan_exact=bool(np.isnan(value)) or spot != "patch_seam")
    assert poisoned >= (n // 2) ** 2  # at least the lattice tile around the pixel


@pytest.mark.parametrize(("n", "shape"), [(32, (160, 192)), (128, (512, 640)), (256, (1024, 1280))])
def test_nan_mask_regions_in_a_batch_and_other_pad_modes(n, shape):
    """A masked block (as a detector mask would be), several isolated NaNs, 'reflect' / 'constant' / 'wrap' padding, and the same
    frames through the streamed batch path: the pattern is the reference's in every frame, and clean frames of the batch stay clean."""
    coords, k, image = _setup(n, shape, 3 * n)
    h, w = shape
    masked = image.copy()
    masked[h // 3 : h // 3 + 9, w // 4 : w // 4 + 17] = np.nan
    masked[0, 0] = np.nan
    masked[h - 2, 5] = np.inf  # (off the patch seams: NaN wherever the reference has NaN)
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    for pad_mode in ("reflect", "constant", "wrap"):
        _compare(t.apply(masked, pad_mode=pad_mode), orc.apply_transfer(masked, coords, k, pad_mode=pad_mode))
    batch = t.apply_batch(np.stack([image, masked, image[::-1].copy()]))
    _compare(batch[1], orc.apply_transfer(masked, coords, k))
    assert np.isfinite(batch[0]).all() and np.isfinite(batch[2]).all()
    assert np.array_equal(batch[0], t.apply(image))


@pytest.mark.parametrize(("n", "shape"), [(32, (160, 192)), (128, (512, 640)), (256, (768, 1024))])
def test_float64_image_on_a_1e7_pedestal(n, shape):
    """The reference computes in float64 (transform.py:117); the kernels narrow to float32.  A frame riding on a 1e7 pedestal (bias not
    subtracted) must still meet the norm-relative bar, float64 in and float32 in alike."""
    coords, k, image = _setup(n, shape, 11)
    image64 = image.astype(np.float64) + 1.0e7
    ref = orc.apply_transfer(image64, coords, k)
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    for frame in (image64, image64.astype(np.float32)):
        out = t.apply(frame)
        ref_f = ref if frame.dtype == np.float64 else orc.apply_transfer(frame, coords, k)
        d = out - ref_f
        assert np.abs(d).max() <= TOL * np.abs(ref_f).max() and np.linalg.norm(d) <= TOL * np.linalg.norm(ref_f)


@pytest.mark.parametrize(("n", "shape", "pad_mode", "dilation", "width", "dtype"), [
    (32, (96, 128), "symmetric", 1, 7, np.float32), (32, (96, 128), "reflect", 2, 5, np.float64), (64, (200, 192), "constant", 1, 7, np.float32),
    (64, (200, 192), "edge", 3, 2, np.float32), (32, (70, 90), "wrap", 1, 1, np.float64), (128, (300, 260), "symmetric", 2, 7, np.float32),
    (16, (40, 48), "symmetric", 1, 0, np.float32), (64, (192, 192), "symmetric", 1, 7, np.int32), (256, (512, 640), "symmetric", 1, 7, np.float32)])
def test_saturation_branch_in_one_library_call(n, shape, pad_mode, dilation, width, dtype):
    """`apply(..., saturation_threshold=...)` through rpsf_apply_host_saturated: pad, mask, dilation, sequential fill, restore as the
    reference does them (regularizepsf/transform.py:117-138,171-172) - saturated pixels inside, on the rim (their mirror images in the
    pad are masked and filled on their own), in the corners, in clusters, next to NaN pixels; the raw values come back exactly."""
    h, w = shape
    coords, k = orc.synthetic_transfer(h, w, n, alpha=1.0, epsilon=0.1)
    rng = np.random.default_rng(n + dilation + width)
    image = orc.starfield(h, w, seed=3 * n).astype(np.float64)
    hot = [(0, 0), (h - 1, w - 1), (1, w // 2), (h // 2, 0), (h // 2, w // 2), (h // 2, w // 2 + 1), (h // 2 + 1, w // 2)]
    hot += [(int(r), int(c)) for r, c in zip(rng.integers(0, h, 12), rng.integers(0, w, 12))]
    for r, c in hot:
        image[r, c] = 5.0e4 + r + c
    image[h // 3 : h // 3 + 4, w // 3 : w // 3 + 5] = 7.0e4  # a saturated blob: later fills see earlier ones
    if dtype == np.float64:
        image[h // 4, w // 4] = np.nan  # a masked detector pixel next to nothing in particular
    image = image.astype(dtype)
    threshold = 2.0e4
    ref = orc.apply_transfer(image, coords, k, pad_mode=pad_mode, saturation_threshold=threshold, saturation_dilation=dilation,
                             neighborhood_width=width)
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    before = image.copy()
    out = t.apply(image, pad_mode=pad_mode, saturation_threshold=threshold, saturation_dilation=dilation, neighborhood_width=width)
    assert np.array_equal(image, before, equal_nan=True)  # the input is never modified
    _compare(out, ref)
    for r, c in hot:  # restored raw values, exactly (transform.py:172)
        assert out[r, c] == float(image[r, c]) == ref[r, c]
    # the same transform without saturated pixels in the frame, and a second saturated call on another frame size
    calm = np.minimum(np.nan_to_num(before.astype(np.float64), nan=100.0), 1.0e4)
    _compare(t.apply(calm, pad_mode=pad_mode, saturation_threshold=threshold, saturation_dilation=dilation, neighborhood_width=width),
             orc.apply_transfer(calm, coords, k, pad_mode=pad_mode, saturation_threshold=threshold, saturation_dilation=dilation,
                                neighborhood_width=width))


@pytest.mark.parametrize(("n", "shape", "frames"), [(64, (200, 192), 7), (32, (96, 128), 1), (128, (384, 320), 4)])
def test_saturated_frames_in_sequence_equal_the_loop(n, shape, frames):
    """`apply_batch(..., saturation_threshold=...)` - what the reference's example does frame by frame - prepares frame i + 1 on the host while the
    GPU corrects frame i (two staging slots in turn): every frame is the single call's, bit for bit, saturated or not, and matches the oracle."""
    h, w = shape
    coords, k = orc.synthetic_transfer(h, w, n, alpha=1.0, epsilon=0.1)
    rng = np.random.default_rng(7 * n)
    stack = []
    for f in range(frames):
        im = orc.starfield(h, w, seed=50 + f).astype(np.float64)
        if f % 3 != 2:  # every third frame has nothing above the threshold
            for r, c in zip(rng.integers(0, h, 6), rng.integers(0, w, 6)):
                im[int(r), int(c)] = 6.0e4 + f
        else:
            im = np.minimum(im, 1.0e4)
        stack.append(im.astype(np.float32))
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    kwargs = dict(saturation_threshold=2.0e4, saturation_dilation=2, neighborhood_width=5)
    loop = np.stack([t.apply(im, **kwargs) for im in stack])
    assert np.array_equal(t.apply_batch(stack, **kwargs), loop, equal_nan=True)
    assert np.array_equal(t.apply_batch(np.stack(stack), dtype=np.float32, **kwargs), loop.astype(np.float32), equal_nan=True)
    _compare(loop[0], orc.apply_transfer(stack[0], coords, k, **kwargs))
    _compare(loop[-1], orc.apply_transfer(stack[-1], coords, k, **kwargs))


def _device_free_bytes():
    """Free device memory as the HIP runtime that librpsf_hip.so loaded reports it (hipMemGetInfo)."""
    import ctypes
    import gc

    from regularizepsf_amd import _native

    _native.lib()
    with open("/proc/self/maps") as maps:
        hip = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
    assert hip, "the HIP runtime is not loaded"
    gc.collect()  # (plans of earlier tests that are only waiting for the collector)
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert ctypes.CDLL(hip[0]).hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _teardown_cases():
    """(name, round): one round creates a plan of one apply path, sets K, applies once and closes the plan."""
    from regularizepsf_amd import _native

    sym = _native.PAD_MODES["symmetric"]

    def plan_of(shape, n, k=None, coords=None, edit=None):
        c, kk = orc.synthetic_transfer(*shape, n, alpha=1.0, epsilon=0.1)
        coords, k = np.asarray(coords if coords is not None else c), k if k is not None else kk
        if edit is not None:
            coords, k = edit(coords.copy(), k)
        return coords, k

    def run(n, coords, k, image, mode=None, apply=lambda plan, im: plan.apply(im, sym), check=None):
        def one_round():
            plan = _native.Plan(n, coords)
            try:
                if mode:
                    plan.set_overlap_mode(mode)
                plan.set_transfer(k)
                out = apply(plan, image)
                assert np.isfinite(out).all()
                if check:
                    check(plan)
            finally:
                plan.close()
        return one_round

    def shift_one(coords, k):  # one corner off the half-overlap lattice: float atomics
        coords[len(coords) // 2, 0] += 3
        return coords, k

    def drop_one(coords, k):  # an incomplete lattice: colour planes, no sweep kernel
        keep = np.arange(len(coords)) != len(coords) // 2
        return coords[keep], k[keep]

    cases = []
    for name, n, shape, edit, mode in [("fallback_96", 96, (288, 288), None, None), ("atomics_32", 32, (160, 192), shift_one, None),
                                       ("planes_64", 64, (256, 320), drop_one, None), ("sweep_32", 32, (160, 192), None, None),
                                       ("fused_128", 128, (512, 640), None, None), ("persistent_256", 256, (1024, 1280), None, None),
                                       ("direct_256", 256, (1024, 1280), None, "direct")]:
        coords, k = plan_of(shape, n, edit=edit)
        cases.append((name, run(n, coords, k, orc.starfield(*shape, seed=n), mode)))
    # a 4096^2 host frame is cut into row bands: views of the plan that borrow its tables, packed K and error word
    big = np.asarray(rp.calculate_covering((4096, 4096), 64))
    k_big = np.ones((len(big), 64, 64), np.complex64)

    def banded(plan):
        assert plan.host_bands() >= 2

    cases.append(("host_bands_64", run(64, big, k_big, orc.starfield(4096, 4096, seed=5), check=banded)))
    coords, k = plan_of((96, 128), 32)
    hot = orc.starfield(96, 128, seed=9).astype(np.float64)
    hot[40:44, 50:55] = 7.0e4
    cases.append(("saturated_32", run(32, coords, k, hot, apply=lambda plan, im: plan.apply_host_saturated(im, sym, 5.0e4, 1, 7))))
    return cases


def test_plans_of_every_apply_path_give_back_all_device_memory():
    """20 rounds of create / set K / apply / close on every apply path leave device memory as one warm-up round of each left it
    (code objects, the process-wide host pool and hipFFT's own state are allocated once per process, not per plan)."""
    cases = _teardown_cases()
    for name, one_round in cases:
        print(name)  # (shown with a failure: which path)
        one_round()
    before = _device_free_bytes()
    for name, one_round in cases:
        for _ in range(20):
            one_round()
        after = _device_free_bytes()
        assert after >= before, f"{name}: {before - after} bytes of device memory not given back after 20 plans"
