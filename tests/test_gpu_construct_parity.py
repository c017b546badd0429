"""The construct side - PSF samples -> spectra (K3) -> transfer kernel (K2, one-pass packer) -> apply - per PSF and per frequency bin.

The other GPU modules hand `apply` a K of their own, or compare the chain with the oracle run on the K the device itself produced, and
judge spectra and K by 1e-5 of the largest value of a whole cube.  Here every step is compared with the oracle's step in the next wider
precision on THE SAME inputs, and bounded by MARGIN (tests/helpers.py, 4) x the yardstick: the same step carried out by NumPy / SciPy in
the kernel's precision.  tests/test_construct_cases.py proves on the CPU that every yardstick is float rounding and nothing else and
that the cases contain what the global bar hides.

    K3   per PSF: max over bins |got - fft2(float64(v))| / max over bins |fft2(float64(v))| - its OWN peak; figure of a cube = the largest
         over its PSFs; yardstick = the same for scipy.fft.fft2 on the float32 cube.  Cubes cycle through narrow Gaussians, coma PSFs,
         white noise, a shifted unit sample (every bin has the same modulus: the figure is a per-bin relative error there, asserted on
         its own) and a constant, each times 10**k, k in [-3, 3].  No tolerance: the three entry points agree bit for bit;
         psf_fft(1024 v) == 1024 psf_fft(v) and the same for 1 / 1024; PSF i inside a cube == PSF i alone (idle teams of a workgroup,
         chunk borders); rasterised samples == the same samples uploaded.
    K2   per bin: max |k - truth| / |truth| over the in-range bins (every quantity of the formula finite and inside 2**-120 ... 2**120 in
         the float64 evaluation; 2**-1000 ... 2**1000 in long double for the double kernel); truth = orc.construct_transfer one precision
         up, yardstick = orc.construct_transfer in the kernel's precision.  Ten alphas x three epsilons reach every branch of np_pow.  A bin
         whose truth is exactly 0 is exactly 0; where the truth is not finite, NaN and +-Inf sit where NumPy's same-precision result has them.
    chain   float32 samples of PSFs whose float32 chain is well-conditioned (broadband_psfs) -> ArrayPSF -> construct -> apply, local error
         (LocalCase) against the chain done in float64; yardstick = the reference's chain done in float32; the global 1e-5 bar beside it.

Measured on an MI355X (kernel / yardstick; log: profiles/construct_parity_gpu.log;
the whole module takes 48 s there, nearly all of it the float64 and long-double references on the host).  min ... max over the cases of a row; K2 rows by
the np_pow branches that alpha - 1 / alpha + 1 take, over four input pairs and three epsilons:

    kernel                                                     N = 16        24            32            64            128           256
    K3 psf_fft, counts 1 ... 23 and the chunk-crossing cubes   1.09 ... 2.79               0.87 ... 1.61 1.08 ... 1.70 0.89 ... 1.35 1.00 ... 1.27
      the shifted unit samples of those cubes (per bin)        2.05 ... 3.20               0.80 ... 1.58 1.08          1.10 ... 1.35 1.13 ... 1.27
    K2 float (build_transfer_device == build_transfer, bitwise)
      1/x / x                 (alpha 0)                                                    0.72 ... 0.99 0.80 ... 1.27               0.85 ... 1.00
      pow / pow               (alpha 0.5, 2.5)                                             0.52 ... 1.18 0.77 ... 1.15               0.71 ... 1.10
      1 / x*x                 (alpha 1)                                                    0.68 ... 1.03 0.71 ... 1.00               0.85 ... 0.98
      sqrt / pow              (alpha 1.5)                                                  0.55 ... 0.96 0.79 ... 1.09               0.82 ... 0.95
      x / float64 product     (alpha 2)                                                    0.64 ... 1.14 0.74 ... 1.03               0.74 ... 1.10
      x*x / float64 product   (alpha 3)                                                    0.53 ... 0.98 0.68 ... 1.19               0.76 ... 1.04
      float64 product twice   (alpha 4, 5, 7)                                              0.63 ... 2.40 0.62 ... 1.76               0.74 ... 1.45
    K2 float through construct() on resident spectra           (all branches)              0.63 ... 1.10 0.70 ... 1.38               0.65 ... 1.25
    K2 float, host route in two rounds (131 PSFs, alpha 3)                                                                           0.88
    K2 double (no product branch: 3 ... 8 go to pow)
      1/x / x, 1 / x*x, x / pow, x*x / pow                                                 0.63 ... 1.17 0.72 ... 1.04               0.72 ... 1.14
      sqrt / pow, pow / pow                                                                0.48 ... 1.22 0.67 ... 1.33               0.62 ... 1.26
    chain, device-resident spectra: HDR frame                                              0.97 ... 1.03 0.84 ... 1.09 0.82 ... 1.00 0.96 ... 0.97
                                    star field                                             1.25 ... 1.48 1.00 ... 1.58 1.04 ... 1.29 0.66 ... 1.88
    chain, host spectra (scipy):    HDR frame                                1.03 ... 1.05 0.91 ... 1.00 0.83 ... 1.06 0.90 ... 0.98 0.98 ... 1.00
                                    star field                               1.17 ... 1.29 1.13 ... 1.51 1.02 ... 1.50 1.04 ... 1.39 0.66 ... 1.88

Yardsticks: K3 2.9e-8 ... 3.6e-7, K2 float 1.7e-7 ... 1.8e-6, K2 double 2.9e-16 ... 3.6e-15, chain 1.1e-7 ... 3.5e-7 (global 9e-8 ... 8e-7).  Nothing comes
near MARGIN = 4 except the shifted unit sample at N = 16, where the yardstick itself is 0.6 float32 epsilon (7.5e-8: pocketfft's 16-point
transform of a unit sample is nearly exact) and the kernel's 2.4e-7 is two epsilon.  The generic-pow branch (device libm) stays within 1.18 x
NumPy's powf / 1.33 x its pow.  Every bit-for-bit property held: entry points, homogeneity, isolation, rasterised == uploaded, host == device K2 route.
"""

import numpy as np
import pytest
import scipy.fft

import regularizepsf_amd as rp
from oracle import regpsf_oracle as orc
from regularizepsf_amd.psf import varied_functional_psf
from tests.helpers import (CHAIN_CASES, CHAIN_PARAMETERS, CONSTRUCT_ALPHAS, CONSTRUCT_EPSILONS, CONSTRUCT_INPUTS, CONSTRUCT_SIZES, MARGIN,
                           YARDSTICK_EPSILONS_F64, TransferCase, chain_case, construct_samples, construct_spectra, pow_branches, psf_cube, rel_errors,
                           spectrum_errors)

pytestmark = pytest.mark.gpu
TOL = 1e-5  # the global bar of the other modules, kept beside the local one
SCALES = (np.float32(1024.0), np.float32(1.0 / 1024.0))
K3_SIZES = (16, 32, 64, 128, 256)
K3_COUNTS = (1, 2, 3, 5, 7, 23)  # small odd counts leave teams of the last workgroup idle at every N
K3_CHUNK_CROSSING = ((256, 131, 128), (128, 515, 512))  # (N, PSFs, PSFs per chunk of 64 MiB of spectra in psf_fft_impl)
CHAIN_LAUNCH = {32: "sweep", 64: "sweep", 128: "persistent + fused", 256: "persistent + fused", 24: "hipFFT fallback, host spectra"}


def _line(kernel, n, case, yardstick, ratio):
    print(f"CONSTRUCT-RATIO | {kernel} | N={n} | {case} | yardstick {yardstick:.2e} | ratio {ratio:.2f}")


# ---- K3 ----------------------------------------------------------------------------------------------------------------------------
def _coords(count):
    return [(i, i) for i in range(count)]


def _spectra_by_every_entry(cube):
    """_native.psf_fft (host out), _native.psf_fft_device + download, ArrayPSF(device=0).fft_evaluations: one kernel, the same bits."""
    from regularizepsf_amd import _native

    got = _native.psf_fft(cube)
    buf = _native.psf_fft_device(cube)
    try:
        resident = buf.download(cube.shape, np.complex64)
    finally:
        buf.free()
    by_class = rp.ArrayPSF(rp.IndexedCube(_coords(len(cube)), cube), device=0).fft_evaluations
    assert got.dtype == resident.dtype == by_class.dtype == np.complex64
    assert np.array_equal(got, resident), "psf_fft_device differs from psf_fft"
    assert np.array_equal(got, by_class), "ArrayPSF(device=0) differs from psf_fft"
    return got


def _spectra_bound(n, cube, kinds, got):
    truth = scipy.fft.fft2(cube.astype(np.float64))
    errors, yard = spectrum_errors(got, truth), spectrum_errors(scipy.fft.fft2(cube), truth)
    ratio = errors.max() / yard.max()
    _line("K3 psf_fft", n, f"{len(cube)} PSFs", yard.max(), ratio)
    assert 0 < yard.max() < 1e-6
    assert ratio <= MARGIN, (n, len(cube), int(errors.argmax()), kinds[int(errors.argmax())], errors.max(), yard.max())
    delta = [i for i, kind in enumerate(kinds) if kind == "delta"]
    if delta:
        ratio = errors[delta].max() / yard[delta].max()
        _line("K3 psf_fft", n, f"{len(cube)} PSFs, the shifted unit samples (per bin)", yard[delta].max(), ratio)
        assert 0 < yard[delta].max() < 1e-6 and ratio <= MARGIN, (n, len(cube), errors[delta], yard[delta])


def _spectra_scale_exactly(cube, base):
    """(samples below 2**-60 - float32 denormals in the far tails of the Gaussians, which a division by 1024 would round - are zero in ``cube``)"""
    from regularizepsf_amd import _native

    for s in SCALES:
        assert np.array_equal(_native.psf_fft(s * cube), s * base), float(s)


def _without_denormal_tails(cube):
    out = cube.copy()
    out[np.abs(out) < 2.0 ** -60] = 0
    return out


@pytest.mark.parametrize("n", K3_SIZES)
def test_spectra_per_psf_small_cubes(n):
    from regularizepsf_amd import _native

    assert K3_SIZES == _native.SUPPORTED_PATCH_SIZES
    for count in K3_COUNTS:
        cube, kinds = psf_cube(n, count, 0)
        got = _spectra_by_every_entry(cube)
        _spectra_bound(n, cube, kinds, got)
        for i in range(count):
            assert np.array_equal(got[i], _native.psf_fft(cube[i : i + 1])[0]), (n, count, i, kinds[i], "differs from the PSF alone")
        trimmed = _without_denormal_tails(cube)
        _spectra_scale_exactly(trimmed, _native.psf_fft(trimmed))


@pytest.mark.parametrize(("n", "count", "chunk"), K3_CHUNK_CROSSING)
def test_spectra_per_psf_across_a_chunk_border(n, count, chunk):
    from regularizepsf_amd import _native

    assert chunk * n * n * 8 == 64 << 20 and chunk < count
    cube, kinds = psf_cube(n, count, 0)
    got = _spectra_by_every_entry(cube)
    _spectra_bound(n, cube, kinds, got)
    for i in (0, chunk - 1, chunk, count - 1):
        assert np.array_equal(got[i], _native.psf_fft(cube[i : i + 1])[0]), (n, count, i, kinds[i], "differs from the PSF alone")
    trimmed = _without_denormal_tails(cube)
    _spectra_scale_exactly(trimmed, _native.psf_fft(trimmed))


@pytest.mark.parametrize("n", [32, 128, 256])
def test_rasterised_samples_give_the_spectra_of_the_same_samples_uploaded(n):
    """as_array_psf(device=0) rasterises into the buffer K3 reads; psf_fft uploads the downloaded samples into another: same kernel, same bits."""
    from regularizepsf_amd import _native

    shape = (3 * n, 4 * n)
    coords = [tuple(int(v) for v in c) for c in rp.calculate_covering(shape, n)]

    @varied_functional_psf(rp.elliptical_gaussian)
    def field(row, col):
        return {"amplitude": 2.0 + row / 300, "row0": n / 2 + 0.3 * col / 420, "col0": n / 2 - 0.2, "sigma_row": 0.7 + row / (4 * shape[0]),
                "sigma_col": 0.9 + col / (5 * shape[1]), "theta": 0.4 + (row + col) / 700, "background": 1e-3}

    for normalize in (False, True):
        dev = field.as_array_psf(coords, n, device=0, normalize=normalize)
        got = dev.fft_evaluations
        values = dev.values
        assert values.dtype == np.float32 and got.dtype == np.complex64
        assert np.array_equal(got, _native.psf_fft(values)), (n, normalize)
        _spectra_bound(n, values, ["gauss"] * len(values), got)


# ---- K2 ----------------------------------------------------------------------------------------------------------------------------
def _branch_summary(kernel, n, worst):
    for branches, ratio in sorted(worst.items()):
        print(f"CONSTRUCT-BRANCH | {kernel} | N={n} | np_pow {branches} | worst ratio {ratio:.2f}")


@pytest.mark.parametrize("n", CONSTRUCT_SIZES)
@pytest.mark.parametrize("kind", CONSTRUCT_INPUTS)
def test_transfer_kernel_per_bin_float(kind, n):
    """build_transfer_kernel<float> through _native.build_transfer_device (spectra uploaded once) and _native.build_transfer (host arrays):
    the per-bin bound for every alpha and epsilon, the two routes bit-identical."""
    from regularizepsf_amd import _native

    s, t = construct_spectra(kind, n, np.complex64)
    bufs = [_native.DeviceBuffer(s.nbytes) for _ in range(3)]
    worst = {}
    try:
        bufs[0].upload(s)
        bufs[1].upload(t)
        for alpha in CONSTRUCT_ALPHAS:
            for eps in CONSTRUCT_EPSILONS:
                case = TransferCase(s, t, alpha, eps, label=f"{kind} alpha {alpha} eps {eps}")
                _native.build_transfer_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, s.size, False, alpha, eps)
                k = bufs[2].download(s.shape, np.complex64)
                ratio = case.ratio(k)
                _line("K2 float", n, f"{case.label} [np_pow {pow_branches(alpha)}] in range {case.share:.2f}", case.yardstick, ratio)
                worst[pow_branches(alpha)] = max(worst.get(pow_branches(alpha), 0.0), ratio)
                case.check(k, what="build_transfer_device")
                assert np.array_equal(_native.build_transfer(s, t, alpha, eps), k, equal_nan=True), (case.label, "host route differs")
    finally:
        for b in bufs:
            b.free()
    _branch_summary(f"K2 float {kind}", n, worst)


@pytest.mark.parametrize(("n", "count"), [(32, None), (64, None), (256, 2)])
@pytest.mark.parametrize("kind", CONSTRUCT_INPUTS)
def test_transfer_kernel_per_bin_double(kind, n, count):
    """build_transfer_kernel<double> against the formula in long double."""
    from regularizepsf_amd import _native

    if not np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        pytest.skip("long double is no wider than double here: no truth for the double kernel")
    s, t = construct_spectra(kind, n, np.complex128, count)
    worst = {}
    for alpha in CONSTRUCT_ALPHAS:
        for eps in CONSTRUCT_EPSILONS:
            case = TransferCase(s, t, alpha, eps, label=f"{kind} alpha {alpha} eps {eps}")
            assert case.truth.dtype == np.clongdouble and case.share >= 0.10 and 0 < case.yardstick < YARDSTICK_EPSILONS_F64 * np.finfo(np.float64).eps, (case.label, case.share, case.yardstick)
            k = _native.build_transfer(s, t, alpha, eps)
            ratio = case.ratio(k)
            branches = pow_branches(alpha, double=True)
            _line("K2 double", n, f"{case.label} [np_pow {branches}] in range {case.share:.2f}", case.yardstick, ratio)
            worst[branches] = max(worst.get(branches, 0.0), ratio)
            case.check(k, what="build_transfer (complex128)")
    _branch_summary(f"K2 double {kind}", n, worst)


@pytest.mark.parametrize("n", CONSTRUCT_SIZES)
@pytest.mark.parametrize("kind", ["coma", "scaled"])
def test_transfer_kernel_per_bin_class_route_on_resident_spectra(kind, n):
    """ArrayPSF(device=0) -> ArrayPSFTransform.construct: the spectra are K3's and stay on the GPU, the plan gets K from the one-pass
    packer, and `_transfer_kernel.values` is K2 on the same resident spectra.  Inputs of the bound = the spectra the device holds."""
    from regularizepsf_amd import _native

    src, tgt = construct_samples(kind, n)
    coords = _coords(len(src))
    ps = rp.ArrayPSF(rp.IndexedCube(coords, src), device=0)
    pt = rp.ArrayPSF(rp.IndexedCube(coords, tgt), device=0)
    built = []
    for alpha in CONSTRUCT_ALPHAS:
        for eps in CONSTRUCT_EPSILONS:
            tr = rp.ArrayPSFTransform.construct(ps, pt, alpha, eps)
            assert tr._transfer_kernel._loader is not None and tr._plan is not None  # the resident route
            built.append((alpha, eps, tr._transfer_kernel.values))
    s, t = ps.fft_evaluations, pt.fft_evaluations  # fetched only now: every construct above read the resident copies
    assert s.dtype == t.dtype == np.complex64
    worst = {}
    for alpha, eps, k in built:
        case = TransferCase(s, t, alpha, eps, label=f"{kind} alpha {alpha} eps {eps}")
        assert case.share >= 0.10 and 0 < case.yardstick < 2e-6, (case.label, case.share, case.yardstick)
        ratio = case.ratio(k)
        _line("K2 float, construct() on resident spectra", n, f"{case.label} [np_pow {pow_branches(alpha)}] in range {case.share:.2f}", case.yardstick, ratio)
        worst[pow_branches(alpha)] = max(worst.get(pow_branches(alpha), 0.0), ratio)
        case.check(k, what="construct() on resident spectra")
        assert np.array_equal(k, _native.build_transfer(s, t, alpha, eps), equal_nan=True), case.label
    _branch_summary(f"K2 float, class route {kind}", n, worst)


def test_transfer_kernel_host_route_across_its_round_of_8_mi_elements():
    """131 x 256 x 256 complex64 = 8.6 Mi elements: rpsf_build_transfer takes two rounds.  The same bits as the cube built in two halves
    (one round each), and the per-bin bound over the whole cube."""
    from regularizepsf_amd import _native

    n, count, alpha, eps = 256, 131, 3.0, 0.1
    s, t = construct_spectra("coma", n, np.complex64, count)
    assert s.size > 8 << 20 > (count // 2 + 1) * n * n
    k = _native.build_transfer(s, t, alpha, eps)
    half = count // 2
    assert np.array_equal(k[:half], _native.build_transfer(s[:half], t[:half], alpha, eps), equal_nan=True)
    assert np.array_equal(k[half:], _native.build_transfer(s[half:], t[half:], alpha, eps), equal_nan=True)
    case = TransferCase(s, t, alpha, eps, label=f"coma alpha {alpha} eps {eps}, {count} PSFs")
    assert case.share >= 0.10 and 0 < case.yardstick < 2e-6
    _line("K2 float, host route in two rounds", n, f"{case.label} in range {case.share:.2f}", case.yardstick, case.ratio(k))
    case.check(k, what="build_transfer in two rounds")


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
def _chain_bound(case, out, path):
    out = np.asarray(out, np.float64)
    rel_max, rel_l2 = rel_errors(out, case.ref)
    ratio = case.ratio(out)
    _line(f"chain | {path}", case.n, f"{case.shape[0]}x{case.shape[1]} dim share {case.share:.2f} global {rel_max:.1e}", case.yardstick, ratio)
    assert rel_max <= TOL and rel_l2 <= TOL, (path, rel_max, rel_l2)
    case.check(out, MARGIN, path)


@pytest.mark.parametrize(("alpha", "eps"), CHAIN_PARAMETERS)
@pytest.mark.parametrize(("n", "shape", "seed"), CHAIN_CASES)
def test_chain_against_the_chain_in_float64(n, shape, seed, alpha, eps):
    """float32 samples -> ArrayPSF -> construct -> apply on an HDR frame and on a star field.  Truth: orc.psf_fft, orc.construct_transfer and
    the per-patch apply in float64 from the same samples - NOT the oracle run on the K the device made, so an error of K3 or K2 is inside
    the comparison.  Device-resident spectra (one-pass packer) and host spectra from scipy (K2 + pack; _native.build_transfer and the
    hipFFT fallback at N = 24, where ArrayPSF has no spectrum kernel and device=0 is the host route as well)."""
    from regularizepsf_amd import _native

    hdr, src, tgt = chain_case(n, shape, seed, alpha, eps)
    star = chain_case(n, shape, seed, alpha, eps, image=orc.starfield(*shape, seed), min_share=0.0)[0]
    coords = hdr.coords
    tag = f"alpha {alpha} eps {eps}, {CHAIN_LAUNCH[n]}"
    routes = [("host spectra", None)]
    if n in _native.SUPPORTED_PATCH_SIZES:
        routes.insert(0, ("device chain", 0))
    for name, device in routes:
        ps = rp.ArrayPSF(rp.IndexedCube(coords, src), device=device)
        pt = rp.ArrayPSF(rp.IndexedCube(coords, tgt), device=device)
        tr = rp.ArrayPSFTransform.construct(ps, pt, alpha, eps)
        assert (tr._transfer_kernel._loader is not None) == (device is not None)  # resident spectra: K is still on the device only
        _chain_bound(hdr, tr.apply(hdr.image), f"{name}, HDR frame, {tag}")
        _chain_bound(star, tr.apply(star.image), f"{name}, star field, {tag}")
        assert tr._transfer_kernel.values.dtype == np.complex64
