"""The conditions of tests/test_gpu_construct_parity.py, proved from NumPy / SciPy and the oracle alone.

That module bounds the kernels that MAKE the transfer kernel K (PSF samples -> spectra -> K -> apply) by MARGIN x a yardstick, the same step
carried out by the reference's arithmetic in the kernel's precision.  Such a bound says something only if the yardstick is float rounding
and nothing else, and if the cases contain what a global bar hides: PSFs far dimmer than the brightest of their cube, bins of K decades
below its peak, frames with dim regions.  Nothing here touches the GPU, so the cases are checked wherever the suite runs.
"""

import functools

import numpy as np
import pytest
import scipy.fft

from oracle import regpsf_oracle as orc
from tests.helpers import (CHAIN_CASES, CHAIN_PARAMETERS, CONSTRUCT_ALPHAS, CONSTRUCT_EPSILONS, CONSTRUCT_INPUTS, CONSTRUCT_SIZES, PSF_KINDS,
                           RANGE_F32, YARDSTICK_EPSILONS_F64, LocalCase, TransferCase, chain_case, chain_samples, chain_transfer, construct_spectra, dim_psf_share,
                           in_range_bins, make_psfs, pow_branch, psf_cube, spectrum_errors, transfer_terms)

K3_SIZES = (16, 32, 64, 128, 256)  # _native.SUPPORTED_PATCH_SIZES (asserted equal in the GPU module)
K3_COUNTS = (1, 2, 3, 5, 7, 23)
K3_CHUNK_CROSSING = ((256, 131), (128, 515))  # (N, PSFs): one more than two / a few more than one chunk of 64 MiB of spectra


@pytest.mark.parametrize(("n", "count"), [(n, c) for n in K3_SIZES for c in K3_COUNTS] + list(K3_CHUNK_CROSSING))
def test_psf_cubes_have_dim_psfs_and_a_rounding_yardstick(n, count):
    cube, kinds = psf_cube(n, count, 0)
    assert cube.dtype == np.float32 and cube.shape == (count, n, n) and kinds == [PSF_KINDS[i % 5] for i in range(count)]
    assert np.array_equal(cube, psf_cube(n, count, 0)[0])  # seeded
    truth = scipy.fft.fft2(cube.astype(np.float64))
    single = scipy.fft.fft2(cube)
    assert single.dtype == np.complex64
    yardstick = spectrum_errors(single, truth).max()
    assert 0 < yardstick < 1e-6, yardstick
    if count >= 23:
        assert dim_psf_share(truth) >= 0.5, dim_psf_share(truth)
    delta = [i for i, kind in enumerate(kinds) if kind == "delta"]
    if delta:  # every bin of a shifted unit sample has the same modulus: the per-PSF figure is a per-bin relative error there
        mod = np.abs(truth[delta])
        assert np.allclose(mod, mod[:, :1, :1], rtol=1e-12, atol=0)
        assert 0 < spectrum_errors(single[delta], truth[delta]).max() < 1e-6


def test_psf_amplitudes_span_six_decades():
    cube, kinds = psf_cube(16, 200, 0)
    amps = sorted({float(cube[i].max()) for i, kind in enumerate(kinds) if kind in ("delta", "constant")})
    assert np.allclose(amps, 10.0 ** np.arange(-3, 4), rtol=1e-6), amps


def test_transfer_terms_is_the_oracles_formula():
    s, t = construct_spectra("coma", 32, np.complex128)
    for alpha, eps in ((3.0, 0.1), (0.5, 1e-3), (7.0, 1.0)):
        k, terms = transfer_terms(s, t, alpha, eps)
        assert len(terms) == 9 and np.array_equal(k, orc.construct_transfer(s, t, alpha, eps), equal_nan=True)


def test_alphas_reach_every_power_branch():
    exponents = {a + d for a in CONSTRUCT_ALPHAS for d in (-1.0, 1.0)}
    assert {-1.0, 0.0, 0.5, 1.0, 2.0} <= exponents and {3.0, 4.0, 5.0, 6.0, 8.0} <= exponents and {-0.5, 1.5, 2.5, 3.5} <= exponents
    assert {pow_branch(e) for e in exponents} == {"1", "x", "x*x", "sqrt", "1/x", "float64 product", "pow"}


@functools.lru_cache(maxsize=2)
def _spectra(kind, n):
    return construct_spectra(kind, n, np.complex64)


@pytest.mark.parametrize("n", CONSTRUCT_SIZES)
@pytest.mark.parametrize("kind", CONSTRUCT_INPUTS)
def test_transfer_cases_are_in_range_and_the_yardstick_is_rounding(kind, n):
    """Every alpha and epsilon: at least a tenth of the bins in range, NumPy's complex64 evaluation finite and within 2e-6 per bin there; the
    coma cases at alpha 3 / eps 0.1 span 3.5 decades of |K| inside the in-range bins."""
    s, t = _spectra(kind, n)
    assert s.dtype == t.dtype == np.complex64
    for alpha in CONSTRUCT_ALPHAS:
        for eps in CONSTRUCT_EPSILONS:
            case = TransferCase(s, t, alpha, eps)
            assert case.share >= 0.10, (alpha, eps, case.share)
            assert np.isfinite(case.same_precision[case.mask]).all()
            assert 0 < case.yardstick < 2e-6, (alpha, eps, case.yardstick)
            if kind == "coma" and (alpha, eps) == (3.0, 0.1):
                assert case.decades() >= 3.5, case.decades()


def test_exact_zeros_in_float32_spectra():
    """What the two assertions of the GPU module outside the in-range bins rest on.  scipy's float32 spectrum of the Gaussian 1.8 is
    exactly 0 in a few bins at N = 256 (its tail is below float32 rounding there).  As a source: alpha < 1 divides by it and the truth is not
    finite; at alpha 2 the truth is exactly 0 with nothing out of range on the way, so K has to be 0.  As the coma case's target: the
    truth is exactly 0 there; it counts as an owed zero at alpha 1 ... 2, and not at alpha 7, where |S|**8 underflows in float32 and the
    reference's own complex64 evaluation is 0 / 0 (asserted here, so that the exclusion rests on the reference, not on a kernel)."""
    s, t = _spectra("gauss", 256)
    at = s == 0
    assert at.sum() >= len(s) and not (t == 0).any()
    truth, mask, zero = in_range_bins(s.astype(np.complex128), t.astype(np.complex128), 0.5, 0.1, RANGE_F32)
    assert not np.isfinite(truth[at]).any() and not mask[at].any() and not zero.any()
    truth, mask, zero = in_range_bins(s.astype(np.complex128), t.astype(np.complex128), 2.0, 1.0, RANGE_F32)
    assert (truth[at] == 0).all() and np.array_equal(zero, at) and not (mask & zero).any()
    s, t = _spectra("coma", 256)
    at = t == 0
    assert at.sum() >= len(s) and not (s == 0).any()
    for alpha in (1.0, 1.5, 2.0):
        case = TransferCase(s, t, alpha, 0.1)
        assert (case.truth[at] == 0).all() and np.array_equal(case.zero, at) and (case.same_precision[at] == 0).all()
    case = TransferCase(s, t, 7.0, 1.0)
    assert (case.truth[at] == 0).all() and not case.zero.any() and np.isnan(case.same_precision[at]).all()


def test_double_cases_are_in_range():
    if not np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        pytest.skip("long double is no wider than double here: no truth for the double kernel")
    s, t = construct_spectra("coma", 32, np.complex128)
    for alpha in CONSTRUCT_ALPHAS:
        case = TransferCase(s, t, alpha, 0.1)
        assert case.truth.dtype == np.clongdouble and case.share >= 0.10 and 0 < case.yardstick < YARDSTICK_EPSILONS_F64 * np.finfo(np.float64).eps, (alpha, case.share, case.yardstick)


@pytest.mark.parametrize(("n", "shape", "seed"), CHAIN_CASES)
def test_chain_cases_are_well_conditioned_in_float32(n, shape, seed):
    """Broadband PSFs: no spectrum bin below 1e-3 of the peak, the reference's float32 chain within float32 rounding of its float64 chain
    (LocalCase asserts 0 < yardstick < 1e-6 and a dim share of at least 0.10 on the HDR frame)."""
    coords, src, tgt = chain_samples(n, shape)
    assert src.dtype == tgt.dtype == np.float32
    s32 = np.abs(scipy.fft.fft2(src))
    assert s32.min() / s32.max() >= 1e-3, s32.min() / s32.max()
    for alpha, eps in CHAIN_PARAMETERS:
        case, _, _ = chain_case(n, shape, seed, alpha, eps)
        assert isinstance(case, LocalCase) and case.share >= 0.10 and 0 < case.yardstick < 1e-6
        print(f"CHAIN-CASE | N={n} {shape[0]}x{shape[1]} alpha {alpha} eps {eps} | dim share {case.share:.2f} | yardstick {case.yardstick:.2e}")


def test_yardstick_k_defaults_to_k():
    """LocalCase with the yardstick's K given explicitly as what it takes by default gives the same figures."""
    a = LocalCase((100, 135), 16, 16)
    b = LocalCase((100, 135), 16, 16, yardstick_k=a.k)
    assert a.yardstick == b.yardstick and a.share == b.share and np.array_equal(a.ref, b.ref)


def test_float32_chain_of_the_benchmark_psfs_is_ill_conditioned():
    """NumPy / SciPy against themselves, not the kernels: for the coma PSFs of the benchmark the float32 spectra bottom out in rounding
    noise, and K from them differs from K from float64 spectra of the SAME samples by more than half the peak of K.  Whoever
    wants to move the chain test to these PSFs finds here why it is on broadband ones."""
    n, shape = 32, (130, 203)
    coords = [tuple(int(v) for v in c) for c in orc.calculate_covering(shape, n)]
    src, tgt = (np.asarray(a, np.float32) for a in make_psfs("coma", coords, n, *shape))
    with np.errstate(all="ignore"):
        s32, k32 = chain_transfer(src, tgt, 3.0, 0.1, np.float32)
        s64, k64 = chain_transfer(src, tgt, 3.0, 0.1, np.float64)
    floor32, floor64 = np.abs(s32)[np.abs(s32) > 0].min(), np.abs(s64).min()
    assert floor32 > 5 * floor64, (floor32, floor64)
    good = np.isfinite(k32)
    assert good.mean() > 0.99
    worst = np.abs(k32.astype(np.complex128) - k64)[good].max() / np.abs(k64).max()
    print(f"CHAIN-CASE | coma N=32: float32 K - float64 K = {worst:.2f} x peak, spectrum floor {floor32:.1e} (float32) / {floor64:.1e} (float64)")
    assert worst > 0.5, worst
