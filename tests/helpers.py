"""Shared test helpers: seeded synthetic cases used by the golden generator and the parity tests."""

from __future__ import annotations

import hashlib
import pathlib

import numpy as np

from oracle import regpsf_oracle as orc

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"

# (name, H, W, N, alpha, eps, psf kind, pad_mode, image seed)
APPLY_CASES = [
    ("n32_sym", 96, 80, 32, 3.0, 0.1, "coma", "symmetric", 11),
    ("n32_reflect", 96, 80, 32, 1.0, 0.1, "coma", "reflect", 12),
    ("n32_constant", 70, 100, 32, 2.0, 0.01, "gauss", "constant", 13),
    ("n32_edge", 64, 64, 32, 1.0, 0.1, "coma", "edge", 14),
    ("n32_wrap", 64, 96, 32, 1.0, 0.1, "coma", "wrap", 15),
    ("n32_mean", 64, 96, 32, 1.0, 0.1, "coma", "mean", 16),
    ("n16_sym", 40, 56, 16, 1.0, 0.1, "gauss", "symmetric", 17),
    ("n64_sym", 160, 200, 64, 3.0, 0.1, "coma", "symmetric", 21),
    ("n64_identity", 128, 128, 64, 3.0, 0.1, "identity", "symmetric", 22),
    ("n128_sym", 300, 256, 128, 1.0, 0.1, "coma", "symmetric", 31),
    ("n256_sym", 300, 280, 256, 3.0, 0.1, "coma", "symmetric", 41),
    ("n256_identity", 512, 512, 256, 3.0, 0.1, "identity", "symmetric", 42),
]


def make_psfs(kind: str, coords, n: int, h: int, w: int):
    """Source / target PSF cubes (float64) for a case; shared with tests via tests/helpers.py."""
    if kind == "coma":
        src = np.stack([orc.coma_psf(n, r, c, h, w) for r, c in coords])
        tgt = np.broadcast_to(orc.gaussian_psf(n, 1.8), src.shape).copy()
    elif kind == "gauss":
        src = np.broadcast_to(orc.gaussian_psf(n, 1.8), (len(coords), n, n)).copy()
        tgt = np.broadcast_to(orc.gaussian_psf(n, 1.5), src.shape).copy()
    else:  # identity: source == target, as in the reference's tests/test_transform.py:29-49
        src = np.broadcast_to(orc.gaussian_psf(n, 3 / 2.355), (len(coords), n, n)).astype(np.float32)
        tgt = src
    return src, tgt




def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_apply_case(name: str):
    """Return (fixture dict, coords list, K complex64 rebuilt with the oracle and checked against the stored hash)."""
    fx = np.load(GOLDEN / f"apply_{name}.npz")
    h, w, n = (int(v) for v in fx["meta"])
    coords = [tuple(int(v) for v in t) for t in fx["coords"]]
    kind = str(fx["kind"])
    src, tgt = make_psfs(kind, coords, n, h, w)
    s_fft = orc.psf_fft(src)
    t_fft = s_fft if kind == "identity" else orc.psf_fft(tgt)
    with np.errstate(all="ignore"):
        k = orc.construct_transfer(s_fft, t_fft, float(fx["alpha"]), float(fx["eps"])).astype(np.complex64)
    assert sha(k) == str(fx["k_sha256"]), f"oracle construct differs from the reference for case {name}"
    return fx, coords, k


def rel_errors(out: np.ndarray, ref: np.ndarray) -> tuple[float, float]:
    """(max|d| / max|ref|, ||d||2 / ||ref||2): the parity metric of SURVEY.md 8d."""
    d = out.astype(np.float64) - ref.astype(np.float64)
    return float(np.abs(d).max() / np.abs(ref).max()), float(np.linalg.norm(d) / np.linalg.norm(ref))


def load_c128_case():
    """The complex128 fixture (tests/golden/make_golden.py, case v): (fixture, coords, K complex128 rebuilt with the oracle)."""
    fx = np.load(GOLDEN / "apply_c128_n64.npz")
    h, w, n = (int(v) for v in fx["meta"])
    coords = [tuple(int(v) for v in t) for t in fx["coords"]]
    src, tgt = make_psfs("coma", coords, n, h, w)
    k = orc.construct_transfer(orc.psf_fft(src), orc.psf_fft(tgt), float(fx["alpha"]), float(fx["eps"]))
    assert k.dtype == np.complex128 and sha(k) == str(fx["k_sha256"]), "oracle construct differs from the reference (complex128 case)"
    return fx, coords, k


# ---- local parity: error measured against what a pixel's own patches carry, not against the brightest thing in the frame ---------
#: a result passes if its local error is at most MARGIN x the local error of the float32 yardstick on the same inputs.  The kernels use
#: radix-2 / split-radix networks, their own twiddle and window tables and another add order than pocketfft, and the GPU contracts to FMA;
#: the CPU emulators measure 0.73 ... 1.74 x and the kernels on an MI355X 0.65 ... 1.52 x (tests/test_gpu_local_parity.py), so 4 x leaves
#: a factor of 2.3 for those differences.
MARGIN = 4.0
DIM = 1e-3  # a pixel is "dim" when its local scale is at most this fraction of the frame's largest
KERNEL_PAD_MODES = ("constant", "symmetric", "reflect", "edge", "wrap")  # the np.pad modes the kernels evaluate themselves


def per_patch_reference(image, coords, k, pad_mode="symmetric", dtype=np.float64):
    """The steps of ``orc.apply_transfer`` without its saturation branch (np.pad by 2 N, sine window, scipy.fft.fft2, x K, real part of
    ifft2, window, add patch by patch in list order, crop), carried out in ``dtype``.

    float64: returns (result, local scale), the scale at a pixel being the sum over the patches that cover it of max|patch result after
    the second window|; the result is asserted equal to the pinned oracle to rounding.  float32 (K as complex64, scipy.fft stays in single
    precision): returns (result, None) - the yardstick, what a plain float32 implementation of the reference achieves on these inputs."""
    import scipy.fft

    dtype = np.dtype(dtype)
    cdtype = np.dtype(np.complex128 if dtype == np.float64 else np.complex64)
    n0, n1 = k.shape[1], k.shape[2]
    kk = np.asarray(k).astype(cdtype, copy=False)
    padded = np.pad(np.asarray(image).astype(dtype), ((2 * n0, 2 * n0), (2 * n1, 2 * n1)), mode=pad_mode)
    window = orc.apodization_window(n0, n1).astype(dtype)
    rows = np.array([c[0] for c in coords]) + 2 * n0
    cols = np.array([c[1] for c in coords]) + 2 * n1
    patches = np.stack([padded[r : r + n0, c : c + n1] for r, c in zip(rows, cols)])
    spectra = scipy.fft.fft2(window * patches)
    assert spectra.dtype == cdtype, spectra.dtype
    patches = np.real(scipy.fft.ifft2(spectra * kk)) * window
    assert patches.dtype == dtype, patches.dtype
    recon = np.zeros_like(padded)
    scale = np.zeros_like(padded) if dtype == np.float64 else None
    with np.errstate(invalid="ignore"):
        peaks = np.abs(patches).max(axis=(1, 2))
    for r, c, patch, peak in zip(rows, cols, patches, peaks):
        recon[r : r + n0, c : c + n1] += patch
        if scale is not None:
            scale[r : r + n0, c : c + n1] += peak
    crop = (slice(2 * n0, image.shape[0] + 2 * n0), slice(2 * n1, image.shape[1] + 2 * n1))
    result = recon[crop]
    if scale is None:
        return result, None
    pinned = orc.apply_transfer(image, coords, k, pad_mode=pad_mode)
    good = np.isfinite(pinned)
    assert np.array_equal(good, np.isfinite(result))
    assert np.abs(result[good] - pinned[good]).max() <= 1e-12 * np.abs(pinned[good]).max(), "per_patch_reference drifted from the oracle"
    return result, scale[crop]


def local_error(out, ref, scale) -> float:
    """max |out - ref| / scale over the pixels where the reference is finite (and some patch contributes)."""
    good = np.isfinite(ref) & np.isfinite(scale) & (scale > 0)
    d = np.abs(np.asarray(out, np.float64)[good] - ref[good]) / scale[good]
    return float(d.max()) if np.isfinite(d).all() else float("inf")


def dim_share(scale, dim=DIM) -> float:
    """Share of the pixels whose local scale is at most ``dim`` x the frame's largest."""
    good = np.isfinite(scale)
    return float(np.count_nonzero(scale[good] <= dim * scale[good].max()) / scale.size)


def hdr_frame(shape, n, seed, decades=6):
    """A frame whose amplitude steps through ``decades`` decades: 10**k, k a random integer in [-decades/2, decades/2], constant on blocks
    of 2 N x 2 N pixels, times (standard normal + 2); float32."""
    rng = np.random.default_rng(seed)
    h, w = shape
    block = 2 * n
    half = decades // 2
    exps = rng.integers(-half, half + 1, size=(-(-h // block), -(-w // block)))
    amp = np.kron(10.0 ** exps, np.ones((block, block)))[:h, :w]
    return (amp * (rng.standard_normal(shape) + 2)).astype(np.float32)


def random_transfer(shape, n, seed):
    """(corner list of the covering, random complex64 K) for a frame shape."""
    rng = np.random.default_rng(seed)
    coords = [tuple(int(v) for v in c) for c in orc.calculate_covering(shape, n)]
    k = (rng.standard_normal((len(coords), n, n)) + 1j * rng.standard_normal((len(coords), n, n))).astype(np.complex64)
    return coords, k


class LocalCase:
    """One HDR case with everything the local bound needs, computed once: frame, corners, K, float64 oracle, local scale, the yardstick's
    local error.  ``check(out)`` returns (ratio to the yardstick, local error) after asserting the bound."""

    def __init__(self, shape, n, seed, pad_mode="symmetric", image=None, coords=None, k=None, dim=DIM, min_share=0.10, yardstick_k=None):
        """``yardstick_k``: the K the float32 yardstick applies, where it is not ``k`` rounded to complex64 (a chain test: ``k`` is the
        K of the chain done in float64, ``yardstick_k`` what the reference's own float32 chain makes of the same samples)."""
        self.shape, self.n, self.pad_mode = tuple(shape), n, pad_mode
        if coords is None:
            coords, k = random_transfer(shape, n, seed + 1000)
        self.coords, self.k = coords, k
        self.image = hdr_frame(shape, n, seed) if image is None else image
        self.ref, self.scale = per_patch_reference(self.image, coords, k, pad_mode, np.float64)
        self.share = dim_share(self.scale, dim)
        assert self.share >= min_share, f"only {self.share:.2f} of the pixels are dim: the case proves nothing ({shape}, N={n}, seed {seed}, {pad_mode})"
        yard, _ = per_patch_reference(self.image, coords, k if yardstick_k is None else yardstick_k, pad_mode, np.float32)
        self.yardstick = local_error(yard, self.ref, self.scale)
        assert 0 < self.yardstick < 1e-6, self.yardstick  # float32 rounding, nothing else

    def ratio(self, out) -> float:
        return local_error(out, self.ref, self.scale) / self.yardstick

    def check(self, out, margin=MARGIN, what=""):
        assert out.shape == self.ref.shape
        ratio = self.ratio(out)
        assert ratio <= margin, f"{what}: local error {ratio:.2f} x the float32 yardstick ({self.yardstick:.2e}), margin {margin}"
        return ratio


# ---- construct parity: what makes K (PSF samples -> spectra -> transfer kernel) judged per PSF and per frequency bin ------------------------
PSF_KINDS = ("gauss", "coma", "normal", "delta", "constant")


def psf_cube(n, count, seed, kinds=PSF_KINDS):
    """(float32 cube, kind of every PSF): cycles through narrow Gaussians (sigma 0.6 ... 0.9, unit sum), orc.coma_psf somewhere on a frame of
    8 N x 8 N pixels, standard-normal samples, a single 1 at a random pixel, a constant; each PSF times 10**k, k a seeded integer in [-3, 3]."""
    rng = np.random.default_rng(seed)
    frame = 8 * n
    cube = np.empty((count, n, n), np.float32)
    names = []
    for i in range(count):
        kind = kinds[i % len(kinds)]
        if kind == "gauss":
            p = orc.gaussian_psf(n, float(rng.uniform(0.6, 0.9)))
        elif kind == "coma":
            r, c = (int(v) for v in rng.integers(-n // 2, frame - n // 2, 2))
            p = orc.coma_psf(n, r, c, frame, frame)
        elif kind == "normal":
            p = rng.standard_normal((n, n))
        elif kind == "delta":
            p = np.zeros((n, n))
            p[tuple(rng.integers(0, n, 2))] = 1.0
        else:
            p = np.ones((n, n))
        cube[i] = p * 10.0 ** rng.integers(-3, 4)
        names.append(kind)
    return cube, names


def spectrum_errors(got, truth):
    """Per PSF: max over bins |got - truth| / max over bins |truth| - every PSF against its OWN peak."""
    d = np.abs(np.asarray(got).astype(np.complex128) - truth).max(axis=(1, 2))
    return d / np.abs(truth).max(axis=(1, 2))


def dim_psf_share(truth, dim=DIM):
    """Share of the PSFs whose spectral peak is at most ``dim`` x the largest of the cube."""
    peaks = np.abs(truth).max(axis=(1, 2))
    return float(np.count_nonzero(peaks <= dim * peaks.max()) / peaks.size)


def broadband_psfs(n, coords):
    """Per patch a Gaussian core (sigma 0.6 ... 0.9) plus a weak displaced blob, unit sum, float32: spectra without a noise floor
    (min|S| / max|S| ~ 2e-3), so that the reference's own float32 chain samples -> spectra -> K is well-conditioned."""
    x = np.arange(n) - n // 2
    out = []
    for r, c in coords:
        s = 0.6 + 0.3 * ((r + c) % 7) / 7
        d = 1 + ((r * 3 + c) % 5) / 3
        p = np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2 * s * s)) + 0.2 * np.exp(-((x[:, None] - d) ** 2 + (x[None, :] + d / 2) ** 2) / 2.0)
        out.append(p / p.sum())
    return np.stack(out).astype(np.float32)


CONSTRUCT_ALPHAS = (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 7.0)
CONSTRUCT_EPSILONS = (1.0, 0.1, 1e-3)
CONSTRUCT_SIZES = (32, 64, 256)
#: source / target pairs of the K2 cases: the suite's coma and Gaussian pairs, the chain's broadband PSFs, and the coma sources against the
#: Gaussians and comas of psf_cube (amplitudes 1e-3 ... 1e3, so that |T| and |S| are decades apart)
CONSTRUCT_INPUTS = ("coma", "gauss", "broadband", "scaled")
RANGE_F32 = (2.0 ** -120, 2.0 ** 120)  # a normal float32 number with room to spare
RANGE_F64 = (2.0 ** -1000, 2.0 ** 1000)
#: what a same-precision evaluation of the formula may err by per in-range bin, in units of the format's epsilon, for a case to count as
#: "rounding and nothing else" in double: |S| and eps |T| carry up to 1.5 epsilon each (hypot within an ulp, one product) and enter to
#: the power alpha + 1 <= 8, 2 x 8 x 1.5 = 24, plus half an epsilon for each of the remaining dozen operations.  (In float32 the bound
#: is the 2e-6 = 17 epsilon that the cases were chosen by.)
YARDSTICK_EPSILONS_F64 = 32.0


def pow_branch(e):
    """The branch of the kernels' np_pow that an exponent takes (rpsf_kernels.hpp)."""
    fast = {0.0: "1", 1.0: "x", 2.0: "x*x", 0.5: "sqrt", -1.0: "1/x"}
    return fast.get(e, "float64 product" if e in (3.0, 4.0, 5.0, 6.0, 8.0) else "pow")


def pow_branches(alpha, double=False):
    """'branch of alpha - 1 / branch of alpha + 1' (the double kernel has no product branch: its 3 ... 8 go to pow)."""
    names = [pow_branch(alpha - 1), pow_branch(alpha + 1)]
    return " / ".join("pow" if double and b == "float64 product" else b for b in names)


def construct_samples(kind, n, count=None):
    """(source, target) float32 samples of one K2 input kind; two patch rows of a covering by default (a handful of PSFs at every N)."""
    shape = (n, 3 * n)
    coords = [tuple(int(v) for v in c) for c in orc.calculate_covering(shape, n)]
    if count is not None:
        rows = -(-count // 4)
        shape = (n * rows, 2 * n)
        coords = [tuple(int(v) for v in c) for c in orc.calculate_covering(shape, n)][:count]
        assert len(coords) == count
    if kind in ("coma", "gauss"):
        src, tgt = make_psfs(kind, coords, n, *shape)
    elif kind == "broadband":
        src = broadband_psfs(n, coords)
        tgt = np.broadcast_to(orc.gaussian_psf(n, 0.9), src.shape)
    else:
        src = make_psfs("coma", coords, n, *shape)[0]
        tgt = psf_cube(n, len(coords), n, kinds=PSF_KINDS[:2])[0]
    return np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)


def construct_spectra(kind, n, dtype=np.complex64, count=None):
    """The spectra a K2 case reads: scipy.fft.fft2 of the float32 samples (complex64, noise bins included), or of the same samples promoted
    to float64 (complex128) for the double kernel."""
    import scipy.fft

    src, tgt = construct_samples(kind, n, count)
    real = np.float32 if np.dtype(dtype) == np.complex64 else np.float64
    s, t = scipy.fft.fft2(src.astype(real)), scipy.fft.fft2(tgt.astype(real))
    assert s.dtype == t.dtype == np.dtype(dtype)
    return s, t


def transfer_terms(s, t, alpha, eps):
    """(K, every real quantity orc.construct_transfer forms on the way), in the precision of ``s`` and ``t``: the oracle's expressions one by
    one, so K is its K bit for bit (tests/test_construct_cases.py asserts that)."""
    with np.errstate(all="ignore"):
        sabs, tabs = abs(s), abs(t)
        p1, p2, p3 = sabs ** (alpha - 1), sabs ** (alpha + 1), (eps * tabs) ** (alpha + 1)
        num = s.conjugate() * p1
        den = p2 + p3
        quo = num / den
        k = quo * t
        return k, (sabs, tabs, p1, p2, p3, abs(num), den, abs(quo), abs(k))


def in_range_bins(s, t, alpha, eps, bounds=RANGE_F32):
    """(truth K, mask, zero mask).  mask: the bins where every quantity of the formula, evaluated in the precision of ``s`` / ``t`` (the
    truth's), is finite and inside ``bounds`` - where the kernel's number format neither underflows nor overflows, so that a few ulp per
    bin is owed.  zero mask: the bins where the truth is exactly 0 (S or T is) with the denominator in range and every other quantity
    exactly 0 or in range - nothing underflows in the kernel's format on the way there either, so K has to be exactly 0.  (Where, say,
    |S|**8 underflows in float32 beside a T of 0, the reference's own complex64 evaluation gives 0 / 0 = NaN.)"""
    k, terms = transfer_terms(s, t, alpha, eps)
    with np.errstate(invalid="ignore"):
        mask = np.ones(s.shape, bool)
        zero = (k == 0)
        for i, q in enumerate(terms):
            inside = np.isfinite(q) & (q >= bounds[0]) & (q <= bounds[1])
            mask &= inside
            zero &= inside if i == 6 else inside | (q == 0)
    return k, mask, zero


def bin_error(k, truth, mask) -> float:
    """max over the bins of ``mask`` of |k - truth| / |truth|."""
    d = np.abs(np.asarray(k)[mask].astype(truth.dtype) - truth[mask]) / np.abs(truth[mask])
    return float(d.max()) if np.isfinite(d).all() else float("inf")


class TransferCase:
    """One K2 case: spectra, truth (orc.construct_transfer one precision up), in-range bins, yardstick (orc.construct_transfer evaluated by NumPy
    in the kernel's precision on the same arrays, same bins)."""

    def __init__(self, s, t, alpha, eps, wide=None, label=""):
        self.s, self.t, self.alpha, self.eps, self.label = s, t, alpha, eps, label
        double = s.dtype == np.complex128
        wide = wide or (np.clongdouble if double else np.complex128)
        self.truth, self.mask, self.zero = in_range_bins(s.astype(wide), np.broadcast_to(t, s.shape).astype(wide), alpha, eps, RANGE_F64 if double else RANGE_F32)
        self.share = float(self.mask.mean())
        with np.errstate(all="ignore"):
            self.same_precision = orc.construct_transfer(s, np.broadcast_to(t, s.shape), alpha, eps)
        assert self.same_precision.dtype == s.dtype
        self.yardstick = bin_error(self.same_precision, self.truth, self.mask) if self.mask.any() else float("nan")

    def decades(self) -> float:
        mag = np.abs(self.truth[self.mask]).astype(np.float64)
        return float(np.log10(mag.max() / mag.min()))

    def ratio(self, k) -> float:
        return bin_error(k, self.truth, self.mask) / self.yardstick

    def check(self, k, margin=MARGIN, what=""):
        """The per-bin bound on the in-range bins; exact zeros (in_range_bins); and the non-finite pattern where the truth itself is not finite."""
        assert k.shape == self.truth.shape and k.dtype == self.s.dtype
        ratio = self.ratio(k)
        assert ratio <= margin, f"{what} {self.label}: per-bin error {ratio:.2f} x the same-precision yardstick ({self.yardstick:.2e}), margin {margin}"
        assert np.array_equal(k[self.zero], np.zeros(int(self.zero.sum()), k.dtype)), f"{what} {self.label}: a bin that is exactly 0 is not"
        for part in (np.real, np.imag):
            bad = ~np.isfinite(part(self.truth))
            got, want = part(k)[bad], part(self.same_precision)[bad]
            assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what} {self.label}: NaN pattern where the truth is not finite"
            inf = np.isinf(want)
            assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), f"{what} {self.label}: Inf pattern"
        return ratio


# (N, shape, HDR seed) of the chain cases: shapes and seeds of tests/test_gpu_local_parity.py, so that the launch forms are the ones labelled there
CHAIN_CASES = [(32, (130, 203), 32), (64, (333, 390), 64), (128, (520, 640), 129), (256, (520, 768), 272), (24, (100, 130), 24)]
CHAIN_PARAMETERS = [(3.0, 0.1), (1.0, 0.05)]


def chain_samples(n, shape):
    """(corner list of the covering, broadband source samples, Gaussian 0.9 target samples), float32."""
    coords = [tuple(int(v) for v in c) for c in orc.calculate_covering(shape, n)]
    src = broadband_psfs(n, coords)
    tgt = np.ascontiguousarray(np.broadcast_to(orc.gaussian_psf(n, 0.9).astype(np.float32), src.shape))
    return coords, src, tgt


def chain_transfer(src, tgt, alpha, eps, real):
    """The reference's chain samples -> spectra -> K carried out in ``real`` (float64: the truth; float32: the yardstick, scipy.fft and NumPy
    stay in single precision)."""
    import scipy.fft

    s, t = scipy.fft.fft2(src.astype(real)), scipy.fft.fft2(tgt.astype(real))
    k = orc.construct_transfer(s, t, alpha, eps)
    assert k.dtype == (np.complex128 if np.dtype(real) == np.float64 else np.complex64)
    return s, k


def chain_case(n, shape, seed, alpha, eps, image=None, min_share=0.10):
    """LocalCase whose truth is the whole chain in float64 and whose yardstick is the whole chain in float32; also returns the float32 samples."""
    coords, src, tgt = chain_samples(n, shape)
    k64 = chain_transfer(src, tgt, alpha, eps, np.float64)[1]
    k32 = chain_transfer(src, tgt, alpha, eps, np.float32)[1]
    case = LocalCase(shape, n, seed, "symmetric", image=image, coords=coords, k=k64, yardstick_k=k32, min_share=min_share)
    return case, src, tgt
