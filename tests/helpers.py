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

    def __init__(self, shape, n, seed, pad_mode="symmetric", image=None, coords=None, k=None, dim=DIM, min_share=0.10):
        self.shape, self.n, self.pad_mode = tuple(shape), n, pad_mode
        if coords is None:
            coords, k = random_transfer(shape, n, seed + 1000)
        self.coords, self.k = coords, k
        self.image = hdr_frame(shape, n, seed) if image is None else image
        self.ref, self.scale = per_patch_reference(self.image, coords, k, pad_mode, np.float64)
        self.share = dim_share(self.scale, dim)
        assert self.share >= min_share, f"only {self.share:.2f} of the pixels are dim: the case proves nothing ({shape}, N={n}, seed {seed}, {pad_mode})"
        yard, _ = per_patch_reference(self.image, coords, k, pad_mode, np.float32)
        self.yardstick = local_error(yard, self.ref, self.scale)
        assert 0 < self.yardstick < 1e-6, self.yardstick  # float32 rounding, nothing else

    def ratio(self, out) -> float:
        return local_error(out, self.ref, self.scale) / self.yardstick

    def check(self, out, margin=MARGIN, what=""):
        assert out.shape == self.ref.shape
        ratio = self.ratio(out)
        assert ratio <= margin, f"{what}: local error {ratio:.2f} x the float32 yardstick ({self.yardstick:.2e}), margin {margin}"
        return ratio
