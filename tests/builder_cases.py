"""Seeded star-field frames for the PSF-builder tests and their golden generator (tests/golden/make_builder_golden.py).

The fixtures store seeds and star positions, not frames: both sides regenerate the frames here.  Every frame is rounded to
float32 before anybody sees it (the reference included), so input rounding drops out of every comparison.
"""

from __future__ import annotations

import functools
import pathlib

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
METHODS = (("mean", 50.0), ("median", 50.0), ("percentile", 30.0))

# name: frame shape, patch size, frames, random stars per frame, options
#   edge:       frame 0 also gets stars within half a pixel of every edge and corner, and two whose corner is k + 0.5 (round half to even)
#   zero / nan: frame 1 gets one exact-zero pixel, the last frame one NaN pixel, each inside the patch of a star
#   rows:       stars are drawn from these rows only, which leaves covering cells without any star
#   thresholds: finite saturation_threshold, star_minimum, star_maximum
CASES = {
    "n16": {"shape": (96, 80), "n": 16, "frames": 3, "stars": 30, "edge": True, "zero": True, "nan": True},
    "n15": {"shape": (50, 44), "n": 15, "frames": 2, "stars": 14, "thresholds": (330.0, 90.0, 300.0)},
    "n32": {"shape": (128, 96), "n": 32, "frames": 2, "stars": 12, "rows": (0, 56), "thresholds": (360.0, 70.0, 330.0)},
}


def thresholds(name: str) -> dict:
    t = CASES[name].get("thresholds")
    return {} if t is None else {"saturation_threshold": t[0], "star_minimum": t[1], "star_maximum": t[2]}


def star_frame(shape: tuple[int, int], pos: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    """The recipe of every frame here: a tilted background, noise, and one Gaussian star of sigma 1.1 ... 1.5 per position (float64)."""
    h, w = shape
    rows, cols = np.mgrid[0:h, 0:w].astype(np.float64)
    amp = rng.uniform(60, 400, len(pos))
    sig_r, sig_c = rng.uniform(1.1, 1.5, len(pos)), rng.uniform(1.1, 1.5, len(pos))
    frame = 10.0 + 0.03 * rows - 0.02 * cols + rng.normal(0.0, 0.3, (h, w))
    for (r, c), a, sr, sc in zip(pos, amp, sig_r, sig_c):
        frame += a * np.exp(-0.5 * (((rows - r) / sr) ** 2 + ((cols - c) / sc) ** 2))
    return frame


def make_case(name: str, seed: int) -> tuple[np.ndarray, list[np.ndarray]]:
    """(frames, stars): frames (F, H, W) float64 holding float32 values; stars[f] (k, 2) float64 (row, col)."""
    case = CASES[name]
    (h, w), n = case["shape"], case["n"]
    frames, stars = [], []
    for f in range(case["frames"]):
        rng = np.random.default_rng([seed, f])
        lo, hi = case.get("rows", (0, h))
        k = case["stars"]
        pos = np.stack([rng.uniform(lo, hi - 1, k), rng.uniform(0, w - 1, k)], axis=-1)
        if case.get("edge") and f == 0:
            extra = [(0.3, 0.2), (0.4, w - 0.6), (h - 0.7, 0.1), (h - 0.6, w - 0.7), (0.2, w / 2 + 0.37), (h - 0.55, w / 3 + 0.21),
                     (h / 2 + 0.13, 0.45), (h / 2 - 3.3, w - 0.8), (20.5, 30.25), (41.5, 52.5)]
            pos = np.concatenate([pos, np.array(extra)])
        frame = star_frame((h, w), pos, rng)
        if case.get("zero") and f == 1:
            r, c = np.rint(pos[0]).astype(int)
            frame[min(r + 3, h - 1), max(c - 2, 0)] = 0.0
        if case.get("nan") and f == case["frames"] - 1:
            r, c = np.rint(pos[1]).astype(int)
            frame[max(r - 4, 0), min(c + 3, w - 1)] = np.nan
        frames.append(frame.astype(np.float32).astype(np.float64))
        stars.append(pos)
    return np.stack(frames), stars


@functools.lru_cache(maxsize=None)
def load(name: str) -> dict:
    """Everything the generator stored for a case, plus the regenerated frames (shared between the tests; do not modify)."""
    base = dict(np.load(GOLDEN / f"builder_{name}.npz"))
    frames, stars = make_case(name, int(base["seed"]))
    split = np.cumsum(base["stars_per_frame"])[:-1]
    stored = np.split(base["stars"], split)
    assert all(np.array_equal(a, b) for a, b in zip(stars, stored)), "the frame generator no longer reproduces the fixture"
    out = {**base, "frames": frames, "stars": stars, "n": CASES[name]["n"]}  # stars: per frame, as make_case returns them
    for method, _ in METHODS:
        per = np.load(GOLDEN / f"builder_{name}_{method}.npz")
        out.update({f"{key}_{method}": per[key] for key in per.files})
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return out


@functools.cache
def emulator():
    """tests/emu/libemu_builder.so: the kernels' per-thread phases on the CPU.  __graft_entry__.build() compiles it; like the emulators
    of tests/test_emulator.py it is compiled here when it is missing or older than its sources, so the tests do not hang on a build
    product under tests/.  Without a compiler that is an error, not a skip."""
    import ctypes
    import os
    import shutil
    import subprocess

    root = pathlib.Path(__file__).resolve().parent.parent
    src, out = root / "tests" / "emu" / "emu_builder.cpp", root / "tests" / "emu" / "libemu_builder.so"
    core = root / "regularizepsf_amd" / "csrc" / "rpsf_core_builder.hpp"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, core.stat().st_mtime):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++") or shutil.which("hipcc")
        assert clang is not None, "no clang++ to build tests/emu/emu_builder.cpp"
        fresh = out.with_name(f"libemu_builder.{os.getpid()}.so")  # written aside and moved into place: test processes may run side by side
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(fresh), str(src)], check=True)
        os.replace(fresh, out)
    lib = ctypes.CDLL(str(out))
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emub_patches.argtypes = [i, vp, i, i, i, vp, vp, d, d, d, vp, vp]
    lib.emub_average.argtypes = [vp, i, i, d, i, vp, vp, vp]
    return lib


def emu_patches(frame: np.ndarray, n: int, rounded: np.ndarray, shift: np.ndarray, saturation_threshold: float = np.inf,
                star_minimum: float = 0.0, star_maximum: float = np.inf) -> tuple[np.ndarray, np.ndarray]:
    """Kernel B1 on the emulator: (float32 patches of every star, flags)."""
    img = np.ascontiguousarray(frame, np.float32)
    corners = np.ascontiguousarray(rounded, np.int32)
    frac = np.ascontiguousarray(shift, np.float64)
    patches = np.full((len(corners), n, n), np.nan, np.float32)
    flags = np.zeros(len(corners), np.uint8)
    rc = emulator().emub_patches(n, img.ctypes.data, img.shape[0], img.shape[1], len(corners), corners.ctypes.data, frac.ctypes.data,
                                 saturation_threshold, star_minimum, star_maximum, patches.ctypes.data, flags.ctypes.data)
    assert rc == 0
    return patches, flags


def emu_average(stack: np.ndarray, method: int, percentile: float, offsets: np.ndarray, members: np.ndarray) -> np.ndarray:
    """Kernel B2 on the emulator."""
    stack = np.ascontiguousarray(stack, np.float32)
    offsets, members = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(members, np.int32)
    n = stack.shape[-1]
    cells = np.empty((len(offsets) - 1, n, n), np.float64)
    assert emulator().emub_average(stack.ctypes.data, n, method, percentile, len(offsets) - 1, offsets.ctypes.data, members.ctypes.data,
                                   cells.ctypes.data) == 0
    return cells


AVERAGE_COUNTS = (1, 2, 3, 64, 65, 257, 2500)  # members per cell; an empty cell is appended
AVERAGE_PERCENTILES = (30.0, 99.9)


@functools.lru_cache(maxsize=None)
def average_case() -> dict:
    """A seeded float32 stack of 2500 16 x 16 patches, one cell per member count (members in a shuffled order: the mean's additions
    follow it), and what NumPy gives for the same samples in float64 - computed once, shared by the emulator and the GPU test."""
    import warnings

    n, total = 16, max(AVERAGE_COUNTS)
    rng = np.random.default_rng(2500)
    stack = (rng.normal(0.0, 0.05, (total, n, n)) + 0.2 * rng.random((total, 1, 1))).astype(np.float32)
    stack[:, n // 2, n // 2] = rng.uniform(0.5, 2.0, total).astype(np.float32)
    lists = [rng.permutation(total)[:m].astype(np.int32) for m in AVERAGE_COUNTS] + [np.zeros(0, np.int32)]
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int64)
    wide = stack.astype(np.float64)
    expected = {"mean": [], "median": [], **{q: [] for q in AVERAGE_PERCENTILES}}
    for members in lists:
        if len(members) == 0:
            for v in expected.values():
                v.append(np.zeros((n, n)))
            continue
        samples = [wide[j] / wide[j, n // 2, n // 2] for j in members]
        acc = np.zeros((n, n))
        for s in samples:  # the reference's accumulation, builder.py:66
            acc = np.nansum([acc, s], axis=0)
        expected["mean"].append(acc / np.full((n, n), float(len(samples))))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            expected["median"].append(np.nanmedian(samples, axis=0))
            for q in AVERAGE_PERCENTILES:
                expected[q].append(np.nanpercentile(samples, q, axis=0))
    out = {"stack": stack, "offsets": offsets, "members": np.concatenate(lists), **{k: np.stack(v) for k, v in expected.items()}}
    for v in out.values():
        v.flags.writeable = False
    return out


def check_average(got: dict) -> None:
    """The criteria of the averaging test: mean and median bit for bit, percentiles within 1e-12 relative (one float64 lerp, for
    which NumPy switches formula at t >= 0.5: an ulp or two)."""
    want = average_case()
    for key in ("mean", "median"):
        assert got[key].dtype == np.float64
        assert np.array_equal(got[key].view(np.int64), want[key].view(np.int64)), f"{key} is not bit-identical to NumPy"
    for q in AVERAGE_PERCENTILES:
        err = np.abs(got[q] - want[q]).max(axis=(1, 2))
        scale = np.abs(want[q]).max(axis=(1, 2))
        print(f"percentile {q}: max relative error per cell {err / np.maximum(scale, 1e-300)}")
        assert np.all(err <= 1e-12 * scale)


def bowl_frame(shape: tuple[int, int], centre: tuple[float, float]) -> np.ndarray:
    """A frame whose 'star' is the minimum of a bowl: no border pixel of its patch lies below the patch centre."""
    rows, cols = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    return (1.0 + (rows - centre[0]) ** 2 + (cols - centre[1]) ** 2).astype(np.float32)


# ---------------------------------------------------------------------------------------- every patch-size path against float64 SciPy
# The fixtures above stop at N = 32.  The cases below need none: their reference is a float64 restatement of the per-star and per-cell
# stages with NumPy and SciPy calls only (np.pad, scipy.ndimage.shift, builder.background_plane, np.median, np.percentile), computed
# once per case and shared between the emulator tests (tests/test_builder_host.py) and the GPU tests (tests/test_gpu_builder_sizes.py).
TOL = 1e-5  # the project's parity bound, per patch and per cell

# name: patch size, frame shape, frames, seed, thresholds (saturation_threshold, star_minimum, star_maximum) or None.
# Every frame carries 5 random stars, one star within half a pixel of each of two opposite corners, of a row edge and of a column edge,
# and one whose corner is k + 0.5 on both axes (k even on the rows: rounds down, shift -1; odd on the columns: rounds up, shift 0;
# at N = 5 odd on both, see size_stars).  No corner is an exact integer (shift -0.5): at N = 4 the mirror would make ring pixel (3, 2)
# equal to the centre.
# The seed is the first from 1 on for which well_posed() holds for every star; the thresholds were read off the oracle's centres.
SIZE_CASES = {
    "n4": {"n": 4, "shape": (9, 7), "frames": 1, "seed": 2},  # smallest size: 8 table threads
    "n5": {"n": 5, "shape": (11, 8), "frames": 1, "seed": 1},  # smallest odd size
    "n16": {"n": 16, "shape": (40, 36), "frames": 1, "seed": 1},  # one pixel per thread (the isolation tests' small size)
    "n33": {"n": 33, "shape": (70, 61), "frames": 2, "seed": 1},  # 5 pixels per thread with a ragged last pass, odd pitch equal to N
    "n63": {"n": 63, "shape": (130, 100), "frames": 1, "seed": 1},  # odd size just below the 256-thread limit
    "n64": {"n": 64, "shape": (130, 100), "frames": 2, "seed": 1, "thresholds": (350.0, 70.0, 300.0)},  # 16 pixels per thread at 256
    "n65": {"n": 65, "shape": (140, 131), "frames": 1, "seed": 1},  # first 1024-thread launch
    "n127": {"n": 127, "shape": (140, 131), "frames": 1, "seed": 1},  # odd size just below the maximum
    "n128": {"n": 128, "shape": (140, 131), "frames": 2, "seed": 1, "thresholds": (390.0, 70.0, 330.0)},  # 16 per thread at 1024, 141 KiB
    "n32_small": {"n": 32, "shape": (20, 24), "frames": 1, "seed": 1},  # frame smaller than the patch: the mirror map wraps
    "n128_small": {"n": 128, "shape": (50, 40), "frames": 1, "seed": 1},  # ... more than once
}
END_TO_END = ("n33", "n64", "n128")  # frames -> cells


def size_thresholds(name: str) -> tuple[float, float, float]:
    t = SIZE_CASES[name].get("thresholds")
    return (np.inf, 0.0, np.inf) if t is None else t


def size_stars(shape: tuple[int, int], n: int, rng: np.random.Generator, random: int = 5) -> np.ndarray:
    h, w = shape
    pos = np.stack([rng.uniform(0, h - 1, random), rng.uniform(0, w - 1, random)], axis=-1)
    # a shift of -1 makes line N - 1 of the shifted patch a copy of line N - 3 (the mirror), which is the centre line at N = 5 and 6:
    # a ring pixel would equal the centre and rounding would decide the fit mask, so there both corners round up
    k_row = 2 * np.floor((h / 3 - n / 2) / 2) + (n in (5, 6))
    k_col = 2 * np.floor((w / 2 - n / 2) / 2) + 1
    extra = [(0.3, 0.2), (h - 0.6, w - 0.7), (0.2, w / 2 + 0.37), (h / 2 + 0.13, 0.45), (k_row + 0.5 + n / 2, k_col + 0.5 + n / 2)]
    return np.concatenate([pos, np.array(extra)])


def make_size_case(shape: tuple[int, int], n: int, frames: int, seed: int, stars: list[np.ndarray] | None = None):
    """make_case's recipe for any shape, patch size and star list: (frames (F, H, W) float64 holding float32 values, stars per frame)."""
    out_frames, out_stars = [], []
    for f in range(frames):
        rng = np.random.default_rng([seed, n, f])
        pos = size_stars(shape, n, rng) if stars is None else np.asarray(stars[f], np.float64).reshape(-1, 2)
        out_frames.append(star_frame(shape, pos, rng).astype(np.float32).astype(np.float64))
        out_stars.append(pos)
    return np.stack(out_frames), out_stars


def _oracle_star(padded: np.ndarray, n: int, corner: np.ndarray, shift: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """One star in float64: (the patch shifted onto the pixel grid, the same minus its background plane with NaN where it was zero)."""
    from scipy.ndimage import shift as spline_shift

    from regularizepsf_amd import builder as bld

    r, c = int(corner[0]) + n, int(corner[1]) + n
    shifted = spline_shift(padded[r:r + n, c:c + n], shift=tuple(shift), mode="mirror")
    with np.errstate(invalid="ignore"):
        patch = shifted - bld.background_plane(shifted)
    patch[shifted == 0] = np.nan
    return shifted, patch


def _oracle_frame(frame, n, rounded, shift):
    padded = np.pad(np.asarray(frame, np.float64), n, mode="reflect")
    pairs = [_oracle_star(padded, n, corner, amount) for corner, amount in zip(np.asarray(rounded).reshape(-1, 2), np.asarray(shift).reshape(-1, 2))]
    if not pairs:
        return np.zeros((0, n, n)), np.zeros((0, n, n))
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _oracle_flags(patches: np.ndarray, saturation: float, minimum: float, maximum: float) -> np.ndarray:
    n = patches.shape[-1]
    with np.errstate(invalid="ignore"):
        centre = patches[:, n // 2, n // 2]
        return (np.all(patches < saturation, axis=(1, 2)) & (centre > minimum) & (centre < maximum)).astype(np.uint8)


def oracle_patches(frame: np.ndarray, n: int, rounded: np.ndarray, shift: np.ndarray, saturation: float = np.inf, minimum: float = 0.0,
                   maximum: float = np.inf) -> tuple[np.ndarray, np.ndarray]:
    """Kernel B1's job in float64 with NumPy and SciPy: (patches of every star, float64, NaN where the shifted patch is zero; flags,
    1 where all three accept tests pass and 0 otherwise)."""
    _, patches = _oracle_frame(frame, n, rounded, shift)
    return patches, _oracle_flags(patches, saturation, minimum, maximum)


def oracle_cells(patches: np.ndarray, offsets: np.ndarray, members: np.ndarray, method: str, q: float = 50.0) -> np.ndarray:
    """Kernel B2's job with NumPy: per cell the samples patch / patch[centre] of its members; the mean as a running sum in list order
    divided by the count, np.median, np.percentile.  A cell without a member is all zero."""
    patches = np.asarray(patches, np.float64)
    n = patches.shape[-1]
    cells = np.zeros((len(offsets) - 1, n, n))
    for cell in range(len(offsets) - 1):
        listed = members[offsets[cell]:offsets[cell + 1]]
        if len(listed) == 0:
            continue
        samples = [patches[j] / patches[j, n // 2, n // 2] for j in listed]
        if method == "mean":
            acc = np.zeros((n, n))
            for s in samples:
                acc = acc + s
            cells[cell] = acc / float(len(samples))
        elif method == "median":
            cells[cell] = np.median(samples, axis=0)
        else:
            cells[cell] = np.percentile(samples, q, axis=0)
    return cells


def _freeze(out: dict) -> dict:
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.flags.writeable = False
    return out


def oracle_case(n: int, frames: np.ndarray, stars: list[np.ndarray], thresholds: tuple[float, float, float] = (np.inf, 0.0, np.inf)) -> dict:
    """Frames and star lists with the oracle's answer.  Lists are per frame: stars, corner (float), rounded, shift, shifted (the
    oracle's patches before the plane is subtracted), patches (after), flags."""
    from regularizepsf_amd import builder as bld

    out = {"n": n, "frames": frames, "stars": stars, "thresholds": thresholds, "finite_thresholds": bool(np.isfinite(thresholds[0])),
           "corner": [], "rounded": [], "shift": [], "shifted": [], "patches": [], "flags": []}
    for frame, pos in zip(frames, stars):
        corner, rounded, shift = bld.star_geometry(pos, n)
        shifted, patches = _oracle_frame(frame, n, rounded, shift)
        for key, value in (("corner", corner), ("rounded", rounded), ("shift", shift), ("shifted", shifted), ("patches", patches),
                           ("flags", _oracle_flags(patches, *thresholds))):
            out[key].append(value)
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def size_case(name: str) -> dict:
    """A case of SIZE_CASES with the oracle's answer (shared; do not modify)."""
    case = SIZE_CASES[name]
    frames, stars = make_size_case(case["shape"], case["n"], case["frames"], case["seed"])
    return oracle_case(case["n"], frames, stars, size_thresholds(name))


GROWTH_STARS = (3, 9, 20)  # stars per frame: every per-frame device buffer has to grow on the second and on the third frame


@functools.lru_cache(maxsize=None)
def growth_case() -> dict:
    """Three 60 x 52 frames for N = 16 with 3, 9 and 20 random stars (seed: the first from 1 on for which well_posed() holds)."""
    shape, n, seed = (60, 52), 16, 1
    rng = np.random.default_rng([seed, 3920])
    stars = [np.stack([rng.uniform(0, shape[0] - 1, k), rng.uniform(0, shape[1] - 1, k)], axis=-1) for k in GROWTH_STARS]
    frames, stars = make_size_case(shape, n, len(stars), seed, stars)
    return oracle_case(n, frames, stars)


@functools.lru_cache(maxsize=None)
def near_float32_max_case() -> dict:
    """A float32 frame for N = 16 with two neighbouring pixels of 3.3e38 and the star half-way between them: every pixel fits
    float32, the spline's value between the two does not (about 1.2 x 3.3e38), so the float64 oracle keeps the patch and the kernel,
    which stores float32, must reject it."""
    n, shape = 16, (40, 36)
    rng = np.random.default_rng(338)
    frame = (10.0 + rng.normal(0.0, 0.3, shape)).astype(np.float32)
    frame[20, 17] = frame[20, 18] = np.float32(3.3e38)
    return oracle_case(n, frame.astype(np.float64)[None], [np.array([[20.45, 17.95]])])


def well_posed(case: dict) -> None:
    """What makes a case decidable, asserted on the oracle's data alone for EVERY star of it (none is ever dropped; a case that fails
    gets another seed): no decision of the kernel may hang on a rounding.
    - the fit mask (border ring without its corners, below the centre) has at least 4 pixels, not nearly on one line:
      det / (sxx syy) = 1 - rho^2 of their centred coordinates above 1e-3;
    - no ring pixel within 1e-9 |centre| of the centre (it would be in the mask on one side and out of it on the other);
    - finite thresholds: the centre at least 1e-6 (relative) away from star_minimum and star_maximum, the patch maximum from
      saturation_threshold."""
    n = case["n"]
    saturation, minimum, maximum = case["thresholds"]
    ring = np.zeros((n, n), bool)
    ring[0, 1:-1] = ring[-1, 1:-1] = ring[1:-1, 0] = ring[1:-1, -1] = True
    rows, cols = np.indices((n, n))
    for f, (shifted, patches) in enumerate(zip(case["shifted"], case["patches"])):
        for j, (before, after) in enumerate(zip(shifted, patches)):
            where = f"frame {f} star {j}"
            assert np.isfinite(before).all() and not np.any(before == 0), where
            centre = before[n // 2, n // 2]
            assert np.all(np.abs(before[ring] - centre) > 1e-9 * abs(centre)), where
            mask = ring & (before < centre)
            assert mask.sum() >= 4, where
            dx, dy = cols[mask] - cols[mask].mean(), rows[mask] - rows[mask].mean()
            sxx, syy, sxy = (dx * dx).sum(), (dy * dy).sum(), (dx * dy).sum()
            assert sxx > 0 and syy > 0 and (sxx * syy - sxy * sxy) / (sxx * syy) > 1e-3, where
            for value, limit in ((after[n // 2, n // 2], minimum), (after[n // 2, n // 2], maximum), (after.max(), saturation)):
                if np.isfinite(limit) and limit != 0:
                    assert abs(value - limit) >= 1e-6 * abs(limit), where


def check_size_patches(name: str, got: np.ndarray, flags: np.ndarray) -> float:
    """The criteria of the per-size patch test, the same for the emulator and the GPU: `got` are the accepted float32 patches in star
    order over all frames, `flags` the flags of every star.  Returns the worst per-patch error."""
    case = size_case(name)
    want_flags = np.concatenate(case["flags"])
    assert np.array_equal(flags, want_flags)
    want = np.concatenate(case["patches"])[want_flags == 1]
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
    print(f"{name}: N = {case['n']}, frame {case['frames'].shape[1:]}, {len(want_flags)} stars, {len(want)} accepted, "
          f"max per-patch error {err.max():.3e}")
    assert np.all(err <= TOL)
    if case["finite_thresholds"]:
        assert 0 < want_flags.sum() < len(want_flags)  # the thresholds reject somebody and keep somebody
    return float(err.max())


@functools.lru_cache(maxsize=None)
def end_to_end_case(name: str) -> dict:
    """Frames -> cells of a case in float64: the oracle's accepted patches, their membership in the cells of the covering, and
    oracle_cells per method of METHODS."""
    from regularizepsf_amd import builder as bld
    from regularizepsf_amd.util import calculate_covering

    case = size_case(name)
    n = case["n"]
    keys = np.concatenate([corner[flags == 1] for corner, flags in zip(case["corner"], case["flags"])])
    patches = np.concatenate(case["patches"])[np.concatenate(case["flags"]) == 1]
    offsets, members = bld.cell_membership(keys, calculate_covering(case["frames"][0].shape, n), n)
    out = {"offsets": offsets, "members": members}
    for method, q in METHODS:
        out[method] = oracle_cells(patches, offsets, members, method, q)
    assert (np.diff(offsets) == 0).any() and (np.diff(offsets) > 1).any()  # an empty cell, and a cell that really averages
    return _freeze(out)


def check_end_to_end(name: str, average) -> None:
    """`average(method, q, offsets, members)` gives the cells of the side under test from ITS patches; per cell within TOL of the
    oracle cell's maximum, a cell without a star all zero on both sides."""
    want = end_to_end_case(name)
    empty = np.diff(want["offsets"]) == 0
    for method, q in METHODS:
        cells = average(method, q, want["offsets"], want["members"])
        assert cells.dtype == np.float64 and cells.shape == want[method].shape
        assert np.all(cells[empty] == 0) and np.all(want[method][empty] == 0)
        err = np.abs(cells - want[method]).max(axis=(1, 2))[~empty]
        scale = np.abs(want[method]).max(axis=(1, 2))[~empty]
        print(f"{name} {method}: {len(scale)} cells with stars, max per-cell error {np.max(err / scale):.3e}")
        assert np.all(err <= TOL * scale)


# ---------------------------------------------------------------------------------------------------- B2 alone: ties and sizes
TIE_COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 101, 400)
TIE_PERCENTILES = (0.0, 0.1, 12.5, 25.0, 30.0, 50.0, 66.6, 75.0, 99.9, 100.0)
B2_SIZES = (4, 5, 33, 128)  # 33: 5 blocks of 256 lanes, the last with 65 live ones; 128: 64 blocks
B2_SIZE_COUNTS = (1, 2, 5, 12)


def _b2_case(stack: np.ndarray, lists: list[np.ndarray], percentiles: tuple[float, ...]) -> dict:
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int64)
    members = np.concatenate(lists).astype(np.int32)
    out = {"stack": stack, "offsets": offsets, "members": members, "percentiles": percentiles,
           "mean": oracle_cells(stack, offsets, members, "mean"), "median": oracle_cells(stack, offsets, members, "median")}
    for q in percentiles:
        out[q] = oracle_cells(stack, offsets, members, "percentile", q)
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def tie_case() -> dict:
    """400 patches of 8 x 8 small integers (-3 ... 3 without 0: NumPy's choice between +0 and -0 is not pinned) with centres in
    {1, 2, 4, -2}: the samples come from a small exact set with both signs, so nearly every order statistic is tied.  One cell per
    count of TIE_COUNTS (members in a shuffled order) and an empty one."""
    n, total = 8, max(TIE_COUNTS)
    rng = np.random.default_rng(8)
    stack = rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float32), (total, n, n))
    stack[:, n // 2, n // 2] = rng.choice(np.array([1, 2, 4, -2], np.float32), total)
    lists = [rng.permutation(total)[:m] for m in TIE_COUNTS] + [np.zeros(0, np.int64)]
    return _b2_case(stack, lists, TIE_PERCENTILES)


@functools.lru_cache(maxsize=None)
def b2_size_case(n: int) -> dict:
    """12 random float32 patches of n x n, cells of 1, 2, 5 and 12 members and an empty one."""
    rng = np.random.default_rng([12, n])
    stack = (rng.normal(0.0, 0.05, (12, n, n)) + 0.2 * rng.random((12, 1, 1))).astype(np.float32)
    stack[:, n // 2, n // 2] = rng.uniform(0.5, 2.0, 12).astype(np.float32)
    lists = [rng.permutation(12)[:m] for m in B2_SIZE_COUNTS] + [np.zeros(0, np.int64)]
    return _b2_case(stack, lists, TIE_PERCENTILES)


def check_b2(case: dict, average) -> dict:
    """`average(method, q)` on the case's stack, offsets and members: mean and median bit-identical to NumPy, every percentile
    within 1e-12 relative of the cell's maximum (check_average's bound), the empty cell all zero.  Returns what `average` gave."""
    got = {"mean": average("mean", 50.0), "median": average("median", 50.0)}
    for key in ("mean", "median"):
        assert got[key].dtype == np.float64
        assert np.array_equal(got[key].view(np.int64), case[key].view(np.int64)), f"{key} is not bit-identical to NumPy"
    worst = 0.0
    for q in case["percentiles"]:
        got[q] = average("percentile", q)
        err = np.abs(got[q] - case[q]).max(axis=(1, 2))
        scale = np.abs(case[q]).max(axis=(1, 2))
        worst = max(worst, float(np.max(err / np.maximum(scale, 1e-300))))
        assert np.all(err <= 1e-12 * scale), f"percentile {q}"
    print(f"N = {case['stack'].shape[-1]}: percentiles {case['percentiles']}, max relative error {worst:.3e}")
    assert all(np.all(v[-1] == 0) for v in got.values())  # the empty cell
    return got
