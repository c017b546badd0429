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


def make_case(name: str, seed: int) -> tuple[np.ndarray, list[np.ndarray]]:
    """(frames, stars): frames (F, H, W) float64 holding float32 values; stars[f] (k, 2) float64 (row, col)."""
    case = CASES[name]
    (h, w), n = case["shape"], case["n"]
    rows, cols = np.mgrid[0:h, 0:w].astype(np.float64)
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
        amp = rng.uniform(60, 400, len(pos))
        sig_r, sig_c = rng.uniform(1.1, 1.5, len(pos)), rng.uniform(1.1, 1.5, len(pos))
        frame = 10.0 + 0.03 * rows - 0.02 * cols + rng.normal(0.0, 0.3, (h, w))
        for (r, c), a, sr, sc in zip(pos, amp, sig_r, sig_c):
            frame += a * np.exp(-0.5 * (((rows - r) / sr) ** 2 + ((cols - c) / sc) ** 2))
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


def emulator():
    """tests/emu/libemu_builder.so (built by __graft_entry__.build()): the kernels' per-thread phases on the CPU."""
    import ctypes

    lib = ctypes.CDLL(str(pathlib.Path(__file__).resolve().parent / "emu" / "libemu_builder.so"))
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
