"""Cases and the float64 / NumPy restatement of kernel B1n (DESIGN.md 3.6 "Neighbour-subtracted patches"): phase 1n - every pixel of a patch
takes out the fitted stars of the patch's neighbour list while it is gathered - followed by B1's own phases, operation for operation in the
order csrc/rpsf_core_builder_sub.hpp and csrc/rpsf_core_builder.hpp spell them, so that the emulator (tests/test_builder_sub_host.py) and the
restatement agree bit for bit.  tests/test_gpu_builder_sub.py runs the same cases on the GPU against the composition of S10 and B1."""

import ctypes
import functools
import math
import pathlib
import struct

import numpy as np

from tests import emulib
from regularizepsf_amd.builder import star_geometry

ROOT = pathlib.Path(__file__).resolve().parent.parent
REJECTED, ACCEPTED, DEGENERATE_RING = 0, 1, 2
CHUNK, BUCKET = 64, 32
POLE = -0.26794919243112270647
FLT_MAX = 3.40282346638528859812e38


# ---------------------------------------------------------------------------------------------------------------------- the restatement
def mirror_index(i, length: int):
    """np.pad(mode='reflect') as an index map (rpsfb::mirror_index), for an integer or an integer array."""
    period = 2 * (length - 1)
    m = np.mod(np.asarray(i, np.int64), period)
    return np.where(m < length, m, period - m)


def mirror_coordinate(x: float, length: int) -> float:
    """rpsfb::mirror_coordinate (scipy's NI_EXTEND_MIRROR), float64 as Python computes it."""
    sz2 = 2.0 * length - 2.0
    if x < 0:
        x = sz2 * float(int(-x / sz2)) + x
        return x + sz2 if x <= 1 - length else -x
    if x > length - 1:
        x -= sz2 * float(int(x / sz2))
        return sz2 - x if x > length - 1 else x
    return x


def star_drawn(flux: np.ndarray, cell: np.ndarray, n_cells: int) -> np.ndarray:
    return np.isfinite(flux) & (cell >= 0) & (cell < n_cells)


def model_sum(fr: np.ndarray, fc: np.ndarray, stars, cube: np.ndarray, radius: float, pos, flux, cell) -> np.ndarray:
    """s of phase 1n (and of S10) on the pixel grid fr x fc for the stars `stars` in the order given: for each, pr = fr - y, pc = fc - x,
    q = pr pr + pc pc, and where q <= R R: s = s + flux * model_at(...)."""
    n = cube.shape[1]
    h, r2 = n / 2.0 - 0.5, radius * radius
    s = np.zeros((len(fr), len(fc)), np.float64)
    for j in stars:
        pr = (fr.astype(np.float64) - pos[j, 0])[:, None]
        pc = (fc.astype(np.float64) - pos[j, 1])[None, :]
        q = pr * pr + pc * pc
        inside = q <= r2
        if not inside.any():
            continue
        rows, cols = np.nonzero(inside)
        u, v = pr[rows, 0] + h, pc[0, cols] + h
        fu, fv = np.floor(u), np.floor(v)
        i, k = fu.astype(np.int64), fv.astype(np.int64)
        a, b = u - fu, v - fv
        c = cube[cell[j]]
        m = ((1.0 - a) * ((1.0 - b) * c[i, k] + b * c[i, k + 1])) + (a * ((1.0 - b) * c[i + 1, k] + b * c[i + 1, k + 1]))
        s[rows, cols] = s[rows, cols] + flux[j] * m
    return s


def restate_gather(frame: np.ndarray, n: int, corner, neighbours, cube, radius, pos, flux, cell) -> np.ndarray:
    """Phase 1n of one patch: (double)(float)((double)img - s), float64 N x N."""
    fr, fc = mirror_index(corner[0] + np.arange(n), frame.shape[0]), mirror_index(corner[1] + np.arange(n), frame.shape[1])
    s = model_sum(fr, fc, neighbours, cube, radius, pos, flux, cell)
    with np.errstate(invalid="ignore", over="ignore"):
        return (frame[np.ix_(fr, fc)].astype(np.float64) - s).astype(np.float32).astype(np.float64)


def _prefilter(p: np.ndarray) -> None:
    """b1_prefilter of every line along axis 0 of `p`, in place."""
    n, z = p.shape[0], POLE
    gain = (1.0 - z) * (1.0 - 1.0 / z)
    p *= gain
    z_n_1 = 1.0
    for _ in range(n - 1):
        z_n_1 *= z
    z_i = z
    c0 = p[0] + z_n_1 * p[n - 1]
    for i in range(1, n - 1):
        c0 = c0 + z_i * (p[i] + z_n_1 * p[n - 1 - i])
        z_i *= z
    p[0] = c0 / (1.0 - z_n_1 * z_n_1)
    for i in range(1, n):
        p[i] = p[i] + z * p[i - 1]
    p[n - 1] = (z * p[n - 2] + p[n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        p[i] = z * (p[i + 1] - p[i])


def _tables(n: int, shift: float) -> tuple[np.ndarray, np.ndarray]:
    w, tap = np.empty((n, 4)), np.empty((n, 4), np.int64)
    for i in range(n):
        cc = mirror_coordinate(float(i) - shift, n)
        fl = math.floor(cc)
        x = cc - fl
        z = 1.0 - x
        w[i, 0] = z * z * z / 6.0
        w[i, 1] = (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0
        w[i, 2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
        w[i, 3] = 1.0 - w[i, 0] - w[i, 1] - w[i, 2]
        tap[i] = mirror_index(int(fl) - 1 + np.arange(4), n)
    return w, tap


def restate_b1(patch: np.ndarray, shift, saturation=np.inf, minimum=0.0, maximum=np.inf) -> tuple[np.ndarray, int]:
    """B1's phases 2 - 5 and the verdict on a gathered float64 patch: (float32 patch - NaN where phase 5 did not run -, flag)."""
    n = patch.shape[0]
    p = patch.copy()
    out = np.full((n, n), np.nan, np.float32)
    with np.errstate(all="ignore"):
        _prefilter(p)      # axis 0: every column walked down the rows
        _prefilter(p.T)    # axis 1 (a view: in place)
        (w0, t0), (w1, t1) = _tables(n, shift[0]), _tables(n, shift[1])
        acc = np.zeros((n, n))
        for j in range(4):
            acc = acc + w0[:, j, None] * p[t0[:, j], :]
        p = acc
        acc = np.zeros((n, n))
        for j in range(4):
            acc = acc + w1[None, :, j] * p[:, t1[:, j]]
        p = acc
        if np.any((p == 0.0) | ~(np.abs(p) <= 1.79769313486231570815e308)):
            return out, REJECTED
        centre = float(p[n // 2, n // 2])
        ring = ([(0, c) for c in range(1, n - 1)] + [(n - 1, c) for c in range(1, n - 1)] + [(r, 0) for r in range(1, n - 1)]
                + [(r, n - 1) for r in range(1, n - 1)])
        used = [(r, c, float(p[r, c])) for r, c in ring if float(p[r, c]) < centre]
        cnt = float(len(used))
        if cnt < 3:
            return out, DEGENERATE_RING
        sx = sy = sv = 0.0
        for r, c, v in used:
            sx, sy, sv = sx + c, sy + r, sv + v
        mx, my, mv = sx / cnt, sy / cnt, sv / cnt
        sxx = sxy = syy = sxv = syv = 0.0
        for r, c, v in used:
            dx, dy, dv = c - mx, r - my, v - mv
            sxx, sxy, syy, sxv, syv = sxx + dx * dx, sxy + dx * dy, syy + dy * dy, sxv + dx * dv, syv + dy * dv
        det = sxx * syy - sxy * sxy
        if not det > 1e-9 * sxx * syy:
            return out, DEGENERATE_RING
        a, b = (sxv * syy - syv * sxy) / det, (syv * sxx - sxv * sxy) / det
        c0 = mv - a * mx - b * my
        rows, cols = np.arange(n, dtype=np.float64)[:, None], np.arange(n, dtype=np.float64)[None, :]
        v = p - ((a * cols + b * rows) + c0)
        bad = bool(np.any(~(v < saturation) | ~(np.abs(v) <= FLT_MAX)))
        out = v.astype(np.float32)
        centre = float(v[n // 2, n // 2])
        ok = (not bad) and centre > minimum and centre < maximum and float(np.float32(centre)) != 0.0
        return out, ACCEPTED if ok else REJECTED


def brute_lists(case: dict) -> list[np.ndarray]:
    """The neighbour lists by the all-pairs rule: j != own, drawn, and S10's box of j clipped to the frame meets the hull of the patch's
    mirrored rows and columns."""
    h, w = case["frame"].shape
    n, radius, pos = case["n"], case["radius"], case["pos"]
    drawn = star_drawn(case["flux"], case["cell"], len(case["cube"]))
    r0 = np.maximum(np.floor(pos[:, 0] - radius) - 1, 0)
    r1 = np.minimum(np.ceil(pos[:, 0] + radius) + 1, h - 1)
    c0 = np.maximum(np.floor(pos[:, 1] - radius) - 1, 0)
    c1 = np.minimum(np.ceil(pos[:, 1] + radius) + 1, w - 1)
    on_frame = drawn & (r0 <= r1) & (c0 <= c1)
    lists = []
    for own, corner in zip(case["own"], case["rounded"]):
        fr, fc = mirror_index(corner[0] + np.arange(n), h), mirror_index(corner[1] + np.arange(n), w)
        meets = on_frame & (r0 <= fr.max()) & (r1 >= fr.min()) & (c0 <= fc.max()) & (c1 >= fc.min())
        if own >= 0:
            meets[own] = False
        lists.append(np.flatnonzero(meets).astype(np.int32))
    return lists


def restate_case(case: dict, lists: list[np.ndarray] | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(patches, flags) of a case by the restatement; `lists`: the neighbour lists (None: every other drawn star - a superset)."""
    drawn = star_drawn(case["flux"], case["cell"], len(case["cube"]))
    patches, flags = [], []
    for k, (own, corner, shift) in enumerate(zip(case["own"], case["rounded"], case["shift"])):
        neighbours = [j for j in (np.flatnonzero(drawn) if lists is None else lists[k]) if j != own]
        gathered = restate_gather(case["frame"], case["n"], corner, neighbours, case["cube"], case["radius"], case["pos"], case["flux"],
                                  case["cell"])
        patch, flag = restate_b1(gathered, shift, *case["thresholds"])
        patches.append(patch)
        flags.append(flag)
    return np.stack(patches), np.array(flags, np.uint8)


# ---------------------------------------------------------------------------------------------------------------------- the cases
def gaussian_cube(n_cells: int, n: int, rng, sigma: float = 1.3) -> np.ndarray:
    """Cells that hold a star the way build cuts it (centre at N / 2 - 0.5), each a little different."""
    d = np.arange(n) - (n / 2.0 - 0.5)
    cell = np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2 * sigma * sigma))
    return np.stack([cell * (1.0 + 0.05 * rng.random((n, n))) * (1.0 + 0.1 * k) for k in range(n_cells)])


def star_frame(shape, pos, flux, rng, sigma: float = 1.3) -> np.ndarray:
    rows, cols = np.arange(shape[0])[:, None], np.arange(shape[1])[None, :]
    frame = 5.0 + 0.02 * rows + 0.01 * cols + 0.05 * rng.random(shape)
    for (y, x), f in zip(pos, flux):
        if np.isfinite(f):
            frame = frame + f * np.exp(-((rows - y) ** 2 + (cols - x) ** 2) / (2 * sigma * sigma))
    return frame.astype(np.float32)


def _finish(case: dict) -> dict:
    case["pos"] = np.ascontiguousarray(case["pos"], np.float64).reshape(-1, 2)
    case["flux"] = np.ascontiguousarray(case["flux"], np.float64)
    case["cell"] = np.ascontiguousarray(case["cell"], np.int32)
    case["own"] = np.ascontiguousarray(case["own"], np.int32)
    case["cut"] = np.ascontiguousarray(case["cut"], np.float64).reshape(-1, 2)
    corner, rounded, shift = star_geometry(case["cut"], case["n"])
    case["corner"], case["rounded"], case["shift"] = corner, rounded.astype(np.int32), shift
    case.setdefault("thresholds", (np.inf, 0.0, np.inf))
    for value in case.values():
        if isinstance(value, np.ndarray):
            value.flags.writeable = False
    return case


def _field(seed: int, n: int, model_n: int, radius: float, shape, positions, *, own=None, extra_cut=(), n_cells: int = 2, nan_pixels=()) -> dict:
    """A star field: every star of `positions` is in the set with a flux of its own and is cut (`own`: which ones), `extra_cut` positions are
    cut with own = -1."""
    rng = np.random.default_rng([67, seed])
    pos = np.asarray(positions, np.float64).reshape(-1, 2)
    flux = 40.0 * (1.0 + 9.0 * rng.random(len(pos)))
    cell = rng.integers(0, n_cells, len(pos))
    frame = star_frame(shape, pos, flux, rng)
    frame = frame.copy()
    for r, c in nan_pixels:
        frame[r, c] = np.nan
    own = np.arange(len(pos)) if own is None else np.asarray(own)
    cut = np.concatenate([pos[own], np.asarray(extra_cut, np.float64).reshape(-1, 2)])
    own = np.concatenate([own, np.full(len(cut) - len(own), -1)])
    return {"n": n, "radius": radius, "frame": frame, "cube": gaussian_cube(n_cells, model_n, rng), "pos": pos, "flux": flux * (0.9 + 0.2 * rng.random(len(pos))),
            "cell": cell, "own": own, "cut": cut}


def _cluster(rng, centre, count: int, spread: float) -> np.ndarray:
    return np.asarray(centre) + spread * (rng.random((count, 2)) - 0.5)


@functools.cache
def case(name: str) -> dict:
    rng = np.random.default_rng([67, 1000 + sorted(CASES).index(name)])
    if name == "n5, model 8, R = 3, the odd rows":
        # a NaN flux (4), a cell above the model (5) and below it (6), two rows at one position (7, 8), a patch with nobody left in
        pos = [(10.2, 12.7), (12.9, 14.1), (20.5, 30.5), (22.0, 33.0), (11.5, 10.4), (13.3, 11.2), (9.1, 14.8), (30.25, 20.75), (30.25, 20.75),
               (33.1, 23.6)]
        c = _field(1, 5, 8, 3.0, (40, 48), pos, extra_cut=[(21.3, 31.6), (5.5, 40.5)])
        c["flux"] = c["flux"].copy()
        c["cell"] = c["cell"].copy()
        c["flux"][4], c["cell"][5], c["cell"][6] = np.nan, 2, -1
        return _finish(c)
    if name == "n16, model 16, R = 7, folds at every edge":
        # corners above and left of the frame and beyond its far edges; star 1's disc covers pixels patch 0 reads twice through the fold
        pos = [(2.3, 1.7), (1.5, 4.2), (37.6, 46.2), (36.1, 42.9), (20.4, 3.1), (3.2, 24.5), (38.9, 25.5), (19.5, 45.0), (20.0, 24.0), (24.5, 27.5)]
        return _finish(_field(2, 16, 16, 7.0, (40, 48), pos, extra_cut=[(0.0, 0.0), (39.0, 47.0)]))
    if name == "n16, model 4, R = 0.3":
        # the low end of R: a disc holds a pixel only when the star sits within 0.3 of it
        pos = [(10.0, 12.0), (12.1, 14.9), (13.0, 12.2), (20.5, 30.5), (22.0, 31.0), (9.8, 16.1)]
        return _finish(_field(3, 16, 4, 0.3, (40, 48), pos))
    if name == "n33, model 16, R = 7, a patch as wide as the frame":
        pos = [(16.4, 17.2), (20.5, 25.5), (30.2, 40.8), (8.8, 44.1), (35.5, 6.5), (24.0, 30.0), (27.3, 33.9)]
        return _finish(_field(4, 33, 16, 7.0, (40, 48), pos, extra_cut=[(2.0, 45.0)]))
    if name == "n64, model 32, R = 15, NaN pixels":
        pos = [(30.3, 33.8), (36.5, 39.5), (40.2, 30.1), (60.7, 60.2), (66.0, 57.0), (12.5, 60.5), (70.1, 12.9), (33.3, 30.6)]
        return _finish(_field(5, 64, 32, 15.0, (80, 72), pos, nan_pixels=[(75, 3), (2, 70)]))
    if name == "n65, model 65, R = 31.5":
        pos = [(40.5, 44.5), (47.2, 50.9), (44.0, 38.0), (70.7, 70.2), (75.0, 66.0), (20.5, 70.5), (80.1, 15.9), (38.3, 41.6), (52.5, 33.5)]
        return _finish(_field(6, 65, 65, 31.5, (96, 88), pos, own=[0, 1, 3, 6], extra_cut=[(48.0, 44.0)]))
    if name == "n128, model 128, R = 63, 130 neighbours":
        pos = np.concatenate([[(80.4, 70.6)], _cluster(rng, (80.0, 72.0), 130, 90.0).clip(1.0, 142.0)])
        return _finish(_field(7, 128, 128, 63.0, (160, 144), pos, own=[0, 17], extra_cut=[(100.0, 40.0)]))
    if name.startswith("n16, model 8, R = 3, a list of "):
        count = int(name.rsplit(" ", 1)[1])  # the chunk borders: the patch of star 0 has exactly this many neighbours
        pos = np.concatenate([[(24.3, 20.6)], _cluster(rng, (24.0, 21.0), count, 12.0)])
        return _finish(_field(8, 16, 8, 3.0, (48, 40), pos, own=[0]))
    if name.startswith("n128, model 16, R = 7, a list of "):
        count = int(name.rsplit(" ", 1)[1])
        pos = np.concatenate([[(70.3, 66.6)], _cluster(rng, (70.0, 67.0), count, 100.0).clip(0.5, 130.0)])
        return _finish(_field(9, 128, 16, 7.0, (144, 136), pos, own=[0]))
    if name == "n16, model 8, R = 3, a neighbour that leaves exact zeros":
        return _finish(zero_case())
    raise KeyError(name)


def zero_case() -> dict:
    """The frame IS star 1 drawn in float32 (dyadic cube values, a dyadic flux, a position on the half-pixel grid: every product and sum is
    exact, so float32 holds s itself) and +0.0 elsewhere: with star 1 taken out every pixel of patch 0 is exactly zero, and the zero test
    rejects it - as it rejects the same patch of S10's residual frame.  Patch 1 is star 1's own: nothing is taken out of it."""
    rng = np.random.default_rng([67, 99])
    cube = rng.integers(1, 64, (1, 8, 8)).astype(np.float64) / 16.0
    cube[0, 3:5, 3:5] += 8.0
    pos = np.array([(20.0, 22.0), (21.5, 23.0)])
    flux, cell = np.array([3.0, 2.5]), np.zeros(2, np.int32)
    s = model_sum(np.arange(40), np.arange(48), [1], cube, 3.0, pos, flux, cell)
    frame = s.astype(np.float32)
    assert np.array_equal(frame.astype(np.float64), s) and np.count_nonzero(frame) > 20
    return {"n": 16, "radius": 3.0, "frame": frame, "cube": cube, "pos": pos, "flux": flux, "cell": cell, "own": np.array([0, 1]), "cut": pos.copy()}


COUNTS = (0, 1, 64, 65, 130)
CASES = tuple(sorted([
    "n5, model 8, R = 3, the odd rows",
    "n16, model 16, R = 7, folds at every edge",
    "n16, model 4, R = 0.3",
    "n33, model 16, R = 7, a patch as wide as the frame",
    "n64, model 32, R = 15, NaN pixels",
    "n65, model 65, R = 31.5",
    "n128, model 128, R = 63, 130 neighbours",
    "n16, model 8, R = 3, a neighbour that leaves exact zeros",
    *(f"n16, model 8, R = 3, a list of {k}" for k in COUNTS),
    *(f"n128, model 16, R = 7, a list of {k}" for k in (65, 130)),
]))


@functools.cache
def expected(name: str) -> tuple[np.ndarray, np.ndarray]:
    """The restatement's (patches, flags) of a case on the brute-force lists, computed once and shared."""
    c = case(name)
    patches, flags = restate_case(c, brute_lists(c))
    patches.flags.writeable = flags.flags.writeable = False
    return patches, flags


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_well_posed() -> None:
    """What the issue asks the case table to hold, checked on the restatement and the brute-force lists."""
    lengths = {name: [len(l) for l in brute_lists(case(name))] for name in CASES}
    for k in COUNTS:
        assert lengths[f"n16, model 8, R = 3, a list of {k}"] == [k]
    assert lengths["n128, model 16, R = 7, a list of 65"] == [65] and lengths["n128, model 16, R = 7, a list of 130"] == [130]
    assert lengths["n128, model 128, R = 63, 130 neighbours"][0] == 130
    odd = case("n5, model 8, R = 3, the odd rows")
    assert np.isnan(odd["flux"][4]) and odd["cell"][5] == 2 and odd["cell"][6] == -1 and np.array_equal(odd["pos"][7], odd["pos"][8])
    assert all(4 not in l and 5 not in l and 6 not in l for l in brute_lists(odd)) and (odd["own"] == -1).sum() == 2
    folds = case("n16, model 16, R = 7, folds at every edge")
    h, w = folds["frame"].shape
    assert folds["rounded"][0].max() < 0 and np.all(folds["rounded"][2] + 16 > (h, w))  # above-left of the frame, beyond its far edges
    fr = mirror_index(folds["rounded"][0][0] + np.arange(16), h)
    fc = mirror_index(folds["rounded"][0][1] + np.arange(16), w)
    twice_r, twice_c = [v for v in set(fr) if (fr == v).sum() == 2], [v for v in set(fc) if (fc == v).sum() == 2]
    y, x = folds["pos"][1]  # star 1's disc holds a pixel patch 0 reads twice
    assert any((r - y) ** 2 + (c - x) ** 2 <= 49.0 for r in twice_r for c in twice_c)
    flags = {name: expected(name)[1] for name in CASES}
    assert flags["n16, model 8, R = 3, a neighbour that leaves exact zeros"][0] == REJECTED
    zero = case("n16, model 8, R = 3, a neighbour that leaves exact zeros")
    gathered = restate_gather(zero["frame"], 16, zero["rounded"][0], [1], zero["cube"], 3.0, zero["pos"], zero["flux"], zero["cell"])
    assert np.all(gathered == 0.0)
    nan = case("n64, model 32, R = 15, NaN pixels")
    assert np.isnan(nan["frame"]).sum() == 2 and REJECTED in flags["n64, model 32, R = 15, NaN pixels"] and ACCEPTED in flags["n64, model 32, R = 15, NaN pixels"]
    assert sum(int((f == ACCEPTED).sum()) for f in flags.values()) >= 30  # most patches are kept: the bits compared are real patches


# ---------------------------------------------------------------------------------------------------------------------- the point of it
# Noise-free frames of blended stars drawn from a known cube; with the true fluxes the neighbour-subtracted build must give what the same
# stars give when each is built alone in an empty frame, and the plain build must not.
TRUTH_N, TRUTH_R, TRUTH_SHAPE = 16, 7.0, (80, 96)
U32 = 2.0 ** -24  # the unit roundoff of float32


def truth_case() -> dict:
    """Groups of two and three stars 3 to 10 pixels apart, flux ratios up to 10, on the half-pixel grid: with N_m = 16 the star's centre sits
    at h = 7.5, so model_at samples the cube on its nodes (a = b = 0) and a star in the frame is flux x cell, pixel for pixel."""
    from regularizepsf_amd.util import calculate_covering

    anchors = [(20.5, 20.5), (20.5, 52.5), (24.5, 78.5), (54.5, 24.5), (56.5, 56.5), (58.5, 80.5), (38.5, 38.5), (40.5, 66.5)]
    offsets = [[(3.0, 0.0)], [(0.0, 4.0), (5.0, 5.0)], [(6.0, -3.0)], [(-3.0, 3.0), (4.0, 7.0)], [(10.0, 0.0)], [(-5.0, -5.0)], [(2.0, 3.0)],
               [(0.0, -7.0), (7.0, 2.0)]]
    ratios = iter([10.0, 0.1, 3.0, 0.25, 0.125, 8.0, 10.0, 0.5, 2.0, 0.1, 6.0])  # neighbour / anchor
    pos, flux = [], []
    for anchor, others in zip(anchors, offsets):
        pos.append(anchor)
        flux.append(100.0)
        for dy, dx in others:
            pos.append((anchor[0] + dy, anchor[1] + dx))
            flux.append(100.0 * next(ratios))
    pos, flux = np.array(pos), np.array(flux)
    d = np.linalg.norm(pos[:, None] - pos[None], axis=2)
    near = np.where(d > 0, d, np.inf).min(axis=1)  # every star has a neighbour 3 to 10 pixels away, inside its 16-pixel patch
    assert near.min() >= 3.0 and near.max() <= 10.0 and flux.max() / flux.min() == 100.0
    coordinates = [tuple(int(v) for v in c) for c in calculate_covering(TRUTH_SHAPE, TRUTH_N)]
    dd = np.arange(TRUTH_N) - (TRUTH_N / 2.0 - 0.5)
    cell = np.exp(-(dd[:, None] ** 2 / (2 * 1.6 ** 2) + dd[None, :] ** 2 / (2 * 1.3 ** 2)))
    cube = np.stack([cell * (1.0 + 0.02 * (k % 5)) for k in range(len(coordinates))])
    return {"pos": pos, "flux": flux, "coordinates": coordinates, "cube": cube}


def plane_gain(n: int) -> float:
    """The largest factor by which the least-squares plane through the border ring (without its corners) of an n x n patch, evaluated anywhere
    on the patch, can exceed an error of the ring's values: the largest absolute row sum of A (A_ring^T A_ring)^-1 A_ring^T."""
    ring = ([(0, c) for c in range(1, n - 1)] + [(n - 1, c) for c in range(1, n - 1)] + [(r, 0) for r in range(1, n - 1)]
            + [(r, n - 1) for r in range(1, n - 1)])
    a_ring = np.array([(c, r, 1.0) for r, c in ring], np.float64)
    a_all = np.array([(c, r, 1.0) for r in range(n) for c in range(n)], np.float64)
    return float(np.abs(a_all @ np.linalg.solve(a_ring.T @ a_ring, a_ring.T)).sum(axis=1).max())


def truth_bound(frame_max: float, reference_patches: np.ndarray, reference_cell: np.ndarray) -> float:
    """The bound on |cell of the neighbour-subtracted build - cell of the reference| for one cell, derived and not tuned:

    1. Input.  The frame holds fl32(s_i + s_n) (own star plus neighbours, both exact in float64 up to 1e-16); phase 1n takes s_n out in
       float64 and rounds to float32 again; the reference frame holds fl32(s_i).  Three float32 roundings of values below the frame's
       largest pixel F: |input difference| <= 3 u F, u = 2^-24.
    2. Shift.  The prefilter of the cubic B-spline has the impulse response -6 z / (1 - z^2) z^|k|, whose absolute sum is
       6 |z| (1 + |z|) / ((1 - z^2)(1 - |z|)) = 3 for z = sqrt(3) - 2; mirrored ends fold it without enlarging the sum; the four tap weights
       are non-negative and sum to 1.  Two axes: a factor 9.
    3. Plane.  The fit is linear in the ring's values (the whole ring lies below the centre in both builds): what it subtracts differs by at
       most K = plane_gain(N) times the ring's difference, so a patch differs by at most (1 + K) 9 . 3 u F = e_p.
    4. Sample.  B2 divides the float32 patch by its float32 centre c >= c_min: with q = p / c, |dq| <= (e_p + |q| e_p) / (c_min - e_p), plus four
       float32 roundings (two per patch) of relative size u on a value of size |q| <= q_max.  The mean over a cell's members keeps the bound.
    5. Clean-up.  clean_cell subtracts a second ring plane (the factor 1 + K again), masks (the same mask in both: no pixel of the reference
       lies within the bound of the 0.5 % threshold, asserted by the caller) and divides by the sum S over the M kept pixels: the result v / S
       differs by at most e (1 / S) (1 + M max(v / S)).  Every sample's centre is 1, so the averaged cell's centre is 1 and the cleaned cell's
       centre is (1 - g) / S with g the second plane's value there: 1 / S is the reference cell's centre value divided by 1 - g, and g is
       computed from the reference's averaged cell with the product's own background_plane.
    c_min, q_max, M, max(v / S), g and 1 / S are read from the reference."""
    from regularizepsf_amd.builder import background_plane

    k = plane_gain(TRUTH_N)
    centre = reference_patches[:, TRUTH_N // 2, TRUTH_N // 2].astype(np.float64)
    c_min = float(centre.min())
    q_max = float(np.abs(reference_patches / centre[:, None, None]).max())
    e_p = (1.0 + k) * 9.0 * 3.0 * U32 * frame_max
    e_q = e_p * (1.0 + q_max) / (c_min - e_p) + 4.0 * U32 * q_max
    e = (1.0 + k) * e_q
    kept = int(np.count_nonzero(reference_cell))
    averaged = (reference_patches / centre[:, None, None]).mean(axis=0)
    g = float(background_plane(averaged)[TRUTH_N // 2, TRUTH_N // 2])
    assert abs(g) < 0.5  # the plane through the ring is far below the star's centre
    one_over_s = float(reference_cell[TRUTH_N // 2, TRUTH_N // 2]) / (1.0 - g)
    return e * one_over_s * (1.0 + kept * float(reference_cell.max()))


def truth_frames(render) -> tuple[np.ndarray, list[np.ndarray]]:
    """The blended frame and one frame per star alone; ``render(positions, fluxes, psf)`` draws one float32 frame of TRUTH_SHAPE."""
    from regularizepsf_amd.util import IndexedCube

    c = truth_case()
    psf = IndexedCube(c["coordinates"], c["cube"])
    return render(c["pos"], c["flux"], psf), [render(c["pos"][i:i + 1], c["flux"][i:i + 1], psf) for i in range(len(c["pos"]))]


def host_render(positions, fluxes, psf) -> np.ndarray:
    """S10's model mode restated: (float)s, the cells by nearest_cells."""
    from regularizepsf_amd.stars import nearest_cells

    cells = nearest_cells(positions, psf.coordinates, TRUTH_N)
    return model_sum(np.arange(TRUTH_SHAPE[0]), np.arange(TRUTH_SHAPE[1]), range(len(positions)), np.asarray(psf.values), TRUTH_R,
                     np.asarray(positions, np.float64), np.asarray(fluxes, np.float64), cells).astype(np.float32)


def restated_build(frames: list[np.ndarray], stars: list[np.ndarray], subtract: tuple | None = None) -> tuple[dict, dict, dict]:
    """A mean build through the restatement of B1 (B1n with ``subtract = (fluxes per frame, cells per frame, cube, radius)``) and the product's
    host code for the rest: (cells by corner, counts by corner, float64 patches by key)."""
    from regularizepsf_amd.builder import cell_membership, clean_cell
    from regularizepsf_amd.util import calculate_covering

    n = TRUTH_N
    keys, values = [], []
    for i, (frame, pos) in enumerate(zip(frames, stars)):
        corner, rounded, shift = star_geometry(pos, n)
        for k in range(len(pos)):
            neighbours = []
            if subtract is not None:
                flux, cell, cube, radius = subtract[0][i], subtract[1][i], subtract[2], subtract[3]
                neighbours = [j for j in range(len(pos)) if j != k]
                gathered = restate_gather(frame, n, rounded[k], neighbours, cube, radius, pos, flux, cell)
            else:
                gathered = restate_gather(frame, n, rounded[k], [], np.zeros((1, n, n)), 1.0, pos, None, None)
            patch, flag = restate_b1(gathered, shift[k])
            assert flag == ACCEPTED, (i, k, flag)
            keys.append((i, *corner[k].tolist()))
            values.append(patch.astype(np.float64))
    corners = calculate_covering(frames[0].shape, n)
    offsets, members = cell_membership(np.array([k[1:] for k in keys]).reshape(-1, 2), corners, n)
    cells, counts = {}, {}
    for c, corner in enumerate(corners):
        mine = members[offsets[c]:offsets[c + 1]]
        counts[tuple(corner)] = len(mine)
        if len(mine):
            acc = np.zeros((n, n))
            for m in mine:
                acc = acc + values[m] / values[m][n // 2, n // 2]
            cells[tuple(corner)] = clean_cell(acc / len(mine))
    return cells, counts, dict(zip(keys, values))


def check_truth(subtracted: tuple, alone: tuple, plain: tuple, frame_max: float, label: str = "", verbose: bool = False) -> tuple[float, float]:
    """Each argument is ``(cells by corner, counts by corner, patches by key)`` of a mean build - neighbour-subtracted on the blended frame,
    every star alone in its own frame, plain on the blended frame.  Every cell that holds a star must lie within truth_bound of the
    reference, and the plain build must violate it: returns the largest error / bound of the two."""
    from regularizepsf_amd.builder import cell_membership

    n = TRUTH_N
    assert subtracted[1] == alone[1] == plain[1] and sum(alone[1].values()) >= len(truth_case()["pos"])
    keys = list(alone[2])
    corners = np.array(list(alone[1]))
    offsets, members = cell_membership(np.array([k[1:] for k in keys]).reshape(-1, 2), corners, n)
    worst, worst_plain = 0.0, 0.0
    for c, corner in enumerate(map(tuple, corners)):
        if alone[1][corner] == 0:
            continue
        reference = np.asarray(alone[0][corner])
        patches = np.stack([alone[2][keys[m]] for m in members[offsets[c]:offsets[c + 1]]])
        ring = np.ones((n, n), bool)
        ring[1:-1, 1:-1] = False
        assert np.all(patches[:, ring] < patches[:, n // 2, n // 2][:, None])  # the whole ring enters the plane fit
        bound = truth_bound(frame_max, patches, reference)
        error = float(np.abs(np.asarray(subtracted[0][corner]) - reference).max())
        error_plain = float(np.abs(np.asarray(plain[0][corner]) - reference).max())
        if verbose:
            print(f"{label}cell {corner}: {alone[1][corner]} stars, bound {bound:.3e}, neighbour-subtracted {error:.3e}, plain build {error_plain:.3e}")
        worst, worst_plain = max(worst, error / bound), max(worst_plain, error_plain / bound)
    print(f"{label}largest error / bound over the cells with stars: neighbour-subtracted {worst:.3e}, plain build {worst_plain:.3e}")
    return worst, worst_plain


# ---------------------------------------------------------------------------------------------------------------------- the emulator
_clang = emulib.compiler


@functools.cache
def emulator():
    """tests/emu/libemu_builder_sub.so, compiled here when it is missing or older than its sources (as tests/builder_cases.py does)."""
    lib = emulib.library("emu_builder_sub")
    vp, i, d, q = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
    lib.emubn_lists.argtypes = [i, i, i, i, vp, vp, i, vp, vp, vp, i, d, vp, vp, q]
    lib.emubn_lists.restype = q
    lib.emubn_patches.argtypes = [i, vp, i, i, vp, i, vp, vp, vp, d, i, vp, vp, vp, vp, d, d, d, vp, vp]
    return lib


def emu_lists(c: dict) -> list[np.ndarray]:
    """The product's neighbour lists (rpsfbn::neighbour_lists) of a case."""
    h, w = c["frame"].shape
    k = len(c["own"])
    offsets, index = np.zeros(k + 1, np.int64), np.zeros(k * len(c["pos"]) + 1, np.int32)
    total = emulator().emubn_lists(h, w, c["n"], k, c["rounded"].ctypes.data, c["own"].ctypes.data, len(c["pos"]), c["pos"].ctypes.data,
                                   c["flux"].ctypes.data, c["cell"].ctypes.data, len(c["cube"]), c["radius"], offsets.ctypes.data,
                                   index.ctypes.data, len(index))
    assert total == offsets[-1] >= 0
    return [index[offsets[j]:offsets[j + 1]].copy() for j in range(k)]


def emu_patches(c: dict, lists: list[np.ndarray]) -> tuple[np.ndarray, np.ndarray]:
    """Kernel B1n on the emulator with the given lists: (float32 patches, NaN where phase 5 did not run; flags)."""
    h, w = c["frame"].shape
    k, n = len(c["own"]), c["n"]
    offsets = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    index = np.ascontiguousarray(np.concatenate([*lists, np.zeros(1, np.int32)]), np.int32)
    cube = np.ascontiguousarray(c["cube"], np.float64)
    patches, flags = np.full((k, n, n), np.nan, np.float32), np.zeros(k, np.uint8)
    rc = emulator().emubn_patches(n, c["frame"].ctypes.data, h, w, cube.ctypes.data, cube.shape[1], c["pos"].ctypes.data, c["flux"].ctypes.data,
                                  c["cell"].ctypes.data, c["radius"], k, offsets.ctypes.data, index.ctypes.data, c["rounded"].ctypes.data,
                                  np.ascontiguousarray(c["shift"]).ctypes.data, *c["thresholds"], patches.ctypes.data, flags.ctypes.data)
    assert rc == 0
    return patches, flags


def case_file(c: dict) -> bytes:
    """The input of the stand-alone emulator (EMU_BUILDER_SUB_MAIN)."""
    h, w = c["frame"].shape
    cube = np.ascontiguousarray(c["cube"], np.float64)
    head = struct.pack("<7q4d", c["n"], h, w, len(cube), cube.shape[1], len(c["pos"]), len(c["own"]), c["radius"], *c["thresholds"])
    return head + b"".join(np.ascontiguousarray(a).tobytes() for a in (c["frame"], cube, c["pos"], c["flux"], c["cell"], c["own"], c["rounded"],
                                                                      c["shift"]))


def read_result(c: dict, raw: bytes) -> tuple[np.ndarray, np.ndarray, list[np.ndarray]]:
    k, n = len(c["own"]), c["n"]
    flags = np.frombuffer(raw[:k], np.uint8)
    patches = np.frombuffer(raw[k:k + 4 * k * n * n], np.float32).reshape(k, n, n)
    rest = raw[k + 4 * k * n * n:]
    offsets = np.frombuffer(rest[:8 * (k + 1)], np.int64)
    index = np.frombuffer(rest[8 * (k + 1):], np.int32)
    assert len(index) == offsets[-1]
    return patches, flags, [index[offsets[j]:offsets[j + 1]] for j in range(k)]


# ---------------------------------------------------------------------------------------------------------------------- on the GPU
def _gpu_psf(case):
    import regularizepsf_amd as rp

    return rp.IndexedCube([(0, 16 * k) for k in range(len(case["cube"]))], np.asarray(case["cube"]))


def gpu_subtracted(case, on_device=False):
    """Kernel B1n on a case: (flags of every patch, the accepted float32 patches, B1n's device time)."""
    from regularizepsf_amd import builder as bld
    from regularizepsf_amd import stars
    from regularizepsf_amd.device_array import to_device

    stack, model = bld._Stack(case["n"], 0, 4), stars._Model(np.asarray(case["cube"]), 0)
    try:
        shape = case["frame"].shape
        frame = to_device(np.asarray(case["frame"])) if on_device else np.asarray(case["frame"])
        flags = stack.add_frame_subtracted(frame.ptr if on_device else frame, shape, model, case["pos"], case["flux"], case["cell"], case["radius"],
                                           case["own"], case["rounded"], case["shift"], *case["thresholds"])
        return flags, stack.patches(), stack.kernel_ms()[0]
    finally:
        stack.close()
        model.close()


def gpu_composed(case, rows=None):
    """The reference of the issue: per patch S10's residual into a device frame with the own star's flux set to NaN, then B1 on that frame
    with that one star.  (flags, the accepted patches in order)."""
    import regularizepsf_amd as rp
    from regularizepsf_amd import builder as bld
    from regularizepsf_amd.device_array import device_empty

    psf, shape = _gpu_psf(case), case["frame"].shape
    out = device_empty(shape, np.float32, 0)
    stack = bld._Stack(case["n"], 0, 4)
    try:
        flags = []
        for k in range(len(case["own"])) if rows is None else rows:
            flux = np.array(case["flux"])
            if case["own"][k] >= 0:
                flux[case["own"][k]] = np.nan
            rp.subtract_stars(np.asarray(case["frame"]), [np.asarray(case["pos"])], psf, case["radius"], flux=[flux], cells=[np.asarray(case["cell"])],
                              out=out)
            flags.append(stack.add_frame_device(out.ptr, shape, case["rounded"][k:k + 1], case["shift"][k:k + 1], *case["thresholds"])[0])
        return np.array(flags, np.uint8), stack.patches()
    finally:
        stack.close()
