"""Kernel S1 (the background mesh, `s1_box` of csrc/rpsf_core_stars.hpp) on hard boxes: value domains, ties, degenerate counts, the round
cap, odd box sizes and frame geometry.  The cases and checks that the emulator test (tests/test_mesh_host.py) and the GPU test
(tests/test_gpu_mesh.py) share; the restatement, the emulator and the detection checks are tests/star_cases.py's.

Every case asserts, from the restatement alone, its precondition (no sample within GAP_CLIP sd of a decision) and the branch it is named
for, before it looks at a kernel: a case that no longer reaches its branch fails.

THE BOUND.  u = 2^-53, gamma(k) = k u / (1 - k u).  Per box, on the final kept set v_1 .. v_n of the restatement (float32 values, so
integers times 2^-149): A = sum |v|, and mu, var = the exact mean and variance, from integer arithmetic.  The kernel's level and rms are
compared with the restatement's; the distance allowed is the restatement's own error, which is measured against the exact value, plus a
bound on the kernel's:
  * sums.  Any summation tree in which no term passes through more than D additions returns the sum within gamma(D) sum |terms|
    (every term collects at most D factors 1 + delta).  S1 sums per thread in index order, at most ceil(cnt / 256) terms for a box of
    cnt pixels, then 16 x 16 in two folds; an addition with the 0.0 of a sample outside the kept set is exact, and the others number
    n - 1 in all: D = min(ceil(cnt / 256) + 32, n - 1).  That is never more than the n - 1 of "two summation orders of n terms differ
    by at most 2 n u sum |v|"; check_bound_is_no_looser asserts that the whole bound stays inside what that rule allows, and inside
    star_cases' MESH_TOLERANCE on star_cases' frames.
  * mean: e = gamma(D + 1) A / n + u |mu|   (the sum, the division).
  * median: exact.  For an even count both sides compute (a + b) / 2 on the same two float32 values in IEEE float64: the same bits.
  * level: the median where the rule takes it, bound 0.  Otherwise fl(fl(2.5 med) - fl(1.5 mean)):
    1.5 e + u (2.5 |med| + 1.5 |mu| + |L|) with L = 2.5 med - 1.5 mu.
  * rms: the kernel sums fl(fl(v - m)^2) for its own mean m; exactly, sum (v - m)^2 = n var + n (m - mu)^2.  Three roundings per term, the
    tree, the division: the variance is off by a relative x = gamma(D + 4) + e^2 / var, the root by x / 2 (asserted: x <= 2^-27, so
    x^2 / 8 < u), and the square root itself is allowed one ulp (2 u) - nobody has shown the device's to be correctly rounded:
    rms (x / 2 + 2 u), plus 2 u rms for the float64 roundings of the exact value the restatement's error is measured against.
  * all kept samples equal: n c is exact in float64 for n <= 2^14 and 24-bit c, the mean is c, sd is 0 on both sides: bound 0.
The decisions (clip, the 0.3 sd rule) are the same on both sides when the restatement's gap is larger than these errors; next to
gap >= GAP_CLIP each box asserts e + 3 E_rms <= gap sd for its final set.
"""

from __future__ import annotations

import ctypes
import functools
import math
from fractions import Fraction

import numpy as np

from tests import star_cases as sc

U = 2.0 ** -53
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN_NORMAL = float(np.finfo(np.float32).tiny)
DENORM = 2.0 ** -149
S1_THREADS, MAX_ROUNDS = 256, 16
_SCALE = 2 ** 149


def gamma(k: int) -> float:
    return k * U / (1 - k * U)


def tree_depth(cnt: int) -> int:
    """The largest number of additions one term passes through in a pass of S1 over a box of `cnt` pixels."""
    return -(-cnt // S1_THREADS) + 32


def f32(a) -> np.ndarray:
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def bits(x: float) -> bytes:
    return np.float64(x).tobytes()


# ------------------------------------------------------------------------------------------------------------------ the tracing twin
def trace_box(values: np.ndarray) -> dict:
    """star_cases.ref_box, statement for statement, that also records what happened: per round the count, the extremes, the two middle
    samples and the statistics; why the rounds stopped ("empty", "sd0", "cap", "converged"); which side of the 0.3 sd rule the level took
    ("med", "mode"; "sd0" when sd == 0 decided); the final kept set."""
    v = np.asarray(values, np.float64)
    out = {"level": np.nan, "rms": np.nan, "gap": np.inf, "rounds": [], "stop": "empty", "rule": None, "kept": v}
    if v.size == 0:
        return out
    gap = np.inf
    for clip_round in range(17):
        med, mean = np.median(v), np.mean(v)
        sd = np.sqrt(np.mean((v - mean) ** 2))
        s = np.sort(v)
        out["rounds"].append({"n": v.size, "lo": s[0], "hi": s[-1], "mid": (s[(v.size - 1) // 2], s[v.size // 2]), "med": med, "mean": mean,
                              "sd": sd})
        if clip_round == 16 or sd == 0:
            out["stop"] = "sd0" if sd == 0 else "cap"
            break
        dist = np.abs(v - med)
        gap = min(gap, float(np.min(np.abs(dist - 3 * sd)) / sd))
        keep = dist <= 3 * sd
        if keep.all():
            out["stop"] = "converged"
            break
        v = v[keep]
    out["kept"] = v
    if sd == 0:
        out.update(level=med, rms=sd, gap=gap, rule="sd0")
        return out
    gap = min(gap, abs(abs(mean - med) - 0.3 * sd) / sd)
    rule = "med" if abs(mean - med) >= 0.3 * sd else "mode"
    out.update(level=med if rule == "med" else 2.5 * med - 1.5 * mean, rms=sd, gap=gap, rule=rule)
    return out


def exact_moments(v: np.ndarray) -> tuple[Fraction, Fraction]:
    """Mean and variance of float32 values, exactly."""
    ints = [a * (_SCALE // b) for a, b in (x.as_integer_ratio() for x in v.tolist())]
    n, s1, s2 = len(ints), sum(ints), sum(i * i for i in ints)
    return Fraction(s1, n * _SCALE), Fraction(n * s2 - s1 * s1, n * n * _SCALE * _SCALE)


def box_bounds(t: dict, cnt: int) -> dict:
    """The allowed |kernel - restatement| for level and rms of a traced box of `cnt` pixels (module docstring), the kernel's mean error
    `e`, and what the issue's plain `2 n u sum |v|` rule would allow (`plain_level`, `plain_rms`)."""
    v = t["kept"]
    n = v.size
    if n == 0 or t["rms"] == 0:
        assert n == 0 or (v.min() == v.max() and n <= 2 ** 14)
        return {"level": 0.0, "rms": 0.0, "e": 0.0, "plain_level": 0.0, "plain_rms": 0.0}
    last = t["rounds"][-1]
    A, D = float(np.sum(np.abs(v))), min(tree_depth(cnt), n - 1)  # additions with the 0.0 of a sample outside the kept set are exact
    mu, var = exact_moments(v)
    mu_f, var_f = float(mu), float(var)
    sd_f = math.sqrt(var_f)
    e = gamma(D + 1) * A / n + U * abs(mu_f)
    x = gamma(D + 4) + e * e / var_f
    assert x <= 2.0 ** -27, x
    rms = abs(t["rms"] - sd_f) + sd_f * (x / 2 + 4 * U)
    e_plain = 2 * gamma(n) * A / n + 2 * U * abs(mu_f)
    plain_rms = sd_f * ((2 * gamma(n + 4) + e_plain ** 2 / var_f) / 2 + 8 * U)
    if t["rule"] == "med":
        return {"level": 0.0, "rms": rms, "e": e, "plain_level": 0.0, "plain_rms": plain_rms}
    L = float(Fraction(5, 2) * Fraction(float(last["med"])) - Fraction(3, 2) * mu)
    scale = 2.5 * abs(last["med"]) + 1.5 * abs(mu_f) + abs(L)
    level = abs(t["level"] - L) + U * abs(L) + 1.5 * e + U * scale
    return {"level": level, "rms": rms, "e": e, "plain_level": 1.5 * e_plain + 3 * U * scale, "plain_rms": plain_rms}


def mesh_reference(frame: np.ndarray, mask: np.ndarray | None, box: int) -> dict:
    """Every box of a frame traced: the restatement's raw mesh (asserted bit-equal to star_cases.ref_box's), the bounds, the traces."""
    frame = np.asarray(frame, np.float32).astype(np.float64)
    ok = np.isfinite(frame) & (~mask if mask is not None else True)
    nby, nbx = -(-frame.shape[0] // box), -(-frame.shape[1] // box)
    out = {k: np.empty((nby, nbx)) for k in ("level", "rms", "gap", "bound_level", "bound_rms", "plain_level", "plain_rms")}
    traces = {}
    for i in range(nby):
        for j in range(nbx):
            cut = (slice(i * box, (i + 1) * box), slice(j * box, (j + 1) * box))
            values = frame[cut][ok[cut]]
            t = traces[i, j] = trace_box(values)
            want = sc.ref_box(values)
            assert (bits(t["level"]), bits(t["rms"]), bits(t["gap"])) == tuple(bits(w) for w in want), (i, j)
            b = box_bounds(t, frame[cut].size)
            if t["rms"] > 0:  # the decisions are safe: the kernel's errors stay inside the gap
                assert b["e"] + 3 * b["rms"] <= t["gap"] * t["rms"], (i, j, b, t["gap"])
            out["level"][i, j], out["rms"][i, j], out["gap"][i, j] = t["level"], t["rms"], t["gap"]
            out["bound_level"][i, j], out["bound_rms"][i, j] = b["level"], b["rms"]
            out["plain_level"][i, j], out["plain_rms"][i, j] = b["plain_level"], b["plain_rms"]
    for a in out.values():
        a.flags.writeable = False
    out["traces"] = traces
    return out


def compare_mesh(level: np.ndarray, rms: np.ndarray, ref: dict, what: str) -> float:
    """A kernel's raw mesh against mesh_reference's: the NaN pattern, zeros, and the derived bound; returns the worst error / bound."""
    assert level.shape == ref["level"].shape and rms.shape == ref["rms"].shape, what
    worst, lines = 0.0, []
    for got, want, bound, name in ((level, ref["level"], ref["bound_level"], "level"), (rms, ref["rms"], ref["bound_rms"], "rms")):
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: the NaN pattern of the {name} differs"
        ok = ~np.isnan(want)
        assert np.all(got[ok & (want == 0)] == 0), f"{what}: a {name} that is 0 in the restatement is not 0"
        err = np.abs(got[ok] - want[ok])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound[ok])
        worst = max(worst, float(ratio.max(initial=0.0)))
        lines.append(f"{name} worst error / bound {ratio.max(initial=0.0):.2e}")
        assert np.all(err <= bound[ok]), f"{what}: {name} off by {err.max():.3e}, {ratio.max():.2e} of the bound, in box {np.argwhere(ok)[ratio.argmax()]}"
    print(f"{what}: mesh {level.shape}, clip gap {np.min(ref['gap']):.1e} sd, " + ", ".join(lines))
    return worst


def background(make_finder, frame: np.ndarray, mask: np.ndarray | None, box: int) -> tuple[np.ndarray, np.ndarray]:
    finder = make_finder(frame.shape, box)
    try:
        return finder.background(frame, mask)
    finally:
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ (a) the box table
def _usable_fill(shape, hidden: int = 0):
    """An empty box and its mask with the first `hidden` pixels masked."""
    mask = np.zeros(shape, bool)
    mask.ravel()[:hidden] = True
    return np.zeros(shape), mask


def _ints(lo: int, hi: int, odd: bool):
    def make(shape, rng):
        vals, mask = _usable_fill(shape, hidden=int((shape[0] * shape[1]) % 2 != odd))
        vals[~mask] = rng.integers(lo, hi + 1, int((~mask).sum()))
        return vals, mask
    return make


def _ints_split(shape, rng):
    vals, mask = _usable_fill(shape, hidden=(shape[0] * shape[1]) % 2)
    half = int((~mask).sum()) // 2
    vals[~mask] = rng.permutation(np.concatenate([rng.integers(390, 400, half), rng.integers(401, 411, half)]))
    return vals, mask


def _two_valued(share: float):
    def make(shape, rng):
        n = shape[0] * shape[1]
        low = round(share * n)
        return rng.permutation(np.concatenate([np.full(low, 100.0), np.full(n - low, 103.0)])).reshape(shape), np.zeros(shape, bool)
    return make


def _survivors(count: int):
    def make(shape, rng):
        mask = np.ones(shape, bool)
        mask.ravel()[-count:] = False
        return rng.normal(10.0, 0.3, shape), mask
    return make


def _all_unusable(shape, rng):
    vals, mask = rng.normal(10.0, 0.3, shape), np.zeros(shape, bool)
    kind = rng.integers(0, 4, shape)
    mask[kind == 0] = True
    vals[kind == 1], vals[kind == 2], vals[kind == 3] = np.nan, np.inf, -np.inf
    return vals, mask


def _collapse(shape, rng):
    vals = np.full(shape, 5.0)
    vals.ravel()[rng.choice(vals.size, 3, replace=False)] = (1000.0, -700.0, 1200.0)
    return vals, np.zeros(shape, bool)


def _skewed(shape, rng):
    n = shape[0] * shape[1]
    high = rng.permutation(n) < round(0.35 * n)
    return np.where(high.reshape(shape), rng.normal(12.0, 0.2, shape), rng.normal(10.0, 0.2, shape)), np.zeros(shape, bool)


def _flt_max(shape, rng):
    vals = rng.normal(0.0, 1.0, shape)
    vals.ravel()[rng.choice(vals.size, 4, replace=False)] = (FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX)
    return vals, np.zeros(shape, bool)


def _ladder(steps: int):
    """Uniform noise in [-1.5, 1.5] (no sample beyond 1.8 sd: the noise alone clips nothing) and `steps` outliers +-40^k."""
    def make(shape, rng):
        vals = rng.uniform(-1.5, 1.5, shape)
        k = np.arange(1, steps + 1)
        vals.ravel()[rng.choice(vals.size, steps, replace=False)] = np.where(k % 2 == 1, 1.0, -1.0) * 40.0 ** k
        return vals, np.zeros(shape, bool)
    return make


def _plain(make_values):
    return lambda shape, rng: (make_values(shape, rng), np.zeros(shape, bool))


def _signs(t):  # per round: (a negative sample is kept, a positive sample is kept)
    return [(r["lo"] < 0, r["hi"] > 0) for r in t["rounds"]]


def _reach_ladder(t, steps, n0):
    beyond = np.abs(t["kept"] - t["rounds"][-1]["med"]) > 3 * t["rms"]
    if steps > MAX_ROUNDS:  # the cap, not convergence, ends it: one outlier went per round and the next is still there
        return len(t["rounds"]) == MAX_ROUNDS + 1 and t["stop"] == "cap" and t["kept"].size == n0 - MAX_ROUNDS and beyond.any()
    if steps == MAX_ROUNDS:  # the last outlier goes in the last clip; the cap ends what had converged
        return len(t["rounds"]) == MAX_ROUNDS + 1 and t["stop"] == "cap" and t["kept"].size == n0 - MAX_ROUNDS and not beyond.any()
    return len(t["rounds"]) == steps + 1 and t["stop"] == "converged" and t["kept"].size == n0 - steps


# name: (generator(shape, rng) -> (values, mask), reach(trace, pixels in the box) -> the box took the branch it is named for)
DISTRIBUTIONS = {
    "straddle": (_plain(lambda s, g: g.normal(0.0, 0.3, s)), lambda t, n: all(neg and pos for neg, pos in _signs(t))),
    "negative": (_plain(lambda s, g: g.normal(-1000.0, 5.0, s)), lambda t, n: all(r["hi"] < 0 for r in t["rounds"])),
    "ties_even": (_ints(390, 410, odd=False),
                  lambda t, n: t["kept"].size % 2 == 0 and t["rounds"][-1]["mid"][0] == t["rounds"][-1]["mid"][1]),
    "ties_even_split": (_ints_split, lambda t, n: t["kept"].size % 2 == 0 and t["rounds"][-1]["mid"][0] < t["rounds"][-1]["mid"][1]),
    "ties_odd": (_ints(390, 410, odd=True), lambda t, n: t["kept"].size % 2 == 1 and len(np.unique(t["kept"])) <= 21),
    "two_valued_50": (_two_valued(0.5), lambda t, n: len(np.unique(t["kept"])) == 2 and t["kept"].size == n),
    "two_valued_70": (_two_valued(0.7), lambda t, n: len(np.unique(t["kept"])) == 2 and t["kept"].size == n),
    "constant_7.25": (_plain(lambda s, g: np.full(s, 7.25)), lambda t, n: len(t["rounds"]) == 1 and t["stop"] == "sd0" and t["level"] == 7.25),
    "constant_+0": (_plain(lambda s, g: np.full(s, 0.0)), lambda t, n: len(t["rounds"]) == 1 and t["stop"] == "sd0" and not np.signbit(t["kept"]).any()),
    "constant_-0": (_plain(lambda s, g: np.full(s, -0.0)), lambda t, n: len(t["rounds"]) == 1 and t["stop"] == "sd0" and np.signbit(t["kept"]).all()),
    "collapse": (_collapse, lambda t, n: len(t["rounds"]) == 2 and t["rounds"][0]["sd"] != 0 and t["stop"] == "sd0"
                 and t["rounds"][1]["lo"] == t["rounds"][1]["hi"] and t["kept"].size == n - 3),
    "n1": (_survivors(1), lambda t, n: t["kept"].size == 1 and t["stop"] == "sd0"),
    "n2": (_survivors(2), lambda t, n: t["kept"].size == 2 and t["rms"] > 0),
    "n3": (_survivors(3), lambda t, n: t["kept"].size == 3 and t["rms"] > 0),
    "all_unusable": (_all_unusable, lambda t, n: t["stop"] == "empty" and np.isnan(t["level"]) and np.isnan(t["rms"])),
    "rule_med": (_skewed, lambda t, n: t["rule"] == "med"),
    "rule_mode": (_plain(lambda s, g: g.normal(10.0, 0.3, s)), lambda t, n: t["rule"] == "mode"),
    "narrow": (_plain(lambda s, g: 1.0 + g.integers(0, 9, s) * 2.0 ** -23),
               lambda t, n: t["rounds"][0]["lo"] == 1.0 and t["rounds"][0]["hi"] == 1.0 + 2.0 ** -20),
    "octave": (_plain(lambda s, g: g.uniform(1.9, 2.1, s)), lambda t, n: t["rounds"][-1]["lo"] < 2.0 < t["rounds"][-1]["hi"]),
    "subnormal": (_plain(lambda s, g: g.integers(-1000, 1001, s) * DENORM),
                  lambda t, n: np.abs(t["kept"]).max() < FLT_MIN_NORMAL and t["rounds"][-1]["lo"] < 0 < t["rounds"][-1]["hi"] and t["rms"] > 0),
    "huge": (_plain(lambda s, g: g.normal(0.0, 1.0, s) * 1e37), lambda t, n: t["rms"] > 1e36),
    "flt_max": (_flt_max, lambda t, n: t["rounds"][0]["lo"] == -FLT_MAX and t["rounds"][0]["hi"] == FLT_MAX and t["rounds"][1]["n"] == n - 4),
    "ladder_cap": (_ladder(20), lambda t, n: _reach_ladder(t, 20, n)),
    "ladder_16": (_ladder(16), lambda t, n: _reach_ladder(t, 16, n)),
    "ladder_15": (_ladder(15), lambda t, n: _reach_ladder(t, 15, n)),
}
# table: box, boxes per mesh row, the distributions in mesh raster order.  Box 32: 4 samples per thread; box 64: 16; box 27: an odd box,
# 729 samples, the last pass of a thread short
TABLES = {
    "table32": (32, 5, tuple(DISTRIBUTIONS)),
    "table64": (64, 3, ("straddle", "ties_even_split", "negative", "subnormal", "ladder_cap", "collapse")),
    "table27": (27, 3, ("straddle", "ties_odd", "ties_even", "constant_-0", "ladder_cap", "n2")),
}


@functools.lru_cache(maxsize=None)
def table_case(name: str) -> dict:
    """One frame whose boxes hold one distribution each (shared; do not modify)."""
    box, per_row, names = TABLES[name]
    assert len(names) % per_row == 0
    frame, mask = np.zeros((len(names) // per_row * box, per_row * box)), np.zeros((len(names) // per_row * box, per_row * box), bool)
    for k, dist in enumerate(names):
        cut = (slice(k // per_row * box, (k // per_row + 1) * box), slice(k % per_row * box, (k % per_row + 1) * box))
        values, hidden = DISTRIBUTIONS[dist][0]((box, box), np.random.default_rng([list(DISTRIBUTIONS).index(dist), box, 53]))
        frame[cut], mask[cut] = values, hidden
    with np.errstate(over="ignore"):
        frame = f32(frame)
    assert np.isfinite(frame).sum() >= frame.size - box * box  # nothing overflowed in the rounding to float32
    frame.flags.writeable = mask.flags.writeable = False
    return {"frame": frame, "mask": mask, "box": box, "names": np.array(names).reshape(-1, per_row), "ref": mesh_reference(frame, mask, box)}


def check_table_reaches_its_branches(name: str) -> None:
    """From the restatement alone: every box is clear of its decisions and takes the branch it is named for."""
    case = table_case(name)
    ref, box = case["ref"], case["box"]
    for (i, j), t in ref["traces"].items():
        dist = case["names"][i, j]
        assert t["gap"] >= sc.GAP_CLIP, f"{name} {dist}: a sample lies {t['gap']:.1e} sd from a decision"
        assert DISTRIBUTIONS[dist][1](t, box * box), f"{name} {dist}: the box no longer reaches its branch ({t['stop']}, {len(t['rounds'])} rounds, " \
                                                     f"{t['kept'].size} kept, rule {t['rule']})"
    rules = {t["rule"] for t in ref["traces"].values()}
    if name == "table32":
        assert {"med", "mode", "sd0", None} <= rules
        r = ref["traces"][tuple(np.argwhere(case["names"] == "ladder_cap")[0])]
        assert r["kept"].size == 1008 and len(r["rounds"]) == 17


def check_table(make_finder, name: str) -> float:
    """(a): S1 alone on a table, against the restatement at the derived bound."""
    check_table_reaches_its_branches(name)
    case = table_case(name)
    level, rms = background(make_finder, case["frame"], case["mask"], case["box"])
    ref, worst = case["ref"], 0.0
    for (i, j), dist in np.ndenumerate(case["names"]):
        ratios = []
        for got, want, bound in ((level[i, j], ref["level"][i, j], ref["bound_level"][i, j]), (rms[i, j], ref["rms"][i, j], ref["bound_rms"][i, j])):
            err = abs(got - want)
            ratios.append(0.0 if err == 0 or np.isnan(want) else err / bound if bound > 0 else np.inf)
        worst = max(worst, *ratios)
        t = ref["traces"][i, j]
        print(f"{name} {dist}: {t['kept'].size} kept after {len(t['rounds'])} rounds ({t['stop']}, rule {t['rule']}), gap {t['gap']:.1e} sd, "
              f"level {level[i, j]:.17g} (error / bound {ratios[0]:.2e}), rms {rms[i, j]:.17g} (error / bound {ratios[1]:.2e})")
    return max(worst, compare_mesh(level, rms, ref, name))


# ------------------------------------------------------------------------------------------------------------------ (b), (c) whole frames
BOXES = (8, 9, 27, 63, 65, 100, 127, 128)
GEOMETRY = {  # name: shape, box, star positions.  one_wide: edge boxes of one row and of one column, and a corner box of one pixel
    "one_wide": ((65, 129), 64, ((30.3, 60.4),)),
    "inside_one_box": ((33, 37), 128, ((16.2, 18.7),)),
    "5x7": ((5, 7), 8, ()),
    "1x40": ((1, 40), 8, ()),
    "40x1": ((40, 1), 8, ()),
    "1x1": ((1, 1), 8, ()),
}
DOMAIN_SHAPE, DOMAIN_BOX = (120, 110), 32
DOMAIN_STARS = np.array([(16.3, 15.6), (15.8, 80.2), (80.4, 16.7), (75.2, 76.9)])  # boxes (0,0), (0,2), (2,0), (2,2), 11 pixels inside each
DOMAINS = ("zero_mean", "minus_500", "counts", "flat")


def _stars(shape, pos, amp, sig_r, sig_c) -> np.ndarray:
    rows, cols = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    out = np.zeros(shape)
    for (r, c), a, sr, sc_ in zip(pos, amp, sig_r, sig_c):
        out += a * np.exp(-0.5 * (((rows - r) / sr) ** 2 + ((cols - c) / sc_) ** 2))
    return out


def domain_frame(kind: str) -> np.ndarray:
    rng = np.random.default_rng([DOMAINS.index(kind), 41])
    # flat: amplitudes small enough that the faintest pixel above 10.0 (one float32 ulp of 10, 9.5e-7) stays above 1e-9 of the largest f
    amp = rng.uniform(20, 40, 4) if kind == "flat" else rng.uniform(100, 400, 4)
    stars = _stars(DOMAIN_SHAPE, DOMAIN_STARS, amp, rng.uniform(1.1, 1.5, 4), rng.uniform(1.1, 1.5, 4))
    if kind == "zero_mean":
        return f32(rng.normal(0.0, 0.3, DOMAIN_SHAPE) + stars)
    if kind == "minus_500":
        return f32(-500.0 + rng.normal(0.0, 0.3, DOMAIN_SHAPE) + stars)
    if kind == "counts":
        return f32(rng.poisson(400.0, DOMAIN_SHAPE) + np.rint(stars))
    return f32(10.0 + stars)


@functools.lru_cache(maxsize=None)
def frame_case(name: str) -> dict:
    """A whole-frame case with the restatement's detection and its traced mesh (shared; do not modify)."""
    mask = None
    if name.startswith("box"):
        box = int(name[3:])
        base = sc.frame_case("wide")  # 150 x 200, 20 stars; its clip and threshold gaps hold at every box of BOXES
        frame, truth = base["frame"], base["truth"]
    elif name in GEOMETRY:
        shape, box, pos = GEOMETRY[name]
        truth = np.array(pos, np.float64).reshape(-1, 2)
        frame = sc.star_frame(shape, truth, np.random.default_rng([list(GEOMETRY).index(name), 43]))
    else:
        frame, box, truth = domain_frame(name), DOMAIN_BOX, DOMAIN_STARS
    ref = sc.ref_detect(frame, mask, box)
    mesh = mesh_reference(frame, mask, box)
    assert ref["raw"][0].tobytes() == mesh["level"].tobytes() and ref["raw"][1].tobytes() == mesh["rms"].tobytes()
    return sc._freeze({"frame": frame, "mask": mask, "box": box, "truth": truth, "ref": ref, "mesh": mesh})


FRAME_CASES = tuple(f"box{b}" for b in BOXES) + tuple(GEOMETRY) + DOMAINS


def ref_f(case: dict) -> np.ndarray:
    """The restatement's filtered residual of a case."""
    frame = case["frame"]
    ok = np.isfinite(frame) & (~case["mask"] if case["mask"] is not None else True)
    return sc.ref_filter(np.where(ok, frame - sc.ref_surface(case["ref"]["level"], frame.shape, case["box"]), 0.0))


def check_frame_preconditions(name: str) -> None:
    """From the restatement alone: the clip gap, the threshold gap, and what the case is about."""
    case = frame_case(name)
    ref, frame, box = case["ref"], case["frame"], case["box"]
    assert ref["gap_clip"] >= sc.GAP_CLIP, f"{name}: a sample lies {ref['gap_clip']:.1e} sd from a clip boundary"
    if ref["T"] == 0:  # gap_threshold is inf by ref_detect's own rule: every f is exactly 0 or clearly not
        f = np.abs(ref_f(case))
        assert np.all((f == 0) | (f >= 1e-9 * f.max())), f"{name}: an f of {f[f > 0].min():.1e} next to T = 0, the largest is {f.max():.1e}"
    else:
        assert ref["gap_threshold"] >= sc.GAP_THRESHOLD, f"{name}: an f lies {ref['gap_threshold']:.1e} T from T"
    print(f"{name}: clip gap {ref['gap_clip']:.1e} sd, T = {ref['T']:.6g}, min |f - T| / T = {ref['gap_threshold']:.1e}, {len(ref['rows'])} detections")
    raw_level, raw_rms = ref["raw"]
    if name in DOMAINS or len(case["truth"]) == 1:
        assert len(ref["rows"]) == len(case["truth"])  # the stars are found: the rows compared below are not an empty list
    if name.startswith("box"):
        assert len(ref["rows"]) >= 15
    if name == "one_wide":
        assert raw_level.shape == (2, 3) and frame[64:, :64].shape == (1, 64) and frame[:64, 128:].shape == (64, 1) and raw_rms[1, 2] == 0
    if name == "inside_one_box":
        assert raw_level.shape == (1, 1)
    if name == "zero_mean":
        assert all(r["lo"] < 0 < r["hi"] for t in case["mesh"]["traces"].values() for r in t["rounds"])
        assert np.any(raw_level < 0) and np.any(raw_level > 0)
    if name == "minus_500":
        assert np.all(raw_level < -499)
    if name == "counts":
        assert np.array_equal(frame, np.rint(frame))  # integers, and a box of even count whose middle samples tie
        assert any(t["kept"].size % 2 == 0 and t["rounds"][-1]["mid"][0] == t["rounds"][-1]["mid"][1] for t in case["mesh"]["traces"].values())
    if name == "flat":
        assert ref["T"] == 0 and np.all(ref["level"] == 10.0) and np.all(raw_rms == 0)
        clipped = [len(t["rounds"]) for t in case["mesh"]["traces"].values() if len(t["rounds"]) > 1]
        print(f"flat: the four boxes with a star clip down to the constant in {clipped} rounds")
        assert len(clipped) == 4 and all(t["stop"] == "sd0" for t in case["mesh"]["traces"].values())


def check_frame(make_finder, name: str) -> float:
    """(b), (c): the raw mesh at the derived bound and the rows through star_cases.compare_rows."""
    check_frame_preconditions(name)
    case = frame_case(name)
    level, rms = background(make_finder, case["frame"], case["mask"], case["box"])
    worst = compare_mesh(level, rms, case["mesh"], name)
    sc.compare_rows(sc.run(make_finder, case), case["ref"], case["frame"].shape, name)
    return worst


# ------------------------------------------------------------------------------------------------------------------ (d) exact scaling
def check_scaling(make_finder) -> None:
    """A frame times 2^40 and 2^-40: exact in float32 with no subnormal sample, so every operation of the definition scales exactly.
    Raw level, raw rms and flux are the unscaled ones times the factor bit for bit; row, column and area are bit-equal."""
    case = frame_case("zero_mean")
    frame, box = case["frame"], case["box"]
    base_level, base_rms = background(make_finder, frame, None, box)
    base_rows = sc.run(make_finder, case)
    assert len(base_rows) == 4
    for factor in (2.0 ** 40, 2.0 ** -40):
        scaled = frame * factor
        nonzero = np.abs(scaled[scaled != 0])
        assert np.array_equal(f32(scaled), scaled) and nonzero.min() >= FLT_MIN_NORMAL and nonzero.max() <= FLT_MAX
        level, rms = background(make_finder, scaled, None, box)
        assert level.tobytes() == (base_level * factor).tobytes() and rms.tobytes() == (base_rms * factor).tobytes(), factor
        rows = sc.run(make_finder, {**case, "frame": scaled})
        assert rows.shape == base_rows.shape and rows[:, [0, 1, 3]].tobytes() == base_rows[:, [0, 1, 3]].tobytes(), factor
        assert rows[:, 2].tobytes() == (base_rows[:, 2] * factor).tobytes(), factor
        print(f"times 2^{int(np.log2(factor))}: {level.size} mesh nodes and {len(rows)} rows scale bit for bit")


# ------------------------------------------------------------------------------------------------------------------ (e) against the emulator
def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Float64 values between a and b, for finite values of one sign (or zeros)."""
    ia, ib = np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)
    return np.abs(ia - ib)


def check_against_emulator(make_finder, name: str) -> int:
    """A device's raw level bit-equal to the emulator's; its raw rms within the bound of (a), the distance in ulp printed and returned; on
    a whole-frame case the rows bit-equal."""
    case = table_case(name) if name in TABLES else frame_case(name)
    ref = case["ref"] if name in TABLES else case["mesh"]
    level, rms = background(make_finder, case["frame"], case["mask"], case["box"])
    emu_level, emu_rms = background(sc.EmuFinder, case["frame"], case["mask"], case["box"])
    ok = ~np.isnan(emu_level)
    assert np.array_equal(np.isnan(level), ~ok) and np.array_equal(np.isnan(rms), ~ok)
    assert level[ok].tobytes() == emu_level[ok].tobytes(), f"{name}: {np.count_nonzero(level[ok] != emu_level[ok])} levels differ from the emulator's"
    assert np.all(rms[ok] >= 0) and np.all(np.abs(rms[ok] - emu_rms[ok]) <= ref["bound_rms"][ok])
    ulps = int(ulp_distance(rms[ok], emu_rms[ok]).max(initial=0))
    print(f"{name}: {ok.sum()} boxes, level bit-equal to the emulator's, rms at most {ulps} ulp from it")
    if name not in TABLES:
        assert sc.run(make_finder, case).tobytes() == sc.run(sc.EmuFinder, case).tobytes(), name
    return ulps


# ------------------------------------------------------------------------------------------------------------------ (f) the carve
def s1_carve(box: int) -> tuple[int, int, int]:
    """(byte offset of S1's records in its LDS, bytes of the records, bytes a workgroup asks for) as kernel and launch compute them."""
    lib = sc.emulator()
    out = [ctypes.c_size_t(0) for _ in range(3)]
    lib.emus_s1_carve.argtypes = [ctypes.c_int] + [ctypes.POINTER(ctypes.c_size_t)] * 3
    lib.emus_s1_carve.restype = None
    lib.emus_s1_carve(box, *(ctypes.byref(o) for o in out))
    return tuple(o.value for o in out)


def check_carve() -> None:
    for box in range(8, 129):
        offset, records, total = s1_carve(box)
        assert offset % 16 == 0, f"box {box}: the records start {offset % 16} bytes off a 16-byte boundary"
        assert offset >= 4 * box * box and records == (S1_THREADS + 16) * 24 and total >= offset + records, box
        assert offset < 4 * box * box + 16 and total == offset + records, box  # and nothing is wasted
    assert s1_carve(128)[2] == 65536 + 6528  # what the launch may ask for at most (rpsf_stars_create)


# ------------------------------------------------------------------------------------------------------------------ the bound itself
def check_bound_is_no_looser() -> None:
    """On star_cases' own frames the derived bound is inside the relative MESH_TOLERANCE those frames are held to, and on every case of
    this module inside what `2 n u sum |v|` between two summation orders would allow."""
    for name, make in sc.CASES.items():
        case = make()
        ref = mesh_reference(case["frame"], case["mask"], case["box"])
        ok = ~np.isnan(ref["level"])
        rel_level, rel_rms = np.max(ref["bound_level"][ok] / np.abs(ref["level"][ok])), np.max(ref["bound_rms"][ok] / ref["rms"][ok])
        print(f"star_cases {name}: relative bound level {rel_level:.1e}, rms {rel_rms:.1e} (MESH_TOLERANCE {sc.MESH_TOLERANCE:.0e})")
        assert rel_level <= sc.MESH_TOLERANCE and rel_rms <= sc.MESH_TOLERANCE
    for name in tuple(TABLES) + FRAME_CASES:
        ref = table_case(name)["ref"] if name in TABLES else frame_case(name)["mesh"]
        ok = ~np.isnan(ref["level"])
        # (the measured error of the restatement is itself within one side of the plain rule; one rounding of slack for its measurement)
        assert np.all(ref["bound_level"][ok] <= ref["plain_level"][ok] * (1 + 2.0 ** -20)), name
        assert np.all(ref["bound_rms"][ok] <= ref["plain_rms"][ok] * (1 + 2.0 ** -20)), name
