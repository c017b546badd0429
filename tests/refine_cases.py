"""Gaussian-windowed positions and moments (DESIGN.md 3.7 "Windowed positions", kernel S7) restated in float64 NumPy, the cases, the CPU
emulator of the kernel, and the checks the emulator tests (tests/test_refine_host.py) and the GPU tests (tests/test_gpu_refine.py) share.

There is no outside implementation (this is not sep's winpos): the reference is the restatement below, written from the definition, one
position at a time, with array operations over the position's box.  A check takes `make_finder(shape, box)`:
regularizepsf_amd.stars._Finder on the GPU, EmuFinder here.

THE MESH is photometry_cases': the restatement takes the filtered mesh of the finder under test, so d is the same double on both sides.

THE WINDOW.  w = g(q h) is the same double on both sides too: q = pr pr + pc pc and h = 1 / (2 sigma sigma) are the same float64
expressions, and g is restated here operation for operation (`ref_g`), not through a math library.  `check_g` holds the emulator's g to
`ref_g` bit for bit and `ref_g` to exp in np.longdouble within G_BOUND, which is derived below from the polynomial's truncation and its
rounding steps.

THE COUNTS are integers from the same comparison q <= R R on both sides: N_use and N_all are compared exactly.

THE BOUND is photometry_cases' argument: both sides add the same rounded terms in different orders, so with n the number of pixels of
the box, A = sum w |d| over the usable pixels of the window, P = max |pr| and Q = max |pc| over the box,
    |S - ref| <= 2 n u A,  |A - ref| <= 2 n u A,  |mr - ref| <= 2 n u A P,  |mc - ref| <= 2 n u A Q,
    |mrr - ref| <= 2 n u A P^2,  |mcc - ref| <= 2 n u A Q^2,  |mrc - ref| <= 2 n u A P Q.
Nothing measured goes into it.  Where every term is zero (a window off the frame) the bound is zero and the sums are compared exactly.

THE CHAIN.  The iteration is not compared between two implementations whose roundings differ; it is pinned from the finder's own rows.
A call with max_iter = j delivers, for a star that has not stopped before, the walk at p_j - and the iteration walk and the measurement
walk are the same code in the same order.  So what the call with max_iter = j + 1 returns follows from the rules of the definition,
evaluated in NumPy float64 on run j's delivered sums, bit for bit (`check_chain`).  With THE BOUND on every walk that pins the trajectory.
"""

from __future__ import annotations

import ctypes
import functools
import math

import numpy as np

from tests import emulib
from regularizepsf_amd import stars
from tests import photometry_cases as pc
from tests import star_cases as sc

ROOT = sc.ROOT
U = 2.0 ** -53
COLUMNS = 18
Y0, X0, Y, X, SIGMA, NITER, FLAGS, DY, DX, N_USE, N_ALL, S, A, MR, MC, MRR, MCC, MRC = range(COLUMNS)
SUMS = slice(S, COLUMNS)
NO_FLUX, RAN_AWAY, NOT_CONVERGED = 1, 2, 4
SHAPE, BOX = pc.SHAPE, pc.BOX
DEFAULTS = {"max_iter": 16, "eps": 1e-4, "max_shift": 2.0}

# ------------------------------------------------------------------------------------------------------------------ the window function
LOG2E, LN2_HI, LN2_LO = 1.44269504088896338700e+00, 6.93147180369123816490e-01, 1.90821492927058770002e-10
INV_FACTORIAL = tuple(1.0 / float(math.factorial(j)) for j in range(14))  # j! is exact in float64 up to 13!


def ref_g(t):
    """g(t) of the definition, operation for operation, on float64 arrays."""
    t = np.asarray(t, np.float64)
    n = np.floor(t * LOG2E + 0.5)
    r = (t - n * LN2_HI) - n * LN2_LO
    z = -r
    p = np.full(t.shape, INV_FACTORIAL[13])
    for j in range(12, -1, -1):
        p = p * z + INV_FACTORIAL[j]
    return p * np.ldexp(1.0, -n.astype(np.int64))


# G_BOUND: |g(t) - exp(-t)| / exp(-t) for 0 <= t <= 8.  g = P(z) 2^-n with z = -r, and the scaling is exact (n <= 12: no subnormal), so
# the relative error is that of P(z) against exp(-r_true), r_true = t - n ln 2.  With a = G_REDUCED >= |r| (ln 2 / 2 and the slack of the
# rounded n; check_g asserts it on its grid), E = exp(a), all absolute, on a value that is at least 1 / E:
#   truncation   the series stops at z^13 / 13!: Lagrange's remainder, at most a^14 / 14! E;
#   Horner       p_k = fl(fl(p_(k+1) z) + c_k) with |p_k| <= sum_(j >= k) |z|^(j - k) / j! k!/k! <= E / k!: the error e_k of p_k obeys
#                e_k <= a e_(k+1) + u (a |p_(k+1)| + |p_k|), so e_0 <= u E sum_k a^k (a / (k + 1)! + 1 / k!) = u E (2 E - 1);
#   coefficients 1 / j! rounded once: at most u sum_j a^j / j! <= u E;
#   reduction    n LN2_HI is exact (LN2_HI ends in 20 zero bits, n <= 12); two subtractions and the product n LN2_LO round once each, and
#                LN2_HI + LN2_LO is ln 2 within 2^-64 (asserted in np.longdouble): r is off by at most 2 u a + 12 u LN2_LO + 12 2^-64, and
#                exp(-r) moves by at most E times that;
# second-order terms are covered by the factor 1 + 2^-40, and np.longdouble's own exp by one more 2^-62.
G_REDUCED = 0.3466
_E = math.exp(G_REDUCED)
G_BOUND = ((G_REDUCED ** 14 / math.factorial(14) * _E + U * _E * (2 * _E - 1) + U * _E
            + _E * (2 * U * G_REDUCED + 12 * U * LN2_LO + 12 * 2.0 ** -64)) * (1 + 2.0 ** -40)) * _E + 2.0 ** -62  # about 7.2 u


# ------------------------------------------------------------------------------------------------------------------ the restatement
def ref_walk(d, ok, y, x, sigma) -> tuple[int, int, np.ndarray, np.ndarray]:
    """One walk of the definition at (y, x): N_use, N_all, the seven sums (S, A, mr, mc, mrr, mcc, mrc) and THE BOUND on each."""
    H, W = d.shape
    y, x, sigma = np.float64(y), np.float64(x), np.float64(sigma)
    R = 4.0 * sigma
    R2, h = R * R, 1.0 / (2.0 * sigma * sigma)
    rr = np.arange(int(np.floor(y - R)) - 1, int(np.ceil(y + R)) + 2)
    cc = np.arange(int(np.floor(x - R)) - 1, int(np.ceil(x + R)) + 2)
    pr, pc_ = rr.astype(np.float64) - y, cc.astype(np.float64) - x
    q = (pr * pr)[:, None] + (pc_ * pc_)[None, :]
    window = q <= R2
    inside = ((rr >= 0) & (rr < H))[:, None] & ((cc >= 0) & (cc < W))[None, :]
    ri, ci = np.clip(rr, 0, H - 1), np.clip(cc, 0, W - 1)
    use = window & inside & ok[ri[:, None], ci[None, :]]
    dv = d[ri[:, None], ci[None, :]][use]
    w = ref_g(q[use] * h)
    PR, PC = np.broadcast_to(pr[:, None], use.shape)[use], np.broadcast_to(pc_[None, :], use.shape)[use]
    t = w * dv
    sums = np.array([np.sum(t), np.sum(w * np.abs(dv)), np.sum(t * PR), np.sum(t * PC), np.sum(t * (PR * PR)), np.sum(t * (PC * PC)),
                     np.sum(t * (PR * PC))])
    P, Q = np.abs(pr).max(), np.abs(pc_).max()
    bounds = 2 * use.size * U * sums[1] * np.array([1.0, 1.0, P, Q, P * P, Q * Q, P * Q])
    return int(use.sum()), int(window.sum()), sums, bounds


def ref_refine(frame, mask, box, level_f, positions, sigma, background: str, max_iter=16, eps=1e-4, max_shift=2.0) -> dict:
    """The definition.  rows: (k, COLUMNS) in the kernel's layout; bounds: (k, 7), THE BOUND on the seven sums of the delivered walk."""
    d, ok = pc.ref_residual(frame, mask, box, level_f, background)
    no_mesh = background == "mesh" and level_f is None
    positions = np.asarray(positions, np.float64).reshape(-1, 2)
    sigma = np.broadcast_to(np.asarray(sigma, np.float64), (len(positions),))
    rows, bounds = np.empty((len(positions), COLUMNS)), np.empty((len(positions), 7))
    eps2, shift2 = np.float64(eps) * np.float64(eps), np.float64(max_shift) * np.float64(max_shift)
    for i, ((y0, x0), sg) in enumerate(zip(positions, sigma)):
        y, x, niter, flags, dy, dx = y0, x0, 0, 0, np.nan, np.nan
        walk = None
        if no_mesh:
            flags = NO_FLUX
        for j in range(0 if no_mesh else max_iter):
            walk = ref_walk(d, ok, y, x, sg)  # 1
            total = walk[2][0]
            if not np.isfinite(total) or total <= 0.0:  # 2
                flags |= NO_FLUX
                break
            with np.errstate(over="ignore", invalid="ignore"):
                dy, dx = walk[2][2] / total, walk[2][3] / total  # 3
                ny, nx = y + 2.0 * dy, x + 2.0 * dx
                ey, ex = ny - y0, nx - x0
                away = not (np.isfinite(ny) and np.isfinite(nx)) or ey * ey + ex * ex > shift2
            if away:  # 4
                flags |= RAN_AWAY
                break
            y, x, niter, walk = ny, nx, j + 1, None  # 5
            if dy * dy + dx * dx < eps2:
                break
            if niter == max_iter:  # 6
                flags |= NOT_CONVERGED
        if walk is None:  # the measurement walk; after a stop at 2 or 4 it is the walk just made
            walk = ref_walk(d, ok, y, x, sg)
        rows[i, :N_USE] = y0, x0, y, x, sg, niter, flags, dy, dx
        rows[i, N_USE], rows[i, N_ALL] = walk[0], walk[1]
        rows[i, SUMS] = np.nan if no_mesh else walk[2]
        bounds[i] = walk[3]
    return {"rows": rows, "bounds": bounds}


# ------------------------------------------------------------------------------------------------------------------ the cases
SIGMAS = (0.5, 1.0, 1.5, 16.0)


def field():
    return pc.field()


def _case(frame, positions, sigma, background="mesh", mask=None, box=BOX, **iteration) -> dict:
    positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
    return {"frame": frame, "mask": mask, "box": box, "positions": positions, "background": background,
            "sigma": np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, np.float64), (len(positions),))), **DEFAULTS, **iteration}


def _walk_positions() -> np.ndarray:
    """The field's true positions and photometry_cases' hard ones: .5 ties, (0, 0), partly and wholly off the frame, two windows over one
    another."""
    return np.concatenate([field()["truth"], pc.hard_positions()])


def _mixture(k: int) -> np.ndarray:
    return np.resize(np.array(SIGMAS + (2.5, 1.2)), k)


def _masked_frame():
    c = pc.case("masked, mesh")
    return c["frame"], c["mask"]


def whole_pixel_starts() -> np.ndarray:
    return np.rint(field()["truth"])


def _stop_frame() -> np.ndarray:
    """A flat frame of 10 with a negative blob at (20, 20), a bright star at (60.3, 40.6), a faint one two pixels from it at (60.3, 42.6)
    a lone star at (30.4, 70.2), and two stars six pixels apart at (80.3, 38) and (80.3, 44) that the detector sees as one."""
    rows, cols = np.mgrid[0:SHAPE[0], 0:SHAPE[1]].astype(np.float64)

    def blob(r, c, amplitude, sigma=1.3):
        return amplitude * np.exp(-0.5 * ((rows - r) ** 2 + (cols - c) ** 2) / sigma ** 2)

    return (10.0 + blob(20.0, 20.0, -200.0) + blob(60.3, 40.6, 800.0) + blob(60.3, 42.6, 40.0) + blob(30.4, 70.2, 300.0)
            + blob(80.3, 38.0, 800.0) + blob(80.3, 44.0, 500.0)).astype(np.float32)


WALK_CASES = {
    **{f"walk, sigma {s:g}, {b}": functools.partial(lambda s, b: _case(field()["frame"], _walk_positions(), s, b, max_iter=0), s, b)
       for s in SIGMAS for b in ("mesh", "none")},
    **{f"walk, mixture, {b}": functools.partial(lambda b: _case(field()["frame"], _walk_positions(), _mixture(23), b, max_iter=0), b)
       for b in ("mesh", "none")},
    **{f"walk, masked, {b}": functools.partial(
        lambda b: _case(_masked_frame()[0], _walk_positions(), _mixture(23), b, _masked_frame()[1], max_iter=0), b) for b in ("mesh", "none")},
}
CHAIN_CASES = {
    "chain, sigma 1.5": lambda: _case(field()["frame"], whole_pixel_starts(), 1.5),
    "chain, sigma 2.5": lambda: _case(field()["frame"], whole_pixel_starts(), 2.5),
}
CHAIN_J = 17
STOP_CASES = {
    "negative blob": lambda: _case(_stop_frame(), [(20.0, 20.0), (21.0, 19.0)], 1.5, "none"),
    "faint next to bright": lambda: _case(_stop_frame(), [(60.3, 42.6), (60.0, 43.0)], 1.5, max_shift=0.5),
    "between two stars": lambda: _case(_stop_frame(), [(80.3, 40.3), (80.0, 40.5)], 1.0),
    "far start, one iteration": lambda: _case(_stop_frame(), [(31.0, 71.0), (30.0, 70.0)], 1.5, max_iter=1),
    "off the frame": lambda: _case(_stop_frame(), [(-30.0, -30.0), (200.5, 48.0), (48.0, -70.25)], (1.0, 16.0, 2.5)),
    "no valid mesh node": lambda: _case(np.full(SHAPE, np.nan, np.float32), [(30.2, 40.7), (0.0, 0.0), (-30.0, -30.0)], 1.5),
    # one workgroup: a star that stops at j = 0, one that converges, one that runs to the cap, and another converging one
    "one workgroup, three ends": lambda: _case(field()["frame"], np.concatenate([[(-30.0, -30.0)], whole_pixel_starts()[[0, 1, 2]]]),
                                               (1.5, 1.5, 2.5, 1.0), max_iter=6),
}
ROW_COUNTS = (0, 1, 3, 4, 5, 9)  # 0, 1, WALK_WAVES - 1, WALK_WAVES, WALK_WAVES + 1, 2 WALK_WAVES + 1 (check_row_counts asserts that)
ROW_CASES = {f"{k} rows": functools.partial(lambda k: _case(field()["frame"], np.concatenate([whole_pixel_starts(), [(0.0, 0.0)]])[:k],
                                                             _mixture(9)[:k]), k) for k in ROW_COUNTS}
CASES = {**WALK_CASES, **CHAIN_CASES, **STOP_CASES, **ROW_CASES}


@functools.cache
def case(name: str) -> dict:
    return sc._freeze(CASES[name]())


@functools.lru_cache(maxsize=None)
def _reference(name: str, mesh_bytes: bytes | None, max_iter: int) -> dict:
    c = case(name)
    level_f = None if mesh_bytes is None else np.frombuffer(mesh_bytes).reshape(-(-c["frame"].shape[0] // c["box"]), -(-c["frame"].shape[1] // c["box"]))
    return sc._freeze(ref_refine(c["frame"], c["mask"], c["box"], level_f, c["positions"], c["sigma"], c["background"], max_iter, c["eps"],
                                 c["max_shift"]))


def reference(name: str, level_f, max_iter: int | None = None) -> dict:
    """The restatement's answer for the case on the filtered mesh `level_f` (None: no valid node), computed once per case and mesh."""
    c = case(name)
    mesh = None if level_f is None or c["background"] == "none" else np.ascontiguousarray(level_f).tobytes()
    return _reference(name, mesh, c["max_iter"] if max_iter is None else max_iter)


# ------------------------------------------------------------------------------------------------------------------ the emulator
@functools.cache
def emulator():
    """tests/emu/libemu_refine.so: the kernel's driver on the CPU, compiled here when missing or older than its sources."""
    lib = emulib.library("emu_refine")
    vp, i, n, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    lib.emurf_info.argtypes = [vp]
    lib.emurf_window.argtypes = [n, vp, vp]
    lib.emurf_refine.argtypes = [vp, vp, i, i, i, vp, i, n, vp, vp, i, f, f, i, vp]
    return lib


def emulator_info() -> tuple[int, int, int]:
    """WALK_WAVES, the workgroups of S7 the last refine ran, s7_lds_bytes()."""
    info = (ctypes.c_long * 3)(0, 0, 0)
    emulator().emurf_info(info)
    return tuple(info)


def emulator_g(t) -> np.ndarray:
    t = np.ascontiguousarray(t, np.float64)
    out = np.empty_like(t)
    emulator().emurf_window(t.size, t.ctypes.data, out.ctypes.data)
    return out


EmuError = pc.EmuError


class EmuFinder(pc.EmuFinder):
    """photometry_cases.EmuFinder with ``refine``: regularizepsf_amd.stars._Finder's interface on the emulator."""

    def __init__(self, shape, box, device=0) -> None:
        super().__init__(shape, box, device)
        self._refined = 0

    def refine(self, positions, sigma, max_iter=16, eps=1e-4, max_shift=2.0, use_mesh=True):
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        sigma = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, np.float64), (len(positions),)))
        out = np.empty((len(positions), COLUMNS))
        level = None if self._filtered is None else np.ascontiguousarray(self._filtered[0])
        frame, mask = (self._frame, self._mask) if self._frame is not None else (np.zeros(self.shape, np.float32), None)
        code = emulator().emurf_refine(frame.ctypes.data, None if mask is None else mask.ctypes.data, *self.shape, self.box,
                                       None if level is None else level.ctypes.data, int(level is None), len(positions),
                                       positions.ctypes.data, sigma.ctypes.data, int(max_iter), float(eps), float(max_shift),
                                       int(bool(use_mesh)), out.ctypes.data)
        if code != 0:
            raise EmuError(-1, "bad argument")
        if not self._have_mesh:  # (the library checks its arguments first, then its state)
            raise EmuError(-6, "refine before background_device")
        self._refined = emulator_info()[1]
        return out

    def refine_ms(self) -> float:
        """In the place of the device time: the workgroups of S7 that ran - 0.0 exactly when nothing was launched."""
        return float(self._refined)


# ------------------------------------------------------------------------------------------------------------------ the checks
def run(make_finder, c: dict, times: list | None = None, **iteration):
    """The product's per-frame route on a finder: (the filtered mesh or None, S7's rows)."""
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        level, rms = finder.background(c["frame"], c["mask"])  # the raw mesh of the finder under test (photometry_cases, THE MESH)
        filtered = stars.filter_mesh(level, rms)
        finder.background_device(c["frame"], c["mask"])
        args = {k: c[k] for k in DEFAULTS} | iteration
        rows = finder.refine(c["positions"], c["sigma"], args["max_iter"], args["eps"], args["max_shift"], c["background"] == "mesh")
        if times is not None:
            times.append(finder.refine_ms())
        return (None if filtered is None else filtered[0]), rows
    finally:
        finder.close()


def compare_walk(got: np.ndarray, ref: dict, what: str) -> float:
    """The delivered walk against the restatement's at the same position: the counts exact, the sums within THE BOUND.  The rows must sit at
    the restatement's positions bit for bit (max_iter = 0, or a stop at j = 0).  Returns the worst error / bound."""
    want, bounds = ref["rows"], ref["bounds"]
    assert got.dtype == np.float64 and got.shape == want.shape, f"{what}: {got.shape}, the restatement has {want.shape}"
    if len(want) == 0:
        return 0.0
    assert got[:, :SIGMA + 1].tobytes() == want[:, :SIGMA + 1].tobytes(), f"{what}: the positions or sigma are not the restatement's"
    assert np.array_equal(got[:, NITER:DX + 1], want[:, NITER:DX + 1], equal_nan=True), f"{what}: niter, flags or the step differ"
    assert np.array_equal(got[:, N_USE:N_ALL + 1], want[:, N_USE:N_ALL + 1]), f"{what}: N_use or N_all differ"
    assert np.array_equal(np.isnan(got[:, SUMS]), np.isnan(want[:, SUMS])), f"{what}: NaN in other places"
    err = np.nan_to_num(np.abs(got[:, SUMS] - want[:, SUMS]))
    worst = float(np.max(err[bounds > 0] / bounds[bounds > 0], initial=0.0))
    print(f"{what}: {len(want)} positions, N_all <= {int(want[:, N_ALL].max())}, worst error {err.max():.2e}, worst error / bound {worst:.2e}")
    assert np.all(err <= bounds), what
    return worst


def check_walk(make_finder, name: str) -> float:
    """Check 1: the walk against the restatement, max_iter = 0."""
    c = case(name)
    assert c["max_iter"] == 0
    level_f, rows = run(make_finder, c)
    assert np.all(rows[:, NITER] == 0) and np.all(rows[:, FLAGS] == 0) and np.isnan(rows[:, DY:DX + 1]).all()
    assert rows[:, Y:X + 1].tobytes() == rows[:, Y0:X0 + 1].tobytes() == c["positions"].tobytes()
    return compare_walk(rows, reference(name, level_f), name)


def check_hard_positions(make_finder) -> None:
    """What the hard positions are there for, said from the counts."""
    c = case("walk, mixture, none")
    _, got = run(make_finder, c)
    at = {tuple(p): i for i, p in enumerate(c["positions"].tolist())}
    R = 4.0 * c["sigma"]
    assert np.all(np.abs(got[:, N_ALL] - np.pi * R * R) <= 4 * (R + 1)) and np.all(got[:, N_USE] <= got[:, N_ALL])
    for off in ((-30.0, -30.0), (200.5, 48.0), (48.0, -70.25)):
        i = at[off]
        if R[i] < 30.0:  # wholly off the frame
            assert got[i, N_USE] == 0 and got[i, N_ALL] > 0 and np.all(got[i, SUMS] == 0.0)
    for partly in ((0.0, 0.0), (-1.3, 40.2), (96.7, 50.1), (40.4, -2.2), (33.3, 97.0), (95.0, 95.0)):
        assert 0 < got[at[partly], N_USE] < got[at[partly], N_ALL], partly
    twice = [i for i, p in enumerate(c["positions"].tolist()) if tuple(p) == (60.2, 60.4)]
    assert len(twice) == 2 and c["sigma"][twice[0]] != c["sigma"][twice[1]]  # (the mixture gives them different windows)


def predict(before: np.ndarray, c: dict, j: int) -> np.ndarray:
    """Run j + 1's rows from run j's (max_iter = j), by the rules 2 - 6 of the definition in NumPy float64 on run j's delivered sums."""
    after = before.copy()
    eps2, shift2 = np.float64(c["eps"]) * np.float64(c["eps"]), np.float64(c["max_shift"]) * np.float64(c["max_shift"])
    for i, row in enumerate(before):
        cap = NOT_CONVERGED if j > 0 else 0
        if int(row[FLAGS]) != cap or int(row[NITER]) != j:
            continue  # it stopped before: by convergence (no flag, niter <= j), without flux or by running away - the row stays as it is
        flags = 0
        total = row[S]
        if not np.isfinite(total) or total <= 0.0:
            after[i, FLAGS] = NO_FLUX
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            dy, dx = row[MR] / total, row[MC] / total
            ny, nx = row[Y] + 2.0 * dy, row[X] + 2.0 * dx
            ey, ex = ny - row[Y0], nx - row[X0]
            away = not (np.isfinite(ny) and np.isfinite(nx)) or ey * ey + ex * ex > shift2
        after[i, DY], after[i, DX] = dy, dx
        if away:
            after[i, FLAGS] = RAN_AWAY
            continue
        if not dy * dy + dx * dx < eps2:
            flags = NOT_CONVERGED  # niter == max_iter == j + 1
        after[i, Y], after[i, X], after[i, NITER], after[i, FLAGS] = ny, nx, j + 1, flags
        after[i, N_USE:] = np.nan  # a new position: its walk is run j + 1's own
    return after


def check_chain(make_finder, name: str, J: int = CHAIN_J) -> list[np.ndarray]:
    """Check 2: the chain, bit for bit, from the finder's own rows.  Returns the rows of max_iter = 0 ... J."""
    c = case(name)
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        finder.background_device(c["frame"], c["mask"])
        runs = [finder.refine(c["positions"], c["sigma"], j, c["eps"], c["max_shift"], c["background"] == "mesh") for j in range(J + 1)]
    finally:
        finder.close()
    no_mesh = NO_FLUX if np.isnan(runs[0][:, S]).all() else 0  # (no valid mesh node: flagged before anything iterates)
    assert np.all(runs[0][:, NITER] == 0) and np.all(runs[0][:, FLAGS] == no_mesh) and runs[0][:, Y:X + 1].tobytes() == c["positions"].tobytes()
    moved = 0
    for j in range(J):
        want = predict(runs[j], c, j)
        new = np.isnan(want[:, N_USE])
        moved += int(new.sum())
        assert runs[j + 1][:, :N_USE].tobytes() == want[:, :N_USE].tobytes(), f"{name}: max_iter = {j + 1} is not the rules applied to max_iter = {j}"
        assert runs[j + 1][~new].tobytes() == want[~new].tobytes(), f"{name}: a stopped star's row changed at max_iter = {j + 1}"
    print(f"{name}: {J + 1} runs, {moved} steps predicted bit for bit, niter at the end {runs[-1][:, NITER].astype(int).tolist()}, flags "
          f"{runs[-1][:, FLAGS].astype(int).tolist()}")
    return runs


def chain_condition(name: str, level_f) -> np.ndarray:
    """What the chain's input must satisfy, from the restatement alone: at sigma 1.5 all eight converge in at most 10 iterations, at 2.5 at
    least one stops by convergence and at least one by the cap.  Returns the restatement's rows."""
    rows = reference(name, level_f)["rows"]
    niter, flags = rows[:, NITER].astype(int), rows[:, FLAGS].astype(int)
    print(f"{name}: the restatement's niter {niter.tolist()}, flags {flags.tolist()}")
    if name.endswith("1.5"):
        assert len(rows) == 8 and np.all(flags == 0) and np.all((niter > 0) & (niter <= 10))
    else:
        assert np.any((flags == 0) & (niter > 0)) and np.any(flags == NOT_CONVERGED)
    return rows


def check_chain_case(make_finder, name: str) -> None:
    c = case(name)
    level_f, got = run(make_finder, c)
    ref = chain_condition(name, level_f)
    runs = check_chain(make_finder, name)
    assert runs[c["max_iter"]].tobytes() == got.tobytes() and np.all(runs[-1][:, NITER] > 0)
    # the ends are the restatement's (its trajectory differs in the last places only; none of these stars sits on a rule's edge)
    assert np.array_equal(got[:, NITER:FLAGS + 1], ref[:, NITER:FLAGS + 1])
    truth = field()["truth"]
    off = np.hypot(*(got[:, Y:X + 1] - truth).T)
    print(f"{name}: {np.hypot(*(c['positions'] - truth).T).round(2).tolist()} px off at the start, {off.round(4).tolist()} at the end")
    assert np.all(off[got[:, FLAGS] == 0] < 0.02)  # (noise of 0.3 under stars of 100 ... 400: not a bound on the kernel, a sanity check)


def check_stop_rules(make_finder) -> None:
    """Check 3: every stop rule fires on a case built for it; the chain holds on each, and the ends are the restatement's."""
    ends = {}
    for name in STOP_CASES:
        c = case(name)
        level_f, got = run(make_finder, c)
        ref = reference(name, level_f)["rows"]
        assert np.array_equal(got[:, NITER:FLAGS + 1], ref[:, NITER:FLAGS + 1]), (name, got[:, NITER:FLAGS + 1], ref[:, NITER:FLAGS + 1])
        assert check_chain(make_finder, name, c["max_iter"])[-1].tobytes() == got.tobytes()
        ends[name] = got
        print(f"{name}: niter {got[:, NITER].astype(int).tolist()}, flags {got[:, FLAGS].astype(int).tolist()}")
    got = ends["negative blob"]
    assert np.all(got[:, FLAGS] == NO_FLUX) and np.all(got[:, NITER] == 0) and np.isnan(got[:, DY:DX + 1]).all() and np.all(got[:, S] < 0)
    assert got[:, Y:X + 1].tobytes() == got[:, Y0:X0 + 1].tobytes()
    got, c = ends["faint next to bright"], case("faint next to bright")
    assert np.all(got[:, FLAGS] == RAN_AWAY)
    kept, rejected = got[:, Y:X + 1] - got[:, Y0:X0 + 1], got[:, Y:X + 1] + 2.0 * got[:, DY:DX + 1] - got[:, Y0:X0 + 1]
    assert np.all((kept ** 2).sum(axis=1) <= c["max_shift"] ** 2) and np.all((rejected ** 2).sum(axis=1) > c["max_shift"] ** 2)
    assert np.all(got[:, DX] < 0)  # towards the bright star
    got, c = ends["between two stars"], case("between two stars")  # accepted steps towards the brighter one, then one too far
    assert np.all(got[:, FLAGS] == RAN_AWAY) and np.all(got[:, NITER] > 0) and np.all(got[:, X] < got[:, X0]) and np.all(got[:, DX] < 0)
    kept, rejected = got[:, Y:X + 1] - got[:, Y0:X0 + 1], got[:, Y:X + 1] + 2.0 * got[:, DY:DX + 1] - got[:, Y0:X0 + 1]
    assert np.all((kept ** 2).sum(axis=1) <= c["max_shift"] ** 2) and np.all((rejected ** 2).sum(axis=1) > c["max_shift"] ** 2)
    got = ends["far start, one iteration"]
    assert np.all(got[:, FLAGS] == NOT_CONVERGED) and np.all(got[:, NITER] == 1)
    assert (got[:, Y:X + 1] + 0.0).tobytes() == (got[:, Y0:X0 + 1] + 2.0 * got[:, DY:DX + 1]).tobytes()
    got = ends["off the frame"]
    assert np.all(got[:, FLAGS] == NO_FLUX) and np.all(got[:, N_USE] == 0) and np.all(got[:, N_ALL] > 0) and np.all(got[:, SUMS] == 0.0)
    assert np.all(got[:, NITER] == 0)
    got, c = ends["no valid mesh node"], case("no valid mesh node")
    assert np.all(got[:, FLAGS] == NO_FLUX) and np.all(got[:, NITER] == 0) and np.isnan(got[:, SUMS]).all() and np.isnan(got[:, DY:DX + 1]).all()
    assert got[:, Y:X + 1].tobytes() == c["positions"].tobytes() and np.all(got[:, N_USE] == 0) and np.all(got[:, N_ALL] > 0)
    compare_walk(got, reference("no valid mesh node", None), "no valid mesh node")
    got, c = ends["one workgroup, three ends"], case("one workgroup, three ends")
    assert len(got) == emulator_info()[0]  # one workgroup
    assert got[0, FLAGS] == NO_FLUX and got[0, NITER] == 0  # stops at j = 0
    assert got[1, FLAGS] == 0 and 0 < got[1, NITER] < c["max_iter"]  # converges, and sits the remaining rounds out
    assert got[2, FLAGS] == NOT_CONVERGED and got[2, NITER] == c["max_iter"]  # runs to the cap


def check_row_counts(make_finder, walk_waves: int) -> None:
    """Check 4: 0 ... 2 WALK_WAVES + 1 positions; row i is the same position refined alone; 0 launches nothing."""
    assert ROW_COUNTS == (0, 1, walk_waves - 1, walk_waves, walk_waves + 1, 2 * walk_waves + 1)
    whole = None
    for k in reversed(ROW_COUNTS):
        c, times = case(f"{k} rows"), []
        _, got = run(make_finder, c, times)
        assert got.shape == (k, COLUMNS) and got.dtype == np.float64
        whole = got if whole is None else whole
        assert got.tobytes() == whole[:k].tobytes()  # a row does not depend on its neighbours in the workgroup
        assert (times[0] == 0.0) == (k == 0), (k, times)
    c = case(f"{ROW_COUNTS[-1]} rows")
    assert len(set(whole[:, NITER].tolist())) > 2  # the waves of a workgroup stop at different rounds
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        finder.background_device(c["frame"], c["mask"])
        for i in range(len(whole)):
            alone = finder.refine(c["positions"][i:i + 1], c["sigma"][i:i + 1], c["max_iter"], c["eps"], c["max_shift"], True)
            assert alone.tobytes() == whole[i:i + 1].tobytes(), i
    finally:
        finder.close()


def check_reproducible(make_finder, name: str) -> None:
    """Repeats are bit-equal: on a fresh finder, by a second call on the same frame, and with another call in between."""
    c = case(name)
    _, rows = run(make_finder, c)
    assert run(make_finder, c)[1].tobytes() == rows.tobytes()
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        finder.background_device(c["frame"], c["mask"])
        args = (c["positions"], c["sigma"], c["max_iter"], c["eps"], c["max_shift"], c["background"] == "mesh")
        one = finder.refine(*args)
        other = finder.refine(c["positions"][::-1], 3.0, 2, 1e-2, 1.0, False)  # other rows and rules in the same buffers
        two = finder.refine(*args)
        assert one.tobytes() == two.tobytes() == rows.tobytes() and other.shape == (len(c["positions"]), COLUMNS)
    finally:
        finder.close()


def check_isolation(make_finder) -> None:
    """detect, measure and photometry give the bits they gave before a refine, and a refine's rows do not depend on them."""
    c = case("chain, sigma 1.5")
    radii = (2.0, 4.0, 8.0)
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        finder.background_device(c["frame"], c["mask"])
        rows = finder.detect_device(3.0, 5, None)
        shapes = finder.measure()
        phot = finder.photometry(rows[:, :2], radii, 5, True)
        assert len(rows) == 8
        refined = finder.refine(rows[:, :2], 1.5)
        assert finder.measure().tobytes() == shapes.tobytes()
        assert finder.photometry(rows[:, :2], radii, 5, True).tobytes() == phot.tobytes()
        finder.refine(c["positions"], 16.0, 3, 1e-3, 64.0, False)
        assert finder.measure().tobytes() == shapes.tobytes()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes()
        assert finder.refine(rows[:, :2], 1.5).tobytes() == refined.tobytes()
        finder.background_device(c["frame"], c["mask"])  # the refine first, the others after it
        assert finder.refine(rows[:, :2], 1.5).tobytes() == refined.tobytes()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes() and finder.measure().tobytes() == shapes.tobytes()
        assert finder.photometry(rows[:, :2], radii, 5, True).tobytes() == phot.tobytes()
    finally:
        finder.close()


def check_errors(make_finder, error: type) -> None:
    """RPSF_E_STATE (-6) before a background_device of a frame and after the host route's detect; RPSF_E_BADARG (-1) for a bad sigma,
    max_iter, eps, max_shift or position, whatever the state."""
    import pytest

    c = case("chain, sigma 1.5")
    p = c["positions"]
    good = (p, 1.5, 16, 1e-4, 2.0, True)
    bad = [(p, 0.49, 16, 1e-4, 2.0, True), (p, 16.5, 16, 1e-4, 2.0, True), (p, np.nan, 16, 1e-4, 2.0, True), (p, -1.0, 16, 1e-4, 2.0, True),
           (p, np.r_[np.full(7, 1.5), 0.0], 16, 1e-4, 2.0, True), (p, 1.5, -1, 1e-4, 2.0, True), (p, 1.5, 65, 1e-4, 2.0, True),
           (p, 1.5, 16, 0.0, 2.0, True), (p, 1.5, 16, -1e-4, 2.0, True), (p, 1.5, 16, np.nan, 2.0, True), (p, 1.5, 16, np.inf, 2.0, True),
           (p, 1.5, 16, 1e-4, 0.0, True), (p, 1.5, 16, 1e-4, 64.5, True), (p, 1.5, 16, 1e-4, np.nan, False),
           ([(np.nan, 1.0)], 1.5, 16, 1e-4, 2.0, True), ([(1.0, np.inf)], 1.5, 16, 1e-4, 2.0, True), ([(2.0 ** 20, 1.0)], 1.5, 16, 1e-4, 2.0, True),
           ([(1.0, 1.0), (1.0, -2.0 ** 20)], 1.5, 16, 1e-4, 2.0, False)]
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        def refused(args, code):
            with pytest.raises(error) as caught:
                finder.refine(*args)
            assert caught.value.code == code, (args[1:], caught.value.code)

        refused(good, -6)
        for args in bad:
            refused(args, -1)
        level, rms = finder.background(c["frame"], c["mask"])  # the host route: no S1b mesh on the device
        refused(good, -6)
        finder.background_device(c["frame"], c["mask"])
        for args in bad:
            refused(args, -1)
        rows = finder.refine(*good)
        assert finder.refine([(2.0 ** 20 - 1, 1.0 - 2.0 ** 20)], 16.0, 64, 1e-300, 64.0, True).shape == (1, COLUMNS)  # the largest admitted
        assert finder.refine(p[:1], 0.5, 0, 1e-4, 2.0 ** -20, True).shape == (1, COLUMNS)
        level_f, _, global_rms = stars.filter_mesh(level, rms)
        finder.detect(level_f, 3.0 * global_rms, 5, None)  # the host route's detect replaces the mesh on the device
        refused(good, -6)
        finder.background_device(c["frame"], c["mask"])
        assert finder.refine(*good).tobytes() == rows.tobytes()
    finally:
        finder.close()


def check_g() -> float:
    """g: the emulator's against the restatement bit for bit, the restatement against exp in np.longdouble within G_BOUND, on a dense grid
    of [0, 8] and at the ties of n.  Returns the worst relative error in units of u."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is not wider than float64 here"
    ln2 = np.log(np.longdouble(2.0))
    assert abs(ln2 - np.longdouble(LN2_HI) - np.longdouble(LN2_LO)) <= np.longdouble(2.0) ** -64
    rng = np.random.default_rng([7, 67])
    ties = (np.arange(0, 13)[:, None] + 0.5) * float(ln2) + np.arange(-8, 9)[None, :] * 2.0 ** -50
    t = np.concatenate([np.linspace(0.0, 8.0, 400001), rng.uniform(0.0, 8.0, 400000), ties.ravel().clip(0.0, 8.0), [0.0, 8.0, np.nextafter(8.0, 9.0)]])
    n = np.floor(t * LOG2E + 0.5)
    assert np.all(np.abs((t - n * LN2_HI) - n * LN2_LO) <= G_REDUCED) and n.max() == 12
    got = ref_g(t)
    assert emulator_g(t).tobytes() == got.tobytes()
    want = np.exp(-t.astype(np.longdouble))
    worst = float(np.max(np.abs(got.astype(np.longdouble) - want) / want))
    print(f"g: {len(t)} points of [0, 8], worst relative error {worst / U:.3f} u, bound {G_BOUND / U:.3f} u")
    assert worst <= G_BOUND
    assert ref_g(0.0) == 1.0
    return worst / U


# ------------------------------------------------------------------------------------------------------------------ the truth
# photometry_cases.truth_case's noise-free Gaussians (amplitude 1000, sigma 1.2, 1.7, 2.3 at fractional positions), refined on the
# restatement alone with background="none" from starts TRUTH_OFFSET (up to 0.5 px) away, the window's sigma the star's own, the defaults
# for the rest.  On those the restatement's worst errors are MEASURED_*.  The position's error is what the last step, below eps = 1e-4,
# leaves, plus the pixel lattice's; the corrected moments assume the continuous, untruncated window, and the window is cut at 4 sigma and
# sampled at pixel centres: that discretisation, not rounding, is what the moments' figure shows.  The asserted bounds are the measured
# figures times TRUTH_MARGIN = 2, as in photometry_cases.
MEASURED_POSITION = 1.37e-05  # pixels: sigma 1.2, the narrowest star on the lattice (5.3e-7 for 1.7, 1e-12 for 2.3); two iterations each
MEASURED_MOMENTS = 5.94e-05  # |rr - sigma^2| / sigma^2 and |cc - sigma^2| / sigma^2: sigma 1.2 again (4.2e-6 for 1.7, 2.9e-6 for 2.3)
TRUTH_MARGIN = 2.0


def check_truth() -> tuple[float, float]:
    """The definition itself on the restatement alone; returns the worst position error (pixels) and moment error (relative)."""
    t = pc.truth_case()
    sigma = np.array(pc.TRUTH_SIGMAS)
    ref = ref_refine(t["frame"], None, BOX, None, t["positions"], sigma, "none")
    cat = stars.refine_from_sums(ref["rows"])
    assert np.all(cat["converged"]) and np.all(cat["niter"] <= 10)
    position = np.hypot(cat["row"] - t["centres"][:, 0], cat["col"] - t["centres"][:, 1])
    moments = np.maximum(np.abs(cat["rr"] - sigma ** 2), np.abs(cat["cc"] - sigma ** 2)) / sigma ** 2
    print(f"truth: niter {cat['niter'].tolist()}, positions off by {position} pixels: worst {position.max():.2e} (measured {MEASURED_POSITION}); "
          f"rr, cc {cat['rr']}, {cat['cc']} against {sigma ** 2}: worst relative error {moments.max():.2e} (measured {MEASURED_MOMENTS})")
    assert position.max() <= TRUTH_MARGIN * MEASURED_POSITION and moments.max() <= TRUTH_MARGIN * MEASURED_MOMENTS
    assert np.all(np.abs(cat["rc"]) < 1e-3 * sigma ** 2) and np.all(cat["elongation"] < 1.01) and np.all(cat["coverage"] == 1.0)
    return float(position.max()), float(moments.max())
