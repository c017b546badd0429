"""Fitted positions (DESIGN.md 3.7 "Fitted positions", kernel S9) restated in float64 NumPy, the cases, the CPU emulator of the kernel, and
the checks the emulator tests (tests/test_fitpos_host.py) and the GPU tests (tests/test_gpu_fitpos.py) share.

There is no outside implementation: the reference is the restatement below, written from the definition in include/rpsf.h, one star at a
time.  A check takes `make_finder(shape, box)` and `make_model(values)`: regularizepsf_amd.stars._Finder and ._Model on the GPU, EmuFinder
and fit_cases.EmuModel here.

BIT FOR BIT.  Kernel, emulator and restatement agree in every bit of every iteration row, because the restatement does the kernel's float64
operations in the kernel's order: the mesh, the residual d and the sums are fit_cases' (`ordered_sum`; a pixel the kernel skips enters as
+ 0.0), the model m and its gradient (g_u, g_v) are one expression of + - x each (`ref_sample`), the elimination is scalar float64
arithmetic in the definition's order (`ref_solve`), and the stop rules follow in the definition's sequence.  The fit rows are S8's own:
they are compared with fit_cases.ref_fit and with the finder's own `fit` at the positions returned.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np

from tests import emulib
from regularizepsf_amd import stars
from tests import fit_cases as fc
from tests import photometry_cases as pc
from tests import star_cases as sc

ROOT = sc.ROOT
COLUMNS = 8
Y0, X0, Y, X, NITER, FLAGS, DY, DX = range(COLUMNS)
RAN_AWAY, NOT_CONVERGED, SINGULAR, SKIPPED = 1, 2, 4, 8
DEFAULTS = {"max_iter": 16, "eps": 1e-4, "max_shift": 2.0, "max_step": 0.5}
SHAPE, BOX = fc.SHAPE, fc.BOX


# ------------------------------------------------------------------------------------------------------------------ the restatement
def ref_sample(cell: np.ndarray, pr: np.ndarray, pc_: np.ndarray, inside: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(m, g_u, g_v) of the definition on the box pr x pc, operation for operation; 0.0 outside `inside`."""
    n = cell.shape[0]
    h = np.float64(n / 2.0 - 0.5)
    u, v = pr + h, pc_ + h
    fu, fv = np.floor(u), np.floor(v)
    a, b = (u - fu)[:, None], (v - fv)[None, :]
    i, j = np.clip(fu.astype(np.int64), 0, n - 2)[:, None], np.clip(fv.astype(np.int64), 0, n - 2)[None, :]
    rows_ok, cols_ok = (fu >= 0) & (fu <= n - 2), (fv >= 0) & (fv <= n - 2)
    assert np.all(~inside | (rows_ok[:, None] & cols_ok[None, :])), "a pixel of the disc has a model sample outside the cell"
    c00, c01, c10, c11 = cell[i, j], cell[i, j + 1], cell[i + 1, j], cell[i + 1, j + 1]
    with np.errstate(all="ignore"):
        m = ((1.0 - a) * ((1.0 - b) * c00 + b * c01)) + (a * ((1.0 - b) * c10 + b * c11))
        gu = ((1.0 - b) * (c10 - c00)) + (b * (c11 - c01))
        gv = ((1.0 - a) * (c01 - c00)) + (a * (c11 - c10))
    return np.where(inside, m, 0.0), np.where(inside, gu, 0.0), np.where(inside, gv, 0.0)


def ref_solve(A: list, b: list) -> list | None:
    """The LDL^T elimination of the definition on the upper triangle of A (K x K scalars) and b; None at a pivot that is not finite or <= 0."""
    K = len(b)
    A, b = [list(row) for row in A], list(b)
    for j in range(K):
        pivot = A[j][j]
        if not np.isfinite(pivot) or pivot <= 0.0:
            return None
        for i in range(j + 1, K):
            l = A[j][i] / pivot
            for c in range(i, K):
                A[i][c] = A[i][c] - l * A[j][c]
            b[i] = b[i] - l * b[j]
    x = [None] * K
    for j in range(K - 1, -1, -1):
        s = b[j]
        for c in range(j + 1, K):
            s = s - A[j][c] * x[c]
        x[j] = s / A[j][j]
    return x


def ref_walk(d, ok, cell, y, x, R, fit_background: bool):
    """One walk at (y, x) and the solve: (dy, dx) not yet clamped, or None (SINGULAR by count or by a pivot)."""
    H, W = d.shape
    R2 = R * R
    rr = np.arange(int(np.floor(y - R)) - 1, int(np.ceil(y + R)) + 2)
    cc = np.arange(int(np.floor(x - R)) - 1, int(np.ceil(x + R)) + 2)
    pr, pc_ = rr.astype(np.float64) - y, cc.astype(np.float64) - x
    disc = ((pr * pr)[:, None] + (pc_ * pc_)[None, :]) <= R2
    on_frame = ((rr >= 0) & (rr < H))[:, None] & ((cc >= 0) & (cc < W))[None, :]
    ri, ci = np.clip(rr, 0, H - 1), np.clip(cc, 0, W - 1)
    use = disc & on_frame & ok[ri[:, None], ci[None, :]]
    n = int(use.sum())
    m, gu, gv = ref_sample(cell, pr, pc_, use)
    dv = np.where(use, d[ri[:, None], ci[None, :]], 0.0)
    with np.errstate(all="ignore"):
        terms = (m * m, m, m * gu, m * gv, gu, gv, gu * gu, gu * gv, gv * gv, dv * m, dv, dv * gu, dv * gv)
        Smm, Sm, Smu, Smv, Su, Sv, Suu, Suv, Svv, Sdm, Sd, Sdu, Sdv = (fc.ordered_sum(t) for t in terms)
        if fit_background:
            A = [[Smm, Sm, Smu, Smv], [None, np.float64(n), Su, Sv], [None, None, Suu, Suv], [None, None, None, Svv]]
            b = [Sdm, Sd, Sdu, Sdv]
        else:
            A = [[Smm, Smu, Smv], [None, Suu, Suv], [None, None, Svv]]
            b = [Sdm, Sdu, Sdv]
        if n < len(b):
            return None
        solved = ref_solve(A, b)
        if solved is None:
            return None
        return -solved[-2] / solved[0], -solved[-1] / solved[0]


def ref_fit_positions(frame, mask, box, level_f, cube, positions, cells, radius, fit_background: bool, background: str, max_iter=16,
                      eps=1e-4, max_shift=2.0, max_step=0.5) -> np.ndarray:
    """The definition: (k, COLUMNS) iteration rows in the kernel's layout."""
    d, ok = pc.ref_residual(frame, mask, box, level_f, background)
    cube = np.asarray(cube, np.float64)
    no_mesh = background == "mesh" and level_f is None
    positions = np.asarray(positions, np.float64).reshape(-1, 2)
    R, eps2, shift2, step = np.float64(radius), np.float64(eps) * np.float64(eps), np.float64(max_shift) * np.float64(max_shift), np.float64(max_step)
    rows = np.empty((len(positions), COLUMNS))
    for row, (y0, x0), k in zip(rows, positions, np.asarray(cells, np.int64)):
        y, x, niter, flags, last = y0, x0, 0, 0, (np.nan, np.nan)
        if no_mesh or not 0 <= k < len(cube):
            flags = SKIPPED
        else:
            while niter < max_iter:
                with np.errstate(all="ignore"):
                    move = ref_walk(d, ok, cube[k], y, x, R, fit_background)
                    if move is None or not np.isfinite(move[0]) or not np.isfinite(move[1]):
                        flags |= SINGULAR
                        break
                    dy, dx = (step if v > step else -step if v < -step else v for v in move)
                    last = (dy, dx)
                    ny, nx = y + dy, x + dx
                    ey, ex = ny - y0, nx - x0
                    if ey * ey + ex * ex > shift2:
                        flags |= RAN_AWAY
                        break
                    y, x, niter = ny, nx, niter + 1
                    if dy * dy + dx * dx < eps2:
                        break
                    if niter == max_iter:
                        flags |= NOT_CONVERGED
        row[:] = y0, x0, y, x, niter, flags, *last
    return rows


same_bits = fc.same_bits

# ------------------------------------------------------------------------------------------------------------------ the cases
STAR = (20.3, 17.6)  # fit_cases.STARS[0]


def starts() -> tuple[np.ndarray, np.ndarray]:
    """(positions, cells): every star of the field from 0.3 px off; starts on pixel centres and at exact half pixels (a or b = 0 for even
    N, the floor's edge); one a pixel off on one axis (the first step is clamped on that axis only); the other cells, all-zero and constant
    among them, and indices outside the cube; the frame's rim and a start off the frame."""
    G, Z, L, C = fc.GAUSSIAN, fc.ZERO, fc.LOBES, fc.CONSTANT
    rows = [(*(fc.STARS[i] + (0.3, -0.3)), G) for i in range(5)]
    rows += [(20.0, 18.0, G), (12.0, 30.0, G), (20.5, 17.5, G), (33.5, 10.5, G), (20.0, 17.5, G), (21.3, 17.6, G), (20.3, 16.5, G),
             (20.5, 17.5, L), (20.0, 18.0, C), (20.0, 18.0, Z), (20.0, 18.0, -1), (20.0, 18.0, 4), (0.0, 0.0, G), (47.0, 39.0, G), (47.5, 3.25, L),
             (-30.0, -30.0, G)]
    table = np.array(rows, np.float64)
    return np.ascontiguousarray(table[:, :2]), table[:, 2].astype(np.int32)


def _case(frame, positions, cells, n, background="mesh", fit_background=True, mask=None, radii=None, box=BOX, cube=None, **iteration) -> dict:
    c = fc._case(frame, positions, cells, n, background, fit_background, mask, radii, box, cube)
    return c | {"iteration": DEFAULTS | iteration}


def _grid_case(n, background, fit_background) -> dict:
    return _case(fc.field()["frame"], *starts(), n, background, fit_background)


def _masked_case(background, fit_background) -> dict:
    m = fc.masked_field()
    return _case(m["frame"], *starts(), 9, background, fit_background, m["mask"])


@functools.cache
def settled() -> np.ndarray:
    """Where the restatement ends from STAR with the 9-pixel Gaussian cell, R = 3.5, background="none" and the defaults."""
    rows = ref_fit_positions(fc.field()["frame"], None, BOX, None, fc.model(9), [STAR], [fc.GAUSSIAN], 3.5, True, "none")
    assert rows[0, FLAGS] == 0 and rows[0, NITER] > 0
    return rows[0, Y:X + 1].copy()


def fates() -> tuple[np.ndarray, np.ndarray]:
    """Four stars of one workgroup for max_iter = 2, max_shift = 0.25: one that converges (it starts 0.001 px from where the iteration
    settles), one that does not within two steps (0.2 px off), one that runs away (1 px off: the clamped first step of 0.5 is beyond
    max_shift) and one that is skipped (cell -1)."""
    p = settled()
    positions = np.array([p + (1e-3, -1e-3), p + (0.15, -0.12), p + (1.0, 0.0), p])
    return positions, np.array([fc.GAUSSIAN, fc.GAUSSIAN, fc.GAUSSIAN, -1], np.int32)


FATES = {"max_iter": 2, "max_shift": 0.25}
ROW_COUNTS = fc.ROW_COUNTS  # 0, 1, WALK_WAVES - 1, WALK_WAVES, WALK_WAVES + 1, 2 WALK_WAVES + 1


def _row_case(k: int) -> dict:
    """The four fates, a singular star, three more, and in the last workgroup alone a star that iterates to the cap."""
    p, c = fates()
    positions = np.concatenate([p, [(20.0, 18.0)], fc.STARS[1:4] + (0.2, 0.1), [p[1]]])[:k]
    cells = np.concatenate([c, [fc.ZERO], [fc.GAUSSIAN, fc.LOBES, fc.GAUSSIAN], [fc.GAUSSIAN]]).astype(np.int32)[:k]
    return _case(fc.field()["frame"], positions, cells, 9, "none", radii=(3.5,), **FATES)


def _nan_cube() -> np.ndarray:
    return np.where(np.arange(4)[:, None, None] == fc.ZERO, np.nan, fc.model(9))


GRID_CASES = {f"N = {n}, {b}, {'flux and background' if fb else 'flux alone'}": functools.partial(_grid_case, n, b, fb)
              for n in fc.SIZES for b in ("mesh", "none") for fb in (True, False)}
MASKED_CASES = {f"masked, {b}, {'flux and background' if fb else 'flux alone'}": functools.partial(_masked_case, b, fb)
                for b in ("mesh", "none") for fb in (True, False)}
OTHER_CASES = {
    "four fates": lambda: _case(fc.field()["frame"], *fates(), 9, "none", radii=(3.5,), **FATES),
    "no valid mesh node": lambda: _case(np.full(SHAPE, np.nan, np.float32), [(30.2, 20.7), (0.0, 0.0), (-30.0, -30.0), (10.0, 10.0)],
                                        [fc.GAUSSIAN, fc.GAUSSIAN, fc.LOBES, 7], 9, radii=(3.5,)),
    "all NaN, none": lambda: _case(np.full(SHAPE, np.nan, np.float32), [(30.2, 20.7), (0.0, 0.0)], [fc.GAUSSIAN, 4], 9, "none", radii=(3.5,)),
    "a cell of NaN": lambda: _case(fc.field()["frame"], np.repeat(fc.STARS[:2] + 0.25, 3, axis=0), [fc.GAUSSIAN, fc.ZERO, fc.LOBES] * 2, 9,
                                   radii=(3.5,), cube=_nan_cube()),
    "one step, clamped on one axis": lambda: _case(fc.field()["frame"], [(21.3, 17.6), (20.3, 16.5), (21.4, 18.7)], [fc.GAUSSIAN] * 3, 9, "none",
                                                   radii=(3.5,), max_iter=1),
    "no iteration": lambda: _case(fc.field()["frame"], *starts(), 9, radii=(3.5,), max_iter=0),
    "a short step and a wide eps": lambda: _case(fc.field()["frame"], *starts(), 16, radii=(4.6,), max_iter=3, eps=0.01, max_shift=0.4,
                                                 max_step=0.125),
    "box 8": lambda: _case(fc.field()["frame"], fc.STARS + (0.3, 0.2), [fc.GAUSSIAN] * 5, 16, radii=(7.0,), box=8),
}
ROW_CASES = {f"{k} rows": functools.partial(_row_case, k) for k in ROW_COUNTS}
CASES = {**GRID_CASES, **MASKED_CASES, **OTHER_CASES, **ROW_CASES}


@functools.cache
def case(name: str) -> dict:
    return sc._freeze(CASES[name]())


@functools.lru_cache(maxsize=None)
def _reference(name: str, mesh_bytes: bytes | None, radius: float) -> tuple[np.ndarray, np.ndarray]:
    c = case(name)
    level_f = None if mesh_bytes is None else np.frombuffer(mesh_bytes).reshape(-(-c["frame"].shape[0] // c["box"]), -(-c["frame"].shape[1] // c["box"]))
    common = (c["frame"], c["mask"], c["box"], level_f, c["cube"])
    steps = ref_fit_positions(*common, c["positions"], c["cells"], radius, c["fit_background"], c["background"], **c["iteration"])
    fits = fc.ref_fit(*common, steps[:, Y:X + 1], c["cells"], radius, c["fit_background"], c["background"])
    steps.flags.writeable = fits.flags.writeable = False
    return steps, fits


def reference(name: str, level_f, radius: float) -> tuple[np.ndarray, np.ndarray]:
    """The restatement's (iteration rows, fit rows) for the case on the filtered mesh `level_f` (None: no valid node), computed once."""
    mesh = None if level_f is None or case(name)["background"] == "none" else np.ascontiguousarray(level_f).tobytes()
    return _reference(name, mesh, float(radius))


# ------------------------------------------------------------------------------------------------------------------ the emulator
@functools.cache
def emulator():
    """tests/emu/libemu_fitpos.so: the kernel's driver on the CPU, compiled here when missing or older than its sources."""
    lib = emulib.library("emu_fitpos")
    vp, i, n, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    lib.emufp_info.argtypes = [vp]
    lib.emufp_fit_positions.argtypes = [vp, vp, i, i, i, vp, i, n, i, vp, n, vp, vp, f, i, i, f, f, f, i, vp, vp]
    return lib


def emulator_info() -> tuple[int, int, int]:
    """WALK_WAVES, the workgroups of S9 the last fit_positions ran, s9_lds_bytes()."""
    info = (ctypes.c_long * 3)(0, 0, 0)
    emulator().emufp_info(info)
    return tuple(info)


EmuError, EmuModel = fc.EmuError, fc.EmuModel


class EmuFinder(fc.EmuFinder):
    """fit_cases.EmuFinder with ``fit_positions``: regularizepsf_amd.stars._Finder's interface on the emulator."""

    def __init__(self, shape, box, device=0) -> None:
        super().__init__(shape, box, device)
        self._positioned = 0

    def fit_positions(self, model, positions, cells, radius, fit_background=True, max_iter=16, eps=1e-4, max_shift=2.0, max_step=0.5,
                      use_mesh=True):
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        cells = np.ascontiguousarray(cells, np.int32).ravel()
        if len(cells) != len(positions):
            raise ValueError(f"{len(cells)} cells for {len(positions)} positions")
        steps, fits = np.empty((len(positions), COLUMNS)), np.empty((len(positions), fc.COLUMNS))
        level = None if self._filtered is None else np.ascontiguousarray(self._filtered[0])
        frame, mask = (self._frame, self._mask) if self._frame is not None else (np.zeros(self.shape, np.float32), None)
        code = emulator().emufp_fit_positions(frame.ctypes.data, None if mask is None else mask.ctypes.data, *self.shape, self.box,
                                              None if level is None else level.ctypes.data, int(level is None), len(model.values), model.size,
                                              model.values.ctypes.data, len(positions), positions.ctypes.data, cells.ctypes.data, float(radius),
                                              int(bool(fit_background)), int(max_iter), float(eps), float(max_shift), float(max_step),
                                              int(bool(use_mesh)), steps.ctypes.data, fits.ctypes.data)
        if code != 0 or model.device != self._device:
            raise EmuError(-1, "bad argument")
        if not self._have_mesh:  # (the library checks its arguments first, then its state)
            raise EmuError(-6, "fit_positions before background_device")
        self._positioned = emulator_info()[1]
        return steps, fits

    def fit_positions_ms(self) -> float:
        """In the place of the device time: the workgroups of S9 that ran - 0.0 exactly when nothing was launched."""
        return float(self._positioned)


# ------------------------------------------------------------------------------------------------------------------ the checks
def run(make_finder, make_model, c: dict, times: list | None = None, also_fit: bool = False) -> tuple:
    """The product's per-frame route on a finder: (the filtered mesh or None, {radius: (iteration rows, fit rows)}); with `also_fit` a
    third entry per radius, the finder's own `fit` at the positions returned."""
    finder, model = make_finder(c["frame"].shape, c["box"]), None
    try:
        model = make_model(c["cube"])
        level, rms = finder.background(c["frame"], c["mask"])  # the raw mesh of the finder under test (photometry_cases, THE MESH)
        filtered = stars.filter_mesh(level, rms)
        finder.background_device(c["frame"], c["mask"])
        rows, it, mesh = {}, c["iteration"], c["background"] == "mesh"
        for radius in c["radii"]:
            got = finder.fit_positions(model, c["positions"], c["cells"], radius, c["fit_background"], it["max_iter"], it["eps"], it["max_shift"],
                                       it["max_step"], mesh)
            if times is not None:
                times.append(finder.fit_positions_ms())
            if also_fit:
                got = (*got, finder.fit(model, got[0][:, Y:X + 1], c["cells"], radius, c["fit_background"], mesh))
            rows[radius] = got
        return (None if filtered is None else filtered[0]), rows
    finally:
        if model is not None:
            model.close()
        finder.close()


def check_case(make_finder, make_model, name: str) -> dict:
    """Checks 1 and 2: every iteration row of every radius of the case against the restatement, bit for bit; every fit row against
    fit_cases.ref_fit and against the finder's own S8 at the position returned, likewise.  Returns {radius: (iteration rows, fit rows)}."""
    c = case(name)
    level_f, rows = run(make_finder, make_model, c, also_fit=True)
    for radius, (steps, fits, own) in rows.items():
        want_steps, want_fits = reference(name, level_f, radius)
        assert steps.dtype == np.float64 and steps.shape == want_steps.shape and fits.shape == want_fits.shape
        flags = steps[:, FLAGS].astype(int)
        differ = [i for i in range(len(steps)) if not same_bits(steps[i], want_steps[i])]
        print(f"{name}, R = {radius:g}: {len(steps)} rows, flags {sorted(set(flags.tolist()))}, niter <= {int(steps[:, NITER].max(initial=0))}, "
              f"{int(((flags == 0) & (steps[:, NITER] > 0)).sum())} converged, {len(differ)} rows differ from the restatement")
        assert not differ, (name, radius, differ[:3], steps[differ[0]], want_steps[differ[0]])
        assert fits.tobytes() == own.tobytes(), (name, radius)  # S8 itself at the position returned
        differ = [i for i in range(len(fits)) if not same_bits(fits[i], want_fits[i])]
        assert not differ, (name, radius, differ[:3], fits[differ[0]], want_fits[differ[0]])
        assert fits[:, fc.Y:fc.X + 1].tobytes() == steps[:, Y:X + 1].tobytes()
    return {radius: got[:2] for radius, got in rows.items()}


def check_no_iteration(make_finder, make_model) -> None:
    """max_iter = 0: both outputs are the plain S8 call at the input; no flag but SKIPPED."""
    c = case("no iteration")
    finder, model = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"])
    try:
        finder.background_device(c["frame"], c["mask"])
        steps, fits = finder.fit_positions(model, c["positions"], c["cells"], 3.5, True, 0)
        assert fits.tobytes() == finder.fit(model, c["positions"], c["cells"], 3.5).tobytes()
        assert steps[:, Y0:X0 + 1].tobytes() == steps[:, Y:X + 1].tobytes() == c["positions"].tobytes()
        bad = (c["cells"] < 0) | (c["cells"] >= 4)
        assert np.all(steps[:, NITER] == 0) and np.isnan(steps[:, DY:]).all() and bad.any()
        assert steps[:, FLAGS].astype(int).tolist() == np.where(bad, SKIPPED, 0).tolist()
    finally:
        model.close()
        finder.close()


def check_every_stop_rule(make_finder, make_model) -> None:
    """Check 3: four fates in one workgroup, the singular cells, a star off the frame and a frame without a mesh; and what the hard starts
    are there for."""
    steps, fits = run(make_finder, make_model, case("four fates"))[1][3.5]
    p = settled()
    print(f"four fates: flags {steps[:, FLAGS].astype(int).tolist()}, niter {steps[:, NITER].astype(int).tolist()}, last steps "
          f"{np.hypot(steps[:, DY], steps[:, DX]).tolist()}")
    assert steps[:, FLAGS].astype(int).tolist() == [0, NOT_CONVERGED, RAN_AWAY, SKIPPED]
    assert steps[:, NITER].astype(int).tolist() == [2, 2, 0, 0]
    assert np.hypot(*(steps[0, Y:X + 1] - p)) < 1e-4 and np.hypot(steps[0, DY], steps[0, DX]) < 1e-4
    assert np.hypot(*(steps[1, Y:X + 1] - p)) < 0.02 and np.hypot(steps[1, DY], steps[1, DX]) >= 1e-4  # close, and not yet there
    assert steps[2, Y:X + 1].tobytes() == steps[2, Y0:X0 + 1].tobytes() and steps[2, DY] == -0.5 and abs(steps[2, DX]) < 0.5  # the rejected step
    assert steps[3, Y:X + 1].tobytes() == steps[3, Y0:X0 + 1].tobytes() and np.isnan(steps[3, DY:]).all()
    assert fits[:, fc.FLAGS].astype(int).tolist() == [0, 0, 0, fc.BAD_CELL]
    for name in ("N = 9, none, flux and background", "N = 9, none, flux alone"):
        c = case(name)
        at = lambda p, k: next(i for i, (q, j) in enumerate(zip(c["positions"].tolist(), c["cells"].tolist())) if tuple(q) == p and j == k)  # noqa: E731
        for radius, (steps, fits) in run(make_finder, make_model, c)[1].items():
            flags, niter = steps[:, FLAGS].astype(int), steps[:, NITER].astype(int)
            for i in (at((20.0, 18.0), fc.ZERO), at((20.0, 18.0), fc.CONSTANT), at((-30.0, -30.0), fc.GAUSSIAN)):  # a pivot <= 0; no pixel
                assert flags[i] == SINGULAR and niter[i] == 0 and np.isnan(steps[i, DY:]).all()
                assert steps[i, Y:X + 1].tobytes() == steps[i, Y0:X0 + 1].tobytes()
            assert fits[at((-30.0, -30.0), fc.GAUSSIAN), fc.FLAGS] == fc.TOO_FEW
            for k in (-1, 4):
                assert flags[at((20.0, 18.0), k)] == SKIPPED and fits[at((20.0, 18.0), k), fc.FLAGS] == fc.BAD_CELL
            if radius >= 2.0:  # every star of the field is found again from 0.3 px off, whatever the sub-pixel phase of the start
                ends = steps[:5, Y:X + 1]
                assert np.all(flags[:5] == 0) and np.all(niter[:5] > 0) and np.all(np.hypot(*(ends - fc.STARS).T) < 0.1), ends
                for i in (at((20.0, 18.0), fc.GAUSSIAN), at((20.5, 17.5), fc.GAUSSIAN), at((20.0, 17.5), fc.GAUSSIAN), at((21.3, 17.6), fc.GAUSSIAN)):
                    assert flags[i] == 0 and np.hypot(*(steps[i, Y:X + 1] - STAR)) < 0.1, (i, steps[i])
    steps, _ = run(make_finder, make_model, case("one step, clamped on one axis"))[1][3.5]
    assert steps[:, NITER].astype(int).tolist() == [1, 1, 1] and steps[:, FLAGS].astype(int).tolist() == [NOT_CONVERGED] * 3
    assert steps[0, DY] == -0.5 and abs(steps[0, DX]) < 0.25 and steps[1, DX] == 0.5 and abs(steps[1, DY]) < 0.25
    assert steps[2, DY] == -0.5 and steps[2, DX] == -0.5
    assert np.array_equal(steps[:, Y], steps[:, Y0] + steps[:, DY]) and np.array_equal(steps[:, X], steps[:, X0] + steps[:, DX])
    steps, fits = run(make_finder, make_model, case("no valid mesh node"))[1][3.5]
    assert steps[:, FLAGS].astype(int).tolist() == [SKIPPED] * 4 and np.all(steps[:, NITER] == 0)
    assert fits[:, fc.FLAGS].astype(int).tolist() == [fc.NO_MESH] * 3 + [fc.NO_MESH | fc.BAD_CELL]
    steps, _ = run(make_finder, make_model, case("all NaN, none"))[1][3.5]
    assert steps[:, FLAGS].astype(int).tolist() == [SINGULAR, SKIPPED]
    steps, fits = run(make_finder, make_model, case("a cell of NaN"))[1][3.5]
    assert steps[:, FLAGS].astype(int).tolist() == [0, SINGULAR, 0] * 2 and fits[:, fc.FLAGS].astype(int).tolist() == [0, fc.DEGENERATE, 0] * 2
    steps, _ = run(make_finder, make_model, case("a short step and a wide eps"))[1][4.6]
    seen = set(steps[:, FLAGS].astype(int).tolist())
    print(f"a short step and a wide eps: flags {sorted(seen)}, niter {sorted(set(steps[:, NITER].astype(int).tolist()))}")
    assert {0, RAN_AWAY, NOT_CONVERGED, SINGULAR, SKIPPED} <= seen and np.nanmax(np.abs(steps[:, DY:])) == 0.125


def check_row_counts(make_finder, make_model, walk_waves: int) -> None:
    """Check 3, around a workgroup: 0 ... 2 WALK_WAVES + 1 stars of different fates; row i is the same star run alone; 0 launches nothing."""
    assert ROW_COUNTS == (0, 1, walk_waves - 1, walk_waves, walk_waves + 1, 2 * walk_waves + 1)
    whole = None
    for k in reversed(ROW_COUNTS):
        c, times = case(f"{k} rows"), []
        steps, fits = run(make_finder, make_model, c, times)[1][3.5]
        assert steps.shape == (k, COLUMNS) and fits.shape == (k, fc.COLUMNS) and steps.dtype == fits.dtype == np.float64
        whole = (steps, fits) if whole is None else whole
        assert steps.tobytes() == whole[0][:k].tobytes() and fits.tobytes() == whole[1][:k].tobytes()  # no row depends on its neighbours
        assert (times[0] == 0.0) == (k == 0), (k, times)
    flags = whole[0][:, FLAGS].astype(int).tolist()
    assert flags[:5] == [0, NOT_CONVERGED, RAN_AWAY, SKIPPED, SINGULAR] and flags[-1] == NOT_CONVERGED and whole[0][-1, NITER] == 2
    c = case(f"{ROW_COUNTS[-1]} rows")
    finder, model_ = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"])
    try:
        finder.background_device(c["frame"], c["mask"])
        for i in range(len(flags)):
            alone = finder.fit_positions(model_, c["positions"][i:i + 1], c["cells"][i:i + 1], 3.5, True, use_mesh=False, **(DEFAULTS | FATES))
            assert alone[0].tobytes() == whole[0][i:i + 1].tobytes() and alone[1].tobytes() == whole[1][i:i + 1].tobytes(), i
    finally:
        model_.close()
        finder.close()


def check_reproducible(make_finder, make_model, name: str) -> None:
    """Repeats are bit-equal: on a fresh finder and model, by a second call on the same frame, and with other calls in between."""
    c = case(name)
    radius, it, mesh = c["radii"][-1], c["iteration"], c["background"] == "mesh"
    rows = run(make_finder, make_model, c)[1][radius]
    again = run(make_finder, make_model, c)[1][radius]
    assert again[0].tobytes() == rows[0].tobytes() and again[1].tobytes() == rows[1].tobytes()
    finder, model_, other_model = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"]), make_model(fc.model(16))
    try:
        finder.background_device(c["frame"], c["mask"])
        args = (model_, c["positions"], c["cells"], radius, c["fit_background"], it["max_iter"], it["eps"], it["max_shift"], it["max_step"], mesh)
        one = finder.fit_positions(*args)
        finder.fit_positions(other_model, c["positions"][::-1], c["cells"], 6.5, not c["fit_background"], 3, 1e-2, 1.0, 0.25, False)  # other rows in the same buffers
        finder.fit(other_model, c["positions"], c["cells"], 2.0)
        two = finder.fit_positions(*args)
        assert one[0].tobytes() == two[0].tobytes() == rows[0].tobytes() and one[1].tobytes() == two[1].tobytes() == rows[1].tobytes()
    finally:
        model_.close()
        other_model.close()
        finder.close()


def check_isolation(make_finder, make_model) -> None:
    """detect, measure, photometry, refine and fit give the bits they gave before a fit_positions, and its rows do not depend on them; one
    model serves two finders."""
    c = case("N = 9, mesh, flux and background")
    radii = (2.0, 4.0)
    finder, model_ = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"])
    other = make_finder(c["frame"].shape, 8)
    try:
        finder.background_device(c["frame"], c["mask"])
        rows = finder.detect_device(3.0, 5, None)
        shapes = finder.measure()
        phot = finder.photometry(rows[:, :2], radii, 5, True)
        refined = finder.refine(rows[:, :2], 1.5)
        assert len(rows) == 5
        cells = np.zeros(len(rows), np.int32)
        fits = finder.fit(model_, rows[:, :2], cells, 3.5)
        steps, at_end = finder.fit_positions(model_, rows[:, :2], cells, 3.5)
        assert np.all(steps[:, FLAGS] == 0) and np.all(steps[:, NITER] > 0)
        assert finder.measure().tobytes() == shapes.tobytes()
        assert finder.photometry(rows[:, :2], radii, 5, True).tobytes() == phot.tobytes()
        assert finder.refine(rows[:, :2], 1.5).tobytes() == refined.tobytes()
        assert finder.fit(model_, rows[:, :2], cells, 3.5).tobytes() == fits.tobytes()
        finder.fit_positions(model_, c["positions"], c["cells"], 1.0, False, 3, 1e-3, 1.0, 0.25, False)
        assert finder.measure().tobytes() == shapes.tobytes()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes()
        again = finder.fit_positions(model_, rows[:, :2], cells, 3.5)
        assert again[0].tobytes() == steps.tobytes() and again[1].tobytes() == at_end.tobytes()
        finder.background_device(c["frame"], c["mask"])  # fit_positions first, the others after it
        again = finder.fit_positions(model_, rows[:, :2], cells, 3.5)
        assert again[0].tobytes() == steps.tobytes() and again[1].tobytes() == at_end.tobytes()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes() and finder.measure().tobytes() == shapes.tobytes()
        assert finder.photometry(rows[:, :2], radii, 5, True).tobytes() == phot.tobytes()
        assert finder.refine(rows[:, :2], 1.5).tobytes() == refined.tobytes()
        assert finder.fit(model_, rows[:, :2], cells, 3.5).tobytes() == fits.tobytes()
        other.background_device(c["frame"], c["mask"])  # the same model on a second finder, with another mesh
        elsewhere = other.fit_positions(model_, rows[:, :2], cells, 3.5)
        assert elsewhere[0].shape == steps.shape and np.all(elsewhere[0][:, FLAGS] == 0)
        again = finder.fit_positions(model_, rows[:, :2], cells, 3.5)
        assert again[0].tobytes() == steps.tobytes() and again[1].tobytes() == at_end.tobytes()
    finally:
        model_.close()
        other.close()
        finder.close()


def check_errors(make_finder, make_model, error: type) -> None:
    """RPSF_E_STATE (-6) before a background_device of a frame and after the host route's detect; RPSF_E_BADARG (-1) for a bad radius,
    position or iteration argument, whatever the state."""
    import pytest

    c = case("N = 9, mesh, flux and background")
    p, k = c["positions"][:6], c["cells"][:6]
    finder, model_, small = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"]), make_model(fc.model(4))
    good = (model_, p, k, 3.5, True, 16, 1e-4, 2.0, 0.5, True)

    def but(**changes):
        names = ("model", "positions", "cells", "radius", "fit_background", "max_iter", "eps", "max_shift", "max_step", "use_mesh")
        return tuple(changes.get(name, value) for name, value in zip(names, good))

    bad = [but(radius=r) for r in (0.0, -1.0, np.nan, np.inf, 3.5000001, 64.5)] + [but(model=small, radius=1.0000001)]
    bad += [but(max_iter=-1), but(max_iter=65)]
    bad += [but(**{name: v}) for name in ("eps", "max_shift", "max_step") for v in (0.0, -1.0, np.nan)]
    bad += [but(eps=np.inf), but(max_shift=64.5), but(max_step=64.5), but(max_shift=np.inf), but(max_step=np.inf)]
    bad += [but(positions=[(np.nan, 1.0)], cells=[0]), but(positions=[(1.0, np.inf)], cells=[0]), but(positions=[(2.0 ** 20, 1.0)], cells=[0]),
            but(positions=[(1.0, 1.0), (1.0, -2.0 ** 20)], cells=[0, 0], use_mesh=False)]
    try:
        def refused(args, code):
            with pytest.raises(error) as caught:
                finder.fit_positions(*args)
            assert caught.value.code == code, (args[3:], caught.value.code)

        refused(good, -6)
        for args in bad:
            refused(args, -1)
        level, rms = finder.background(c["frame"], c["mask"])  # the host route: no S1b mesh on the device
        refused(good, -6)
        finder.background_device(c["frame"], c["mask"])
        for args in bad:
            refused(args, -1)
        steps, fits = finder.fit_positions(*good)
        assert finder.fit_positions(*but(positions=[(2.0 ** 20 - 1, 1.0 - 2.0 ** 20)], cells=[0]))[0].shape == (1, COLUMNS)  # the largest admitted
        assert finder.fit_positions(*but(model=small, radius=1.0, fit_background=False))[1].shape == (6, fc.COLUMNS)
        assert finder.fit_positions(*but(max_iter=64, eps=5e-324, max_shift=64.0, max_step=64.0))[0].shape == (6, COLUMNS)
        level_f, _, global_rms = stars.filter_mesh(level, rms)
        finder.detect(level_f, 3.0 * global_rms, 5, None)  # the host route's detect replaces the mesh on the device
        refused(good, -6)
        finder.background_device(c["frame"], c["mask"])
        again = finder.fit_positions(*good)
        assert again[0].tobytes() == steps.tobytes() and again[1].tobytes() == fits.tobytes()
    finally:
        model_.close()
        small.close()
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ the truth
# fit_cases' truth case (three 64 x 64 frames of five noise-free Gaussians of sigma 1.5 each) and its float64 16-pixel model, R = 5, the
# fitted background, background="none", the defaults of the iteration; every star started (0.5, -0.5) and (-1.2, 0.9) px off the truth, with
# the cell of its true position.  The figures below are the RESTATEMENT's, in the kernel's order of operations (the kernel is held to the
# restatement bit for bit, so they are the kernel's too); beside them the figures of the NumPy prototype that the definition was tried with
# before the kernel existed (numpy.linalg.solve, np.sum), over nine starts.  The asserted bounds are TRUTH_MARGIN = 2 times the measured
# figures, the convention of fit_cases, refine_cases and photometry_cases: the margin absorbs a later, deliberate change of the definition's
# last places, never a kernel error.  What limits the distance is not the iteration but the model: a cell sampled at whole pixels and
# interpolated bilinearly has its maximum likelihood position a few thousandths of a pixel from the truth, depending on the sub-pixel phase.
TRUTH_STARTS = ((0.5, -0.5), (-1.2, 0.9))
MEASURED_WORST_DISTANCE = 0.00736  # px, the worst of 15 stars and both starts (the prototype: 0.0074)
MEASURED_MEDIAN_DISTANCE = 0.00662  # px (the prototype: 0.0066)
MEASURED_RESIDUAL = 0.0371  # the median residual_fraction at the fitted positions (the prototype: 0.0370; at the truth 0.0375)
MEASURED_NITER = 6  # the largest niter; the two ends of a star lie 6e-9 px apart (the prototype: 2 - 6 over its nine starts)
TRUTH_MARGIN = fc.TRUTH_MARGIN


def truth_rows(values, coordinates, offset, fit_positions=None) -> list[np.ndarray]:
    """fit_positions' result on the truth case from `offset` off the truth: the restatement's, or `fit_positions`' (the product's function,
    on whatever finder stands behind it) when given."""
    t, out = fc.truth_case(), []
    for frame, pos in zip(t["frames"], t["truth"]):
        cells = stars.nearest_cells(pos, coordinates, fc.TRUTH_N)  # the star's cell, wherever the iteration starts
        start = pos + np.asarray(offset)
        if fit_positions is not None:
            from regularizepsf_amd import IndexedCube

            out.extend(fit_positions(frame, start, IndexedCube(coordinates, values), fc.TRUTH_RADIUS, background="none", box=BOX, cells=cells))
            continue
        steps = ref_fit_positions(frame, None, BOX, None, values, start, cells, fc.TRUTH_RADIUS, True, "none")
        fits = fc.ref_fit(frame, None, BOX, None, values, steps[:, Y:X + 1], cells, fc.TRUTH_RADIUS, True, "none")
        out.append(stars.fitpos_from_sums(steps, fits, True))
    return out


def check_truth(values=None, coordinates=None, what="the oracle's model", fit_positions=None, fit_stars_displaced=None) -> dict:
    """Check 6, on the restatement or on `fit_positions`: every star converges from both starts to the same point, near the truth, and the
    model describes it there as well as at the truth - at least DISPLACED_FACTOR better than where the (0.5, -0.5) start stood."""
    if values is None:
        coordinates, values = fc.oracle_model()
    truth = np.concatenate(fc.truth_case()["truth"])
    ends = [np.concatenate(truth_rows(values, coordinates, o, fit_positions)) for o in TRUTH_STARTS]
    for got in ends:
        assert np.all(got["flags"] == 0) and np.all(got["converged"]) and np.all(got["fit_flags"] == 0) and np.all(got["coverage"] == 1.0)
    apart = np.hypot(ends[0]["row"] - ends[1]["row"], ends[0]["col"] - ends[1]["col"])
    distance = np.concatenate([np.hypot(got["row"] - truth[:, 0], got["col"] - truth[:, 1]) for got in ends])
    residual = float(np.median(ends[0]["residual_fraction"]))
    displaced = float(np.median(fc.truth_fits(values, coordinates, np.asarray(TRUTH_STARTS[0]))["residual_fraction"])
                      if fit_stars_displaced is None else fit_stars_displaced)
    figures = {"worst": float(distance.max()), "median": float(np.median(distance)), "residual": residual,
               "niter": int(max(got["niter"].max() for got in ends)), "apart": float(apart.max()), "displaced": displaced}
    print(f"truth, {what}: {len(truth)} stars from {TRUTH_STARTS}: distance to the truth worst {figures['worst']:.4g} px (measured "
          f"{MEASURED_WORST_DISTANCE}), median {figures['median']:.4g} px ({MEASURED_MEDIAN_DISTANCE}); the two ends at most {figures['apart']:.3g} px "
          f"apart; niter <= {figures['niter']} ({MEASURED_NITER}); median residual_fraction {residual:.4g} ({MEASURED_RESIDUAL}), at the "
          f"displaced start {displaced:.4g}")
    assert figures["apart"] <= 10 * DEFAULTS["eps"]
    assert figures["worst"] <= TRUTH_MARGIN * MEASURED_WORST_DISTANCE and figures["median"] <= TRUTH_MARGIN * MEASURED_MEDIAN_DISTANCE
    assert residual <= TRUTH_MARGIN * MEASURED_RESIDUAL and figures["niter"] <= TRUTH_MARGIN * MEASURED_NITER
    assert displaced >= fc.DISPLACED_FACTOR * residual
    return figures
