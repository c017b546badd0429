"""Weighted fits (DESIGN.md 3.7 "Weighted fits", kernel S12) restated in float64 NumPy, the cases, the CPU emulator of the kernel, and the
checks the emulator tests (tests/test_fitw_host.py) and the GPU tests (tests/test_gpu_fitw.py) share.

The reference is the restatement below, written from the definition operation for operation like fit_cases.ref_fit, whose summation order
(`ordered_sum`), model (`ref_model`) and residual (photometry_cases.ref_residual) it uses.  BIT FOR BIT as in fit_cases: kernel, emulator
and restatement agree in every bit of every number.  What is new here:
  the variance  v is a float64: the map rounded to float32 once and widened, or sky_variance + max(raw pixel, 0) / gain on the float32
                pixel, a division and then an addition;
  the weight    w = 1.0 / v, one division; the pixel takes part when S8 would use it and w > 0 and w is finite;
  the terms     wm = w m and wd = w d first, then wm m, wd m, wd d: with v = 1 every term is S8's term, with v = 2^k S8's times 2^-k.
A pixel the kernel skips enters the restatement's sums as + 0.0 (its weight is set to 0 before anything is multiplied).

A check takes `make_finder(shape, box)` and `make_model(values)`: regularizepsf_amd.stars._Finder and ._Model on the GPU, EmuFinder and
EmuModel here.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np

from tests import emulib
from regularizepsf_amd import stars
from tests import fit_cases as fc
from tests import group_cases as gc
from tests import photometry_cases as pc
from tests import star_cases as sc
from tests import wide_cases as wc

ROOT = sc.ROOT
COLUMNS = 25
(Y, X, CELL, FLAGS, N_USE, N_ALL, SM, SM_ALL, SW, SWM, SWMM, SWD, SWDM, SWDD, F, BG, VAR_F, VAR_BG, COV, CHI2, ABS_RES, PEAK_RES, PEAK_E, PEAK_ROW,
 PEAK_COL) = range(COLUMNS)
NO_MESH, TOO_FEW, DEGENERATE, BAD_CELL = fc.NO_MESH, fc.TOO_FEW, fc.DEGENERATE, fc.BAD_CELL
SHAPE, BOX = fc.SHAPE, fc.BOX
S8_SAME = ((F, fc.F), (BG, fc.BG), (ABS_RES, fc.ABS_RES), (PEAK_RES, fc.PEAK_RES), (PEAK_E, fc.PEAK_E), (PEAK_ROW, fc.PEAK_ROW),
           (PEAK_COL, fc.PEAK_COL))  # (S12's column, S8's): what a constant power-of-two variance leaves bit for bit
same_bits = fc.same_bits


# ------------------------------------------------------------------------------------------------------------------ the restatement
def ref_weights(frame, variance, sky_variance, gain) -> tuple[np.ndarray, np.ndarray]:
    """(w, ok): the weight of every pixel of the frame in float64, and where it is positive and finite."""
    with np.errstate(all="ignore"):
        if variance is not None:
            v = np.asarray(variance).astype(np.float32).astype(np.float64)  # rounded to float32 once
        else:
            raw = np.asarray(frame, np.float32)
            v = np.float64(sky_variance) + np.where(raw > 0, raw.astype(np.float64), 0.0) / np.float64(gain)
        w = 1.0 / v
    return w, (w > 0.0) & np.isfinite(w)


def ref_fit_weighted(frame, mask, box, level_f, cube, positions, cells, radius, fit_background: bool, background: str, variance=None,
                     sky_variance=None, gain=np.inf) -> np.ndarray:
    """The definition: (k, COLUMNS) rows in the kernel's layout.  `variance`: the map (any real dtype), or None for the noise model."""
    d, ok = pc.ref_residual(frame, mask, box, level_f, background)
    w, w_ok = ref_weights(frame, variance, sky_variance, gain)
    H, W = d.shape
    cube = np.asarray(cube, np.float64)
    no_mesh = background == "mesh" and level_f is None
    positions = np.asarray(positions, np.float64).reshape(-1, 2)
    R = np.float64(radius)
    R2 = R * R
    rows = np.empty((len(positions), COLUMNS))
    for row, (y, x), k in zip(rows, positions, np.asarray(cells, np.int64)):
        rr = np.arange(int(np.floor(y - R)) - 1, int(np.ceil(y + R)) + 2)
        cc = np.arange(int(np.floor(x - R)) - 1, int(np.ceil(x + R)) + 2)
        pr, pc_ = rr.astype(np.float64) - y, cc.astype(np.float64) - x
        disc = ((pr * pr)[:, None] + (pc_ * pc_)[None, :]) <= R2
        on_frame = ((rr >= 0) & (rr < H))[:, None] & ((cc >= 0) & (cc < W))[None, :]
        ri, ci = np.clip(rr, 0, H - 1)[:, None], np.clip(cc, 0, W - 1)[None, :]
        use = disc & on_frame & ok[ri, ci] & w_ok[ri, ci]
        bad_cell = not 0 <= k < len(cube)
        flags = (NO_MESH if no_mesh else 0) | (BAD_CELL if bad_cell else 0)
        n = int(use.sum())
        row[:] = np.nan
        row[Y], row[X], row[CELL], row[N_USE], row[N_ALL] = y, x, k, n, int(disc.sum())
        row[PEAK_ROW] = row[PEAK_COL] = -1.0
        f = bg = None
        if flags == 0:
            m = fc.ref_model(cube[k], pr, pc_, disc)
            dv, mu, wv = np.where(use, d[ri, ci], 0.0), np.where(use, m, 0.0), np.where(use, w[ri, ci], 0.0)
            with np.errstate(all="ignore"):
                wm, wd = wv * mu, wv * dv
                Sm, Sm_all, Sw, Swm, Swmm, Swd, Swdm, Swdd = (fc.ordered_sum(t) for t in (mu, m, wv, wm, wm * mu, wd, wd * mu, wd * dv))
                row[SM:SWDD + 1] = Sm, Sm_all, Sw, Swm, Swmm, Swd, Swdm, Swdd
                if n < (3 if fit_background else 1):
                    flags |= TOO_FEW
                elif fit_background:
                    D = Sw * Swmm - Swm * Swm
                    if not np.isfinite(D) or D <= 0.0:
                        flags |= DEGENERATE
                    else:
                        f = (Sw * Swdm - Swm * Swd) / D
                        bg = (Swd - f * Swm) / Sw
                        row[VAR_F], row[VAR_BG], row[COV] = Sw / D, Swmm / D, -Swm / D
                else:
                    D = Swmm
                    if not np.isfinite(D) or D <= 0.0:
                        flags |= DEGENERATE
                    else:
                        f, bg = Swdm / D, np.float64(0.0)
                        row[VAR_F], row[VAR_BG], row[COV] = np.float64(1.0) / D, 0.0, 0.0
        row[FLAGS] = flags
        if flags == 0:
            with np.errstate(all="ignore"):
                e = dv - (f * mu + bg)
                e2, ea = np.where(use, wv * (e * e), 0.0), np.where(use, np.abs(e), 0.0)
                key = np.where(use, np.where(np.isnan(e), np.inf, np.abs(e)), -1.0)
            top = int(np.argmax(key.ravel()))  # the first in raster order among equals
            row[F], row[BG], row[CHI2], row[ABS_RES] = f, bg, fc.ordered_sum(e2), fc.ordered_sum(ea)
            row[PEAK_RES], row[PEAK_E] = np.abs(e.ravel()[top]), e.ravel()[top]
            row[PEAK_ROW], row[PEAK_COL] = rr[top // len(cc)], cc[top % len(cc)]
    return rows


# ------------------------------------------------------------------------------------------------------------------ the emulator
@functools.cache
def emulator():
    """tests/emu/libemu_fit_weighted.so: the kernel's driver on the CPU, compiled here when missing or older than its sources."""
    lib = emulib.library("emu_fit_weighted")
    vp, i, n, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    lib.emufw_info.argtypes = [vp]
    lib.emufw_fit.argtypes = [vp, vp, i, i, i, vp, i, n, i, vp, n, vp, vp, f, i, i, i, vp, f, f, vp]
    return lib


def emulator_info() -> tuple[int, int, int]:
    """WALK_WAVES, the workgroups of S12 the last fit ran, s12_lds_bytes()."""
    info = (ctypes.c_long * 3)(0, 0, 0)
    emulator().emufw_info(info)
    return tuple(info)


EmuError, EmuModel = pc.EmuError, gc.EmuModel


class EmuFinder(gc.EmuFinder):
    """group_cases.EmuFinder - every other kernel's method - with ``variance`` and ``fit_weighted``: regularizepsf_amd.stars._Finder's
    interface on the emulator."""

    def __init__(self, shape, box, device=0) -> None:
        super().__init__(shape, box, device)
        self._variance, self._fitted_weighted = None, 0

    def variance(self, frame) -> None:
        frame = np.asarray(frame)
        if frame.shape != tuple(self.shape):
            raise stars.IncorrectShapeError(f"A variance frame of shape {frame.shape} does not fit a finder of shape {self.shape}")
        with np.errstate(all="ignore"):
            self._variance = np.ascontiguousarray(frame if frame.dtype == np.float32 else frame.astype(np.float64).astype(np.float32))

    def fit_weighted(self, model, positions, cells, radius, fit_background=True, use_mesh=True, sky_variance=None, gain=np.inf):
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        cells = np.ascontiguousarray(cells, np.int32).ravel()
        if len(cells) != len(positions):
            raise ValueError(f"{len(cells)} cells for {len(positions)} positions")
        out = np.empty((len(positions), COLUMNS))
        level = None if self._filtered is None else np.ascontiguousarray(self._filtered[0])
        frame, mask = (self._frame, self._mask) if self._frame is not None else (np.zeros(self.shape, np.float32), None)
        mode, sky = (stars.VARIANCE_MAP, 0.0) if sky_variance is None else (stars.VARIANCE_MODEL, float(sky_variance))
        var = self._variance if mode == stars.VARIANCE_MAP else None
        code = emulator().emufw_fit(frame.ctypes.data, None if mask is None else mask.ctypes.data, *self.shape, self.box,
                                    None if level is None else level.ctypes.data, int(level is None), len(model.values), model.size,
                                    model.values.ctypes.data, len(positions), positions.ctypes.data, cells.ctypes.data, float(radius),
                                    int(bool(fit_background)), int(bool(use_mesh)), mode, None if var is None else var.ctypes.data, sky,
                                    float(gain), out.ctypes.data)
        if code == -1 or model.device != self._device:
            raise EmuError(-1, "bad argument")
        if not self._have_mesh:  # (the library checks its arguments first, then its state)
            raise EmuError(-6, "fit_weighted before background_device")
        if code == -6:
            raise EmuError(-6, "fit_weighted with a variance map before variance")
        self._fitted_weighted = emulator_info()[1]
        return out

    def fit_weighted_ms(self) -> float:
        """In the place of the device time: the workgroups of S12 that ran - 0.0 exactly when nothing was launched."""
        return float(self._fitted_weighted)


# ------------------------------------------------------------------------------------------------------------------ the variance maps
STAR = (20.3, 17.6)  # fit_cases' first star: every map's special pixels lie in its disc of R = 3.5
BAD_PIXELS = {(20, 17): np.nan, (21, 17): 0.0, (19, 18): -1.0, (20, 19): np.inf}  # each takes its pixel out of the fit
SUBNORMAL_PIXEL = (22, 18)  # a float32 subnormal: 1 / v is about 1e42, finite in float64 - the pixel stays, with that weight


@functools.cache
def smooth_map(shape=SHAPE) -> np.ndarray:
    """A positive float32 map without a special pixel: 0.05 ... 0.4, a ramp with a ripple."""
    rows, cols = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    v = (0.09 + 0.004 * rows + 0.002 * cols) * (1.0 + 0.4 * np.sin(0.9 * rows + 0.3) * np.cos(0.7 * cols))
    assert v.min() > 0.04
    return sc._freeze({"v": v.astype(np.float32)})["v"]


@functools.cache
def bad_map() -> np.ndarray:
    v = smooth_map().copy()
    for (r, c), value in BAD_PIXELS.items():
        v[r, c] = value
    v[SUBNORMAL_PIXEL] = np.float32(1e-42)
    assert 0.0 < v[SUBNORMAL_PIXEL] < np.finfo(np.float32).tiny
    return sc._freeze({"v": v})["v"]


@functools.cache
def blind_map() -> np.ndarray:
    """No usable variance anywhere within 5 pixels of STAR, a mix of the four kinds."""
    v = smooth_map().copy()
    rows, cols = np.mgrid[0:SHAPE[0], 0:SHAPE[1]]
    inside = (rows - STAR[0]) ** 2 + (cols - STAR[1]) ** 2 <= 25.0
    v[inside] = np.resize(np.array([np.nan, 0.0, -2.5, np.inf], np.float32), int(inside.sum()))
    return sc._freeze({"v": v})["v"]


@functools.cache
def float64_map() -> np.ndarray:
    """The smooth map's formula kept in float64: almost no value is a float32, so the single rounding shows."""
    rows, cols = np.mgrid[0:SHAPE[0], 0:SHAPE[1]].astype(np.float64)
    v = (0.09 + 0.004 * rows + 0.002 * cols) * (1.0 + 0.4 * np.sin(0.9 * rows + 0.3) * np.cos(0.7 * cols)) + 1e-9
    assert np.mean(v.astype(np.float32).astype(np.float64) != v) > 0.9
    return sc._freeze({"v": v})["v"]


# ------------------------------------------------------------------------------------------------------------------ the cases
GAUSSIAN, ZERO, LOBES, CONSTANT = fc.GAUSSIAN, fc.ZERO, fc.LOBES, fc.CONSTANT
OFF = (-30.0, -30.0)
# N = 8 admits R <= N / 2 - 1 = 3 (S8's rule, kept): it runs at 3; R = 3.5 runs on N = 9 and N = 16, R = 7 on N = 16
SIZES = {8: (3.0,), 9: (3.5,), 16: (3.5, 7.0)}


def grid_rows() -> tuple[np.ndarray, np.ndarray]:
    """STAR and a position off the frame with every cell and the indices -1 and 4; the other stars and the hard positions (on the rim, off
    the frame) with the Gaussian and the lobes in turn."""
    every = np.array([STAR, OFF])
    others = np.concatenate([fc.field()["truth"][1:], fc.hard_positions()])
    p, k = fc._every_cell(every)
    return np.concatenate([p, others]), np.concatenate([k, np.resize(np.array([GAUSSIAN, LOBES]), len(others))])


def _wcase(base: dict, variance=None, sky_variance=None, gain=np.inf, flags=(0,), excluded=None) -> dict:
    """`base`: a fit_cases case.  `flags`: values of the flags column the case must show; `excluded`: {row: pixels S8 would use and the
    weight rule takes out} (every other row: none), or "all"."""
    assert (variance is None) != (sky_variance is None)
    return {**base, "variance": variance, "sky_variance": sky_variance, "gain": gain, "flags": tuple(flags), "excluded": excluded or {}}


def _grid_case(n, background, fit_background, how) -> dict:
    base = fc._case(fc.field()["frame"], *grid_rows(), n, background, fit_background, radii=SIZES[n])
    flags = (0, TOO_FEW, DEGENERATE, BAD_CELL)
    return _wcase(base, variance=smooth_map(), flags=flags) if how == "map" else _wcase(base, sky_variance=0.09, gain=4.0, flags=flags)


def _map_case(variance, n=9, flags=(0,), excluded=None, masked=False, background="mesh", fit_background=True, radii=None) -> dict:
    m = fc.masked_field() if masked else {"frame": fc.field()["frame"], "mask": None}
    p = np.concatenate([fc.field()["truth"], fc.hard_positions()[3:8]])  # (none of the others within 8.5 pixels of STAR)
    base = fc._case(m["frame"], p, np.resize(np.array([GAUSSIAN, LOBES, GAUSSIAN]), len(p)), n, background, fit_background, m["mask"],
                    radii=SIZES[n] if radii is None else radii)
    return _wcase(base, variance=variance, flags=flags, excluded=excluded)


def _model_case(sky_variance, gain, flags=(0,), excluded=None, background="mesh", fit_background=True) -> dict:
    p = np.concatenate([fc.field()["truth"], fc.hard_positions()[3:8]])  # (none of the others within 8.5 pixels of STAR)
    base = fc._case(fc.field()["frame"], p, np.resize(np.array([GAUSSIAN, LOBES, GAUSSIAN]), len(p)), 9, background, fit_background, radii=(3.5,))
    return _wcase(base, sky_variance=sky_variance, gain=gain, flags=flags, excluded=excluded)


ROW_COUNTS = (0, 3, 4, 5, 9)  # 0, WALK_WAVES - 1, WALK_WAVES, WALK_WAVES + 1, 2 WALK_WAVES + 1 (check_row_counts asserts that)


def _row_case(k: int) -> dict:
    positions = np.concatenate([fc.field()["truth"], fc.hard_positions()[:4]])[:k]
    base = fc._case(fc.field()["frame"], positions, np.resize(np.array([GAUSSIAN, LOBES, GAUSSIAN, CONSTANT, -1]), k), 9, radii=(3.5,))
    return _wcase(base, variance=smooth_map(), flags=(0, DEGENERATE, BAD_CELL) if k >= 5 else ())


def _wide_case() -> dict:
    base = fc._case(wc.field()["frame"], wc.STARS[:3], [wc.BROAD, wc.LOBES, wc.BROAD], 130, radii=(64.0,), box=wc.BOX, cube=wc.cube(130))
    return _wcase(base, variance=smooth_map(wc.SHAPE))


GRID_CASES = {f"N = {n}, {b}, {'flux and background' if fb else 'flux alone'}, {how}": functools.partial(_grid_case, n, b, fb, how)
              for n in SIZES for b in ("mesh", "none") for fb in (True, False) for how in ("map", "model")}
# row 0 is STAR: its disc of R = 3.5 holds the four bad pixels, and no other row's disc comes near them
MAP_CASES = {
    "a smooth map": lambda: _map_case(smooth_map()),
    "a smooth map, masked frame, flux alone": lambda: _map_case(smooth_map(), masked=True, fit_background=False),
    "bad variances in a disc": lambda: _map_case(bad_map(), excluded={0: len(BAD_PIXELS)}),
    "bad variances in a disc, none, flux alone": lambda: _map_case(bad_map(), excluded={0: len(BAD_PIXELS)}, background="none",
                                                                   fit_background=False),
    "bad variances in a disc, N = 16": lambda: _map_case(bad_map(), 16, excluded={0: len(BAD_PIXELS)}),
    "no variance in a disc": lambda: _map_case(blind_map(), flags=(0, TOO_FEW), excluded={0: "all"}),
    "no variance in a disc, flux alone": lambda: _map_case(blind_map(), flags=(0, TOO_FEW), excluded={0: "all"}, fit_background=False),
    "a float64 map": lambda: _map_case(float64_map()),
    "unit variance": lambda: _map_case(np.ones(SHAPE, np.float32)),
}
MODEL_CASES = {
    "noise model, gain 2.5": lambda: _model_case(0.25, 2.5),
    "noise model, gain inf": lambda: _model_case(0.25, np.inf),
    "noise model, no sky": lambda: _model_case(0.0, 2.5),
    "noise model, none, flux alone": lambda: _model_case(0.25, 2.5, background="none", fit_background=False),
    # 1 / 5e-324 overflows: no pixel has a finite weight
    "noise model, a sky variance whose weight overflows": lambda: _model_case(5e-324, np.inf, flags=(TOO_FEW,), excluded="all"),
}
OTHER_CASES = {
    "no valid mesh node": lambda: _wcase(fc._case(np.full(SHAPE, np.nan, np.float32), [(30.2, 20.7), (0.0, 0.0), OFF, (10.0, 10.0)],
                                                  [GAUSSIAN, GAUSSIAN, LOBES, 7], 9, radii=(3.5,)), variance=smooth_map(),
                                         flags=(NO_MESH, NO_MESH | BAD_CELL)),
    "no valid mesh node, model": lambda: _wcase(fc._case(np.full(SHAPE, np.nan, np.float32), [(30.2, 20.7), OFF], [GAUSSIAN, 4], 9, radii=(3.5,)),
                                                sky_variance=1.0, flags=(NO_MESH, NO_MESH | BAD_CELL)),
    "a cell of NaN": lambda: _wcase(fc._case(fc.field()["frame"], np.repeat(fc.field()["truth"][:2], 3, axis=0), [GAUSSIAN, ZERO, LOBES] * 2, 9,
                                             radii=(3.5,), cube=np.where(np.arange(4)[:, None, None] == ZERO, np.nan, fc.model(9))),
                                    variance=smooth_map(), flags=(0, DEGENERATE)),
}
ROW_CASES = {f"{k} rows": functools.partial(_row_case, k) for k in ROW_COUNTS}
WIDE_CASES = {"wide: N = 130, R = 64, three stars": _wide_case}
TABLE_CASES = {**GRID_CASES, **MAP_CASES, **MODEL_CASES, **OTHER_CASES, **ROW_CASES, **WIDE_CASES}


@functools.cache
def case(name: str) -> dict:
    return sc._freeze(TABLE_CASES[name]())


def constant_case(v: float) -> dict:
    """The rows of the grid with a constant variance `v`, as a map and - run_both - as the noise model without a photon term."""
    base = fc._case(fc.field()["frame"], *grid_rows(), 9, "mesh", True, radii=(3.5,))
    return _wcase(base, variance=np.full(SHAPE, v, np.float32))


@functools.lru_cache(maxsize=None)
def _reference(name: str, mesh_bytes: bytes | None, radius: float) -> np.ndarray:
    c = case(name)
    level_f = None if mesh_bytes is None else np.frombuffer(mesh_bytes).reshape(-(-c["frame"].shape[0] // c["box"]), -(-c["frame"].shape[1] // c["box"]))
    out = ref_fit_weighted(c["frame"], c["mask"], c["box"], level_f, c["cube"], c["positions"], c["cells"], radius, c["fit_background"],
                           c["background"], c["variance"], c["sky_variance"], c["gain"])
    out.flags.writeable = False
    return out


def reference(name: str, level_f, radius: float) -> np.ndarray:
    """The restatement's rows for the case on the filtered mesh `level_f` (None: no valid node), computed once per case, mesh and radius."""
    mesh = None if level_f is None or case(name)["background"] == "none" else np.ascontiguousarray(level_f).tobytes()
    return _reference(name, mesh, float(radius))


# ------------------------------------------------------------------------------------------------------------------ the checks
def run(make_finder, make_model, c: dict, times: list | None = None, unweighted: bool = False) -> tuple:
    """The product's per-frame route on a finder: (the filtered mesh or None, {radius: S12's rows}); `unweighted`: and {radius: S8's rows}
    of the same finder, taken after S12's."""
    finder, model = make_finder(c["frame"].shape, c["box"]), None
    try:
        model = make_model(c["cube"])
        level, rms = finder.background(c["frame"], c["mask"])  # the raw mesh of the finder under test (photometry_cases, THE MESH)
        filtered = stars.filter_mesh(level, rms)
        finder.background_device(c["frame"], c["mask"])
        if c["variance"] is not None:
            finder.variance(c["variance"])
        rows, plain = {}, {}
        for radius in c["radii"]:
            rows[radius] = finder.fit_weighted(model, c["positions"], c["cells"], radius, c["fit_background"], c["background"] == "mesh",
                                               c["sky_variance"], c["gain"])
            if times is not None:
                times.append(finder.fit_weighted_ms())
            if unweighted:
                plain[radius] = finder.fit(model, c["positions"], c["cells"], radius, c["fit_background"], c["background"] == "mesh")
        level_f = None if filtered is None else filtered[0]
        return (level_f, rows, plain) if unweighted else (level_f, rows)
    finally:
        if model is not None:
            model.close()
        finder.close()


def check_case(make_finder, make_model, name: str) -> dict:
    """Every row of every radius of the case against the restatement, bit for bit; the case shows the flags it was built for, and the
    weight rule takes out exactly the pixels it was built to lose (counted against S8 on the same finder).  Returns {radius: rows}."""
    c = case(name)
    level_f, rows, plain = run(make_finder, make_model, c, unweighted=True)
    for radius, got in rows.items():
        want = reference(name, level_f, radius)
        assert got.dtype == np.float64 and got.shape == want.shape, f"{name}: {got.shape}, the restatement has {want.shape}"
        flags = got[:, FLAGS].astype(int)
        differ = [i for i in range(len(want)) if not same_bits(got[i], want[i])]
        lost = (plain[radius][:, fc.N_USE] - got[:, N_USE]).astype(int)
        print(f"{name}, R = {radius:g}: {len(want)} rows, {int((flags == 0).sum())} fitted, flags {sorted(set(flags.tolist()))}, n <= "
              f"{int(want[:, N_USE].max(initial=0))}, pixels lost to the weight rule {lost.tolist()}, {len(differ)} rows differ from the "
              f"restatement")
        assert not differ, (name, radius, differ[:3], got[differ[0]], want[differ[0]])
        assert set(c["flags"]) <= set(flags.tolist()), (name, radius, c["flags"])
        assert got[:, N_ALL].tobytes() == plain[radius][:, fc.N_ALL].tobytes()  # the disc is S8's
        keep = ~np.isnan(got[:, SM_ALL])
        assert got[keep, SM_ALL].tobytes() == plain[radius][keep, fc.SM_ALL].tobytes()
        for i in range(len(got)):
            expected = c["excluded"] if c["excluded"] == "all" else c["excluded"].get(i, 0)
            if expected == "all":
                assert got[i, N_USE] == 0 and (lost[i] > 0 or plain[radius][i, fc.N_USE] == 0), (name, radius, i)
            else:
                assert lost[i] == expected, (name, radius, i, lost[i], expected)
    return rows


def check_every_flag_fires(make_finder, make_model) -> None:
    """Every flag fires on a case built for it and says what it should; the counts come with every flag."""
    c = case("N = 9, none, flux and background, map")
    _, rows = run(make_finder, make_model, c)
    at = lambda p, k: next(i for i, (q, j) in enumerate(zip(c["positions"].tolist(), c["cells"].tolist())) if tuple(q) == p and j == k)
    got = rows[3.5]
    flags = got[:, FLAGS].astype(int)
    assert np.all(flags[(c["cells"] < 0) | (c["cells"] >= 4)] == BAD_CELL) and not np.any(flags[(c["cells"] >= 0) & (c["cells"] < 4)] & BAD_CELL)
    bad = got[flags == BAD_CELL]
    assert np.isnan(bad[:, SM:PEAK_E + 1]).all() and np.all(bad[:, PEAK_ROW:] == -1.0) and np.all(bad[:, N_ALL] > 0)
    star = got[at(STAR, ZERO)]
    assert star[FLAGS] == DEGENERATE and star[SWMM] == 0.0 and star[SW] > 0.0 and star[N_USE] == star[N_ALL] > 0 and np.isnan(star[F:PEAK_E + 1]).all()
    star = got[at(STAR, CONSTANT)]  # a constant model with a fitted background: D = Sw Swmm - Swm Swm is rounding noise around 0 ...
    assert star[SWMM] > 0.0 and (star[FLAGS] == DEGENERATE) == (star[SW] * star[SWMM] - star[SWM] * star[SWM] <= 0.0)
    off = got[at(OFF, GAUSSIAN)]
    assert off[FLAGS] == TOO_FEW and off[N_USE] == 0 and off[N_ALL] > 0 and off[SM] == 0.0 and off[SW] == 0.0 and off[SM_ALL] > 0.0
    assert np.isnan(off[F:PEAK_E + 1]).all() and off[PEAK_ROW] == off[PEAK_COL] == -1.0
    star = got[at(STAR, GAUSSIAN)]
    assert star[FLAGS] == 0 and star[F] > 0 and star[CHI2] >= 0 and star[PEAK_RES] == abs(star[PEAK_E]) and star[PEAK_ROW] >= 0
    assert star[VAR_F] > 0 and star[VAR_BG] > 0 and star[COV] < 0 and star[COV] ** 2 < star[VAR_F] * star[VAR_BG]
    alone = run(make_finder, make_model, case("N = 9, none, flux alone, map"))[1][3.5]
    star = alone[at(STAR, CONSTANT)]  # ... and without one a fit like any other
    assert star[FLAGS] == 0 and star[BG] == 0.0 and not np.signbit(star[BG]) and star[VAR_BG] == 0.0 and star[COV] == 0.0
    assert same_bits(star[VAR_F], np.float64(1.0) / star[SWMM])
    assert alone[at(OFF, GAUSSIAN)][FLAGS] == TOO_FEW and alone[at(STAR, ZERO)][FLAGS] == DEGENERATE
    none = run(make_finder, make_model, case("no valid mesh node"))[1][3.5]
    assert none[:, FLAGS].astype(int).tolist() == [NO_MESH, NO_MESH, NO_MESH, NO_MESH | BAD_CELL]
    assert np.isnan(none[:, SM:PEAK_E + 1]).all() and np.all(none[:, N_USE] == 0) and np.all(none[:, N_ALL] > 0)
    blind = run(make_finder, make_model, case("no variance in a disc"))[1][3.5]
    assert blind[0, FLAGS] == TOO_FEW and blind[0, N_USE] == 0 and blind[0, N_ALL] > 0 and blind[0, SM_ALL] > 0 and np.all(blind[1:5, FLAGS] == 0)
    seen = {int(f) for name in ("N = 9, none, flux and background, map", "no valid mesh node") for f in run(make_finder, make_model, case(name))[1][3.5][:, FLAGS]}
    print(f"flags seen: {sorted(seen)}")
    assert {0, NO_MESH, TOO_FEW, DEGENERATE, BAD_CELL} <= seen


def check_bad_variances(make_finder, make_model) -> None:
    """Each of the four bad variances takes exactly its pixel out, the float32 subnormal stays with its weight of about 1e42 and owns the
    fit, and a pixel out of the fit still counts in n_all and Sm_all and shows as lower coverage."""
    good = run(make_finder, make_model, case("a smooth map"))[1][3.5][0]
    for (r, c_), value in {**BAD_PIXELS, SUBNORMAL_PIXEL: np.float32(1e-42)}.items():
        v = smooth_map().copy()
        v[r, c_] = value
        c = {**case("a smooth map"), "variance": v}
        got = run(make_finder, make_model, c)[1][3.5][0]
        assert got[N_ALL] == good[N_ALL] and same_bits(got[SM_ALL], good[SM_ALL])
        if (r, c_) == SUBNORMAL_PIXEL:  # (one pixel outweighs the rest by 1e43: D is rounding noise, fitted or DEGENERATE as it falls)
            assert got[N_USE] == good[N_USE] and got[SW] > 1e41 and same_bits(got[SM], good[SM]) and got[FLAGS] in (0, DEGENERATE)
        else:
            assert got[N_USE] == good[N_USE] - 1 and got[SM] < good[SM] and got[SW] < good[SW] and got[FLAGS] == 0
            fit = stars.weighted_fit_from_sums(got[None])[0]
            assert fit["coverage"] < 1.0 and fit["flags"] == 0


def check_power_of_two(make_finder, make_model) -> None:
    """v = 1: f, bg, chi2, abs_res and the peak are S8's of the same finder bit for bit, and Sw = n.  v = 4 and v = 1 / 8: f, bg, abs_res and
    the peak stay, chi2 is S8's times 1 / v and var_f is v (n / D) of S8's sums, exactly.  As a map and as the noise model."""
    for v in (1.0, 4.0, 0.125):
        c = constant_case(v)
        for how in ("map", "model"):
            cc = c if how == "map" else {**c, "variance": None, "sky_variance": v, "gain": np.inf}
            _, rows, plain = run(make_finder, make_model, cc, unweighted=True)
            got, s8 = rows[3.5], plain[3.5]
            fitted = got[:, FLAGS] == 0
            assert got[:, :N_ALL + 1].tobytes() == s8[:, :fc.N_ALL + 1].tobytes() and fitted.sum() >= 10  # y, x, cell, flags, n, n_all
            for mine, theirs in S8_SAME:
                assert all(same_bits(a, b) for a, b in zip(got[:, mine], s8[:, theirs])), (v, how, mine)
            assert same_bits(got[:, CHI2], s8[:, fc.CHI2] * (1.0 / v))
            sums = ~np.isnan(got[:, SW])
            assert same_bits(got[sums, SW], s8[sums, fc.N_USE] * (1.0 / v)) and same_bits(got[sums, SM], s8[sums, fc.SM])
            for mine, theirs in ((SWM, fc.SM), (SWMM, fc.SMM), (SWD, fc.SD), (SWDM, fc.SDM), (SWDD, fc.SDD)):
                assert same_bits(got[sums, mine], s8[sums, theirs] * (1.0 / v)), (v, how, mine)
            n, D8 = s8[fitted, fc.N_USE], s8[fitted, fc.N_USE] * s8[fitted, fc.SMM] - s8[fitted, fc.SM] * s8[fitted, fc.SM]
            assert same_bits(got[fitted, VAR_F], v * (n / D8))
            print(f"v = {v:g} as a {how}: {int(fitted.sum())} fitted rows keep S8's f, bg, abs_res and peak; chi2 and var_f scale exactly")


def check_row_counts(make_finder, make_model, walk_waves: int) -> None:
    """0 ... 2 WALK_WAVES + 1 positions; row i is the same position fitted alone; 0 launches nothing."""
    assert ROW_COUNTS == (0, walk_waves - 1, walk_waves, walk_waves + 1, 2 * walk_waves + 1)
    whole = None
    for k in reversed(ROW_COUNTS):
        c, times = case(f"{k} rows"), []
        got = run(make_finder, make_model, c, times)[1][3.5]
        assert got.shape == (k, COLUMNS) and got.dtype == np.float64
        whole = got if whole is None else whole
        assert got.tobytes() == whole[:k].tobytes()  # a row does not depend on its neighbours in the workgroup
        assert (times[0] == 0.0) == (k == 0), (k, times)
    c = case(f"{ROW_COUNTS[-1]} rows")
    assert len(set(whole[:, FLAGS].tolist())) >= 3  # waves of one workgroup that fit, stop at the solve and take counts only
    finder, model_ = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"])
    try:
        finder.background_device(c["frame"], c["mask"])
        finder.variance(c["variance"])
        for i in range(len(whole)):
            alone = finder.fit_weighted(model_, c["positions"][i:i + 1], c["cells"][i:i + 1], 3.5, True, True)
            assert alone.tobytes() == whole[i:i + 1].tobytes(), i
    finally:
        model_.close()
        finder.close()


def check_reproducible(make_finder, make_model, name: str) -> None:
    """Repeats are bit-equal: on a fresh finder and model, by a second call on the same frame, and with other calls in between."""
    c = case(name)
    radius = c["radii"][-1]
    rows = run(make_finder, make_model, c)[1][radius]
    assert run(make_finder, make_model, c)[1][radius].tobytes() == rows.tobytes()
    finder, model_, other_model = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"]), make_model(fc.model(16))
    try:
        finder.background_device(c["frame"], c["mask"])
        if c["variance"] is not None:
            finder.variance(c["variance"])
        args = (model_, c["positions"], c["cells"], radius, c["fit_background"], c["background"] == "mesh", c["sky_variance"], c["gain"])
        one = finder.fit_weighted(*args)
        other = finder.fit_weighted(other_model, c["positions"][::-1], c["cells"], 6.5, not c["fit_background"], False, 0.5, 3.0)
        two = finder.fit_weighted(*args)
        assert one.tobytes() == two.tobytes() == rows.tobytes() and other.shape == one.shape
    finally:
        model_.close()
        other_model.close()
        finder.close()


def check_isolation(make_finder, make_model) -> None:
    """S8, S6, S7, detect and measure give the bytes they gave before a weighted fit and before a variance frame on the same finder; the
    weighted fit's rows do not depend on them; the variance frame outlives a new frame."""
    c = case("N = 9, mesh, flux and background, map")
    radii = (2.0, 4.0)
    finder, model_ = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"])
    try:
        finder.background_device(c["frame"], c["mask"])
        rows = finder.detect_device(3.0, 5, None)
        shapes = finder.measure()
        phot = finder.photometry(rows[:, :2], radii, 5, True)
        refined = finder.refine(rows[:, :2], 1.5)
        cells = np.zeros(len(rows), np.int32)
        fits = finder.fit(model_, rows[:, :2], cells, 3.5)
        assert len(rows) == 5 and np.all(fits[:, fc.FLAGS] == 0)

        def untouched() -> None:
            assert finder.fit(model_, rows[:, :2], cells, 3.5).tobytes() == fits.tobytes()
            assert finder.photometry(rows[:, :2], radii, 5, True).tobytes() == phot.tobytes()
            assert finder.refine(rows[:, :2], 1.5).tobytes() == refined.tobytes()
            assert finder.measure().tobytes() == shapes.tobytes()

        finder.variance(c["variance"])
        untouched()
        weighted = finder.fit_weighted(model_, rows[:, :2], cells, 3.5)
        assert np.all(weighted[:, FLAGS] == 0)
        untouched()
        by_model = finder.fit_weighted(model_, c["positions"], c["cells"], 1.0, False, False, 0.3, 2.0)
        untouched()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes()  # the frame, the mask and the mesh are what they were
        assert finder.fit_weighted(model_, rows[:, :2], cells, 3.5).tobytes() == weighted.tobytes()
        finder.background_device(c["frame"], c["mask"])  # a new frame: the variance frame stays
        assert finder.fit_weighted(model_, rows[:, :2], cells, 3.5).tobytes() == weighted.tobytes()
        assert finder.fit_weighted(model_, c["positions"], c["cells"], 1.0, False, False, 0.3, 2.0).tobytes() == by_model.tobytes()
        finder.variance(np.ones(SHAPE, np.float32))  # another map: other rows, and back
        assert finder.fit_weighted(model_, rows[:, :2], cells, 3.5).tobytes() != weighted.tobytes()
        finder.variance(c["variance"].astype(np.float64))  # (float32 values in float64: the same map)
        assert finder.fit_weighted(model_, rows[:, :2], cells, 3.5).tobytes() == weighted.tobytes()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes()  # (measure needs a detect of the new frame)
        untouched()
    finally:
        model_.close()
        finder.close()


def check_errors(make_finder, make_model, error: type) -> None:
    """RPSF_E_STATE (-6) before a background_device of a frame, and in map mode before a variance frame; RPSF_E_BADARG (-1) for a bad
    radius, position or noise model, whatever the state."""
    import pytest

    c = case("N = 9, mesh, flux and background, map")
    p, k = c["positions"][:6], c["cells"][:6]
    finder, model_, small = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"]), make_model(fc.model(8))
    by_map, by_model = (model_, p, k, 3.5, True, True), (model_, p, k, 3.5, True, True, 0.3, 2.0)
    bad = [(model_, p, k, 0.0, True, True), (model_, p, k, -1.0, True, True), (model_, p, k, np.nan, True, True), (model_, p, k, np.inf, True, True),
           (model_, p, k, 3.5000001, True, True), (model_, p, k, 64.5, False, False),
           (small, p, k, 3.5, True, True), (small, p, k, 3.5, True, True, 0.3, 2.0),  # N = 8 admits R <= 3: the table's R = 3.5 is refused
           (model_, [(np.nan, 1.0)], [0], 3.5, True, True), (model_, [(1.0, np.inf)], [0], 3.5, True, True),
           (model_, [(2.0 ** 20, 1.0)], [0], 3.5, True, True), (model_, [(1.0, 1.0), (1.0, -2.0 ** 20)], [0, 0], 3.5, True, False),
           *((model_, p, k, 3.5, True, True, sky, gain) for sky, gain in ((-0.1, 2.0), (np.nan, 2.0), (np.inf, 2.0), (0.3, 0.0), (0.3, -1.0),
                                                                           (0.3, np.nan), (0.3, -np.inf), (0.0, np.inf), (-0.0, np.inf)))]
    try:
        def refused(args, code):
            with pytest.raises(error) as caught:
                finder.fit_weighted(*args)
            assert caught.value.code == code, (args[3:], caught.value.code)

        refused(by_map, -6)
        refused(by_model, -6)
        finder.variance(c["variance"])  # a variance frame is no frame
        refused(by_map, -6)
        for args in bad:
            refused(args, -1)
        with pytest.raises(stars.IncorrectShapeError):
            finder.variance(np.ones((SHAPE[0], SHAPE[1] + 1), np.float32))
    finally:
        finder.close()
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        finder.background_device(c["frame"], c["mask"])
        refused(by_map, -6)  # no variance frame yet
        assert finder.fit_weighted(*by_model).shape == (6, COLUMNS)  # the noise model needs none
        for args in bad:
            refused(args, -1)
        finder.variance(c["variance"])
        rows = finder.fit_weighted(*by_map)
        assert finder.fit_weighted(small, p, k, 3.0, False, True).shape == (6, COLUMNS)
        assert finder.fit_weighted(model_, p, k, 3.5, True, True, 0.0, 1e-300).shape == (6, COLUMNS)  # any positive gain
        assert finder.fit_weighted(model_, p, k, 3.5, True, True, 1e-300, np.inf).shape == (6, COLUMNS)
        for args in bad:
            refused(args, -1)
        assert finder.fit_weighted(*by_map).tobytes() == rows.tobytes()
    finally:
        model_.close()
        small.close()
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ the statistics
# 256 isolated stars on a grid of 12 pixels, R = 3.5: the discs are disjoint.  The frame is the fitted model itself - the bilinear cell cut at
# R, times the star's flux - on a constant, plus Gaussian noise drawn pixel by pixel from the variance map the fit is given, rounded to
# float32 (the rounding, 6e-5 at a pixel value of 1000, is far below the noise).  The fit is then exactly the linear model the formal errors
# are derived for, so the pulls (flux - true) / flux_err are unit normal and chi2 is chi-square with dof = n - 2 degrees of freedom.
STAT_GRID, STAT_STEP, STAT_RADIUS, STAT_N, STAT_LEVEL = 16, 12, 3.5, 9, 50.0
STAT_SHAPE = (STAT_GRID * STAT_STEP, STAT_GRID * STAT_STEP)


def _stat_field(seed, variance: np.ndarray) -> dict:
    rng = np.random.default_rng(seed)
    gy, gx = np.mgrid[0:STAT_GRID, 0:STAT_GRID]
    truth = np.stack([gy.ravel(), gx.ravel()], axis=-1) * float(STAT_STEP) + STAT_STEP / 2 + rng.uniform(-0.5, 0.5, (STAT_GRID ** 2, 2))
    flux = rng.uniform(2000.0, 20000.0, len(truth))
    cell = fc.model(STAT_N)[GAUSSIAN]
    frame = np.full(STAT_SHAPE, STAT_LEVEL)
    R = np.float64(STAT_RADIUS)
    for (y, x), f in zip(truth, flux):
        rr = np.arange(int(np.floor(y - R)) - 1, int(np.ceil(y + R)) + 2)
        cc = np.arange(int(np.floor(x - R)) - 1, int(np.ceil(x + R)) + 2)
        pr, pc_ = rr.astype(np.float64) - y, cc.astype(np.float64) - x
        disc = ((pr * pr)[:, None] + (pc_ * pc_)[None, :]) <= R * R
        frame[rr[0]:rr[-1] + 1, cc[0]:cc[-1] + 1] += f * fc.ref_model(cell, pr, pc_, disc)
    variance = variance.astype(np.float32)
    frame = frame + rng.normal(0.0, 1.0, STAT_SHAPE) * np.sqrt(variance.astype(np.float64))
    return sc._freeze({"frame": frame.astype(np.float32).astype(np.float64), "variance": variance, "truth": truth, "flux": flux,
                       "cube": fc.model(STAT_N), "cells": np.zeros(len(truth), np.int32)})


@functools.cache
def pull_field() -> dict:
    """A variance map that runs through a factor of 30 within any 8 consecutive pixels of a row or a column."""
    rows, cols = np.mgrid[0:STAT_SHAPE[0], 0:STAT_SHAPE[1]]
    return _stat_field([15, 67], 0.5 * 30.0 ** (((3 * rows + 5 * cols) % 8) / 7.0))


@functools.cache
def outlier_field() -> dict:
    """Unit variance, and in every disc the three pixels next to the star's own at 10^4: (0, 1), (1, 0) and (-1, -1) from it."""
    f = _stat_field([16, 67], np.ones(STAT_SHAPE))
    variance = np.ones(STAT_SHAPE)
    centre = np.rint(f["truth"]).astype(int)
    for dr, dc in ((0, 1), (1, 0), (-1, -1)):
        variance[centre[:, 0] + dr, centre[:, 1] + dc] = 1e4
    return _stat_field([16, 67], variance)


def stat_fits(f: dict, weighted: bool) -> np.ndarray:
    """The restatement's structured fits of a statistics field: fit_stars_weighted's on its map, or fit_stars'."""
    if weighted:
        rows = ref_fit_weighted(f["frame"], None, 64, None, f["cube"], f["truth"], f["cells"], STAT_RADIUS, True, "none", f["variance"])
        return stars.weighted_fit_from_sums(rows, True)
    return stars.fit_from_sums(fc.ref_fit(f["frame"], None, 64, None, f["cube"], f["truth"], f["cells"], STAT_RADIUS, True, "none"), True)


def disc_variance_ratio(f: dict) -> np.ndarray:
    """Per star the largest over the smallest variance inside its disc."""
    rows, cols = np.mgrid[0:STAT_SHAPE[0], 0:STAT_SHAPE[1]]
    v = f["variance"].astype(np.float64)
    out = []
    for y, x in f["truth"]:
        inside = (rows - y) ** 2 + (cols - x) ** 2 <= STAT_RADIUS ** 2
        out.append(v[inside].max() / v[inside].min())
    return np.array(out)
