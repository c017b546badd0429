"""The star kernels (S6 star_photometry, S7 refine_stars, S8 fit_stars, S9 fit_positions, S10 subtract_stars, S11 fit_groups;
3.6: B1n, the neighbour-subtracted gather) at the sizes the product works at: a 200 x 232 frame with a mesh of 4 x 4 nodes and partial last
boxes on both axes, PSF models of 32 ... 256 pixels, fit radii and apertures up to 64 pixels, window sigmas up to 16.  The per-kernel case
modules stay on their small fields; this module holds the wide cases, and the checks the emulator test (tests/test_wide_host.py) and the GPU
test (tests/test_gpu_wide.py) share.

Nothing is restated here: every reference is the per-kernel module's restatement (photometry_cases.ref_photometry, refine_cases.ref_refine,
fit_cases.ref_fit, fitpos_cases.ref_fit_positions, render_cases.ref_render, group_cases.ref_fit_groups, builder_sub_cases.restate_case),
compared as that module compares it: bit for bit for S8, S9, S10, S11 and B1n, counts, peaks and positions exact and sums within THE BOUND
(photometry_cases) for S6 and S7.  A restatement is computed once per case and mesh (`cached`) and shared by the emulator, the GPU and the
repeat checks.

A check takes `make_finder(shape, box)` and `make_model(values)`: regularizepsf_amd.stars._Finder and ._Model on the GPU, EmuFinder and
EmuModel here.  It returns what the finder gave, so that the GPU test can hold it to the emulator byte for byte.
"""

from __future__ import annotations

import functools

import numpy as np

from regularizepsf_amd import stars
from tests import builder_sub_cases as bc
from tests import fit_cases as fc
from tests import fitpos_cases as fp
from tests import group_cases as gc
from tests import photometry_cases as pc
from tests import refine_cases as rc
from tests import render_cases as rn

SHAPE, BOX = (200, 232), 64  # 200 = 3 x 64 + 8, 232 = 3 x 64 + 40: a 4 x 4 mesh; 232 = 7.25 render tiles of 32 columns
# a pixel centre, exact half pixels, and three fractional positions; every disc of R = 64 lies wholly on the frame
STARS = np.array([(100.0, 116.0), (70.5, 150.5), (131.3, 78.6), (64.7, 64.2), (120.4, 167.1)])
AMPLITUDES = (400.0, 250.0, 300.0, 150.0, 500.0)
STAR_SIGMA = 12.0
OFF, FAR = (-40.0, -40.0), (2.0 ** 20 - 0.5, -(2.0 ** 20 - 0.5))
BROAD, NARROW, LOBES, CONSTANT = range(4)
SIZES = ((32, 15.0), (129, 63.5), (130, 64.0), (255, 64.0), (256, 64.0), (256, 40.3))  # (N, R): the issue's table
EmuFinder, EmuModel = gc.EmuFinder, gc.EmuModel  # the last of the chain: every kernel's method


# ------------------------------------------------------------------------------------------------------------------ the frames and models
@functools.cache
def field() -> dict:
    """200 x 232: a tilted background, noise of 0.3 and five Gaussian stars of sigma 12, rounded to float32 once."""
    rng = np.random.default_rng([14, 67])
    rows, cols = np.mgrid[0:SHAPE[0], 0:SHAPE[1]].astype(np.float64)
    frame = 10.0 + 0.01 * rows - 0.02 * cols + rng.normal(0.0, 0.3, SHAPE)
    for (r, c), amplitude in zip(STARS, AMPLITUDES):
        frame += amplitude * np.exp(-0.5 * ((rows - r) ** 2 + (cols - c) ** 2) / STAR_SIGMA ** 2)
    frame = frame.astype(np.float32).astype(np.float64)
    frame.flags.writeable = False
    return {"frame": frame}


@functools.cache
def masked_field() -> dict:
    """The field with a NaN beside a star's centre, both infinities near it, a masked block over the left half of star 1 and one over the
    core of star 2."""
    frame, mask = field()["frame"].copy(), np.zeros(SHAPE, bool)
    frame[100, 117] = np.nan
    frame[101, 114], frame[98, 119] = np.inf, -np.inf
    mask[50:90, 120:151] = True
    mask[110:150, 60:100] = True
    frame.flags.writeable = mask.flags.writeable = False
    return {"frame": frame, "mask": mask}


def positions() -> np.ndarray:
    """The stars, the frame's corners, one position wholly off the frame and the largest one admitted."""
    H, W = SHAPE
    return np.concatenate([STARS, [(0.0, 0.0), (0.0, W - 1.0), (H - 1.0, 0.0), (H - 1.0, W - 1.0), OFF, FAR]])


@functools.cache
def cube(n: int) -> np.ndarray:
    """Four cells of n x n around h = n / 2 - 0.5: a broad positive Gaussian of sigma n / 10 and unit sum, a narrow one of sigma 1.3 whose
    far values are denormal or zero in a large cell, a difference of Gaussians with negative lobes, a constant."""
    h = n / 2.0 - 0.5
    i, j = np.mgrid[0:n, 0:n].astype(np.float64)
    q = (i - h) ** 2 + (j - h) ** 2
    g = lambda sigma: np.exp(-0.5 * q / sigma ** 2)  # noqa: E731
    out = np.stack([g(n / 10.0) / g(n / 10.0).sum(), g(1.3) / g(1.3).sum(), g(n / 16.0) - 0.4 * g(n / 8.0), np.full((n, n), 0.25)])
    assert out[BROAD].min() > 0.0 and out[LOBES].min() < 0.0
    out.flags.writeable = False
    return out


def kind(make_finder) -> str:
    """Which finder a check runs on, for the figures it prints."""
    return "emulator" if isinstance(make_finder, type) and issubclass(make_finder, pc.EmuFinder) else "GPU"


_CACHE: dict = {}


def cached(key: tuple, level_f, compute):
    """`compute()` once per key and filtered mesh."""
    k = (key, None if level_f is None else np.ascontiguousarray(level_f).tobytes())
    if k not in _CACHE:
        _CACHE[k] = compute()
    return _CACHE[k]


def _frame_of(masked: bool) -> tuple:
    m = masked_field() if masked else {"frame": field()["frame"], "mask": None}
    return m["frame"], m["mask"]


# ------------------------------------------------------------------------------------------------------------------ S6
def _phot_case(radii, subpix, background, masked) -> dict:
    frame, mask = _frame_of(masked)
    return pc._case(frame, positions(), radii, subpix, background, mask, BOX)


PHOT_CASES = {
    "eight apertures to 64, s = 8, mesh": lambda: _phot_case((0.05, 1.0, 4.0, 16.0, 32.0, 48.0, 63.5, 64.0), 8, "mesh", False),
    "eight apertures to 64, s = 8, masked, none": lambda: _phot_case((0.05, 1.0, 4.0, 16.0, 32.0, 48.0, 63.5, 64.0), 8, "none", True),
    "R = 64, s = 1, masked, mesh": lambda: _phot_case((64.0,), 1, "mesh", True),
}


@functools.cache
def phot_case(name: str) -> dict:
    return PHOT_CASES[name]()


def check_photometry(make_finder, name: str) -> np.ndarray:
    c = phot_case(name)
    level_f, rows = pc.run(make_finder, c)
    ref = cached(("S6", name), level_f if c["background"] == "mesh" else None, lambda: pc.ref_photometry(
        c["frame"], c["mask"], c["box"], level_f, c["positions"], c["radii"], c["subpix"], c["background"]))
    m = len(c["radii"])
    worst = pc.compare(rows, ref, m, f"{kind(make_finder)}: S6, {name}")
    n_all = ref["rows"][0, 2 + 3 * m - 1] / c["subpix"] ** 2
    print(f"{kind(make_finder)}: S6, {name}: the interior star's outermost aperture holds {n_all:.1f} pixels; worst error / bound {worst:.2e}")
    assert n_all >= 12000 and rows[0, 2 + 3 * m - 1] == ref["rows"][0, 2 + 3 * m - 1]  # pi 64^2 = 12 868
    return rows


# ------------------------------------------------------------------------------------------------------------------ S7
def _refine_case(max_iter, background, masked) -> dict:
    frame, mask = _frame_of(masked)
    return rc._case(frame, positions(), np.resize(np.array([16.0, 12.0, 8.0, 0.5]), len(positions())), background, mask, BOX, max_iter=max_iter)


REFINE_CASES = {
    "sigmas 16 to 0.5, max_iter 0, mesh": lambda: _refine_case(0, "mesh", False),
    "sigmas 16 to 0.5, max_iter 16, mesh": lambda: _refine_case(16, "mesh", False),
    "sigmas 16 to 0.5, max_iter 0, masked, none": lambda: _refine_case(0, "none", True),
    "sigmas 16 to 0.5, max_iter 16, masked, none": lambda: _refine_case(16, "none", True),
}


@functools.cache
def refine_case(name: str) -> dict:
    return REFINE_CASES[name]()


def check_refine(make_finder, name: str) -> np.ndarray:
    """max_iter = 0: the walk against the restatement (compare_walk: positions and counts exact, sums within THE BOUND).  max_iter = 16:
    refine_cases' THE CHAIN - the run with max_iter = j + 1 is the rules applied to the finder's own run with max_iter = j, bit for bit
    (refine_cases.predict); the ends (niter, flags) are the restatement's and the delivered positions lie within a derived bound of the restatement's (the starts
    and the rows that took no step bit for bit); and the delivered walk is the restatement's walk at the
    position the finder delivered, counts exact and sums within THE BOUND."""
    c = refine_case(name)
    mesh = c["background"] == "mesh"
    level_f, rows = rc.run(make_finder, c)
    ref = cached(("S7", name), level_f if mesh else None, lambda: rc.ref_refine(
        c["frame"], c["mask"], c["box"], level_f, c["positions"], c["sigma"], c["background"], c["max_iter"], c["eps"], c["max_shift"]))
    assert c["sigma"][0] == 16.0 and rows[0, rc.N_ALL] >= 12000 and ref["rows"][0, rc.N_ALL] >= 12000
    if c["max_iter"] == 0:
        worst = rc.compare_walk(rows, ref, f"{kind(make_finder)}: S7, {name}")
        print(f"{kind(make_finder)}: S7, {name}: N_all of the interior star at sigma 16: {int(rows[0, rc.N_ALL])}, worst error / bound {worst:.2e}")
        return rows
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        finder.background_device(c["frame"], c["mask"])
        runs = [finder.refine(c["positions"], c["sigma"], j, c["eps"], c["max_shift"], mesh) for j in range(c["max_iter"] + 1)]
    finally:
        finder.close()
    assert runs[-1].tobytes() == rows.tobytes()
    moved = 0
    for j in range(c["max_iter"]):
        want = rc.predict(runs[j], c, j)
        new = np.isnan(want[:, rc.N_USE])
        moved += int(new.sum())
        assert runs[j + 1][:, :rc.N_USE].tobytes() == want[:, :rc.N_USE].tobytes(), f"{name}: max_iter = {j + 1} is not the rules applied to max_iter = {j}"
        assert runs[j + 1][~new].tobytes() == want[~new].tobytes(), f"{name}: a stopped star's row changed at max_iter = {j + 1}"
    niter, flags = rows[:, rc.NITER].astype(int), rows[:, rc.FLAGS].astype(int)
    print(f"{kind(make_finder)}: S7, {name}: {moved} steps predicted bit for bit, niter {niter.tolist()}, flags {flags.tolist()}, the restatement's "
          f"{ref['rows'][:, rc.NITER].astype(int).tolist()} and {ref['rows'][:, rc.FLAGS].astype(int).tolist()}")
    assert np.array_equal(rows[:, rc.NITER:rc.FLAGS + 1], ref["rows"][:, rc.NITER:rc.FLAGS + 1]) and moved >= len(rows) and niter.max() >= 2
    # The delivered positions against the restatement's.  The two sides add the same terms in different orders, so a step (mr, mc) / S is
    # not the same double on both; it is held to a bound, not to the bits.  With b = 2 n u A the bound on S and b P the bound on mr (THE
    # BOUND, P the box's half extent), one step's dy differs by at most (b P + |dy| b) / (S - b), |dy| <= max_shift, and the position moves
    # by twice that.  b, P and S are read from the restatement's delivered walk; the walks before it lie at most max_shift away, for which
    # a factor 2 stands.  The iteration draws the position towards the windowed centroid, it does not push two nearby positions apart,
    # so the errors of the niter accepted steps add at most: |y - ref| <= niter 2 . 2 b (P + max_shift) / (S - b), likewise x with Q.  A
    # row that took no step sits at its start on both sides, bit for bit, and every start is the case's position.
    want, bounds = ref["rows"], ref["bounds"]
    assert rows[:, rc.Y0:rc.X0 + 1].tobytes() == want[:, rc.Y0:rc.X0 + 1].tobytes() == c["positions"].tobytes()
    still = niter == 0
    assert rows[still, rc.Y:rc.X + 1].tobytes() == want[still, rc.Y:rc.X + 1].tobytes() == c["positions"][still].tobytes()
    b, total = bounds[~still, 0], want[~still, rc.S]
    assert np.all(b > 0.0) and np.all(total > b), (name, b, total)
    for column, extent in ((rc.Y, bounds[~still, 2] / b), (rc.X, bounds[~still, 3] / b)):
        limit = niter[~still] * 2.0 * 2.0 * b * (extent + c["max_shift"]) / (total - b)
        off = np.abs(rows[~still, column] - want[~still, column])
        print(f"{kind(make_finder)}: S7, {name}: column {column}: the delivered positions lie at most {off.max():.2e} px from the restatement's, "
              f"the bounds are {limit.min():.2e} ... {limit.max():.2e} px")
        assert np.all(off <= limit), (name, column, off, limit)
    here = cached(("S7 at", name, rows[:, rc.Y:rc.X + 1].tobytes()), level_f if mesh else None, lambda: rc.ref_refine(
        c["frame"], c["mask"], c["box"], level_f, rows[:, rc.Y:rc.X + 1], c["sigma"], c["background"], 0))
    walk = rows.copy()
    walk[:, rc.Y0:rc.X0 + 1], walk[:, rc.NITER:rc.FLAGS + 1], walk[:, rc.DY:rc.DX + 1] = rows[:, rc.Y:rc.X + 1], 0.0, np.nan
    worst = rc.compare_walk(walk, here, f"{kind(make_finder)}: S7, {name}, the delivered walk")
    print(f"{kind(make_finder)}: S7, {name}: worst error / bound of the delivered walk {worst:.2e}")
    return rows


# ------------------------------------------------------------------------------------------------------------------ S8
def fit_rows() -> tuple[np.ndarray, np.ndarray]:
    """Every star with every cell; the corners and the position off the frame with the broad cell, the far one with the narrow one; the
    first star with the cell indices -1 and n_cells."""
    p = positions()
    pos = [s for s in STARS for _ in range(4)] + list(p[5:]) + [STARS[0], STARS[0]]
    cells = [k for _ in STARS for k in range(4)] + [BROAD] * 5 + [NARROW] + [-1, 4]
    return np.array(pos), np.array(cells, np.int32)


def _fit_case(n, radius, background="mesh", fit_background=True, masked=False) -> dict:
    frame, mask = _frame_of(masked)
    return fc._case(frame, *fit_rows(), n, background, fit_background, mask, (radius,), BOX, cube(n))


FIT_SIZE_CASES = {f"N = {n}, R = {r:g}": functools.partial(_fit_case, n, r) for n, r in SIZES}
FIT_CASES = {
    **FIT_SIZE_CASES,
    "N = 130, R = 64, masked, none, flux alone": lambda: _fit_case(130, 64.0, "none", False, True),
    "N = 255, R = 64, masked, mesh, flux alone": lambda: _fit_case(255, 64.0, "mesh", False, True),
    "N = 256, R = 64, none, flux and background": lambda: _fit_case(256, 64.0, "none", True, False),
    "no valid mesh node": lambda: fc._case(np.full(SHAPE, np.nan, np.float32), positions()[:7], [BROAD, NARROW, LOBES, CONSTANT, 7, -1, BROAD], 130,
                                           radii=(64.0,), box=BOX, cube=cube(130)),
}


@functools.cache
def fit_case(name: str) -> dict:
    return FIT_CASES[name]()


def check_fit(make_finder, make_model, name: str) -> np.ndarray:
    c = fit_case(name)
    radius = c["radii"][0]
    level_f, rows = fc.run(make_finder, make_model, c)
    got = rows[radius]
    want = cached(("S8", name), level_f if c["background"] == "mesh" else None, lambda: fc.ref_fit(
        c["frame"], c["mask"], c["box"], level_f, c["cube"], c["positions"], c["cells"], radius, c["fit_background"], c["background"]))
    assert got.dtype == np.float64 and got.shape == want.shape
    flags = got[:, fc.FLAGS].astype(int)
    differ = [i for i in range(len(want)) if not fc.same_bits(got[i], want[i])]
    print(f"{kind(make_finder)}: S8, {name}: {len(want)} rows, {int((flags == 0).sum())} fitted, flags {sorted(set(flags.tolist()))}, N_all of the interior star "
          f"{int(want[0, fc.N_ALL])}, {len(differ)} rows differ from the restatement")
    assert not differ, (name, differ[:3], got[differ[0]], want[differ[0]])
    if name in FIT_SIZE_CASES:
        assert 2 * int((want[:, fc.FLAGS] == 0).sum()) >= len(want) and 2 * int((flags == 0).sum()) >= len(got), name
    if radius == 64.0:
        assert want[0, fc.N_ALL] >= 12000 and got[0, fc.N_ALL] >= 12000
    return got


def check_fit_flags(all_rows: dict) -> None:
    """`all_rows`: {name: rows} of every FIT_CASES entry.  Each flag fires somewhere."""
    seen = {int(f) for rows in all_rows.values() for f in rows[:, fc.FLAGS]}
    bits = {b for f in seen for b in (fc.NO_MESH, fc.TOO_FEW, fc.DEGENERATE, fc.BAD_CELL) if f & b}
    print(f"S8: flags seen over {len(all_rows)} cases: {sorted(seen)}")
    assert set(all_rows) == set(FIT_CASES) and 0 in seen and bits == {fc.NO_MESH, fc.TOO_FEW, fc.DEGENERATE, fc.BAD_CELL}


# ------------------------------------------------------------------------------------------------------------------ S9
def fitpos_rows() -> tuple[np.ndarray, np.ndarray]:
    """Every star from (0.5, -0.5) off, 0.71 px, with the broad cell; the first star with the other cells and a bad index; a corner and
    the position off the frame.  (The far position is left out: a start must stay inside |y|, |x| < 2^20.)"""
    start = STARS + (0.5, -0.5)
    pos = list(start) + [start[0]] * 4 + [(0.0, 0.0), OFF]
    cells = [BROAD] * 5 + [NARROW, LOBES, CONSTANT, -1] + [BROAD, BROAD]
    return np.array(pos), np.array(cells, np.int32)


def _fitpos_case(n, radius, background="mesh", fit_background=True, masked=False, **iteration) -> dict:
    frame, mask = _frame_of(masked)
    return fp._case(frame, *fitpos_rows(), n, background, fit_background, mask, (radius,), BOX, cube(n), **iteration)


FITPOS_CASES = {
    **{f"N = {n}, R = {r:g}": functools.partial(_fitpos_case, n, r) for n, r in SIZES},
    "N = 130, R = 64, masked, none, flux alone, max_shift 0.3": lambda: _fitpos_case(130, 64.0, "none", False, True, max_shift=0.3),
}


@functools.cache
def fitpos_case(name: str) -> dict:
    return FITPOS_CASES[name]()


def check_fitpos(make_finder, make_model, name: str) -> tuple[np.ndarray, np.ndarray]:
    c = fitpos_case(name)
    radius = c["radii"][0]
    level_f, rows = fp.run(make_finder, make_model, c, also_fit=True)
    steps, fits, own = rows[radius]

    def compute():
        common = (c["frame"], c["mask"], c["box"], level_f, c["cube"])
        s = fp.ref_fit_positions(*common, c["positions"], c["cells"], radius, c["fit_background"], c["background"], **c["iteration"])
        return s, fc.ref_fit(*common, s[:, fp.Y:fp.X + 1], c["cells"], radius, c["fit_background"], c["background"])

    want_steps, want_fits = cached(("S9", name), level_f if c["background"] == "mesh" else None, compute)
    flags, niter = steps[:, fp.FLAGS].astype(int), steps[:, fp.NITER].astype(int)
    differ = [i for i in range(len(steps)) if not fp.same_bits(steps[i], want_steps[i])]
    print(f"{kind(make_finder)}: S9, {name}: {len(steps)} rows, flags {flags.tolist()}, niter {niter.tolist()}, {len(differ)} rows differ from the restatement")
    assert steps.shape == want_steps.shape and not differ, (name, differ[:3], steps[differ[0]], want_steps[differ[0]])
    assert fits.tobytes() == own.tobytes()  # S8 itself at the position returned
    differ = [i for i in range(len(fits)) if not fc.same_bits(fits[i], want_fits[i])]
    assert not differ, (name, differ[:3])
    return steps, fits


def check_fitpos_ends(all_steps: dict) -> None:
    """`all_steps`: {name: iteration rows} of every FITPOS_CASES entry: some rows converge after two iterations or more, and in the run
    with the small max_shift a star stops on it."""
    assert set(all_steps) == set(FITPOS_CASES)
    converged = sum(int(((s[:, fp.FLAGS] == 0) & (s[:, fp.NITER] >= 2)).sum()) for s in all_steps.values())
    away = all_steps["N = 130, R = 64, masked, none, flux alone, max_shift 0.3"]
    print(f"S9: {converged} rows converge after >= 2 iterations; with max_shift 0.3 the flags are {away[:, fp.FLAGS].astype(int).tolist()}")
    assert converged >= 5 and np.any(away[:, fp.FLAGS].astype(int) & fp.RAN_AWAY)


# ------------------------------------------------------------------------------------------------------------------ S10
def render_frame() -> np.ndarray:
    return masked_field()["frame"].astype(np.float32)  # a NaN and both infinities among the pixels


@functools.cache
def render_stars() -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(positions, flux, cells): the positions above, 300 uniform ones on the frame and a 30-pixel skirt around it, and a pile of two
    chunks and five inside one tile; fluxes of both signs, a NaN flux and a cell outside the model among them."""
    rng = np.random.default_rng([15, 67])
    tile_r, tile_c, chunk = rn.emulator_info()[:3]
    uniform = np.stack([rng.uniform(-30.0, SHAPE[0] + 30.0, 300), rng.uniform(-30.0, SHAPE[1] + 30.0, 300)], axis=-1)
    i = np.arange(2 * chunk + 5, dtype=np.float64)
    pile = np.stack([tile_r * 10.5 + 0.37 * np.sin(i), tile_c * 3.5 + 1.9 * np.cos(0.7 * i)], axis=-1)
    pos = np.concatenate([positions(), uniform, pile])
    flux = rng.uniform(20.0, 400.0, len(pos)) * np.where(rng.random(len(pos)) < 0.3, -1.0, 1.0)
    cells = rng.integers(0, 4, len(pos)).astype(np.int32)
    flux[13], cells[17], cells[19] = np.nan, 4, -1
    for a in (pos, flux, cells):
        a.flags.writeable = False
    return pos, flux, cells


ALL_OUTPUTS = tuple((mode, dtype) for mode in rn.MODES for dtype in rn.DTYPES)


def _render_case(n, radius, outputs=ALL_OUTPUTS, few=False) -> dict:
    pos, flux, cells = render_stars()
    if few:  # the eleven positions alone: most tiles see no star
        pos, flux, cells = pos[:11], flux[:11], cells[:11]
    return {"frame": render_frame(), "box": BOX, "cube": cube(n), "positions": pos, "flux": flux, "cells": cells, "radius": radius,
            "outputs": tuple(outputs)}


SOME_OUTPUTS = ((rn.MODEL, np.float64), (rn.RESIDUAL_MESH, np.float32))
RENDER_CASES = {
    "N = 32, R = 15": lambda: _render_case(32, 15.0),
    "N = 32, R = 15, eleven stars": lambda: _render_case(32, 15.0, few=True),
    "N = 129, R = 63.5": lambda: _render_case(129, 63.5, SOME_OUTPUTS),
    "N = 130, R = 64": lambda: _render_case(130, 64.0),
    "N = 255, R = 64": lambda: _render_case(255, 64.0, SOME_OUTPUTS),
    "N = 256, R = 64": lambda: _render_case(256, 64.0),
    "N = 256, R = 40.3": lambda: _render_case(256, 40.3, SOME_OUTPUTS),
}


@functools.cache
def render_case(name: str) -> dict:
    return RENDER_CASES[name]()


def check_render(make_finder, make_model, name: str) -> dict:
    """Every output of the case against the restatement, bit for bit.  Returns {(mode, dtype name): frame}."""
    c = render_case(name)
    finder, model = make_finder(SHAPE, BOX), None
    try:
        model = make_model(c["cube"])
        level, rms = finder.background(c["frame"], None)
        level_f = stars.filter_mesh(level, rms)[0]
        finder.background_device(c["frame"], None)
        frames = {(mode, np.dtype(dtype).name): finder.render(model, c["positions"], c["flux"], c["cells"], c["radius"], mode, dtype)
                  for mode, dtype in c["outputs"]}
    finally:
        if model is not None:
            model.close()
        finder.close()
    want_drawn = int(rn.drawn(c["flux"], c["cells"], len(c["cube"])).sum())
    for (mode, dtype), (got, count) in frames.items():
        want = cached(("S10", name, mode, dtype), level_f if mode == rn.RESIDUAL_MESH else None, lambda: rn.ref_render(
            c["frame"], c["box"], level_f, c["cube"], c["positions"], c["flux"], c["cells"], c["radius"], mode, np.dtype(dtype)))
        differ = int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want)))))
        print(f"{kind(make_finder)}: S10, {name}, mode {mode}, {dtype}: {len(c['positions'])} stars, {count} drawn, {differ} pixels differ from the restatement")
        assert count == want_drawn and rn.same_frame(got, want), (name, mode, dtype, differ)
    return {key: got for key, (got, _) in frames.items()}


def check_render_lists() -> None:
    """The tile lists of the cases, from the host code the product builds them with: some list is longer than two chunks, some list is
    empty, and the last tile column is partial."""
    tile_r, tile_c, chunk = rn.emulator_info()[:3]
    longest, empty = 0, 0
    for name in RENDER_CASES:
        c = render_case(name)
        offsets, _, _ = rn.tile_lists(SHAPE, c["cube"], c["positions"], c["flux"], c["cells"], c["radius"])
        lengths = np.diff(offsets)
        assert len(lengths) == -(-SHAPE[0] // tile_r) * -(-SHAPE[1] // tile_c)
        print(f"S10, {name}: {len(lengths)} tiles of {tile_r} x {tile_c}, lists of {int(lengths.min())} ... {int(lengths.max())} stars, "
              f"{int((lengths == 0).sum())} empty (a chunk holds {chunk})")
        longest, empty = max(longest, int(lengths.max())), empty + int((lengths == 0).sum())
        if not name.endswith("eleven stars"):
            assert lengths.max() > 2 * chunk, name
    assert longest > 2 * chunk and empty > 0 and SHAPE[1] % tile_c != 0 and SHAPE[0] % tile_r == 0


# ------------------------------------------------------------------------------------------------------------------ S11
LINK = 20.0
GROUP_SIZES = [2, 2, 3, 3, 3] + [8] * 8 + [9] * 9 + [1] + [2, 2] + [2, 2]


def crowd() -> tuple[np.ndarray, np.ndarray]:
    """Groups whose members are at most LINK apart and which are more than LINK from one another: a pair across the box line at row 128,
    three, a chain of eight across the mesh's node line at column 159.5, a pile of nine (crowded), a star alone, a pair across the rim, a pair wholly off the frame."""
    pair = [(120.3, 100.6), (134.8, 103.1)]
    three = [(60.5, 60.5), (70.0, 66.0), (64.0, 75.2)]
    eight = [(100.2 + 0.3 * k, 150.0 + 6.0 * k) for k in range(8)]
    pile = [(160.0, 40.0 + 1.5 * k) for k in range(9)]
    alone = [(30.3, 200.6)]
    rim = [(198.5, 120.0), (203.0, 131.0)]
    off = [(-80.0, -80.0), (-85.5, -73.0)]
    pos = np.array(pair + three + eight + pile + alone + rim + off)
    cells = np.resize(np.array([BROAD, NARROW, BROAD, LOBES], np.int32), len(pos))
    return pos, cells


def _group_case(n, radius, background, fit_background, masked=False) -> dict:
    frame, mask = _frame_of(masked)
    return gc._case(frame, *crowd(), n, background, fit_background, mask, (radius,), BOX, cube(n), LINK)


GROUP_CASES = {
    **{f"N = 130, R = 64, {b}, {'flux and background' if fb else 'flux alone'}": functools.partial(_group_case, 130, 64.0, b, fb)
       for b in ("mesh", "none") for fb in (True, False)},
    "N = 32, R = 15, mesh, flux and background": lambda: _group_case(32, 15.0, "mesh", True),
    "N = 256, R = 40.3, masked, none, flux alone": lambda: _group_case(256, 40.3, "none", False, True),
    "N = 255, R = 64, masked, mesh, flux and background": lambda: _group_case(255, 64.0, "mesh", True, True),
}


@functools.cache
def group_case(name: str) -> dict:
    return GROUP_CASES[name]()


def group_reference(name: str, level_f) -> np.ndarray:
    c = group_case(name)
    return cached(("S11", name), level_f if c["background"] == "mesh" else None, lambda: gc.ref_fit_groups(
        c["frame"], c["mask"], c["box"], level_f, c["cube"], c["positions"], c["cells"], c["radii"][0], c["fit_background"], c["background"],
        c["link"], c["max_group"]))


def check_group(make_finder, make_model, name: str) -> np.ndarray:
    c = group_case(name)
    level_f, rows = gc.run(make_finder, make_model, c)
    got, want = rows[c["radii"][0]], group_reference(name, level_f)
    sizes, flags = got[:, gc.GROUP_SIZE].astype(int), got[:, fc.FLAGS].astype(int)
    differ = [i for i in range(len(want)) if not gc.same_bits(got[i], want[i])]
    print(f"{kind(make_finder)}: S11, {name}: {len(want)} rows, group sizes {sizes.tolist()}, flags {flags.tolist()}, group_n <= "
          f"{int(np.nanmax(want[:, gc.GROUP_N]))}, {len(differ)} rows differ from the restatement")
    assert got.shape == want.shape and not differ, (name, differ[:3], got[differ[0]], want[differ[0]])
    for rows_ in (want, got):
        assert rows_[:, gc.GROUP_SIZE].astype(int).tolist() == GROUP_SIZES  # sizes {1, 2, 3, 8} and a crowded 9
        assert {1, 2, 3, 8, 9} == set(rows_[:, gc.GROUP_SIZE].astype(int).tolist()) and gc.MAX_GROUP == 8
    pos = c["positions"]
    assert pos[0, 0] // BOX != pos[1, 0] // BOX and sizes[0] == 2  # the pair lies across the box line at row 128
    node = np.floor((pos[5:13, 1] + 0.5) / BOX - 0.5)  # axis_coord's lower node column: the surface changes node pair at column 159.5
    assert set(node.tolist()) == {1.0, 2.0} and np.all(sizes[5:13] == 8)  # the chain of eight has members in different mesh cells
    return got


# ------------------------------------------------------------------------------------------------------------------ B1n
@functools.cache
def builder_case() -> dict:
    """Patches of 64 pixels cut on the wide frame with a 130-pixel model at R = 64; the neighbours are the fitted set of the S11 case
    "N = 130, R = 64, none, flux and background": its positions, its cells and the restatement's fluxes (NaN where a fit was flagged: such
    a star is not drawn)."""
    name = "N = 130, R = 64, none, flux and background"
    c = group_case(name)
    flux = group_reference(name, None)[:, fc.F].copy()
    own = np.array([0, 2, 13, 22, 23])  # of the pair, of the three, of the pile, the star alone, of the pair across the rim
    case = {"n": 64, "radius": 64.0, "frame": field()["frame"].astype(np.float32), "cube": np.array(cube(130)), "pos": c["positions"].copy(),
            "flux": flux, "cell": c["cells"].copy(), "own": np.concatenate([own, [-1, -1]]),
            "cut": np.concatenate([c["positions"][own], [STARS[0], (10.5, 220.25)]])}
    return bc._finish(case)


@functools.cache
def builder_expected() -> tuple[np.ndarray, np.ndarray]:
    c = builder_case()
    lists = bc.brute_lists(c)
    drawn = bc.star_drawn(c["flux"], c["cell"], len(c["cube"]))
    assert drawn.sum() >= 10 and min(len(l) for l in lists) >= 1 and max(len(l) for l in lists) >= 20, (int(drawn.sum()), [len(l) for l in lists])
    return bc.restate_case(c, lists)
