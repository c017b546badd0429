"""Forced aperture photometry (DESIGN.md 3.7 "Apertures", kernel S6) restated in float64 NumPy, the cases, the CPU emulator of the kernel,
and the checks the emulator tests (tests/test_photometry_host.py) and the GPU tests (tests/test_gpu_photometry.py) share.

There is no outside implementation (this is not sep's sum_circle): the reference is the restatement below, written from the definition
with array operations over each position's box.  A check takes `make_finder(shape, box)`: regularizepsf_amd.stars._Finder on the GPU,
EmuFinder here.

THE MESH.  With background="mesh" the definition's d is step 4's residual against the filtered mesh, and the mesh is S1's and S1b's
business (tests/star_cases.py, tests/stars_fused_cases.py).  The restatement therefore takes the filtered mesh as an input: the finder
under test hands out its raw mesh (`background`), the host filter (stars.filter_mesh, S1b's bits) filters it, and the restatement and the
kernel subtract the same surface, by the same expression (star_cases.ref_surface is background_at operation for operation).  So d is the
same double on both sides, and what is tested here is S6 alone.

THE COUNTS are integers computed from the same float64 expressions (o_a, pr + o_a, the products, their sum, R R, the comparison <=) on
both sides: N_use and N_all are compared exactly, as are the peak and its pixel.

THE BOUND.  Both sides add the same rounded terms in different orders.  A sum of n terms x_i added in any order is off by at most
gamma_(n-1) sum |x_i| with gamma_j = j u / (1 - j u), u = 2^-53, and gamma_(n-1) <= n u while n (n - 1) u <= 1; two orders differ by at most
twice that.  With n the number of pixels of the box (at most 133^2; the terms that are not zero are fewer), A_k = sum w_k |d| over the usable
pixels, and P = max |pr|, Q = max |pc| over the box, every term of flux_k is at most w_k |d|, of abs the same with k = m - 1, of mr at most
w |d| P, of mc w |d| Q, of mrr w |d| P^2, of mcc w |d| Q^2, of mrc w |d| P Q (their own roundings, 3 u relative, vanish in the step from n - 1
to n).  Hence
    |flux_k - ref| <= 2 n u A_k,   |abs - ref| <= 2 n u A,   |mr - ref| <= 2 n u A P,   |mc - ref| <= 2 n u A Q,
    |mrr - ref| <= 2 n u A P^2,    |mcc - ref| <= 2 n u A Q^2,    |mrc - ref| <= 2 n u A P Q
with A = A_(m-1).  Nothing measured goes into it.  Where every term is zero (an aperture off the frame) the bound is zero and the sums are
compared exactly.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np

from tests import emulib
from regularizepsf_amd import stars
from tests import shape_cases as shc
from tests import star_cases as sc

ROOT = sc.ROOT
U = 2.0 ** -53
SUMS = ("abs_flux", "mr", "mc", "mrr", "mcc", "mrc")


def columns(m: int) -> int:
    return 2 + 3 * m + 9


# ------------------------------------------------------------------------------------------------------------------ the restatement
def ref_residual(frame, mask, box, level_f, background: str):
    """(d, usable): the frame rounded to float32 once, minus the bilinear surface through `level_f` with background="mesh"."""
    frame = np.asarray(frame, np.float32).astype(np.float64)
    ok = np.isfinite(frame) & (~np.asarray(mask, bool) if mask is not None else True)
    if background == "mesh" and level_f is not None:
        with np.errstate(invalid="ignore"):
            frame = frame - sc.ref_surface(level_f, frame.shape, box)
    return frame, ok


def ref_photometry(frame, mask, box, level_f, positions, radii, subpix: int, background: str) -> dict:
    """The definition.  rows: (k, columns(m)) in the kernel's layout; bounds: (k, m + 6), THE BOUND on flux[m] and the six sums."""
    d, ok = ref_residual(frame, mask, box, level_f, background)
    H, W = d.shape
    radii = np.asarray(radii, np.float64)
    m, s = len(radii), int(subpix)
    no_mesh = background == "mesh" and level_f is None
    o = (2 * np.arange(s) + 1 - s).astype(np.float64) / np.float64(2 * s)
    r2 = radii * radii
    rows, bounds = np.empty((len(positions), columns(m))), np.empty((len(positions), m + 6))
    for i, (y, x) in enumerate(np.asarray(positions, np.float64).reshape(-1, 2)):
        rmax = radii[-1]
        rr = np.arange(int(np.floor(y - rmax)) - 1, int(np.ceil(y + rmax)) + 2)
        cc = np.arange(int(np.floor(x - rmax)) - 1, int(np.ceil(x + rmax)) + 2)
        pr, pc = rr.astype(np.float64) - y, cc.astype(np.float64) - x
        ur, uc = pr[:, None] + o[None, :], pc[:, None] + o[None, :]
        q = (ur * ur)[:, None, :, None] + (uc * uc)[None, :, None, :]  # q[r, c, a, b]
        n = np.stack([(q <= r2[k]).sum(axis=(2, 3)) for k in range(m)])  # n[k, r, c]
        inside = ((rr >= 0) & (rr < H))[:, None] & ((cc >= 0) & (cc < W))[None, :]
        use = np.zeros(inside.shape, bool)
        dbox = np.zeros(inside.shape)
        ri, ci = np.clip(rr, 0, H - 1), np.clip(cc, 0, W - 1)
        use[inside] = ok[ri[:, None], ci[None, :]][inside]
        dbox[use] = d[ri[:, None], ci[None, :]][use]
        w = n.astype(np.float64) / np.float64(s * s)
        PR, PC = np.broadcast_to(pr[:, None], use.shape)[use], np.broadcast_to(pc[None, :], use.shape)[use]
        dv, wv = dbox[use], w[:, use]
        t = wv[-1] * dv
        flux = [np.sum(wv[k] * dv) for k in range(m)]
        six = [np.sum(wv[-1] * np.abs(dv)), np.sum(t * PR), np.sum(t * PC), np.sum(t * (PR * PR)), np.sum(t * (PC * PC)), np.sum(t * (PR * PC))]
        row = rows[i]
        row[0], row[1] = y, x
        row[2:2 + m] = np.nan if no_mesh else flux
        row[2 + m:2 + 2 * m] = [n[k][use].sum() for k in range(m)]
        row[2 + 2 * m:2 + 3 * m] = [n[k].sum() for k in range(m)]
        row[2 + 3 * m:2 + 3 * m + 6] = np.nan if no_mesh else six
        seen = use & (n[-1] > 0)
        if seen.any() and not no_mesh:
            flat = np.flatnonzero(seen.ravel())
            top = flat[np.argmax(dbox.ravel()[flat])]  # the first in raster order among equals
            row[-3:] = dbox.ravel()[top], rr[top // len(cc)], cc[top % len(cc)]
        else:
            row[-3:] = np.nan, -1.0, -1.0
        npx, P, Q = use.size, np.abs(pr).max(), np.abs(pc).max()
        A = [np.sum(wv[k] * np.abs(dv)) for k in range(m)]
        bounds[i, :m] = [2 * npx * U * a for a in A]
        bounds[i, m:] = 2 * npx * U * A[-1] * np.array([1.0, P, Q, P * P, Q * Q, P * Q])
    return {"rows": rows, "bounds": bounds}


# ------------------------------------------------------------------------------------------------------------------ the frames
SHAPE, BOX = (96, 96), 32


@functools.cache
def field() -> dict:
    """96 x 96, star_cases.star_frame's background, noise and eight Gaussian stars."""
    rng = np.random.default_rng([6, 67])
    truth = sc.scattered(SHAPE, 8, rng)
    return sc._freeze({"frame": sc.star_frame(SHAPE, truth, rng), "truth": truth})


def hard_positions() -> np.ndarray:
    """On .5 ties, at (0, 0), partly off every edge, wholly off the frame, and two apertures over one another."""
    return np.array([(0.0, 0.0), (20.5, 30.5), (20.0, 30.5), (41.5, 17.0), (-1.3, 40.2), (96.7, 50.1), (40.4, -2.2), (33.3, 97.0), (95.0, 95.0),
                     (-30.0, -30.0), (200.5, 48.0), (48.0, -70.25), (60.2, 60.4), (62.9, 61.1), (60.2, 60.4)])


def _case(frame, positions, radii, subpix=5, background="mesh", mask=None, box=BOX) -> dict:
    return {"frame": frame, "mask": mask, "box": box, "positions": np.ascontiguousarray(positions, np.float64).reshape(-1, 2),
            "radii": np.asarray(radii, np.float64), "subpix": subpix, "background": background}


def _field_case(radii, subpix=5, background="mesh", count=None, box=BOX) -> dict:
    f = field()
    positions = np.concatenate([f["truth"], hard_positions()])
    return _case(f["frame"], positions if count is None else positions[:count], radii, subpix, background, box=box)


def _masked_case(background) -> dict:
    """NaN, infinities and masked pixels inside apertures: a star's centre pierced, half of another star masked, a masked block that holds
    a whole small aperture."""
    f = field()
    frame, mask = f["frame"].copy(), np.zeros(SHAPE, bool)
    (r0, c0), (r1, c1), (r2, c2) = np.rint(f["truth"][:3]).astype(int)
    frame[r0, c0] = np.nan
    frame[r0 + 1, c0 - 2], frame[r0 - 3, c0 + 1] = np.inf, -np.inf
    mask[r1 - 8:r1 + 9, c1:c1 + 9] = True
    mask[r2 - 3:r2 + 4, c2 - 3:c2 + 4] = True
    return _case(frame, f["truth"], (1.5, 3.0, 6.0), 5, background, mask)


def _unusable_case(background, how) -> dict:
    frame = field()["frame"].copy()
    mask = None
    if how == "nan":
        frame[:] = np.nan
    else:
        mask = np.ones(SHAPE, bool)
    return _case(frame, [(30.2, 40.7), (0.0, 0.0), (-30.0, -30.0)], (2.0, 4.0), 5, background, mask)


ROW_COUNTS = (0, 1, 3, 4, 5)  # 0, 1, WALK_WAVES - 1, WALK_WAVES, WALK_WAVES + 1 (check_row_counts asserts that they are)

CASES = {
    "field, mesh": lambda: _field_case((2.0, 4.0, 8.0)),
    "field, none": lambda: _field_case((2.0, 4.0, 8.0), background="none"),
    "field, box 16": lambda: _field_case((2.5, 5.0), box=16),
    "masked, mesh": lambda: _masked_case("mesh"),
    "masked, none": lambda: _masked_case("none"),
    "one radius, s = 1": lambda: _field_case((3.0,), 1),
    "eight radii, s = 8": lambda: _field_case((0.05, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 12.0), 8, count=12),  # 0.05: below one sub-sample
    "below one sub-sample, s = 5": lambda: _field_case((0.05, 0.11, 0.3), 5, "none"),
    "s = 1": lambda: _field_case((1.0, 1.5, 4.0), 1, "none"),
    "s = 8": lambda: _field_case((2.0, 4.0, 8.0), 8, count=10),
    "R = 64": lambda: _case(field()["frame"], [(48.2, 47.7), (0.0, 0.0), (95.5, 10.5)], (16.0, 64.0), 2),
    "unusable, mesh": lambda: _unusable_case("mesh", "nan"),
    "masked out, mesh": lambda: _unusable_case("mesh", "mask"),
    "unusable, none": lambda: _unusable_case("none", "nan"),
    **{f"{k} rows": functools.partial(_field_case, (2.0, 4.0, 8.0), count=k) for k in ROW_COUNTS},
}


@functools.cache
def case(name: str) -> dict:
    return sc._freeze(CASES[name]())


@functools.lru_cache(maxsize=None)
def _reference(name: str, mesh_bytes: bytes | None) -> dict:
    c = case(name)
    level_f = None if mesh_bytes is None else np.frombuffer(mesh_bytes).reshape(-(-c["frame"].shape[0] // c["box"]), -(-c["frame"].shape[1] // c["box"]))
    return sc._freeze(ref_photometry(c["frame"], c["mask"], c["box"], level_f, c["positions"], c["radii"], c["subpix"], c["background"]))


def reference(name: str, level_f) -> dict:
    """The restatement's answer for the case on the filtered mesh `level_f` (None: no valid node), computed once per case and mesh."""
    return _reference(name, None if level_f is None or case(name)["background"] == "none" else np.ascontiguousarray(level_f).tobytes())


# ------------------------------------------------------------------------------------------------------------------ the emulator
@functools.cache
def emulator():
    """tests/emu/libemu_photometry.so: the kernel's driver on the CPU, compiled here when missing or older than its sources."""
    lib = emulib.library("emu_photometry")
    vp, i, n = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.emuph_info.argtypes = [vp]
    lib.emuph_photometry.argtypes = [vp, vp, i, i, i, vp, i, n, vp, i, vp, i, i, vp]
    return lib


def emulator_info(m: int = 1) -> tuple[int, int, int]:
    """WALK_WAVES, the workgroups of S6 the last photometry ran, s6_lds_bytes(m)."""
    info = (ctypes.c_long * 4)(0, 0, 0, m)
    emulator().emuph_info(info)
    return tuple(info)[:3]


class EmuError(RuntimeError):
    """What the emulated finder raises where the library returns an error code."""

    def __init__(self, code: int, message: str) -> None:
        super().__init__(message)
        self.code = code


class EmuFinder(shc.EmuFinder):
    """shape_cases.EmuFinder with the fused route's ``background_device`` / ``detect_device`` (S1 on the emulator, S1b by the host filter
    whose bits it has) and ``photometry``: regularizepsf_amd.stars._Finder's interface on the emulator."""

    def __init__(self, shape, box, device=0) -> None:
        super().__init__(shape, box, device)
        self._filtered, self._have_mesh, self._launched = None, False, 0

    def background(self, frame, mask):
        self._have_mesh = False  # the host route: S1b's mesh is not the frame's any more
        return super().background(frame, mask)

    def background_device(self, frame, mask) -> None:
        level, rms = self.background(np.asarray(frame), mask)
        self._filtered, self._have_mesh = stars.filter_mesh(level, rms), True

    def detect_device(self, threshold, min_area, max_area):
        if not self._have_mesh:
            raise EmuError(-6, "detect_device before background_device")
        if self._filtered is None:
            return np.zeros((0, 4))
        rows = self.detect(self._filtered[0], threshold * self._filtered[2], min_area, max_area)
        self._have_mesh = True  # (detect_device leaves S1b's mesh where it is)
        return rows

    def detect(self, level, threshold_abs, min_area, max_area):
        self._have_mesh = False
        return super().detect(level, threshold_abs, min_area, max_area)

    def photometry(self, positions, radii, subpix=5, use_mesh=True):
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        radii = np.ascontiguousarray(radii, np.float64).ravel()
        out = np.empty((len(positions), columns(max(len(radii), 0))))
        level = None if self._filtered is None else np.ascontiguousarray(self._filtered[0])
        frame, mask = (self._frame, self._mask) if self._frame is not None else (np.zeros(self.shape, np.float32), None)
        code = emulator().emuph_photometry(frame.ctypes.data, None if mask is None else mask.ctypes.data, *self.shape, self.box,
                                           None if level is None else level.ctypes.data, int(level is None), len(positions),
                                           positions.ctypes.data, len(radii), radii.ctypes.data, int(subpix), int(bool(use_mesh)),
                                           out.ctypes.data)
        if code != 0:
            raise EmuError(-1, "bad argument")
        if not self._have_mesh:  # (the library checks its arguments first, then its state)
            raise EmuError(-6, "photometry before background_device")
        self._launched = emulator_info()[1]
        return out

    def photometry_ms(self) -> float:
        """In the place of the device time: the workgroups of S6 that ran - 0.0 exactly when nothing was launched."""
        return float(self._launched)


# ------------------------------------------------------------------------------------------------------------------ the checks
def run(make_finder, c: dict, times: list | None = None):
    """The product's per-frame route on a finder: (the filtered mesh or None, S6's rows)."""
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        level, rms = finder.background(c["frame"], c["mask"])  # the raw mesh of the finder under test (see THE MESH)
        filtered = stars.filter_mesh(level, rms)
        finder.background_device(c["frame"], c["mask"])
        rows = finder.photometry(c["positions"], c["radii"], c["subpix"], c["background"] == "mesh")
        if times is not None:
            times.append(finder.photometry_ms())
        return (None if filtered is None else filtered[0]), rows
    finally:
        finder.close()


def compare(got: np.ndarray, ref: dict, m: int, what: str) -> float:
    """Counts, peak and positions exact, sums within THE BOUND; returns the worst error / bound."""
    want, bounds = ref["rows"], ref["bounds"]
    assert got.dtype == np.float64 and got.shape == want.shape, f"{what}: {got.shape}, the restatement has {want.shape}"
    if len(want) == 0:
        return 0.0
    assert got[:, :2].tobytes() == want[:, :2].tobytes(), f"{what}: row, col are not the positions given"
    assert np.array_equal(got[:, 2 + m:2 + 3 * m], want[:, 2 + m:2 + 3 * m]), f"{what}: N_use or N_all differ"
    assert np.array_equal(got[:, -3:], want[:, -3:], equal_nan=True), f"{what}: the peak or its pixel differ"
    sums = np.concatenate([np.arange(2, 2 + m), np.arange(2 + 3 * m, 2 + 3 * m + 6)])
    assert np.array_equal(np.isnan(got[:, sums]), np.isnan(want[:, sums])), f"{what}: NaN in other places"
    err = np.nan_to_num(np.abs(got[:, sums] - want[:, sums]))
    worst = float(np.max(err[bounds > 0] / bounds[bounds > 0], initial=0.0))
    print(f"{what}: {len(want)} positions, {m} radii, N_all <= {int(want[:, 2 + 2 * m:2 + 3 * m].max())}, worst error {err.max():.2e}, worst "
          f"error / bound {worst:.2e}")
    assert np.all(err <= bounds), what
    return worst


def check_case(make_finder, name: str) -> float:
    c = case(name)
    level_f, rows = run(make_finder, c)
    return compare(rows, reference(name, level_f), len(c["radii"]), name)


def check_hard_positions(make_finder) -> None:
    """What the hard positions of the field cases are there for, said from the restatement and held by the finder."""
    for name in ("field, mesh", "field, none"):
        c = case(name)
        m, s2 = len(c["radii"]), c["subpix"] ** 2
        level_f, got = run(make_finder, c)
        compare(got, reference(name, level_f), m, name)
        flux, n_use, n_all = got[:, 2:2 + m], got[:, 2 + m:2 + 2 * m], got[:, 2 + 2 * m:2 + 3 * m]
        at = {tuple(p): i for i, p in enumerate(c["positions"].tolist())}
        # every aperture has its whole area, wherever it lies: N_all / s^2 is pi R^2 within the lattice's error, 4 (R + 1) pixels of rim
        assert np.all(np.abs(n_all / s2 - np.pi * c["radii"] ** 2) <= 4 * (c["radii"] + 1))
        assert np.all(n_all[:, 1:] > n_all[:, :-1]) and np.all(n_use <= n_all)
        for off in ((-30.0, -30.0), (200.5, 48.0), (48.0, -70.25)):  # wholly off the frame
            i = at[off]
            assert np.all(n_use[i] == 0) and np.all(n_all[i] > 0) and np.all(flux[i] == 0.0) and np.all(got[i, 2 + 3 * m:-3] == 0.0)
            assert np.isnan(got[i, -3]) and got[i, -2] == got[i, -1] == -1.0
        for partly in ((0.0, 0.0), (-1.3, 40.2), (96.7, 50.1), (40.4, -2.2), (33.3, 97.0), (95.0, 95.0)):
            i = at[partly]
            assert 0 < n_use[i, -1] < n_all[i, -1], partly
        quarter = n_use[at[(0.0, 0.0)]] / n_all[at[(0.0, 0.0)]]
        assert np.all(quarter > 0.25) and np.all(quarter < 0.5)  # a quarter of the disc and the half pixels along the two edges
        inner = at[(60.2, 60.4)]  # given twice, and a third aperture over both: every row is its own
        twice = [i for i, p in enumerate(c["positions"].tolist()) if tuple(p) == (60.2, 60.4)]
        assert len(twice) == 2 and got[twice[0]].tobytes() == got[twice[1]].tobytes() and inner in twice
        assert np.all(n_use[at[(20.5, 30.5)]] == n_all[at[(20.5, 30.5)]])  # on a pixel corner, inside the frame


def check_exact(make_finder) -> None:
    """The exact cases: lattice counts on a pixel centre, dyadic weights on a constant frame, and a frame times two."""
    frame = np.full(SHAPE, 3.0, np.float32)
    c = _case(frame, [(40.0, 50.0), (0.0, 0.0)], (1.0, 1.5), 1, "none")
    _, got = run(make_finder, c)
    assert got[:, 6:8].tolist() == [[5.0, 9.0], [5.0, 9.0]] and got[:, 4:6].tolist() == [[5.0, 9.0], [3.0, 4.0]]  # N_all; N_use
    assert got[:, 2:4].tolist() == [[15.0, 27.0], [9.0, 12.0]]
    c = _case(frame, np.concatenate([field()["truth"], hard_positions()]), (0.3, 1.0, 2.7, 5.0, 9.5), 4, "none")
    _, got = run(make_finder, c)
    m = 5
    assert got[:, 2:2 + m].tobytes() == (3.0 * got[:, 2 + m:2 + 2 * m] / 16.0).tobytes()  # the weights are dyadic: no rounding anywhere
    assert got[:, 2 + 3 * m].tobytes() == got[:, 2 + m - 1].tobytes()  # sum w |d| = sum w d
    seen = got[:, 2 + 2 * m - 1] > 0
    assert np.all(got[seen, -3] == 3.0) and np.all(np.isnan(got[~seen, -3]))
    for name in ("field, mesh", "field, none", "masked, mesh"):  # 2 x frame: every power of two passes through S1, S1b and S6 exactly
        c = case(name)
        _, one = run(make_finder, c)
        _, two = run(make_finder, {**c, "frame": 2.0 * c["frame"]})
        m = len(c["radii"])
        scaled = np.concatenate([np.arange(2, 2 + m), np.arange(2 + 3 * m, 2 + 3 * m + 7)])  # the fluxes, the six sums, the peak
        same = np.setdiff1d(np.arange(one.shape[1]), scaled)
        assert two[:, scaled].tobytes() == (2.0 * one[:, scaled]).tobytes(), name
        assert two[:, same].tobytes() == one[:, same].tobytes(), name


def check_unusable(make_finder) -> None:
    """No valid mesh node under "mesh": NaN fluxes, sums and peak, the counts kept.  Under "none" zeros, as off the frame."""
    for name in ("unusable, mesh", "masked out, mesh", "unusable, none"):
        c = case(name)
        m = len(c["radii"])
        level_f, got = run(make_finder, c)
        assert level_f is None
        compare(got, reference(name, None), m, name)
        values = np.concatenate([got[:, 2:2 + m], got[:, 2 + 3 * m:-2]], axis=1)
        assert np.all(got[:, 2 + m:2 + 2 * m] == 0) and np.all(got[:, 2 + 2 * m:2 + 3 * m] > 0)
        if c["background"] == "mesh":
            assert np.isnan(values).all()
        else:
            assert np.all(values[:, :-1] == 0.0) and np.isnan(values[:, -1]).all()
        assert np.all(got[:, -2:] == -1.0)
        cat = stars.photometry_from_sums(got, c["radii"], c["subpix"])
        assert np.all(cat["area"] == 0.0) and np.all(cat["coverage"] == 0.0) and np.isnan(cat["half_light_radius"]).all()


def check_row_counts(make_finder, walk_waves: int) -> None:
    """0, 1, WALK_WAVES - 1, WALK_WAVES and WALK_WAVES + 1 positions; 0 launches nothing (the finder's timer stays 0)."""
    assert ROW_COUNTS == (0, 1, walk_waves - 1, walk_waves, walk_waves + 1)
    whole = None
    for k in reversed(ROW_COUNTS):
        c, times = case(f"{k} rows"), []
        level_f, got = run(make_finder, c, times)
        assert got.shape == (k, columns(3)) and got.dtype == np.float64
        compare(got, reference(f"{k} rows", level_f), 3, f"{k} rows")
        whole = got if whole is None else whole
        assert got.tobytes() == whole[:k].tobytes()  # a row does not depend on its neighbours in the workgroup
        assert (times[0] == 0.0) == (k == 0), (k, times)


def check_reproducible(make_finder, name: str) -> None:
    """Repeats are bit-equal: on a fresh finder, by a second call on the same frame, and with another call in between."""
    c = case(name)
    _, rows = run(make_finder, c)
    assert run(make_finder, c)[1].tobytes() == rows.tobytes()
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        finder.background_device(c["frame"], c["mask"])
        args = (c["positions"], c["radii"], c["subpix"], c["background"] == "mesh")
        one = finder.photometry(*args)
        other = finder.photometry(c["positions"][::-1], c["radii"][:1], 3, False)  # other rows, radii and sampling in the same buffers
        two = finder.photometry(*args)
        assert one.tobytes() == two.tobytes() == rows.tobytes() and other.shape == (len(c["positions"]), columns(1))
    finally:
        finder.close()


def check_isolation(make_finder) -> None:
    """detect -> photometry -> measure gives the bits of detect -> measure, and the detect's rows do not depend on a photometry before."""
    c = case("field, mesh")
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        finder.background_device(c["frame"], c["mask"])
        rows = finder.detect_device(3.0, 5, None)
        shapes = finder.measure()
        assert len(rows) == 8 and shapes[:, :4].tobytes() == rows.tobytes()
        phot = finder.photometry(rows[:, :2], c["radii"], c["subpix"], True)
        assert finder.measure().tobytes() == shapes.tobytes()  # S5 reads the frame, the mesh, the labels and the rows: all as they were
        finder.photometry(c["positions"], (1.0, 64.0), 8, False)
        assert finder.measure().tobytes() == shapes.tobytes()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes()
        assert finder.photometry(rows[:, :2], c["radii"], c["subpix"], True).tobytes() == phot.tobytes()
        finder.background_device(c["frame"], c["mask"])  # photometry first, the detect after it
        assert finder.photometry(rows[:, :2], c["radii"], c["subpix"], True).tobytes() == phot.tobytes()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes() and finder.measure().tobytes() == shapes.tobytes()
    finally:
        finder.close()


def check_errors(make_finder, error: type) -> None:
    """RPSF_E_STATE (-6) before a background_device of a frame and after the host route's detect; RPSF_E_BADARG (-1) for bad radii, subpix,
    m and positions, whatever the state."""
    import pytest

    c = case("field, mesh")
    good = (c["positions"], c["radii"], 5, True)
    bad = [(c["positions"], (), 5, True), (c["positions"], np.arange(1.0, 10.0), 5, True), (c["positions"], (2.0, 2.0), 5, True),
           (c["positions"], (3.0, 2.0), 5, True), (c["positions"], (0.0, 2.0), 5, True), (c["positions"], (-1.0,), 5, True),
           (c["positions"], (2.0, 64.5), 5, True), (c["positions"], (np.nan,), 5, True), (c["positions"], (2.0,), 0, True),
           (c["positions"], (2.0,), 9, True), ([(np.nan, 1.0)], (2.0,), 5, True), ([(1.0, np.inf)], (2.0,), 5, True),
           ([(2.0 ** 20, 1.0)], (2.0,), 5, True), ([(1.0, 1.0), (1.0, -2.0 ** 20)], (2.0,), 5, False)]
    finder = make_finder(c["frame"].shape, c["box"])
    try:
        def refused(args, code):
            with pytest.raises(error) as caught:
                finder.photometry(*args)
            assert caught.value.code == code, (args[1:], caught.value.code)

        refused(good, -6)
        for args in bad:
            refused(args, -1)
        level, rms = finder.background(c["frame"], c["mask"])  # the host route: no S1b mesh on the device
        refused(good, -6)
        finder.background_device(c["frame"], c["mask"])
        for args in bad:
            refused(args, -1)
        rows = finder.photometry(*good)
        assert finder.photometry([(2.0 ** 20 - 1, 1.0 - 2.0 ** 20)], (64.0,), 8, True).shape == (1, columns(1))  # the largest admitted
        level_f, _, global_rms = stars.filter_mesh(level, rms)
        finder.detect(level_f, 3.0 * global_rms, 5, None)  # the host route's detect replaces the mesh on the device
        refused(good, -6)
        finder.background_device(c["frame"], c["mask"])
        assert finder.photometry(*good).tobytes() == rows.tobytes()
    finally:
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ the truth
# Noise-free Gaussians (amplitude 1000) of known sigma at fractional positions, measured on the restatement alone with background="none",
# at positions TRUTH_OFFSET away from the true centres.  On the committed positions the restatement's worst errors are MEASURED_*.  The
# half-light radius is interpolated linearly between the chosen radii, and the curve of growth 1 - exp(-R^2 / 2 sigma^2) is not linear: that
# discretisation, not rounding, is what the figures show; likewise the centroid's offset is that of the light inside R = 8, whose window is
# centred on the given position and not on the star.  The asserted bounds are the measured figures times TRUTH_MARGIN = 2: other
# fractional positions move a star against the pixel lattice and the radii against sigma by amounts of the same kind, not larger ones.
TRUTH_SIGMAS = (1.2, 1.7, 2.3)
TRUTH_RADII = (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 8.0)
TRUTH_OFFSET = np.array([(0.3, -0.2), (-0.45, 0.1), (0.0, 0.5)])
MEASURED_HALF_LIGHT = 0.0412  # relative to sigma sqrt(2 ln 2): sigma 1.2 between R = 1 and 1.5 (4.12 %, 4.05 % for 1.7, 1.79 % for 2.3)
MEASURED_CENTROID = 0.0079  # pixels: sigma 2.3, whose R = 8 window cuts 0.2 % of the light off-centre (1.1e-4 and 8e-9 for the others)
TRUTH_MARGIN = 2.0


def truth_case() -> dict:
    centres = np.array([(20.3, 22.6), (24.75, 70.2), (66.5, 40.0)])
    rows, cols = np.mgrid[0:SHAPE[0], 0:SHAPE[1]].astype(np.float64)
    frame = np.zeros(SHAPE)
    for (r, c), sigma in zip(centres, TRUTH_SIGMAS):
        frame += 1000.0 * np.exp(-0.5 * ((rows - r) ** 2 + (cols - c) ** 2) / sigma ** 2)
    return {"frame": frame.astype(np.float32), "centres": centres, "positions": centres - TRUTH_OFFSET}


def check_truth() -> tuple[float, float]:
    """The definition itself on the restatement alone; returns the worst half-light error (relative) and centroid error (pixels)."""
    t = truth_case()
    ref = ref_photometry(t["frame"], None, BOX, None, t["positions"], TRUTH_RADII, 5, "none")
    cat = stars.photometry_from_sums(ref["rows"], TRUTH_RADII, 5)
    want = np.array(TRUTH_SIGMAS) * np.sqrt(2 * np.log(2))
    half = np.abs(cat["half_light_radius"] - want) / want
    centroid = np.hypot(cat["drow"] - TRUTH_OFFSET[:, 0], cat["dcol"] - TRUTH_OFFSET[:, 1])
    print(f"truth: half-light radii {cat['half_light_radius']} against {want}: worst relative error {half.max():.4f} (measured "
          f"{MEASURED_HALF_LIGHT}); centroid offsets off by {centroid} pixels: worst {centroid.max():.4f} (measured {MEASURED_CENTROID})")
    assert half.max() <= TRUTH_MARGIN * MEASURED_HALF_LIGHT and centroid.max() <= TRUTH_MARGIN * MEASURED_CENTROID
    assert np.all(np.abs(np.sqrt(cat["rr"]) - TRUTH_SIGMAS) < 0.1 * np.array(TRUTH_SIGMAS)) and np.all(cat["elongation"] < 1.05)
    return float(half.max()), float(centroid.max())
