"""Second moments and shape per detection of the star finder (kernel S5) restated in float64 NumPy, the cases, the CPU
emulator of the kernel, and the checks the emulator tests (tests/test_shapes_host.py) and the GPU tests (tests/test_gpu_shapes.py) share.

As for the detector there is no outside implementation: the reference is the restatement below, written from the definition with array
operations (np.bincount over the object map), computed once per case.  For every case it first asserts that its rows are
star_cases.ref_detect's resp. deblend_cases.ref_deblend's bit for bit, so that it restates the same objects.  A check takes
`make_finder(shape, box)`: regularizepsf_amd.stars._Finder on the GPU, EmuFinder here.

THE BOUND.  The kernel and the restatement add the same terms d (dr dr) in different orders and divide by their own sum of d.  With
u = 2^-53, n = area, S = sum |d|, F = sum d and rho^2 the largest squared distance from the centroid inside the bounding box (so every
term is at most |d| rho^2 in magnitude and the moment itself at most rho^2 S / F):
  * two sums of n terms in different orders differ by at most 2 (n - 1) u S rho^2 in the numerator:      2 n u rho^2 S / F  after / F
  * the two F differ by at most 2 (n - 1) u S (compare_rows' bound), a relative 2 n u S / F of the moment:  2 n u (S / F) rho^2 S / F
  * the two centroids differ by D <= 8 n u (S / F) max(H, W) (compare_rows); sum d (dr + D)^2 = sum d dr^2 + 2 D sum d dr + D^2 F, and
    sum d dr is zero but for rounding: second order, as are the three roundings of each term
With S / F <= RATIO_MAX = 2 (a precondition of every case, asserted from the restatement) that is at most 6 n u rho^2 S / F; the bound is
    8 n u rho^2 S / F,
the form compare_rows uses for positions with rho^2 in the place of max(H, W).  For abs_flux nothing is divided and every term is |d|:
rho^2 = 1 and the bound, on abs_flux / F, is 8 n u S / F - that is 8 n u S on abs_flux itself, compare_rows' bound for the flux.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np

from tests import emulib
from regularizepsf_amd import stars
from tests import deblend_cases as dc
from tests import star_cases as sc

ROOT = sc.ROOT
COLUMNS = ("row", "col", "flux", "area", "peak", "peak_row", "peak_col", "row_min", "row_max", "col_min", "col_max", "abs_flux", "rr", "cc",
           "rc")
FIELDS = (*COLUMNS, "a", "b", "theta", "elongation")
COL = {name: j for j, name in enumerate(COLUMNS)}
RATIO_MAX = 2.0  # sum |d| / sum d of every kept row of every case (see THE BOUND)
LAMBDA_GAP = 1e-9  # the derived fields are compared with the restatement's only where lambda- is not within this, relative to lambda+, of zero
DEFAULTS = {"threshold": 3.0, "min_area": 5, "max_area": None, "deblend": False, "contrast": 0.005, "prominence": 1.0}


# ------------------------------------------------------------------------------------------------------------------ the restatement
def ref_ellipse(rr, cc, rc):
    """(lambda+, lambda-, a, b, theta, elongation) from the definition."""
    with np.errstate(invalid="ignore", divide="ignore"):
        mean, half = (rr + cc) / 2, np.sqrt(((rr - cc) / 2) ** 2 + rc ** 2)
        a, b = np.sqrt(mean + half), np.sqrt(mean - half)
        return mean + half, mean - half, a, b, 0.5 * np.arctan2(2 * rc, cc - rr), a / b


def _object_keys(f, detected, d, labels, pix, T, min_area, contrast, prominence) -> np.ndarray:
    """D1 - D4 (deblend_cases.ref_deblend's steps): per detected pixel the root of its unsplit component or the peak of its object."""
    shape = f.shape
    peak = dc.ref_basins(f, detected).ravel()
    rr, cc = np.divmod(pix, shape[1])
    dv, fv = d.ravel()[pix], f.ravel()
    comps, comp_of = np.unique(labels[pix], return_inverse=True)
    basins, basin_of = np.unique(peak[pix], return_inverse=True)
    bcomp = np.searchsorted(comps, labels[basins])
    area, flux, F = np.bincount(basin_of), np.bincount(basin_of, dv), np.bincount(comp_of, dv)
    saddle, slot = np.full(len(basins), -np.inf), np.full(f.size, -1)
    slot[pix] = basin_of
    slot = slot.reshape(shape)
    for dr, dc_ in dc.HALF:
        both = detected & dc._shifted(detected, dr, dc_, False)
        fq, sq = dc._shifted(f, dr, dc_, 0.0), dc._shifted(slot, dr, dc_, -1)
        across = both & (slot != sq)
        low = np.minimum(f, fq)[across]
        np.maximum.at(saddle, slot[across], low)
        np.maximum.at(saddle, sq[across], low)
    significant = (area >= min_area) & (flux >= contrast * F[bcomp]) & (fv[basins] - saddle >= prominence * T)
    count = np.bincount(bcomp, significant, minlength=len(comps))
    owner, is_split = peak[pix].copy(), count[comp_of] >= 2
    for k in np.flatnonzero(count >= 2):
        tops = basins[(bcomp == k) & significant]
        stray = np.flatnonzero((comp_of == k) & ~significant[basin_of])
        tr, tc = np.divmod(tops, shape[1])
        dist = (rr[stray, None] - tr[None, :]) ** 2 + (cc[stray, None] - tc[None, :]) ** 2
        owner[stray] = tops[np.argmin(dist, axis=1)]
    return np.where(is_split, owner, labels[pix])


def ref_shapes(frame, mask, box, threshold=3.0, min_area=5, max_area=None, deblend=False, contrast=0.005, prominence=1.0) -> dict:
    """The definition.  rows: (k, 4) of (row, col, flux, area) in raster order of each object's first pixel; map: per pixel the index of
    its kept row, -1 elsewhere; columns: (k, len(COLUMNS)); rho2: per row the largest squared distance from the centroid inside the box."""
    frame = np.asarray(frame, np.float32).astype(np.float64)
    ok = np.isfinite(frame) & (~mask if mask is not None else True)
    out = {"rows": np.zeros((0, 4)), "map": np.full(frame.shape, -1), "columns": np.zeros((0, len(COLUMNS))), "rho2": np.zeros(0)}
    level, rms, _ = sc.ref_mesh(frame, mask, box)
    filtered = sc.ref_filter_mesh(level, rms)
    if filtered is None:
        return out
    level_f, _, global_rms = filtered
    T = threshold * global_rms
    with np.errstate(invalid="ignore"):
        d = np.where(ok, frame - sc.ref_surface(level_f, frame.shape, box), 0.0)
    f = sc.ref_filter(d)
    detected = (f > T) & ok
    if not detected.any():
        return out
    labels, pix = sc.ref_labels(detected).ravel(), np.flatnonzero(detected)
    key = _object_keys(f, detected, d, labels, pix, T, min_area, contrast, prominence) if deblend else labels[pix]
    _, obj = np.unique(key, return_inverse=True)
    first = np.full(obj.max() + 1, frame.size)
    np.minimum.at(first, obj, pix)
    rank = np.empty(len(first), int)
    rank[np.argsort(first)] = np.arange(len(first))
    obj = rank[obj]  # the objects in raster order of their first pixels
    r, c = np.divmod(pix, frame.shape[1])
    dv = d.ravel()[pix]
    area, flux = np.bincount(obj), np.bincount(obj, dv)
    keep = (area >= min_area) & (flux > 0)
    if max_area is not None:
        keep &= area <= max_area
    with np.errstate(invalid="ignore", divide="ignore"):
        rows = np.stack([np.bincount(obj, dv * r) / flux, np.bincount(obj, dv * c) / flux, flux, area.astype(np.float64)], axis=-1)[keep]
    k = len(rows)
    index = np.where(keep, np.cumsum(keep) - 1, -1)[obj]  # per detected pixel: its kept row, or -1
    objmap = np.full(frame.size, -1)
    objmap[pix] = index
    kept = index >= 0
    o, r, c, dv, p = index[kept], r[kept], c[kept], dv[kept], pix[kept]
    dr, dc_ = r - rows[o, 0], c - rows[o, 1]
    columns = np.empty((k, len(COLUMNS)))
    columns[:, :4] = rows
    columns[:, COL["abs_flux"]] = np.bincount(o, np.abs(dv), minlength=k)
    columns[:, COL["rr"]] = np.bincount(o, dv * (dr * dr), minlength=k) / rows[:, 2]
    columns[:, COL["cc"]] = np.bincount(o, dv * (dc_ * dc_), minlength=k) / rows[:, 2]
    columns[:, COL["rc"]] = np.bincount(o, dv * (dr * dc_), minlength=k) / rows[:, 2]
    rho2 = np.empty(k)
    for i in range(k):
        mine = o == i
        top = np.argmax(dv[mine])  # the first in raster order among equals: p ascends
        box_ = (r[mine].min(), r[mine].max(), c[mine].min(), c[mine].max())
        columns[i, COL["peak"]], columns[i, COL["peak_row"]], columns[i, COL["peak_col"]] = dv[mine][top], r[mine][top], c[mine][top]
        columns[i, COL["row_min"]:COL["col_max"] + 1] = box_
        rho2[i] = max((rb - rows[i, 0]) ** 2 + (cb - rows[i, 1]) ** 2 for rb in box_[:2] for cb in box_[2:])
    out.update(rows=rows, map=objmap.reshape(frame.shape), columns=columns, rho2=rho2, d=d)
    return out


# ------------------------------------------------------------------------------------------------------------------ the frames
def _plain(case: dict, **options) -> dict:
    return {"frame": case["frame"], "mask": case["mask"], "box": case["box"], "options": {**DEFAULTS, **options}}


def _frame(shape, box, add, seed, noise=0.3, **options) -> dict:
    """star_cases.star_frame's background and noise with `add(rows, cols)` on top, rounded to float32."""
    rows, cols = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    frame = 10.0 + 0.004 * rows - 0.003 * cols + np.random.default_rng([seed, 53]).normal(0.0, noise, shape) + add(rows, cols)
    return {"frame": frame.astype(np.float32).astype(np.float64), "mask": None, "box": box, "options": {**DEFAULTS, **options}}


# Single hot pixels of 5 above the background: the 3 x 3 filter leaves 5 / 4 at the pixel and 5 / 8 beside it, T is about 0.9.  The first
# four lie at power-of-two coordinates: there d * row and d * col are exact, the centroid is the pixel bit for bit, and the moments are 0
# exactly.  The others are single pixels whose centroid may be off by a rounding.
EXACT_PIXELS = ((16, 32), (32, 8), (8, 64), (32, 64))
OTHER_PIXELS = ((21, 23), (45, 51), (50, 13))


def _single_pixels(rows, cols):
    out = np.zeros(rows.shape)
    for r, c in EXACT_PIXELS + OTHER_PIXELS:
        out[r, c] = 5.0
    return out


def _gauss(rows, cols, r, c, amp, sigma):
    return amp * np.exp(-0.5 * ((rows - r) ** 2 + (cols - c) ** 2) / sigma ** 2)


def _arc_and_star(rows, cols):
    """An arc of radius 14 around (32.3, 36.4), open over 80 degrees, and a star at its centre: the star's pixels lie inside the arc's
    bounding box and are not connected to it."""
    rho, phi = np.hypot(rows - 32.3, cols - 36.4), np.degrees(np.arctan2(rows - 32.3, cols - 36.4))
    arc = 200.0 * np.exp(-0.5 * ((rho - 14.0) / 1.2) ** 2) * (np.abs(phi) > 40.0)
    return arc + _gauss(rows, cols, 32.3, 36.4, 300.0, 1.3)


def _streak(rows, cols, r0, c0, length, amp, sigma):
    """A diagonal streak from (r0, c0) to (r0 + length, c0 + length)."""
    along = np.clip(((rows - r0) + (cols - c0)) / 2.0, 0.0, length)
    return amp * np.exp(-0.5 * ((rows - r0 - along) ** 2 + (cols - c0 - along) ** 2) / sigma ** 2)


def _parallel_streaks(rows, cols):
    """Two diagonal streaks 12.7 pixels apart: each lies inside the other's bounding box, neither touches the other."""
    return _streak(rows, cols, 12.2, 12.4, 30.0, 150.0, 1.1) + _streak(rows, cols, 21.3, 3.1, 30.0, 120.0, 1.1)


ELLIPSES = {"sigma": (2.4, 1.2), "angles": (-75.0, -50.0, -25.0, 0.0, 25.0, 50.0, 75.0, 90.0), "amp": 300.0}
# The restatement alone, on the committed seed: the worst |theta - angle| (modulo 180 degrees) is MEASURED_THETA degrees and the smallest
# a / b MEASURED_ELONGATION (the footprint truncates the wings, a and b come out low).  THETA_BOUND carries a margin of 2 for other seeds.
MEASURED_THETA = 0.114
MEASURED_ELONGATION = 1.98
THETA_BOUND = 2 * MEASURED_THETA
ELONGATION_MIN = 1.3


def ellipse_truth() -> tuple[np.ndarray, np.ndarray]:
    """Centres (8, 2) and angles (degrees; the major axis from the column axis towards the row axis)."""
    rng = np.random.default_rng([8, 59])
    centre = np.array([(25.0 + 50.0 * (i // 4), 20.0 + 40.0 * (i % 4)) for i in range(8)]) + rng.uniform(-0.5, 0.5, (8, 2))
    return centre, np.array(ELLIPSES["angles"])


def _ellipses(rows, cols):
    centre, angles = ellipse_truth()
    major, minor = ELLIPSES["sigma"]
    out = np.zeros(rows.shape)
    for (r, c), angle in zip(centre, np.radians(angles)):
        u = (rows - r) * np.sin(angle) + (cols - c) * np.cos(angle)
        v = (rows - r) * np.cos(angle) - (cols - c) * np.sin(angle)
        out += ELLIPSES["amp"] * np.exp(-0.5 * ((u / major) ** 2 + (v / minor) ** 2))
    return out


def _stars(count: int) -> dict:
    """`count` stars in 64 x 96: the number of kept rows around the rows a workgroup of S5 takes."""
    rng = np.random.default_rng([count, 61])
    truth = sc.scattered((64, 96), count, rng)
    return {"frame": sc.star_frame((64, 96), truth, rng), "mask": None, "box": 32, "options": dict(DEFAULTS)}


ROW_COUNTS = {"1 row": 1, "4 rows": 4, "5 rows": 5}  # 1, WALK_WAVES and WALK_WAVES + 1 (check_row_counts asserts that they are)

CASES = {
    **{name: functools.partial(lambda name: _plain(sc.CASES[name]()), name) for name in sc.CASES},
    "background": lambda: _plain(sc.background_case()),
    "one component": lambda: _plain(dc.one_component_case(), **dc.ONE_COMPONENT),  # 9 100 pixels in a box 70 wide: the lane stride wraps rows
    "one component, split": lambda: _plain(dc.one_component_case(), deblend=True, **dc.ONE_COMPONENT),
    "single pixels": lambda: _frame((64, 80), 32, _single_pixels, 1, min_area=1),
    "arc and star": lambda: _frame((64, 72), 32, _arc_and_star, 2),
    "parallel streaks": lambda: _frame((64, 64), 32, _parallel_streaks, 3),
    **{name: functools.partial(_stars, count) for name, count in ROW_COUNTS.items()},
    **{name: functools.partial(lambda name: _plain(dc.pair_case(name), deblend=True), name) for name in dc.PAIRS},
    **{name: functools.partial(lambda name: _plain(dc.special_case(name), deblend=True), name) for name in dc.SPECIAL},
    "ellipses": lambda: _frame((100, 160), 32, _ellipses, 4),
}


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """The case with the restatement's answer (shared; do not modify): frame, mask, box, options, ref."""
    case = CASES[name]()
    o = case["options"]
    ref = ref_shapes(case["frame"], case["mask"], case["box"], **o)
    if o["deblend"]:
        same = dc.ref_deblend(case["frame"], case["mask"], case["box"], o["threshold"], o["min_area"], o["max_area"], o["contrast"], o["prominence"])
        dc.admitted(name, same)
    else:
        same = sc.ref_detect(case["frame"], case["mask"], case["box"], o["threshold"], o["min_area"], o["max_area"])
        assert same["gap_clip"] >= sc.GAP_CLIP and same["gap_threshold"] >= sc.GAP_THRESHOLD, (name, same["gap_clip"], same["gap_threshold"])
    assert ref["rows"].tobytes() == same["rows"].tobytes(), f"{name}: the restatement of the shapes restates other objects"
    assert np.array_equal(ref["columns"][:, COL["abs_flux"]], same["abs_flux"])
    if len(ref["rows"]):
        ratio = ref["columns"][:, COL["abs_flux"]] / ref["rows"][:, 2]
        assert ratio.max() <= RATIO_MAX, f"{name}: sum |d| / sum d = {ratio.max():.3f}"
    return sc._freeze({**case, "ref": ref})


# ------------------------------------------------------------------------------------------------------------------ the emulator
@functools.cache
def emulator():
    """tests/emu/libemu_shapes.so: the kernels' drivers on the CPU, compiled here when missing or older than its sources."""
    lib = emulib.library("emu_shapes")
    vp, i, d, n = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_long
    lib.emush_info.argtypes = [vp]
    lib.emush_measure.argtypes = [vp, vp, i, i, i, vp, d, n, n, i, d, d, vp, vp, n, vp]
    return lib


def emulator_info() -> tuple[int, int, int]:
    """WALK_WAVES, the shape columns, the workgroups of S5 the last measure ran."""
    info = (ctypes.c_long * 3)()
    emulator().emush_info(info)
    return tuple(info)


class EmuStateError(RuntimeError):
    """What the emulated finder raises where the library returns RPSF_E_BADARG."""

    code = -1


class EmuFinder(dc.EmuFinder):
    """deblend_cases.EmuFinder with ``measure``: regularizepsf_amd.stars._Finder's interface on the emulator.  The emulator runs the detect
    and S5 in one call; ``measure`` hands out what the last detect computed, under the library's rules of when that is allowed."""

    def __init__(self, shape, box, device=0) -> None:
        super().__init__(shape, box, device)
        self._shapes, self._workgroups = None, 0

    def background(self, frame, mask):
        self._shapes = None  # a new frame: the rows of the last detect are gone
        return super().background(frame, mask)

    def detect(self, level, threshold_abs, min_area, max_area):
        level = np.ascontiguousarray(level, np.float64)
        capacity = self.shape[0] * self.shape[1]
        rows, shapes, count = np.empty((capacity, 4)), np.empty((capacity, len(COLUMNS))), ctypes.c_long(0)
        on, contrast, prominence = self._deblend
        assert emulator().emush_measure(self._frame.ctypes.data, None if self._mask is None else self._mask.ctypes.data, *self.shape, self.box,
                                        level.ctypes.data, float(threshold_abs), int(min_area), -1 if max_area is None else int(max_area),
                                        int(on), contrast, prominence, rows.ctypes.data, shapes.ctypes.data, capacity, ctypes.byref(count)) == 0
        self._shapes, self._workgroups = shapes[:count.value].copy(), emulator_info()[2]
        return rows[:count.value].copy()

    def measure(self):
        if self._shapes is None:
            raise EmuStateError("measure without a detect of the frame")
        return self._shapes.copy()

    def shape_ms(self) -> float:
        """In the place of the device time: the workgroups of S5 that ran - 0.0 exactly when nothing was launched."""
        return float(self._workgroups)


# ------------------------------------------------------------------------------------------------------------------ the checks
def run(make_finder, case: dict, measure: bool = True, times: list | None = None):
    """The product's per-frame pipeline on a finder with the case's options, then ``measure``: (rows, shapes)."""
    o = case["options"]
    finder = make_finder(case["frame"].shape, case["box"])
    try:
        if o["deblend"]:
            finder.set_deblend(True, o["contrast"], o["prominence"])
        rows = stars.frame_stars(finder, case["frame"], case["mask"], o["threshold"], o["min_area"], o["max_area"])
        shapes = finder.measure() if measure else None
        if times is not None:
            times.append(finder.shape_ms())
        return rows, shapes
    finally:
        finder.close()


def moment_bounds(ref: dict) -> tuple[np.ndarray, np.ndarray]:
    """THE BOUND per row: on rr, cc, rc, and on abs_flux."""
    eps = 8 * ref["rows"][:, 3] * 2.0 ** -53
    abs_flux = ref["columns"][:, COL["abs_flux"]]
    return eps * (abs_flux / ref["rows"][:, 2]) * ref["rho2"], eps * abs_flux


def angle_between(a, b):
    """|a - b| modulo pi (an axis has no sign)."""
    return np.abs((a - b + np.pi / 2) % np.pi - np.pi / 2)


def check_shapes(make_finder, name: str) -> float:
    """One case against the restatement; returns the worst error / bound of the moments."""
    case = reference(name)
    ref = case["ref"]
    want = ref["columns"]
    rows, got = run(make_finder, case)
    assert got.dtype == np.float64 and got.shape == want.shape, f"{name}: {got.shape}, the restatement has {want.shape}"
    assert got[:, :4].tobytes() == rows.tobytes(), f"{name}: row, col, flux, area are not the detect's"
    sc.compare_rows(rows, {"rows": ref["rows"], "abs_flux": want[:, COL["abs_flux"]]}, case["frame"].shape, name)
    if len(want) == 0:
        return 0.0
    exact = [COL[c] for c in ("peak", "peak_row", "peak_col", "row_min", "row_max", "col_min", "col_max")]
    assert np.array_equal(got[:, exact], want[:, exact]), f"{name}: peak, its position or the box differ"
    bound, bound_abs = moment_bounds(ref)
    moments = [COL[c] for c in ("rr", "cc", "rc")]
    err = np.abs(got[:, moments] - want[:, moments]).max(axis=1)
    err_abs = np.abs(got[:, COL["abs_flux"]] - want[:, COL["abs_flux"]])
    worst = float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0))  # (a single pixel at its own centroid: rho^2 = 0, error 0)
    print(f"{name}: {len(want)} rows, areas {int(want[:, 3].min())} ... {int(want[:, 3].max())}, rho^2 <= {ref['rho2'].max():.0f}, moment error "
          f"{err.max():.2e} (worst error / bound {worst:.2e}), abs_flux error / bound {np.max(err_abs / bound_abs):.2e}")
    assert np.all(err <= bound) and np.all(err_abs <= bound_abs), name
    # the derived fields: exactly the host formula on the kernel's moments ...
    catalog = stars.catalog_from_shapes(got)
    assert catalog.dtype.names == FIELDS and all(catalog.dtype[n] == np.float64 for n in FIELDS)
    for j, column in enumerate(COLUMNS):
        assert catalog[column].tobytes() == got[:, j].tobytes()
    _, _, a, b, theta, elongation = ref_ellipse(got[:, COL["rr"]], got[:, COL["cc"]], got[:, COL["rc"]])
    for field, values in (("a", a), ("b", b), ("theta", theta), ("elongation", elongation)):
        assert catalog[field].tobytes() == values.tobytes(), (name, field)
    # ... and near the restatement's where lambda- is not within LAMBDA_GAP of zero (the precondition of this comparison): a moment off by
    # e moves the mean of the eigenvalues by at most e and their distance `half` from it by at most 2 e, so an eigenvalue by at most 3 e;
    # d sqrt(x) = dx / (2 sqrt(x)); theta moves by at most (2 e + e + e) / (4 half) = 2 e / (lambda+ - lambda-); 8 roundings of slack for
    # sqrt, atan2 and the sums
    lp, lm, ra, rb, rtheta, _ = ref_ellipse(want[:, COL["rr"]], want[:, COL["cc"]], want[:, COL["rc"]])
    far = np.abs(lm) > LAMBDA_GAP * np.abs(lp)
    slack = 8 * 2.0 ** -53
    with np.errstate(invalid="ignore", divide="ignore"):
        ok_a = np.abs(a - ra) <= 3 * bound / (2 * ra) + slack * ra
        ok_b = np.abs(b - rb) <= 3 * bound / (2 * rb) + slack * rb
        ok_theta = angle_between(theta, rtheta) <= 2 * bound / (lp - lm) + slack * np.pi
    positive = far & (lm > 0)
    assert np.all(ok_a[far & (lp > 0)]) and np.all(ok_b[positive]) and np.all(ok_theta[far & (lp - lm > 0)]), name
    assert np.array_equal(np.isnan(b[far]), lm[far] < 0)
    return worst


def check_empty(make_finder) -> None:
    """Pure background: zero rows of the right shape and dtype, and nothing launched."""
    case, times = reference("background"), []
    assert case["ref"]["rows"].shape == (0, 4)
    rows, shapes = run(make_finder, case, times=times)
    assert rows.shape == (0, 4) and shapes.shape == (0, len(COLUMNS)) and shapes.dtype == np.float64
    assert times == [0.0]
    catalog = stars.catalog_from_shapes(shapes)
    assert catalog.shape == (0,) and catalog.dtype.names == FIELDS
    times = []
    run(make_finder, reference("1 row"), times=times)
    assert times[0] > 0.0  # (the figure does move when S5 runs)


def check_single_pixels(make_finder) -> None:
    """min_area = 1: a detection of one pixel has no extent - zero moments exactly, a = b = 0, elongation NaN."""
    case = reference("single pixels")
    want = case["ref"]["columns"]
    single = want[:, 3] == 1
    at = {(int(r), int(c)) for r, c in want[single][:, [COL["peak_row"], COL["peak_col"]]]}
    assert set(EXACT_PIXELS + OTHER_PIXELS) <= at, at  # every planted pixel is a detection of its own
    exact = np.array([single[i] and (int(want[i, COL["peak_row"]]), int(want[i, COL["peak_col"]])) in EXACT_PIXELS for i in range(len(want))])
    assert exact.sum() == len(EXACT_PIXELS)
    assert np.array_equal(want[exact][:, :2], want[exact][:, [COL["peak_row"], COL["peak_col"]]])  # the centroid is the pixel, bit for bit
    _, got = run(make_finder, case)
    catalog = stars.catalog_from_shapes(got)[exact]
    for field in ("rr", "cc", "rc", "a", "b"):
        assert np.all(catalog[field] == 0.0), field
    assert np.isnan(catalog["elongation"]).all() and np.array_equal(catalog["peak"], catalog["flux"])
    assert np.array_equal(catalog["abs_flux"], catalog["flux"]) and np.array_equal(catalog["row_min"], catalog["row_max"])


def check_enclosure(make_finder) -> None:
    """Objects inside one another's bounding boxes: the moments of each hold its own pixels only."""
    for name in ("arc and star", "parallel streaks"):
        case = reference(name)
        ref = case["ref"]
        want, objmap, d = ref["columns"], ref["map"], ref["d"]
        big = np.argsort(want[:, 3])[-2:]  # the two objects of the case (noise may add small ones)
        foreign = {}
        for i, j in ((big[0], big[1]), (big[1], big[0])):
            r0, r1, c0, c1 = (int(v) for v in want[i, COL["row_min"]:COL["col_max"] + 1])
            inside = objmap[r0:r1 + 1, c0:c1 + 1] == j
            foreign[int(i)] = int(inside.sum())
            if inside.any():  # what the moment would be with the other's pixels in it: far outside the bound
                rr, cc = np.mgrid[r0:r1 + 1, c0:c1 + 1]
                both = (objmap[r0:r1 + 1, c0:c1 + 1] == i) | inside
                wrong = np.sum(d[r0:r1 + 1, c0:c1 + 1][both] * (rr[both] - want[i, 0]) ** 2) / want[i, 2]
                assert abs(wrong - want[i, COL["rr"]]) > 1e6 * moment_bounds(ref)[0][i]
        print(f"{name}: pixels of the other object inside the bounding box: {foreign}")
        if name == "arc and star":
            arc, star = (big[1], big[0]) if want[big[1], 3] > want[big[0], 3] else (big[0], big[1])
            assert foreign[int(arc)] == want[star, 3] and want[star, 3] > 20  # the whole star lies in the arc's box
        else:
            assert all(n > 20 for n in foreign.values())  # each streak has pixels in the other's box
        check_shapes(make_finder, name)


def check_row_counts(make_finder, walk_waves: int) -> None:
    """1, WALK_WAVES and WALK_WAVES + 1 kept rows: a lone wave, a full workgroup, and one with three idle waves."""
    assert sorted(ROW_COUNTS.values()) == [1, walk_waves, walk_waves + 1]
    for name, count in ROW_COUNTS.items():
        assert len(reference(name)["ref"]["rows"]) == count
        check_shapes(make_finder, name)


def check_reproducible(make_finder, name: str) -> None:
    """Repeats are bit-equal - on a fresh finder and by a second measure of the same detect - and find_stars' rows do not depend on
    whether measure ran in between."""
    case = reference(name)
    o = case["options"]
    rows, shapes = run(make_finder, case)
    again_rows, again = run(make_finder, case)
    assert shapes.tobytes() == again.tobytes() and rows.tobytes() == again_rows.tobytes()
    assert run(make_finder, case, measure=False)[0].tobytes() == rows.tobytes()
    finder = make_finder(case["frame"].shape, case["box"])
    try:
        if o["deblend"]:
            finder.set_deblend(True, o["contrast"], o["prominence"])
        args = (case["frame"], case["mask"], o["threshold"], o["min_area"], o["max_area"])
        first = stars.frame_stars(finder, *args)
        second = stars.frame_stars(finder, *args)  # no measure in between
        one, two = finder.measure(), finder.measure()
        third = stars.frame_stars(finder, *args)  # two of them in between
        assert first.tobytes() == second.tobytes() == third.tobytes() == rows.tobytes()
        assert one.tobytes() == two.tobytes() == shapes.tobytes() == finder.measure().tobytes()
    finally:
        finder.close()


def check_state_errors(make_finder, error: type) -> None:
    """measure before any detect, or after a new background, is refused with RPSF_E_BADARG's code; after the next detect it works."""
    import pytest

    case = reference("one_box")
    o = case["options"]
    finder = make_finder(case["frame"].shape, case["box"])
    try:
        with pytest.raises(error) as caught:
            finder.measure()
        assert caught.value.code == -1
        level, rms = finder.background(case["frame"], case["mask"])
        with pytest.raises(error) as caught:
            finder.measure()
        assert caught.value.code == -1
        level_f, _, global_rms = stars.filter_mesh(level, rms)
        rows = finder.detect(level_f, o["threshold"] * global_rms, o["min_area"], o["max_area"])
        shapes = finder.measure()
        assert len(rows) == 4 and shapes[:, :4].tobytes() == rows.tobytes()
        finder.background(case["frame"], case["mask"])  # the same frame again: still a new background
        with pytest.raises(error) as caught:
            finder.measure()
        assert caught.value.code == -1
        assert finder.detect(level_f, o["threshold"] * global_rms, o["min_area"], o["max_area"]).tobytes() == rows.tobytes()
        assert finder.measure().tobytes() == shapes.tobytes()
    finally:
        finder.close()


def check_ellipse_truth() -> tuple[float, float]:
    """The definition itself, on the restatement alone: every ellipse is one detection, theta is its angle within THETA_BOUND and
    a / b > ELONGATION_MIN.  Returns the worst angle error (degrees) and the smallest a / b."""
    ref = reference("ellipses")["ref"]
    centre, angles = ellipse_truth()
    assert len(ref["rows"]) == len(centre)
    dist = np.hypot(*(ref["rows"][:, None, :2] - centre[None]).transpose(2, 0, 1))
    match = dist.argmin(axis=1)
    assert sorted(match.tolist()) == list(range(len(centre))) and dist.min(axis=1).max() < 0.2
    cols = ref["columns"]
    _, _, a, b, theta, elongation = ref_ellipse(cols[:, COL["rr"]], cols[:, COL["cc"]], cols[:, COL["rc"]])
    err = np.degrees(angle_between(theta, np.radians(angles[match])))
    print(f"ellipses: sigma {ELLIPSES['sigma']}, a {a.min():.2f} ... {a.max():.2f}, b {b.min():.2f} ... {b.max():.2f}, worst angle error "
          f"{err.max():.3f} degrees (bound {THETA_BOUND}), smallest a / b {elongation.min():.3f}")
    assert np.all(a > b) and err.max() <= THETA_BOUND and elongation.min() > ELONGATION_MIN
    assert np.all(a < ELLIPSES["sigma"][0]) and np.all(b < ELLIPSES["sigma"][1])  # the truncation biases both low
    return float(err.max()), float(elongation.min())
