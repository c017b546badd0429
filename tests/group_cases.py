"""Group fits (DESIGN.md 3.7 "Group fits", kernel S11) and the host grouping restated in float64 NumPy / SciPy, the cases, the CPU
emulator of the kernel, and the checks the emulator tests (tests/test_group_host.py) and the GPU tests (tests/test_gpu_group.py) share.

THE GROUPING is restated with SciPy: `cKDTree.query_pairs` at a slightly larger radius proposes the pairs, the exact formula dy dy + dx dx
<= L L in float64 decides, `scipy.sparse.csgraph.connected_components` finds the components.

S11 is restated BIT FOR BIT, as fit_cases restates S8 (see there for the mesh, the model, the sums and the peak): the restatement does
the kernel's float64 operations in the kernel's order.  What is new here:
  the sums    of pass 1 and of the group's residual run over SEVERAL boxes: lane j of 64 takes pixels j, j + 64, ... of member 0's box,
              then of member 1's, and so on, into one running sum, which folds once, as S8's (`ordered_sum_boxes`);
  the solve   is the LDL^T elimination of fitpos_cases at a runtime order, in scalar float64, in the kernel's order (`ref_solve`);
  the model   sum at a pixel is render_cases': S = 0.0, then S = S + f_b m_b over the members that hold the pixel, ascending.
A member's own S8 sums are fit_cases.ref_fit's, which is what the kernel delivers.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np

from tests import emulib
from regularizepsf_amd import stars
from tests import fit_cases as fc
from tests import photometry_cases as pc
from tests import render_cases as rn
from tests import star_cases as sc

ROOT = sc.ROOT
COLUMNS = 25
GROUP, GROUP_SIZE, GROUP_N, GROUP_CHI2, GROUP_ABS = range(fc.COLUMNS, COLUMNS)
CROWDED, MAX_GROUP = 16, 8
SHAPE, BOX, LANES = fc.SHAPE, fc.BOX, fc.LANES
same_bits = fc.same_bits


# ------------------------------------------------------------------------------------------------------------------ the grouping
def ref_groups(positions, eligible, link: float, max_group: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, list[np.ndarray]]:
    """(label, size, crowded, groups): the definition, with SciPy.  groups: the components of 2 .. max_group members, ascending label,
    members ascending."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree

    positions = np.asarray(positions, np.float64).reshape(-1, 2)
    n = len(positions)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, bool), []
    eligible = np.ones(n, bool) if eligible is None else np.asarray(eligible, bool)
    L = np.float64(link)
    pairs = cKDTree(positions).query_pairs(float(L) * (1 + 1e-9) + 1e-12, output_type="ndarray").reshape(-1, 2)
    dy, dx = positions[pairs[:, 0], 0] - positions[pairs[:, 1], 0], positions[pairs[:, 0], 1] - positions[pairs[:, 1], 1]
    keep = (dy * dy + dx * dx <= L * L) & eligible[pairs[:, 0]] & eligible[pairs[:, 1]]
    pairs = pairs[keep]
    graph = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, component = connected_components(graph, directed=False)
    first = np.full(component.max() + 1, n, np.int64)
    np.minimum.at(first, component, np.arange(n))
    label = first[component].astype(np.int32)
    size = np.bincount(component)[component].astype(np.int32)
    crowded = size > max_group
    groups = [np.flatnonzero(label == root) for root in np.flatnonzero((label == np.arange(n)) & (size >= 2) & ~crowded)]
    return label, size, crowded, groups


# ------------------------------------------------------------------------------------------------------------------ the restatement
def ordered_sum_boxes(boxes) -> np.float64:
    """S11's summation order over several boxes (`boxes`: per member one value per pixel of its box in raster order, 0.0 where the kernel
    skips the pixel): a lane's sum runs on from one box to the next; one fold."""
    lanes = np.zeros(LANES)
    for terms in boxes:
        flat = np.asarray(terms, np.float64).ravel()
        padded = np.zeros(-(-max(flat.size, 1) // LANES) * LANES)
        padded[:flat.size] = flat
        for chunk in padded.reshape(-1, LANES):
            lanes = lanes + chunk
    groups = np.zeros(8)
    for j in range(8):
        groups = groups + lanes.reshape(8, 8)[:, j]
    total = np.float64(0.0)
    for g in groups:
        total = total + g
    return total


def ref_solve(A: np.ndarray, b: np.ndarray):
    """solve_ldl_n: the unknowns, or None at a pivot that is not finite or <= 0.  A's upper triangle is read."""
    A, b = np.array(A, np.float64), np.array(b, np.float64)
    K = len(b)
    x = np.zeros(K)
    with np.errstate(all="ignore"):
        for j in range(K):
            pivot = A[j, j]
            if not np.isfinite(pivot) or pivot <= 0.0:
                return None
            for i in range(j + 1, K):
                l = A[j, i] / pivot
                for c in range(i, K):
                    A[i, c] = A[i, c] - l * A[j, c]
                b[i] = b[i] - l * b[j]
        for j in range(K - 1, -1, -1):
            s = b[j]
            for c in range(j + 1, K):
                s = s - A[j, c] * x[c]
            x[j] = s / A[j, j]
    return x


def _boxes(d, ok, cube, positions, cells, members, R):
    """Per member a of the group its box and, on it: `inside[b]` and `m[b]` for every member b, and which pixels count for the fit."""
    H, W = d.shape
    R2 = R * R
    out = []
    for a in members:
        y, x = positions[a]
        rr = np.arange(int(np.floor(y - R)) - 1, int(np.ceil(y + R)) + 2)
        cc = np.arange(int(np.floor(x - R)) - 1, int(np.ceil(x + R)) + 2)
        inside, m = [], []
        for b in members:
            pr, pc_ = rr.astype(np.float64) - positions[b][0], cc.astype(np.float64) - positions[b][1]
            disc = ((pr * pr)[:, None] + (pc_ * pc_)[None, :]) <= R2
            inside.append(disc)
            m.append(fc.ref_model(cube[cells[b]], pr, pc_, disc))
        on_frame = ((rr >= 0) & (rr < H))[:, None] & ((cc >= 0) & (cc < W))[None, :]
        ri, ci = np.clip(rr, 0, H - 1), np.clip(cc, 0, W - 1)
        use = on_frame & ok[ri[:, None], ci[None, :]]
        dv = np.where(use, d[ri[:, None], ci[None, :]], 0.0)
        out.append({"rr": rr, "cc": cc, "inside": inside, "m": m, "use": use, "d": dv})
    return out


def ref_group(d, ok, cube, positions, cells, members, radius, fit_background: bool, single: np.ndarray) -> tuple[np.ndarray, dict]:
    """One group: (len(members), COLUMNS) rows, and what the independent solve needs.  `single`: fit_cases.ref_fit's rows of the members."""
    g, R = len(members), np.float64(radius)
    boxes = _boxes(d, ok, cube, positions, cells, members, R)
    counted = []
    for a, box in enumerate(boxes):
        owned = box["inside"][a].copy()
        for b in range(a):
            owned &= ~box["inside"][b]
        box["owned"] = owned
        counted.append(owned & box["use"])
    n = int(sum(c.sum() for c in counted))
    held = lambda a, b: counted[a] & boxes[a]["inside"][b]
    term = lambda f: ordered_sum_boxes([f(a, box) for a, box in enumerate(boxes)])
    with np.errstate(all="ignore"):
        Sd = term(lambda a, box: np.where(counted[a], box["d"], 0.0))
        Sm = [term(lambda a, box: np.where(held(a, b), box["m"][b], 0.0)) for b in range(g)]
        Sdm = [term(lambda a, box: np.where(held(a, b), box["d"] * box["m"][b], 0.0)) for b in range(g)]
        p = g + int(fit_background)
        A, rhs = np.zeros((p, p)), np.zeros(p)
        for b in range(g):
            for c in range(b, g):
                A[b, c] = term(lambda a, box: np.where(held(a, b) & held(a, c), box["m"][b] * box["m"][c], 0.0))
            rhs[b] = Sdm[b]
            if fit_background:
                A[b, g] = Sm[b]
        if fit_background:
            A[g, g], rhs[g] = np.float64(n), Sd
    flags, x = 0, None
    if n < p:
        flags = fc.TOO_FEW
    else:
        x = ref_solve(A, rhs)
        if x is None or not np.all(np.isfinite(x)):
            flags, x = fc.DEGENERATE, None
    rows = np.full((g, COLUMNS), np.nan)
    rows[:, :fc.COLUMNS] = single
    rows[:, fc.FLAGS] = flags
    rows[:, fc.F:fc.PEAK_E + 1] = np.nan
    rows[:, fc.PEAK_ROW], rows[:, fc.PEAK_COL] = -1.0, -1.0
    rows[:, GROUP], rows[:, GROUP_SIZE], rows[:, GROUP_N] = members[0], g, n
    design = {"A": A, "rhs": rhs, "x": x, "n": n, "boxes": boxes, "counted": counted}
    if flags:
        return rows, design
    bg = x[g] if fit_background else np.float64(0.0)
    ge2, gea = [], []
    for a, box in enumerate(boxes):
        use = box["inside"][a] & box["use"]
        with np.errstate(all="ignore"):
            S = np.zeros(use.shape)
            for b in range(g):
                S = np.where(box["inside"][b], S + x[b] * box["m"][b], S)
            e = box["d"] - (S + bg)
            e2, ea = np.where(use, e * e, 0.0), np.where(use, np.abs(e), 0.0)
            key = np.where(use, np.where(np.isnan(e), np.inf, np.abs(e)), -1.0)
        ge2.append(np.where(box["owned"], e2, 0.0)), gea.append(np.where(box["owned"], ea, 0.0))
        rows[a, fc.F], rows[a, fc.BG], rows[a, fc.CHI2], rows[a, fc.ABS_RES] = x[a], bg, fc.ordered_sum(e2), fc.ordered_sum(ea)
        if use.any():
            top = int(np.argmax(key.ravel()))
            rows[a, fc.PEAK_RES], rows[a, fc.PEAK_E] = np.abs(e.ravel()[top]), e.ravel()[top]
            rows[a, fc.PEAK_ROW], rows[a, fc.PEAK_COL] = box["rr"][top // len(box["cc"])], box["cc"][top % len(box["cc"])]
    rows[:, GROUP_CHI2], rows[:, GROUP_ABS] = ordered_sum_boxes(ge2), ordered_sum_boxes(gea)
    return rows, design


def ref_fit_groups(frame, mask, box, level_f, cube, positions, cells, radius, fit_background: bool, background: str, link=None,
                   max_group: int = MAX_GROUP, designs: list | None = None) -> np.ndarray:
    """The definition of rpsf_stars_fit_groups: (k, COLUMNS) rows in the kernel's layout."""
    cube = np.asarray(cube, np.float64)
    positions = np.asarray(positions, np.float64).reshape(-1, 2)
    cells = np.asarray(cells, np.int64)
    link = 2.0 * float(radius) if link is None else float(link)
    single = fc.ref_fit(frame, mask, box, level_f, cube, positions, cells, radius, fit_background, background)
    no_mesh = background == "mesh" and level_f is None
    in_model = (cells >= 0) & (cells < len(cube))
    finite = np.isfinite(cube).all(axis=(1, 2))
    eligible = in_model & finite[np.clip(cells, 0, len(cube) - 1)] & (not no_mesh)
    label, size, crowded, groups = ref_groups(positions, eligible, link, max_group)
    rows = np.empty((len(positions), COLUMNS))
    rows[:, :fc.COLUMNS] = single
    rows[:, GROUP], rows[:, GROUP_SIZE] = label, size
    rows[:, GROUP_N], rows[:, GROUP_CHI2], rows[:, GROUP_ABS] = single[:, fc.N_USE], single[:, fc.CHI2], single[:, fc.ABS_RES]
    if groups:
        d, ok = pc.ref_residual(frame, mask, box, level_f, background)
    for members in groups:
        rows[members], design = ref_group(d, ok, cube, positions, cells, members, radius, fit_background, single[members])
        if designs is not None:
            designs.append((members, design))
    return rows


# ------------------------------------------------------------------------------------------------------------------ the cases
GAUSSIAN, ZERO, LOBES, CONSTANT = fc.GAUSSIAN, fc.ZERO, fc.LOBES, fc.CONSTANT
CROWD_LINK = 4.5  # below 2 R of every radius the crowd is fitted with, so the groups below are the same at every model size


def crowd() -> tuple[np.ndarray, np.ndarray]:
    """On the 48 x 40 field, more than CROWD_LINK apart from one another: a pair 1.5 px apart on a star, a pair 3 px apart on another, a
    chain of three whose ends are not linked, a full group of 8, a star alone, a pair of mixed cells, a pile of 9 (crowded), and a star
    of no cell of the model between two others."""
    pairs = [(20.3, 17.6), (20.3, 19.1), (12.0, 30.0), (12.0, 33.0), (33.5, 10.5), (33.5, 14.5), (33.5, 18.5)]
    eight = [(42.2, 8.0 + 2.5 * k) for k in range(8)]
    rest = [(8.0, 8.5), (5.0, 20.0), (6.5, 22.0)]
    pile = [(25.0, 33.0 + 0.5 * k) for k in range(9)]
    between = [(31.5, 26.0), (31.5, 30.0), (31.5, 34.0)]
    positions = np.array(pairs + eight + rest + pile + between)
    cells = np.full(len(positions), GAUSSIAN)
    cells[len(pairs) + len(eight) + 2] = LOBES
    cells[-2] = -1
    return positions, cells


CROWD_SIZES = [2, 2, 2, 2, 3, 3, 3] + [8] * 8 + [1, 2, 2] + [9] * 9 + [1, 1, 1]
GROUP_RADII = {8: (2.5, 3.0), 9: (2.3, 3.5), 16: (4.6,)}  # one that is no integer at every size, and N / 2 - 1


def _case(frame, positions, cells, n, background="mesh", fit_background=True, mask=None, radii=None, box=BOX, cube=None, link=None,
          max_group=MAX_GROUP) -> dict:
    c = fc._case(frame, positions, cells, n, background, fit_background, mask, GROUP_RADII[n] if radii is None else radii, box, cube)
    c.update(link=link, max_group=max_group)
    return c


def _crowd_case(n, background, fit_background) -> dict:
    return _case(fc.field()["frame"], *crowd(), n, background, fit_background, link=CROWD_LINK)


def _masked_case(background, fit_background) -> dict:
    m = fc.masked_field()
    return _case(m["frame"], *crowd(), 9, background, fit_background, m["mask"], link=CROWD_LINK)


GROUP_COUNTS = (0, 1, 3, 4, 5, 9)  # 0, 1, WALK_WAVES - 1, WALK_WAVES, WALK_WAVES + 1, 2 WALK_WAVES + 1 (check_group_counts asserts that)


def _count_case(k: int) -> dict:
    """k pairs, 2 px apart, on a 3 x 3 grid of the field, and two stars alone."""
    at = [(r, c) for r in (8.0, 24.0, 40.0) for c in (7.0, 20.0, 33.0)][:k]
    positions = [(16.0, 14.0)] + [p for r, c in at for p in ((r, c), (r + 0.5, c + 2.0))] + [(32.0, 27.0)]
    cells = [GAUSSIAN] + [GAUSSIAN, LOBES] * len(at) + [GAUSSIAN]
    return _case(fc.field()["frame"], positions, cells, 9, radii=(2.0,))


CROWD_CASES = {f"crowd, N = {n}, {b}, {'flux and background' if fb else 'flux alone'}": functools.partial(_crowd_case, n, b, fb)
               for n in (8, 9, 16) for b in ("mesh", "none") for fb in (True, False)}
MASKED_CASES = {f"masked crowd, {b}, {'flux and background' if fb else 'flux alone'}": functools.partial(_masked_case, b, fb)
                for b in ("mesh", "none") for fb in (True, False)}
OTHER_CASES = {
    # exactly 2 R apart: linked (49 <= 49), and the discs share the pixel (20, 17)
    "a pair exactly 2 R apart": lambda: _case(fc.field()["frame"], [(20.0, 14.0), (20.0, 20.0), (30.0, 14.0), (30.0, np.nextafter(20.0, 21.0))],
                                               [GAUSSIAN] * 4, 8, radii=(3.0,)),
    "a group across the rim": lambda: _case(fc.field()["frame"], [(0.5, 1.0), (1.5, 3.0), (47.2, 38.0), (46.0, 40.5), (49.0, 39.0)], [GAUSSIAN] * 5, 9,
                                            radii=(3.5,)),
    "a group off the frame": lambda: _case(fc.field()["frame"], [(-30.0, -30.0), (-31.0, -30.5), (20.3, 17.6), (60.0, 20.0), (61.0, 22.0), (60.5, 18.0)],
                                           [GAUSSIAN] * 6, 9, "none", radii=(3.5,)),
    "a zero cell in a group": lambda: _case(fc.field()["frame"], [(20.3, 17.6), (21.3, 19.1), (12.0, 30.0), (13.0, 31.0), (14.5, 32.0)],
                                            [GAUSSIAN, ZERO, ZERO, GAUSSIAN, LOBES], 9, radii=(3.5,)),
    "two members at one position": lambda: _case(fc.field()["frame"], [(20.3, 17.6), (20.3, 17.6), (12.0, 30.0), (12.0, 30.0), (13.5, 31.0)],
                                                 [GAUSSIAN] * 5, 9, "none", radii=(3.5,)),
    "two at one position, flux alone": lambda: _case(fc.field()["frame"], [(20.3, 17.6), (20.3, 17.6), (12.0, 30.0), (12.0, 30.0), (13.5, 31.0)],
                                                     [GAUSSIAN] * 5, 9, "none", False, radii=(3.5,)),
    "no valid mesh node": lambda: _case(np.full(SHAPE, np.nan, np.float32), [(30.2, 20.7), (31.0, 21.0), (-30.0, -30.0), (10.0, 10.0)],
                                        [GAUSSIAN, GAUSSIAN, LOBES, 7], 9, radii=(3.5,)),
    "a cell of NaN": lambda: _case(fc.field()["frame"], [(20.3, 17.6), (21.3, 19.1), (22.3, 20.6)], [GAUSSIAN, ZERO, LOBES], 9, radii=(3.5,),
                                   cube=np.where(np.arange(4)[:, None, None] == ZERO, np.nan, fc.model(9))),
    "max_group 1": lambda: _case(fc.field()["frame"], *crowd(), 9, radii=(2.3,), link=CROWD_LINK, max_group=1),
    "max_group 2": lambda: _case(fc.field()["frame"], *crowd(), 9, radii=(2.3,), link=CROWD_LINK, max_group=2),
    "a link below every separation": lambda: _case(fc.field()["frame"], *crowd(), 9, radii=(2.3,), link=0.25),
    "the default link": lambda: _case(fc.field()["frame"], *crowd(), 9, "none", radii=(2.3,)),
    "box 8": lambda: _case(fc.field()["frame"], *crowd(), 16, radii=(7.0,), box=8, link=CROWD_LINK),
}
COUNT_CASES = {f"{k} groups": functools.partial(_count_case, k) for k in GROUP_COUNTS}
CASES = {**CROWD_CASES, **MASKED_CASES, **OTHER_CASES, **COUNT_CASES}


@functools.cache
def case(name: str) -> dict:
    return sc._freeze(CASES[name]())


@functools.lru_cache(maxsize=None)
def _reference(name: str, mesh_bytes: bytes | None, radius: float) -> tuple:
    c = case(name)
    level_f = None if mesh_bytes is None else np.frombuffer(mesh_bytes).reshape(-(-c["frame"].shape[0] // c["box"]), -(-c["frame"].shape[1] // c["box"]))
    designs = []
    out = ref_fit_groups(c["frame"], c["mask"], c["box"], level_f, c["cube"], c["positions"], c["cells"], radius, c["fit_background"],
                         c["background"], c["link"], c["max_group"], designs)
    out.flags.writeable = False
    return out, designs


def reference(name: str, level_f, radius: float, with_designs: bool = False):
    """The restatement's rows for the case on the filtered mesh `level_f` (None: no valid node), computed once per case, mesh and radius."""
    mesh = None if level_f is None or case(name)["background"] == "none" else np.ascontiguousarray(level_f).tobytes()
    rows, designs = _reference(name, mesh, float(radius))
    return (rows, designs) if with_designs else rows


# ------------------------------------------------------------------------------------------------------------------ the emulator
@functools.cache
def emulator():
    """tests/emu/libemu_group.so: the kernel's driver and the grouping on the CPU, compiled here when missing or older than its sources."""
    lib = emulib.library("emu_group")
    vp, i, n, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    lib.emugr_info.argtypes = [vp]
    lib.emugr_link.argtypes = [n, vp, vp, f, i, vp, vp, vp]
    lib.emugr_fit_groups.argtypes = [vp, vp, i, i, i, vp, i, n, i, vp, n, vp, vp, f, i, i, f, i, vp]
    return lib


def emulator_info() -> tuple[int, int, int, int, int, int]:
    """WALK_WAVES, the workgroups of S11 and of S8 the last fit ran, s11_lds_bytes(), MAX_GROUP, the columns of a row."""
    info = (ctypes.c_long * 6)(0, 0, 0, 0, 0, 0)
    emulator().emugr_info(info)
    return tuple(info)


def emu_link(positions, eligible, link, max_group) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """rpsf_stars_link_groups on the emulator's copy of the host code: (label, size, crowded)."""
    positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
    flags = None if eligible is None else np.ascontiguousarray(np.asarray(eligible, bool), np.uint8)
    labels, sizes, crowded = np.zeros(len(positions), np.int32), np.zeros(len(positions), np.int32), np.zeros(len(positions), np.uint8)
    code = emulator().emugr_link(len(positions), positions.ctypes.data, None if flags is None else flags.ctypes.data, float(link), int(max_group),
                                 labels.ctypes.data, sizes.ctypes.data, crowded.ctypes.data)
    if code != 0:
        raise EmuError(-1, "bad argument")
    return labels, sizes, crowded != 0


EmuError, EmuModel = fc.EmuError, fc.EmuModel


class EmuFinder(rn.EmuFinder):
    """render_cases.EmuFinder with ``fit_groups``: regularizepsf_amd.stars._Finder's interface on the emulator."""

    def __init__(self, shape, box, device=0) -> None:
        super().__init__(shape, box, device)
        self._grouped = 0

    def fit_groups(self, model, positions, cells, radius, fit_background=True, use_mesh=True, link=None, max_group=MAX_GROUP):
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        cells = np.ascontiguousarray(cells, np.int32).ravel()
        if len(cells) != len(positions):
            raise ValueError(f"{len(cells)} cells for {len(positions)} positions")
        out = np.empty((len(positions), COLUMNS))
        level = None if self._filtered is None else np.ascontiguousarray(self._filtered[0])
        frame, mask = (self._frame, self._mask) if self._frame is not None else (np.zeros(self.shape, np.float32), None)
        code = emulator().emugr_fit_groups(frame.ctypes.data, None if mask is None else mask.ctypes.data, *self.shape, self.box,
                                           None if level is None else level.ctypes.data, int(level is None), len(model.values), model.size,
                                           model.values.ctypes.data, len(positions), positions.ctypes.data, cells.ctypes.data, float(radius),
                                           int(bool(fit_background)), int(bool(use_mesh)), 2.0 * float(radius) if link is None else float(link),
                                           int(max_group), out.ctypes.data)
        if code != 0 or model.device != self._device:
            raise EmuError(-1, "bad argument")
        if not self._have_mesh:  # (the library checks its arguments first, then its state)
            raise EmuError(-6, "fit_groups before background_device")
        self._grouped = sum(emulator_info()[1:3])
        return out

    def fit_groups_ms(self) -> float:
        """In the place of the device time: the workgroups of S11 and S8 that ran - 0.0 exactly when nothing was launched."""
        return float(self._grouped)


# ------------------------------------------------------------------------------------------------------------------ the checks
def check_grouping(link_groups) -> None:
    """The grouping against the SciPy restatement.  `link_groups(positions, eligible, link, max_group)` -> (label, size, crowded)."""
    rng = np.random.default_rng([12, 67])

    def same(positions, eligible, link, max_group, what):
        label, size, crowded = link_groups(positions, eligible, link, max_group)
        want = ref_groups(positions, eligible, link, max_group)
        print(f"grouping, {what}: {len(label)} stars, {len(set(label.tolist()))} components, largest {int(size.max(initial=0))}, "
              f"{int(np.sum(crowded))} crowded, {len(want[3])} groups to fit")
        assert label.tolist() == want[0].tolist() and size.tolist() == want[1].tolist() and crowded.tolist() == want[2].tolist(), what
        return label, size, crowded

    same(np.zeros((0, 2)), None, 3.0, 8, "n = 0")
    assert same([(5.0, 5.0)], None, 3.0, 8, "n = 1")[0].tolist() == [0]
    label, size, _ = same([(0.0, 0.0), (0.0, 2.0), (0.0, 4.0)], None, 2.5, 8, "a chain of three")
    assert label.tolist() == [0, 0, 0] and size.tolist() == [3, 3, 3]
    ring = np.array([(10 * np.cos(t), 10 * np.sin(t)) for t in np.linspace(0, 2 * np.pi, 6, endpoint=False)])  # neighbours 10 apart
    assert same(ring, None, 10.5, 8, "a ring")[1].tolist() == [6] * 6
    assert same(ring, None, 9.5, 8, "a ring, cut")[1].tolist() == [1] * 6
    assert same([(0.0, 0.0), (3.0, 4.0)], None, 5.0, 8, "(0, 0) and (3, 4), link 5")[0].tolist() == [0, 0]
    assert same([(0.0, 0.0), (3.0, 4.0)], None, np.nextafter(5.0, 0.0), 8, "the same, a bit below 5")[0].tolist() == [0, 1]
    assert same([(7.0, 7.0)] * 3 + [(20.0, 20.0)], None, 1e-3, 8, "coincident stars")[0].tolist() == [0, 0, 0, 3]
    label, size, _ = same([(0.0, 0.0), (0.0, 2.0), (0.0, 4.0)], [True, False, True], 2.5, 8, "an ineligible star between two others")
    assert label.tolist() == [0, 1, 2] and size.tolist() == [1, 1, 1]
    cluster = np.concatenate([[(30.0 + 0.3 * k, 30.0) for k in range(9)], [(0.0, 0.0), (0.0, 1.0)]])
    label, size, crowded = same(cluster, None, 1.0, 8, "a cluster of 9")
    assert size[:9].tolist() == [9] * 9 and crowded.tolist() == [True] * 9 + [False] * 2 and label[:9].tolist() == [0] * 9
    label, size, crowded = same(cluster, None, 1.0, 1, "max_group = 1")
    assert crowded.all() and size.tolist() == [9] * 9 + [2, 2]
    many = rng.uniform(0.0, 200.0, (2000, 2))
    many[::7] = np.rint(many[::7])  # some on a lattice: exact distances, among them == link
    eligible = rng.random(2000) > 0.05
    for link, max_group in ((3.0, 8), (5.0, 4), (1.0, 8), (2.0 ** -12, 8)):
        label, size, crowded = same(many, eligible, link, max_group, f"2 000 random positions, link {link:g}")
        order = rng.permutation(len(many))
        plabel, psize, pcrowded = same(many[order], eligible[order], link, max_group, "the same set permuted")
        # the same partition, whatever the order: members of one component before are members of one after
        assert psize.tolist() == size[order].tolist() and pcrowded.tolist() == crowded[order].tolist()
        groups_before = {frozenset(np.flatnonzero(label == root).tolist()) for root in set(label.tolist())}
        groups_after = {frozenset(order[np.flatnonzero(plabel == root)].tolist()) for root in set(plabel.tolist())}
        assert groups_before == groups_after
        assert all(plabel[i] == min(np.flatnonzero(plabel == plabel[i])) for i in range(0, len(many), 97))  # the smallest index
    far = np.array([(2.0 ** 20 - 1, 1 - 2.0 ** 20), (2.0 ** 20 - 1, 2 - 2.0 ** 20), (1 - 2.0 ** 20, 2.0 ** 20 - 1)])
    assert same(far, None, 1.0, 8, "the largest coordinates")[0].tolist() == [0, 0, 2]


def run(make_finder, make_model, c: dict, times: list | None = None) -> tuple:
    """The product's per-frame route on a finder: (the filtered mesh or None, {radius: S11's and S8's rows})."""
    finder, model = make_finder(c["frame"].shape, c["box"]), None
    try:
        model = make_model(c["cube"])
        level, rms = finder.background(c["frame"], c["mask"])
        filtered = stars.filter_mesh(level, rms)
        finder.background_device(c["frame"], c["mask"])
        rows = {}
        for radius in c["radii"]:
            rows[radius] = finder.fit_groups(model, c["positions"], c["cells"], radius, c["fit_background"], c["background"] == "mesh", c["link"],
                                             c["max_group"])
            if times is not None:
                times.append(finder.fit_groups_ms())
        return (None if filtered is None else filtered[0]), rows
    finally:
        if model is not None:
            model.close()
        finder.close()


def check_case(make_finder, make_model, name: str) -> dict:
    """Every row of every radius of the case against the restatement, bit for bit.  Returns {radius: rows}."""
    c = case(name)
    level_f, rows = run(make_finder, make_model, c)
    for radius, got in rows.items():
        want = reference(name, level_f, radius)
        assert got.dtype == np.float64 and got.shape == want.shape, f"{name}: {got.shape}, the restatement has {want.shape}"
        flags, sizes = got[:, fc.FLAGS].astype(int), got[:, GROUP_SIZE].astype(int)
        differ = [i for i in range(len(want)) if not same_bits(got[i], want[i])]
        print(f"{name}, R = {radius:g}: {len(want)} rows, group sizes {np.bincount(sizes, minlength=2)[1:].tolist()} (stars per size 1, 2, ...), "
              f"flags {sorted(set(flags.tolist()))}, group_n <= {int(want[:, GROUP_N].max(initial=0))}, {len(differ)} rows differ from the restatement")
        assert not differ, (name, radius, differ[:3], got[differ[0]], want[differ[0]])
    return rows


def check_crowd_groups(make_finder, make_model) -> None:
    """The crowd is grouped as it was laid out, at every model size; a group's members carry one label, one n and one chi2."""
    for n in (8, 9, 16):
        c = case(f"crowd, N = {n}, mesh, flux and background")
        for radius, got in run(make_finder, make_model, c)[1].items():
            assert got[:, GROUP_SIZE].astype(int).tolist() == CROWD_SIZES, (n, radius)
            fitted = (got[:, GROUP_SIZE] >= 2) & (got[:, GROUP_SIZE] <= MAX_GROUP)
            assert np.all(got[fitted, fc.FLAGS] == 0) and np.isfinite(got[fitted]).all()
            for root in set(got[fitted, GROUP].astype(int).tolist()):
                members = np.flatnonzero(got[:, GROUP] == root)
                assert members[0] == root and len(members) == got[root, GROUP_SIZE]
                for column in (GROUP_N, GROUP_CHI2, GROUP_ABS, fc.BG):
                    assert len(set(got[members, column].tolist())) == 1
                assert got[root, GROUP_N] <= got[members, fc.N_USE].sum() and got[root, GROUP_N] >= got[members, fc.N_USE].max()
            alone = ~fitted
            assert np.array_equal(got[alone, GROUP_N], got[alone, fc.N_USE])
            assert same_bits(got[alone, GROUP_CHI2], got[alone, fc.CHI2]) and same_bits(got[alone, GROUP_ABS], got[alone, fc.ABS_RES])


def check_every_flag_fires(make_finder, make_model) -> None:
    """TOO_FEW and DEGENERATE go to every member of a group and leave NaN; a member without a pixel of its own has no peak."""
    got = run(make_finder, make_model, case("a group off the frame"))[1][3.5]
    assert got[:, fc.FLAGS].astype(int).tolist() == [fc.TOO_FEW, fc.TOO_FEW, 0, fc.TOO_FEW, fc.TOO_FEW, fc.TOO_FEW]
    assert got[:, GROUP_SIZE].astype(int).tolist() == [2, 2, 1, 3, 3, 3] and np.all(got[[0, 1, 3, 4, 5], GROUP_N] == 0)
    flagged = got[[0, 1, 3, 4, 5]]
    assert np.isnan(flagged[:, fc.F:fc.PEAK_E + 1]).all() and np.all(flagged[:, fc.PEAK_ROW:fc.PEAK_COL + 1] == -1.0)
    assert np.isnan(flagged[:, GROUP_CHI2:]).all() and np.all(flagged[:, fc.N_ALL] > 0) and np.all(flagged[:, fc.SM] == 0.0)
    got = run(make_finder, make_model, case("a zero cell in a group"))[1][3.5]
    assert np.all(got[:, fc.FLAGS] == fc.DEGENERATE) and got[:, GROUP_SIZE].astype(int).tolist() == [2, 2, 3, 3, 3]
    assert np.isnan(got[:, fc.F:fc.PEAK_E + 1]).all() and np.all(got[:, fc.N_USE] > 0) and np.all(got[:, GROUP_N] > 0)
    assert got[1, fc.SMM] == 0.0 and got[0, fc.SMM] > 0.0  # the members' own sums are delivered
    for name in ("two members at one position", "two at one position, flux alone"):
        got = run(make_finder, make_model, case(name))[1][3.5]
        assert np.all(got[:, fc.FLAGS] == fc.DEGENERATE) and got[:, GROUP_SIZE].astype(int).tolist() == [2, 2, 3, 3, 3]
    got = run(make_finder, make_model, case("a group across the rim"))[1][3.5]
    assert got[:, GROUP_SIZE].astype(int).tolist() == [2, 2, 3, 3, 3] and np.all(got[:, fc.FLAGS] == 0)
    assert np.all(got[:, fc.N_USE] < got[:, fc.N_ALL]) and np.all(got[:, GROUP_N] > 0)
    got = run(make_finder, make_model, case("no valid mesh node"))[1][3.5]  # every star alone, through S8: NO_MESH
    assert got[:, fc.FLAGS].astype(int).tolist() == [fc.NO_MESH] * 3 + [fc.NO_MESH | fc.BAD_CELL] and np.all(got[:, GROUP_SIZE] == 1)
    got = run(make_finder, make_model, case("a cell of NaN"))[1][3.5]  # the star of the NaN cell is alone and DEGENERATE, the others a pair
    assert got[:, fc.FLAGS].astype(int).tolist() == [0, fc.DEGENERATE, 0] and got[:, GROUP_SIZE].astype(int).tolist() == [2, 1, 2]
    got = run(make_finder, make_model, case("a pair exactly 2 R apart"))[1][3.0]
    assert got[:, GROUP_SIZE].astype(int).tolist() == [2, 2, 1, 1] and np.all(got[:, fc.FLAGS] == 0)
    assert got[0, GROUP_N] == got[0, fc.N_USE] + got[1, fc.N_USE] - 1  # the discs share one pixel, (20, 17)


def check_group_counts(make_finder, make_model, walk_waves: int) -> None:
    """0 ... 2 WALK_WAVES + 1 groups: a group's rows do not depend on the other groups of its workgroup; nothing to fit launches nothing."""
    assert GROUP_COUNTS == (0, 1, walk_waves - 1, walk_waves, walk_waves + 1, 2 * walk_waves + 1)
    whole = None
    for k in reversed(GROUP_COUNTS):
        c, times = case(f"{k} groups"), []
        got = run(make_finder, make_model, c, times)[1][2.0]
        assert got.shape == (2 * k + 2, COLUMNS) and times[0] > 0.0
        assert got[:, GROUP_SIZE].astype(int).tolist() == [1] + [2] * (2 * k) + [1] and np.all(got[:, fc.FLAGS] == 0)
        whole = got if whole is None else whole
        assert got[:-1, :GROUP].tobytes() == whole[:2 * k + 1, :GROUP].tobytes()  # (the labels of later stars move with the count)
        assert got[-1, :GROUP].tobytes() == whole[-1, :GROUP].tobytes()
    finder, model_ = make_finder(SHAPE, BOX), make_model(fc.model(9))
    try:
        finder.background_device(fc.field()["frame"], None)
        assert finder.fit_groups(model_, np.zeros((0, 2)), np.zeros(0, np.int32), 2.0).shape == (0, COLUMNS) and finder.fit_groups_ms() == 0.0
    finally:
        model_.close()
        finder.close()


def check_against_fit(make_finder, make_model) -> None:
    """Identities with S8 that need no restatement: every star's eight sums and two counts are fit's, bit for bit, in a group or not; with
    max_group = 1, or a link below the smallest separation, every common column is."""
    for name in ("crowd, N = 9, mesh, flux and background", "masked crowd, none, flux alone", "max_group 1", "a link below every separation",
                 "a zero cell in a group", "a group across the rim"):
        c = case(name)
        finder, model_ = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"])
        try:
            finder.background_device(c["frame"], c["mask"])
            for radius in c["radii"]:
                args = (model_, c["positions"], c["cells"], radius, c["fit_background"], c["background"] == "mesh")
                single, group = finder.fit(*args), finder.fit_groups(*args, c["link"], c["max_group"])
                keep = [fc.Y, fc.X, fc.CELL, fc.N_USE, fc.N_ALL, *range(fc.SM, fc.SDD + 1)]
                assert same_bits(group[:, keep], single[:, keep]), (name, radius)
                alone = ~((group[:, GROUP_SIZE] >= 2) & (group[:, GROUP_SIZE] <= c["max_group"]))
                assert same_bits(group[alone, :fc.COLUMNS], single[alone]), (name, radius)
                if name in ("max_group 1", "a link below every separation"):
                    assert alone.all() and same_bits(group[:, :fc.COLUMNS], single)
                    assert np.all(group[:, GROUP_SIZE] == 1) == (name != "max_group 1")
                else:
                    assert not alone.all()
        finally:
            model_.close()
            finder.close()


def check_against_render(make_finder, make_model) -> None:
    """Identities with S10: without a mesh and without a fitted constant the float64 residual frame of the fitted fluxes holds every
    member's peak_e at (peak_row, peak_col), bit for bit, and the sum of its squares over a group's owned pixels is group_chi2."""
    c = case("crowd, N = 9, none, flux alone")
    positions, cells = c["positions"][:21], c["cells"][:21]  # without the pile, whose stars are fitted alone where their discs overlap
    finder, model_ = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"])
    try:
        finder.background_device(c["frame"], None)
        for radius in c["radii"]:
            got = finder.fit_groups(model_, positions, cells, radius, False, False, None, MAX_GROUP)
            assert np.all(got[:, fc.FLAGS] == 0) and np.all(got[:, fc.BG] == 0.0)
            residual, drawn = finder.render(model_, positions, got[:, fc.F], cells, radius, rn.RESIDUAL, np.float64)
            assert drawn == len(positions)
            at = (got[:, fc.PEAK_ROW].astype(int), got[:, fc.PEAK_COL].astype(int))
            assert same_bits(residual[at], got[:, fc.PEAK_E]), radius
            R2 = np.float64(radius) * np.float64(radius)
            for root in sorted(set(got[:, GROUP].astype(int).tolist())):
                members = np.flatnonzero(got[:, GROUP] == root)
                taken, boxes = np.zeros(SHAPE, bool), []
                for a in members:
                    y, x = positions[a]
                    rr = np.arange(int(np.floor(y - radius)) - 1, int(np.ceil(y + radius)) + 2)
                    cc = np.arange(int(np.floor(x - radius)) - 1, int(np.ceil(x + radius)) + 2)
                    pr, pc_ = rr.astype(np.float64) - y, cc.astype(np.float64) - x
                    disc = ((pr * pr)[:, None] + (pc_ * pc_)[None, :]) <= R2
                    on = ((rr >= 0) & (rr < SHAPE[0]))[:, None] & ((cc >= 0) & (cc < SHAPE[1]))[None, :]
                    ri, ci = np.clip(rr, 0, SHAPE[0] - 1)[:, None], np.clip(cc, 0, SHAPE[1] - 1)[None, :]
                    owned = disc & on & ~taken[ri, ci]
                    e = residual[ri, ci]
                    boxes.append(np.where(owned, e * e, 0.0))
                    rows_on, cols_on = (rr >= 0) & (rr < SHAPE[0]), (cc >= 0) & (cc < SHAPE[1])
                    taken[np.ix_(rr[rows_on], cc[cols_on])] |= disc[np.ix_(rows_on, cols_on)]
                assert same_bits(ordered_sum_boxes(boxes), got[root, GROUP_CHI2]), (radius, root)
    finally:
        model_.close()
        finder.close()


def check_against_lstsq(make_finder, make_model, names=None) -> float:
    """The restatement (and with it the kernel, which equals it) against an independent solve: numpy.linalg.lstsq on the explicit design
    matrix of every group.  The fluxes agree within p^2 cond(A^T A) 2^-52 of the group's largest |flux|; returns the largest share."""
    worst = 0.0
    for name in (tuple(CROWD_CASES) + tuple(MASKED_CASES)) if names is None else names:
        c = case(name)
        level_f, rows = run(make_finder, make_model, c)
        for radius, got in rows.items():
            _, designs = reference(name, level_f, radius, with_designs=True)
            for members, design in designs:
                if design["x"] is None:
                    continue
                g, p = len(members), len(design["rhs"])
                columns, data = [[] for _ in range(p)], []
                for a, box in enumerate(design["boxes"]):
                    counted = design["counted"][a]
                    data.append(box["d"][counted])
                    for b in range(g):
                        columns[b].append(np.where(box["inside"][b], box["m"][b], 0.0)[counted])
                    if p > g:
                        columns[g].append(np.ones(int(counted.sum())))
                M, d = np.stack([np.concatenate(col) for col in columns], axis=1), np.concatenate(data)
                assert len(d) == design["n"]
                independent = np.linalg.lstsq(M, d, rcond=None)[0]
                cond = np.linalg.cond(M.T @ M)
                bound = p * p * cond * 2.0 ** -52 * np.abs(independent[:g]).max()
                error = np.abs(got[members, fc.F] - independent[:g]).max()
                worst = max(worst, error / bound)
                assert error <= bound, (name, radius, members.tolist(), error, bound, cond)
    print(f"against numpy.linalg.lstsq: the largest flux error is {worst:.3g} of the bound p^2 cond(A^T A) 2^-52 max |flux|")
    return worst


def check_reproducible(make_finder, make_model, name: str) -> None:
    """Repeats are bit-equal: on a fresh finder and model, by a second call on the same frame, and with other calls in between."""
    c = case(name)
    radius = c["radii"][-1]
    rows = run(make_finder, make_model, c)[1][radius]
    assert run(make_finder, make_model, c)[1][radius].tobytes() == rows.tobytes()
    finder, model_, other_model = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"]), make_model(fc.model(16))
    try:
        finder.background_device(c["frame"], c["mask"])
        args = (model_, c["positions"], c["cells"], radius, c["fit_background"], c["background"] == "mesh", c["link"], c["max_group"])
        one = finder.fit_groups(*args)
        other = finder.fit_groups(other_model, c["positions"][::-1], c["cells"], 6.5, not c["fit_background"], False, 3.0, 3)
        finder.fit(model_, c["positions"], c["cells"], radius)
        two = finder.fit_groups(*args)
        assert one.tobytes() == two.tobytes() == rows.tobytes() and other.shape == one.shape
    finally:
        model_.close()
        other_model.close()
        finder.close()


def check_isolation(make_finder, make_model) -> None:
    """detect, measure, photometry, refine, fit, fit_positions and render give the bits they gave before a group fit, a group fit's rows do
    not depend on them, and one model serves two finders."""
    c = case("crowd, N = 9, mesh, flux and background")
    radii = (2.0, 4.0)
    finder, model_ = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"])
    other = make_finder((40, 56), 8)
    try:
        finder.background_device(c["frame"], c["mask"])
        rows = finder.detect_device(3.0, 5, None)
        shapes = finder.measure()
        phot = finder.photometry(rows[:, :2], radii, 5, True)
        refined = finder.refine(rows[:, :2], 1.5)
        cells = np.zeros(len(rows), np.int32)
        fits = finder.fit(model_, rows[:, :2], cells, 3.5)
        steps, moved = finder.fit_positions(model_, rows[:, :2], cells, 3.5)
        drawn = finder.render(model_, rows[:, :2], fits[:, fc.F], cells, 3.5, rn.RESIDUAL, np.float64)[0]
        args = (model_, c["positions"], c["cells"], 2.3, True, True, CROWD_LINK, MAX_GROUP)
        groups = finder.fit_groups(*args)
        assert finder.measure().tobytes() == shapes.tobytes()
        assert finder.photometry(rows[:, :2], radii, 5, True).tobytes() == phot.tobytes()
        assert finder.refine(rows[:, :2], 1.5).tobytes() == refined.tobytes()
        assert finder.fit(model_, rows[:, :2], cells, 3.5).tobytes() == fits.tobytes()
        again = finder.fit_positions(model_, rows[:, :2], cells, 3.5)
        assert again[0].tobytes() == steps.tobytes() and again[1].tobytes() == moved.tobytes()
        assert finder.render(model_, rows[:, :2], fits[:, fc.F], cells, 3.5, rn.RESIDUAL, np.float64)[0].tobytes() == drawn.tobytes()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes()
        assert finder.fit_groups(*args).tobytes() == groups.tobytes()
        other.background_device(np.ascontiguousarray(c["frame"][:40, :40].repeat(2, axis=1)[:, :56]), None)
        assert other.fit_groups(model_, c["positions"], c["cells"], 2.3, True, True, CROWD_LINK, 4).shape == groups.shape
        assert finder.fit_groups(*args).tobytes() == groups.tobytes()
        finder.background_device(c["frame"], c["mask"])  # the group fit first, the others after it
        assert finder.fit_groups(*args).tobytes() == groups.tobytes()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes() and finder.measure().tobytes() == shapes.tobytes()
        assert finder.fit(model_, rows[:, :2], cells, 3.5).tobytes() == fits.tobytes()
    finally:
        model_.close()
        other.close()
        finder.close()


def check_errors(make_finder, make_model, error: type) -> None:
    """RPSF_E_STATE (-6) before a background_device of a frame; RPSF_E_BADARG (-1) for a bad radius, position, link or max_group, whatever
    the state."""
    import pytest

    c = case("crowd, N = 9, mesh, flux and background")
    p, k = c["positions"][:6], c["cells"][:6]
    finder, model_ = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"])
    good = (model_, p, k, 3.5, True, True, None, 8)
    bad = [(model_, p, k, 0.0, True, True, None, 8), (model_, p, k, np.nan, True, True, None, 8), (model_, p, k, 3.5000001, True, True, None, 8),
           (model_, [(np.nan, 1.0)], [0], 3.5, True, True, None, 8), (model_, [(2.0 ** 20, 1.0)], [0], 3.5, True, True, None, 8),
           (model_, p, k, 3.5, True, True, 0.0, 8), (model_, p, k, 3.5, True, True, -1.0, 8), (model_, p, k, 3.5, True, True, np.nan, 8),
           (model_, p, k, 3.5, True, True, np.inf, 8), (model_, p, k, 3.5, True, True, np.nextafter(7.0, 8.0), 8),
           (model_, p, k, 3.5, True, True, None, 0), (model_, p, k, 3.5, True, True, None, 9), (model_, p, k, 3.5, True, True, None, -1)]
    try:
        def refused(args, code):
            with pytest.raises(error) as caught:
                finder.fit_groups(*args)
            assert caught.value.code == code, (args[3:], caught.value.code)

        refused(good, -6)
        for args in bad:
            refused(args, -1)
        finder.background(c["frame"], c["mask"])  # the host route: no S1b mesh on the device
        refused(good, -6)
        finder.background_device(c["frame"], c["mask"])
        for args in bad:
            refused(args, -1)
        rows = finder.fit_groups(*good)
        assert finder.fit_groups(model_, p, k, 3.5, True, True, 7.0, 1).shape == (6, COLUMNS)  # the largest link, the smallest group
        assert finder.fit_groups(model_, p, k, 3.5, True, True, 2.0 ** -30, 8).shape == (6, COLUMNS)
        assert finder.fit_groups(model_, p, np.array([-2 ** 31, 2 ** 31 - 1, 4, -1, 0, 3]), 2.0 ** -20, True, True).shape == (6, COLUMNS)
        assert finder.fit_groups(*good).tobytes() == rows.tobytes()
    finally:
        model_.close()
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ the truth
# Three 64 x 64 noise-free frames built as fit_cases.truth_case builds its own (Gaussians of sigma 1.5 on a flat background of 10, rounded
# to float32): each holds four pairs, 2, 3, 4.5 and 7 px apart, one in each quadrant at a random sub-pixel position and angle; the brighter
# star of a pair has amplitude 1000 and the other 1000 / ratio, with ratio 1 in the first frame, 3 in the second and 10 in the third.  The
# model is fit_cases.oracle_model(), every star pointed at one finite cell of it (TRUTH_CELL) through cells=, R = 5, flux and background,
# background="none".  Per star flux_iso is the restatement's fit_stars flux of that star rendered alone on the same background.
# MEASURED_GROUP_ERROR is the median |flux / flux_iso - 1| of the restatement's group fit, on the CPU; the asserted bound is that times
# TRUTH_MARGIN = 2, as in fit_cases.  The single-star fit of the blended frame is worse by MEASURED_SINGLE_FACTOR; a third of that is asked
# (SINGLE_FACTOR), after the practice of fit_cases.DISPLACED_FACTOR: the figure is there to show that the joint fit matters, not to pin it.
TRUTH_SEPARATIONS, TRUTH_RATIOS = (2.0, 3.0, 4.5, 7.0), (1.0, 3.0, 10.0)
MEASURED_GROUP_ERROR = 0.00996  # the median of 24 stars; the single-star fit of the same frames: 0.1204
MEASURED_SINGLE_FACTOR = 12.1
TRUTH_MARGIN = fc.TRUTH_MARGIN


@functools.cache
def truth_case() -> dict:
    rng = np.random.default_rng([13, 67])
    shape = fc.TRUTH_SHAPE
    rows, cols = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    star = lambda r, c, amplitude: amplitude * np.exp(-0.5 * ((rows - r) ** 2 + (cols - c) ** 2) / fc.TRUTH_SIGMA ** 2)
    frames, truth, alone = [], [], []
    for ratio in TRUTH_RATIOS:
        frame, pos, single = np.full(shape, 10.0), [], []
        for separation, centre in zip(TRUTH_SEPARATIONS, ((16.0, 16.0), (16.0, 48.0), (48.0, 16.0), (48.0, 48.0))):
            middle, angle = np.array(centre) + rng.uniform(-0.5, 0.5, 2), rng.uniform(0.0, 2.0 * np.pi)
            half = 0.5 * separation * np.array([np.sin(angle), np.cos(angle)])
            for (r, c), amplitude in ((middle - half, 1000.0), (middle + half, 1000.0 / ratio)):
                frame += star(r, c, amplitude)
                pos.append((r, c))
                single.append((np.full(shape, 10.0) + star(r, c, amplitude)).astype(np.float32).astype(np.float64))
        frames.append(frame.astype(np.float32).astype(np.float64))
        truth.append(np.array(pos))
        alone.append(single)
    return sc._freeze({"frames": np.stack(frames), "truth": truth, "alone": alone})


@functools.cache
def truth_cell() -> int:
    """The first cell of the oracle's model that is all finite and not all zero."""
    values = fc.oracle_model()[1]
    return int(np.flatnonzero(np.isfinite(values).all(axis=(1, 2)) & (np.abs(values).sum(axis=(1, 2)) > 0))[0])


@functools.cache
def truth_flux_iso() -> list[np.ndarray]:
    values, k = fc.oracle_model()[1], truth_cell()
    t = truth_case()
    return [np.array([fc.ref_fit(single, None, BOX, None, values, [p], [k], fc.TRUTH_RADIUS, True, "none")[0, fc.F] for single, p in zip(alone, pos)])
            for alone, pos in zip(t["alone"], t["truth"])]


def truth_errors(fluxes) -> float:
    """The median |flux / flux_iso - 1| over the stars of the three frames."""
    return float(np.median(np.abs(np.concatenate([np.asarray(f) for f in fluxes]) / np.concatenate(truth_flux_iso()) - 1.0)))


@functools.cache
def truth_restated() -> tuple[float, float]:
    """On the restatement alone: the group fit's median error and the single-star fit's."""
    values, k = fc.oracle_model()[1], truth_cell()
    t = truth_case()
    joint, single = [], []
    for frame, pos in zip(t["frames"], t["truth"]):
        cells = np.full(len(pos), k)
        rows = ref_fit_groups(frame, None, BOX, None, values, pos, cells, fc.TRUTH_RADIUS, True, "none")
        assert np.all(rows[:, fc.FLAGS] == 0) and np.all(rows[:, GROUP_SIZE] == 2)
        joint.append(rows[:, fc.F])
        single.append(fc.ref_fit(frame, None, BOX, None, values, pos, cells, fc.TRUTH_RADIUS, True, "none")[:, fc.F])
    return truth_errors(joint), truth_errors(single)


def check_truth(fit_groups=None, fit_stars=None, what="the restatement") -> tuple[float, float]:
    """The group fit recovers the fluxes the stars have alone; the single-star fit of the blended frame does not.  Without arguments the
    restatement itself; with ``fit_groups`` and ``fit_stars`` (the public functions) what they give."""
    from regularizepsf_amd import util

    restated, restated_single = truth_restated()
    if fit_groups is None:
        error, single = restated, restated_single
    else:
        t = truth_case()
        coordinates, values = fc.oracle_model()
        psf = util.IndexedCube(coordinates, values)
        cells = [np.full(len(p), truth_cell()) for p in t["truth"]]
        options = dict(background="none", box=BOX, cells=cells)
        got = fit_groups(t["frames"], t["truth"], psf, fc.TRUTH_RADIUS, **options)
        assert all(np.all(g["flags"] == 0) and np.all(g["group_size"] == 2) for g in got)
        error = truth_errors([g["flux"] for g in got])
        single = truth_errors([g["flux"] for g in fit_stars(t["frames"], t["truth"], psf, fc.TRUTH_RADIUS, **options)])
    factor = single / error
    print(f"truth, {what}: {sum(len(p) for p in truth_case()['truth'])} stars in pairs {TRUTH_SEPARATIONS} px apart, flux ratios {TRUTH_RATIOS}: median "
          f"|flux / flux_iso - 1| of the group fit {error:.4g} (measured {MEASURED_GROUP_ERROR}, at most {TRUTH_MARGIN:g} times that asked), of the "
          f"single-star fit {single:.4g}, worse by {factor:.1f} (measured {MEASURED_SINGLE_FACTOR}, at least {SINGLE_FACTOR:.3g} asked)")
    assert error <= TRUTH_MARGIN * MEASURED_GROUP_ERROR
    assert factor >= SINGLE_FACTOR
    return error, factor


SINGLE_FACTOR = MEASURED_SINGLE_FACTOR / 3.0
