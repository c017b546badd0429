"""The star finder's definition restated in float64 NumPy / SciPy, seeded frames, the CPU emulator of its kernels, and the checks
the emulator tests (tests/test_stars_host.py) and the GPU tests (tests/test_gpu_stars.py) share.

The detector is defined by this project, so there is no outside implementation to compare with: the reference is
the restatement below, written from the definition with array operations only (np.median, np.mean, scipy.ndimage.median_filter,
scipy.ndimage.label), and computed once per case.  Every frame is rounded to float32 before anybody sees it, as the library
uploads it.  A check takes `make_finder(shape, box)`: regularizepsf_amd.stars._Finder on the GPU, EmuFinder here.
"""

from __future__ import annotations

import functools
import pathlib

import numpy as np

from tests import emulib

ROOT = pathlib.Path(__file__).resolve().parent.parent
EIGHT = np.ones((3, 3), int)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def ref_box(values: np.ndarray) -> tuple[float, float, float]:
    """One background box: (level, rms, gap).  `gap` is the smallest distance, in units of sd, between any sample and a clip
    boundary in any round, and between |mean - med| and 0.3 sd at the end: how far the box is from a decision that hangs on rounding."""
    v = np.asarray(values, np.float64)
    if v.size == 0:
        return np.nan, np.nan, np.inf
    gap = np.inf
    for clip_round in range(17):
        med, mean = np.median(v), np.mean(v)
        sd = np.sqrt(np.mean((v - mean) ** 2))
        if clip_round == 16 or sd == 0:
            break
        dist = np.abs(v - med)
        gap = min(gap, float(np.min(np.abs(dist - 3 * sd)) / sd))
        keep = dist <= 3 * sd
        if keep.all():
            break
        v = v[keep]
    if sd == 0:
        return med, sd, gap
    gap = min(gap, abs(abs(mean - med) - 0.3 * sd) / sd)
    return (med if abs(mean - med) >= 0.3 * sd else 2.5 * med - 1.5 * mean), sd, gap


def ref_mesh(frame: np.ndarray, mask: np.ndarray | None, box: int) -> tuple[np.ndarray, np.ndarray, float]:
    """The raw mesh (level, rms; NaN for a box without a usable pixel) and the smallest gap of ref_box over the boxes."""
    frame = np.asarray(frame, np.float32).astype(np.float64)
    ok = np.isfinite(frame) & (~mask if mask is not None else True)
    nby, nbx = -(-frame.shape[0] // box), -(-frame.shape[1] // box)
    level, rms, gap = np.empty((nby, nbx)), np.empty((nby, nbx)), np.inf
    for i in range(nby):
        for j in range(nbx):
            cut = (slice(i * box, (i + 1) * box), slice(j * box, (j + 1) * box))
            level[i, j], rms[i, j], g = ref_box(frame[cut][ok[cut]])
            gap = min(gap, g)
    return level, rms, gap


def ref_filter_mesh(level: np.ndarray, rms: np.ndarray):
    from scipy.ndimage import median_filter

    valid = np.isfinite(level)
    if not valid.any():
        return None
    level, rms = level.copy(), rms.copy()
    level[~valid], rms[~valid] = np.median(level[valid]), np.median(rms[valid])
    level, rms = median_filter(level, 3, mode="nearest"), median_filter(rms, 3, mode="nearest")
    return level, rms, float(np.median(rms))


def _axis(n: int, box: int, nb: int):
    u = np.clip((np.arange(n) + 0.5) / box - 0.5, 0, nb - 1)
    i0 = np.minimum(np.floor(u).astype(int), max(nb - 2, 0))
    t = u - i0 if nb > 1 else np.zeros(n)
    return i0, np.minimum(i0 + 1, nb - 1), t


def ref_surface(level: np.ndarray, shape: tuple[int, int], box: int) -> np.ndarray:
    i0, i1, t = _axis(shape[0], box, level.shape[0])
    j0, j1, s = _axis(shape[1], box, level.shape[1])
    t, s = t[:, None], s[None, :]
    return (1 - t) * ((1 - s) * level[i0][:, j0] + s * level[i0][:, j1]) + t * ((1 - s) * level[i1][:, j0] + s * level[i1][:, j1])


def ref_filter(d: np.ndarray) -> np.ndarray:
    p = np.pad(d, 1)
    h = (p[:, :-2] + 2 * p[:, 1:-1]) + p[:, 2:]
    return ((h[:-2] + 2 * h[1:-1]) + h[2:]) / 16


def ref_labels(detected: np.ndarray) -> np.ndarray:
    """scipy.ndimage.label with 8-connectivity, every label replaced by its component's smallest linear index; -1 off the mask."""
    from scipy.ndimage import label

    lab, _ = label(detected, EIGHT)
    flat = lab.ravel()
    _, first = np.unique(flat, return_index=True)  # first occurrence in raster order
    first = first if flat.min() == 0 else np.concatenate([[0], first])  # no background pixel: label 0 is absent
    out = first[flat]
    out[flat == 0] = -1
    return out.reshape(lab.shape).astype(np.int32)


def ref_detect(frame: np.ndarray, mask: np.ndarray | None, box: int, threshold: float = 3.0, min_area: int = 5,
               max_area: int | None = None) -> dict:
    """The whole definition.  rows: (k, 4) of (row, col, flux, area) in scipy.ndimage.label's order; per kept component also
    abs_flux = sum |d|; level: the filtered mesh; T; gap_clip and gap_threshold: the preconditions' figures."""
    from scipy.ndimage import label

    frame = np.asarray(frame, np.float32).astype(np.float64)
    ok = np.isfinite(frame) & (~mask if mask is not None else True)
    level, rms, gap_clip = ref_mesh(frame, mask, box)
    filtered = ref_filter_mesh(level, rms)
    empty = {"rows": np.zeros((0, 4)), "abs_flux": np.zeros(0), "gap_clip": gap_clip, "gap_threshold": np.inf, "raw": (level, rms), "components": 0}
    if filtered is None:
        return empty
    level_f, _, global_rms = filtered
    T = threshold * global_rms
    with np.errstate(invalid="ignore"):
        d = np.where(ok, frame - ref_surface(level_f, frame.shape, box), 0.0)
    f = ref_filter(d)
    detected = (f > T) & ok
    lab, n = label(detected, EIGHT)
    flat, rr, cc = lab.ravel(), *np.indices(frame.shape).reshape(2, -1)
    area = np.bincount(flat, minlength=n + 1)[1:]
    flux = np.bincount(flat, d.ravel(), minlength=n + 1)[1:]
    abs_flux = np.bincount(flat, np.abs(d).ravel(), minlength=n + 1)[1:]
    sr = np.bincount(flat, (d * rr.reshape(d.shape)).ravel(), minlength=n + 1)[1:]
    sc = np.bincount(flat, (d * cc.reshape(d.shape)).ravel(), minlength=n + 1)[1:]
    keep = (area >= min_area) & (flux > 0)
    if max_area is not None:
        keep &= area <= max_area
    with np.errstate(invalid="ignore", divide="ignore"):
        rows = np.stack([sr / flux, sc / flux, flux, area.astype(np.float64)], axis=-1)[keep]
    return {"rows": rows, "abs_flux": abs_flux[keep], "level": level_f, "T": T, "gap_clip": gap_clip, "raw": (level, rms),
            "gap_threshold": float(np.min(np.abs(f - T)) / abs(T)) if T != 0 else np.inf, "components": n}


# ------------------------------------------------------------------------------------------------------------------ the frames
# name: shape, box, stars, seed.  wide: short edge boxes of 22 rows and 8 columns; one_box: one box, the degenerate bilinear case
FRAMES = {
    "wide": {"shape": (150, 200), "box": 64, "stars": 20, "seed": 1},
    "one_box": {"shape": (64, 64), "box": 64, "stars": 4, "seed": 2},
    "tall": {"shape": (130, 70), "box": 32, "stars": 6, "seed": 3},
}
TRUTH_TOLERANCE = 0.06  # pixels between a found position and the Gaussian's centre


def star_frame(shape: tuple[int, int], pos: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    """A gently tilted background, noise of 0.3, and one Gaussian star of amplitude 100 ... 400 and sigma 1.1 ... 1.5 per position,
    rounded to float32 (returned as float64)."""
    h, w = shape
    rows, cols = np.mgrid[0:h, 0:w].astype(np.float64)
    amp = rng.uniform(100, 400, len(pos))
    sig_r, sig_c = rng.uniform(1.1, 1.5, len(pos)), rng.uniform(1.1, 1.5, len(pos))
    frame = 10.0 + 0.004 * rows - 0.003 * cols + rng.normal(0.0, 0.3, (h, w))
    for (r, c), a, sr, sc in zip(pos, amp, sig_r, sig_c):
        frame += a * np.exp(-0.5 * (((rows - r) / sr) ** 2 + ((cols - c) / sc) ** 2))
    return frame.astype(np.float32).astype(np.float64)


def scattered(shape: tuple[int, int], count: int, rng: np.random.Generator, margin: float = 10.0, apart: float = 14.0) -> np.ndarray:
    """`count` positions at least `margin` from every edge and `apart` from one another."""
    pos: list[np.ndarray] = []
    while len(pos) < count:
        p = np.array([rng.uniform(margin, shape[0] - 1 - margin), rng.uniform(margin, shape[1] - 1 - margin)])
        if all(np.hypot(*(p - q)) >= apart for q in pos):
            pos.append(p)
    return np.array(pos).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def frame_case(name: str, seed_offset: int = 0) -> dict:
    """A frame of FRAMES with its true star positions and the restatement's answer (shared; do not modify)."""
    spec = FRAMES[name]
    rng = np.random.default_rng([spec["seed"] + seed_offset, 37])
    truth = scattered(spec["shape"], spec["stars"], rng)
    frame = star_frame(spec["shape"], truth, rng)
    return _freeze({"frame": frame, "truth": truth, "box": spec["box"], "mask": None, "ref": ref_detect(frame, None, spec["box"])})


@functools.lru_cache(maxsize=None)
def masked_case() -> dict:
    """The wide frame with one whole box masked, one star (`hidden`) under a mask of its own, and NaN, +Inf and -Inf pixels (one of them
    on another star's centre)."""
    base = frame_case("wide")
    frame, mask = base["frame"].copy(), np.zeros(base["frame"].shape, bool)
    mask[64:128, 64:128] = True
    clear = [k for k, (r, c) in enumerate(base["truth"]) if not (50 <= r < 142 and 50 <= c < 142)]  # stars well away from that box
    hidden, pierced = clear[0], clear[1]
    r, c = np.rint(base["truth"][hidden]).astype(int)
    mask[r - 10:r + 11, c - 10:c + 11] = True
    r, c = np.rint(base["truth"][pierced]).astype(int)
    frame[r, c] = np.nan
    frame[3, 5], frame[140, 190], frame[20, 150] = np.inf, -np.inf, np.nan
    return _freeze({"frame": frame, "truth": base["truth"], "box": 64, "mask": mask, "hidden": hidden, "ref": ref_detect(frame, mask, 64)})


@functools.lru_cache(maxsize=None)
def edge_case() -> dict:
    """Stars centred (within half a pixel) on a frame corner, on the left edge and on the top edge, and one inside."""
    shape, box = (64, 80), 32
    rng = np.random.default_rng(64)
    truth = np.array([(0.2, 0.3), (30.4, 0.1), (0.3, 50.2), (40.3, 40.6)])
    frame = star_frame(shape, truth, rng)
    return _freeze({"frame": frame, "truth": truth, "box": box, "mask": None, "ref": ref_detect(frame, None, box)})


@functools.lru_cache(maxsize=None)
def background_case() -> dict:
    shape, box = (70, 90), 32
    frame = star_frame(shape, np.zeros((0, 2)), np.random.default_rng(7))
    return _freeze({"frame": frame, "truth": np.zeros((0, 2)), "box": box, "mask": None, "ref": ref_detect(frame, None, box)})


def _freeze(out: dict) -> dict:
    for v in list(out.values()) + list(out.get("ref", {}).values()):
        for a in (v if isinstance(v, tuple) else [v]):
            if isinstance(a, np.ndarray):
                a.flags.writeable = False
    return out


CASES = {"wide": lambda: frame_case("wide"), "one_box": lambda: frame_case("one_box"), "tall": lambda: frame_case("tall"),
         "masked": masked_case, "edge": edge_case}


# ------------------------------------------------------------------------------------------------------------------ the emulator
@functools.cache
def emulator():
    """tests/emu/libemu_stars.so: the kernels' drivers on the CPU.  __graft_entry__.build() compiles it; it is compiled here when it
    is missing or older than its sources.  Without a compiler that is an error, not a skip."""
    import ctypes
    lib = emulib.library("emu_stars")
    vp, i, d, n = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_long
    lib.emus_info.argtypes = [vp, vp]
    lib.emus_background.argtypes = [vp, vp, i, i, i, vp, vp]
    lib.emus_label.argtypes = [vp, i, i, vp]
    lib.emus_detect.argtypes = [vp, vp, i, i, i, vp, d, n, n, vp, n, vp]
    return lib


class EmuFinder:
    """regularizepsf_amd.stars._Finder's interface on the emulator."""

    def __init__(self, shape: tuple[int, int], box: int, device: int = 0) -> None:  # noqa: ARG002
        self.shape, self.box = (int(shape[0]), int(shape[1])), int(box)
        self.mesh_shape = (-(-self.shape[0] // self.box), -(-self.shape[1] // self.box))
        self._frame = self._mask = None

    def background(self, frame, mask):
        assert frame.shape == self.shape
        self._frame = np.ascontiguousarray(frame, np.float32)
        self._mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        level, rms = np.empty(self.mesh_shape), np.empty(self.mesh_shape)
        assert emulator().emus_background(self._frame.ctypes.data, None if self._mask is None else self._mask.ctypes.data, *self.shape,
                                          self.box, level.ctypes.data, rms.ctypes.data) == 0
        return level, rms

    def detect(self, level, threshold_abs, min_area, max_area):
        import ctypes

        level = np.ascontiguousarray(level, np.float64)
        capacity = self.shape[0] * self.shape[1]
        out, count = np.empty((capacity, 4)), ctypes.c_long(0)
        assert emulator().emus_detect(self._frame.ctypes.data, None if self._mask is None else self._mask.ctypes.data, *self.shape, self.box,
                                      level.ctypes.data, float(threshold_abs), int(min_area), -1 if max_area is None else int(max_area),
                                      out.ctypes.data, capacity, ctypes.byref(count)) == 0
        return out[:count.value].copy()

    def label(self, detected):
        flags = np.ascontiguousarray(detected, np.uint8)
        labels = np.empty(self.shape, np.int32)
        assert emulator().emus_label(flags.ctypes.data, *self.shape, labels.ctypes.data) == 0
        return labels

    def info(self):
        import ctypes

        rows, cols = ctypes.c_int(0), ctypes.c_int(0)
        emulator().emus_info(ctypes.byref(rows), ctypes.byref(cols))
        return rows.value, cols.value

    def close(self) -> None:
        pass


# ------------------------------------------------------------------------------------------------------------------ labelling
def label_masks(tr: int, tc: int) -> dict[str, np.ndarray]:
    """The masks of the labelling test for a kernel tile of tr x tc: a frame of (2 tr + 3) x (2 tc + 5), where four tiles meet and
    both far edges are partial, and the degenerate frames."""
    h, w = 2 * tr + 3, 2 * tc + 5
    rows, cols = np.indices((h, w))
    out: dict[str, np.ndarray] = {}
    corners = np.zeros((h, w), bool)
    for r0 in range(0, h, tr):
        for c0 in range(0, w, tc):
            r1, c1 = min(r0 + tr, h) - 1, min(c0 + tc, w) - 1
            corners[[r0, r0, r1, r1], [c0, c1, c0, c1]] = True
    out["tile corners"] = corners
    for name, pixels in (("diagonal link", [(tr - 3, tc - 3), (tr - 2, tc - 2), (tr - 1, tc - 1), (tr, tc), (tr + 1, tc + 1)]),
                         ("anti-diagonal link", [(tr - 2, tc + 1), (tr - 1, tc), (tr, tc - 1), (tr + 1, tc - 2)])):
        m = np.zeros((h, w), bool)
        m[tuple(zip(*pixels))] = True
        out[name] = m
    out["horizontal lines"] = np.isin(rows, (5, tr + 8, 2 * tr + 1))
    out["vertical lines"] = np.isin(cols, (7, tc + 4, 2 * tc + 3))
    serpentine = rows % 2 == 0
    serpentine |= (rows % 4 == 1) & (cols == w - 1)
    serpentine |= (rows % 4 == 3) & (cols == 0)
    out["serpentine"] = serpentine
    out["checkerboard"] = (rows + cols) % 2 == 0
    out["sparse checkerboard"] = ((rows + cols) % 2 == 0) & (rows % 2 == 0)
    out["all true"], out["all false"] = np.ones((h, w), bool), np.zeros((h, w), bool)
    for density in (0.3, 0.5, 0.6):
        for seed in (1, 2, 3):
            out[f"random {density} seed {seed}"] = np.random.default_rng([seed, int(density * 10)]).random((h, w)) < density
    for shape in ((1, 1), (1, w), (h, 1), (tr - 5, tc - 3)):
        out[f"{shape} all true"] = np.ones(shape, bool)
        out[f"{shape} random"] = np.random.default_rng(shape).random(shape) < 0.5
    return out


def check_labels(make_finder) -> None:
    """Every mask of label_masks: exactly scipy.ndimage.label's components, each labelled with its smallest linear index."""
    probe = make_finder((1, 1), 64)
    tr, tc = probe.info()
    probe.close()
    finders: dict[tuple[int, int], object] = {}
    for name, mask in label_masks(tr, tc).items():
        finder = finders.get(mask.shape) or finders.setdefault(mask.shape, make_finder(mask.shape, 64))
        got = finder.label(mask)
        want = ref_labels(mask)
        assert got.dtype == np.int32 and got.shape == want.shape
        assert np.array_equal(got, want), f"{name}: {np.count_nonzero(got != want)} of {mask.size} labels differ"
    for finder in finders.values():
        finder.close()
    serpentine = ref_labels(label_masks(tr, tc)["serpentine"])
    assert np.unique(serpentine).tolist() == [-1, 0]  # the mask is one component, as intended


# ------------------------------------------------------------------------------------------------------------------ mesh
MESH_TOLERANCE = 1e-12  # relative: the median is exact, the sums are float64 over at most 16 384 terms in a fixed tree order
GAP_CLIP = 1e-6  # in units of sd
GAP_THRESHOLD = 1e-6  # relative to T


def check_mesh(make_finder, name: str) -> None:
    case = CASES[name]()
    want_level, want_rms = case["ref"]["raw"]
    assert case["ref"]["gap_clip"] >= GAP_CLIP, f"{name}: a sample lies {case['ref']['gap_clip']:.1e} sd from a clip boundary"
    finder = make_finder(case["frame"].shape, case["box"])
    level, rms = finder.background(case["frame"], case["mask"])
    finder.close()
    assert np.array_equal(np.isnan(level), np.isnan(want_level)) and np.array_equal(np.isnan(rms), np.isnan(want_rms))
    if name == "masked":
        assert np.isnan(want_level[1, 1]) and np.isnan(want_level).sum() == 1
    ok = ~np.isnan(want_level)
    err_level = np.max(np.abs(level[ok] - want_level[ok]) / np.abs(want_level[ok]))
    err_rms = np.max(np.abs(rms[ok] - want_rms[ok]) / np.abs(want_rms[ok]))
    print(f"{name}: mesh {level.shape}, clip gap {case['ref']['gap_clip']:.1e} sd, relative error level {err_level:.1e}, rms {err_rms:.1e}")
    assert err_level <= MESH_TOLERANCE and err_rms <= MESH_TOLERANCE


# ------------------------------------------------------------------------------------------------------------------ detection
def run(make_finder, case: dict, threshold: float = 3.0, min_area: int = 5, max_area: int | None = None) -> np.ndarray:
    """The product's per-frame pipeline (background, host mesh filter, detect) on a finder: (k, 4) rows."""
    from regularizepsf_amd import stars

    finder = make_finder(case["frame"].shape, case["box"])
    try:
        return stars.frame_stars(finder, case["frame"], case["mask"], threshold, min_area, max_area)
    finally:
        finder.close()


def compare_rows(got: np.ndarray, ref: dict, shape: tuple[int, int], what: str) -> None:
    """Count, order and areas equal; positions within 8 area 2^-53 (sum |d| / sum d) max(H, W) pixels, the flux within the same
    number of roundings of sum |d|."""
    want = ref["rows"]
    assert got.shape == want.shape, f"{what}: {len(got)} detections, the restatement has {len(want)}"
    assert np.array_equal(got[:, 3], want[:, 3]), f"{what}: areas or order differ"
    if len(want) == 0:
        return
    eps = 8 * want[:, 3] * 2.0 ** -53
    bound = eps * (ref["abs_flux"] / want[:, 2]) * max(shape)
    err = np.abs(got[:, :2] - want[:, :2]).max(axis=1)
    print(f"{what}: {len(want)} components, areas {int(want[:, 3].min())} ... {int(want[:, 3].max())}, sum|d|/sum d <= "
          f"{np.max(ref['abs_flux'] / want[:, 2]):.3f}, max position error {err.max():.2e} px (bound {bound.min():.2e} ... {bound.max():.2e})")
    assert np.all(err <= bound), what
    assert np.all(np.abs(got[:, 2] - want[:, 2]) <= eps * ref["abs_flux"]), what


def check_detect(make_finder, name: str) -> None:
    case = CASES[name]()
    ref = case["ref"]
    assert ref["gap_clip"] >= GAP_CLIP and ref["gap_threshold"] >= GAP_THRESHOLD, (ref["gap_clip"], ref["gap_threshold"])
    print(f"{name}: min |f - T| / T = {ref['gap_threshold']:.1e}")
    compare_rows(run(make_finder, case), ref, case["frame"].shape, name)


def check_truth(name: str) -> None:
    """The definition itself: on the seeded frames the restatement finds exactly the generator's stars."""
    case = frame_case(name)
    rows, truth = case["ref"]["rows"], case["truth"]
    assert len(rows) == len(truth) == FRAMES[name]["stars"]
    dist = np.hypot(*(rows[:, None, :2] - truth[None, :, :]).transpose(2, 0, 1))
    assert sorted(dist.argmin(axis=1).tolist()) == list(range(len(truth)))  # one detection per star
    print(f"{name}: {len(truth)} stars, worst distance to the truth {dist.min(axis=1).max():.3f} px")
    assert dist.min(axis=1).max() <= TRUTH_TOLERANCE


def check_area_limits(make_finder, name: str) -> None:
    """min_area just above the smallest area drops exactly that component, max_area just below the largest likewise."""
    case = frame_case(name)
    rows = case["ref"]["rows"]
    areas = rows[:, 3]
    small, large = int(areas.min()), int(areas.max())
    assert small >= 5 and small < large
    same = run(make_finder, case, min_area=small, max_area=large)
    assert np.array_equal(same[:, 3], areas)
    fewer = run(make_finder, case, min_area=small + 1)
    assert len(fewer) < len(same) and np.array_equal(fewer, same[areas > small])
    fewer = run(make_finder, case, max_area=large - 1)
    assert len(fewer) < len(same) and np.array_equal(fewer, same[areas < large])


def check_special_frames(make_finder) -> None:
    """A masked star is not found; pure background gives nothing; a frame that is one component returns and is dropped by max_area."""
    case = masked_case()
    rows = run(make_finder, case)
    compare_rows(rows, case["ref"], case["frame"].shape, "masked")
    assert 0 < len(rows) < len(case["truth"])
    assert np.hypot(*(rows[:, :2] - case["truth"][case["hidden"]]).T).min() > 10
    case = background_case()
    assert case["ref"]["components"] == 0 and case["ref"]["rows"].shape == (0, 4)
    assert run(make_finder, case).shape == (0, 4)
    case = frame_case("tall")
    npix = case["frame"].size
    ref = ref_detect(case["frame"], None, case["box"], threshold=-1000.0)
    assert ref["components"] == 1 and ref["gap_threshold"] >= GAP_THRESHOLD
    assert run(make_finder, case, threshold=-1000.0, max_area=npix - 1).shape == (0, 4)
    whole = run(make_finder, case, threshold=-1000.0, max_area=npix)
    full = ref_detect(case["frame"], None, case["box"], threshold=-1000.0, max_area=npix)
    assert len(full["rows"]) == 1 and full["rows"][0, 3] == npix and full["rows"][0, 2] > 1e-3 * full["abs_flux"][0]  # clearly positive flux
    compare_rows(whole, full, case["frame"].shape, "one component")


def check_reproducible(make_finder, name: str) -> None:
    """Two runs agree bit for bit, and float64 input equals its float32 rounding."""
    case = frame_case(name)
    first, second = run(make_finder, case), run(make_finder, case)
    assert first.tobytes() == second.tobytes()
    rng = np.random.default_rng(5)
    wide = case["frame"] * (1 + 1e-9 * rng.standard_normal(case["frame"].shape))  # float64 values that are not float32 values
    assert not np.array_equal(wide, wide.astype(np.float32))
    a = run(make_finder, {**case, "frame": wide})
    b = run(make_finder, {**case, "frame": wide.astype(np.float32)})
    assert len(a) > 0 and a.tobytes() == b.tobytes()
