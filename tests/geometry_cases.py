"""The apply geometry contract (rpsf_geometry, include/rpsf.h): the case table of tests/test_gpu_geometry.py and its float64 reference.

NumPy and the oracle only; the band planner of regularizepsf_amd/sharding.py (NumPy too) supplies the row windows.  A case is: apply path, patch
size, frame shape, pad mode, a view of the input and one of the output (byte offset of the pointer into its allocation + row stride), an origin, a
pad value, a row window, and for a batch the frame count and the kind of frame stride.  Everything the library's predicates look at
(`hot_geometry`, `fused`, `aligned_in` / `aligned_out`, `quads_aligned`, `pairs_aligned`, the tile sums) is a plain arithmetic fact of those
numbers: `facts(case)` states them, and tests/test_geometry_cases.py asserts that every path has a case on each side of every fact.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from oracle import regpsf_oracle as orc
from tests.helpers import KERNEL_PAD_MODES, random_transfer

PAD_CODES = {"constant": 0, "symmetric": 1, "reflect": 2, "edge": 3, "wrap": 4}  # RPSF_PAD_* of include/rpsf.h

#: path -> patch sizes, overlap mode to force (None: what the plan selects by itself), launch options to pin
PATHS = {
    "sweep": {"sizes": (16, 32, 64), "overlap": None, "options": {}},           # auto on a complete covering
    "planes1": {"sizes": (16, 32, 64), "overlap": "planes", "options": {}},     # first-generation patch kernel + separate plane sum
    "atomic": {"sizes": (32, 128), "overlap": "atomic", "options": {}},
    "gen2_sum": {"sizes": (128, 256), "overlap": None, "options": {"persist": 0, "fuse": 0}},    # one patch per workgroup, separate sum
    "gen2_fused": {"sizes": (128, 256), "overlap": None, "options": {"persist": 0, "fuse": 1}},  # plane sum inside the patch launch
    "gen2_persistent": {"sizes": (128, 256), "overlap": None, "options": {}},                    # the defaults
    "direct": {"sizes": (128,), "overlap": "direct", "options": {}},
    "fallback": {"sizes": (24, 9), "overlap": None, "options": {}},             # generic plan: hipFFT, colour classes on a covering
}
#: paths whose additions run in a fixed order: an aligned and an unaligned load of one pixel must give the same bits
ORDERED_PATHS = tuple(p for p in PATHS if p != "atomic")

#: patch size -> frame shapes; the first has a width that is a multiple of 4 (of 32 except at N = 24: 120 = 8 x 15), the last one that is not
SHAPES = {
    16: ((40, 64), (40, 50)),
    32: ((96, 128), (70, 90)),
    64: ((192, 256), (130, 201)),
    128: ((384, 256), (300, 262)),
    256: ((512, 608), (512, 768), (300, 521)),
    24: ((96, 120), (96, 121)),
    9: ((40, 33),),
}
#: view -> (byte offset of the pointer into its allocation, floats added to the width for the row stride)
VIEWS = {
    "A": (16, 4),  # alignment kept, pitch != width: a kernel that takes the width for the stride on its fast path
    "B": (8, 2),   # 8-byte units survive, 16-byte units do not
    "C": (4, 3),   # nothing is aligned
    "D": (0, 1),   # aligned base, every second row misaligned
}
DENSE = (0, 0)
#: the patch size whose first shape carries a path's origin, pad-value, window and batch cases
THIN_SIZE = {"sweep": 32, "planes1": 16, "atomic": 128, "gen2_sum": 256, "gen2_fused": 128, "gen2_persistent": 128, "direct": 128, "fallback": 24}
WINDOW_SIZE = {"sweep": 32, "planes1": 64, "atomic": 32, "gen2_sum": 128, "gen2_fused": 128, "gen2_persistent": 128, "direct": 128, "fallback": 24}
PAD_VALUES = (0.0, -7.25, 3e4)
BATCH_FRAMES = 3


def origins(n):
    return ((0, 0), (3, 5), (n // 2, 4), (-1, -3), (2 * n, 2 * n))


@dataclass(frozen=True)
class Case:
    path: str
    n: int
    shape: tuple            # of the frame the plan's corner list covers
    pad_mode: str = "symmetric"
    view_in: str | None = None   # key of VIEWS, None: dense
    view_out: str | None = None
    origin: tuple = (0, 0)
    pad_value: float = 0.0
    window: tuple | None = None  # (world, rank) of the band planner
    frames: int = 1
    strides: str | None = None   # batches: "odd" (rows x ld + 1 / + 3 floats) or "mult4"
    host_padded: bool = False    # the frame handed over is np.pad(frame, 2 N, pad_mode); goes with origin (2 N, 2 N)

    @property
    def frame_shape(self):
        pad = 4 * self.n if self.host_padded else 0
        return (self.shape[0] + pad, self.shape[1] + pad)

    @property
    def plan_key(self):
        return (self.path, self.n, self.shape, self.window)

    @property
    def name(self):
        parts = [self.path, f"N{self.n}", f"{self.shape[0]}x{self.shape[1]}", self.pad_mode, f"in{self.view_in or '-'}", f"out{self.view_out or '-'}"]
        if self.origin != (0, 0):
            parts.append(f"o{self.origin[0]}_{self.origin[1]}")
        if self.pad_value:
            parts.append(f"v{self.pad_value:g}")
        if self.window:
            parts.append(f"band{self.window[1]}of{self.window[0]}")
        if self.frames > 1:
            parts.append(f"{self.frames}f_{self.strides}")
        return "-".join(parts)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def transfer(n, shape):
    """(corner list of the covering of ``shape``, random complex64 K): what a plan of (N, shape) is made of."""
    return random_transfer(shape, n, 7000 + n + shape[0] * 31 + shape[1])


@functools.lru_cache(maxsize=None)
def base_frames(n, shape, frames):
    rng = np.random.default_rng(9000 + n + shape[0] * 17 + shape[1])
    return (rng.standard_normal((frames, *shape)) * 10 + 30).astype(np.float32)


@functools.lru_cache(maxsize=None)
def band(n, shape, world, rank):
    """Row band ``rank`` of ``world`` from the project's own planner; seam "recompute": the band runs every patch that reaches its rows, so its
    output window holds rows of the whole-frame result."""
    from regularizepsf_amd.sharding import make_band_plans

    return make_band_plans(transfer(n, shape)[0], n, shape[0], world, "symmetric", seam="recompute")[rank]


def plan_transfer(case):
    """(corner list, K) of the case's plan: the covering, or the band's patches in their original order."""
    coords, k = transfer(case.n, case.shape)
    if case.window is None:
        return coords, k
    index = band(case.n, case.shape, *case.window).patch_index
    return [coords[i] for i in index], k[index]


def frames_of(case):
    """The float32 frames the case hands over, (frames, height, width)."""
    frames = base_frames(case.n, case.shape, case.frames)
    if not case.host_padded:
        return frames
    p = 2 * case.n
    return np.stack([np.pad(f, p, mode=case.pad_mode) for f in frames])


# ---- the numbers of a case ------------------------------------------------------------------------------------------------------------------
def geometry_numbers(case):
    """Every number of the call: the fields of rpsf_geometry, the pointer offsets in bytes and the frame strides in floats (0: single apply)."""
    h, w = case.frame_shape
    off_in, extra_in = VIEWS[case.view_in] if case.view_in else DENSE
    off_out, extra_out = VIEWS[case.view_out] if case.view_out else DENSE
    g = {"height": h, "width": w, "pad_mode": PAD_CODES[case.pad_mode], "pad_value": case.pad_value, "origin_row": case.origin[0],
         "origin_col": case.origin[1], "image_row0": 0, "image_rows": h, "ld_image": w + extra_in, "out_row0": 0, "out_rows": h,
         "ld_out": w + extra_out, "offset_in": off_in, "offset_out": off_out, "image_stride": 0, "out_stride": 0}
    if case.window:
        b = band(case.n, case.shape, *case.window)
        g.update(image_row0=b.image_row0, image_rows=b.image_rows, out_row0=b.out_row0, out_rows=b.out_rows)
    if case.frames > 1:
        im, out = g["image_rows"] * g["ld_image"], g["out_rows"] * g["ld_out"]
        if case.strides == "odd":
            g.update(image_stride=im + 1, out_stride=out + 3)
        else:
            g.update(image_stride=(im + 7) // 4 * 4, out_stride=(out + 11) // 4 * 4)
    return g


def lattice_col0(case):
    return min(c for _, c in plan_transfer(case)[0])


def facts(case):
    """The library's path predicates as arithmetic facts of the case (True: the fast side of that term)."""
    g = geometry_numbers(case)
    c0 = lattice_col0(case) + g["origin_col"]
    return {
        "ld_image % 4": g["ld_image"] % 4 == 0, "ld_out % 4": g["ld_out"] % 4 == 0,
        "ld_image % 2": g["ld_image"] % 2 == 0, "ld_out % 2": g["ld_out"] % 2 == 0,
        "image offset % 16": g["offset_in"] % 16 == 0, "out offset % 16": g["offset_out"] % 16 == 0,
        "image offset % 8": g["offset_in"] % 8 == 0, "out offset % 8": g["offset_out"] % 8 == 0,
        "width % 4": g["width"] % 4 == 0, "width % 32": g["width"] % 32 == 0,
        "origin_col % 4": g["origin_col"] % 4 == 0,
        "(lat_c0 + origin_col) % 4": c0 % 4 == 0, "(lat_c0 + origin_col) % 32": c0 % 32 == 0,
        "image_stride % 4": g["image_stride"] % 4 == 0, "out_stride % 4": g["out_stride"] % 4 == 0,
    }


#: facts a path need not straddle.  Only the `fused` predicate of the second-generation plans asks for multiples of 32, and the fallback's sizes
#: offer none: 120 = 8 x 15 and 33 are the widths, -12 and -5 the lattice origins.
EXEMPT = {"fallback": ("width % 32", "(lat_c0 + origin_col) % 32")}


def admitted(case):
    """check_geometry's bounds, restated from include/rpsf.h: row strides at least the width; the resident windows inside the image; every corner
    plus the origin inside the 2 N-padded image, rows in [-2 N, height + N] and columns in [-2 N, width + N]; from the second frame of a
    batch on, a frame stride of at least (rows - 1) x ld + width."""
    g, n = geometry_numbers(case), case.n
    coords = plan_transfer(case)[0]
    rows = [r + g["origin_row"] for r, _ in coords]
    cols = [c + g["origin_col"] for _, c in coords]
    ok = g["ld_image"] >= g["width"] and g["ld_out"] >= g["width"]
    ok &= 0 <= g["image_row0"] and g["image_rows"] > 0 and g["image_row0"] + g["image_rows"] <= g["height"]
    ok &= 0 <= g["out_row0"] and g["out_rows"] > 0 and g["out_row0"] + g["out_rows"] <= g["height"]
    ok &= min(rows) >= -2 * n and max(rows) <= g["height"] + n and min(cols) >= -2 * n and max(cols) <= g["width"] + n
    if case.frames > 1:
        ok &= g["image_stride"] >= (g["image_rows"] - 1) * g["ld_image"] + g["width"]
        ok &= g["out_stride"] >= (g["out_rows"] - 1) * g["ld_out"] + g["width"]
    return bool(ok)


def refused(case):
    """The one refusal of an admitted geometry: the fallback takes whole-image geometry only (rpsf_plan_create's comment, launch_apply_generic)."""
    return case.path == "fallback" and case.window is not None


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------------
def reference_by_shift(image, coords, k, pad_mode, origin=(0, 0)):
    """View and origin: the oracle on the array the view denotes, every corner shifted by the origin."""
    return orc.apply_transfer(image, [(r + origin[0], c + origin[1]) for r, c in coords], k, pad_mode=pad_mode)


def reference_by_padding(image, coords, k, n, pad_value):
    """pad_value: the frame padded by 2 N with the value in NumPy, the oracle on it with every corner shifted by 2 N and 'constant', the crop.  No
    patch reads beyond 2 N, so the oracle's own (zero) padding is never seen."""
    p = 2 * n
    padded = np.pad(np.asarray(image, np.float64), p, mode="constant", constant_values=pad_value)
    out = orc.apply_transfer(padded, [(r + p, c + p) for r, c in coords], k, pad_mode="constant")
    return out[p : p + image.shape[0], p : p + image.shape[1]]


@functools.lru_cache(maxsize=None)
def _reference(n, shape, pad_mode, origin, pad_value, window, frames, host_padded):
    case = Case("sweep", n, shape, pad_mode, origin=origin, pad_value=pad_value, window=window, frames=frames, host_padded=host_padded)
    coords, k = plan_transfer(case)
    g = geometry_numbers(case)
    out = []
    for image in frames_of(case):
        if pad_mode == "constant" and pad_value != 0.0:
            assert origin == (0, 0)
            full = reference_by_padding(image, coords, k, n, pad_value)
        else:  # (a pad value under another mode must change nothing)
            full = reference_by_shift(image, coords, k, pad_mode, origin)
        out.append(full[g["out_row0"] : g["out_row0"] + g["out_rows"]])
    out = np.stack(out)
    out.setflags(write=False)
    return out


def reference(case):
    """float64 (frames, out_rows, width): computed once per distinct input, shared by every path and view, read-only."""
    return _reference(case.n, case.shape, case.pad_mode, case.origin, case.pad_value, case.window, case.frames, case.host_padded)


# ---- the table --------------------------------------------------------------------------------------------------------------------------------
def window_bands(n, shape):
    """(world, rank) of the bands of world 2 and 3 that start below the first image row on both sides."""
    picks = []
    for world in (2, 3):
        for rank in range(1, world):
            b = band(n, shape, world, rank)
            if b.image_row0 > 0 and b.out_row0 > 0:
                picks.append((world, rank))
    return picks


def _build():
    cases = []
    for path, spec in PATHS.items():
        # every view, on the input only, on the output only and on both, on every shape
        for n in spec["sizes"]:
            for shape in SHAPES[n]:
                for view in VIEWS:
                    cases += [Case(path, n, shape, view_in=view), Case(path, n, shape, view_out=view), Case(path, n, shape, view_in=view, view_out=view)]
        # origins x pad modes on one shape, dense views: the origin alone decides the path
        n = THIN_SIZE[path]
        shape = SHAPES[n][0]
        for pad_mode in KERNEL_PAD_MODES:
            for origin in origins(n):
                padded = origin == (2 * n, 2 * n)  # only a host-padded frame admits it
                cases.append(Case(path, n, shape, pad_mode, origin=origin, host_padded=padded))
        cases.append(Case(path, n, shape, "symmetric", view_in="C", view_out="B", origin=(3, 5)))  # an odd origin through unaligned views
        # pad values
        for value in PAD_VALUES:
            cases.append(Case(path, n, shape, "constant", pad_value=value))
        cases.append(Case(path, n, SHAPES[n][-1], "constant", view_in="C", view_out="C", pad_value=-7.25))
        cases.append(Case(path, n, shape, "symmetric", pad_value=-7.25))
        # batches: odd strides and multiples of 4, dense and through views
        for strides in ("odd", "mult4"):
            cases.append(Case(path, n, shape, frames=BATCH_FRAMES, strides=strides))
            cases.append(Case(path, n, shape, view_in="A", view_out="A", frames=BATCH_FRAMES, strides=strides))
        cases.append(Case(path, n, SHAPES[n][-1], view_in="C", view_out="C", frames=BATCH_FRAMES, strides="mult4"))
        # row windows with a pitch
        n = WINDOW_SIZE[path]
        shape = SHAPES[n][0]
        for window in window_bands(n, shape):
            for view in ("B", "C"):
                cases.append(Case(path, n, shape, view_in=view, view_out=view, window=window))
    cases = [c for c in dict.fromkeys(cases) if admitted(c)]  # (pad value 0 under 'constant' is also an origin case: once)
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _build()

#: what check_geometry must refuse before any launch: name -> changes to the numbers of a dense whole-frame call (N = 32, 96 x 128)
ERROR_CASE = Case("planes1", 32, (96, 128))
ERRORS = {
    "ld_image below the width": {"ld_image": 127},
    "ld_out below the width": {"ld_out": 127},
    "image window past the last row": {"image_row0": 90, "image_rows": 7},
    "output window past the last row": {"out_row0": 1, "out_rows": 96},
    "output window of no rows": {"out_rows": 0},
    "origin pushes a corner above -2 N": {"origin_row": -(2 * 32 - 16) - 1},
    "origin pushes a corner past height + N": {"origin_row": 2 * 32},
    "origin pushes a corner past width + N": {"origin_col": 2 * 32},
    "image frame stride below (rows - 1) x ld + width": {"frames": 3, "image_stride": 95 * 128 + 127, "out_stride": 96 * 128},
    "output frame stride below (rows - 1) x ld + width": {"frames": 3, "image_stride": 96 * 128, "out_stride": 95 * 128 + 127},
}
