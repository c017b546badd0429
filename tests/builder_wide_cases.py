"""Cases, checks and emulator loaders for the PSF builder at the wide sizes 129 ... 256 (kernels B1w and B3w), shared between the
emulator tests (tests/test_builder_wide_host.py) and the GPU tests (tests/test_gpu_builder_wide.py).

The oracle is the float64 NumPy / SciPy restatement of tests/builder_cases.py and tests/cleanup_cases.py, called as it is: only what
is keyed to their case tables (``check_size_patches``, ``end_to_end_case``) and the one labelling pattern that does not settle at these
sizes are restated here.  The bounds are theirs: ``builder_cases.TOL`` per patch and per cell, ``cleanup_cases.BOUND`` for the clean-up.
"""

from __future__ import annotations

import ctypes
import functools
import pathlib

import numpy as np

from tests import builder_cases as bc
from tests import cleanup_cases as cc
from tests import emulib

ROOT = pathlib.Path(__file__).resolve().parent.parent

# name: patch size, frame shape, frames, seed, thresholds or None - the recipe of builder_cases.SIZE_CASES (10 stars per frame).
# Every case is well_posed() at seed 1 for every star.
WIDE_CASES = {
    "n129": {"n": 129, "shape": (270, 261), "frames": 1, "seed": 1},  # first wide size, odd, row pitch = N
    "n160": {"n": 160, "shape": (330, 300), "frames": 1, "seed": 1},  # even, not a multiple of 64
    "n255": {"n": 255, "shape": (270, 261), "frames": 1, "seed": 1},  # odd, just below the maximum
    "n256": {"n": 256, "shape": (270, 261), "frames": 2, "seed": 1, "thresholds": (350.0, 80.0, 300.0)},  # the maximum
    "n192_small": {"n": 192, "shape": (100, 90), "frames": 1, "seed": 1},  # frame smaller than the patch: the mirror map wraps
    "n256_small": {"n": 256, "shape": (50, 40), "frames": 1, "seed": 1},  # ... more than once
}
ISOLATION = ("n129", "n256")
END_TO_END = ("n129", "n256")
CLEAN_SIZES = (129, 192, 255, 256)
PARITY_SIZES = ("n64", "n128")  # cases of builder_cases.SIZE_CASES on which the wide phases must give kernel B1's bits


# ---------------------------------------------------------------------------------------------------------------- emulators
@functools.cache
def emulator_b1w():
    lib = emulib.library("emu_builder_wide")
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emubw_patches.argtypes = [i, vp, i, i, i, vp, vp, d, d, d, i, vp, vp]
    for name in ("emubw_lds_bytes", "emubw_slot_bytes"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [i], ctypes.c_size_t
    lib.emubw_slots.argtypes = [i]
    return lib


@functools.cache
def emulator_b3w():
    lib = emulib.library("emu_cleanup_wide")
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emucw_clean.argtypes = [i, i, vp, vp, vp, i]
    for name in ("emucw_lds_bytes", "emucw_slot_bytes"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [i], ctypes.c_size_t
    return lib


def slots(n: int) -> int:
    """The number of workspace slots the kernels use at patch size n (rpsf_builder_wide_slots says the same of a live handle)."""
    return int(emulator_b1w().emubw_slots(n))


def emu_patches(frame: np.ndarray, n: int, rounded: np.ndarray, shift: np.ndarray, saturation_threshold: float = np.inf,
                star_minimum: float = 0.0, star_maximum: float = np.inf, n_slots: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """Kernel B1w on the emulator, with the kernel's slots unless told otherwise: (float32 patches of every star, flags)."""
    img = np.ascontiguousarray(frame, np.float32)
    corners = np.ascontiguousarray(rounded, np.int32).reshape(-1, 2)
    frac = np.ascontiguousarray(shift, np.float64).reshape(-1, 2)
    patches = np.full((len(corners), n, n), np.nan, np.float32)
    flags = np.zeros(len(corners), np.uint8)
    rc = emulator_b1w().emubw_patches(n, img.ctypes.data, img.shape[0], img.shape[1], len(corners), corners.ctypes.data, frac.ctypes.data,
                                      saturation_threshold, star_minimum, star_maximum, slots(n) if n_slots is None else n_slots,
                                      patches.ctypes.data, flags.ctypes.data)
    assert rc == 0
    return patches, flags


def emu_clean(cells: np.ndarray, n_slots: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """Kernel B3w on the emulator: (cleaned cells, flags)."""
    cells = np.ascontiguousarray(cells, np.float64)
    assert cells.ndim == 3 and cells.shape[1] == cells.shape[2]
    out = np.full_like(cells, 7.0)
    flags = np.full(len(cells), 9, np.uint8)
    rc = emulator_b3w().emucw_clean(cells.shape[-1], len(cells), cells.ctypes.data, out.ctypes.data, flags.ctypes.data,
                                    slots(cells.shape[-1]) if n_slots is None else n_slots)
    assert rc == 0
    return out, flags


# ---------------------------------------------------------------------------------------------------------------- B1w
@functools.lru_cache(maxsize=None)
def wide_case(name: str) -> dict:
    """A case of WIDE_CASES with the oracle's answer (shared; do not modify)."""
    case = WIDE_CASES[name]
    frames, stars = bc.make_size_case(case["shape"], case["n"], case["frames"], case["seed"])
    return bc.oracle_case(case["n"], frames, stars, case.get("thresholds", (np.inf, 0.0, np.inf)))


def emu_case(case: dict, n_slots: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """Every frame of a case through the emulator: (patches of EVERY star in star order over all frames, flags)."""
    pairs = [emu_patches(frame, case["n"], rounded, shift, *case["thresholds"], n_slots=n_slots)
             for frame, rounded, shift in zip(case["frames"], case["rounded"], case["shift"])]
    return np.concatenate([p for p, _ in pairs]), np.concatenate([f for _, f in pairs])


def check_patches(name: str, got: np.ndarray, flags: np.ndarray) -> float:
    """builder_cases.check_size_patches for a case of WIDE_CASES: `got` are the accepted float32 patches in star order over all
    frames, `flags` the flags of every star.  Returns the worst per-patch error."""
    case = wide_case(name)
    want_flags = np.concatenate(case["flags"])
    assert np.array_equal(flags, want_flags)
    want = np.concatenate(case["patches"])[want_flags == 1]
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
    print(f"{name}: N = {case['n']}, frame {case['frames'].shape[1:]}, {len(want_flags)} stars, {len(want)} accepted, "
          f"max per-patch error {err.max():.3e}")
    assert np.all(err <= bc.TOL)
    if case["finite_thresholds"]:
        assert 0 < want_flags.sum() < len(want_flags)  # the thresholds reject somebody and keep somebody
    return float(err.max())


@functools.lru_cache(maxsize=None)
def slot_case() -> dict:
    """One 270 x 261 frame for N = 129 with 2 slots + 3 stars, drawn as builder_cases.size_stars draws them (2 slots - 2 random stars
    and its five fixed ones): in one launch every slot gets a second star and three slots a third.  No oracle: the emulator's bits
    are what is asked for."""
    from regularizepsf_amd import builder as bld

    n, shape = 129, (270, 261)
    rng = np.random.default_rng([1, n, 2 * slots(n) + 3])
    stars = bc.size_stars(shape, n, rng, random=2 * slots(n) - 2)
    assert len(stars) == 2 * slots(n) + 3
    frame = bc.star_frame(shape, stars, rng).astype(np.float32)  # a star at every position: its patch has a bright centre and is kept
    _, rounded, shift = bld.star_geometry(stars, n)
    return bc._freeze({"n": n, "frame": frame, "rounded": rounded, "shift": shift})


# ---------------------------------------------------------------------------------------------------------------- frames -> cells
@functools.lru_cache(maxsize=None)
def end_to_end_case(name: str) -> dict:
    """builder_cases.end_to_end_case for a case of WIDE_CASES: the oracle's accepted patches, their membership in the cells of the
    covering and oracle_cells per method of METHODS.  n129 and n256 as they stand hold an empty cell and a cell that really averages."""
    from regularizepsf_amd import builder as bld
    from regularizepsf_amd.util import calculate_covering

    case = wide_case(name)
    n = case["n"]
    keys = np.concatenate([corner[flags == 1] for corner, flags in zip(case["corner"], case["flags"])])
    patches = np.concatenate(case["patches"])[np.concatenate(case["flags"]) == 1]
    offsets, members = bld.cell_membership(keys, calculate_covering(case["frames"][0].shape, n), n)
    out = {"offsets": offsets, "members": members}
    for method, q in bc.METHODS:
        out[method] = bc.oracle_cells(patches, offsets, members, method, q)
    assert (np.diff(offsets) == 0).any() and (np.diff(offsets) > 1).any()  # an empty cell, and a cell that really averages
    return bc._freeze(out)


def check_end_to_end(name: str, average) -> None:
    """builder_cases.check_end_to_end for a case of WIDE_CASES: `average(method, q, offsets, members)` gives the cells of the side under test from
    ITS patches; per cell within TOL of the oracle cell's maximum, a cell without a star all zero on both sides."""
    want = end_to_end_case(name)
    empty = np.diff(want["offsets"]) == 0
    for method, q in bc.METHODS:
        cells = average(method, q, want["offsets"], want["members"])
        assert cells.dtype == np.float64 and cells.shape == want[method].shape
        assert np.all(cells[empty] == 0) and np.all(want[method][empty] == 0)
        err = np.abs(cells - want[method]).max(axis=(1, 2))[~empty]
        scale = np.abs(want[method]).max(axis=(1, 2))[~empty]
        print(f"{name} {method}: {len(scale)} cells with stars, max per-cell error {np.max(err / scale):.3e}")
        assert np.all(err <= bc.TOL * scale)


# ---------------------------------------------------------------------------------------------------------------- B3w: labelling cells
def label_pattern(n: int, name: str) -> np.ndarray:
    """cleanup_cases.label_pattern, with a second blob at [1:4, n-4:n-1] as well in `second_blob`: one blob alone leaves, above
    N of about 190, two tight clusters of ring pixels far apart, which are nearly on one line."""
    p = cc.label_pattern(n, name)
    if name == "second_blob":
        p[1:4, n - 4:n - 1] = True
    return p


def label_cell(n: int, name: str, seed: int) -> np.ndarray:
    """cleanup_cases.label_cell on the pattern above."""
    from scipy.ndimage import binary_dilation, binary_erosion

    rng = np.random.default_rng([seed, n, 100 + cc.LABEL_PATTERNS.index(name)])
    pattern = label_pattern(n, name)
    inner = binary_erosion(pattern)
    inner[0, :] = inner[-1, :] = False
    inner[:, 0] = inner[:, -1] = False
    candidates = binary_dilation(inner) & ~inner & pattern
    cell = np.where(pattern, 3.0 + rng.normal(0.0, 1e-3, (n, n)), 0.0)
    cell[candidates] = 1.0 + rng.normal(0.0, 1e-3, int(candidates.sum()))
    cell[n // 2, n // 2] = 2.0
    return cell


@functools.lru_cache(maxsize=None)
def label_case(n: int) -> dict:
    """cleanup_cases.label_case on the cells above, with its assertions: step 4 leaves exactly the pattern, the diagonal block stays
    separate, BOTH blobs are removed, the borders stay, the serpentine is one component."""
    cells = []
    for name in cc.LABEL_PATTERNS:
        got = cc._settle(lambda seed, k=name: label_cell(n, k, seed), f"N = {n} {name}")
        assert got["flag"] == cc.CLEANED, name
        assert got["seed"] == 1, name
        assert np.array_equal(got["after_cut"] != 0, label_pattern(n, name)), f"N = {n} {name}: step 4 does not leave the pattern"
        cells.append(got)
    out = dict(cc._batch(cells, list(cc.LABEL_PATTERNS)))
    ctr, want = n // 2, out["want"]
    at = cc.LABEL_PATTERNS.index
    assert np.all(want[at("diagonal")][ctr + 2:ctr + 5, ctr + 2:ctr + 5] == 0)
    assert np.all(want[at("second_blob")][1:4, 1:4] == 0) and np.all(want[at("second_blob")][1:4, n - 4:n - 1] == 0)
    assert np.all(want[at("borders")][[0, -1], :] != 0) and np.all(want[at("borders")][:, [0, -1]] != 0)
    assert np.array_equal(want[at("serpentine")] != 0, label_pattern(n, "serpentine"))
    return cc._freeze(out)
