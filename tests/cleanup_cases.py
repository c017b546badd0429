"""Seeded cells for the tests of the builder's clean-up kernel B3 (csrc/rpsf_core_cleanup.hpp), their oracle and the checks, shared
between the emulator tests (tests/test_cleanup_host.py) and the GPU tests (tests/test_gpu_cleanup.py).

The oracle is ``builder.clean_cell`` on the same float64 cell.  ``steps`` restates it call for call to get at its intermediates
(the fit mask, p before and after the cut) and asserts that it ends with ``clean_cell``'s bits; from those intermediates alone
``well_posed`` decides whether a cell is decidable, and a cell that is not takes the next seed.  No cell is ever left out.
"""

from __future__ import annotations

import functools
import pathlib

import numpy as np

from regularizepsf_amd import builder as bld

BOUND = 1e-12  # the project's bound for a float64 step against NumPy / SciPy, per cell, relative to the cell's maximum
SIZES = (4, 5, 16, 33, 64, 65, 127, 128)  # smallest, smallest odd, 1 pixel per thread, ragged last pass, 16 per thread at 256, first 1024, odd, LDS maximum
LABEL_SIZES = (16, 33, 128)
LABEL_PATTERNS = ("serpentine", "diagonal", "checkerboard", "borders", "second_blob")
RECIPES = ("zero_first", "star", "holes", "border_zeros", "zero_centre", "negative_plateau", "zero_after")
MAX_SEEDS = 5
CLEANED, DEGENERATE = 0, 1


# ---------------------------------------------------------------------------------------------------------------- emulator
@functools.cache
def emulator():
    """tests/emu/libemu_cleanup.so: kernel B3's driver on the CPU.  __graft_entry__.build() compiles it; it is compiled here when it is
    missing or older than its sources.  Without a compiler that is an error, not a skip."""
    import ctypes
    import os
    import shutil
    import subprocess

    root = pathlib.Path(__file__).resolve().parent.parent
    src, out = root / "tests" / "emu" / "emu_cleanup.cpp", root / "tests" / "emu" / "libemu_cleanup.so"
    cores = [root / "regularizepsf_amd" / "csrc" / n for n in ("rpsf_core_cleanup.hpp", "rpsf_core_builder.hpp", "rpsf_core_stars.hpp")]
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, *(c.stat().st_mtime for c in cores)):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++") or shutil.which("hipcc")
        assert clang is not None, "no clang++ to build tests/emu/emu_cleanup.cpp"
        fresh = out.with_name(f"libemu_cleanup.{os.getpid()}.so")  # written aside and moved into place: test processes may run side by side
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(fresh), str(src)], check=True)
        os.replace(fresh, out)
    lib = ctypes.CDLL(str(out))
    lib.emuc_clean.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.emuc_lds_bytes.argtypes = [ctypes.c_int]
    lib.emuc_lds_bytes.restype = ctypes.c_size_t
    return lib


def emu_clean(cells: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Kernel B3 on the emulator: (cleaned cells, flags)."""
    cells = np.ascontiguousarray(cells, np.float64)
    assert cells.ndim == 3 and cells.shape[1] == cells.shape[2]
    out = np.full_like(cells, 7.0)
    flags = np.full(len(cells), 9, np.uint8)
    assert emulator().emuc_clean(cells.shape[-1], len(cells), cells.ctypes.data, out.ctypes.data, flags.ctypes.data) == 0
    return out, flags


class EmulatedStack:
    """``builder._Stack`` with the three kernels on the emulators: what lets ``ArrayPSFBuilder.build`` run without a GPU."""

    def __init__(self, psf_size: int, device: int = 0, capacity: int = 1) -> None:  # noqa: ARG002
        self.psf_size = int(psf_size)
        self._patches = np.zeros((0, self.psf_size, self.psf_size), np.float32)

    def add_frame(self, frame, rounded, shift, saturation_threshold, star_minimum, star_maximum):
        from tests import builder_cases as bc

        patches, flags = bc.emu_patches(frame, self.psf_size, np.asarray(rounded).reshape(-1, 2), np.asarray(shift).reshape(-1, 2),
                                        saturation_threshold, star_minimum, star_maximum)
        self.load(patches[flags == bld.ACCEPTED])
        return flags

    def load(self, patches):
        self._patches = np.concatenate([self._patches, np.asarray(patches, np.float32).reshape(-1, self.psf_size, self.psf_size)])

    def __len__(self):
        return len(self._patches)

    def patches(self, first=0, count=None):
        return self._patches[first:None if count is None else first + count].copy()

    def average(self, method, percentile, offsets, members):
        from tests import builder_cases as bc

        return bc.emu_average(self._patches, bld.AVERAGE_METHODS[method], percentile, offsets, members)

    def clean(self, cells):
        return emu_clean(np.asarray(cells, np.float64).reshape(-1, self.psf_size, self.psf_size))

    def model(self, method, percentile, offsets, members):
        return self.clean(self.average(method, percentile, offsets, members))

    def close(self):
        pass


# ---------------------------------------------------------------------------------------------------------------- oracle
def steps(cell: np.ndarray) -> dict:
    """``clean_cell`` (with ``background_plane``) call for call, keeping the intermediates.  ``out`` is asserted to be ``clean_cell``'s
    own result bit for bit, so everything read off here is the oracle's."""
    from scipy.ndimage import binary_dilation, binary_erosion, label

    cell = np.asarray(cell, np.float64)
    n = cell.shape[0]
    inner = binary_erosion(cell != 0)
    inner[0, :] = inner[-1, :] = False
    inner[:, 0] = inner[:, -1] = False
    candidates = binary_dilation(inner) & ~inner
    ring = candidates & (cell < cell[n // 2, n // 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        p = cell - bld.background_plane(cell)
        p[p == 0] = np.nan
        before_cut = p.copy()
        centre = p[n // 2, n // 2]
        p[binary_erosion(p < 0.005 * centre, border_value=1)] = np.nan
        p[~np.isfinite(p)] = 0
        after_cut = p.copy()
        labels = label(p)[0]
        core = binary_dilation(labels == labels[n // 2, n // 2])
        p = p * core
        out = p / np.nansum(p)
        want = bld.clean_cell(cell)
    assert np.array_equal(out.view(np.int64), want.view(np.int64)), "steps() no longer restates clean_cell"
    return {"candidates": candidates, "ring": ring, "before_cut": before_cut, "centre": centre, "after_cut": after_cut, "out": want}


def expected_flag(cell: np.ndarray, ring: np.ndarray) -> int:
    """What the kernel must say, from the oracle's fit mask: DEGENERATE for a non-zero cell with fewer than three ring pixels."""
    return DEGENERATE if (np.any(cell != 0) and ring.sum() < 3) else CLEANED


def well_posed(cell: np.ndarray, s: dict) -> str | None:
    """Why no decision of the kernel may hang on a rounding for this cell - None - or the first reason why one may.  Asserted on the
    oracle's float64 data only.
    - the fit mask has at least 4 pixels, not nearly on one line: 1 - rho^2 of their centred coordinates above 1e-3;
    - no pixel that could be in the fit mask within 1e-9 |centre| of the centre value;
    - no non-zero pixel with |p| < 1e-9 |p[centre]| (it could be an exact zero on one side);
    - no pixel within 1e-9 |p[centre]| of the cut at 0.005 p[centre].
    With a zero centre p[centre] is NaN and nothing is cut; the scale of the third test is then the largest |p|."""
    n = cell.shape[0]
    centre_value = cell[n // 2, n // 2]
    ring = s["ring"]
    if ring.sum() < 4:
        return f"{ring.sum()} ring pixels"
    rows, cols = np.nonzero(ring)
    dx, dy = cols - cols.mean(), rows - rows.mean()
    sxx, syy, sxy = (dx * dx).sum(), (dy * dy).sum(), (dx * dy).sum()
    if not (sxx > 0 and syy > 0 and (sxx * syy - sxy * sxy) / (sxx * syy) > 1e-3):
        return "ring pixels nearly on one line"
    if np.any(np.abs(cell[s["candidates"]] - centre_value) <= 1e-9 * abs(centre_value)) and centre_value != 0:
        return "a ring candidate at the centre value"
    if centre_value == 0 and np.any(np.abs(cell[s["candidates"]]) <= 1e-9 * np.abs(cell).max()):
        return "a ring candidate at the (zero) centre value"
    p = s["before_cut"]
    live = np.isfinite(p)
    scale = abs(s["centre"]) if np.isfinite(s["centre"]) else np.abs(p[live]).max()
    with np.errstate(invalid="ignore"):
        plane_subtracted = cell - bld.background_plane(cell)
    if np.any(np.abs(plane_subtracted[cell != 0]) < 1e-9 * scale):
        return "a non-zero pixel on the plane"
    if np.isfinite(s["centre"]) and np.any(np.abs(p[live] - 0.005 * s["centre"]) <= 1e-9 * scale):
        return "a pixel at the cut"
    return None


def _freeze(out: dict) -> dict:
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return out


def _settle(make, what: str) -> dict:
    """The cell `make(seed)` gives for the first of MAX_SEEDS seeds for which it is decidable: all zero, structurally degenerate
    (fewer than three ring pixels: flag 1, whatever the values), or well posed."""
    reasons = []
    for seed in range(1, MAX_SEEDS + 1):
        cell = np.ascontiguousarray(make(seed), np.float64)
        assert np.isfinite(cell).all()
        if not np.any(cell != 0):
            return _freeze({"cell": cell, "flag": CLEANED, "want": np.full_like(cell, np.nan), "seed": seed, "after_cut": np.zeros_like(cell)})
        s = steps(cell)
        if expected_flag(cell, s["ring"]) == DEGENERATE:
            return _freeze({"cell": cell, "flag": DEGENERATE, "want": cell.copy(), "seed": seed, "after_cut": s["after_cut"]})
        reason = well_posed(cell, s)
        if reason is None:
            return _freeze({"cell": cell, "flag": CLEANED, "want": s["out"], "seed": seed, "after_cut": s["after_cut"]})
        reasons.append(reason)
    raise AssertionError(f"{what}: no well-posed cell within {MAX_SEEDS} seeds: {reasons}")


# ---------------------------------------------------------------------------------------------------------------- recipe cells
def star_cell(n: int, rng: np.random.Generator) -> np.ndarray:
    """builder_cases.star_frame's recipe for one star at the centre of an n x n cell, averaged by hand: what B1 and B2 leave of it is
    the star over a background near zero (tilted, with noise of both signs), divided by the centre pixel."""
    rows, cols = np.mgrid[0:n, 0:n].astype(np.float64)
    amp, sig_r, sig_c = rng.uniform(60, 400), rng.uniform(1.1, 1.5), rng.uniform(1.1, 1.5)
    r0, c0 = n // 2 + rng.uniform(-0.3, 0.3), n // 2 + rng.uniform(-0.3, 0.3)
    cell = 0.1 + 0.03 * (rows - n / 2) - 0.02 * (cols - n / 2) + rng.normal(0.0, 0.3, (n, n))
    cell += amp * np.exp(-0.5 * (((rows - r0) / sig_r) ** 2 + ((cols - c0) / sig_c) ** 2))
    return cell / cell[n // 2, n // 2]


def recipe_cell(n: int, recipe: str, seed: int) -> np.ndarray:
    rng = np.random.default_rng([seed, n, RECIPES.index(recipe)])
    if recipe in ("zero_first", "zero_after"):
        return np.zeros((n, n))
    cell = star_cell(n, rng)
    ctr = n // 2
    if recipe == "holes":  # 3 - 6 interior pixels (not the centre) set to 0: the rings form around them
        interior = [(r, c) for r in range(1, n - 1) for c in range(1, n - 1) if (r, c) != (ctr, ctr)]
        count = min(int(rng.integers(3, 7)), len(interior))
        for k in rng.choice(len(interior), count, replace=False):
            cell[interior[k]] = 0.0
    elif recipe == "border_zeros":  # zeros on the border lines, a corner among them
        border = [(r, c) for r in range(n) for c in range(n) if r in (0, n - 1) or c in (0, n - 1)]
        for k in rng.choice(len(border), min(int(rng.integers(3, 7)), n), replace=False):
            cell[border[k]] = 0.0
        cell[0, n - 1] = 0.0
    elif recipe == "zero_centre":  # the background-as-core branch
        cell[ctr, ctr] = 0.0
    elif recipe == "negative_plateau":  # non-zero, so labelled; solid, so its inside is below the cut and eroded away
        size = max(2, n // 4)
        r0, c0 = int(rng.integers(0, max(1, ctr - size))), int(rng.integers(0, n - size + 1))
        cell[r0:r0 + size, c0:c0 + size] = -0.3 + rng.normal(0.0, 0.01, (size, size))
    return cell


@functools.lru_cache(maxsize=None)
def size_case(n: int) -> dict:
    """The cells of one size in launch order: an all-zero cell first, the five recipes, the all-zero cell after a normal one (it sees
    whatever LDS the cell before it left)."""
    cells = [_settle(lambda seed, r=recipe: recipe_cell(n, r, seed), f"N = {n} {recipe}") for recipe in RECIPES]
    return _batch(cells, [f"{r}" for r in RECIPES])


def _batch(cells: list[dict], names: list[str]) -> dict:
    return _freeze({"names": tuple(names), "cells": np.stack([c["cell"] for c in cells]), "flags": np.array([c["flag"] for c in cells], np.uint8),
                    "want": np.stack([c["want"] for c in cells]), "after_cut": np.stack([c["after_cut"] for c in cells])})


# ---------------------------------------------------------------------------------------------------------------- labelling cells
def label_pattern(n: int, name: str) -> np.ndarray:
    """The non-zero pattern step 4 has to leave (True: non-zero).  Every pattern holds the 3 x 3 block around the centre: its centre
    pixel is the only one of it with a whole cross, so its four neighbours are ring pixels."""
    ctr = n // 2
    p = np.zeros((n, n), bool)
    p[ctr - 1:ctr + 2, ctr - 1:ctr + 2] = True
    if name == "serpentine":  # one pixel wide, from the centre block through every row: the longest chains a cell can hold
        for side in (-1, 1):  # above and below the block: every second row is a full line, the rows between hold one link at alternating ends
            r, k = ctr + 2 * side, 0
            while 0 <= r < n:
                p[r, :] = True
                link = r + side
                if 0 <= link < n:
                    p[link, n - 1 if k % 2 == 0 else 0] = True
                r, k = r + 2 * side, k + 1
    elif name == "diagonal":  # a second block touching the first at one corner only: 4-connectivity keeps them apart
        p[ctr + 2:ctr + 5, ctr + 2:ctr + 5] = True
    elif name == "checkerboard":
        rows, cols = np.indices((n, n))
        p |= (rows + cols) % 2 == 0
    elif name == "borders":  # one component along all four border lines, tied to the centre by a spoke
        p[0, :] = p[-1, :] = p[:, 0] = p[:, -1] = True
        p[0:ctr, ctr] = True
    elif name == "second_blob":  # bright, away from the centre: removed
        p[1:4, 1:4] = True
    else:
        raise KeyError(name)
    return p


def label_cell(n: int, name: str, seed: int) -> np.ndarray:
    """A cell whose non-zero pixels are the pattern: centre 2, the pixels the oracle can take into its fit mask about 1 (below the
    centre, so they are), everything else about 3.  The plane through the ring lies near 1, so p is about 1 at the centre, 2 on the
    pattern and a small residual on the ring; a ring pixel is below the cut but has a neighbour that is not, so the erosion keeps it."""
    from scipy.ndimage import binary_dilation, binary_erosion

    rng = np.random.default_rng([seed, n, 100 + LABEL_PATTERNS.index(name)])
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
    """The labelling cells of one size.  That step 4 leaves exactly the prescribed pattern is asserted here, from the oracle's own
    intermediate."""
    cells = []
    for name in LABEL_PATTERNS:
        got = _settle(lambda seed, k=name: label_cell(n, k, seed), f"N = {n} {name}")
        assert got["flag"] == CLEANED, name
        assert np.array_equal(got["after_cut"] != 0, label_pattern(n, name)), f"N = {n} {name}: step 4 does not leave the pattern"
        cells.append(got)
    out = dict(_batch(cells, list(LABEL_PATTERNS)))
    ctr = n // 2
    want = out["want"]
    # what the patterns are there for, read off the oracle's result
    assert np.all(want[LABEL_PATTERNS.index("diagonal")][ctr + 2:ctr + 5, ctr + 2:ctr + 5] == 0)  # the second block stayed separate
    assert np.all(want[LABEL_PATTERNS.index("second_blob")][1:4, 1:4] == 0)  # removed
    assert np.all(want[LABEL_PATTERNS.index("borders")][[0, -1], :] != 0) and np.all(want[LABEL_PATTERNS.index("borders")][:, [0, -1]] != 0)
    snake = want[LABEL_PATTERNS.index("serpentine")]
    assert np.array_equal(snake != 0, label_pattern(n, "serpentine"))  # one component, reached through every row
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def degenerate_case() -> dict:
    """N = 8, zero except the 3 x 3 block at rows and columns 3 ... 5 with value 1, centre 2, (4, 3) and (4, 5) set to 3: the ring
    candidates are the centre's four neighbours and two of them are below the centre."""
    cell = np.zeros((8, 8))
    cell[3:6, 3:6] = 1.0
    cell[4, 4] = 2.0
    cell[4, 3] = cell[4, 5] = 3.0
    s = steps(cell)
    assert s["ring"].sum() == 2 and expected_flag(cell, s["ring"]) == DEGENERATE
    return _freeze({"cell": cell, "want": s["out"]})


# ---------------------------------------------------------------------------------------------------------------- checks
def check(case: dict, out: np.ndarray, flags: np.ndarray, label: str) -> float:
    """The criteria of every comparison with the oracle, the same for the emulator and the GPU.  Flags as expected; per cleaned cell
    the non-zero pixels and the NaN pixels exactly the oracle's and max|got - oracle| <= 1e-12 max|oracle|; a flagged cell comes
    back as it went in.  Prints and returns the largest relative error."""
    assert out.dtype == np.float64 and out.shape == case["cells"].shape and flags.dtype == np.uint8
    assert np.array_equal(flags, case["flags"]), f"{label}: flags {flags.tolist()} != {case['flags'].tolist()}"
    worst = 0.0
    for name, cell, got, want, flag in zip(case["names"], case["cells"], out, case["want"], case["flags"]):
        if flag == DEGENERATE:
            assert np.array_equal(got.view(np.int64), cell.view(np.int64)), f"{label} {name}: a flagged cell must come back as it went in"
            continue
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{label} {name}: NaN pixels"
        if np.isnan(want).all():
            continue
        assert np.isfinite(want).all()
        assert np.array_equal(got != 0, want != 0), f"{label} {name}: support"
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"{label} {name}: {int((want != 0).sum())} pixels kept, max|got - oracle| / max|oracle| = {err:.3e}")
        assert err <= BOUND, f"{label} {name}"
        worst = max(worst, err)
    print(f"{label}: {len(flags)} cells, {int((case['flags'] == DEGENERATE).sum())} flagged, worst {worst:.3e}")
    return worst


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ---------------------------------------------------------------------------------------------------------------- frames -> model
MODEL_SIZES = ("n16", "n33")


@functools.lru_cache(maxsize=None)
def model_case(name: str) -> dict:
    """builder_cases.size_case(name) with the membership of its accepted patches in the cells of the covering (as
    builder_cases.end_to_end_case builds it, without its demand for an empty cell)."""
    from regularizepsf_amd.util import calculate_covering
    from tests import builder_cases as bc

    case = bc.size_case(name)
    n = case["n"]
    keys = np.concatenate([corner[flags == 1] for corner, flags in zip(case["corner"], case["flags"])])
    offsets, members = bld.cell_membership(keys, calculate_covering(case["frames"][0].shape, n), n)
    assert (np.diff(offsets) > 0).any()
    return _freeze({"n": n, "offsets": offsets, "members": members})


def fill(stack, name: str) -> None:
    """The frames of builder_cases.size_case(name) through kernel B1 of `stack` (a builder._Stack or an EmulatedStack)."""
    from tests import builder_cases as bc

    case = bc.size_case(name)
    for frame, rounded, shift, want in zip(case["frames"], case["rounded"], case["shift"], case["flags"]):
        flags = stack.add_frame(frame, rounded, shift, *case["thresholds"])
        assert np.array_equal(flags, want)


def check_model_is_average_then_clean(stack, name: str) -> None:
    """rpsf_builder_model's contract: the bits of rpsf_builder_average followed by rpsf_builder_clean, a flagged cell holding the
    averaged one - and that against the oracle."""
    from tests import builder_cases as bc

    case = model_case(name)
    for method, q in bc.METHODS:
        cells = stack.average(method, q, case["offsets"], case["members"])
        separate, separate_flags = stack.clean(cells)
        fused, fused_flags = stack.model(method, q, case["offsets"], case["members"])
        assert np.array_equal(fused_flags, separate_flags) and same_bits(fused, separate)
        assert same_bits(fused[fused_flags == DEGENERATE], cells[fused_flags == DEGENERATE])
        want = np.stack([bld.clean_cell(c) for c in cells])
        final = bld.model_on_device(stack, method, q, case["offsets"], case["members"])
        compare_models(final, want, f"{name} {method}")


def compare_models(got: np.ndarray, want: np.ndarray, label: str) -> None:
    """Two models cell by cell: the same NaN cells, every other cell within BOUND of its maximum."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{label}: NaN pixels"
    worst, compared = 0.0, 0
    for a, b in zip(got, want):
        if np.isnan(b).all():
            continue
        assert np.isfinite(b).all()
        err = float(np.abs(a - b).max() / np.abs(b).max())
        assert err <= BOUND, label
        worst, compared = max(worst, err), compared + 1
    assert compared > 0
    print(f"{label}: {compared} cells with stars of {len(want)}, worst {worst:.3e}")


def check_build(name: str) -> None:
    """A build with cleanup="device" against one with cleanup="host" on the frames and stars of a golden case (read only): the same counts,
    the same NaN cells, every other cell within the bound; return_patches is unaffected."""
    import regularizepsf_amd as rp
    from tests import builder_cases as bc

    g = bc.load(name)
    builder = rp.ArrayPSFBuilder(g["n"])
    on_host, on_device = rp.ArrayPSFBuilder(g["n"], cleanup="host"), rp.ArrayPSFBuilder(g["n"], cleanup="device")
    for method, q in bc.METHODS:
        kw = dict(average_method=method, percentile=q, stars=g["stars"], return_patches=True, **bc.thresholds(name))
        host, host_counts, host_patches = on_host.build(g["frames"], **kw)
        device, device_counts, device_patches = on_device.build(g["frames"], **kw)
        assert host_counts == device_counts and list(host_counts) == list(device_counts)
        assert [tuple(c) for c in host.coordinates] == [tuple(c) for c in device.coordinates]
        compare_models(device.values, host.values, f"build {name} {method}")
        assert list(host_patches) == list(device_patches)
        assert all(same_bits(host_patches[k], device_patches[k]) for k in host_patches)
        plain, _ = builder.build(g["frames"], average_method=method, percentile=q, stars=g["stars"], **bc.thresholds(name))
        assert same_bits(plain.values, host.values)  # the default is the host clean-up
