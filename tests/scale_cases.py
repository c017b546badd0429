"""Cases, float64 oracle and stand-ins for the tests of ``interpolation_scale`` (tests/test_scale_host.py on the emulator,
tests/test_gpu_scale.py on the device) and for the fixture generator tests/golden/make_builder_scale_golden.py.

The oracle of the upscale is ``RectBivariateSpline`` called the way the reference calls it (image_processing.py:49-59).  The oracle of
the block mean is NumPy's reshape-mean: for a cell whose side the scale divides that IS ``skimage.transform.downscale_local_mean`` by
definition (it pads to a multiple of the block and takes ``block_reduce(..., np.mean)``); scikit-image is not a dependency of this
package or of its tests, so it is not imported here.
"""

from __future__ import annotations

import functools
import pathlib

import numpy as np

from tests import builder_cases as bc
from tests import cleanup_cases as cc

GOLDEN = bc.GOLDEN
SCALES = (2, 3, 4)
UPSCALE_BOUND = 1e-12  # x max|frame|: the project's figure for a float64 step on the device (cleanup_cases.BOUND)

# The kernels' own boundaries (csrc/rpsf_core_scale.hpp): the transposes move 32 x 32 tiles of Hs x W and of Ws x Hs, the line kernel runs
# 256 lanes per workgroup over W lanes (axis 0) and over Hs lanes (axis 1).  Lines are never cut, so there is no chunk length.
SHAPES = (
    (4, 4),  # no interior unknown on either axis
    (5, 9),  # one interior unknown on axis 0
    (6, 7),
    (63, 64),
    (65, 130),  # Hs = 257 at s = 4
    (17, 32), (17, 33),  # W on either side of a tile; Hs = 33, 49, 65 just past one
    (16, 31),  # Hs = 31 at s = 2: one below a tile; Ws = 61, 91, 121
    (5, 256), (5, 257),  # axis 0: the last lane of one workgroup, the first of a second
    (128, 5), (129, 5),  # axis 1: Hs = 255 and 257 at s = 2
)
PEDESTAL = ((63, 64), 3)  # this (shape, scale) is also run on a 1e7 pedestal


def block_mean(cells: np.ndarray, scale: int) -> np.ndarray:
    """(..., P, P) -> (..., P / s, P / s): the mean of every s x s block (downscale_local_mean for s | P)."""
    cells = np.asarray(cells, np.float64)
    p = cells.shape[-1]
    assert cells.shape[-2] == p and p % scale == 0
    return cells.reshape(*cells.shape[:-2], p // scale, scale, p // scale, scale).mean(axis=(-3, -1))


def oracle_upscale(frame: np.ndarray, scale: int) -> np.ndarray:
    """``_scale_image`` of the reference with the same SciPy call, float64."""
    from scipy.interpolate import RectBivariateSpline

    frame = np.asarray(frame, np.float64)
    h, w = frame.shape
    spline = RectBivariateSpline(np.arange(h), np.arange(w), frame)
    return spline(np.linspace(0, h - 1, 1 + (h - 1) * scale), np.linspace(0, w - 1, 1 + (w - 1) * scale))


def case_names() -> list[str]:
    names = []
    for index, (h, w) in enumerate(SHAPES):
        for s in SCALES:
            names.append(f"{h}x{w}_s{s}_f64")
        names.append(f"{h}x{w}_s{SCALES[index % 3]}_f32")
    names.append(f"{PEDESTAL[0][0]}x{PEDESTAL[0][1]}_s{PEDESTAL[1]}_f64_pedestal")
    return names


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """One upscale case: the frame (builder_cases.star_frame's recipe, two stars; float32 or float64), the scale and the oracle's
    answer for exactly that frame - computed once, shared by the emulator and the GPU tests; do not modify."""
    shape, s, kind, *extra = name.split("_")
    h, w = (int(v) for v in shape.split("x"))
    scale = int(s[1:])
    rng = np.random.default_rng([h, w, scale, kind == "f32"])
    pos = np.stack([rng.uniform(0, h - 1, 2), rng.uniform(0, w - 1, 2)], axis=-1)
    frame = bc.star_frame((h, w), pos, rng)
    if extra:
        frame = frame + 1e7
    frame = frame.astype(np.float32 if kind == "f32" else np.float64)
    out = {"frame": frame, "scale": scale, "want": oracle_upscale(frame, scale), "peak": float(np.abs(frame).max())}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return out


def check_upscale(name: str, got: np.ndarray) -> float:
    """The criteria of one upscale, the same for the emulator and the device.  Returns the error over the frame's peak."""
    c = case(name)
    s = c["scale"]
    assert got.dtype == np.float64 and got.shape == c["want"].shape == scaled_shape(c["frame"].shape, s)
    err = float(np.abs(got - c["want"]).max() / c["peak"])
    print(f"{name}: max|d| / max|frame| = {err:.3e}")
    assert err <= UPSCALE_BOUND
    assert np.array_equal(got[::s, ::s], c["frame"].astype(np.float64))  # an interpolating spline: the data points come back as they went
    return err


def scaled_shape(shape, scale):
    return 1 + (shape[0] - 1) * scale, 1 + (shape[1] - 1) * scale


# ------------------------------------------------------------------------------------------------------------------ block mean
BLOCK_CASES = ((4, 2), (5, 3), (8, 2), (16, 3), (16, 4), (33, 3), (64, 2), (32, 4))  # (N, s): one lane, ragged last workgroup, P = 128


@functools.lru_cache(maxsize=None)
def block_case(n: int, scale: int) -> dict:
    """Three P x P cells (a star-like cell with both signs, a cell on a 1e7 pedestal, all zero) and NumPy's block means."""
    rng = np.random.default_rng([n, scale, 4])
    p = n * scale
    cells = np.stack([rng.normal(0.0, 0.05, (p, p)) + np.exp(-0.5 * ((np.indices((p, p)) - p / 2) ** 2).sum(axis=0) / (0.1 * p) ** 2),
                      1e7 + rng.normal(0.0, 1.0, (p, p)), np.zeros((p, p))])
    out = {"cells": cells, "want": block_mean(cells, scale), "scale": scale, "n": n}
    for v in (out["cells"], out["want"]):
        v.flags.writeable = False
    return out


def check_block_mean(n: int, scale: int, got: np.ndarray) -> float:
    """Per output pixel within s^2 2^-53 of the largest sample of its block."""
    c = block_case(n, scale)
    assert got.dtype == np.float64 and got.shape == c["want"].shape
    p = n * scale
    largest = np.abs(c["cells"]).reshape(-1, n, scale, n, scale).max(axis=(2, 4))
    bound = scale * scale * 2.0 ** -53 * largest
    err = np.abs(got - c["want"])
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.where(largest > 0, err / (2.0 ** -53 * largest), 0.0)))
    print(f"N = {n}, s = {scale}, P = {p}: worst error {worst:.2f} x 2^-53 x the block's largest sample (bound {scale * scale})")
    assert np.all(err <= bound)
    assert np.all(got[-1] == 0)
    return worst


# -------------------------------------------------------------------------------------------------------------------- emulator
@functools.cache
def emulator():
    """tests/emu/libemu_scale.so: the launches of the upscale and kernel B4 on the CPU.  __graft_entry__.build() compiles it; it is
    compiled here when it is missing or older than its sources.  Without a compiler that is an error, not a skip."""
    import ctypes
    import os
    import shutil
    import subprocess

    root = pathlib.Path(__file__).resolve().parent.parent
    src, out = root / "tests" / "emu" / "emu_scale.cpp", root / "tests" / "emu" / "libemu_scale.so"
    core = root / "regularizepsf_amd" / "csrc" / "rpsf_core_scale.hpp"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, core.stat().st_mtime):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++") or shutil.which("hipcc")
        assert clang is not None, "no clang++ to build tests/emu/emu_scale.cpp"
        fresh = out.with_name(f"libemu_scale.{os.getpid()}.so")  # written aside and moved into place: test processes may run side by side
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(fresh), str(src)], check=True)
        os.replace(fresh, out)
    lib = ctypes.CDLL(str(out))
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emus_pivots.argtypes = [i, vp]
    lib.emus_upscale.argtypes = [vp, i, i, i, i, vp, i]
    lib.emus_block_mean.argtypes = [vp, i, i, i, vp]
    return lib


def emu_pivots(m: int) -> np.ndarray:
    ip = np.full(max(m - 4, 0) + 1, np.nan)  # one guard element the table must leave alone
    assert emulator().emus_pivots(m, ip.ctypes.data) == 0
    assert np.isnan(ip[-1])
    return ip[:-1]


def emu_upscale(frame: np.ndarray, scale: int, out_dtype=np.float64) -> np.ndarray:
    """U1 / U2 on the emulator: the float64 result of the public function, or the float32 one of the builder's frame buffer."""
    if frame.dtype != np.float32:
        frame = frame.astype(np.float64, copy=False)
    frame = np.ascontiguousarray(frame)
    out = np.full(scaled_shape(frame.shape, scale), np.nan, out_dtype)
    rc = emulator().emus_upscale(frame.ctypes.data, int(frame.dtype == np.float64), frame.shape[0], frame.shape[1], scale, out.ctypes.data,
                                 int(out.dtype == np.float32))
    assert rc == 0
    return out


def emu_block_mean(cells: np.ndarray, scale: int) -> np.ndarray:
    cells = np.ascontiguousarray(cells, np.float64)
    n = cells.shape[-1] // scale
    out = np.full((len(cells), n, n), np.nan)
    assert emulator().emus_block_mean(cells.ctypes.data, len(cells), n, scale, out.ctypes.data) == 0
    return out


class ScaledEmulatedStack(cc.EmulatedStack):
    """``builder._Stack`` for a scaled build with every kernel on its emulator: U1 / U2 into a float32 frame, B1 and B2 at
    ``psf_size * scale``, B4, B3 at ``psf_size``."""

    def __init__(self, psf_size: int, device: int = 0, capacity: int = 1, scale: int = 1) -> None:
        super().__init__(psf_size * scale, device, capacity)
        self.patch_size, self.psf_size, self.scale = psf_size * scale, int(psf_size), int(scale)

    def add_frame(self, frame, rounded, shift, saturation_threshold, star_minimum, star_maximum):
        if self.scale > 1:
            frame = emu_upscale(np.asarray(frame), self.scale, np.float32)
        patches, flags = bc.emu_patches(frame, self.patch_size, np.asarray(rounded).reshape(-1, 2), np.asarray(shift).reshape(-1, 2),
                                        saturation_threshold, star_minimum, star_maximum)
        self.load(patches[flags == 1])
        return flags

    def load(self, patches):
        self._patches = np.concatenate([self._patches, np.asarray(patches, np.float32).reshape(-1, self.patch_size, self.patch_size)])

    def downscale(self, cells):
        return emu_block_mean(np.asarray(cells, np.float64).reshape(-1, self.patch_size, self.patch_size), self.scale)

    def average(self, method, percentile, offsets, members):
        return self.downscale(super().average(method, percentile, offsets, members))


# ------------------------------------------------------------------------------------------- scaled builds: fixtures and oracle chain
# name: frame shape, model size N, scale, frames, stars per frame.  Fixtures: tests/golden/builder_scale_<name>*.npz, written by
# tests/golden/make_builder_scale_golden.py from the real reference (its build with its _scale_image).
BUILD_CASES = {
    "n8s2": {"shape": (41, 37), "n": 8, "scale": 2, "frames": 2, "stars": 12},
    "n16s3": {"shape": (60, 52), "n": 16, "scale": 3, "frames": 2, "stars": 8},
}


def make_build_case(name: str, seed: int) -> tuple[np.ndarray, list[np.ndarray]]:
    """(frames, stars): unscaled frames (F, H, W) float64 holding float32 values (builder_cases.star_frame's recipe), and per frame the
    star positions in SCALED-frame pixels - the unscaled centre times the scale, which is where the upscaled star peaks."""
    c = BUILD_CASES[name]
    (h, w), frames, stars = c["shape"], [], []
    for f in range(c["frames"]):
        rng = np.random.default_rng([seed, f, c["scale"]])
        pos = np.stack([rng.uniform(0, h - 1, c["stars"]), rng.uniform(0, w - 1, c["stars"])], axis=-1)
        frames.append(bc.star_frame((h, w), pos, rng).astype(np.float32).astype(np.float64))
        stars.append(pos * c["scale"])
    return np.stack(frames), stars


@functools.lru_cache(maxsize=None)
def load_build(name: str) -> dict:
    """Everything the generator stored for a scaled build, plus the regenerated frames (shared between the tests; do not modify)."""
    base = dict(np.load(GOLDEN / f"builder_scale_{name}.npz"))
    frames, stars = make_build_case(name, int(base["seed"]))
    stored = np.split(base["stars"], np.cumsum(base["stars_per_frame"])[:-1])
    assert all(np.array_equal(a, b) for a, b in zip(stars, stored)), "the frame generator no longer reproduces the fixture"
    c = BUILD_CASES[name]
    out = {**base, "frames": frames, "stars": stars, "n": c["n"], "scale": c["scale"], "p": c["n"] * c["scale"]}
    for method, _ in bc.METHODS:
        per = np.load(GOLDEN / f"builder_scale_{name}_{method}.npz")
        out.update({f"{key}_{method}": per[key] for key in per.files})
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return out


def per_frame(g: dict, key: str) -> list[np.ndarray]:
    return np.split(g[key], np.cumsum(g["stars_per_frame"])[:-1])


@functools.lru_cache(maxsize=None)
def oracle_chain(name: str) -> dict:
    """A scaled build in float64 without the fixture: oracle upscale, builder_cases.oracle_case at P, oracle_cells per method, block
    mean, clean_cell.  Keys: oracle (oracle_case's dict), offsets, members, corners, and per method cells_<m> (N x N) and values_<m>."""
    from regularizepsf_amd import builder as bld
    from regularizepsf_amd.util import calculate_covering

    g = load_build(name)
    s, p = g["scale"], g["p"]
    scaled = np.stack([oracle_upscale(frame, s) for frame in g["frames"]])
    oracle = bc.oracle_case(p, scaled, g["stars"])
    keys = np.concatenate([corner[flags == 1] for corner, flags in zip(oracle["corner"], oracle["flags"])])
    patches = np.concatenate(oracle["patches"])[np.concatenate(oracle["flags"]) == 1]
    corners = calculate_covering((scaled.shape[1] * s, scaled.shape[2] * s), p)
    offsets, members = bld.cell_membership(keys, corners, p)
    out = {"oracle": oracle, "offsets": offsets, "members": members, "corners": corners, "patches": patches}
    with np.errstate(all="ignore"):
        for method, q in bc.METHODS:
            cells = block_mean(bc.oracle_cells(patches, offsets, members, method, q), s)
            out[f"cells_{method}"] = cells
            out[f"values_{method}"] = np.stack([bld.clean_cell(cell) for cell in cells])
    return out


def check_patches(g: dict, got: np.ndarray, flags: np.ndarray) -> float:
    """The patch criteria of tests/test_gpu_builder.py at P: accept flags exact, per accepted patch within builder_cases.TOL of the
    reference patch's maximum."""
    assert np.array_equal(flags, g["accepted"])
    want = g["patches"]
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
    print(f"{len(got)} patches of {want.shape[-1]} pixels, max per-patch error {err.max():.3e}")
    assert np.all(err <= bc.TOL)
    return float(err.max())


def check_cells(cells: np.ndarray, want: np.ndarray, label: str) -> None:
    """Per cell within builder_cases.TOL of the cell's maximum; a cell without a star is all zeros on both sides."""
    assert cells.dtype == np.float64 and cells.shape == want.shape
    err = np.abs(cells - want).max(axis=(1, 2))
    scale = np.abs(want).max(axis=(1, 2))
    print(f"{label}: {int((scale > 0).sum())} cells with stars of {len(want)}, max per-cell error {np.max(err[scale > 0] / scale[scale > 0]):.3e}")
    assert np.all(err <= bc.TOL * scale)


def check_values(got: np.ndarray, want: np.ndarray, excluded: np.ndarray, counts: np.ndarray, label: str) -> None:
    """The final-model criteria of tests/test_gpu_builder.py: the same NaN pixels, per cell within builder_cases.TOL; cells the
    generator flagged as near the clean-up's cut are left out, cells without a star are all NaN on both sides."""
    assert got.dtype == np.float64 and got.shape == want.shape and excluded.mean() <= 0.10
    compared, worst = 0, 0.0
    for a, b, skip in zip(got, want, excluded):
        if skip:
            continue
        assert np.array_equal(np.isnan(a), np.isnan(b)), label
        if np.isnan(b).all():
            continue
        err = float(np.abs(a - b).max() / np.abs(b).max())
        assert err <= bc.TOL, label
        compared, worst = compared + 1, max(worst, err)
    assert compared == int(((counts > 0) & ~excluded).sum()) > 0
    print(f"{label}: {compared} cells compared, worst {worst:.3e}")


def check_build(name: str, cleanup: str, method: str, q: float) -> None:
    """``ArrayPSFBuilder(N, interpolation="device", cleanup=cleanup).build(frames, interpolation_scale=s, stars=...)`` against the
    fixture (coordinates, counts, patch keys, patches, final values) and against the oracle chain (final values)."""
    import regularizepsf_amd as rp

    g = load_build(name)
    builder = rp.ArrayPSFBuilder(g["n"], interpolation="device", cleanup=cleanup)
    psf, counts, patches = builder.build(g["frames"], interpolation_scale=g["scale"], average_method=method, percentile=q, stars=g["stars"],
                                         return_patches=True)
    assert [tuple(c) for c in psf.coordinates] == [tuple(c) for c in g["corners"]]
    assert list(counts) == [tuple(c) for c in g["corners"]] and list(counts.values()) == g["counts"].tolist()
    assert [tuple(k) for k in g["patch_keys"]] == list(patches)
    stack = np.stack(list(patches.values()))
    assert stack.shape[1:] == (g["p"], g["p"]) and np.array_equal(stack, stack.astype(np.float32).astype(np.float64))
    check_patches(g, stack.astype(np.float32), g["accepted"])
    label = f"{name} {cleanup} {method}"
    check_values(psf.values, g[f"values_{method}"], g[f"excluded_{method}"], g["counts"], label + " against the reference")
    chain = oracle_chain(name)
    assert np.array_equal(chain["corners"], g["corners"]) and np.array_equal(chain["offsets"], g["offsets"])
    check_values(psf.values, chain[f"values_{method}"], g[f"excluded_{method}"], g["counts"], label + " against the oracle chain")


def check_large_patch_small_model(stack) -> None:
    """A stack for N = 64, s = 2 (the device's, or the emulated one): B1 and B2 at 128 pixels, B4, B3 at 64.  One 70 x 66 frame of
    builder_cases.star_frame's recipe with four stars, spread so that every patch is well posed at 128 pixels."""
    from regularizepsf_amd import builder as bld

    n, s = 64, 2
    rng = np.random.default_rng(642)
    shape = (70, 66)
    pos = np.array([[20.3, 18.7], [48.6, 45.2], [22.4, 47.9], [50.1, 17.3]])
    frame = bc.star_frame(shape, pos, rng).astype(np.float32)
    stars = [pos * s]
    scaled = oracle_upscale(frame, s)
    oracle = bc.oracle_case(n * s, scaled[None], stars)
    bc.well_posed(oracle)
    flags = stack.add_frame(frame, oracle["rounded"][0], oracle["shift"][0], np.inf, 0.0, np.inf)
    assert np.array_equal(flags, oracle["flags"][0]) and flags.all()
    got, want = stack.patches(), oracle["patches"][0]
    assert got.shape == (4, 128, 128) and stack.patch_size == 128 and stack.psf_size == 64
    assert np.all(np.abs(got - want).max(axis=(1, 2)) <= bc.TOL * np.abs(want).max(axis=(1, 2)))
    offsets, members = np.array([0, 4, 4, 5], np.int64), np.array([0, 1, 2, 3, 2], np.int32)
    cells = stack.average("mean", 50.0, offsets, members)
    want_cells = block_mean(bc.oracle_cells(want, offsets, members, "mean"), s)
    assert cells.shape == (3, 64, 64) and np.all(cells[1] == 0)
    check_cells(cells, want_cells, "N = 64, s = 2")
    values, clean_flags = stack.model("mean", 50.0, offsets, members)
    assert values.shape == (3, 64, 64) and clean_flags.tolist() == [0] * 3
    for got_cell, cell in zip(values[[0, 2]], cells[[0, 2]]):
        want_cell = bld.clean_cell(cell)
        assert np.abs(got_cell - want_cell).max() <= cc.BOUND * np.abs(want_cell).max()
    assert np.isnan(values[1]).all()
