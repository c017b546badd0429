"""Model and residual frames (DESIGN.md 3.7 "Model and residual frames", kernel S10) restated in float64 NumPy, the cases, the CPU
emulator of the kernel with the host's tile lists, and the checks the emulator tests (tests/test_render_host.py) and the GPU tests
(tests/test_gpu_render.py) share.

There is no outside implementation: the reference is the restatement below, written from the definition, one star at a time in ascending
index, with array operations over the star's box clipped to the frame.  A check takes `make_finder(shape, box)` and
`make_model(values)`: regularizepsf_amd.stars._Finder and ._Model on the GPU, EmuFinder and EmuModel here.

BIT FOR BIT.  Kernel, emulator and restatement agree in every bit of every pixel, not within a bound:
  the model   m is fit_cases.ref_model, S8's expression, evaluated per pixel on both sides;
  the sum     starts at + 0.0 and takes flux x m of the stars drawn in ascending index, and only where q <= R R: a pixel outside a
              star's disc keeps its bits (the restatement selects, it does not add a zero);
  the mesh    is photometry_cases': the restatement takes the filtered mesh of the finder under test;
  the output  is the float64 value, or that value rounded once to float32 (numpy's astype rounds to nearest even, as the hardware does).
NaN is compared by position (`same_frame`).
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np

from tests import emulib
from regularizepsf_amd import stars
from tests import fit_cases as fc
from tests import fitpos_cases as fp
from tests import photometry_cases as pc
from tests import star_cases as sc

ROOT = sc.ROOT
MODEL, RESIDUAL, RESIDUAL_MESH = 0, 1, 2
MODES = (MODEL, RESIDUAL, RESIDUAL_MESH)
DTYPES = (np.float32, np.float64)
SHAPE, SMALL, BOX = (43, 70), (5, 7), 16  # a few tiles across with partial tiles on both axes; smaller than one tile
GAUSSIAN, ZERO, LOBES, CONSTANT = fc.GAUSSIAN, fc.ZERO, fc.LOBES, fc.CONSTANT


# ------------------------------------------------------------------------------------------------------------------ the restatement
def drawn(flux, cells, n_cells: int) -> np.ndarray:
    """Which stars are drawn: a finite flux and a cell of the model."""
    flux, cells = np.asarray(flux, np.float64), np.asarray(cells, np.int64)
    return np.isfinite(flux) & (cells >= 0) & (cells < n_cells)


def ref_sum(shape, cube, positions, flux, cells, radius) -> tuple[np.ndarray, np.ndarray]:
    """(s, reached): the definition's sum at every pixel of the frame, stars in ascending index, and which pixels lie in a drawn star's
    disc at all."""
    H, W = shape
    cube = np.asarray(cube, np.float64)
    positions = np.asarray(positions, np.float64).reshape(-1, 2)
    R = np.float64(radius)
    R2 = R * R
    s, reached = np.zeros(shape), np.zeros(shape, bool)
    keep = drawn(flux, cells, len(cube))
    for (y, x), f, k, take in zip(positions, np.asarray(flux, np.float64), np.asarray(cells, np.int64), keep):
        if not take:
            continue
        r0, r1 = max(int(np.floor(y - R)) - 1, 0), min(int(np.ceil(y + R)) + 1, H - 1)
        c0, c1 = max(int(np.floor(x - R)) - 1, 0), min(int(np.ceil(x + R)) + 1, W - 1)
        if r0 > r1 or c0 > c1:
            continue
        rr, cc = np.arange(r0, r1 + 1), np.arange(c0, c1 + 1)
        pr, pc_ = rr.astype(np.float64) - y, cc.astype(np.float64) - x
        disc = ((pr * pr)[:, None] + (pc_ * pc_)[None, :]) <= R2
        with np.errstate(all="ignore"):
            m = fc.ref_model(cube[k], pr, pc_, disc)
            part = s[r0:r1 + 1, c0:c1 + 1]
            s[r0:r1 + 1, c0:c1 + 1] = np.where(disc, part + f * m, part)
        reached[r0:r1 + 1, c0:c1 + 1] |= disc
    return s, reached


def ref_render(frame, box, level_f, cube, positions, flux, cells, radius, mode: int, dtype) -> np.ndarray:
    """The definition: the output frame of the mode, float64 or rounded once to float32."""
    frame = np.asarray(frame, np.float32)
    s, _ = ref_sum(frame.shape, cube, positions, flux, cells, radius)
    with np.errstate(all="ignore"):
        if mode == MODEL:
            v = s
        elif mode == RESIDUAL:
            v = frame.astype(np.float64) - s
        else:
            assert level_f is not None, "RESIDUAL_MESH has no restatement without a mesh: the call is an error"
            v = (frame.astype(np.float64) - sc.ref_surface(level_f, frame.shape, box)) - s
        return v.astype(dtype)


def same_frame(got: np.ndarray, want: np.ndarray) -> bool:
    """The same dtype and shape, NaN where NaN is, every other pixel the same bits (+ 0.0 is not - 0.0)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    keep = ~np.isnan(want)
    return got[keep].tobytes() == want[keep].tobytes()


# ------------------------------------------------------------------------------------------------------------------ the emulator
@functools.cache
def emulator():
    """tests/emu/libemu_render.so: the kernel's driver and the host's tile lists on the CPU, compiled here when missing or older than its
    sources."""
    lib = emulib.library("emu_render")
    vp, i, n, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    lib.emurd_info.argtypes = [vp]
    lib.emurd_lists.argtypes = [i, i, n, i, n, vp, vp, vp, f, vp, vp, n, vp]
    lib.emurd_lists.restype = n
    lib.emurd_render.argtypes = [vp, i, i, i, vp, i, n, i, vp, n, vp, vp, vp, f, i, i, vp, vp]
    return lib


def emulator_info() -> tuple[int, int, int, int, int]:
    """The tile's rows and columns, the chunk's records, the workgroups of S10 the last render ran, s10_lds_bytes()."""
    info = (ctypes.c_long * 5)(0, 0, 0, 0, 0)
    emulator().emurd_info(info)
    return tuple(info)


def tile_lists(shape, cube, positions, flux, cells, radius) -> tuple[np.ndarray, np.ndarray, int]:
    """The host's tile lists as rpsf_stars_render builds them: (offsets per tile in raster order, star indices, the stars drawn)."""
    tile_r, tile_c = emulator_info()[:2]
    tiles = -(-shape[0] // tile_r) * -(-shape[1] // tile_c)
    positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
    flux, cells = np.ascontiguousarray(flux, np.float64), np.ascontiguousarray(cells, np.int32)
    offsets, room = np.full(tiles + 1, -1, np.int64), max(1, tiles * len(positions))
    index, count = np.full(room, -1, np.int32), ctypes.c_long(-1)
    total = emulator().emurd_lists(*shape, len(cube), cube.shape[1], len(positions), positions.ctypes.data, flux.ctypes.data,
                                   cells.ctypes.data, float(radius), offsets.ctypes.data, index.ctypes.data, room, ctypes.byref(count))
    assert 0 <= total <= room
    return offsets, index[:total], count.value


EmuError, EmuModel = fc.EmuError, fc.EmuModel


class EmuFinder(fp.EmuFinder):
    """fitpos_cases.EmuFinder with ``render``: regularizepsf_amd.stars._Finder's interface on the emulator."""

    def __init__(self, shape, box, device=0) -> None:
        super().__init__(shape, box, device)
        self._rendered = 0

    def render(self, model, positions, flux, cells, radius, mode=RESIDUAL, dtype=np.float32, out=None):
        assert out is None, "the emulator has no device memory"
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        flux = np.ascontiguousarray(flux, np.float64).ravel()
        cells = np.ascontiguousarray(cells, np.int32).ravel()
        if len(cells) != len(positions) or len(flux) != len(positions):
            raise ValueError(f"{len(flux)} fluxes and {len(cells)} cells for {len(positions)} positions")
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError(f"dtype must be float32 or float64, not {dtype}")
        level = None if self._filtered is None else np.ascontiguousarray(self._filtered[0])
        frame = self._frame if self._frame is not None else np.zeros(self.shape, np.float32)
        result, count = np.empty(self.shape, dtype), ctypes.c_long(-1)
        if model.device != self._device:
            raise EmuError(-1, "bad argument")
        no_state = mode != MODEL and not self._have_mesh
        code = emulator().emurd_render(frame.ctypes.data, *self.shape, self.box, None if level is None else level.ctypes.data,
                                       int(level is None or no_state), len(model.values), model.size, model.values.ctypes.data, len(positions),
                                       positions.ctypes.data, flux.ctypes.data, cells.ctypes.data, float(radius), int(mode),
                                       int(dtype == np.float64), result.ctypes.data, ctypes.byref(count))
        if code == -1:
            raise EmuError(-1, "bad argument")
        if no_state or code == -6:  # (the library checks its arguments first, then its state)
            raise EmuError(-6, "render of a residual before background_device, or of a frame without a mesh")
        assert code == 0
        self._rendered = emulator_info()[3]
        return result, count.value

    def render_ms(self) -> float:
        """In the place of the device time: the workgroups of S10 that ran."""
        return float(self._rendered)


# ------------------------------------------------------------------------------------------------------------------ the cases
@functools.cache
def frame(shape=SHAPE) -> np.ndarray:
    """A tilted background with noise, float32, with a NaN, both infinities and a - 0.0 among the pixels."""
    rng = np.random.default_rng([10, 67, *shape])
    rows, cols = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    out = (10.0 + 0.01 * rows - 0.02 * cols + rng.normal(0.0, 0.3, shape)).astype(np.float32)
    out[shape[0] // 2, shape[1] // 3] = np.nan
    out[1, 2], out[shape[0] - 2, shape[1] - 1], out[0, 0] = np.inf, -np.inf, -0.0
    out.flags.writeable = False
    return out


def _case(positions, flux, cells, n, radii=None, shape=SHAPE, cube=None) -> dict:
    positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
    return {"frame": frame(shape), "box": BOX, "n": n, "cube": fc.model(n) if cube is None else cube, "positions": positions,
            "flux": np.ascontiguousarray(np.resize(np.asarray(flux, np.float64), len(positions))),
            "cells": np.ascontiguousarray(np.resize(np.asarray(cells, np.int32), len(positions))),
            "radii": fc.RADII[n] if radii is None else tuple(radii)}


FLUXES = (400.0, -250.0, 300.5, 1e-3, 5e7, 0.0, -0.0)


def _grid_case(n) -> dict:
    """fit_cases.STARS and hard_positions(): pixel centres, half pixels, the rim, partly and wholly off the frame; every kind of cell."""
    return _case(np.concatenate([fc.STARS, fc.hard_positions()]), FLUXES, (GAUSSIAN, LOBES, CONSTANT, ZERO, GAUSSIAN), n)


def _off_frame() -> np.ndarray:
    """Around a frame of SHAPE: partly off at each side and each corner, and wholly off."""
    H, W = SHAPE
    return np.array([(-2.0, 10.0), (H + 1.5, 30.0), (20.0, -3.0), (20.0, W + 2.0), (-1.0, -1.0), (H, W), (-0.5, W - 0.5), (H - 0.5, -0.5),
                     (-20.0, 10.0), (H + 20.0, 10.0), (10.0, -20.0), (10.0, W + 20.0), (-9.0, 35.0), (21.0, W + 8.0), (-8.5, -8.5)])


def _skipped_case() -> dict:
    """Stars that are not drawn among stars that are: NaN and infinite fluxes, cells outside the model."""
    positions = np.repeat(fc.STARS, 2, axis=0)
    flux = (100.0, np.nan, 200.0, np.inf, 300.0, -np.inf, 400.0, 50.0, 500.0, 60.0)
    cells = (GAUSSIAN, GAUSSIAN, LOBES, LOBES, CONSTANT, CONSTANT, GAUSSIAN, -1, LOBES, 4)
    return _case(positions, flux, cells, 9, (3.5,))


def _pile(k: int) -> np.ndarray:
    """k positions inside tile (1, 1) of the emulator's tiling, a little apart from each other."""
    tile_r, tile_c = emulator_info()[:2]
    i = np.arange(k, dtype=np.float64)
    return np.stack([tile_r * 1.5 + 0.37 * np.sin(i), tile_c * 1.5 + 1.9 * np.cos(0.7 * i)], axis=-1)


def _pile_case(chunks: int, extra: int) -> dict:
    k = chunks * emulator_info()[2] + extra
    return _case(_pile(k), 1.0 + np.arange(k) % 7 - 0.125 * (np.arange(k) % 3), (GAUSSIAN, LOBES, CONSTANT), 9, (2.3,))


ORDER_FLUXES = (1e16, 1.0, -1e16, 1.0)


def _order_case() -> dict:
    """More than two chunks of stars at one position with a constant cell: the pixel's value is the sum of the fluxes / 4 in the order
    they are added."""
    k = 2 * emulator_info()[2] + 4
    tile_r, tile_c = emulator_info()[:2]
    return _case(np.tile([(tile_r * 1.5, tile_c * 1.5)], (k, 1)), ORDER_FLUXES, (CONSTANT,), 9, (2.0,))


def _nan_cube() -> np.ndarray:
    cube = np.where(np.arange(4)[:, None, None] == ZERO, np.nan, fc.model(9))  # a cell without a star, as build leaves it
    cube.flags.writeable = False
    return cube


def _corner() -> np.ndarray:
    tile_r, tile_c = emulator_info()[:2]
    return np.array([(tile_r, tile_c), (tile_r - 0.5, tile_c - 0.5), (2 * tile_r, 2 * tile_c), (3 * tile_r - 0.5, tile_c), (tile_r, 2 * tile_c - 0.5)],
                    np.float64)


CASES = {
    **{f"N = {n}": functools.partial(_grid_case, n) for n in (4, 9, 16)},
    "tile corners": lambda: _case(_corner(), FLUXES, (GAUSSIAN, LOBES), 9),
    # a disc of diameter 15 meets at most 3 tile rows and 2 tile columns of 8 x 32 tiles
    "N = 16, R = 7 over six tiles": lambda: _case([(14.0, 31.0), (30.5, 63.5)], (1000.0, -3.0), (LOBES, GAUSSIAN), 16, (7.0,)),
    "a disc over fifteen tiles": lambda: _case([(20.0, 48.0), (21.0, 20.0)], (1000.0, 70.0), (GAUSSIAN, LOBES), 36, (17.0, 16.4)),
    "off the frame": lambda: _case(_off_frame(), FLUXES, (GAUSSIAN, LOBES, CONSTANT), 16, (7.0, 4.6)),
    "skipped stars": _skipped_case,
    "a cell of NaN": lambda: _case(fc.STARS[:3], (100.0, 200.0, 300.0), (GAUSSIAN, ZERO, LOBES), 9, (3.5,), cube=_nan_cube()),
    "no stars": lambda: _case(np.zeros((0, 2)), (), (), 9, (3.5,)),
    "smaller than a tile, N = 4": lambda: _case([(2.0, 3.0), (0.0, 0.0), (4.5, 6.5), (-1.0, 3.0), (9.0, 9.0)], FLUXES, (GAUSSIAN, LOBES), 4, shape=SMALL),
    "smaller than a tile, N = 9": lambda: _case([(2.0, 3.0), (0.0, 0.0), (4.5, 6.5), (-1.0, 3.0), (12.0, 3.0)], FLUXES, (LOBES, CONSTANT), 9, shape=SMALL),
    "a chunk less one": lambda: _pile_case(1, -1),
    "a chunk": lambda: _pile_case(1, 0),
    "a chunk and one": lambda: _pile_case(1, 1),
    "two chunks and one": lambda: _pile_case(2, 1),
    "the order of the sum": _order_case,
}


@functools.cache
def case(name: str) -> dict:
    return sc._freeze(CASES[name]())


@functools.lru_cache(maxsize=None)
def _reference(name: str, mesh_bytes: bytes | None, radius: float, mode: int, dtype) -> np.ndarray:
    c = case(name)
    shape = c["frame"].shape
    level_f = None if mesh_bytes is None else np.frombuffer(mesh_bytes).reshape(-(-shape[0] // c["box"]), -(-shape[1] // c["box"]))
    out = ref_render(c["frame"], c["box"], level_f, c["cube"], c["positions"], c["flux"], c["cells"], radius, mode, dtype)
    out.flags.writeable = False
    return out


def reference(name: str, level_f, radius: float, mode: int, dtype) -> np.ndarray:
    """The restatement's frame for the case on the filtered mesh `level_f`, computed once per case, mesh, radius, mode and dtype."""
    mesh = None if mode != RESIDUAL_MESH else np.ascontiguousarray(level_f).tobytes()
    return _reference(name, mesh, float(radius), int(mode), np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def reach(name: str, radius: float) -> np.ndarray:
    c = case(name)
    return ref_sum(c["frame"].shape, c["cube"], c["positions"], c["flux"], c["cells"], radius)[1]


# ------------------------------------------------------------------------------------------------------------------ the checks
def run(make_finder, make_model, c: dict, times: list | None = None) -> tuple:
    """The product's per-frame route on a finder: (the filtered mesh, {(radius, mode, dtype name): (frame, stars drawn)})."""
    finder, model = make_finder(c["frame"].shape, c["box"]), None
    try:
        model = make_model(c["cube"])
        level, rms = finder.background(c["frame"], None)  # the raw mesh of the finder under test (photometry_cases, THE MESH)
        filtered = stars.filter_mesh(level, rms)
        finder.background_device(c["frame"], None)
        frames = {}
        for radius in c["radii"]:
            for mode in MODES:
                for dtype in DTYPES:
                    frames[radius, mode, np.dtype(dtype).name] = finder.render(model, c["positions"], c["flux"], c["cells"], radius, mode, dtype)
                    if times is not None:
                        times.append(finder.render_ms())
        return filtered[0], frames
    finally:
        if model is not None:
            model.close()
        finder.close()


def check_case(make_finder, make_model, name: str) -> dict:
    """Checks 1 and 3: every frame of every radius, mode and dtype of the case against the restatement, bit for bit; the stars drawn; a
    pixel outside every disc is the input's bits (RESIDUAL) or + 0.0 (MODEL).  Returns {(radius, mode, dtype name): frame}."""
    c = case(name)
    level_f, frames = run(make_finder, make_model, c)
    want_drawn = int(drawn(c["flux"], c["cells"], len(c["cube"])).sum())
    for (radius, mode, dtype), (got, count) in frames.items():
        want = reference(name, level_f, radius, mode, dtype)
        differ = int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want))))) if got.shape == want.shape else -1
        if mode == MODEL and dtype == "float64":
            print(f"{name}, R = {radius:g}: {len(c['positions'])} stars, {count} drawn, {int(reach(name, radius).sum())} of {got.size} pixels "
                  f"reached, {int(np.isnan(want).sum())} NaN")
        assert count == want_drawn, (name, count, want_drawn)
        assert same_frame(got, want), (name, radius, mode, dtype, differ)
        outside = ~reach(name, radius)
        if mode == MODEL:
            assert got[outside].tobytes() == np.zeros(int(outside.sum()), got.dtype).tobytes(), (name, radius, dtype)
        elif mode == RESIDUAL:
            assert got[outside].tobytes() == c["frame"][outside].astype(got.dtype).tobytes(), (name, radius, dtype)
    return {key: got for key, (got, _) in frames.items()}


def check_lists(name: str) -> None:
    """Check 2: the host's tile lists of the case.  Offsets start at 0, never fall and end at the length of the index array; a tile's
    indices ascend strictly (so there are no duplicates); no star that is not drawn is on a list; and every (star, pixel) pair with q <=
    R R has the star on the list of the pixel's tile."""
    c = case(name)
    H, W = c["frame"].shape
    tile_r, tile_c = emulator_info()[:2]
    across = -(-W // tile_c)
    keep = drawn(c["flux"], c["cells"], len(c["cube"]))
    rows, cols = np.mgrid[0:H, 0:W]
    tile_of = (rows // tile_r) * across + cols // tile_c
    for radius in c["radii"]:
        offsets, index, count = tile_lists((H, W), c["cube"], c["positions"], c["flux"], c["cells"], radius)
        assert offsets[0] == 0 and np.all(np.diff(offsets) >= 0) and offsets[-1] == len(index) and count == int(keep.sum())
        lists = [index[a:b] for a, b in zip(offsets[:-1], offsets[1:])]
        assert all(np.all(np.diff(one) > 0) for one in lists)
        assert np.all(keep[index]) and (len(index) == 0 or (index.min() >= 0 and index.max() < len(keep)))
        R2 = np.float64(radius) * np.float64(radius)
        pairs = 0
        for i, (y, x) in enumerate(c["positions"]):
            if not keep[i]:
                continue
            pr, pc_ = rows.astype(np.float64) - y, cols.astype(np.float64) - x
            for t in np.unique(tile_of[(pr * pr + pc_ * pc_) <= R2]):
                assert i in lists[t], (name, radius, i, t)
                pairs += 1
        print(f"{name}, R = {radius:g}: {len(lists)} tiles, {len(index)} list entries, {pairs} (star, tile) pairs needed, longest list "
              f"{max((len(one) for one in lists), default=0)}")


def check_nan_cell(make_finder, make_model) -> None:
    """A star with a cell of NaN: the pixels of its disc are NaN and no other pixel is."""
    c = case("a cell of NaN")
    frames = check_case(make_finder, make_model, "a cell of NaN")
    y, x = c["positions"][1]
    rows, cols = np.mgrid[0:SHAPE[0], 0:SHAPE[1]].astype(np.float64)
    disc = ((rows - y) * (rows - y) + (cols - x) * (cols - x)) <= 3.5 * 3.5
    assert disc.sum() > 30
    assert np.array_equal(np.isnan(frames[3.5, MODEL, "float64"]), disc)
    assert np.array_equal(np.isnan(frames[3.5, RESIDUAL, "float32"]), disc | np.isnan(c["frame"]))


def check_skipped(make_finder, make_model) -> None:
    """Stars with a NaN or infinite flux or a cell outside the model are counted out, and the frame is the one without them."""
    c = case("skipped stars")
    keep = drawn(c["flux"], c["cells"], len(c["cube"]))
    assert keep.sum() == 5 and len(keep) == 10
    frames = check_case(make_finder, make_model, "skipped stars")
    finder, model = make_finder(SHAPE, BOX), make_model(c["cube"])
    try:
        finder.background_device(c["frame"], None)
        for mode in (MODEL, RESIDUAL):
            got, count = finder.render(model, c["positions"][keep], c["flux"][keep], c["cells"][keep], 3.5, mode, np.float64)
            assert count == 5 and same_frame(got, frames[3.5, mode, "float64"])
    finally:
        model.close()
        finder.close()


def check_order(make_finder, make_model) -> None:
    """The order case: first, in NumPy alone, the fluxes added in descending index give other bits than in ascending index; then the
    kernel's pixel is the ascending sum (check_case holds the whole frame to the ascending restatement)."""
    c = case("the order of the sum")
    terms = c["flux"] * 0.25  # the constant cell: m = 0.25 at every pixel of the disc, exactly
    up = down = np.float64(0.0)
    for t in terms:
        up = up + t
    for t in terms[::-1]:
        down = down + t
    assert up.tobytes() != down.tobytes(), "the order case does not tell the orders apart"
    frames = check_case(make_finder, make_model, "the order of the sum")
    y, x = (int(v) for v in c["positions"][0])
    got = frames[2.0, MODEL, "float64"][y, x]
    print(f"the order of the sum: {len(terms)} stars on pixel ({y}, {x}): ascending {up!r}, descending {down!r}, the kernel {got!r}")
    assert got.tobytes() == up.tobytes() and got.tobytes() != down.tobytes()


def check_chunks(make_finder, make_model) -> None:
    """Chunk - 1, chunk, chunk + 1 and 2 chunk + 1 stars on one tile's list."""
    chunk = emulator_info()[2]
    tile_r, tile_c = emulator_info()[:2]
    across = -(-SHAPE[1] // tile_c)
    for name, k in (("a chunk less one", chunk - 1), ("a chunk", chunk), ("a chunk and one", chunk + 1), ("two chunks and one", 2 * chunk + 1)):
        c = case(name)
        offsets, _, count = tile_lists(SHAPE, c["cube"], c["positions"], c["flux"], c["cells"], c["radii"][0])
        assert count == k and offsets[across + 2] - offsets[across + 1] == k, (name, k)  # all of them on tile (1, 1)
        check_case(make_finder, make_model, name)


def isolated() -> dict:
    """fit_cases' field (48 x 40, five stars at least 14 px apart) and its 9-pixel model: every disc of R = 3.5 is on the frame and apart
    from the others."""
    return {"frame": fc.field()["frame"].astype(np.float32), "positions": fc.STARS.copy(),
            "cells": np.array([GAUSSIAN, LOBES, GAUSSIAN, LOBES, GAUSSIAN], np.int32), "cube": fc.model(9), "radius": 3.5, "box": fc.BOX}


def check_tie_to_fit(make_finder, make_model) -> None:
    """Check 4: with isolated stars, fit_background off and float64 output, in the mode of the fit's background: the residual at each
    star's (peak_row, peak_col) is fit's peak_e bit for bit, and over the disc it is e = d - (f m + 0.0): s = 0.0 + f m has the same
    bits."""
    t = isolated()
    finder, model = make_finder(t["frame"].shape, t["box"]), make_model(t["cube"])
    try:
        level, rms = finder.background(t["frame"], None)
        level_f = stars.filter_mesh(level, rms)[0]
        finder.background_device(t["frame"], None)
        rows, cols = np.mgrid[0:t["frame"].shape[0], 0:t["frame"].shape[1]]
        for use_mesh, mode in ((False, RESIDUAL), (True, RESIDUAL_MESH)):
            fits = finder.fit(model, t["positions"], t["cells"], t["radius"], False, use_mesh)
            assert np.all(fits[:, fc.FLAGS] == 0) and np.all(fits[:, fc.N_USE] == fits[:, fc.N_ALL])
            residual, count = finder.render(model, t["positions"], fits[:, fc.F], t["cells"], t["radius"], mode, np.float64)
            assert count == len(fits)
            d, _ = pc.ref_residual(t["frame"], None, t["box"], level_f, "mesh" if use_mesh else "none")
            for (y, x), k, row in zip(t["positions"], t["cells"], fits):
                at = int(row[fc.PEAK_ROW]), int(row[fc.PEAK_COL])
                assert residual[at].tobytes() == row[fc.PEAK_E].tobytes(), (use_mesh, at, residual[at], row[fc.PEAK_E])
                pr, pc_ = rows[:, 0].astype(np.float64) - y, cols[0].astype(np.float64) - x
                disc = ((pr * pr)[:, None] + (pc_ * pc_)[None, :]) <= np.float64(t["radius"]) ** 2
                m = fc.ref_model(t["cube"][k], pr, pc_, disc)
                e = d - (row[fc.F] * m + 0.0)
                assert residual[disc].tobytes() == e[disc].tobytes(), (use_mesh, y, x)
                assert np.abs(e[disc]).max() == row[fc.PEAK_RES]
            print(f"the tie to S8, {'mesh' if use_mesh else 'none'}: {len(fits)} stars, peak_e {fits[:, fc.PEAK_E]}")
    finally:
        model.close()
        finder.close()


ROUND_TRIP_FLUX = np.array([1000.0, 37.5, 2.0e5, 0.125, 640.25])
U32 = 2.0 ** -24  # the relative error of one rounding to float32, away from the subnormals


def check_round_trip(make_finder, make_model) -> None:
    """Check 5, on the finder: a float32 model frame of isolated stars, fitted by S8 without a background, returns each flux within (2^-24
    + 1e-12) |flux|: every pixel of a disc is flux x m rounded once to float32 (relative error <= 2^-24; the case asserts that none is
    subnormal), the estimator sum d m / sum m m is a mean of d / m with the positive weights m m, and 1e-12 covers the float64 sums of
    some fifty terms.  The residual of that frame with the true fluxes is at most 2^-24 |s| per pixel (the subtraction of two doubles that
    close is exact), times 1 + 2^-24 for a float32 output."""
    t = isolated()
    shape = t["frame"].shape
    finder, model = make_finder(shape, t["box"]), make_model(t["cube"])
    try:
        drawn_frame, count = finder.render(model, t["positions"], ROUND_TRIP_FLUX, t["cells"], t["radius"], MODEL, np.float32)
        s, reached = ref_sum(shape, t["cube"], t["positions"], ROUND_TRIP_FLUX, t["cells"], t["radius"])
        assert count == 5 and drawn_frame.dtype == np.float32
        tiny = float(np.finfo(np.float32).tiny)
        assert np.all((s == 0.0) | (np.abs(s) >= 2 * tiny)), "a pixel of the round trip is subnormal in float32"
        finder.background_device(drawn_frame, None)
        fits = finder.fit(model, t["positions"], t["cells"], t["radius"], False, False)
        error = np.abs(fits[:, fc.F] - ROUND_TRIP_FLUX) / np.abs(ROUND_TRIP_FLUX)
        print(f"round trip: relative flux errors {error} (the bound: {U32 + 1e-12:.3e})")
        assert np.all(fits[:, fc.FLAGS] == 0) and np.all(error <= U32 + 1e-12)
        for dtype, slack in ((np.float64, 1.0), (np.float32, 1.0 + U32)):
            residual = finder.render(model, t["positions"], ROUND_TRIP_FLUX, t["cells"], t["radius"], RESIDUAL, dtype)[0]
            ratio = np.abs(residual[reached].astype(np.float64)) / np.maximum(np.abs(s[reached]), tiny)
            print(f"round trip, {np.dtype(dtype).name} residual: max |res| / |s| = {ratio.max():.3e} (the bound: {U32 * slack:.3e})")
            assert np.all(np.abs(residual.astype(np.float64)) <= U32 * slack * np.abs(s)) and np.all(residual[~reached] == 0.0)
    finally:
        model.close()
        finder.close()


def check_reproducible(make_finder, make_model, name: str) -> None:
    """Check 8: two runs of a case give the same bytes, on one finder and on a fresh one."""
    c = case(name)
    first = run(make_finder, make_model, c)[1]
    again = run(make_finder, make_model, c)[1]
    for key, (got, count) in first.items():
        assert got.tobytes() == again[key][0].tobytes() and count == again[key][1], (name, key)


def check_isolation(make_finder, make_model) -> None:
    """Check 9: detect, measure, photometry, refine, fit and fit_positions give the bits they gave before a render, and a render's frame
    does not depend on them; one model serves two finders."""
    c = fp.case("N = 9, mesh, flux and background")
    radii = (2.0, 4.0)
    finder, model_ = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"])
    other = make_finder(c["frame"].shape, 8)
    try:
        finder.background_device(c["frame"], c["mask"])
        rows = finder.detect_device(3.0, 5, None)
        shapes = finder.measure()
        phot = finder.photometry(rows[:, :2], radii, 5, True)
        refined = finder.refine(rows[:, :2], 1.5)
        assert len(rows) == 5
        cells = np.zeros(len(rows), np.int32)
        fits = finder.fit(model_, rows[:, :2], cells, 3.5)
        steps, at_end = finder.fit_positions(model_, rows[:, :2], cells, 3.5)
        frames = [finder.render(model_, rows[:, :2], fits[:, fc.F], cells, 3.5, mode, np.float64)[0] for mode in MODES]
        assert finder.render_ms() > 0.0
        assert finder.measure().tobytes() == shapes.tobytes()
        assert finder.photometry(rows[:, :2], radii, 5, True).tobytes() == phot.tobytes()
        assert finder.refine(rows[:, :2], 1.5).tobytes() == refined.tobytes()
        assert finder.fit(model_, rows[:, :2], cells, 3.5).tobytes() == fits.tobytes()
        again = finder.fit_positions(model_, rows[:, :2], cells, 3.5)
        assert again[0].tobytes() == steps.tobytes() and again[1].tobytes() == at_end.tobytes()
        finder.render(model_, c["positions"], np.ones(len(c["positions"])), c["cells"], 1.0, MODEL, np.float32)
        assert finder.measure().tobytes() == shapes.tobytes()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes()
        for mode, before in zip(MODES, frames):
            assert finder.render(model_, rows[:, :2], fits[:, fc.F], cells, 3.5, mode, np.float64)[0].tobytes() == before.tobytes()
        finder.background_device(c["frame"], c["mask"])  # render first, the others after it
        for mode, before in zip(MODES, frames):
            assert finder.render(model_, rows[:, :2], fits[:, fc.F], cells, 3.5, mode, np.float64)[0].tobytes() == before.tobytes()
        assert finder.detect_device(3.0, 5, None).tobytes() == rows.tobytes() and finder.measure().tobytes() == shapes.tobytes()
        assert finder.photometry(rows[:, :2], radii, 5, True).tobytes() == phot.tobytes()
        assert finder.refine(rows[:, :2], 1.5).tobytes() == refined.tobytes()
        assert finder.fit(model_, rows[:, :2], cells, 3.5).tobytes() == fits.tobytes()
        other.background_device(c["frame"], c["mask"])  # the same model on a second finder, with another mesh
        elsewhere = other.render(model_, rows[:, :2], fits[:, fc.F], cells, 3.5, RESIDUAL, np.float64)[0]
        assert elsewhere.tobytes() == frames[RESIDUAL].tobytes()  # (RESIDUAL does not read the mesh)
        assert other.render(model_, rows[:, :2], fits[:, fc.F], cells, 3.5, RESIDUAL_MESH, np.float64)[0].tobytes() != frames[RESIDUAL_MESH].tobytes()
        assert finder.render(model_, rows[:, :2], fits[:, fc.F], cells, 3.5, MODEL, np.float64)[0].tobytes() == frames[MODEL].tobytes()
    finally:
        model_.close()
        other.close()
        finder.close()


def check_errors(make_finder, make_model, error: type) -> None:
    """RPSF_E_STATE (-6) for a residual before a background_device of a frame, after the host route's detect, and for RESIDUAL_MESH on a
    frame without a usable pixel; MODEL needs no state; RPSF_E_BADARG (-1) for a bad radius, mode or position, whatever the state."""
    import pytest

    c = case("N = 9")
    p, f, k = c["positions"][:6], c["flux"][:6], c["cells"][:6]
    finder, model_, small = make_finder(c["frame"].shape, c["box"]), make_model(c["cube"]), make_model(fc.model(4))
    good = (model_, p, f, k, 3.5, RESIDUAL, np.float32)

    def but(**changes):
        names = ("model", "positions", "flux", "cells", "radius", "mode", "dtype")
        return tuple(changes.get(name, value) for name, value in zip(names, good))

    bad = [but(radius=r) for r in (0.0, -1.0, np.nan, np.inf, 3.5000001, 64.5)] + [but(model=small, radius=1.0000001)]
    bad += [but(mode=m) for m in (-1, 3)]
    bad += [but(positions=[(np.nan, 1.0)], flux=[1.0], cells=[0]), but(positions=[(1.0, np.inf)], flux=[1.0], cells=[0]),
            but(positions=[(2.0 ** 20, 1.0)], flux=[1.0], cells=[0]),
            but(positions=[(1.0, 1.0), (1.0, -2.0 ** 20)], flux=[1.0, 1.0], cells=[0, 0], mode=MODEL)]
    try:
        def refused(args, code):
            with pytest.raises(error) as caught:
                finder.render(*args)
            assert caught.value.code == code, (args[4:], caught.value.code)

        refused(good, -6)
        refused(but(mode=RESIDUAL_MESH), -6)
        model_frame = finder.render(*but(mode=MODEL))[0]  # no state beyond the shape
        for args in bad:
            refused(args, -1)
        level, rms = finder.background(c["frame"], None)  # the host route: no S1b mesh on the device
        refused(good, -6)
        finder.background_device(c["frame"], None)
        for args in bad:
            refused(args, -1)
        residual = finder.render(*good)[0]
        assert finder.render(*but(mode=MODEL))[0].tobytes() == model_frame.tobytes()
        assert finder.render(*but(positions=[(2.0 ** 20 - 1, 1.0 - 2.0 ** 20)], flux=[1.0], cells=[0]))[1] == 1  # the largest admitted
        assert finder.render(*but(model=small, radius=1.0))[0].shape == c["frame"].shape
        level_f, _, global_rms = stars.filter_mesh(level, rms)
        finder.detect(level_f, 3.0 * global_rms, 5, None)  # the host route's detect replaces the mesh on the device
        refused(good, -6)
        finder.background_device(np.full(c["frame"].shape, np.nan, np.float32), None)  # no usable pixel: no mesh
        refused(but(mode=RESIDUAL_MESH), -6)
        assert np.all(np.isnan(finder.render(*good)[0]))
        finder.background_device(c["frame"], None)
        assert finder.render(*good)[0].tobytes() == residual.tobytes()
    finally:
        model_.close()
        small.close()
        finder.close()


def check_python_errors(subtract_stars, render_stars) -> None:
    """Check 10: what the public functions refuse before anything runs."""
    import pytest

    from regularizepsf_amd.util import IndexedCube

    image = np.zeros(SHAPE, np.float32)
    psf = IndexedCube([(0, 0), (0, 35)], np.ascontiguousarray(fc.model(9)[[GAUSSIAN, LOBES]]))
    pos = fc.STARS[:3]
    with pytest.raises(ValueError, match="flux"):
        subtract_stars(image, pos, psf, 3.5)  # plain positions need flux=
    with pytest.raises(ValueError, match="flux"):
        subtract_stars(image, pos, psf, 3.5, flux=[np.ones(2)])
    with pytest.raises(ValueError, match="cells"):
        subtract_stars(image, pos, psf, 3.5, flux=[np.ones(3)], cells=[np.zeros(4, np.int32)])
    with pytest.raises(TypeError, match="cells"):
        subtract_stars(image, pos, psf, 3.5, flux=[np.ones(3)], cells=[np.zeros(3)])
    with pytest.raises(ValueError, match="frames"):
        subtract_stars(image, [pos, pos], psf, 3.5, flux=[np.ones(3), np.ones(3)])
    with pytest.raises(ValueError, match="radius"):
        subtract_stars(image, pos, psf, 3.5000001, flux=[np.ones(3)])
    with pytest.raises(ValueError, match="radius"):
        render_stars(SHAPE, pos, [np.ones(3)], psf, 0.0)
    with pytest.raises(ValueError, match="background"):
        subtract_stars(image, pos, psf, 3.5, flux=[np.ones(3)], background="median")
    with pytest.raises(TypeError, match="dtype"):
        subtract_stars(image, pos, psf, 3.5, flux=[np.ones(3)], dtype=np.float16)
    with pytest.raises(TypeError, match="dtype"):
        render_stars(SHAPE, pos, [np.ones(3)], psf, 3.5, dtype=np.int32)
    with pytest.raises(ValueError, match="position"):
        render_stars(SHAPE, np.array([(np.nan, 1.0)]), [np.ones(1)], psf, 3.5)
    with pytest.raises(ValueError, match="flux"):
        render_stars(SHAPE, pos, [np.ones(4)], psf, 3.5)
    with pytest.raises(TypeError, match="DeviceArray"):
        render_stars(SHAPE, pos, [np.ones(3)], psf, 3.5, out=np.zeros(SHAPE, np.float32))


def check_public_round_trip(render_stars, fit_stars, subtract_stars) -> None:
    """Check 5 through the public functions: render_stars' float32 frame, fitted by fit_stars(background="none", fit_background=False),
    gives the fluxes back within (2^-24 + 1e-12) |flux|, and subtract_stars with the true fluxes leaves at most 2^-24 |s| per pixel (times
    1 + 2^-24 in float32) - check_round_trip derives both bounds."""
    from regularizepsf_amd.util import IndexedCube

    t = isolated()
    shape = t["frame"].shape
    psf = IndexedCube([(0, 0), (0, 20), (20, 0), (20, 20)], np.ascontiguousarray(t["cube"]))
    frames = render_stars(shape, [t["positions"]], [ROUND_TRIP_FLUX], psf, t["radius"], cells=[t["cells"]])
    assert len(frames) == 1 and frames[0].dtype == np.float32 and frames[0].shape == shape
    s, reached = ref_sum(shape, t["cube"], t["positions"], ROUND_TRIP_FLUX, t["cells"], t["radius"])
    assert np.all((s == 0.0) | (np.abs(s) >= 2 * float(np.finfo(np.float32).tiny))), "a pixel of the round trip is subnormal in float32"
    assert same_frame(frames[0], s.astype(np.float32))
    fits = fit_stars(frames[0], t["positions"], psf, t["radius"], background="none", fit_background=False, cells=[t["cells"]], box=t["box"])
    error = np.abs(fits[0]["flux"] - ROUND_TRIP_FLUX) / np.abs(ROUND_TRIP_FLUX)
    print(f"round trip through the package: relative flux errors {error} (the bound: {U32 + 1e-12:.3e})")
    assert np.all(fits[0]["flags"] == 0) and np.all(error <= U32 + 1e-12)
    for dtype, slack in ((np.float64, 1.0), (np.float32, 1.0 + U32)):
        residual, counts = subtract_stars(frames[0], t["positions"], psf, t["radius"], flux=[ROUND_TRIP_FLUX], cells=[t["cells"]], dtype=dtype,
                                          box=t["box"], return_counts=True)
        assert counts == [5] and residual[0].dtype == dtype
        assert np.all(np.abs(residual[0].astype(np.float64)) <= U32 * slack * np.abs(s)) and np.all(residual[0][~reached] == 0.0)


def check_composition(fit_positions, subtract_stars) -> None:
    """Check 6 on fit_cases.truth_case(): fit_positions -> subtract_stars draws every star with the `cell` field it was fitted with; the
    same frames come from cells= given explicitly and from plain arrays with flux= and cells=."""
    t = fc.truth_case()
    frames = t["frames"].astype(np.float32)
    coordinates, values = fc.oracle_model()
    psf = _Psf(coordinates, values)
    fitted = fit_positions(frames, [p + (0.3, -0.2) for p in t["truth"]], psf, fc.TRUTH_RADIUS, background="none", box=fc.BOX,
                           cells=[stars.nearest_cells(p, coordinates, fc.TRUTH_N) for p in t["truth"]])
    assert all(np.all(f["fit_flags"] == 0) for f in fitted)
    for background in ("none", "mesh"):
        for dtype in DTYPES:
            by_field, models, counts = subtract_stars(frames, fitted, psf, fc.TRUTH_RADIUS, background=background, box=fc.BOX, dtype=dtype,
                                                      return_model=True, return_counts=True)
            explicit = subtract_stars(frames, fitted, psf, fc.TRUTH_RADIUS, background=background, box=fc.BOX, dtype=dtype,
                                      cells=[f["cell"] for f in fitted])
            plain = subtract_stars(frames, [np.stack([f["row"], f["col"]], axis=-1) for f in fitted], psf, fc.TRUTH_RADIUS,
                                   background=background, box=fc.BOX, dtype=dtype, flux=[f["flux"] for f in fitted],
                                   cells=[f["cell"] for f in fitted])
            assert counts == [5, 5, 5] and len(by_field) == len(models) == 3
            for a, b, c_, m in zip(by_field, explicit, plain, models):
                assert a.dtype == dtype and a.shape == fc.TRUTH_SHAPE and a.tobytes() == b.tobytes() == c_.tobytes() and m.dtype == dtype
    residual, models = subtract_stars(frames, fitted, psf, fc.TRUTH_RADIUS, dtype=np.float64, return_model=True)
    for frame, res, model, f in zip(frames, residual, models, fitted):
        assert np.array_equal(res, frame.astype(np.float64) - model)  # one subtraction of the same s
        inside = model != 0.0
        left = np.abs(res - f["background"].mean())[inside].sum() / np.abs(model[inside]).sum()
        print(f"composition: |residual - fitted constant| / |model| over the discs = {left:.4f} (fit_stars' residual_fraction there: "
              f"{np.median(f['residual_fraction']):.4f})")
    # a frame's array for a single frame, and the nearest cell when the stars carry none
    one = subtract_stars(frames[0], fitted[0], psf, fc.TRUTH_RADIUS, box=fc.BOX)
    assert len(one) == 1 and one[0].tobytes() == subtract_stars(frames, fitted, psf, fc.TRUTH_RADIUS, box=fc.BOX)[0].tobytes()
    nearest = subtract_stars(frames[0], np.stack([fitted[0]["row"], fitted[0]["col"]], axis=-1), psf, fc.TRUTH_RADIUS, box=fc.BOX,
                             flux=[fitted[0]["flux"]])
    assert nearest[0].tobytes() == subtract_stars(frames[0], fitted[0], psf, fc.TRUTH_RADIUS, box=fc.BOX, cells=[
        stars.nearest_cells(np.stack([fitted[0]["row"], fitted[0]["col"]], axis=-1), coordinates, fc.TRUTH_N)])[0].tobytes()


class _Psf:
    """What model_cube needs of an ArrayPSF: coordinates and values."""

    def __init__(self, coordinates, values) -> None:
        self.coordinates, self.values = coordinates, values
