"""The tables a plan uploads at creation (regularizepsf_amd/csrc/rpsf_lattice.hpp), checked on the CPU.

A fused or persistent launch at N = 128 / 256 waits on counters whose targets, tile order and slot order are these tables: a wrong one is a
wait that never ends, so they are checked here before any GPU run.  Three parts:
  1. byte for byte the tables of tests/golden/lattice_tables.npz, which the previous host code (setup_lattice / ensure_bands of rpsf.hip,
     text unchanged, compiled over stubs that keep what would be uploaded) produced for tests/lattice_cases.py: speed depends on these orders;
  2. the properties the kernels rely on, over a grid of lattice shapes, full and thinned, written without the builder's loops;
  3. launch() of tests/local_parity_cases.py, which labels the GPU cases, against the C++ geometry predicates.
"""

import ctypes
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from oracle import regpsf_oracle as orc
from tests.helpers import KERNEL_PAD_MODES
from tests.lattice_cases import BAND_CASES, GOLDEN_CASES, GRID_N, GRID_NLI, GRID_NLJ, MAX_BANDS, SCALARS, TABLES, lattice, thinned
from tests.local_parity_cases import ISOLATION_CASES, ROUTE_CASES, SECOND_CASES, launch

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "emu" / "emu_lattice.cpp"
LIB = ROOT / "tests" / "emu" / "libemu_lattice.so"
DEPS = [ROOT / "regularizepsf_amd" / "csrc" / "rpsf_lattice.hpp", ROOT / "regularizepsf_amd" / "csrc" / "rpsf_core.hpp", ROOT / "include" / "rpsf.h"]
GOLDEN = ROOT / "tests" / "golden" / "lattice_tables.npz"
MODES = {"constant": 0, "symmetric": 1, "reflect": 2, "edge": 3, "wrap": 4}
TEAMS = {256: 1, 128: 1, 64: 2, 32: 8, 16: 32}  # patches per workgroup of the patch kernels
QUAD_SIDE, QUAD_DIRECT = 1, 2
VP = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists() or LIB.stat().st_mtime < max([SRC.stat().st_mtime] + [d.stat().st_mtime for d in DEPS]):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++")
        if clang is None:
            pytest.skip("no clang++ to build the emulator")
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(LIB), str(SRC)], check=True)
    so = ctypes.CDLL(str(LIB))
    so.emu_lattice_fetch.restype = so.emu_lattice_bands_fetch.restype = ctypes.c_int64
    return so


def _fetch(fn, which, dtype, cols=0):
    size = fn(which, None)
    assert size >= 0
    a = np.zeros(size // np.dtype(dtype).itemsize, dtype)
    fn(which, a.ctypes.data_as(VP))
    return a.reshape(-1, cols) if cols else a


def _build(lib, n, coords, k_index=None, parent=None):
    c = np.ascontiguousarray(coords, np.int32)
    s = np.zeros(16, np.int64)
    lib.emu_lattice_build(n, len(c), c.ctypes.data_as(VP), None if k_index is None else k_index.ctypes.data_as(VP), int(n >= 128),
                          None if parent is None else parent.ctypes.data_as(VP), s.ctypes.data_as(VP))
    t = {name: _fetch(lib.emu_lattice_fetch, which, dtype, cols) for name, (which, dtype, cols) in TABLES.items()}
    t["cell"] = _fetch(lib.emu_lattice_fetch, 8, np.int32)
    t["scalars"] = s
    t.update(zip(SCALARS[:7], (int(v) for v in s[:7])))
    t["prefetch_first"] = s[7:]
    return t


def _bands(lib, n, coords, h, want):
    c = np.ascontiguousarray(coords, np.int32)
    b = lib.emu_lattice_bands(n, len(c), c.ctypes.data_as(VP), h, want, MAX_BANDS)
    if not b:
        return 0, None, None, []
    return (b, _fetch(lib.emu_lattice_bands_fetch, 0, np.int32), _fetch(lib.emu_lattice_bands_fetch, 1, np.int32),
            [_fetch(lib.emu_lattice_bands_fetch, 2 + i, np.int32) for i in range(b)])


# ---- 1. the recorded tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_tables_are_the_recorded_ones_byte_for_byte(lib, name):
    golden = np.load(GOLDEN)
    n, coords, k_index, parent = GOLDEN_CASES[name]
    t = _build(lib, n, coords, k_index, parent)
    assert np.array_equal(t["scalars"], golden[f"{name}.scalars"]), dict(zip(SCALARS, zip(t["scalars"], golden[f"{name}.scalars"])))
    for table in TABLES:
        want = golden[f"{name}.{table}"]
        assert t[table].dtype == want.dtype and np.array_equal(t[table], want), table


@pytest.mark.parametrize("name", sorted(BAND_CASES))
def test_row_bands_are_the_recorded_ones(lib, name):
    golden = np.load(GOLDEN)
    n, coords, h, want = BAND_CASES[name]
    b, cut, in_rows, patches = _bands(lib, n, coords, h, want)
    assert b == int(golden[f"{name}.B"][0])
    if b:
        assert np.array_equal(cut, golden[f"{name}.cut"]) and np.array_equal(in_rows, golden[f"{name}.in_rows"])
        for i in range(b):
            assert np.array_equal(patches[i], golden[f"{name}.patches{i}"]), i


def test_the_recorded_cases_take_the_branches_they_are_there_for():
    golden = np.load(GOLDEN)
    lattice_of = {name: int(golden[f"{name}.scalars"][0]) for name in GOLDEN_CASES}
    assert lattice_of == {name: int(name not in ("n64_moved", "n64_twice")) for name in GOLDEN_CASES}
    assert (golden["n128_5x9_holes.cover"] == 0).sum() == 1  # the tile only cell (0, 0) would cover
    assert set(golden["n128_view.desc"][:, 3]) == {0, 1, 2, 3} and golden["n128_view.desc"][:, 2].max() == 4 * 9 - 1
    assert not golden["n64_moved.desc"][:, 3].any() and golden["n64_moved.cover"].size == 0
    assert golden["n32_2x2.sweep_slot"].size == 4 and golden["n64_5x9.quads"].size == 0
    assert int(golden["bands_three_rows.B"][0]) == 0 and int(golden["bands_n256_want8.B"][0]) == 8


# ---- 2. the properties the kernels rely on -------------------------------------------------------------------------------------------------
def _check_tables(n, coords, t, k_index=None, par=(0, 0)):
    """Every table of a lattice from the corner list alone (NumPy over whole arrays; none of the builder's loops)."""
    coords = np.asarray(coords, np.int64)
    count, half, v2, direct = len(coords), n // 2, n >= 128, n >= 128
    (r0, c0), (r1, c1) = coords.min(0), coords.max(0)
    li, lj = (coords[:, 0] - r0) // half, (coords[:, 1] - c0) // half
    nli, nlj = int(li.max()) + 1, int(lj.max()) + 1
    nti, ntj = nli + 1, nlj + 1
    assert (t["lattice"], t["direct_ok"], t["r0"], t["c0"], t["nti"], t["ntj"]) == (1, int(direct), r0, c0, nti, ntj)
    grid = np.full((nli, nlj), -1, np.int64)
    grid[li, lj] = np.arange(count)
    assert np.array_equal(t["cell"], grid.ravel())
    colour = 2 * ((li + par[0]) & 1) + ((lj + par[1]) & 1)
    chunk = -(-(-(-count // 8)) // TEAMS[n]) * TEAMS[n]  # an eighth of the patches, in whole workgroups
    order = t["order"].astype(np.int64)

    # order: a permutation; desc: corner, K index and colour of the patch in each slot
    assert np.array_equal(np.sort(order), np.arange(count))
    k_of = np.arange(count) if k_index is None else np.asarray(k_index, np.int64)
    assert np.array_equal(t["desc"], np.column_stack([coords[order], k_of[order], colour[order]]))
    # the walk: column strips about 8 patches wide; in a strip the upper half of the rows top-down, then the lower half bottom-up;
    # inside each chunk of it the rim patches first (last at N = 256), nothing else moved
    strips = max(4, nlj // 8) if nlj >= 8 else 1
    strip = np.searchsorted(nlj * np.arange(1, strips + 1) // strips, lj, side="right")
    mid = (nli + 1) // 2
    walk = np.lexsort((lj, np.where(li < mid, li, mid + nli - 1 - li), strip))
    rim = (coords[:, 0] == r0) | (coords[:, 0] == r1) | (coords[:, 1] == c0) | (coords[:, 1] == c1)
    for lo in range(0, count, chunk):
        got, was = order[lo:lo + chunk], walk[lo:lo + chunk]
        first = rim[got] if n != 256 else ~rim[got]
        assert not np.any(~first[:-1] & first[1:]), lo  # a prefix (the rim at N != 256, the others at N = 256)
        head = rim[was] if n != 256 else ~rim[was]
        assert np.array_equal(got, np.concatenate([was[head], was[~head]])), lo  # stable
    seq = np.empty(count, np.int64)
    seq[order] = np.arange(count)
    chunk_of = seq // chunk

    # tiles: patch i writes tiles[i, q], q = 2 * (lower half) + (right half)
    q = np.arange(4)
    tiles = (li[:, None] + (q >> 1)) * ntj + lj[:, None] + (q & 1)
    n_tiles = nti * ntj
    cover = np.zeros(n_tiles, np.int64)
    np.bitwise_or.at(cover, tiles, (1 << colour)[:, None])
    contributors = np.bincount(tiles.ravel(), minlength=n_tiles)
    assert np.array_equal(t["cover"], cover)
    assert np.array_equal([bin(int(c)).count("1") for c in t["cover"]], contributors)  # what a summing workgroup waits for

    if v2:
        last = np.full(n_tiles, -1, np.int64)
        np.maximum.at(last, tiles, (seq % chunk)[:, None])
        assert np.array_equal(np.sort(t["sum_order"]), np.arange(n_tiles))
        assert np.all(np.diff(last[t["sum_order"]]) >= 0)
        assert np.array_equal(t["sum_order"], np.argsort(last, kind="stable"))
        first = t["prefetch_first"]
        assert first[0] == 0 and np.all(np.diff(first) >= 0) and first[8] == len(t["prefetch_tiles"])
        for x in range(8):
            touched = tiles[order[x * chunk:(x + 1) * chunk]].ravel()
            _, where = np.unique(touched, return_index=True)
            assert np.array_equal(t["prefetch_tiles"][first[x]:first[x + 1]], touched[np.sort(where)]), x
    else:
        assert t["sum_order"].size == 0 and t["prefetch_tiles"].size == 0 and not t["prefetch_first"].any()

    if direct:
        words = t["quads"].astype(np.int64)  # [slot, q]
        assert np.array_equal(words >> 8, tiles[order])
        mode, rank = words & 3, (words >> 2) & 3
        assert not np.any(words & 0xF0) and np.all((mode == QUAD_SIDE) | (mode == QUAD_DIRECT))
        # a tile's owner: the chunk most of its contributors run in, ties to the chunk of the earliest contributor
        padded = np.full((nli + 2, nlj + 2), -1, np.int64)
        padded[1:-1, 1:-1] = grid
        who = np.stack([padded[1 - a:1 - a + nti, 1 - b:1 - b + ntj] for a in (0, 1) for b in (0, 1)], -1).reshape(n_tiles, 4)
        there = who >= 0
        who_chunk = np.where(there, chunk_of[who], -1)
        who_seq = np.where(there, seq[who], count)
        same = (who_chunk[:, :, None] == who_chunk[:, None, :]) & there[:, :, None] & there[:, None, :]
        members = same.sum(2)
        earliest = np.where(same, who_seq[:, None, :], count).min(2)
        best = np.argmax(np.where(there, members * (count + 1) - earliest, -1), 1)
        owner = np.where(there.any(1), who_chunk[np.arange(n_tiles), best], -1)
        is_direct = chunk_of[order][:, None] == owner[tiles[order]]
        assert np.array_equal(mode == QUAD_DIRECT, is_direct)
        assert not rank[~is_direct].any()
        # direct ranks of a tile: 0 .. k - 1 in processing order (slots ascend along axis 0)
        tile_d, rank_d = tiles[order][is_direct], rank[is_direct]
        by_tile = np.argsort(tile_d, kind="stable")
        tile_d, rank_d = tile_d[by_tile], rank_d[by_tile]
        assert np.array_equal(rank_d, np.arange(len(tile_d)) - np.searchsorted(tile_d, tile_d, side="left"))
        info = np.zeros(n_tiles, np.int64)
        np.bitwise_or.at(info, tiles[order][~is_direct], np.broadcast_to((1 << colour[order])[:, None], is_direct.shape)[~is_direct])
        assert np.array_equal(t["tile_info"], info | 16 * (contributors > 0))
    else:
        assert t["quads"].size == 0 and t["tile_info"].size == 0

    if n <= 64 and nli >= 2 and nlj >= 2 and count == nli * nlj:
        assert np.array_equal(t["sweep_slot"], k_of[grid.ravel()])
    else:
        assert t["sweep_slot"].size == 0


@pytest.mark.parametrize("n", GRID_N)
def test_tables_hold_what_the_kernels_rely_on_over_a_grid_of_lattices(lib, n):
    seed = 0
    for nli in GRID_NLI:
        for nlj in GRID_NLJ:
            seed += 1
            for coords in (lattice(n, nli, nlj), thinned(n, nli, nlj, seed)):
                _check_tables(n, coords, _build(lib, n, coords))


def test_a_view_takes_k_indices_and_colours_from_its_parent(lib):
    n, coords, k_index, parent = GOLDEN_CASES["n128_view"]
    _check_tables(n, coords, _build(lib, n, coords, k_index, parent), k_index, par=(1, 0))


@pytest.mark.parametrize("n", GRID_N)
def test_row_bands_cut_the_frame_and_list_every_patch_that_reaches_in(lib, n):
    half = n // 2
    for nli in GRID_NLI:
        coords = lattice(n, nli, 3)
        h = max(half, nli * half - 3)  # the lattice (origin -N / 2) covers the frame; the last rows are a partial tile
        rows = coords[:, 0].astype(np.int64)
        for want in (0, 1, 2, 3, 4, 8, 20):
            b, cut, in_rows, patches = _bands(lib, n, coords, h, want)
            expect = min(want, MAX_BANDS, nli // 2)  # at least two lattice rows per band
            assert b == (expect if expect >= 2 else 0), (nli, want)
            if not b:
                continue
            assert len(cut) == b + 1 and cut[0] == 0 and cut[-1] == h and np.all(np.diff(cut) > 0)
            for i in range(b):
                mine = np.flatnonzero((rows < cut[i + 1]) & (rows + n > cut[i]))
                assert np.array_equal(patches[i], mine), (nli, want, i)
                assert in_rows[i] == max(min(h, (rows[mine] + n).max()), cut[i + 1])


# ---- 3. the labels of the GPU cases ---------------------------------------------------------------------------------------------------------
LABELLED = sorted({(n, shape) for n, shape, *_ in SECOND_CASES + ROUTE_CASES + ISOLATION_CASES if n >= 128})
FORMS = ("separate plane sum", "fused, one patch per workgroup", "persistent + fused")


@pytest.mark.parametrize(("n", "shape"), LABELLED)
def test_launch_labels_of_the_gpu_cases_match_the_geometry_predicates(lib, n, shape):
    """Whole-frame geometry (ld = width, origin 0, aligned buffers, one frame) on the lattice of the case's covering."""
    coords = np.ascontiguousarray(orc.calculate_covering(shape, n), np.int32)
    for mode in KERNEL_PAD_MODES:
        form = lib.emu_lattice_launch(n, len(coords), coords.ctypes.data_as(VP), shape[0], shape[1], MODES[mode])
        assert form & 4, "the covering covers the frame"
        assert launch(n, shape, mode) == FORMS[form & 3], mode
