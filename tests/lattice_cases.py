"""Corner lists for the host-side lattice tables (regularizepsf_amd/csrc/rpsf_lattice.hpp): the cases recorded in
tests/golden/lattice_tables.npz and the grid tests/test_lattice_host.py checks property by property."""

import numpy as np

#: tables in the order of emu_lattice_fetch(): name -> (index, dtype, columns)
TABLES = {"order": (0, np.int32, 0), "desc": (1, np.int32, 4), "cover": (2, np.uint8, 0), "tile_info": (3, np.uint8, 0),
          "quads": (4, np.uint32, 4), "sum_order": (5, np.uint32, 0), "prefetch_tiles": (6, np.uint32, 0), "sweep_slot": (7, np.int32, 0)}
SCALARS = ("lattice", "direct_ok", "r0", "c0", "nti", "ntj", "par_j") + tuple(f"prefetch_first{i}" for i in range(9))
MAX_BANDS = 16  # HostPipe::MAX_BANDS


def lattice(n, nli, nlj, origin=None, missing=()):
    """Corners of an nli x nlj half-overlap lattice of n-pixel patches, row-major, without the cells in ``missing``."""
    r0, c0 = origin if origin is not None else (-n // 2, -n // 2)
    return np.array([(r0 + li * (n // 2), c0 + lj * (n // 2)) for li in range(nli) for lj in range(nlj) if (li, lj) not in missing], np.int32)


def _view():
    """Lattice rows 1..3 of a 6 x 9 parent: an odd row parity, K indices and colours of the parent."""
    parent = lattice(128, 6, 9)
    k_index = np.array([i for i, (r, _) in enumerate(parent) if r in (0, 64, 128)], np.int32)
    return parent[k_index], k_index, np.array([-64, -64, 1], np.int32)


def _moved():
    coords = lattice(64, 5, 9)
    coords[17, 1] += 1
    return coords


#: name -> (N, corners, k_index or None, parent (r0, c0, lattice) or None); the second-generation tables are wanted for N >= 128
GOLDEN_CASES = {
    "n256_5x9": (256, lattice(256, 5, 9), None, None),  # eight chunks, the last short; four strips walked "meet"; rim last; direct words
    "n128_5x9_holes": (128, lattice(128, 5, 9, missing={(0, 0), (2, 3)}), None, None),  # a tile nobody covers, holes in the fused order; rim first
    "n128_3x7": (128, lattice(128, 3, 7), None, None),  # one strip
    "n128_view": (128, *_view()),
    "n256_17x17": (256, lattice(256, 17, 17), None, None),  # the 2048^2 covering
    "n64_5x9": (64, lattice(64, 5, 9), None, None),  # two patches per workgroup
    "n32_2x2": (32, lattice(32, 2, 2), None, None),  # the smallest sweep lattice; chunks rounded to eight patches, seven of them empty
    "n16_3x40": (16, lattice(16, 3, 40), None, None),  # 32 patches per workgroup
    "n64_moved": (64, _moved(), None, None),  # one corner off by a pixel: Morton order, colour 0, nothing else
    "n64_twice": (64, np.concatenate([lattice(64, 5, 9), lattice(64, 5, 9)[7:8]]), None, None),  # a corner listed twice: no lattice
}
#: name -> (N, corners, frame rows, bands wanted)
BAND_CASES = {
    "bands_n256_want4": (256, lattice(256, 17, 17), 2048, 4),
    "bands_n256_want8": (256, lattice(256, 17, 17), 2048, 8),
    "bands_n64_want3": (64, lattice(64, 18, 5), 520, 3),
    "bands_three_rows": (128, lattice(128, 3, 7), 256, 4),  # lattice rows / 2 < 2: not cut
}

GRID_N = (16, 32, 64, 128, 256)
GRID_NLI = (1, 2, 3, 5, 9, 17, 33)
GRID_NLJ = (1, 2, 7, 8, 9, 16, 17, 33, 65)


def thinned(n, nli, nlj, seed):
    """The lattice with about a tenth of its cells removed by a seeded draw (cell (0, 0) stays: a plan has at least one patch)."""
    rng = np.random.default_rng(seed)
    missing = {(li, lj) for li in range(nli) for lj in range(nlj) if rng.random() < 0.1 and (li, lj) != (0, 0)}
    return lattice(n, nli, nlj, missing=missing)
