"""Cases of the fused star finding that tests/test_stars_fused_host.py (the CPU emulator) and tests/test_gpu_stars_fused.py
share: the mesh table of kernel S1b, its emulator, and the frames of the fused build.  The frames of the detector come from
tests/star_cases.py.

The reference of S1b is regularizepsf_amd.stars.filter_mesh - two np.median and two scipy.ndimage.median_filter calls - and the
comparison is of bytes: S1b selects elements, its only arithmetic is (a + b) / 2.0 of the two middle elements and threshold * global_rms.
"""

from __future__ import annotations

import functools
import pathlib

import numpy as np

from tests import emulib
from tests import star_cases as sc

ROOT = pathlib.Path(__file__).resolve().parent.parent

# 40 x 50: 2000 nodes, eight strides of a 256-thread workgroup; 129 x 128: 16 512 nodes, above the switch to the many-workgroup route
MESH_SHAPES = ((1, 1), (1, 2), (2, 1), (1, 5), (2, 2), (3, 4), (5, 3), (9, 13), (16, 16), (40, 50), (1, 300))
LARGE_MESH_SHAPE = (129, 128)
INVALID_SHARES = (0.0, 0.3, 0.9, 1.0)
THRESHOLDS = (3.0, 0.1)


def _mesh(shape: tuple[int, int], share: float, kind: str, rng: np.random.Generator) -> tuple[np.ndarray, np.ndarray]:
    """A raw mesh pair as S1 leaves it: level around 10, rms around 0.3.  `kind` says where the invalid nodes carry their NaN (level,
    rms or both, +-Inf mixed in) or that the values are rounded so that many are tied."""
    level = 10.0 + rng.normal(0.0, 0.5, shape)
    rms = np.abs(0.3 + rng.normal(0.0, 0.05, shape))
    if kind == "ties":
        level, rms = np.round(level, 0), np.round(rms, 1)
    bad = rng.random(shape) < share if share < 1.0 else np.ones(shape, bool)
    where = {"level": 0, "rms": 1}.get(kind)
    for index in zip(*np.nonzero(bad)):
        target = where if where is not None else int(rng.integers(0, 3))  # 2: both
        value = np.nan if kind != "inf" else (np.nan, np.inf, -np.inf)[int(rng.integers(0, 3))]
        if target in (0, 2):
            level[index] = value
        if target in (1, 2):
            rms[index] = value
    return level, rms


@functools.cache
def mesh_table(shapes: tuple = MESH_SHAPES) -> tuple:
    """(name, level, rms) for every shape, invalid share and kind; read-only."""
    out = []
    for shape in shapes:
        for share in INVALID_SHARES:
            for kind in (("plain",) if share == 0.0 else ("level", "rms", "both", "inf")) + ("ties",):
                rng = np.random.default_rng([shape[0], shape[1], int(share * 10), len(kind)])
                level, rms = _mesh(shape, share, kind, rng)
                level.flags.writeable = rms.flags.writeable = False
                out.append((f"{shape[0]}x{shape[1]} {int(share * 100)}% {kind}", level, rms))
    return tuple(out)


def check_filter_mesh(run, table=None) -> None:
    """`run(level, rms, threshold)` -> (level_f, rms_f, global_rms, T, none) against stars.filter_mesh, bit for bit."""
    from regularizepsf_amd import stars

    seen_none = seen_filled = 0
    for name, level, rms in (mesh_table() if table is None else table):
        want = stars.filter_mesh(level, rms)
        for threshold in THRESHOLDS:
            level_f, rms_f, global_rms, T, none = run(level, rms, threshold)
            if want is None:
                assert none == 1, name
                seen_none += 1
                continue
            assert none == 0, name
            seen_filled += not (np.isfinite(level) & np.isfinite(rms)).all()
            assert level_f.tobytes() == want[0].tobytes(), f"{name}: level differs at {np.flatnonzero(level_f.ravel() != want[0].ravel())[:5]}"
            assert rms_f.tobytes() == want[1].tobytes(), f"{name}: rms differs"
            assert np.float64(global_rms).tobytes() == np.float64(want[2]).tobytes(), f"{name}: global rms {global_rms!r} != {want[2]!r}"
            assert np.float64(T).tobytes() == np.float64(threshold * want[2]).tobytes(), f"{name}: T"
    assert seen_none > 0 and seen_filled > 0


# ------------------------------------------------------------------------------------------------------------------ the emulator
@functools.cache
def emulator():
    """tests/emu/libemu_stars_mesh.so: kernel S1b on the CPU.  __graft_entry__.build() compiles it; it is compiled here when it is missing
    or older than its sources.  Without a compiler that is an error, not a skip."""
    import ctypes
    lib = emulib.library("emu_stars_mesh")
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emusm_info.argtypes = [vp, vp, vp]
    lib.emusm_filter_mesh.argtypes = [vp, vp, i, i, d, i, vp, vp, vp, vp, vp]
    return lib


def emu_filter_mesh(level: np.ndarray, rms: np.ndarray, threshold: float, many: int = -1):
    import ctypes

    level, rms = np.ascontiguousarray(level, np.float64), np.ascontiguousarray(rms, np.float64)
    level_f, rms_f = np.full(level.shape, -5.0), np.full(level.shape, -5.0)
    global_rms, T, none = ctypes.c_double(-5.0), ctypes.c_double(-5.0), ctypes.c_int(-5)
    assert emulator().emusm_filter_mesh(level.ctypes.data, rms.ctypes.data, *level.shape, float(threshold), many, level_f.ctypes.data,
                                        rms_f.ctypes.data, ctypes.byref(global_rms), ctypes.byref(T), ctypes.byref(none)) == 0
    return level_f, rms_f, global_rms.value, T.value, none.value


# ------------------------------------------------------------------------------------------------------------------ frames
def detection_cases() -> dict:
    """name -> (frame, mask, box): the cases of tests/star_cases.py the fused detection is compared on, a fully masked frame and two
    frames with box = 8 - 40 x 50 nodes (eight strides of the one workgroup) and 130 x 127 nodes (the many-workgroup route)."""
    out = {name: (make()["frame"], make()["mask"], make()["box"]) for name, make in sc.CASES.items()}
    case = sc.background_case()
    out["background"] = (case["frame"], None, case["box"])
    wide = sc.frame_case("wide")
    out["fully masked"] = (wide["frame"], np.ones(wide["frame"].shape, bool), wide["box"])
    out["box 8"] = (_box8_frame((320, 400), 12, 11), None, 8)
    out["box 8 large"] = (_box8_frame((1040, 1016), 40, 12), None, 8)
    return out


@functools.cache
def _box8_frame(shape: tuple[int, int], count: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng([seed, 41])
    frame = sc.star_frame(shape, sc.scattered(shape, count, rng), rng)
    frame.flags.writeable = False
    return frame


@functools.cache
def build_frames() -> tuple:
    """The wide frame, an all-background frame of its shape and the wide frame's sibling: a starless frame between two with stars."""
    shape = sc.FRAMES["wide"]["shape"]
    empty = sc.star_frame(shape, np.zeros((0, 2)), np.random.default_rng(77))
    empty.flags.writeable = False
    return (sc.frame_case("wide")["frame"], empty, sc.frame_case("wide", 1)["frame"])


@functools.cache
def scaled_frames() -> tuple:
    """Two frames of 40 x 50 with three stars each."""
    out = []
    for seed in (5, 6):
        rng = np.random.default_rng([seed, 43])
        frame = sc.star_frame((40, 50), np.array([(10.3, 12.6), (28.7, 20.2), (18.4, 38.9)]) + rng.uniform(-0.5, 0.5, (3, 2)), rng)
        frame.flags.writeable = False
        out.append(frame)
    return tuple(out)


def crater_frame() -> np.ndarray:
    """A frame whose one 'star' is a crater: a bowl 1 + r^2 of radius 14 around (32.3, 31.6) on a flat background of 1.  The detector
    finds the bowl's walls, their centroid is the bottom of the bowl, and no border pixel of the patch cut there lies below its centre:
    the ring of the background plane is degenerate (the recipe of tests/builder_cases.py's bowl_frame, made findable)."""
    rows, cols = np.mgrid[0:64, 0:64].astype(np.float64)
    r2 = (rows - 32.3) ** 2 + (cols - 31.6) ** 2
    return np.where(r2 <= 14.0 ** 2, 1.0 + r2, 1.0).astype(np.float32).astype(np.float64)


def assert_same_build(got, want, what: str) -> None:
    """Two results of ArrayPSFBuilder.build agree bit for bit: model values (NaN cells included), coordinates, counts, patches."""
    assert got[0].coordinates == want[0].coordinates, what
    assert got[0].values.tobytes() == want[0].values.tobytes(), f"{what}: model differs"
    assert got[1] == want[1], f"{what}: counts differ"
    assert len(got) == len(want)
    if len(got) == 3:
        assert list(got[2].keys()) == list(want[2].keys()), f"{what}: patch keys differ"
        for key in want[2]:
            assert got[2][key].tobytes() == want[2][key].tobytes(), f"{what}: patch {key} differs"
