"""What the per-star kernels share (DESIGN.md 3.7 "The disc walk", csrc/rpsf_core_stars_disc.hpp) without a GPU and without any of
the drivers: the box and the walk of a disc against a NumPy enumeration, the fold steps against ordered float64 sums, and the record
template against the byte counts the five drivers had when each kept a struct of its own."""

import ctypes
import functools
import subprocess

import numpy as np
import pytest

from tests import emulib

LANES, WAVES = 64, 4
THREADS, GROUPS = LANES * WAVES, 8 * WAVES
H, W = 12, 10
NAN_PIXEL, MASKED_PIXEL = (4, 4), (5, 5)
# position, radius: integer and half-pixel centres, a box that leaves the frame, the frame's last pixel, no pixel of the frame at all, and
# a disc of more than 64 pixels
WALKS = [(p, r) for p in ((5.0, 4.0), (5.5, 4.5), (-0.25, 0.0), (11.0, 9.0)) for r in (1.0, 2.0)] + [((-100.0, -100.0), 1.0), ((5.0, 4.0), 6.0)]


@functools.cache
def emulator():
    lib = emulib.library("emu_disc")
    vp, i, n, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    lib.emudk_info.argtypes = [vp]
    lib.emudk_box.argtypes = [f, f, f, vp]
    lib.emudk_walk.argtypes = [vp, vp, i, i, f, f, f, f, n, vp, vp]
    lib.emudk_walk.restype = n
    lib.emudk_record_bytes.argtypes = [i, i, i]
    lib.emudk_record_bytes.restype = n
    lib.emudk_fold.argtypes = [vp] * 8
    return lib


@functools.cache
def frame() -> tuple[np.ndarray, np.ndarray]:
    img = (np.arange(H * W, dtype=np.float32).reshape(H, W) + 1.0)
    mask = np.zeros((H, W), np.uint8)
    img[NAN_PIXEL], mask[MASKED_PIXEL] = np.nan, 1
    img.flags.writeable = mask.flags.writeable = False
    return img, mask


def ref_box(y: float, x: float, R: float) -> tuple[int, int, int, int, int, int]:
    r0, r1 = int(np.floor(y - R)) - 1, int(np.ceil(y + R)) + 1
    c0, c1 = int(np.floor(x - R)) - 1, int(np.ceil(x + R)) + 1
    return r0, r1, c0, c1, c1 - c0 + 1, (r1 - r0 + 1) * (c1 - c0 + 1)


def ref_walk(y: float, x: float, R: float) -> list[tuple]:
    """The visitor calls of all 64 lanes, lane by lane: (lane, kind, r, c, pr, pc, q, p) as tests/emu/emu_disc.cpp records them."""
    img, mask = frame()
    r0, _, c0, _, bw, npx = ref_box(y, x, R)
    R2 = np.float64(R) * np.float64(R)
    calls = []
    for lane in range(LANES):
        for j in range(lane, npx, LANES):
            r, c = r0 + j // bw, c0 + j % bw
            pr, pc = np.float64(r) - np.float64(y), np.float64(c) - np.float64(x)
            q = pr * pr + pc * pc
            if not q <= R2:
                continue
            calls.append((lane, 0, 0, 0, pr, pc, 0.0, -1.0))
            if 0 <= r < H and 0 <= c < W and np.isfinite(img[r, c]) and not mask[r, c]:
                calls.append((lane, 1, r, c, pr, pc, q, float(r * W + c)))
    return calls


def emu_walk(y: float, x: float, R: float) -> list[tuple]:
    img, mask = frame()
    cap = 4096
    ints, doubles = np.full((cap, 4), -7, np.int32), np.full((cap, 4), -7.0)
    k = emulator().emudk_walk(img.ctypes.data, mask.ctypes.data, H, W, y, x, R, R * R, cap, ints.ctypes.data, doubles.ctypes.data)
    assert 0 <= k <= cap
    return [(*ints[i].tolist(), *doubles[i].tolist()) for i in range(k)]


def test_the_emulator_has_the_kernels_geometry():
    info = (ctypes.c_long * 2)(0, 0)
    emulator().emudk_info(info)
    assert tuple(info) == (LANES, WAVES)


@pytest.mark.parametrize(("position", "radius"), WALKS)
def test_the_box_is_not_clipped(position, radius):
    box = (ctypes.c_long * 6)()
    emulator().emudk_box(*position, radius, box)
    assert tuple(box) == ref_box(*position, radius)


@pytest.mark.parametrize(("position", "radius"), WALKS)
def test_the_walk_visits_the_enumerated_pixels_in_order(position, radius):
    got, want = emu_walk(*position, radius), ref_walk(*position, radius)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a[:4] == b[:4] and np.array(a[4:]).tobytes() == np.array(b[4:], np.float64).tobytes(), (a, b)
    # the disc by brute force over a grid far larger than the box, and the usable pixels of the frame among it
    img, mask = frame()
    rr, cc = np.mgrid[-120:40, -120:40]
    disc = (rr - position[0]) ** 2 + (cc - position[1]) ** 2 <= radius * radius
    on = disc & (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
    usable = [(r, c) for r, c in zip(rr[on], cc[on]) if np.isfinite(img[r, c]) and not mask[r, c]]
    assert sum(1 for g in got if g[1] == 0) == int(disc.sum()) > 0
    assert sorted((g[2], g[3]) for g in got if g[1] == 1) == sorted(usable)


def test_the_rim_the_excluded_pixels_and_the_second_round():
    """q == R R exactly counts (integer centres), the NaN and the masked pixel are in the disc and not usable, a position far off the
    frame has a disc and no usable pixel, and a disc of more than 64 pixels gives lanes a second pixel."""
    for radius in (1.0, 2.0):
        got = emu_walk(5.0, 4.0, radius)
        assert sum(1 for g in got if g[1] == 1 and g[6] == radius * radius) == (2 if radius == 1.0 else 4)  # (of R = 1's four, (4, 4) is NaN, (5, 5) masked)
        assert sum(1 for g in got if g[1] == 0) == (5 if radius == 1.0 else 13)
    assert [len([g for g in emu_walk(5.5, 4.5, radius) if g[1] == 0]) for radius in (1.0, 2.0)] == [4, 12]
    got = emu_walk(5.0, 4.0, 2.0)
    assert not {NAN_PIXEL, MASKED_PIXEL} & {(g[2], g[3]) for g in got if g[1] == 1}
    got = emu_walk(-100.0, -100.0, 1.0)
    assert len(got) == 5 and all(g[1] == 0 for g in got)
    got = emu_walk(5.0, 4.0, 6.0)
    assert ref_box(5.0, 4.0, 6.0)[5] == 225 and max(sum(1 for g in got if g[0] == lane and g[1] == 0) for lane in range(LANES)) >= 2
    assert (11, 9) in {(g[2], g[3]) for g in emu_walk(11.0, 9.0, 1.0) if g[1] == 1}


# ---------------------------------------------------------------------------------------------------------------------- the fold
def ordered(values) -> np.float64:
    s = np.float64(0.0)
    for v in values:
        s = s + np.float64(v)
    return s


def key(e: float) -> float:
    return abs(e) if e == e else np.inf


def ref_peak(es, ats) -> tuple[float, int]:
    e, at = 0.0, -1
    for ne, nat in zip(es, ats):
        if nat < 0:
            continue
        if at < 0 or key(ne) > key(e) or (key(ne) == key(e) and nat < at):
            e, at = ne, nat
    return e, at


def fold_inputs() -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    rng = np.random.default_rng(12)
    d = np.empty((3, THREADS))
    d[0] = rng.permutation(np.resize([1e16, 1.0, -1e16, 3.0, 1e-3], THREADS))  # a sum that depends on its order
    d[1] = rng.uniform(-1.0, 1.0, THREADS) * 10.0 ** rng.integers(-8, 8, THREADS)
    d[2] = rng.integers(-5, 6, THREADS).astype(np.float64)  # the residuals: many exact ties in |e|, of both signs
    at = rng.permutation(THREADS).astype(np.int64) + 100
    at[rng.choice(THREADS, 40, replace=False)] = -1  # lanes without a pixel
    # wave 1: a NaN wins over everything; wave 2: +7 and -7 tie and the smaller index wins, whichever comes first; wave 3: no pixel
    d[2, LANES + 17], at[LANES + 17] = np.nan, 5000
    d[2, 2 * LANES + 40], at[2 * LANES + 40] = 7.0, 9000
    d[2, 2 * LANES + 3], at[2 * LANES + 3] = -7.0, 9001
    at[3 * LANES:] = -1
    cnt = rng.integers(0, 1000, (2, THREADS)).astype(np.int32)
    return d, at, cnt


def test_the_fold_is_the_ordered_sum_of_8_groups_of_8():
    d, at, cnt = fold_inputs()
    sums, counts = np.full((WAVES, 2), -7.0), np.full((WAVES, 2), -7, np.int32)
    peak_e, peak_at, offsets = np.full(WAVES, -7.0), np.full(WAVES, -7, np.int64), np.zeros(4, np.int64)
    emulator().emudk_fold(*(a.ctypes.data for a in (d, at, cnt, sums, counts, peak_e, peak_at, offsets)))
    straight = 0
    for wave in range(WAVES):
        lanes = slice(wave * LANES, (wave + 1) * LANES)
        for f in range(2):
            want = ordered(ordered(d[f, lanes][8 * g:8 * g + 8]) for g in range(8))
            assert sums[wave, f].tobytes() == want.tobytes(), (wave, f)
            straight += want.tobytes() != ordered(d[f, lanes]).tobytes()
            assert counts[wave, f] == int(cnt[f, lanes].astype(np.int64).sum())
        groups = [ref_peak(d[2, lanes][8 * g:8 * g + 8], at[lanes][8 * g:8 * g + 8]) for g in range(8)]
        e, where = ref_peak(*zip(*groups))
        assert (e, where) == ref_peak(d[2, lanes], at[lanes]) or e != e  # a total order: the fold's grouping does not matter
        assert peak_at[wave] == where and np.float64(peak_e[wave]).tobytes() == np.float64(e).tobytes(), wave
    assert straight > 0  # the grouping shows: these are not the sums of 64 terms in lane order
    assert np.isnan(peak_e[1]) and peak_at[1] == 5000
    assert peak_e[2] == 7.0 and peak_at[2] == 9000
    assert peak_at[3] == -1


def test_the_records_are_field_major():
    """Field f of record i of n is word f n + i: three doubles, the index and two ints of 256 lane records, then of 32 group records."""
    d, at, cnt = fold_inputs()
    out = [np.zeros(8) for _ in range(2)] + [np.zeros(8, np.int32)] + [np.zeros(WAVES), np.zeros(WAVES, np.int64)]
    offsets = np.zeros(4, np.int64)
    emulator().emudk_fold(d.ctypes.data, at.ctypes.data, cnt.ctypes.data, out[0].ctypes.data, out[2].ctypes.data, out[3].ctypes.data,
                          out[4].ctypes.data, offsets.ctypes.data)
    lanes = THREADS * (3 * 8 + 8 + 2 * 4)
    assert offsets.tolist() == [3 * THREADS * 8, 4 * THREADS * 8, lanes, lanes + 4 * GROUPS * 8]


def test_record_bytes_are_what_the_five_drivers_had():
    """S8: six doubles, the index, two ints; S12: eight doubles; S7: seven doubles and two ints; S9: thirteen doubles and one int; S11:
    eighteen doubles, the index, two ints."""
    b = emulator().emudk_record_bytes
    assert (b(6, 1, 2), b(8, 1, 2), b(7, 0, 2), b(13, 0, 1), b(18, 1, 2)) == (64, 80, 64, 108, 160)


def test_the_emulator_under_the_host_sanitizers(tmp_path):
    """The walk and the fold as a plain program with a main of its own (EMU_DISC_MAIN) under -fsanitize=address,undefined; nothing that is
    loaded into Python is touched by a sanitizer."""
    program = tmp_path / "emu_disc_sanitized"
    built = subprocess.run([emulib.compiler(), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-DEMU_DISC_MAIN", str(emulib.EMU / "emu_disc.cpp"), "-o", str(program)], capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitizer" in built.stderr):
        pytest.skip("the host compiler cannot link the sanitizers' runtimes: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr[-2000:]
    done = subprocess.run([str(program)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "visitor calls" in done.stdout, (done.returncode, done.stdout[-500:], done.stderr[-3000:])
