"""Drive the kernel's per-thread phases (regularizepsf_amd/csrc/rpsf_core.hpp, and rpsf_core2.hpp for the
second-generation 128/256-pixel plans) on the CPU, thread by thread, and check the result against the reference goldens.  This pins the index algebra shared with the HIP
kernel (digit layouts, LDS addressing, slot table, packed-K format) without needing a GPU."""

import ctypes
import functools
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import APPLY_CASES, KERNEL_PAD_MODES, MARGIN, LocalCase, load_apply_case, local_error, per_patch_reference, rel_errors

ROOT = pathlib.Path(__file__).resolve().parent.parent
EMU_SRC = ROOT / "tests" / "emu" / "emu.cpp"
EMU_LIB = ROOT / "tests" / "emu" / "libemu.so"
CORE = ROOT / "regularizepsf_amd" / "csrc" / "rpsf_core.hpp"
MODES = {"constant": 0, "symmetric": 1, "reflect": 2, "edge": 3, "wrap": 4}


@pytest.fixture(scope="module")
def emu():
    if not EMU_LIB.exists() or EMU_LIB.stat().st_mtime < max(EMU_SRC.stat().st_mtime, CORE.stat().st_mtime):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++")
        if clang is None:
            pytest.skip("no clang++ to build the emulator")
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(EMU_LIB), str(EMU_SRC)], check=True)
    return ctypes.CDLL(str(EMU_LIB))


@pytest.mark.parametrize("case", [c[0] for c in APPLY_CASES if c[7] in MODES])
def test_emulated_kernel_matches_reference_golden(emu, case):
    fx, coords, k = load_apply_case(case)
    image = np.ascontiguousarray(fx["image"], np.float32)
    h, w = image.shape
    c = np.ascontiguousarray(np.array(coords, np.int32))
    kk = np.ascontiguousarray(k, np.complex64)
    out = np.zeros((h, w), np.float32)
    vp = ctypes.c_void_p
    rc = emu.emu_apply(k.shape[1], len(coords), c.ctypes.data_as(vp), h, w, MODES[str(fx["pad_mode"])],
                       ctypes.c_float(0.0), image.ctypes.data_as(vp), kk.ctypes.data_as(vp), out.ctypes.data_as(vp))
    assert rc == 0
    rel_max, rel_l2 = rel_errors(out, fx["expected"])
    assert rel_max <= 1e-5 and rel_l2 <= 1e-5, (rel_max, rel_l2)


EMU2_SRC = ROOT / "tests" / "emu" / "emu2.cpp"
EMU2_LIB = ROOT / "tests" / "emu" / "libemu2.so"
CORE2 = ROOT / "regularizepsf_amd" / "csrc" / "rpsf_core2.hpp"
LATTICE = ROOT / "regularizepsf_amd" / "csrc" / "rpsf_lattice.hpp"


@pytest.fixture(scope="module")
def emu2():
    if not EMU2_LIB.exists() or EMU2_LIB.stat().st_mtime < max(EMU2_SRC.stat().st_mtime, CORE.stat().st_mtime, CORE2.stat().st_mtime, LATTICE.stat().st_mtime):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++")
        if clang is None:
            pytest.skip("no clang++ to build the emulator")
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(EMU2_LIB), str(EMU2_SRC)], check=True)
    return ctypes.CDLL(str(EMU2_LIB))


@pytest.mark.parametrize("direct", [0, 1, 2])
@pytest.mark.parametrize("case", [c[0] for c in APPLY_CASES if c[7] in MODES and c[3] >= 128])
def test_emulated_second_generation_kernel_matches_reference_golden(emu2, case, direct):
    """direct = 1: quadrant by quadrant, the first patch over a lattice tile stores and the later ones accumulate
    (what the tile flags arrange on the GPU); direct = 0: plain adds into a cleared image; direct = 2: four colour planes
    (16-byte stores, rim patches included where the image width allows) summed at the end."""
    fx, coords, k = load_apply_case(case)
    image = np.ascontiguousarray(fx["image"], np.float32)
    h, w = image.shape
    c = np.ascontiguousarray(np.array(coords, np.int32))
    kk = np.ascontiguousarray(k, np.complex64)
    out = np.zeros((h, w), np.float32)
    vp = ctypes.c_void_p
    rc = emu2.emu2_apply(k.shape[1], len(coords), c.ctypes.data_as(vp), h, w, MODES[str(fx["pad_mode"])],
                         ctypes.c_float(0.0), image.ctypes.data_as(vp), kk.ctypes.data_as(vp), out.ctypes.data_as(vp), direct)
    assert rc == 0
    rel_max, rel_l2 = rel_errors(out, fx["expected"])
    assert rel_max <= 1e-5 and rel_l2 <= 1e-5, (rel_max, rel_l2)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", [(256, 384), (200, 250)])
def test_emulated_rim_patches_every_pad_mode(emu2, mode, shape):
    """Rim patches of the second-generation plans take 16-byte loads where the np.pad map keeps a unit of four pixels
    together (ascending, or mirrored by 'symmetric') and pixel-by-pixel loads elsewhere; 16-byte plane stores where the
    image width is a multiple of 4.  Every pad mode the kernel evaluates itself, an aligned and an unaligned width,
    against the oracle."""
    from oracle import regpsf_oracle as orc

    n = 128
    h, w = shape
    rng = np.random.default_rng(5)
    image = (100 + 5 * rng.standard_normal((h, w))).astype(np.float32)
    coords = [tuple(int(v) for v in c) for c in orc.calculate_covering((h, w), n)]
    k = (rng.standard_normal((len(coords), n, n)) + 1j * rng.standard_normal((len(coords), n, n))).astype(np.complex64)
    expected = orc.apply_transfer(image, coords, k, pad_mode=mode)
    c = np.ascontiguousarray(np.array(coords, np.int32))
    vp = ctypes.c_void_p
    for direct in (0, 2):
        out = np.zeros((h, w), np.float32)
        rc = emu2.emu2_apply(n, len(coords), c.ctypes.data_as(vp), h, w, MODES[mode], ctypes.c_float(0.0), image.ctypes.data_as(vp),
                             k.ctypes.data_as(vp), out.ctypes.data_as(vp), direct)
        assert rc == 0
        rel_max, rel_l2 = rel_errors(out, expected)
        assert rel_max <= 1e-5 and rel_l2 <= 1e-5, (mode, direct, rel_max, rel_l2)


@pytest.mark.parametrize("n", [256, 128])
def test_slot_table_keeps_the_gid_indexed_exchange_free_of_bank_conflicts(emu2, n):
    """The slot table the plan uploads (build_slot_table2, rpsf_core2.hpp) against MI355X's LDS banking: ds_read_b64 serves the two
    32-lane halves of a wave from 64 banks, ds_write_b64 four runs of 16 lanes from 32 banks, one LDS-array cycle per distinct address on
    a bank and group.  Every half wave reads conflict-free; the writes are conflict-free except for the run that holds the two self-paired
    slots (lanes 0 and 1 of wave 0, fixed by the kernel), where a 2-way conflict stays under the instruction's own issue cycles."""
    tab = np.zeros(2 * 512, np.uint16)
    units = np.zeros(1024, np.int32)
    threads, nslot, dealt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    vp = ctypes.c_void_p
    assert emu2.emu2_slot_table(n, tab.ctypes.data_as(vp), units.ctypes.data_as(vp), ctypes.byref(threads), ctypes.byref(nslot), ctypes.byref(dealt)) == 0
    t, ns = threads.value, nslot.value
    assert dealt.value == 1 and t * ns == 512
    gids = tab.reshape(t, ns, 2).astype(np.int64)
    assert sorted(gids.ravel().tolist()) == list(range(1024))  # every group once
    u = units[gids]  # [thread, slot, member]
    read_cycles = write_cycles = 0
    worst_write = 0
    for s in range(ns):
        for member in range(2):
            for w in range(t // 64):
                lanes = u[w * 64:(w + 1) * 64, s, member]
                for lo in (0, 32):  # ds_read_b64: bank pair of an 8-byte unit = unit mod 32
                    read_cycles += np.bincount(lanes[lo:lo + 32] % 32, minlength=32).max()
                for lo in range(0, 64, 16):  # ds_write_b64: unit mod 16
                    c = np.bincount(lanes[lo:lo + 16] % 16, minlength=16).max()
                    write_cycles += c
                    worst_write = max(worst_write, c)
    halves, runs = ns * (t // 64) * 2 * 2, ns * (t // 64) * 4 * 2
    assert read_cycles == halves, (read_cycles, halves)
    assert write_cycles <= runs + 4 and worst_write <= 2, (write_cycles, runs, worst_write)


# ---- third generation (N = 16, 32, 64): the sweep kernel's per-lane phases and its job lists ----------------------------------
EMU3_SRC = ROOT / "tests" / "emu" / "emu3.cpp"
EMU3_LIB = ROOT / "tests" / "emu" / "libemu3.so"
CORE3 = [ROOT / "regularizepsf_amd" / "csrc" / n for n in ("rpsf_core.hpp", "rpsf_core3.hpp", "rpsf_plan3.hpp", "rpsf_lattice.hpp")]


@pytest.fixture(scope="module")
def emu3():
    if not EMU3_LIB.exists() or EMU3_LIB.stat().st_mtime < max([EMU3_SRC.stat().st_mtime] + [c.stat().st_mtime for c in CORE3]):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++")
        if clang is None:
            pytest.skip("no clang++ to build the emulator")
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(EMU3_LIB), str(EMU3_SRC)], check=True)
    lib = ctypes.CDLL(str(EMU3_LIB))
    lib.emu3_check_plan.restype = ctypes.c_long
    return lib


def _emu3_run(emu3, case, target_regions, order_seed, aligned):
    fx, coords, k = load_apply_case(case)
    image = np.ascontiguousarray(fx["image"], np.float32)
    h, w = image.shape
    c = np.ascontiguousarray(np.array(coords, np.int32))
    kk = np.ascontiguousarray(k, np.complex64)
    out = np.full((h, w), np.nan, np.float32)
    stats = (ctypes.c_int64 * 4)()
    vp = ctypes.c_void_p
    rc = emu3.emu3_apply(k.shape[1], len(coords), c.ctypes.data_as(vp), h, w, MODES[str(fx["pad_mode"])], ctypes.c_float(0.0),
                         image.ctypes.data_as(vp), kk.ctypes.data_as(vp), out.ctypes.data_as(vp), target_regions, order_seed, aligned, stats)
    assert rc == 0, rc  # (-6: a pixel written twice, -7: a covered pixel never written, -4: a job waits for one not yet drawn)
    return out, fx, list(stats)


@pytest.mark.parametrize("case", [c[0] for c in APPLY_CASES if c[7] in MODES and c[3] <= 64])
def test_emulated_sweep_kernel_matches_reference_golden(emu3, case):
    """The lane phases of the third-generation kernel (transposes, row-pair packing, packed K with the a / b rule of column 0,
    ring addressing, store / add / flush modes) over the library's own job lists, every output pixel written exactly once."""
    out, fx, _ = _emu3_run(emu3, case, 8, 0, 1)
    rel_max, rel_l2 = rel_errors(out, fx["expected"])
    assert rel_max <= 1e-5 and rel_l2 <= 1e-5, (rel_max, rel_l2)


@pytest.mark.parametrize("case", ["n32_sym", "n32_constant", "n16_sym", "n64_sym"])
def test_sweep_result_does_not_depend_on_the_cut_or_on_the_waves_timing(emu3, case):
    """Bit for bit the same image whatever the number of regions, whether the 16-byte paths are taken, and in whatever order
    the dependency flags let the jobs of a region finish."""
    base, _, _ = _emu3_run(emu3, case, 8, 0, 1)
    for target, seed, aligned in ((8, 1, 1), (8, 2, 1), (64, 3, 1), (1, 4, 1), (256, 5, 0), (3, 0, 0)):
        out, _, _ = _emu3_run(emu3, case, target, seed, aligned)
        assert np.array_equal(out, base), (target, seed, aligned)


def test_sweep_job_lists_order_every_conflicting_pair_and_flush_every_band_once(emu3):
    """rpsf_plan3.hpp over a grid of lattice shapes: two jobs of a region that touch the same ring words inside the owned columns (one of
    them writing) are ordered by the dependency lists, and every (row band, column band) cell is flushed by exactly one job."""
    for n, ksmax in ((16, 4), (32, 2), (64, 2)):
        for nli in (2, 3, 4, 5, 9, 17, 33, 65, 129):
            for nlj in (2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 129):
                for target in (1, 8, 256, 1024):
                    stats = (ctypes.c_int64 * 4)()
                    assert emu3.emu3_check_plan(n, ksmax, 8, nli, nlj, target, stats) == 0, (n, nli, nlj, target, list(stats))


def test_sweep_recompute_factor_at_the_benchmark_sizes(emu3):
    """Patches on region borders are computed twice: the planner keeps that below what the LDS ring allows at the sizes VERDICT round 5 names."""
    for n, ksmax, lattice, bound in ((32, 2, 257, 1.16), (64, 2, 129, 1.30), (16, 4, 513, 1.09)):
        stats = (ctypes.c_int64 * 4)()
        assert emu3.emu3_check_plan(n, ksmax, 8, lattice, lattice, 256, stats) == 0
        assert stats[2] / (lattice * lattice) <= bound, (n, list(stats))


# ---- local parity: the emulated kernel phases on frames that span six decades, per patch neighbourhood -----------------------------
# The tests above bound the error by 1e-5 of the brightest pixel of the frame; the reference treats every patch on its own, so a correct
# float32 implementation errs at a pixel by ~2e-7 of what the (at most four) patches over that pixel carry.  Below: max |d| / local scale
# (tests/helpers.py) of every emulator against the same quantity of the float32 yardstick (the oracle's own steps in single precision),
# at most MARGIN x; every case has at least 10 % of its pixels below 1e-3 of the frame's largest scale (asserted from the float64 oracle
# alone in LocalCase).  And exact homogeneity: a power-of-two factor on the frame comes out as that factor on every pixel, bit for bit.

LOCAL_SEEDS = {128: 129, 256: 272}  # HDR seeds for which every pad mode leaves >= 10 % of the frame dim (asserted per case)


@functools.lru_cache(maxsize=8)
def _local_case(shape, n, seed, mode):
    return LocalCase(shape, n, seed, mode)


def _run_emu(lib, case, image):
    out = np.zeros(case.shape, np.float32)
    c = np.ascontiguousarray(np.array(case.coords, np.int32))
    vp = ctypes.c_void_p
    img = np.ascontiguousarray(image, np.float32)
    rc = lib.emu_apply(case.n, len(case.coords), c.ctypes.data_as(vp), *case.shape, MODES[case.pad_mode], ctypes.c_float(0.0),
                       img.ctypes.data_as(vp), case.k.ctypes.data_as(vp), out.ctypes.data_as(vp))
    assert rc == 0
    return out


def _run_emu2(lib, case, image, direct):
    out = np.zeros(case.shape, np.float32)
    c = np.ascontiguousarray(np.array(case.coords, np.int32))
    vp = ctypes.c_void_p
    img = np.ascontiguousarray(image, np.float32)
    rc = lib.emu2_apply(case.n, len(case.coords), c.ctypes.data_as(vp), *case.shape, MODES[case.pad_mode], ctypes.c_float(0.0),
                        img.ctypes.data_as(vp), case.k.ctypes.data_as(vp), out.ctypes.data_as(vp), direct)
    assert rc == 0
    return out


def _run_emu3(lib, case, image, target_regions, order_seed=0):
    out = np.full(case.shape, np.nan, np.float32)
    c = np.ascontiguousarray(np.array(case.coords, np.int32))
    vp = ctypes.c_void_p
    img = np.ascontiguousarray(image, np.float32)
    stats = (ctypes.c_int64 * 4)()
    rc = lib.emu3_apply(case.n, len(case.coords), c.ctypes.data_as(vp), *case.shape, MODES[case.pad_mode], ctypes.c_float(0.0),
                        img.ctypes.data_as(vp), case.k.ctypes.data_as(vp), out.ctypes.data_as(vp), target_regions, order_seed,
                        int(case.shape[1] % 4 == 0), stats)
    assert rc == 0, rc
    return out


def _local_bound_and_homogeneity(case, run, what):
    """The 1e-5 bar of the tests above, the local bound, and run(s x frame) == s x run(frame) bit for bit for s = 2^10 and 2^-10."""
    out = run(case.image)
    rel_max, rel_l2 = rel_errors(out, case.ref)
    ratio = case.ratio(out)
    print(f"{what}: dim share {case.share:.2f}, yardstick {case.yardstick:.2e}, local error {ratio:.2f} x yardstick, global {rel_max:.2e}")
    assert rel_max <= 1e-5 and rel_l2 <= 1e-5, (rel_max, rel_l2)
    case.check(out, MARGIN, what)
    for s in (np.float32(1024.0), np.float32(1.0 / 1024.0)):
        assert np.array_equal(run(s * case.image), s * out), (what, float(s))


def test_per_patch_reference_is_the_pinned_oracle_and_its_float32_form_is_homogeneous():
    """The helper every local bound rests on: its float64 result equals orc.apply_transfer to rounding (asserted inside the helper, on
    every call, here once per pad mode and on a golden case with a non-random K), its float32 form stays in single precision, and a
    power-of-two factor on the frame goes through the float32 steps exactly."""
    for mode in KERNEL_PAD_MODES:
        case = _local_case((130, 203), 32, 32, mode)
        yard, none = per_patch_reference(case.image, case.coords, case.k, mode, np.float32)
        assert none is None and yard.dtype == np.float32
        assert 1e-7 < local_error(yard, case.ref, case.scale) < 5e-7
        for s in (np.float32(1024.0), np.float32(1.0 / 1024.0)):
            assert np.array_equal(per_patch_reference(s * case.image, case.coords, case.k, mode, np.float32)[0], s * yard)
    fx, coords, k = load_apply_case("n64_sym")
    ref, scale = per_patch_reference(fx["image"], coords, k, "symmetric", np.float64)
    assert np.abs(ref - fx["expected"]).max() <= 1e-12 * np.abs(fx["expected"]).max()
    assert scale.shape == ref.shape and (scale > 0).all()


@pytest.mark.parametrize("mode", KERNEL_PAD_MODES)
def test_first_generation_emulator_local_parity_and_homogeneity(emu, mode):
    case = _local_case((130, 203), 32, 32, mode)
    _local_bound_and_homogeneity(case, lambda image: _run_emu(emu, case, image), f"emu N=32 {mode}")


@pytest.mark.parametrize("direct", [0, 1, 2])
@pytest.mark.parametrize("mode", KERNEL_PAD_MODES)
@pytest.mark.parametrize(("n", "shape", "seed"), [(128, (520, 650), LOCAL_SEEDS[128]), (256, (520, 770), LOCAL_SEEDS[256])])
def test_second_generation_emulator_local_parity_and_homogeneity(emu2, n, shape, seed, mode, direct):
    """Plain adds, first-store-then-accumulate and the four colour planes; rim patches and a width that is no multiple of four."""
    case = _local_case(shape, n, seed, mode)
    _local_bound_and_homogeneity(case, lambda image: _run_emu2(emu2, case, image, direct), f"emu2 N={n} direct={direct} {mode}")


@pytest.mark.parametrize("mode", KERNEL_PAD_MODES)
@pytest.mark.parametrize(("n", "shape", "seed"), [(16, (100, 135), 16), (16, (100, 136), 16), (32, (300, 500), 32), (32, (130, 203), 32),
                                                  (64, (333, 390), 64), (64, (320, 392), 64)])
def test_sweep_emulator_local_parity_and_homogeneity(emu3, n, shape, seed, mode):
    """The sweep kernel's lane phases (128 / N patches in a wave, two rows in one complex transform, the LDS ring) cut into one region
    and into many, widths that take the 16-byte paths and widths that do not."""
    case = _local_case(shape, n, seed, mode)
    for target in (1, 8):
        _local_bound_and_homogeneity(case, lambda image: _run_emu3(emu3, case, image, target, target), f"emu3 N={n} {shape} regions={target} {mode}")
