"""The PSF builder at the wide sizes 129 ... 256 without a GPU: the per-thread phases of kernels B1w and B3w on the CPU lane emulators
(tests/emu/emu_builder_wide.cpp, tests/emu/emu_cleanup_wide.cpp) against the float64 NumPy / SciPy oracle of tests/builder_cases.py and
tests/cleanup_cases.py, with the cases of tests/builder_wide_cases.py, which tests/test_gpu_builder_wide.py shares.

1. B1w per case: flags equal the oracle's, every accepted patch within 1e-5 of the oracle patch's maximum.
2. The wide phases at N = 64 and 128 give kernel B1's flags and float32 bits: the arithmetic order is B1's.
3. B3w per size and per labelling case: flags, NaN pixels and support exactly the oracle's, values within 1e-12.
4. The refusals of rpsf_builder_create_wide, which return before any HIP call.
"""

import ctypes

import numpy as np
import pytest

from regularizepsf_amd import _native
from tests import builder_cases as bc
from tests import builder_wide_cases as wc
from tests import cleanup_cases as cc


def _bits(a):
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


# ------------------------------------------------------------------------------------------------ 1. B1w against the oracle
@pytest.mark.parametrize("name", list(wc.WIDE_CASES))
def test_emulated_wide_patches_against_scipy(name):
    case = wc.wide_case(name)
    bc.well_posed(case)
    assert all(len(pos) == 10 for pos in case["stars"])
    patches, flags = wc.emu_case(case)
    wc.check_patches(name, patches[flags == 1], flags)
    if name.endswith("_small"):  # the frame is smaller than the patch
        assert max(case["frames"].shape[1:]) < case["n"]


def test_the_slots_do_not_change_a_bit():
    case = wc.wide_case("n129")
    want, want_flags = wc.emu_case(case)
    for n_slots in (1, 3):  # every star in one slot, one after the other; and a ragged last round
        got, flags = wc.emu_case(case, n_slots=n_slots)
        assert np.array_equal(flags, want_flags) and np.array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------ 2. B1's bits at B1's sizes
@pytest.mark.parametrize("name", wc.PARITY_SIZES)
def test_wide_phases_give_the_narrow_kernels_bits(name):
    case = bc.size_case(name)
    for frame, rounded, shift in zip(case["frames"], case["rounded"], case["shift"]):
        want, want_flags = bc.emu_patches(frame, case["n"], rounded, shift, *case["thresholds"])
        got, flags = wc.emu_patches(frame, case["n"], rounded, shift, *case["thresholds"])
        assert np.array_equal(flags, want_flags) and 0 < (flags == 1).sum()
        keep = flags == 1  # (a rejected star's staging slot is not defined by either kernel)
        assert got.dtype == want.dtype == np.float32 and np.array_equal(_bits(got[keep]), _bits(want[keep]))


def test_storage_plan_at_the_maximum():
    b1, b3 = wc.emulator_b1w(), wc.emulator_b3w()
    assert b1.emubw_lds_bytes(256) == (12 * 256 + 16) * 8 + (8 * 256 + 8) * 4 <= 160 * 1024
    assert b1.emubw_slot_bytes(256) == 2 * 256 * 257 * 8
    assert b3.emucw_lds_bytes(256) == 2 * 65536 + 64 <= 160 * 1024
    assert b3.emucw_slot_bytes(256) == 4 * 65536 + (1024 + 64 + 16) * 40
    assert (wc.slots(129), wc.slots(255), wc.slots(256)) == (256, 256, 255)
    for n in (129, 255, 256):
        assert wc.slots(n) * b1.emubw_slot_bytes(n) <= 256 << 20  # the workspace of a handle is bounded
        assert b3.emucw_slot_bytes(n) <= b1.emubw_slot_bytes(n)  # one workspace serves both kernels


# ------------------------------------------------------------------------------------------------ 3. B3w against clean_cell
@pytest.mark.parametrize("n", wc.CLEAN_SIZES)
def test_emulated_wide_cleanup_per_size(n):
    case = cc.size_case(n)
    assert case["names"][0] == "zero_first" and case["names"][-1] == "zero_after"  # an all-zero cell comes after a normal one
    out, flags = wc.emu_clean(case["cells"], n_slots=1)  # one slot: every cell sees what the cell before left
    cc.check(case, out, flags, f"emulator N = {n}")
    spread, spread_flags = wc.emu_clean(case["cells"])
    assert np.array_equal(flags, spread_flags) and cc.same_bits(out, spread)


@pytest.mark.parametrize("n", wc.CLEAN_SIZES)
def test_emulated_wide_cleanup_on_the_labelling_cells(n):
    case = wc.label_case(n)
    out, flags = wc.emu_clean(case["cells"], n_slots=2)
    cc.check(case, out, flags, f"emulator labelling N = {n}")


def test_wide_cleanup_gives_the_narrow_kernels_bits():
    for n in (33, 128):
        cells = np.concatenate([cc.size_case(n)["cells"], cc.label_case(n)["cells"]])
        want, want_flags = cc.emu_clean(cells)
        got, flags = wc.emu_clean(cells)
        assert np.array_equal(flags, want_flags)
        if n == 128:  # 1024 threads on both sides: the sums run in the same order
            assert cc.same_bits(got, want)
        else:
            assert np.array_equal(got != 0, want != 0) and np.array_equal(np.isnan(got), np.isnan(want))


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_create_wide_refuses_before_any_hip_call():
    lib = _native.lib()
    handle = ctypes.c_void_p()
    assert lib.rpsf_builder_create_wide(None, 0, 256, 8) == _native.E_BADARG and b"null" in lib.rpsf_last_error()
    for size in (128, 257, -1):
        assert lib.rpsf_builder_create_wide(ctypes.byref(handle), 0, size, 8) == _native.E_UNSUPPORTED
        assert str(size).encode() in lib.rpsf_last_error() and not handle.value
    slots = ctypes.c_int(7)
    assert lib.rpsf_builder_wide_slots(None, ctypes.byref(slots)) == _native.E_BADARG and slots.value == 7
    # the narrow entry points keep refusing the wide sizes
    assert lib.rpsf_builder_create(ctypes.byref(handle), 0, 129, 8) == _native.E_UNSUPPORTED and not handle.value
    assert lib.rpsf_builder_create_scaled(ctypes.byref(handle), 0, 129, 1, 8) == _native.E_UNSUPPORTED and not handle.value
