"""The builder's clean-up kernel B3 on the GPU: the cases and checks of tests/cleanup_cases.py, which tests/test_cleanup_host.py runs
on the emulator - against ``builder.clean_cell`` (flags, support exactly, values to 1e-12 per cell) and bit for bit against the
emulator, whose sums run in the same order - and what only hardware shows, tested as bits: cells in one launch, one launch per
cell on a fresh handle and in reversed order; two handles of different sizes in turn; the same call twice.
"""

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native
from regularizepsf_amd import builder as bld
from tests import cleanup_cases as cc

pytestmark = pytest.mark.gpu


def _clean(cells):
    stack = bld._Stack(cells.shape[-1], 0, 1)
    try:
        return stack.clean(cells)
    finally:
        stack.close()


def _against_oracle_and_emulator(case, label):
    out, flags = _clean(case["cells"])
    cc.check(case, out, flags, label)
    emulated, emulated_flags = cc.emu_clean(case["cells"])
    assert np.array_equal(flags, emulated_flags) and cc.same_bits(out, emulated)


@pytest.mark.parametrize("n", cc.SIZES)
def test_kernel_per_size_against_clean_cell_and_the_emulator(n):
    _against_oracle_and_emulator(cc.size_case(n), f"GPU N = {n}")


@pytest.mark.parametrize("n", cc.LABEL_SIZES)
def test_kernel_on_the_labelling_cells(n):
    _against_oracle_and_emulator(cc.label_case(n), f"GPU labelling N = {n}")


def test_degenerate_ring_is_flagged_and_the_host_takes_over():
    case = cc.degenerate_case()
    out, flags = _clean(case["cell"][None])
    assert flags.tolist() == [cc.DEGENERATE] and cc.same_bits(out[0], case["cell"])
    stack = bld._Stack(8, 0, 1)
    stack.load(case["cell"].astype(np.float32)[None])
    got = bld.model_on_device(stack, "mean", 50.0, np.array([0, 1]), np.array([0]))
    assert cc.same_bits(got[0], bld.clean_cell(case["cell"] / 2.0))
    stack.close()


def _all_cells(n):
    cells = cc.size_case(n)["cells"]
    return np.concatenate([cells, cc.label_case(n)["cells"]]) if n in cc.LABEL_SIZES else cells


@pytest.mark.parametrize("n", (16, 64, 128))
def test_launch_shape_and_order_do_not_change_a_bit(n):
    cells = _all_cells(n)
    stack = bld._Stack(n, 0, 1)
    together, flags = stack.clean(cells)
    again, flags_again = stack.clean(cells)
    assert cc.same_bits(together, again) and np.array_equal(flags, flags_again)  # the same call twice
    assert stack.clean_ms() > 0.0
    backwards, flags_backwards = stack.clean(cells[::-1])
    assert cc.same_bits(together, backwards[::-1]) and np.array_equal(flags, flags_backwards[::-1])
    stack.close()
    for k, cell in enumerate(cells):  # one launch per cell, each on a fresh handle
        alone, flag = _clean(cell[None])
        assert cc.same_bits(alone[0], together[k]) and flag[0] == flags[k], k


def test_two_handles_of_different_sizes_in_turn():
    big, small = _all_cells(128), _all_cells(16)
    want_big, want_small = _clean(big)[0], _clean(small)[0]
    a, b = bld._Stack(128, 0, 1), bld._Stack(16, 0, 1)
    for _ in range(2):
        assert cc.same_bits(a.clean(big)[0], want_big)
        assert cc.same_bits(b.clean(small)[0], want_small)
    a.close()
    b.close()


@pytest.mark.parametrize("name", cc.MODEL_SIZES)
def test_model_is_average_then_clean(name):
    stack = bld._Stack(cc.model_case(name)["n"], 0, 4)
    cc.fill(stack, name)
    cc.check_model_is_average_then_clean(stack, name)
    stack.close()


@pytest.mark.parametrize("name", ("n16", "n15"))
def test_build_with_device_cleanup_against_host_cleanup(name):
    cc.check_build(name)


def test_argument_errors_are_errors():
    stack = bld._Stack(16, 0, 1)
    good = cc.size_case(16)["cells"][1:3]
    for value in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[1, 3, 4] = value
        with pytest.raises(_native.NativeError) as info:
            stack.clean(bad)
        assert info.value.code == _native.E_BADARG and "cell 1" in str(info.value)
    with pytest.raises(_native.NativeError) as info:
        stack.clean(np.zeros((0, 16, 16)))  # n_cells = 0
    assert info.value.code == _native.E_BADARG
    with pytest.raises(_native.NativeError) as info:
        stack.model("mean", 50.0, np.array([0]), np.zeros(0, np.int32))  # n_cells = 0
    assert info.value.code == _native.E_BADARG
    out, flags = stack.clean(good)  # the handle still works
    assert not flags.any() and np.isfinite(out).all()
    stack.close()
    with pytest.raises(ValueError, match="cleanup"):
        rp.ArrayPSFBuilder(16, cleanup="gpu")
