"""The builder's clean-up kernel B3 without a GPU: its driver (csrc/rpsf_core_cleanup.hpp) on the CPU lane emulator
(tests/emu/emu_cleanup.cpp) against ``builder.clean_cell`` on the cases and with the checks of tests/cleanup_cases.py - the ones
tests/test_gpu_cleanup.py runs on the device - and the host side of ``ArrayPSFBuilder(..., cleanup=...)``.

``ArrayPSFBuilder.build`` needs a stack of patches; here ``builder._Stack`` is replaced by ``cleanup_cases.EmulatedStack``, the
three kernels on their emulators.
"""

import ctypes
import inspect

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native
from regularizepsf_amd import builder as bld
from tests import cleanup_cases as cc


@pytest.mark.parametrize("n", cc.SIZES)
def test_emulated_kernel_per_size_against_clean_cell(n):
    case = cc.size_case(n)
    out, flags = cc.emu_clean(case["cells"])
    cc.check(case, out, flags, f"emulator N = {n}")
    assert np.isnan(out[0]).all() and np.isnan(out[-1]).all()  # the all-zero cell, first and after a normal one
    if n >= 16:
        assert not case["flags"].any()  # from 16 on every recipe has a ring: all of them are compared


@pytest.mark.parametrize("n", cc.LABEL_SIZES)
def test_emulated_kernel_on_the_labelling_cells(n):
    case = cc.label_case(n)
    out, flags = cc.emu_clean(case["cells"])
    cc.check(case, out, flags, f"emulator labelling N = {n}")


def test_emulated_kernel_flags_the_degenerate_ring_and_the_host_takes_over():
    case = cc.degenerate_case()
    out, flags = cc.emu_clean(case["cell"][None])
    assert flags.tolist() == [cc.DEGENERATE] and cc.same_bits(out[0], case["cell"])
    # as a model: one patch, the mean of one sample is the patch over its centre, cell / 2 - as degenerate as the cell
    stack = cc.EmulatedStack(8)
    stack.load(case["cell"].astype(np.float32)[None])
    got = bld.model_on_device(stack, "mean", 50.0, np.array([0, 1]), np.array([0]))
    assert cc.same_bits(got[0], bld.clean_cell(case["cell"] / 2.0))


def test_lds_fits_and_two_workgroups_of_64_share_a_cu():
    lds = {n: cc.emulator().emuc_lds_bytes(n) for n in (4, 64, 65, 128)}
    assert lds[128] == 128 * 128 * 4 + 64 + 2 * 128 * 128 == 98368 <= 160 * 1024
    assert lds[64] <= 32 * 1024 and lds[4] >= (256 + 16 + 16) * 40  # the reductions' partial sums need more than a 4 x 4 cell's labels


@pytest.mark.parametrize("name", cc.MODEL_SIZES)
def test_emulated_model_is_average_then_clean(name):
    stack = cc.EmulatedStack(cc.model_case(name)["n"])
    cc.fill(stack, name)
    cc.check_model_is_average_then_clean(stack, name)


@pytest.mark.parametrize("name", ("n16", "n15"))
def test_build_with_device_cleanup_against_host_cleanup_on_the_emulators(name, monkeypatch):
    monkeypatch.setattr(bld, "_Stack", cc.EmulatedStack)
    cc.check_build(name)


def test_cleanup_argument():
    last = list(inspect.signature(rp.ArrayPSFBuilder).parameters.values())[-1]
    assert (last.name, last.default, last.kind) == ("cleanup", "host", inspect.Parameter.KEYWORD_ONLY)
    assert "cleanup" not in inspect.signature(rp.ArrayPSFBuilder.build).parameters  # build keeps the reference's list plus stars
    assert rp.ArrayPSFBuilder(16).cleanup == "host" and rp.ArrayPSFBuilder(16, cleanup="device").cleanup == "device"
    for bad in ("gpu", "Device", None, 1):
        with pytest.raises(ValueError, match="cleanup"):
            rp.ArrayPSFBuilder(16, cleanup=bad)


def test_host_cleanup_never_touches_the_new_entry_points(monkeypatch):
    from tests import builder_cases as bc

    def forbidden(*args):  # noqa: ARG001
        raise AssertionError("a build with cleanup='host' called a clean-up entry point")

    class HostOnlyStack(cc.EmulatedStack):
        clean = model = forbidden

    lib = _native.lib()
    for name in ("rpsf_builder_clean", "rpsf_builder_model", "rpsf_builder_clean_ms"):
        monkeypatch.setattr(lib, name, forbidden)
    monkeypatch.setattr(bld, "_Stack", HostOnlyStack)
    monkeypatch.setattr(bld, "model_on_device", forbidden)
    g = bc.load("n15")
    for kw in ({}, {"cleanup": "host"}):
        psf, counts = rp.ArrayPSFBuilder(15, **kw).build(g["frames"], stars=g["stars"], **bc.thresholds("n15"))
        assert np.isfinite(psf.values[np.array(list(counts.values())) > 0]).all()
    with pytest.raises(AssertionError, match="clean-up entry point"):
        rp.ArrayPSFBuilder(15, cleanup="device").build(g["frames"], stars=g["stars"], **bc.thresholds("n15"))


def test_clean_entry_points_return_codes_for_null_arguments():
    lib = _native.lib()
    ms = ctypes.c_double(7.0)
    assert lib.rpsf_builder_clean(None, 1, None, None, None) == _native.E_BADARG and b"null" in lib.rpsf_last_error()
    assert lib.rpsf_builder_model(None, 0, 50.0, 1, None, None, None, None) == _native.E_BADARG
    assert lib.rpsf_builder_clean_ms(None, ctypes.byref(ms)) == _native.E_BADARG and ms.value == 7.0
