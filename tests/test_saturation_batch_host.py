"""The batched device saturation route on the CPU lane emulator (tests/emu/emu_saturation_batch.cpp runs the batch drivers of
csrc/rpsf_core_saturation_batch.hpp, the code the GPU runs), and the surface that needs no GPU.

Every frame of a stack must come out with the bits of ``saturation_cases.reference_fill`` of that frame alone, NaN positions included,
and with SciPy's mask: a batch shares launches, never data.  tests/test_gpu_saturation_batch.py holds the GPU to the same cases.
"""

import re

import numpy as np
import pytest

from regularizepsf_amd import _native
from tests import saturation_batch_cases as bc
from tests import saturation_cases as sc

RUN = bc.emu_fill_batch


# 1 - 4: one stack of every frame kind, an odd padded size, one layout with different values, a fully hot frame between ordinary ones
@pytest.mark.parametrize("name", ["kinds_wrap", "kinds_edge", "odd_stride", "same_layout", "around_fully_hot"])
def test_every_frame_of_a_stack_has_the_bits_of_its_own_reference(name):
    bc.precondition(name)
    got = bc.run_stack(RUN, name)
    bc.check_against_reference(got, name, single_groups=bc.emu_single_groups(name))
    assert got[3][1] == 1


def test_a_batch_in_which_nothing_is_hot_has_no_groups():
    bc.precondition("nothing_hot")
    got = bc.run_stack(RUN, "nothing_hot")
    bc.check_against_reference(got, "nothing_hot")
    assert got[3] == (3, 1, 0, 0)


# 5
def test_the_cut_into_frame_groups_changes_no_bit():
    bc.precondition("the_cut")
    whole = bc.run_stack(RUN, "the_cut", group=0)
    bc.check_against_reference(whole, "the_cut")
    assert whole[3][1] == 1
    for group, frame_groups in ((1, 5), (2, 3)):
        cut = bc.run_stack(RUN, "the_cut", group=group)
        bc.check_same_results(cut, whole, f"frame-groups of {group}")
        assert cut[3] == (5, frame_groups, whole[3][2], whole[3][3])
    for bad in (-1, 65536):
        with pytest.raises(ValueError, match="bad argument"):
            bc.run_stack(RUN, "the_cut", group=bad)


# 6
def test_the_order_in_which_f4_takes_the_groups_changes_no_bit():
    bc.precondition("order")
    longest_first = bc.run_stack(RUN, "order")
    bc.check_against_reference(longest_first, "order")
    for order in (bc.ORDER_REVERSED, bc.ORDER_FRAMES):
        bc.check_same_results(bc.run_stack(RUN, "order", order=order), longest_first, f"order {order}")


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_a_frame_group_of_one_is_the_single_frame_emulator_bit_for_bit_in_every_order(name):
    """The device route has one driver, and a single frame is a frame-group of one: the batch drivers must give such a group what the
    per-thread functions give the frame when they are driven directly (tests/emu/emu_saturation.cpp)."""
    _, n, _, pad_mode, (dilation, width) = sc.CASES[name]
    want, want_mask, want_groups = sc.emu_fill(sc.frame(name), n, pad_mode, dilation, width)
    for order in (bc.ORDER_LONGEST_FIRST, bc.ORDER_REVERSED, bc.ORDER_FRAMES):
        padded, masks, groups, info = bc.emu_fill_batch([sc.frame(name)], n, pad_mode, dilation, width, order=order)
        assert padded.shape == (1, *want.shape) and np.array_equal(padded[0].view(np.uint32), want.view(np.uint32)), (name, order)
        assert np.array_equal(masks[0], want_mask), (name, order)
        assert list(groups) == [want_groups] and info[:3] == (1, 1, want_groups), (name, order)


def test_restore_gives_every_frame_its_own_values_crop_and_list():
    name = "kinds_edge"
    _, n, (h, w), pad_mode, (dilation, width) = bc.STACKS[name]
    frames, ref = bc.stack(name), bc.reference(name)
    rng = np.random.default_rng(5)
    for out_row0, rows in ((2 * n, h), (0, h + 4 * n)):  # the compiled plans hand back the caller's rows, a generic-size plan the whole frame
        corrected = rng.standard_normal((len(frames), rows * (w + 4 * n) + 2)).astype(np.float32)
        outs, lists = bc.emu_restore_batch(frames, n, pad_mode, dilation, width, corrected, out_row0)
        for f, (_, mask, _) in enumerate(ref):
            inner = mask[2 * n : 2 * n + h, 2 * n : 2 * n + w]
            rows_f = corrected[f, : rows * (w + 4 * n)].reshape(rows, w + 4 * n)
            want = np.where(inner, frames[f], rows_f[2 * n - out_row0 : 2 * n - out_row0 + h, 2 * n : 2 * n + w])
            sc.assert_same_bits(outs[f], want, f"frame {f}")
            assert np.array_equal(lists[f], np.flatnonzero(inner)), f


def test_header_ctypes_and_library_have_the_batch_entry_points():
    import pathlib

    header = (pathlib.Path(__file__).resolve().parent.parent / "include" / "rpsf.h").read_text()
    for name in ("rpsf_apply_batch_device_saturated", "rpsf_apply_frames_host_saturated_device", "rpsf_saturation_batch_info",
                 "rpsf_saturation_fill_batch_device"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _native._PROTOTYPES
        assert hasattr(_native.lib(), name)
    assert re.search(r"RPSF_OPT_SAT_GROUP = 10\b", header) and _native.Plan.OPTIONS["sat_group"] == 10
