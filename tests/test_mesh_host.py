"""Kernel S1 on hard boxes without a GPU: the driver of csrc/rpsf_core_stars.hpp on the CPU emulator through the cases and checks of
tests/mesh_cases.py, which tests/test_gpu_mesh.py runs on the device, and S1's LDS carve for every box size."""

import pytest

from tests import mesh_cases as mc
from tests import star_cases as sc


def test_lds_records_start_on_16_bytes_for_every_box():
    mc.check_carve()


def test_tracing_twin_returns_the_restatements_bits_and_the_bound_is_no_looser():
    """mesh_reference asserts per box that trace_box returns ref_box's level, rms and gap bit for bit."""
    mc.check_bound_is_no_looser()


@pytest.mark.parametrize("name", tuple(mc.TABLES))
def test_box_table_matches_the_restatement(name):
    mc.check_table(sc.EmuFinder, name)


@pytest.mark.parametrize("name", mc.FRAME_CASES)
def test_mesh_and_detections_match_the_restatement(name):
    mc.check_frame(sc.EmuFinder, name)


def test_powers_of_two_scale_every_result_exactly():
    mc.check_scaling(sc.EmuFinder)
