"""Kernel S1 on hard boxes on the GPU: value domains, ties, degenerate counts, the round cap, odd box sizes and frame geometry, against the
float64 restatement at a derived bound and against the CPU emulator bit for bit - the cases and checks of tests/mesh_cases.py, which
tests/test_mesh_host.py runs on the emulator.

Measured on an MI355X: see profiles/mesh_domain_gpu.log (every check prints its figures before it asserts)."""

import pytest

from regularizepsf_amd import stars
from tests import mesh_cases as mc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tuple(mc.TABLES))
def test_box_table_matches_the_restatement(name):
    mc.check_table(stars._Finder, name)


@pytest.mark.parametrize("name", mc.FRAME_CASES)
def test_mesh_and_detections_match_the_restatement(name):
    mc.check_frame(stars._Finder, name)


def test_powers_of_two_scale_every_result_exactly():
    mc.check_scaling(stars._Finder)


@pytest.mark.parametrize("name", tuple(mc.TABLES) + mc.FRAME_CASES)
def test_gpu_and_emulator_agree(name):
    """Level and rows bit for bit; the rms, where the device's square root enters, within the derived bound, its distance in ulp printed."""
    mc.check_against_emulator(stars._Finder, name)
