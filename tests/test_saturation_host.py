"""The saturation branch's device kernels F1 - F5 on the CPU lane emulator (tests/emu/emu_saturation.cpp runs the drivers of
csrc/rpsf_core_saturation.hpp, the code the GPU runs), and the Python surface that needs no GPU.

The filled padded frame must have the bits of the host route's fill (``rpsf_saturation_fill``) on the NumPy-padded float32 frame,
NaN positions included, and the mask must be SciPy's.  tests/test_gpu_saturation.py holds the GPU to the same cases.
"""

import re

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native
from tests import saturation_cases as sc


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_filled_padded_frame_and_mask_have_the_host_fills_bits(name):
    sc.precondition(name)
    _, n, _, pad_mode, (dilation, width) = sc.CASES[name]
    want, mask, _ = sc.reference(name)
    got, got_mask, groups = sc.emu_fill(sc.frame(name), n, pad_mode, dilation, width)
    assert np.array_equal(got_mask, mask)
    sc.assert_same_bits(got, want, name)
    assert (groups == 0) == (not mask.any())


@pytest.mark.parametrize("name", ["pair_h", "pair_h_plus_1", "mixed", "fully_hot"])
def test_the_order_in_which_groups_are_taken_does_not_matter(name):
    _, n, _, pad_mode, (dilation, width) = sc.CASES[name]
    forward, _, groups = sc.emu_fill(sc.frame(name), n, pad_mode, dilation, width)
    backward, _, _ = sc.emu_fill(sc.frame(name), n, pad_mode, dilation, width, reverse=True)
    sc.assert_same_bits(backward, forward, name)
    assert groups >= 1


def test_groups_blobs_h_apart_share_one_and_blobs_further_apart_need_not():
    """h = 3, box reach 1: masked pixels 3 apart are joined by their boxes, 4 apart they are not."""
    for name, want in (("pair_h", 1), ("pair_h_plus_1", 2)):
        _, n, _, pad_mode, (dilation, width) = sc.CASES[name]
        assert sc.emu_fill(sc.frame(name), n, pad_mode, dilation, width)[2] == want


@pytest.mark.parametrize("name", ["corners_edges", "mixed_edge", "nothing_hot"])
def test_restore_writes_the_raw_values_on_the_mask_crops_and_lists_the_masked_pixels(name):
    _, n, (h, w), pad_mode, (dilation, width) = sc.CASES[name]
    image = sc.frame(name)
    _, mask, _ = sc.reference(name)
    rng = np.random.default_rng(5)
    for out_row0, rows in ((2 * n, h), (0, h + 4 * n)):  # the compiled plans hand back the caller's rows, a generic-size plan the whole frame
        corrected = rng.standard_normal((rows, w + 4 * n)).astype(np.float32)
        out, listed = sc.emu_restore(image, n, pad_mode, dilation, width, corrected, out_row0)
        inner = mask[2 * n : 2 * n + h, 2 * n : 2 * n + w]
        want = np.where(inner, image, corrected[2 * n - out_row0 : 2 * n - out_row0 + h, 2 * n : 2 * n + w])
        sc.assert_same_bits(out, want, name)
        assert np.array_equal(listed, np.flatnonzero(inner))


def test_saturation_keyword_default_values_and_property():
    cube = rp.IndexedCube([(0, 0)], np.ones((1, 16, 16), np.complex64))
    t = rp.ArrayPSFTransform(cube)
    assert t.saturation == "host"
    assert rp.ArrayPSFTransform(cube, saturation="device").saturation == "device"
    t.saturation = "device"
    assert t.saturation == "device"
    with pytest.raises(ValueError, match="saturation"):
        t.saturation = "gpu"
    with pytest.raises(ValueError, match="saturation"):
        rp.ArrayPSFTransform(cube, saturation="auto")
    assert t.saturation == "device"


def test_header_and_ctypes_declare_the_new_entry_points():
    import pathlib

    header = (pathlib.Path(__file__).resolve().parent.parent / "include" / "rpsf.h").read_text()
    for name in ("rpsf_apply_device_saturated", "rpsf_apply_host_saturated_device", "rpsf_saturation_kernel_ms", "rpsf_saturation_fill_device"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _native._PROTOTYPES
        assert hasattr(_native.lib(), name)
