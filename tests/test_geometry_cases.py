"""The case table of tests/test_gpu_geometry.py checked without a GPU: its three reference constructions agree where they overlap, the table
holds a case on each side of every predicate the library's launch paths branch on, and every case is one check_geometry admits."""

import numpy as np
import pytest

from oracle import regpsf_oracle as orc
from tests import geometry_cases as gc
from tests.geometry_cases import CASES, Case


def close(a, b):
    return a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("n, shape, pad_mode", [(32, (70, 90), "symmetric"), (16, (40, 50), "wrap"), (24, (96, 121), "reflect")])
def test_origin_2n_on_a_host_padded_frame_is_the_plain_oracle(n, shape, pad_mode):
    case = Case("sweep", n, shape, pad_mode, origin=(2 * n, 2 * n), host_padded=True)
    assert gc.admitted(case) and not gc.admitted(Case("sweep", n, shape, pad_mode, origin=(2 * n, 2 * n)))
    coords, k = gc.plan_transfer(case)
    plain = orc.apply_transfer(gc.base_frames(n, shape, 1)[0], coords, k, pad_mode=pad_mode)
    got = gc.reference(case)[0]
    assert got.shape == (shape[0] + 4 * n, shape[1] + 4 * n)
    p = 2 * n
    assert close(got[p:-p, p:-p], plain)
    # what the corners never reach stays zero
    far = got.copy()
    far[p - n // 2 : -(p - n), p - n // 2 : -(p - n)] = 0
    assert not far.any()


@pytest.mark.parametrize("n, shape", [(32, (70, 90)), (16, (40, 64)), (9, (40, 33))])
def test_pad_value_zero_is_the_plain_constant_oracle_and_a_value_shows(n, shape):
    coords, k = gc.transfer(n, shape)
    image = gc.base_frames(n, shape, 1)[0]
    plain = orc.apply_transfer(image, coords, k, pad_mode="constant")
    assert close(gc.reference_by_padding(image, coords, k, n, 0.0), plain)
    assert close(gc.reference(Case("sweep", n, shape, "constant"))[0], plain)
    valued = gc.reference(Case("sweep", n, shape, "constant", pad_value=-7.25))[0]
    assert np.abs(valued - plain).max() > 1e-3 * np.abs(plain).max()  # the rim sees the value
    inner = (slice(n, shape[0] - n), slice(n, shape[1] - n))
    if valued[inner].size:
        assert close(valued[inner], plain[inner])                     # nothing else does
    # under another pad mode the value is not read
    assert np.array_equal(gc.reference(Case("sweep", n, shape, "symmetric", pad_value=-7.25)), gc.reference(Case("sweep", n, shape, "symmetric")))


def test_origin_reference_moves_with_the_frame():
    """Corners shifted by (3, 5) on a frame that is the original moved by (3, 5), constant padding: the interior is the original result moved."""
    n, shape = 16, (40, 64)
    coords, k = gc.transfer(n, shape)
    image = gc.base_frames(n, shape, 1)[0]
    moved = np.zeros((shape[0] + 3, shape[1] + 5), np.float32)
    moved[3:, 5:] = image
    a = orc.apply_transfer(image, coords, k, pad_mode="constant")
    b = gc.reference_by_shift(moved, coords, k, "constant", (3, 5))
    assert close(b[3:, 5:], a)


@pytest.mark.parametrize("n, shape", [(32, (96, 128)), (128, (384, 256)), (24, (96, 120))])
@pytest.mark.parametrize("world", [2, 3])
def test_bands_stitched_together_are_the_whole_frame(n, shape, world):
    whole = gc.reference(Case("sweep", n, shape))[0]
    parts, row = [], 0
    for rank in range(world):
        case = Case("sweep", n, shape, window=(world, rank))
        g = gc.geometry_numbers(case)
        assert g["out_row0"] == row
        row += g["out_rows"]
        parts.append(gc.reference(case)[0])
    assert row == shape[0]
    assert close(np.concatenate(parts), whole)


FACTS = sorted(gc.facts(CASES[0]))


@pytest.mark.parametrize("path", list(gc.PATHS))
def test_every_path_has_a_case_on_each_side_of_every_predicate(path):
    mine = [c for c in CASES if c.path == path and not gc.refused(c)]
    assert mine
    seen = {f: set() for f in FACTS}
    for c in mine:
        for f, v in gc.facts(c).items():
            seen[f].add(v)
    for f in FACTS:
        if f in gc.EXEMPT.get(path, ()):
            continue
        assert seen[f] == {True, False}, f"{path}: the table has only the {seen[f]} side of '{f}'"
    # the combinations the predicates take as a whole: everything aligned with a pitch (view A), and a multiple of 32 on an odd origin
    assert any(c.view_in == "A" and c.view_out == "A" for c in mine)
    assert {c.n for c in mine} == set(gc.PATHS[path]["sizes"])
    for n in gc.PATHS[path]["sizes"]:
        for shape in gc.SHAPES[n]:
            views = {(c.view_in, c.view_out) for c in mine if c.n == n and c.shape == shape and c.frames == 1 and not c.window and c.origin == (0, 0)}
            for v in gc.VIEWS:
                assert {(v, None), (None, v), (v, v)} <= views, (path, n, shape, v)


def test_the_shapes_are_what_the_table_says():
    for n, shapes in gc.SHAPES.items():
        if n != 9:
            assert shapes[0][1] % 4 == 0 and shapes[-1][1] % 4 != 0
        if n not in (24, 9):
            assert all(s[1] % 32 == 0 for s in shapes[:-1])
    for name, (offset, extra) in gc.VIEWS.items():
        assert offset % 4 == 0 and extra > 0, name
    assert [(o % 16 == 0, o % 8 == 0, e % 4 == 0, e % 2 == 0) for o, e in gc.VIEWS.values()] == [
        (True, True, True, True), (False, True, False, True), (False, False, False, False), (True, True, False, False)]


def test_thinned_families_are_present_on_every_path():
    for path in gc.PATHS:
        mine = [c for c in CASES if c.path == path]
        n = gc.THIN_SIZE[path]
        pairs = {(c.pad_mode, c.origin) for c in mine if c.view_in is None and c.view_out is None and c.frames == 1 and not c.window and not c.pad_value}
        for mode in gc.KERNEL_PAD_MODES:
            for origin in gc.origins(n):
                assert (mode, origin) in pairs, (path, mode, origin)
        assert {c.pad_value for c in mine if c.pad_mode == "constant"} == set(gc.PAD_VALUES)
        assert any(c.pad_value and c.pad_mode == "symmetric" for c in mine)
        assert {c.strides for c in mine if c.frames > 1} == {"odd", "mult4"}
        windows = [c for c in mine if c.window]
        assert {c.view_in for c in windows} == {"B", "C"}, path
        for c in windows:
            g = gc.geometry_numbers(c)
            assert g["image_row0"] > 0 and g["out_row0"] > 0 and g["ld_image"] > g["width"] and g["ld_out"] > g["width"]
        assert {c.window[0] for c in windows} == {2, 3}, path
        assert all(gc.refused(c) == (path == "fallback") for c in windows)
    for c in CASES:
        if c.frames > 1:
            g = gc.geometry_numbers(c)
            assert g["image_stride"] % 4 == g["out_stride"] % 4 == 0 or c.strides == "odd"
            if c.strides == "odd":
                assert g["image_stride"] == g["image_rows"] * g["ld_image"] + 1 and g["out_stride"] == g["out_rows"] * g["ld_out"] + 3


def test_every_case_is_one_check_geometry_admits_and_every_error_is_not():
    assert 300 <= len(CASES) <= 1000
    for c in CASES:
        assert gc.admitted(c), c.name
        h, w = c.frame_shape
        assert h * w <= 512 * 768 or c.host_padded, c.name
    base = gc.geometry_numbers(gc.ERROR_CASE)
    coords = gc.plan_transfer(gc.ERROR_CASE)[0]
    n = gc.ERROR_CASE.n
    for name, change in gc.ERRORS.items():
        g = {**base, **{k: v for k, v in change.items() if k != "frames"}}
        rows = [r + g["origin_row"] for r, _ in coords]
        cols = [c + g["origin_col"] for _, c in coords]
        ok = g["ld_image"] >= g["width"] and g["ld_out"] >= g["width"]
        ok = ok and g["image_rows"] > 0 and g["image_row0"] + g["image_rows"] <= g["height"] and g["out_rows"] > 0 and g["out_row0"] + g["out_rows"] <= g["height"]
        ok = ok and min(rows) >= -2 * n and max(rows) <= g["height"] + n and min(cols) >= -2 * n and max(cols) <= g["width"] + n
        if change.get("frames", 1) > 1:
            ok = ok and g["image_stride"] >= (g["image_rows"] - 1) * g["ld_image"] + g["width"]
            ok = ok and g["out_stride"] >= (g["out_rows"] - 1) * g["ld_out"] + g["width"]
        assert not ok, name
