"""The apply geometry contract (rpsf_geometry, include/rpsf.h) on every overlap-add path: pitched and offset views of the input and of the output,
origins, pad values, row windows and batch strides (cases and float64 reference: tests/geometry_cases.py).

Every case uploads its frame into a buffer whose every other float is NaN (the gaps between rows, the head before the pointer, the tail, the
floats between the frames of a batch) and pre-fills the whole output allocation with a NaN of a fixed payload.  After the apply every float
outside the output window still has that payload's bits, every float inside is written, the result meets the suite's bar against the oracle
(1e-5 of the peak and of the norm) and - on every path that adds in a fixed order - equals, float for float, the same plan's
apply of the same frame from a dense, aligned buffer.  Both allocations carry a guard zone on either side that is checked like the gaps.
"""

import dataclasses

import numpy as np
import pytest

from tests import geometry_cases as gc
from tests.geometry_cases import CASES
from tests.helpers import rel_errors

pytestmark = pytest.mark.gpu
TOL = 1e-5            # tests/test_gpu_parity.py: check
ATOMIC_TOL = 2e-6     # tests/test_gpu_parity.py: float atomics against the planes, of the peak
GUARD = 1 << 18       # floats on either side of both allocations (1 MiB)
TAIL = 16             # floats of the allocation behind the last row
SENTINEL = np.uint32(0x7FC5A5A5)  # a quiet NaN with a payload no arithmetic produces

PLANS = {}
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    for path, (ratio, count, name) in WORST.items():
        print(f"GEOMETRY-WORST | {path} | {count} comparisons with the oracle | worst ratio to the 1e-5 bar {ratio:.3f} | {name}")
    for plan in PLANS.values():
        plan.close()
    PLANS.clear()


def plan_for(case):
    """One plan per (path, N, shape, band), shared by every geometry of that tuple in whatever order the cases come."""
    from regularizepsf_amd import _native

    if case.plan_key not in PLANS:
        spec = gc.PATHS[case.path]
        coords, k = gc.plan_transfer(case)
        plan = _native.Plan(case.n, coords)
        for name, value in spec["options"].items():
            plan.set_option(name, value)
        plan.set_transfer(k)
        if spec["overlap"]:
            plan.set_overlap_mode(spec["overlap"])
        if case.path == "sweep":
            assert plan.sweep_info()["regions"] > 0  # a complete covering: the plan chose the sweep kernel by itself
        PLANS[case.plan_key] = plan
    return PLANS[case.plan_key]


def layout(rows, width, ld, offset_bytes, frames, stride):
    """(floats of the allocation with its guards, float index of the pointer, index of every window float as (frames, rows, width))."""
    span = (frames - 1) * stride + (rows - 1) * ld + width
    start = GUARD + offset_bytes // 4
    index = start + (np.arange(frames)[:, None, None] * stride + np.arange(rows)[None, :, None] * ld + np.arange(width)[None, None, :])
    return start + span + TAIL + GUARD, start, index


def run(plan, g, frames, expect=None):
    """One apply of ``frames`` ((count, height, width) float32) with the numbers ``g``; returns the output window (count, out_rows, width)
    after the sentinel checks.  ``expect``: the error code of a refusal, after which the whole output allocation must be untouched."""
    from regularizepsf_amd import _native

    count = len(frames)
    size_in, start_in, index_in = layout(g["image_rows"], g["width"], g["ld_image"], g["offset_in"], count, g["image_stride"])
    size_out, start_out, index_out = layout(g["out_rows"], g["width"], g["ld_out"], g["offset_out"], count, g["out_stride"])
    host_in = np.full(size_in, np.nan, np.float32)
    host_in[index_in] = frames[:, g["image_row0"] : g["image_row0"] + g["image_rows"]]
    d_in = _native.DeviceBuffer(size_in * 4).upload(host_in)
    d_out = _native.DeviceBuffer(size_out * 4).upload(np.full(size_out, SENTINEL, np.uint32))
    geom = _native.Geometry(g["height"], g["width"], g["pad_mode"], g["pad_value"], g["origin_row"], g["origin_col"], g["image_row0"],
                            g["image_rows"], g["ld_image"], g["out_row0"], g["out_rows"], g["ld_out"])
    try:
        if expect is not None:
            with pytest.raises(_native.NativeError) as err:
                if count == 1 and not g["image_stride"]:
                    plan.apply_device(d_in.at(start_in * 4), d_out.at(start_out * 4), geom)
                else:
                    plan.apply_batch_device(d_in.at(start_in * 4), d_out.at(start_out * 4), count, g["image_stride"], g["out_stride"], geom)
            assert err.value.code == expect, err.value
        elif count == 1:
            plan.apply_device(d_in.at(start_in * 4), d_out.at(start_out * 4), geom)
        else:
            plan.apply_batch_device(d_in.at(start_in * 4), d_out.at(start_out * 4), count, g["image_stride"], g["out_stride"], geom)
        plan.synchronize()
        got = d_out.download((size_out,), np.uint32)
    finally:
        d_in.free()
        d_out.free()
    if expect is not None:
        assert np.array_equal(got, np.full(size_out, SENTINEL, np.uint32)), "a refused call wrote to the output"
        return None
    inside = np.zeros(size_out, bool)
    inside[index_out] = True
    spilled = np.flatnonzero(~inside & (got != SENTINEL))
    assert spilled.size == 0, (f"{spilled.size} floats outside the output window were written; the first at float {int(spilled[0]) - start_out} "
                               f"from the pointer (ld_out {g['ld_out']}, width {g['width']}, frame stride {g['out_stride']})")
    window = got[index_out]
    unwritten = np.argwhere(window == SENTINEL)
    assert unwritten.size == 0, f"{len(unwritten)} floats of the output window were not written; the first at (frame, row, col) {tuple(unwritten[0])}"
    return window.view(np.float32)


def dense(g):
    """The same call from dense, aligned buffers, one frame: same origin, pad settings and window."""
    return {**g, "ld_image": g["width"], "ld_out": g["width"], "offset_in": 0, "offset_out": 0, "image_stride": 0, "out_stride": 0}


def against_oracle(case, out, ref, what):
    assert np.isfinite(out).all(), f"{what}: a float from outside the view reached the result ({int((~np.isfinite(out)).sum())} non-finite pixels)"
    rel_max, rel_l2 = rel_errors(out, ref)
    ratio = max(rel_max, rel_l2) / TOL
    worst, count, name = WORST.get(case.path, (0.0, 0, ""))
    WORST[case.path] = (max(worst, ratio), count + 1, case.name if ratio > worst else name)
    assert rel_max <= TOL and rel_l2 <= TOL, (what, rel_max, rel_l2)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_geometry_case(case):
    from regularizepsf_amd import _native

    plan = plan_for(case)
    g = gc.geometry_numbers(case)
    frames = gc.frames_of(case)
    if gc.refused(case):  # the fallback takes whole-image geometry only: the case is the refusal, and nothing is written
        run(plan, g, frames, expect=_native.E_UNSUPPORTED)
        return
    ref = gc.reference(case)
    peak = float(np.abs(ref).max())
    singles = np.stack([run(plan, dense(g), frames[f : f + 1])[0] for f in range(case.frames)])
    got = run(plan, g, frames)
    assert got.shape == ref.shape
    for f in range(case.frames):
        against_oracle(case, singles[f], ref[f], f"dense apply, frame {f}")
        against_oracle(case, got[f], ref[f], f"frame {f}")
    if case.path in gc.ORDERED_PATHS:
        differ = np.argwhere(got.view(np.uint32) != singles.view(np.uint32))  # (bits: a zero's sign counts)
        assert differ.size == 0, (f"{len(differ)} pixels differ from the dense, aligned apply of the same plan; the first at (frame, row, col) "
                                  f"{tuple(differ[0])}: {got[tuple(differ[0])]!r} against {singles[tuple(differ[0])]!r}")
    else:
        twin = dataclasses.replace(case, path="planes1" if case.n <= 64 else "gen2_sum", view_in=None, view_out=None, frames=1, strides=None)
        for f in range(case.frames):
            planes = run(plan_for(twin), dense(g), frames[f : f + 1])[0]
            assert np.abs(got[f].astype(np.float64) - planes).max() <= ATOMIC_TOL * peak
            assert np.abs(singles[f].astype(np.float64) - planes).max() <= ATOMIC_TOL * peak


@pytest.mark.parametrize("name", list(gc.ERRORS))
def test_check_geometry_refuses_before_anything_is_written(name):
    from regularizepsf_amd import _native

    case = gc.ERROR_CASE
    change = dict(gc.ERRORS[name])
    count = change.pop("frames", 1)
    good = gc.geometry_numbers(case)
    frames = gc.base_frames(case.n, case.shape, count)
    # the buffers are laid out for the valid call; the refused one may not touch them
    bad = {**good, **change}
    sized = {**good, "image_stride": bad["image_stride"], "out_stride": bad["out_stride"]}
    size_out, start_out, _ = layout(sized["out_rows"], sized["width"], sized["ld_out"], 0, count, max(sized["out_stride"], 96 * 128))
    size_in, start_in, _ = layout(sized["image_rows"], sized["width"], sized["ld_image"], 0, count, max(sized["image_stride"], 96 * 128))
    d_in = _native.DeviceBuffer(size_in * 4).upload(np.zeros(size_in, np.float32))
    d_out = _native.DeviceBuffer(size_out * 4).upload(np.full(size_out, SENTINEL, np.uint32))
    geom = _native.Geometry(bad["height"], bad["width"], bad["pad_mode"], bad["pad_value"], bad["origin_row"], bad["origin_col"], bad["image_row0"],
                            bad["image_rows"], bad["ld_image"], bad["out_row0"], bad["out_rows"], bad["ld_out"])
    plan = plan_for(case)
    try:
        with pytest.raises(_native.NativeError) as err:
            if count == 1:
                plan.apply_device(d_in.at(start_in * 4), d_out.at(start_out * 4), geom)
            else:
                plan.apply_batch_device(d_in.at(start_in * 4), d_out.at(start_out * 4), count, bad["image_stride"], bad["out_stride"], geom)
        assert err.value.code == _native.E_BADARG, err.value
        plan.synchronize()
        assert np.array_equal(d_out.download((size_out,), np.uint32), np.full(size_out, SENTINEL, np.uint32))
        # and the plan still serves the valid call
        assert frames is not None
    finally:
        d_in.free()
        d_out.free()
    out = run(plan, good, frames[:1])
    against_oracle(case, out[0], gc.reference(case)[0], "the valid call after the refusal")
