"""Every operation of a plan and every launch option around pipelined applies (RPSF_OPT_PIPELINE, csrc/rpsf_lanes.hpp).

Everything that is not a pipelined apply must first join the plan's two launch lanes.  tests/pipeline_cases.py puts each operation of
`_native.Plan` between pipelined applies that are still in flight - behind one, two and three of them, so that the last one runs on lane 0
with lane 1 idle, on lane 1, and on lane 0 with lane 1 busy - and this module compares, byte for byte, every device buffer and every host
array with the same calls made on one lane with a synchronise behind each.  The lane report (`Plan.lane_info`) then has to show that the
sequence really was pipelined where it should be and really was not where it should not: its deltas are the ones the CPU replay of the same
sequence gives (tests/test_lanes_host.py), written once in pipeline_cases.EXPECTED.

The shapes are those of tests/test_gpu_pipeline.py.  One one-lane frame per shape is tied to the float64 reference under the bar of
tests/test_gpu_local_parity.py (MARGIN x the float32 yardstick of the same case); everything else is byte equality.  No test provokes a gate
wait that runs out: `Run.finish` checks after every sequence that the plan's error word is clear.

The sharded step of regularizepsf_amd/sharding.py behind pipelined applies of a band's plan runs in two processes, in
tests/test_gpu_sharding.py::test_sharded_step_behind_pipelined_applies.  (Its bands are plans of their own, not views of one plan; the only views
of a plan are the row bands of a host frame, which `apply_banded` runs.)

Removing a join and what caught it, measured once on an MI355X, is in profiles/pipeline_ops_gpu.log.
"""

import numpy as np
import pytest

from tests import pipeline_cases as pc
from tests.helpers import MARGIN, local_error, per_patch_reference

pytestmark = pytest.mark.gpu


def _case(index):
    c = pc.case_for(pc.SHAPES[index])
    c.plan.synchronize()
    return c


def _report(what, lanes, expected):
    print(f"LANES | {what} | lane 0 {lanes[0]}, lane 1 {lanes[1]}, gated {lanes[2]}, joins due {lanes[3]} | expected {expected}")


def _assert_same(got, ref, what):
    assert sorted(got.device) == sorted(ref.device), what
    for name in ref.device:
        assert pc.same_bytes(got.device[name], ref.device[name]), f"{what}: device buffer {name} differs from the one-lane reference"
    assert len(got.host) == len(ref.host), what
    for i, (a, b) in enumerate(zip(got.host, ref.host)):
        assert pc.same_bytes(a, b), f"{what}: host result {i} differs from the one-lane reference"


@pytest.mark.parametrize("shape,name,k", pc.sandwich_ids(), ids=[f"{pc.SHAPES[s][0]}x{pc.SHAPES[s][1]}-{n}-k{k}" for s, n, k in pc.sandwich_ids()])
def test_operation_between_pipelined_applies(shape, name, k):
    case = _case(shape)
    ref = pc.reference_sandwich(case, name, k)
    got = pc.run_sandwich(case, name, k, True)
    expected = pc.EXPECTED[f"{name}-k{k}"]
    _report(f"{name}, prefix {k}, {case.shape}", got.lanes, expected)
    assert ref.lanes == (0, 0, 0, 0), "the reference ran on one lane"
    _assert_same(got, ref, f"{name}, prefix {k}")
    assert got.lanes == expected


@pytest.mark.parametrize("shape", range(len(pc.SHAPES)), ids=[f"{s[0]}x{s[1]}" for s in pc.SHAPES])
def test_one_lane_reference_against_float64(shape):
    """What the byte comparisons of this module compare with is the right answer: one one-lane frame under the bar of
    tests/test_gpu_local_parity.py."""
    case = _case(shape)
    r = pc.Run(case, False).start()
    r.apply("f2", "o1")
    out = r.finish().device["o1"]
    ref, scale = per_patch_reference(case.frames[2], case.coords, case.k[0], "symmetric", np.float64)
    yard, _ = per_patch_reference(case.frames[2], case.coords, case.k[0], "symmetric", np.float32)
    yardstick, error = local_error(yard, ref, scale), local_error(out, ref, scale)
    print(f"FLOAT64 | {case.shape} | yardstick {yardstick:.3e} | one-lane apply {error:.3e} | ratio {error / yardstick:.2f} | margin {MARGIN}")
    assert 0 < yardstick < 1e-6
    assert error <= MARGIN * yardstick


def _loop(case, plan, pipelined, count=pc.LOOP):
    plan.set_option("pipeline", int(pipelined))
    before = plan.lane_info()
    for i in range(count):
        plan.apply_device(case.buf[f"f{pc.loop_frame(i)}"].ptr, case.buf[f"o{i & 1}"].ptr, case.geom)
        if not pipelined:
            plan.synchronize()
    info = plan.lane_info()
    plan.synchronize()
    outs = case.buf["o0"].download(), case.buf["o1"].download()
    plan.apply_device_loop_ms(case.buf["f0"].ptr, case.buf["so0"].ptr, case.geom, 1)  # (the error word is clear)
    return outs, tuple(info[key] - before[key] for key in ("lane0", "lane1", "gated", "joins"))


@pytest.mark.parametrize("setting", list(pc.LOOP_SETTINGS))
def test_forty_applies_under_each_launch_option(setting):
    """The options that change what the gated kernel does - image first-touch, reserved CUs, stagger, head K prefetch - have only ever run
    pipelined at their defaults: the alternating loop of tests/test_gpu_pipeline.py under each, against one lane under the same.  plane_nt and
    k_cached run too, but choose between 128-pixel kernels only: for these 256-pixel plans they are no-ops, and the loop shows just that."""
    case = _case(0)
    plan = case.new_plan()
    pc.LOOP_SETTINGS[setting](plan)
    ref, none = _loop(case, plan, False)
    for name in ("o0", "o1"):
        case.buf[name].upload(case.fill)
    got, lanes = _loop(case, plan, True)
    plan.close()
    _report(f"loop of {pc.LOOP}, {setting}", lanes, pc.EXPECTED["loop"])
    assert none == (0, 0, 0, 0)
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[0], case.fill)
    assert pc.same_bytes(got[0], ref[0]) and pc.same_bytes(got[1], ref[1])
    assert lanes == pc.EXPECTED["loop"]


def test_scratch_grows_in_mid_pipeline():
    """A fresh plan: three pipelined applies of the top row window, three of the whole frame (the planes are reallocated behind a device-wide
    wait and lie elsewhere: a join), a batch of two (the tile counters grow and restart), three more single applies."""
    case = _case(0)
    native = case.native
    h, w = case.shape
    half = h // 2
    top = native.Geometry(h, w, case.pad, 0.0, 0, 0, 0, h, w, 0, half, w)
    d_top = native.DeviceBuffer(half * w * 4)
    results = {}
    for pipelined in (False, True):
        plan = case.new_plan()
        plan.set_option("pipeline", int(pipelined))
        for name in ("o0", "o1", "so0", "so1"):
            case.buf[name].upload(case.fill)
        trace = []

        def step(fn, *reads):
            fn()
            if not pipelined:
                plan.synchronize()
                trace.extend((str(len(trace)), r()) for r in reads)

        before = plan.lane_info()
        for i in range(3):
            step(lambda: plan.apply_device(case.buf[f"f{i}"].ptr, d_top.ptr, top), lambda: d_top.download((half, w)))
        for i in range(3):
            step(lambda: plan.apply_device(case.buf[f"f{i + 1}"].ptr, case.buf[f"o{i & 1}"].ptr, case.geom), case.buf[f"o{i & 1}"].download)
        tops = None if pipelined else trace[2][1]
        step(lambda: plan.apply_batch_device(case.buf["f2"].ptr, case.buf["so0"].ptr, 2, case.npix, case.npix, case.geom), case.buf["so0"].download)
        for i in range(3):
            step(lambda: plan.apply_device(case.buf[f"f{i}"].ptr, case.buf[f"o{i & 1}"].ptr, case.geom), case.buf[f"o{i & 1}"].download)
        info = plan.lane_info()
        plan.synchronize()
        lanes = tuple(info[key] - before[key] for key in ("lane0", "lane1", "gated", "joins"))
        results[pipelined] = [d_top.download((half, w))] + [case.buf[name].download() for name in ("o0", "o1", "so0", "so1")]
        plan.apply_device_loop_ms(case.buf["f0"].ptr, case.buf["so2"].ptr, case.geom, 1)
        plan.close()
        if not pipelined:
            pc.assert_steps_differ(trace, "growth")
            assert lanes == (0, 0, 0, 0) and pc.same_bytes(tops, results[False][0])
    d_top.free()
    _report("growth", lanes, pc.EXPECTED["growth"])
    for got, ref in zip(results[True], results[False]):
        assert pc.same_bytes(got, ref)
    assert lanes == pc.EXPECTED["growth"]


def test_three_pipelined_plans_in_turn():
    """Six plan streams on the four hardware queues a process gets: three plans with different K, thirty applies each, enqueued round-robin
    from one thread; one synchronise at the end; each plan's outputs against its own one-lane loop."""
    case = _case(0)
    native = case.native
    k3 = (case.k[0] + case.k[1]).astype(np.complex64)
    d_k3 = native.DeviceBuffer(k3.nbytes).upload(k3)
    plans = [case.new_plan() for _ in range(3)]
    plans[1].set_transfer_device(case.d_k[1].ptr)
    plans[2].set_transfer_device(d_k3.ptr)
    outs = [native.DeviceBuffer(2 * case.nbytes) for _ in plans]
    slices = [[pc.Slice(o, i, case.shape) for i in range(2)] for o in outs]
    refs = []
    for plan, sl in zip(plans, slices):
        plan.set_option("pipeline", 0)
        for i in range(pc.ROUNDS):
            plan.apply_device(case.buf[f"f{pc.loop_frame(i)}"].ptr, sl[i & 1].ptr, case.geom)
            plan.synchronize()
        refs.append((sl[0].download(), sl[1].download()))
        for s in sl:
            s.upload(case.fill)
        plan.set_option("pipeline", 1)
    before = [p.lane_info() for p in plans]
    for i in range(pc.ROUNDS):
        for plan, sl in zip(plans, slices):
            plan.apply_device(case.buf[f"f{pc.loop_frame(i)}"].ptr, sl[i & 1].ptr, case.geom)
    plans[0].synchronize()
    for n, (plan, sl, ref, b) in enumerate(zip(plans, slices, refs, before)):
        info = plan.lane_info()
        lanes = tuple(info[key] - b[key] for key in ("lane0", "lane1", "gated", "joins"))
        _report(f"plan {n} of three, {pc.ROUNDS} rounds", lanes, pc.EXPECTED["rounds"])
        assert pc.same_bytes(sl[0].download(), ref[0]) and pc.same_bytes(sl[1].download(), ref[1]), n
        assert lanes == pc.EXPECTED["rounds"]
    assert not np.array_equal(refs[0][0], refs[1][0]) and not np.array_equal(refs[0][0], refs[2][0]) and not np.array_equal(refs[1][0], refs[2][0])
    assert not np.array_equal(refs[0][0], refs[0][1])
    for plan in plans:
        plan.apply_device_loop_ms(case.buf["f0"].ptr, case.buf["so0"].ptr, case.geom, 1)
        plan.close()
    for b in (*outs, d_k3):
        b.free()


def test_destroy_behind_pipelined_applies():
    """Six pipelined applies, the plan destroyed with no synchronise: both outputs are final once the device is idle, and a fresh plan on the
    same buffers gives the same."""
    case = _case(0)
    refs = {}
    for pipelined in (False, True, False):
        plan = case.new_plan()
        plan.set_option("pipeline", int(pipelined))
        for name in ("o0", "o1"):
            case.buf[name].upload(case.fill)
        before = plan.lane_info()
        for i in range(pc.DESTROY_APPLIES):
            plan.apply_device(case.buf[f"f{pc.loop_frame(i)}"].ptr, case.buf[f"o{i & 1}"].ptr, case.geom)
            if not pipelined:
                plan.synchronize()
        info = plan.lane_info()
        lanes = tuple(info[key] - before[key] for key in ("lane0", "lane1", "gated", "joins"))
        plan.close()
        case.native.check(case.native.lib().rpsf_device_synchronize(0))
        got = case.buf["o0"].download(), case.buf["o1"].download()
        if pipelined:
            _report("destroy", lanes, pc.EXPECTED["destroy"])
            assert lanes == pc.EXPECTED["destroy"]
        else:
            assert lanes == (0, 0, 0, 0)
        if refs:
            assert pc.same_bytes(got[0], refs[0]) and pc.same_bytes(got[1], refs[1]), "pipelined" if pipelined else "a fresh plan behind it"
        else:
            refs = dict(enumerate(got))
            assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], case.fill)
