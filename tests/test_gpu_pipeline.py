"""Back-to-back applies of one 256-pixel plan overlap head under tail (RPSF_OPT_PIPELINE, csrc/rpsf_lanes.hpp): same bytes as one lane.

The shapes are the smallest that still run the fused persistent 256-pixel kernel with rim patches, interior patches and fewer patches than
workgroups - a 1024 x 1024 frame (9 x 9 patches) - and a 1280 x 1024 one, whose lattice is not square.  Every reference is the same plan with
the option off and a synchronise behind every apply; the references of a shape are computed once.  None of the tests provokes a gate wait that
runs out: that branch is covered by reading it and by tests/test_lanes_host.py.
"""

import time

import numpy as np
import pytest

from oracle import regpsf_oracle as orc

pytestmark = pytest.mark.gpu

N = 256
SHAPES = [(1024, 1024), (1280, 1024)]
FRAMES = 4


class Case:
    def __init__(self, shape):
        from regularizepsf_amd import _native

        self.native = _native
        h, w = self.shape = shape
        self.coords = [tuple(int(v) for v in t) for t in orc.calculate_covering(shape, N)]
        rng = np.random.default_rng(h * 7 + w)
        n = len(self.coords)
        self.k = [(rng.standard_normal((n, N, N)) + 1j * rng.standard_normal((n, N, N))).astype(np.complex64) for _ in range(2)]
        self.frames = [(rng.standard_normal(shape) * 10 + 50 + 20 * f).astype(np.float32) for f in range(FRAMES)]
        self.geom = _native.Geometry.whole(h, w, _native.PAD_MODES["symmetric"])
        self.plan = _native.Plan(N, self.coords)
        self.plan.set_transfer(self.k[0])
        self.d_img = [_native.DeviceBuffer(f.nbytes).upload(f) for f in self.frames]
        self.d_out = [_native.DeviceBuffer(self.frames[0].nbytes) for _ in range(2)]
        stack = np.stack(self.frames[:3])
        self.d_stack = _native.DeviceBuffer(stack.nbytes).upload(stack)
        self.d_stack_out = _native.DeviceBuffer(stack.nbytes)
        # one lane, a synchronise behind every apply: per K and frame, and the batch of the first three frames
        self.plan.set_option("pipeline", 0)
        self.ref = {}
        for ki in (1, 0):
            self.plan.set_transfer(self.k[ki])
            for f in range(FRAMES):
                self.ref[ki, f] = self.one(f, 0)
        self.ref_batch = self.batch()
        self.plan.set_option("persist", 0)
        self.ref_plain = self.one(1, 0)  # one patch per workgroup: the same bits (tests/test_gpu_parity.py), kept to say so here
        self.plan.set_option("persist", 1)
        self.plan.set_option("pipeline", 1)

    def one(self, f, o):
        self.plan.apply_device(self.d_img[f].ptr, self.d_out[o].ptr, self.geom)
        self.plan.synchronize()
        return self.d_out[o].download(self.shape)

    def batch(self):
        h, w = self.shape
        self.plan.apply_batch_device(self.d_stack.ptr, self.d_stack_out.ptr, 3, h * w, h * w, self.geom)
        self.plan.synchronize()
        return self.d_stack_out.download((3, h, w))

    def apply(self, f, o):
        self.plan.apply_device(self.d_img[f].ptr, self.d_out[o].ptr, self.geom)

    def out(self, o):
        return self.d_out[o].download(self.shape)

    def error_word_clear(self):
        """rpsf_apply_device_loop_ms ends with the check of the plan's error word and fails when a gate wait ran out."""
        self.plan.apply_device_loop_ms(self.d_img[0].ptr, self.d_out[0].ptr, self.geom, 1)


_cases = {}


@pytest.fixture(params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    c = _cases[request.param]
    c.plan.synchronize()
    return c


def test_references_are_the_plain_kernels_bits(case):
    assert np.array_equal(case.ref_plain, case.ref[0, 1])
    assert not np.array_equal(case.ref[0, 1], case.ref[1, 1]) and not np.array_equal(case.ref[0, 1], case.ref[0, 2])


def test_forty_applies_of_different_frames_into_one_output(case):
    for i in range(40):
        case.apply(i % FRAMES, 0)
    case.plan.synchronize()
    assert np.array_equal(case.out(0), case.ref[0, 39 % FRAMES])
    case.error_word_clear()


def test_forty_applies_into_two_alternating_outputs(case):
    for i in range(40):
        case.apply((3 * i + 1) % FRAMES, i & 1)
    case.plan.synchronize()
    assert np.array_equal(case.out(0), case.ref[0, (3 * 38 + 1) % FRAMES])
    assert np.array_equal(case.out(1), case.ref[0, (3 * 39 + 1) % FRAMES])
    case.error_word_clear()


def test_set_transfer_between_applies(case):
    case.apply(0, 0)
    case.apply(1, 0)
    case.apply(2, 1)
    case.plan.set_transfer(case.k[1])  # (joins the lanes and waits: both outputs are final)
    got = case.out(0), case.out(1)
    case.apply(2, 0)
    case.apply(3, 1)
    case.plan.synchronize()
    new = case.out(0), case.out(1)
    case.plan.set_transfer(case.k[0])
    assert np.array_equal(got[0], case.ref[0, 1]) and np.array_equal(got[1], case.ref[0, 2])
    assert np.array_equal(new[0], case.ref[1, 2]) and np.array_equal(new[1], case.ref[1, 3])


def test_batch_between_applies(case):
    case.apply(3, 0)
    case.apply(0, 1)
    h, w = case.shape
    case.plan.apply_batch_device(case.d_stack.ptr, case.d_stack_out.ptr, 3, h * w, h * w, case.geom)
    case.apply(1, 0)
    case.apply(2, 1)
    case.plan.synchronize()
    assert np.array_equal(case.d_stack_out.download((3, h, w)), case.ref_batch)
    assert np.array_equal(case.out(0), case.ref[0, 1]) and np.array_equal(case.out(1), case.ref[0, 2])
    case.error_word_clear()


def test_hot_apply_after_one_patch_per_workgroup(case):
    """The launch that is not persistent writes no sequence numbers; it joins the lanes, and the persistent apply behind it does not wait."""
    case.apply(0, 0)
    case.apply(1, 1)
    case.plan.set_option("persist", 0)
    case.apply(2, 0)
    case.plan.set_option("persist", 1)
    case.apply(3, 1)
    case.apply(0, 1)
    case.apply(3, 1)
    case.plan.synchronize()
    assert np.array_equal(case.out(0), case.ref[0, 2]) and np.array_equal(case.out(1), case.ref[0, 3])
    case.error_word_clear()


def test_output_of_one_apply_as_input_of_the_next(case):
    """The caller's own buffers order applies too: an apply that reads what the previous one writes runs behind it."""
    native = case.native
    d_mid = native.DeviceBuffer(case.frames[0].nbytes)
    case.plan.apply_device(case.d_img[1].ptr, d_mid.ptr, case.geom)
    case.plan.apply_device(d_mid.ptr, case.d_out[0].ptr, case.geom)
    case.plan.synchronize()
    chained = case.out(0)
    case.plan.set_option("pipeline", 0)
    case.plan.apply_device(case.d_img[1].ptr, d_mid.ptr, case.geom)
    case.plan.synchronize()
    case.plan.apply_device(d_mid.ptr, case.d_out[0].ptr, case.geom)
    case.plan.synchronize()
    case.plan.set_option("pipeline", 1)
    assert np.array_equal(chained, case.out(0))
    d_mid.free()


def test_alternating_geometries(case):
    """Where the planes of a tile lie depends on the geometry (line length, first output row, origin), so applies of one plan with different
    geometries - the whole frame and its two row windows here, all three fused, persistent and covered by the lattice - do not overlap; applies
    of one geometry in a row still do.  Same bytes as one lane."""
    native = case.native
    h, w = case.shape
    pad = native.PAD_MODES["symmetric"]
    half = h // 2
    geoms = {"whole": case.geom, "top": native.Geometry(h, w, pad, 0.0, 0, 0, 0, h, w, 0, half, w),
             "bottom": native.Geometry(h, w, pad, 0.0, 0, 0, 0, h, w, half, h - half, w)}
    outs = {"whole": case.d_out[0], "top": native.DeviceBuffer(half * w * 4), "bottom": native.DeviceBuffer((h - half) * w * 4)}
    shapes = {"whole": (h, w), "top": (half, w), "bottom": (h - half, w)}
    order = ["whole", "top", "bottom", "whole", "whole", "bottom", "bottom", "top", "whole", "top", "top", "bottom", "whole", "bottom", "top"]
    results = {}
    for mode in (0, 1):
        case.plan.set_option("pipeline", mode)
        last = {}
        for i, name in enumerate(order):
            case.plan.apply_device(case.d_img[i % FRAMES].ptr, outs[name].ptr, geoms[name])
            last[name] = i % FRAMES
            if mode == 0:
                case.plan.synchronize()
        case.plan.synchronize()
        results[mode] = {name: outs[name].download(shapes[name]) for name in outs}
    for name in outs:
        assert np.array_equal(results[0][name], results[1][name]), name
    assert np.array_equal(results[1]["whole"], case.ref[0, last["whole"]])
    case.error_word_clear()
    outs["top"].free()
    outs["bottom"].free()


def test_banded_host_apply_straight_after_pipelined_applies(case):
    """The row bands a host frame is cut into are views of the plan: plans of their own over a subset of the patches that run on the parent's
    stream.  A host-array apply straight behind pipelined applies of the parent joins the parent's lanes first - through the entry point and
    through every band's launch - and returns the bytes of one lane; what the pipelined applies wrote is final when it returns."""
    pad = case.native.PAD_MODES["symmetric"]
    case.plan.set_option("host_bands", 2)
    host = {}
    for mode in (0, 1):
        case.plan.set_option("pipeline", mode)
        for i in (0, 1, 3):
            case.apply(i, i & 1)
            if mode == 0:
                case.plan.synchronize()
        host[mode] = case.plan.apply(case.frames[2], pad)
        assert case.plan.host_bands() == 2
        got = case.out(0), case.out(1)  # (the host call has drained the plan's stream, and with it both lanes)
        assert np.array_equal(got[0], case.ref[0, 0]) and np.array_equal(got[1], case.ref[0, 3])
    case.plan.set_option("host_bands", -1)
    assert np.array_equal(host[0], host[1])
    case.error_word_clear()


def test_two_hundred_applies_finish_in_time(case):
    """A gate wait that ran out would take 0.4 s and set the plan's error word; the loop may take a few times what one lane takes for it (the
    bound leaves room for the host: the applies are enqueued from Python)."""
    times = {}
    for mode in (0, 1, 0, 1):
        case.plan.set_option("pipeline", mode)
        case.plan.synchronize()
        t0 = time.perf_counter()
        for i in range(200):
            case.apply(i % FRAMES, i & 1)
        case.plan.synchronize()
        times[mode] = min(times.get(mode, 1e9), time.perf_counter() - t0)
    print(f"200 applies of {case.shape}: one lane {1e3 * times[0]:.2f} ms, two lanes {1e3 * times[1]:.2f} ms")
    assert times[1] < 3 * times[0] + 0.02
    assert np.array_equal(case.out(1), case.ref[0, 199 % FRAMES]) and np.array_equal(case.out(0), case.ref[0, 198 % FRAMES])
    case.error_word_clear()


def test_device_array_apply_and_download_straight_after_pipelined_applies():
    """An apply through device-array views joins the lanes - it runs behind both pipelined applies - and the download of its result needs no
    synchronise of the caller's; what the pipelined applies wrote is final by then.  The ordering here is the device-array route's own: it waits
    for the plan's stream before it returns.  A bare rpsf_apply_device followed by DeviceBuffer.download with nothing in between is NOT
    covered by any contract, with or without the pipeline: that download is a hipMemcpy on the null stream, which does not wait for the plan's
    non-blocking streams - synchronise first, as every test in this file does."""
    import regularizepsf_amd as rp

    shape = SHAPES[0]
    c = _cases.get(shape) or _cases.setdefault(shape, Case(shape))
    t = rp.ArrayPSFTransform(rp.IndexedCube(c.coords, c.k[0]))
    image = rp.to_device(c.frames[2])
    results = {}
    for mode in (1, 0):  # (two lanes first: the device-array apply hands the plan's stream to Python, and the plan keeps to one lane from then on)
        plan = t._device_plan()
        plan.set_option("pipeline", mode)
        d_out = [c.native.DeviceBuffer(c.frames[0].nbytes) for _ in range(2)]
        for i in range(6):
            plan.apply_device(c.d_img[i % FRAMES].ptr, d_out[i & 1].ptr, c.geom)
            if mode == 0:
                plan.synchronize()
        viewed = t.apply(image).to_host()
        results[mode] = (viewed, d_out[0].download(shape), d_out[1].download(shape))
        for d in d_out:
            d.free()
    for a, b in zip(results[0], results[1]):
        assert np.array_equal(a, b)
    assert np.array_equal(results[1][1], c.ref[0, 0]) and np.array_equal(results[1][2], c.ref[0, 1])
    assert np.array_equal(results[1][0], c.ref[0, 2])
