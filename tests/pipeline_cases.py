"""Every operation of a plan around pipelined applies (RPSF_OPT_PIPELINE, csrc/rpsf_lanes.hpp): the cases of tests/test_gpu_pipeline_ops.py, and
what the lane book must have counted for each - replayed without a GPU by tests/test_lanes_host.py.

The sandwich.  `k` pipelined applies into the two outputs in turn (k = 1, 2, 3: the last one on lane 0 with lane 1 idle, on lane 1, on lane 0
with lane 1 busy), the operation, three pipelined applies into the buffer the operation read.  An operation that takes a device input reads
`src`, the buffer the last apply of the prefix writes - without its join it reads a frame half written -, and one that writes a device output
writes `dst`, the other output, which the apply before that one wrote (batches read both outputs as a stack of two and write the stack
output).  One exception: `apply_view_f64` needs a float64 input and reads a static buffer, so a missing join in front of its C1 would race with
nothing on the input side - the lane report and `apply_view_f32_f64`, which reads `src`, stand in for it.  The reference is the same calls on the same plan with the option off and a synchronise behind every call.

Each operation comes with its SCRIPT: what it means to the lane book, as tokens that tests/test_lanes_host.py replays through
tests/emu/emu_lanes.cpp on the model of the two streams -

    ("hot", image, out, layout)     rpsf_apply_device with stream == NULL: pipelined when the book allows it
    ("cold", frames, fused, gated)  any other launch of the plan: joins, then runs on the public stream (fused: it advances the tile counters'
                                    epoch for `frames` frames - another frame count than the last launch's restarts them, and the launch
                                    that restarts them is never pipelined)
    ("join",)                       everything else that joins: installs, options, fills, launches of a view
    ("enable", v) ("expose", v) ("multi",)   RPSF_OPT_PIPELINE, rpsf_plan_stream / the option set again, an apply on a caller's stream
    ("nop",)                        a setter that does not join

- and EXPECTED holds, per sequence, the lane report's deltas (applies begun on lane 0, on lane 1, begun gated, joins that were due).  They
are written once, here; the replay must produce them on the CPU and the plan must report them on the GPU.

COVERAGE names, for every entry point of include/rpsf.h that takes a plan, the case that runs it behind a busy lane 1 or the reason why it
touches no stream; tests/test_lanes_host.py fails when an entry point is missing from it.
"""

import functools

import numpy as np

N = 256
SHAPES = [(1024, 1024), (1280, 1024)]
FRAMES = 4
PREFIXES = (1, 2, 3)
PREFIX_FRAMES = (1, 2, 3)  # apply i of the prefix: frame PREFIX_FRAMES[i] into output i & 1
SUFFIX_FRAMES = (1, 2, 3)  # the three applies behind the operation, all into `src`
DILATION, WIDTH = 1, 7     # saturation and masks: the reference's defaults
MARKED = 40                # pixels a threshold or a mask marks
BALLAST = 16               # frames of the batch a pipelined sequence starts behind (Run.start)


# ---- tokens ---------------------------------------------------------------------------------------------------------------------------------
JOIN, NOP, MULTI = ("join",), ("nop",), ("multi",)


def hot(image, out, layout="whole"):
    return ("hot", image, out, layout)


def cold(frames=1, fused=True, gated=True):
    return ("cold", frames, fused, gated)


def enable(v):
    return ("enable", int(v))


def expose(v):
    return ("expose", int(v))


def other(o):
    return "o1" if o == "o0" else "o0"


# ---- the case of one shape ------------------------------------------------------------------------------------------------------------------
class Slice:
    """Frame `index` of a DeviceBuffer that holds a stack."""

    def __init__(self, buffer, index, shape, dtype=np.float32):
        self.buffer, self.shape, self.dtype = buffer, shape, np.dtype(dtype)
        self.nbytes = int(np.prod(shape)) * self.dtype.itemsize
        self.offset = index * self.nbytes
        self.ptr = buffer.at(self.offset)

    def download(self):
        return self.buffer.download(self.shape, self.dtype, self.offset)

    def upload(self, array):
        self.buffer.upload(np.ascontiguousarray(array, self.dtype), self.offset)


def marking_threshold(frame, marked=MARKED):
    """A threshold that exactly `marked` pixels of the frame exceed (or reach)."""
    return float(np.partition(np.asarray(frame, np.float64).ravel(), -marked)[-marked])


class Case:
    def __init__(self, shape):
        from oracle import regpsf_oracle as orc
        from regularizepsf_amd import _native

        self.native = _native
        h, w = self.shape = shape
        self.pad = _native.PAD_MODES["symmetric"]
        self.coords = [tuple(int(v) for v in t) for t in orc.calculate_covering(shape, N)]
        rng = np.random.default_rng(h * 11 + w)
        n = len(self.coords)
        self.k = [(rng.standard_normal((n, N, N)) + 1j * rng.standard_normal((n, N, N))).astype(np.complex64) for _ in range(2)]
        self.spectra = [(rng.standard_normal((n, N, N)) + 1j * rng.standard_normal((n, N, N))).astype(np.complex64) for _ in range(2)]
        self.frames = [(rng.standard_normal(shape) * 10 + 50 + 20 * f).astype(np.float32) for f in range(FRAMES)]
        self.fill = (0.5 * self.frames[3]).astype(np.float32)  # what both outputs hold when a sequence starts
        self.geom = _native.Geometry.whole(h, w, self.pad)
        self.npix, self.nbytes = h * w, h * w * 4
        self.d_k = [_native.DeviceBuffer(k.nbytes).upload(k) for k in self.k]
        self.d_spectra = [_native.DeviceBuffer(s.nbytes).upload(s) for s in self.spectra]
        self.d_frames = _native.DeviceBuffer(FRAMES * self.nbytes).upload(np.stack(self.frames))
        self.d_outs = _native.DeviceBuffer(2 * self.nbytes)
        self.d_stack_out = _native.DeviceBuffer(3 * self.nbytes)
        self.d_ballast = [_native.DeviceBuffer(BALLAST * self.nbytes) for _ in range(2)]
        self.d_ballast[0].upload(np.stack([self.frames[f % FRAMES] for f in range(BALLAST)]))
        self.d_f64 = _native.DeviceBuffer(2 * self.npix * 8).upload(np.stack([self.frames[0].astype(np.float64), np.zeros(shape)]))
        mask = np.zeros((2, h, w), np.uint8)
        for f in range(2):
            mask[f].ravel()[rng.choice(h * w, MARKED, replace=False)] = 1
        self.masks = mask
        self.d_masks = _native.DeviceBuffer(mask.nbytes).upload(mask)
        self.buf = {f"f{f}": Slice(self.d_frames, f, shape) for f in range(FRAMES)}
        self.buf.update({f"o{o}": Slice(self.d_outs, o, shape) for o in range(2)})
        self.buf.update({f"so{f}": Slice(self.d_stack_out, f, shape) for f in range(3)})
        self.buf["d0"] = Slice(self.d_f64, 0, shape, np.float64)
        self.buf["d1"] = Slice(self.d_f64, 1, shape, np.float64)
        self.plan = self.new_plan()
        self.references, self.thresholds = {}, {}
        self.thr_host = marking_threshold(self.frames[0])

    def new_plan(self):
        plan = self.native.Plan(N, self.coords)
        plan.set_transfer_device(self.d_k[0].ptr)
        return plan

    def view(self, name):
        b = self.buf[name]
        h, w = self.shape
        return self.native.View(b.ptr.value, self.native.DTYPES[b.dtype.str], h, w, w * b.dtype.itemsize, b.dtype.itemsize)

    def mask_view(self, f):
        h, w = self.shape
        return self.native.View(self.d_masks.ptr.value + f * h * w, self.native.DTYPES["|u1"], h, w, w, 1)


@functools.lru_cache(maxsize=None)
def case_for(shape):
    return Case(shape)


# ---- one run of a sequence, pipelined or as the reference ----------------------------------------------------------------------------------
class Run:
    """The calls of one sequence on one plan.  pipelined: as a caller makes them, nothing between them.  Otherwise the reference: the option
    off, a synchronise behind every call, and a trace of what every step wrote (for the non-vacuity check)."""

    def __init__(self, case, pipelined, plan=None):
        self.case, self.pipelined, self.plan = case, pipelined, plan or case.plan
        self.own_plan = plan is not None
        self.host, self.trace, self.watched, self.deferred = [], [], {"o0", "o1"}, []
        self.lanes = None

    def start(self):
        c = self.case
        self.plan.set_option("pipeline", 0)
        self.plan.apply_device(c.buf["f0"].ptr, c.buf["o0"].ptr, c.geom)  # (the last fused launch was of one frame: the tile counters do not restart)
        self.plan.synchronize()
        for name in ("o0", "o1", "so0", "so1", "so2", "d1"):
            c.buf[name].upload(c.fill)
        self.plan.set_option("pipeline", int(self.pipelined))  # (joins: the book starts every sequence with the lanes joined)
        if self.pipelined:
            # Ballast.  Applies of these frames take the device less time than Python takes to enqueue them: without more, every apply of the
            # prefix would be over before the operation is called, and a missing join would race with nothing.  One call that keeps the public
            # stream busy for a few hundred microseconds - a batch of BALLAST frames, then one frame, so that the tile counters count single
            # frames again - lets the host run ahead: the prefix is still queued or in flight when the operation arrives.
            self.plan.apply_batch_device(c.d_ballast[0].ptr, c.d_ballast[1].ptr, BALLAST, c.npix, c.npix, c.geom)
            self.plan.apply_batch_device(c.d_ballast[0].ptr, c.d_ballast[1].ptr, 1, c.npix, c.npix, c.geom)
        self.before = self.plan.lane_info()
        return self

    def set_pipeline(self, value):
        """RPSF_OPT_PIPELINE inside a sequence; the reference stays on one lane."""
        self.call(lambda: self.plan.set_option("pipeline", int(value) if self.pipelined else 0))

    def call(self, fn, writes=(), label=""):
        got = fn()
        arrays = [a for a in (got if isinstance(got, tuple) else (got,)) if isinstance(a, np.ndarray)]
        self.host += arrays
        self.watched.update(writes)
        if not self.pipelined:
            self.plan.synchronize()
            for a in arrays[:1]:
                self.trace.append((label or "host result", a))
            for name in writes:
                self.trace.append((label or name, self.case.buf[name].download()))
        return got

    def apply(self, image, out, stream=None):
        c = self.case
        self.call(lambda: self.plan.apply_device(c.buf[image].ptr, c.buf[out].ptr, c.geom, stream), writes=(out,), label=f"apply {image} -> {out}")

    def defer(self, fn):
        """Put the shared plan back as it was, once the sequence is over."""
        if not self.own_plan:
            self.deferred.append(fn)

    def finish(self):
        c = self.case
        try:
            self.plan.synchronize()
            info = self.plan.lane_info()
            self.lanes = tuple(info[key] - self.before[key] for key in ("lane0", "lane1", "gated", "joins"))
            self.info = info
            self.device = {name: c.buf[name].download() for name in sorted(self.watched)}
            # rpsf_apply_device_loop_ms ends with the check of the plan's error word and fails when a gate wait ran out
            self.plan.apply_device_loop_ms(c.buf["f0"].ptr, c.buf["o0"].ptr, c.geom, 1)
        finally:
            self.restore()
        return self

    def restore(self):
        """The shared plan as it was before the sequence (or the sequence's own plan closed); also the way out of a sequence that failed."""
        self.plan.synchronize()
        deferred, self.deferred = self.deferred, []
        for fn in deferred:
            fn()
        self.plan.synchronize()
        if self.own_plan:
            self.plan.close()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_steps_differ(trace, what):
    """Non-vacuity: equality could not tell a stale buffer from a fresh one if two steps in a row wrote the same thing."""
    for (la, a), (lb, b) in zip(trace, trace[1:]):
        assert a.shape != b.shape or not np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64)), f"{what}: '{la}' and '{lb}' wrote the same"


# ---- the operations --------------------------------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, body, script, entries, fresh=False, both_shapes=False):
        self.name, self.body, self.script, self.entries, self.fresh, self.both_shapes = name, body, script, tuple(entries), fresh, both_shapes


OPS = []


def op(name, script, entries, **kw):
    def wrap(body):
        OPS.append(Op(name, body, script if callable(script) else (lambda src, dst, s=tuple(script): list(s)), entries, **kw))
        return body
    return wrap


def _stack2(r):
    """Both outputs as a stack of two frames, and the first two frames of the stack output."""
    c = r.case
    return c.buf["o0"].ptr, c.buf["so0"].ptr, ("so0", "so1")


@op("set_transfer", [JOIN], ["rpsf_plan_set_transfer"])
def _(r, src, dst):
    r.call(lambda: r.plan.set_transfer(r.case.k[1]))
    r.defer(lambda: r.plan.set_transfer_device(r.case.d_k[0].ptr))


@op("set_transfer_device", [JOIN], ["rpsf_plan_set_transfer_device"], both_shapes=True)
def _(r, src, dst):
    r.call(lambda: r.plan.set_transfer_device(r.case.d_k[1].ptr))
    r.defer(lambda: r.plan.set_transfer_device(r.case.d_k[0].ptr))


@op("set_transfer_spectra_device", [JOIN], ["rpsf_plan_set_transfer_spectra_device"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.set_transfer_spectra_device(c.d_spectra[0].ptr, c.d_spectra[1].ptr, 1.0, 0.1))
    r.defer(lambda: r.plan.set_transfer_device(c.d_k[0].ptr))


@op("set_overlap_mode", lambda src, dst: [JOIN, cold(1, False, False), JOIN, cold(1, False, False), JOIN, hot("f2", dst)], ["rpsf_plan_set_overlap_mode"])
def _(r, src, dst):
    r.call(lambda: r.plan.set_overlap_mode("direct"))
    r.apply(src, dst)
    r.call(lambda: r.plan.set_overlap_mode("atomic"))
    r.apply("f1", dst)
    r.call(lambda: r.plan.set_overlap_mode("auto"))
    r.apply("f2", dst)


@op("set_option_fuse", [JOIN, cold(1, False, False), JOIN], ["rpsf_plan_set_option"])
def _(r, src, dst):
    r.call(lambda: r.plan.set_option("fuse", 0))
    r.apply(src, dst)
    r.call(lambda: r.plan.set_option("fuse", 1))


def _option_01(name, first, last):
    def body(r, src, dst):
        r.call(lambda: r.plan.set_option(name, first))
        r.apply(src, dst)
        r.call(lambda: r.plan.set_option(name, 1 - first))
        r.apply("f0", dst)
        if last != 1 - first:
            r.call(lambda: r.plan.set_option(name, last))
    script = lambda src, dst: [JOIN, hot(src, dst), JOIN, hot("f0", dst)] + ([JOIN] if last != 1 - first else [])  # noqa: E731
    op(f"set_option_{name}", script, ["rpsf_plan_set_option"])(body)


_option_01("k_cached", 1, 0)
_option_01("plane_nt", 1, -1)
_option_01("head_kprefetch", 1, 0)


@op("set_option_pipeline", lambda src, dst: [JOIN, enable(0), hot(src, dst), hot("f0", src), JOIN, enable(1), hot("f2", dst)], ["rpsf_plan_set_option"])
def _(r, src, dst):
    r.set_pipeline(0)
    r.apply(src, dst)
    r.apply("f0", src)
    r.set_pipeline(1)
    r.apply("f2", dst)


@op("apply_batch_device", lambda src, dst: [cold(2), hot("f0", dst), cold(3)], ["rpsf_apply_batch_device"], both_shapes=True)
def _(r, src, dst):
    c, n = r.case, r.case.npix
    ins, outs, names = _stack2(r)
    r.call(lambda: r.plan.apply_batch_device(ins, outs, 2, n, n, c.geom), writes=names, label="batch of 2")
    r.apply("f0", dst)  # (the tile counters restart: one frame behind two)
    r.call(lambda: r.plan.apply_batch_device(c.buf["f1"].ptr, outs, 3, n, n, c.geom), writes=("so0", "so1", "so2"), label="batch of 3")


@op("apply_batch_device_timed", [cold(2), cold(2)], ["rpsf_apply_batch_device_timed"])
def _(r, src, dst):
    c, n = r.case, r.case.npix
    ins, outs, names = _stack2(r)
    r.call(lambda: r.plan.apply_batch_device_timed(ins, outs, 2, n, n, c.geom, 2) and None, writes=names, label="timed batch")


@op("apply_device_timed", [cold(), cold()], ["rpsf_apply_device_timed"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.apply_device_timed(c.buf[src].ptr, c.buf[dst].ptr, c.geom, 2) and None, writes=(dst,), label="timed apply")


@op("apply_device_loop_ms", lambda src, dst: [JOIN] + [hot(src, dst)] * 5 + [JOIN], ["rpsf_apply_device_loop_ms"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.apply_device_loop_ms(c.buf[src].ptr, c.buf[dst].ptr, c.geom, 5) and None, writes=(dst,), label="loop of 5")


@op("apply_device_saturated", [cold()], ["rpsf_apply_device_saturated"], both_shapes=True)
def _(r, src, dst):
    c, (h, w) = r.case, r.case.shape
    got = r.call(lambda: np.array([r.plan.apply_device_saturated(c.buf[src].ptr, c.buf[dst].ptr, h, w, c.pad, r.thr_src, DILATION, WIDTH)]), writes=(dst,))
    assert got[0] >= MARKED


@op("apply_batch_device_saturated", [cold(2)], ["rpsf_apply_batch_device_saturated"])
def _(r, src, dst):
    c, (h, w), n = r.case, r.case.shape, r.case.npix
    ins, outs, names = _stack2(r)
    got = r.call(lambda: r.plan.apply_batch_device_saturated(ins, outs, 2, n, n, h, w, c.pad, r.thr_src, DILATION, WIDTH), writes=names)
    assert got.max() >= MARKED


@op("apply_host_saturated", [cold()], ["rpsf_apply_host_saturated"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.apply_host_saturated(c.frames[0], c.pad, c.thr_host, DILATION, WIDTH))


@op("apply_frames_host_saturated", [cold(), cold()], ["rpsf_apply_frames_host_saturated"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.apply_frames_host_saturated([c.frames[0], c.frames[1]], c.pad, c.thr_host, DILATION, WIDTH))


@op("apply_host_saturated_device", [cold()], ["rpsf_apply_host_saturated_device"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.apply_host_saturated_device(c.frames[0], c.pad, c.thr_host, DILATION, WIDTH))


@op("apply_frames_host_saturated_device", [cold(2)], ["rpsf_apply_frames_host_saturated_device"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.apply_frames_host_saturated_device([c.frames[0], c.frames[1]], c.pad, c.thr_host, DILATION, WIDTH))


@op("saturation_fill_device", [JOIN], ["rpsf_saturation_fill_device"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.saturation_fill_device(c.frames[0], c.pad, c.thr_host, DILATION, WIDTH)[:2])


@op("saturation_fill_batch_device", [JOIN], ["rpsf_saturation_fill_batch_device"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.saturation_fill_batch_device([c.frames[0], c.frames[1]], c.pad, c.thr_host, DILATION, WIDTH)[:2])


@op("saturation_fill_masked_device", [JOIN], ["rpsf_saturation_fill_masked_device"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.saturation_fill_masked_device([c.frames[0]], c.pad, float("inf"), DILATION, WIDTH, c.masks[:1])[:2])


@op("apply_batch_device_masked", [cold(2), cold(2)], ["rpsf_apply_batch_device_masked"])
def _(r, src, dst):
    c, (h, w), n = r.case, r.case.shape, r.case.npix
    ins, outs, names = _stack2(r)
    inf = float("inf")
    one = r.call(lambda: r.plan.apply_batch_device_masked(ins, outs, 2, n, n, h, w, c.pad, inf, DILATION, WIDTH, [c.mask_view(0)], False), writes=names,
                 label="one mask")
    r.call(lambda: r.plan.apply_batch_device_masked(c.buf["f0"].ptr, outs, 2, n, n, h, w, c.pad, inf, DILATION, WIDTH,
                                                    [c.mask_view(0), c.mask_view(1)], False), writes=names, label="a mask per frame")
    assert one.min() >= MARKED


@op("apply_view_masked", [cold()], ["rpsf_apply_view_masked"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.apply_view_masked(c.view(src), c.view(dst), c.pad, float("inf"), DILATION, WIDTH, c.mask_view(0), False) and None, writes=(dst,))


@op("apply_batch_view_masked", [cold(2)], ["rpsf_apply_batch_view_masked"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.apply_batch_view_masked([c.view("o0"), c.view("o1")], [c.view("so0"), c.view("so1")], c.pad, float("inf"), DILATION, WIDTH,
                                                  [c.mask_view(1)], False) and None, writes=("so0", "so1"))


@op("apply_frames_host_masked_device", [cold(2)], ["rpsf_apply_frames_host_masked_device"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.apply_frames_host_masked_device([c.frames[0], c.frames[1]], c.pad, float("inf"), DILATION, WIDTH, [c.masks[0]], False))


@op("apply", [cold()], ["rpsf_apply"], both_shapes=True)
def _(r, src, dst):
    r.call(lambda: r.plan.apply(r.case.frames[0], r.case.pad))


@op("apply_banded", [JOIN, JOIN, JOIN], ["rpsf_apply"])
def _(r, src, dst):
    """Two row bands: views of the plan, plans of their own that run on the parent's stream and join the parent's lanes at every launch."""
    r.call(lambda: r.plan.set_option("host_bands", 2))
    r.call(lambda: r.plan.apply(r.case.frames[0], r.case.pad))
    assert r.plan.host_bands() == 2
    r.call(lambda: r.plan.set_option("host_bands", -1))


@op("apply_host", [cold()], ["rpsf_apply_host"])
def _(r, src, dst):
    r.call(lambda: r.plan.apply_host(r.case.frames[0].astype(np.float64), r.case.pad, out_dtype=np.float64))


@op("apply_batch", [cold(2)], ["rpsf_apply_batch"])
def _(r, src, dst):
    r.call(lambda: r.plan.apply_batch(np.stack(r.case.frames[:2]), r.case.pad))


@op("apply_batch_host", [cold(2)], ["rpsf_apply_batch_host"])
def _(r, src, dst):
    r.call(lambda: r.plan.apply_frames_host(np.stack(r.case.frames[:2]).astype(np.float64), r.case.pad))  # (a contiguous stack: rpsf_apply_batch_host)


@op("apply_frames_host", [cold(2)], ["rpsf_apply_frames_host"])
def _(r, src, dst):
    r.call(lambda: r.plan.apply_frames_host([r.case.frames[0], r.case.frames[1]], r.case.pad, out_dtype=np.float32))


@op("apply_view", [cold()], ["rpsf_apply_view"])
def _(r, src, dst):
    c = r.case
    route = r.call(lambda: np.array([r.plan.apply_view(c.view(src), c.view(dst), c.pad)]), writes=(dst,))
    assert route[0] == 0  # zero copy on both sides


@op("apply_view_f64", [cold()], ["rpsf_apply_view"], both_shapes=True)
def _(r, src, dst):
    c = r.case
    route = r.call(lambda: np.array([r.plan.apply_view(c.view("d0"), c.view("d1"), c.pad)]), writes=("d1",))
    assert route[0] == c.native.ROUTE_C1 | c.native.ROUTE_C2  # C1 and C2 on the public stream around the apply


@op("apply_view_f32_f64", [cold()], ["rpsf_apply_view"])
def _(r, src, dst):
    """float32 in, zero copy, float64 out: the view route that reads what the last apply of the prefix writes (C2 behind the apply)."""
    c = r.case
    route = r.call(lambda: np.array([r.plan.apply_view(c.view(src), c.view("d1"), c.pad)]), writes=("d1",))
    assert route[0] == c.native.ROUTE_C2


@op("apply_batch_view", [cold(2)], ["rpsf_apply_batch_view"])
def _(r, src, dst):
    c = r.case
    r.call(lambda: r.plan.apply_batch_view([c.view("o0"), c.view("o1")], [c.view("so0"), c.view("so1")], c.pad) and None, writes=("so0", "so1"))


@op("stream", lambda src, dst: [JOIN, expose(1), hot("f0", dst), hot("f1", src), JOIN, enable(1), expose(0)], ["rpsf_plan_stream"], fresh=True)
def _(r, src, dst):
    """The handle of the plan's stream: one lane from then on, until the option is set again."""
    c = r.case
    handle = r.call(lambda: r.plan.stream)
    before = r.plan.lane_info()
    r.apply("f0", dst)
    r.apply("f1", src)
    if r.pipelined:
        info = r.plan.lane_info()
        assert info["exposed"] and info["enabled"] and info["lane1"] == before["lane1"] and info["lane0"] == before["lane0"]
    r.call(lambda: c.native.add_rows(c.buf[dst].ptr, c.buf[src].ptr, c.npix, stream=handle), writes=(dst,), label="add_rows on the handle")
    r.plan.synchronize()
    r.set_pipeline(1)
    if r.pipelined:
        assert not r.plan.lane_info()["exposed"]


@op("apply_device_stream", lambda src, dst: [cold(), MULTI, hot("f0", src), hot("f2", dst)], ["rpsf_apply_device"], fresh=True)
def _(r, src, dst):
    """An apply on a caller's stream - the caller synchronises the plan before it and the stream after it -: one lane from then on."""
    c = r.case
    r.plan.synchronize()
    st = c.native.Stream()
    r.apply(src, dst, stream=st.ptr)
    c.native.stream_synchronize(st.ptr)
    r.apply("f0", src)
    r.apply("f2", dst)
    r.plan.synchronize()
    st.close()


@op("set_cu_mask", lambda src, dst: [JOIN, enable(0), hot(src, dst), JOIN, hot("f0", src)], ["rpsf_plan_set_cu_mask"], fresh=True)
def _(r, src, dst):
    """All CUs but eight: lane 1 is given up for good, the option does not bring it back."""
    c = r.case
    cus = c.native.device_info()[0]
    r.call(lambda: r.plan.set_cu_mask(c.native.cu_masks(cus, 8)[0]))
    r.apply(src, dst)
    r.set_pipeline(1)
    r.apply("f0", src)
    if r.pipelined:
        assert not r.plan.lane_info()["enabled"]


@op("setters_without_join", lambda src, dst: [NOP, hot("f0", dst), NOP, hot("f1", src), NOP, hot("f2", dst), NOP, hot("f3", src)],
    ["rpsf_plan_set_image_prefetch", "rpsf_plan_set_reserved_cus", "rpsf_plan_set_stagger"], fresh=True)
def _(r, src, dst):
    """Host fields that the next launch reads: flipped between pipelined applies, they join nothing."""
    r.call(lambda: r.plan.set_image_prefetch(True))
    r.apply("f0", dst)
    r.call(lambda: r.plan.set_reserved_cus(64))
    r.apply("f1", src)
    r.call(lambda: r.plan.set_stagger(0))
    r.apply("f2", dst)
    r.call(lambda: r.plan.set_stagger(5))
    r.apply("f3", src)


OPS_BY_NAME = {o.name: o for o in OPS}


def sandwich_ids():
    return [(si, o.name, k) for o in OPS for si in range(len(SHAPES) if o.both_shapes else 1) for k in PREFIXES]


def sandwich_script(name, k):
    o = OPS_BY_NAME[name]
    src = f"o{(k - 1) & 1}"
    dst = other(src)
    return ([hot(f"f{PREFIX_FRAMES[i]}", f"o{i & 1}") for i in range(k)] + o.script(src, dst) + [hot(f"f{f}", src) for f in SUFFIX_FRAMES])


def run_sandwich(case, name, k, pipelined):
    o = OPS_BY_NAME[name]
    r = Run(case, pipelined, case.new_plan() if o.fresh else None).start()
    src = f"o{(k - 1) & 1}"
    dst = other(src)
    for i in range(k):
        r.apply(f"f{PREFIX_FRAMES[i]}", f"o{i & 1}")
    if not pipelined:  # (the reference knows what `src` holds: the threshold of the saturation cases marks MARKED of its pixels)
        case.thresholds[k] = marking_threshold(r.trace[-1][1])
    r.thr_src = case.thresholds[k]
    try:
        o.body(r, src, dst)
        for f in SUFFIX_FRAMES:
            r.apply(f"f{f}", src)
    except BaseException:
        r.restore()  # (a failed sequence must not leave the shared plan with another K or option: every later case would fail with it)
        raise
    return r.finish()


def reference_sandwich(case, name, k):
    key = (name, k)
    if key not in case.references:
        r = run_sandwich(case, name, k, False)
        assert_steps_differ(r.trace, f"{name}, prefix {k}")
        case.references[key] = r
    return case.references[key]


# ---- other sequences ------------------------------------------------------------------------------------------------------------------------
LOOP = 40
# (k_cached and plane_nt pick between instantiations of the 128-pixel kernels only: PersistentKernel2<256>::fn_k_cached is patch_kernel2_256p
# itself and plane_nt needs N = 128, so for these 256-pixel plans they are no-ops - what those settings, and the applies inside
# set_option_k_cached / set_option_plane_nt, test is the join in rpsf_plan_set_option and that the option leaves the launch alone)
LOOP_SETTINGS = {  # the 40-apply alternating loop under each launch option
    "defaults": lambda p: None,
    "image_prefetch": lambda p: p.set_image_prefetch(True),
    "reserved_cus_64": lambda p: p.set_reserved_cus(64),
    "stagger_0": lambda p: p.set_stagger(0),
    "stagger_5": lambda p: p.set_stagger(5),
    "head_kprefetch_0": lambda p: p.set_option("head_kprefetch", 0),
    "head_kprefetch_1": lambda p: p.set_option("head_kprefetch", 1),
    "plane_nt_1": lambda p: p.set_option("plane_nt", 1),
    "k_cached_0": lambda p: p.set_option("k_cached", 0),
    "k_cached_1": lambda p: p.set_option("k_cached", 1),
}


def loop_frame(i):
    return (3 * i + 1) % FRAMES


def loop_script(count=LOOP):
    return [hot(f"f{loop_frame(i)}", f"o{i & 1}") for i in range(count)]


GROWTH_SCRIPT = ([hot(f"f{i}", "top", "top") for i in range(3)] + [hot(f"f{i + 1}", f"o{i & 1}") for i in range(3)] + [cold(2)] +
                 [hot(f"f{i}", f"o{i & 1}") for i in range(3)])
ROUNDS = 30  # three plans, applies in turn: six plan streams on the four hardware queues of a process
DESTROY_APPLIES = 6


# ---- the sharded step behind pipelined applies (tests/test_gpu_sharding.py, two processes on one GPU) ---------------------------------------
SHARDED_SHAPE, SHARDED_WORLD = (1024, 1024), 2
SHARDED_FORMS = {"sequence": False, "overlap": True, "pipeline": "pipeline"}  # name -> ShardedApply's `overlap`


def _covered(corners, out_row0, out_rows, width):
    """lattice_covers_window (csrc/rpsf_lattice.hpp) for a plan of these patch corners: a launch that has to clear its output first is not pipelined."""
    half = N // 2
    rows, cols = [c[0] for c in corners], [c[1] for c in corners]
    r0, c0 = min(rows), min(cols)
    nti, ntj = (max(rows) - r0) // half + 2, (max(cols) - c0) // half + 2
    return r0 <= out_row0 and r0 + nti * half >= out_row0 + out_rows and c0 <= 0 and c0 + ntj * half >= width


def sharded_script(form, rank, k):
    """k pipelined applies of the band's main plan, then ShardedApply.step() with a host transport (bench.GlooSeam, whose `stream` is None), as
    sharding.py makes its calls: the band's apply with stream == NULL, then the first use of `plan.stream` - for a wait, for K4 or for the
    seam exchange - which joins and leaves the plan on one lane.  The 'pipeline' form masks the plan's CUs when it is built (no second lane
    from then on) and takes the handle in front of its apply."""
    from oracle import regpsf_oracle as orc
    from regularizepsf_amd.sharding import make_band_plans

    h, w = SHARDED_SHAPE
    coords = [tuple(int(v) for v in c) for c in orc.calculate_covering(SHARDED_SHAPE, N)]
    b = make_band_plans(coords, N, h, SHARDED_WORLD)[rank]
    prefix = [hot(f"f{i + 1}", f"o{i & 1}") for i in range(k)]
    if form == "pipeline":
        return [enable(0)] + prefix + [JOIN, expose(1), hot("f0", "top")]
    corners, out_rows = [coords[i] for i in b.patch_index], b.out_rows
    if form == "overlap":  # the main plan's window is the rows the band owns; where the seam patches run once, they are not the main plan's
        out_rows = b.own_rows
        if b.send_rows > 0:
            own_end = b.out_row0 + b.own_rows
            seam = [c for c in corners if c[0] + N > own_end]
            rest = [c for c in corners if c[0] + N <= own_end]
            if rest and min(c[0] for c in seam) >= b.out_row0:
                corners = rest
    step_apply = hot("f0", "top") if _covered(corners, b.out_row0, out_rows, w) else cold()
    return prefix + [step_apply, JOIN, expose(1)]


def sequences():
    """name -> script of every sequence whose lane report is asserted."""
    out = {f"{name}-k{k}": sandwich_script(name, k) for name in OPS_BY_NAME for k in PREFIXES}
    out["loop"] = loop_script()
    out["growth"] = GROWTH_SCRIPT
    out["rounds"] = loop_script(ROUNDS)
    out["destroy"] = loop_script(DESTROY_APPLIES)
    for form in SHARDED_FORMS:
        for rank in range(SHARDED_WORLD):
            for k in PREFIXES:
                out[f"sharded_{form}-r{rank}-k{k}"] = sharded_script(form, rank, k)
    return out


# name -> (applies begun on lane 0, on lane 1, begun with the gate set, joins that were due): what rpsf_lanes.hpp prescribes
EXPECTED = {
    "set_transfer-k1": (3, 1, 2, 0), "set_transfer-k2": (3, 2, 3, 1), "set_transfer-k3": (4, 2, 4, 1),
    "set_transfer_device-k1": (3, 1, 2, 0), "set_transfer_device-k2": (3, 2, 3, 1), "set_transfer_device-k3": (4, 2, 4, 1),
    "set_transfer_spectra_device-k1": (3, 1, 2, 0), "set_transfer_spectra_device-k2": (3, 2, 3, 1), "set_transfer_spectra_device-k3": (4, 2, 4, 1),
    "set_overlap_mode-k1": (3, 2, 3, 0), "set_overlap_mode-k2": (3, 3, 4, 1), "set_overlap_mode-k3": (4, 3, 5, 1),
    "set_option_fuse-k1": (3, 1, 2, 0), "set_option_fuse-k2": (3, 2, 3, 1), "set_option_fuse-k3": (4, 2, 4, 1),
    "set_option_k_cached-k1": (4, 2, 3, 0), "set_option_k_cached-k2": (4, 3, 4, 1), "set_option_k_cached-k3": (5, 3, 5, 1),
    "set_option_plane_nt-k1": (5, 1, 2, 0), "set_option_plane_nt-k2": (5, 2, 3, 1), "set_option_plane_nt-k3": (6, 2, 4, 1),
    "set_option_head_kprefetch-k1": (4, 2, 3, 0), "set_option_head_kprefetch-k2": (4, 3, 4, 1), "set_option_head_kprefetch-k3": (5, 3, 5, 1),
    "set_option_pipeline-k1": (3, 2, 3, 0), "set_option_pipeline-k2": (3, 3, 4, 1), "set_option_pipeline-k3": (4, 3, 5, 1),
    "apply_batch_device-k1": (2, 1, 1, 0), "apply_batch_device-k2": (2, 2, 2, 1), "apply_batch_device-k3": (3, 2, 3, 1),
    "apply_batch_device_timed-k1": (2, 1, 1, 0), "apply_batch_device_timed-k2": (2, 2, 2, 1), "apply_batch_device_timed-k3": (3, 2, 3, 1),
    "apply_device_timed-k1": (3, 1, 2, 0), "apply_device_timed-k2": (3, 2, 3, 1), "apply_device_timed-k3": (4, 2, 4, 1),
    "apply_device_loop_ms-k1": (6, 3, 6, 1), "apply_device_loop_ms-k2": (6, 4, 7, 2), "apply_device_loop_ms-k3": (7, 4, 8, 2),
    "apply_device_saturated-k1": (3, 1, 2, 0), "apply_device_saturated-k2": (3, 2, 3, 1), "apply_device_saturated-k3": (4, 2, 4, 1),
    "apply_batch_device_saturated-k1": (2, 1, 1, 0), "apply_batch_device_saturated-k2": (2, 2, 2, 1), "apply_batch_device_saturated-k3": (3, 2, 3, 1),
    "apply_host_saturated-k1": (3, 1, 2, 0), "apply_host_saturated-k2": (3, 2, 3, 1), "apply_host_saturated-k3": (4, 2, 4, 1),
    "apply_frames_host_saturated-k1": (3, 1, 2, 0), "apply_frames_host_saturated-k2": (3, 2, 3, 1), "apply_frames_host_saturated-k3": (4, 2, 4, 1),
    "apply_host_saturated_device-k1": (3, 1, 2, 0), "apply_host_saturated_device-k2": (3, 2, 3, 1), "apply_host_saturated_device-k3": (4, 2, 4, 1),
    "apply_frames_host_saturated_device-k1": (2, 1, 1, 0), "apply_frames_host_saturated_device-k2": (2, 2, 2, 1), "apply_frames_host_saturated_device-k3": (3, 2, 3, 1),
    "saturation_fill_device-k1": (3, 1, 2, 0), "saturation_fill_device-k2": (3, 2, 3, 1), "saturation_fill_device-k3": (4, 2, 4, 1),
    "saturation_fill_batch_device-k1": (3, 1, 2, 0), "saturation_fill_batch_device-k2": (3, 2, 3, 1), "saturation_fill_batch_device-k3": (4, 2, 4, 1),
    "saturation_fill_masked_device-k1": (3, 1, 2, 0), "saturation_fill_masked_device-k2": (3, 2, 3, 1), "saturation_fill_masked_device-k3": (4, 2, 4, 1),
    "apply_batch_device_masked-k1": (2, 1, 1, 0), "apply_batch_device_masked-k2": (2, 2, 2, 1), "apply_batch_device_masked-k3": (3, 2, 3, 1),
    "apply_view_masked-k1": (3, 1, 2, 0), "apply_view_masked-k2": (3, 2, 3, 1), "apply_view_masked-k3": (4, 2, 4, 1),
    "apply_batch_view_masked-k1": (2, 1, 1, 0), "apply_batch_view_masked-k2": (2, 2, 2, 1), "apply_batch_view_masked-k3": (3, 2, 3, 1),
    "apply_frames_host_masked_device-k1": (2, 1, 1, 0), "apply_frames_host_masked_device-k2": (2, 2, 2, 1), "apply_frames_host_masked_device-k3": (3, 2, 3, 1),
    "apply-k1": (3, 1, 2, 0), "apply-k2": (3, 2, 3, 1), "apply-k3": (4, 2, 4, 1),
    "apply_banded-k1": (3, 1, 2, 0), "apply_banded-k2": (3, 2, 3, 1), "apply_banded-k3": (4, 2, 4, 1),
    "apply_host-k1": (3, 1, 2, 0), "apply_host-k2": (3, 2, 3, 1), "apply_host-k3": (4, 2, 4, 1),
    "apply_batch-k1": (2, 1, 1, 0), "apply_batch-k2": (2, 2, 2, 1), "apply_batch-k3": (3, 2, 3, 1),
    "apply_batch_host-k1": (2, 1, 1, 0), "apply_batch_host-k2": (2, 2, 2, 1), "apply_batch_host-k3": (3, 2, 3, 1),
    "apply_frames_host-k1": (2, 1, 1, 0), "apply_frames_host-k2": (2, 2, 2, 1), "apply_frames_host-k3": (3, 2, 3, 1),
    "apply_view-k1": (3, 1, 2, 0), "apply_view-k2": (3, 2, 3, 1), "apply_view-k3": (4, 2, 4, 1),
    "apply_view_f64-k1": (3, 1, 2, 0), "apply_view_f64-k2": (3, 2, 3, 1), "apply_view_f64-k3": (4, 2, 4, 1),
    "apply_view_f32_f64-k1": (3, 1, 2, 0), "apply_view_f32_f64-k2": (3, 2, 3, 1), "apply_view_f32_f64-k3": (4, 2, 4, 1),
    "apply_batch_view-k1": (2, 1, 1, 0), "apply_batch_view-k2": (2, 2, 2, 1), "apply_batch_view-k3": (3, 2, 3, 1),
    "stream-k1": (3, 1, 2, 0), "stream-k2": (3, 2, 3, 1), "stream-k3": (4, 2, 4, 1),
    "apply_device_stream-k1": (1, 0, 0, 0), "apply_device_stream-k2": (1, 1, 1, 1), "apply_device_stream-k3": (2, 1, 2, 1),
    "set_cu_mask-k1": (1, 0, 0, 0), "set_cu_mask-k2": (1, 1, 1, 1), "set_cu_mask-k3": (2, 1, 2, 1),
    "setters_without_join-k1": (4, 4, 7, 0), "setters_without_join-k2": (5, 4, 8, 0), "setters_without_join-k3": (5, 5, 9, 0),
    "loop": (20, 20, 39, 0),
    "growth": (5, 3, 5, 2),
    "rounds": (15, 15, 29, 0),
    "destroy": (3, 3, 5, 0),
    # the sharded step at world 2: the band's apply continues the alternation, the first use of the plan's stream handle joins (due: lane 1 is busy
    # from one apply of the prefix on, since the step's own apply takes the other lane)
    "sharded_sequence-r0-k1": (1, 1, 1, 1), "sharded_sequence-r0-k2": (2, 1, 2, 1), "sharded_sequence-r0-k3": (2, 2, 3, 1),
    "sharded_sequence-r1-k1": (1, 1, 1, 1), "sharded_sequence-r1-k2": (2, 1, 2, 1), "sharded_sequence-r1-k3": (2, 2, 3, 1),
    "sharded_overlap-r0-k1": (1, 1, 1, 1), "sharded_overlap-r0-k2": (2, 1, 2, 1), "sharded_overlap-r0-k3": (2, 2, 3, 1),
    "sharded_overlap-r1-k1": (1, 1, 1, 1), "sharded_overlap-r1-k2": (2, 1, 2, 1), "sharded_overlap-r1-k3": (2, 2, 3, 1),
    # ... and the form that masks the plan's CUs has one lane from the start
    "sharded_pipeline-r0-k1": (0, 0, 0, 0), "sharded_pipeline-r0-k2": (0, 0, 0, 0), "sharded_pipeline-r0-k3": (0, 0, 0, 0),
    "sharded_pipeline-r1-k1": (0, 0, 0, 0), "sharded_pipeline-r1-k2": (0, 0, 0, 0), "sharded_pipeline-r1-k3": (0, 0, 0, 0),
}


# ---- completeness: every entry point that takes a plan ---------------------------------------------------------------------------------------
def _cases(*names):
    return ("cases", names)


def _no_stream(why):
    return ("no stream", why)


COVERAGE = {name: _cases(*[o.name for o in OPS if name in o.entries]) for o in OPS for name in o.entries}
COVERAGE.update({
    "rpsf_plan_destroy": _cases("destroy"),
    "rpsf_apply_device": _cases("loop", "apply_device_stream"),
    "rpsf_plan_lane_info": _no_stream("reads the host-side counters of the lane book"),
    "rpsf_plan_host_bands": _no_stream("reads a host field"),
    "rpsf_plan_sweep_info": _no_stream("reads host fields"),
    "rpsf_plan_transfer_bytes": _no_stream("reads host fields"),
    "rpsf_saturation_kernel_ms": _no_stream("reads the times of events that the call which recorded them has waited for"),
    "rpsf_saturation_batch_info": _no_stream("reads host fields of the last batch call"),
    "rpsf_plan_set_sweep_regions": _no_stream("refused, in front of any stream call, by every plan without the sweep kernel - and only 256-pixel plans, "
                                              "which have none, own a second lane; it joins all the same"),
    "rpsf_plan_debug_stamps": _no_stream("refused by builds without -DRPSF_STAMPS; where it copies, it waits for the whole device first, both lanes with it"),
})
