"""The fused launch decision (regularizepsf_amd/csrc/rpsf_launch.hpp), replayed on the CPU against a model of the device side.

launch_decide() settles, for every fused apply of a 128- or 256-pixel plan, how many head summing workgroups stand in front of the patches, how
many persistent patch workgroups each of the eight chunk queues gets, the grid, and how many positions the launch draws from every never-reset
queue word; LaneBook::commit adds those counts to the bases of the next launch.  A count that is not what the kernels draw, or a grid whose
first resident workgroups all wait, is a wait that never ends on the device.

The model below is written from the kernels' text (patch_body2, rpsf_kernels2.hpp; sum_tiles_worker, rpsf_kernels.hpp).  A workgroup's role
follows its block index.  Persistent form: blocks below sum_first are head summing workgroups (which compute one patch of chunk blk & 7 first
when head_patches is set, without a draw), the others draw positions of their chunk's queue (blk - sum_first) & 7 until one past the end and
then sum.  Fused form that is not persistent: head summing workgroups, one patch workgroup per slot and frame, tail summing workgroups.  A
summing workgroup holds up to four drawn tile positions, sums whichever of them has all its contributors (the counter EQUALS epoch x
contributors), draws while it holds fewer than four and none is complete, and returns once it has drawn one position past the end and holds
nothing.  Residency is CUs x workgroups per CU places; a workgroup keeps its place until it returns; dispatch is in block order.  Queue words
are 32-bit counters that are never reset.

A plan's patches form a lattice: every patch covers four tiles and every tile is covered by at most four patches, so a plan has at least as
many tiles as patches - the model lays the patches out row by row on a near-square lattice.
"""

import collections
import ctypes
import math
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_lanes_host import Model as LaneModel
from tests.test_lanes_host import check as lane_check
from tests.test_lanes_host import lib as lanes_lib  # noqa: F401  (the fixture that builds the lane emulator)

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "emu" / "emu_launch.cpp"
LIB = ROOT / "tests" / "emu" / "libemu_launch.so"
DEPS = [ROOT / "regularizepsf_amd" / "csrc" / "rpsf_launch.hpp"]
VP = ctypes.c_void_p
U32 = 1 << 32
GEN2, FUSED, PERSISTENT = 1, 2, 3
LOOKAHEAD = 4  # RPSF_SUM_LOOKAHEAD

INPUTS = ["N", "gen2", "wg_threads", "n_patches", "tiles", "frames", "wgs_per_cu", "cu_count", "round_capacity", "reserved_cus", "sum_first",
          "head_patches", "persist", "fused", "hot_geometry", "out_span_ok", "planes_floats", "k_cached", "plane_nt_opt", "frame_major_opt",
          "stagger_us", "prefetch", "k_prefetch"]
OUTPUTS = ["form", "variant", "grid", "chunk", "patch_blocks", "stagger_ticks", "stagger_blocks", "sum_first", "frame_major", "plane_nt", "rows",
           "head_patches", "prefetch", "k_prefetch", "sum_queue_draws"]


def load(path=LIB):
    so = ctypes.CDLL(str(path))
    so.emu_launch_decide.argtypes = [VP, VP]
    so.emu_launch_chunk.argtypes = [ctypes.c_int, ctypes.c_int]
    return so


def build(src=SRC, out=LIB, include=None):
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not pathlib.Path(clang).exists():
        clang = shutil.which("clang++") or shutil.which("hipcc")
    assert clang is not None, "no clang++ to build the emulator"
    subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(out), str(src)] + (include or []), check=True)


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists() or LIB.stat().st_mtime < max([SRC.stat().st_mtime] + [d.stat().st_mtime for d in DEPS]):
        build()
    return load()


# ---- the inputs -------------------------------------------------------------------------------------------------------------------------------
def lattice_of(n_patches):
    """Tiles and, per patch, its four tiles: the patches row by row on a lattice nlj cells wide."""
    nlj = max(1, math.isqrt(n_patches - 1) + 1)
    nli = (n_patches + nlj - 1) // nlj
    ntj = nlj + 1
    quads = [[(c // nlj + (q >> 1)) * ntj + c % nlj + (q & 1) for q in range(4)] for c in range(n_patches)]
    return (nli + 1) * ntj, quads


def launch_input(N, n_patches, frames, cus, wgs_per_cu=None, reserved=0, head_patches=0, persist=True, tiles=None, **more):
    """What rpsf.hip hands to launch_decide for a fused apply on hot geometry of a plan masked to `cus` CUs."""
    wpc = wgs_per_cu if wgs_per_cu is not None else (1 if N == 256 else 4)
    inp = dict(N=N, gen2=1, wg_threads=512 if N == 256 else 128, n_patches=n_patches, tiles=tiles if tiles is not None else lattice_of(n_patches)[0],
               frames=frames, wgs_per_cu=wpc, cu_count=cus, round_capacity=cus * wpc, reserved_cus=reserved, sum_first=-1, head_patches=head_patches,
               persist=int(persist), fused=1, hot_geometry=1, out_span_ok=1, planes_floats=1024 * 1024, k_cached=int(N == 128), plane_nt_opt=-1,
               frame_major_opt=-1, stagger_us=-1, prefetch=0, k_prefetch=0)
    inp.update(more)
    return inp


def decide(lib, inp):
    a = np.asarray([int(inp[k]) for k in INPUTS], np.int64)
    o = np.zeros(24, np.int64)
    lib.emu_launch_decide(a.ctypes.data_as(VP), o.ctypes.data_as(VP))
    d = {k: int(o[i]) for i, k in enumerate(OUTPUTS)}
    d["xq_draws"] = [int(v) for v in o[15:23]]
    d["too_large"] = int(o[23])
    return d


def parent_decide(inp):
    """The decision as the parent commit made it (patch_launch_for and sum_first_for of rpsf.hip, restated line by line): the head summing
    workgroups by the amount of work alone, whatever the plan's CUs hold."""
    N, n, frames, rc = inp["N"], inp["n_patches"], inp["frames"], inp["round_capacity"]
    n256, n128 = bool(inp["gen2"]) and N == 256, bool(inp["gen2"]) and N == 128
    teams = 1 if N * N // 2 // 64 >= 64 else 64 // (N * N // 2 // 64)
    d = dict.fromkeys(OUTPUTS, 0)
    d["xq_draws"] = [0] * 8
    d["chunk"] = ((n + 7) // 8 + teams - 1) // teams * teams
    d["stagger_ticks"] = max(0, inp["stagger_us"]) * 100
    d["grid"] = 8 * (d["chunk"] // teams) * frames
    d["too_large"] = int(d["grid"] > 0x7FFFFFFF)
    d["form"] = GEN2 if inp["gen2"] else 0
    d["stagger_blocks"] = rc if inp["gen2"] else inp["cu_count"] * max(1, 512 // inp["wg_threads"])
    d["patch_blocks"] = d["grid"] if inp["gen2"] else 0
    if not inp["fused"]:
        return d
    count = inp["tiles"] * frames
    fm = n256 and bool(inp["persist"]) and frames > 1 and n >= 1024 and 16.0 * inp["planes_floats"] * frames > 256.0 * 1048576.0
    if inp["frame_major_opt"] >= 0:
        fm = (bool(inp["persist"]) and frames > 1) if inp["frame_major_opt"] == 2 else (fm and inp["frame_major_opt"] != 0)
    d["frame_major"] = int(fm)
    d["plane_nt"] = int(n128 and bool(inp["k_cached"]) and frames > 1 and not fm and 16.0 * inp["planes_floats"] * frames > 300.0 * 1048576.0)
    if inp["plane_nt_opt"] >= 0:
        d["plane_nt"] = int(inp["plane_nt_opt"] != 0 and n128 and bool(inp["k_cached"]))
    work = n * frames
    if inp["sum_first"] >= 0:
        sf = inp["sum_first"]
    elif N == 128:
        sf = 160 if work >= 4096 else 128 if work >= 2048 else 8 if work >= 512 else 0
    else:
        sf = 32 if work >= 2048 else 16 if work >= 1024 else 8 if work >= 512 else 0
    d["sum_first"] = sf
    rows = min(d["chunk"] * frames, max(1, int((rc - sf - inp["reserved_cus"]) / 8)))  # (int(): C++ division rounds towards zero)
    if not (inp["persist"] and rows > 0 and inp["out_span_ok"] and inp["hot_geometry"]):
        d["form"] = FUSED
        nsum = max(8, min(count, rc)) + sf
        d["sum_queue_draws"] = count + nsum
        d["grid"] += nsum
        return d
    d["form"], d["rows"] = PERSISTENT, rows
    d["variant"] = 0 if not inp["k_cached"] else 2 if d["plane_nt"] else 1
    d["head_patches"] = inp["head_patches"]
    d["prefetch"] = int(bool(inp["prefetch"]))
    d["k_prefetch"] = inp["k_prefetch"] if n256 and not d["head_patches"] else 0
    if inp["stagger_us"] < 0 and work >= 256:
        d["stagger_ticks"] = 2400 if work >= 2048 else 1600 if (work >= 1024 and n256) else 1200
        if n128:
            d["stagger_ticks"] = 600 if frames == 1 and n >= 4096 else 0
    for x in range(8):
        slots = min(d["chunk"], max(0, n - x * d["chunk"])) * frames
        d["xq_draws"][x] = max(0, slots - (sf // 8 if d["head_patches"] else 0)) + rows
    d["sum_queue_draws"] = count + sf + 8 * rows
    d["grid"] = sf + 8 * rows
    return d


# ---- the device side --------------------------------------------------------------------------------------------------------------------------
class Plan:
    """What launches of one plan share on the device: the tile counters, the sequence numbers of the gate and the queue words of both lanes."""

    def __init__(self, n_patches, tiles=None, quads=None, frames=32):
        t, q = lattice_of(n_patches)
        self.n, self.tiles, self.quads = n_patches, tiles if tiles is not None else t, quads if quads is not None else q
        assert self.tiles >= t or quads is not None
        self.contrib = [0] * self.tiles
        for qs in self.quads:
            for tile in qs:
                self.contrib[tile] += 1
        self.done = [[0] * self.tiles for _ in range(frames)]
        self.summed = [0] * self.tiles  # sequence number of the last apply that summed the tile
        self.xq = [[0] * 8, [0] * 8]
        self.sumq = [0, 0]

    def restart(self):
        for row in self.done:
            for i in range(len(row)):
                row[i] = 0


class Launch:
    def __init__(self, plan, inp, d, epoch=1, lane=0, xq_base=None, sum_base=None, gate_want=None, seq=0):
        self.plan, self.inp, self.d, self.epoch, self.lane = plan, inp, d, epoch, lane
        self.xq_base = list(xq_base) if xq_base is not None else list(plan.xq[lane])
        self.sum_base = sum_base if sum_base is not None else plan.sumq[lane]
        self.gate_want, self.seq = gate_want, seq  # gate_want: the previous apply may still be in flight, wait for its sum of every tile a patch writes
        self.frames, self.count = inp["frames"], plan.tiles * inp["frames"]
        self.xq_drawn, self.sum_drawn = [0] * 8, 0
        self.computed, self.summed_n = {}, {}

    def entry(self, i):  # sum_entry: (frame, tile) of list position i
        if self.frames <= 1:
            return 0, i
        if self.d["frame_major"]:
            return i // self.plan.tiles, i % self.plan.tiles
        return i % self.frames, i // self.frames

    def slot_of(self, x, pos):  # patch_body2: queue position (or row of the grid) of chunk x -> (slot, frame), None where there is none
        chunk, n, frame, xrow = self.d["chunk"], self.plan.n, 0, pos
        if self.frames > 1:
            if self.d["frame_major"]:
                left = n - x * chunk
                mine = chunk if left >= chunk else max(left, 1)
                frame = xrow // mine
                xrow = xrow % mine if frame < self.frames else chunk
            else:
                frame, xrow = xrow % self.frames, xrow // self.frames
        seq = x * chunk + xrow
        return None if xrow >= chunk or seq >= n else (seq, frame)


class Workgroup:
    __slots__ = ("L", "blk", "state", "x", "pend", "exhausted", "blocked", "todo")

    def __init__(self, L, blk):
        self.L, self.blk, self.pend, self.exhausted, self.blocked, self.todo = L, blk, [], False, False, None
        d = L.d
        pb = blk - d["sum_first"]
        self.x = pb & 7
        if d["form"] == PERSISTENT:
            if blk < d["sum_first"]:
                self.state = "sum"
                if d["head_patches"] > 0:  # the first positions of chunk blk & 7, without a draw
                    self.x, self.todo, self.state = blk & 7, L.slot_of(blk & 7, blk >> 3), "head"
            else:
                self.state = "draw" if pb < d["patch_blocks"] else "sum"
        else:
            if 0 <= pb < d["patch_blocks"]:
                self.todo, self.state = L.slot_of(pb & 7, pb >> 3), "one"
            else:
                self.state = "sum"


def simulate(launches, places, rng=None, max_steps=10_000_000):
    """Runs the launches (dispatched in the order given, each in block order) on `places` residency places.  rng: the next workgroup to take a
    step is drawn at random instead of in turn.  Returns None when everything returned, else a description of the stall."""
    waiters = {}
    runnable = collections.deque() if rng is None else []
    blocks = [(L, b) for L in launches for b in range(L.d["grid"])]
    nxt, resident, steps = 0, 0, 0

    def wake(key):
        for w in waiters.pop(key, ()):
            if w.blocked:
                w.blocked = False
                runnable.append(w)

    def block(w, keys):
        w.blocked = True
        for k in keys:
            waiters.setdefault(k, []).append(w)

    def compute(w, slot):  # -> False: waits at the gate
        L, plan = w.L, w.L.plan
        seq, frame = slot
        if L.gate_want is not None:
            late = [("s", t) for t in plan.quads[seq] if (plan.summed[t] - L.gate_want) % U32 >= (1 << 31)]  # lane_seq_reached
            if late:
                block(w, late)
                return False
        L.computed[slot] = L.computed.get(slot, 0) + 1
        row = plan.done[frame]
        for t in plan.quads[seq]:
            row[t] += 1
            if row[t] == L.epoch * plan.contrib[t]:
                wake(("d", frame, t))
        return True

    def step(w):  # -> "go", "wait" or "end"
        L, plan, d = w.L, w.L.plan, w.L.d
        if w.state == "one":  # a patch workgroup of the form that is not persistent
            if w.todo is not None and not compute(w, w.todo):
                return "wait"
            return "end"
        if w.state == "head":
            if w.todo is not None and not compute(w, w.todo):
                return "wait"
            w.state, w.todo = "sum", None
            return "go"
        if w.state == "draw":
            if w.todo is None:
                word = plan.xq[L.lane]
                pos = (word[w.x] - L.xq_base[w.x]) % U32
                word[w.x] = (word[w.x] + 1) % U32
                L.xq_drawn[w.x] += 1
                if pos > 0x0FFFFFFF:
                    pos = 0x0FFFFFFF
                pos += d["sum_first"] >> 3 if d["head_patches"] else 0
                w.todo = L.slot_of(w.x, pos)
                if w.todo is None:
                    w.state = "sum"
                    return "go"
            if not compute(w, w.todo):
                return "wait"
            w.todo = None
            return "go"
        # sum_tiles_worker, thread 0's loop
        for j, (frame, tile) in enumerate(w.pend):
            if plan.done[frame][tile] == L.epoch * plan.contrib[tile]:
                del w.pend[j]
                L.summed_n[(frame, tile)] = L.summed_n.get((frame, tile), 0) + 1
                if L.seq:
                    plan.summed[tile] = L.seq
                    wake(("s", tile))
                return "go"
        if not w.exhausted and len(w.pend) < LOOKAHEAD:
            i = (plan.sumq[L.lane] - L.sum_base) % U32
            plan.sumq[L.lane] = (plan.sumq[L.lane] + 1) % U32
            L.sum_drawn += 1
            if i >= L.count:
                w.exhausted = True
            else:
                w.pend.append(L.entry(i))
            return "go"
        if not w.pend:
            return "end"
        block(w, [("d", f, t) for f, t in w.pend])
        return "wait"

    while True:
        while resident < places and nxt < len(blocks):
            runnable.append(Workgroup(*blocks[nxt]))
            nxt, resident = nxt + 1, resident + 1
        if not runnable:
            if resident == 0 and nxt == len(blocks):
                return None
            return dict(resident=resident, dispatched=nxt, grid=len(blocks))
        if rng is None:
            w = runnable.popleft()  # in turn
        else:
            j = int(rng.integers(len(runnable)))
            runnable[j], runnable[-1] = runnable[-1], runnable[j]
            w = runnable.pop()
        steps += 1
        assert steps < max_steps, "the model itself does not end"
        r = step(w)
        if r == "go":
            runnable.append(w)
        elif r == "end":
            resident -= 1


def places_of(inp):
    return inp["cu_count"] * inp["wgs_per_cu"]


def check_accounting(L):
    """Every (slot, frame) computed once, every tile position summed once, every counter at epoch x contributors, and the draws the decision says."""
    plan, d = L.plan, L.d
    want = {(s, f) for s in range(plan.n) for f in range(L.frames)}
    assert set(L.computed) == want and all(v == 1 for v in L.computed.values()), "patches computed"
    assert set(L.summed_n) == {(f, t) for f in range(L.frames) for t in range(plan.tiles)} and all(v == 1 for v in L.summed_n.values()), "tiles summed"
    for f in range(L.frames):
        assert plan.done[f] == [L.epoch * c for c in plan.contrib], f"tile counters of frame {f}"
    assert L.xq_drawn == d["xq_draws"], ("slot queue draws", L.xq_drawn, d["xq_draws"])
    assert L.sum_drawn == d["sum_queue_draws"], ("tile queue draws", L.sum_drawn, d["sum_queue_draws"])


_RUNS = {}  # (input, decision) -> the launch and its stall, in block order at the plan's own residency: each is simulated once for all tests


def run_one(inp, d, rng=None, places=None):
    key = (tuple(inp[k] for k in INPUTS), tuple(d[k] for k in OUTPUTS), tuple(d["xq_draws"]))
    if rng is None and places is None:
        if key not in _RUNS:
            _RUNS[key] = run_one(inp, d, places=places_of(inp))
        return _RUNS[key]
    plan = Plan(inp["n_patches"], tiles=inp["tiles"], frames=inp["frames"])
    L = Launch(plan, inp, d)
    stall = simulate([L], places if places is not None else places_of(inp), rng)
    return L, stall


def finishes(lib, inp):
    """The model's verdict on one configuration: the library's decision, and whether it runs to completion (then with its accounts checked)."""
    d = decide(lib, inp)
    L, stall = run_one(inp, d)
    if stall is None:
        check_accounting(L)
    return d, stall is None


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------------
# patch-frames just below and at every sum_first threshold, by patch counts that fill the chunks, leave the last ones short, or leave some empty
LIGHT = [(1, 1), (7, 3), (9, 1), (17, 2), (81, 1), (81, 6), (81, 7), (63, 8), (81, 13), (43, 24), (17, 31), (33, 32), (520, 1), (1030, 1)]
HEAVY = {256: [(81, 26), (2049, 1)], 128: [(143, 4), (143, 15), (143, 29), (513, 4), (129, 32)]}  # (the 128-pixel plan: 2048 and 4096 patch-frames)
BUDGETS = list(range(8, 41)) + [47, 48, 63, 64, 128, 161, 168, 248, 256]
# ... the long launches at the budgets around which their head summing workgroups fill the plan's places (one and four workgroups per CU)
HEAVY_BUDGETS = [8, 9, 16, 17, 31, 32, 33, 34, 35, 36, 39, 40, 41, 42, 43, 64, 168, 256]


def sweep():
    """Every budget of BUDGETS for both plans at their own residency, other residencies, reserved CUs and both head_patches in rotation."""
    k = 0
    for N in (128, 256):
        for cus in sorted(set(BUDGETS) | set(HEAVY_BUDGETS)):
            for n, frames in LIGHT + (HEAVY[N] if cus in HEAVY_BUDGETS else []):
                for persist in (True, False):
                    k += 1
                    wpc = (1 if N == 256 else 4) if k % 3 else 1 + k % 4
                    yield launch_input(N, n, frames, cus, wgs_per_cu=wpc, reserved=(0, 8, 128, 64, 3)[k % 5], head_patches=(k // 2) % 2, persist=persist)


def random_inputs(seed, count, max_work=5000):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        N = (128, 256)[int(rng.integers(2))]
        frames = int(rng.integers(1, 33))
        n = int(rng.integers(1, 41)) if rng.random() < 0.4 else int(rng.integers(1, 3001))
        n = max(1, min(n, max_work // frames))
        cus = int(rng.integers(8, 257)) if rng.random() < 0.5 else int(rng.integers(8, 49))
        inp = launch_input(N, n, frames, cus, wgs_per_cu=int(rng.integers(1, 5)), reserved=int(rng.integers(0, 129)), head_patches=int(rng.integers(2)),
                           persist=bool(rng.random() < 0.7))
        if N == 256 and frames > 1 and rng.random() < 0.3:
            inp["frame_major_opt"] = 2  # frame after frame (the library's own choice needs 1024 patches and planes beyond the Infinity Cache)
        yield inp


def has_room(inp, d):
    """The condition of FORWARD PROGRESS (rpsf_launch.hpp): beside the head summing workgroups the plan's CUs hold one patch workgroup for
    every chunk that holds a patch (persistent form), or any patch workgroup at all."""
    held = -(-inp["n_patches"] // d["chunk"])
    return places_of(inp) - d["sum_first"] >= (held if d["form"] == PERSISTENT else 1)


def test_the_decision_is_the_parents_and_accounted_for_wherever_it_has_room(lib):
    """The whole sweep.  The header decides field for field what rpsf.hip decided before the arithmetic moved (restated above from the
    parent's lines).  Wherever the plan's CUs have room for the patch workgroups beside the head summing ones, the decision runs to completion
    on the model with every patch computed once, every tile summed once and exactly the draws it committed.  Where they have not, it does not
    end: test_the_decision_stalls_under_tight_masks."""
    checked = 0
    forms, heads = set(), set()
    for inp in list(sweep()) + list(random_inputs(11, 400)):
        d = decide(lib, inp)
        assert not d["too_large"]
        assert d == parent_decide(inp), inp
        L, stall = run_one(inp, d)
        assert (stall is None) == has_room(inp, d), (inp, d, stall)
        if stall is None:
            check_accounting(L)
            checked += 1
            forms.add((inp["N"], d["form"], d["frame_major"]))
            heads.add((d["sum_first"], d["head_patches"]))
    assert checked > 2000
    assert forms >= {(128, FUSED, 0), (128, PERSISTENT, 0), (256, FUSED, 0), (256, PERSISTENT, 0), (256, PERSISTENT, 1)}
    assert {s for s, _ in heads} >= {0, 8, 16, 32, 128, 160} and {h for _, h in heads} == {0, 1}


def test_the_whole_chip_and_the_sharded_step_finish(lib):
    """256 and 248 CUs (the benchmark, the sharded step): room for every amount of work, reserved CUs and form."""
    for cus in (248, 256):
        for N in (128, 256):
            for n, frames in LIGHT + HEAVY[N] + [(4225, 1), (1089, 8), (289, 1), (16641, 1)]:
                for reserved in (0, 8, 64, 128):
                    for head in (0, 1):
                        for persist in (True, False):
                            inp = launch_input(N, n, frames, cus, reserved=reserved, head_patches=head, persist=persist)
                            d = decide(lib, inp)
                            assert d == parent_decide(inp) and has_room(inp, d), inp


@pytest.mark.parametrize("seed", range(6))
def test_accounting_does_not_depend_on_the_order_of_execution(lib, seed):
    """The whole grid resident, the next workgroup to move drawn at random: the same patches, tiles, counters and draw counts."""
    rng = np.random.default_rng(100 + seed)
    for inp in random_inputs(200 + seed, 40, max_work=3000):
        d = decide(lib, inp)
        L, stall = run_one(inp, d, rng=rng, places=d["grid"])
        assert stall is None, (inp, d, stall)
        check_accounting(L)


def test_the_decision_stalls_under_tight_masks(lib):
    """THE FINDING.  rpsf_plan_set_cu_mask admits any mask of 8 CUs or more, and the head summing workgroups follow the amount of work alone.
    Wherever they leave the plan's CUs no room for a patch workgroup of every chunk that holds a patch, the first resident workgroups all
    wait for tiles whose patches are never dispatched: the model stops with every place held by a workgroup that waits.  Recorded here: the
    stalls of the sweep are exactly that region; a 256-pixel plan with a batch of seven 1024^2 frames stalls on 8 ... 15 CUs, a 128-pixel
    plan with 29 frames of 640 x 768 on 8 ... 41; 248 and 256 CUs never stall.  (A cap on sum_first that makes every budget finish on THIS
    model did not finish on an MI355X, where a workgroup takes a place on its own XCD only - rpsf_launch.hpp, FORWARD PROGRESS; the decision
    is therefore unchanged and the limit is documented in include/rpsf.h.)"""
    stalls, live = [], 0
    for inp in sweep():
        d = decide(lib, inp)
        _, stall = run_one(inp, d)
        assert (stall is None) == has_room(inp, d), (inp, d, stall)
        if stall is None:
            live += 1
        else:
            assert stall["resident"] == places_of(inp) and stall["dispatched"] < stall["grid"]  # every place held by a workgroup that waits
            stalls.append((inp["N"], inp["cu_count"], inp["wgs_per_cu"], inp["n_patches"], inp["frames"], d["form"], d["sum_first"]))
    assert live > 1000 and len(stalls) > 200
    assert max(c * w for _, c, w, *_ in stalls) < 168 and all(s[6] >= 8 for s in stalls)
    assert not [s for s in stalls if s[1] >= 168]
    # the 256-pixel plan on 1024^2 (81 patches), seven frames = 567 patch-frames -> 8 head summing workgroups, one workgroup per CU
    for cus in range(8, 33):
        for persist in (True, False):
            inp = launch_input(256, 81, 7, cus, persist=persist)
            d, ok = finishes(lib, inp)
            assert d["sum_first"] == 8
            assert ok == (cus >= 8 + (8 if persist else 1)), (cus, persist)
    # the 128-pixel plan (four workgroups per CU): 160 head summing workgroups fill 40 CUs
    for cus, stalled in ((8, True), (32, True), (40, True), (41, True), (42, False), (64, False)):
        assert finishes(lib, launch_input(128, 143, 29, cus))[1] == (not stalled), cus


# ---- launches one after another, and two in flight --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_the_lane_book_follows_the_models_queue_words(lib, lanes_lib, seed):
    """Random sequences of launches of one plan - frames, form, lane, head_patches and budget vary, and the queue words start just below 2^32 -
    with the lane book of test_lanes_host.py fed the draws the DECISION commits: every launch finds its bases at the model's counters, runs to
    completion, and leaves the counters where the book says the next launch starts."""
    rng = np.random.default_rng(300 + seed)
    N = 256 if seed % 2 == 0 else 128
    n = int(rng.integers(20, 90))
    plan = Plan(n, frames=8)
    m = LaneModel(lanes_lib)
    bufs = [(i * 1000, i * 1000 + 900) for i in range(4)]
    for lane in (0, 1):  # wrap-around: the never-reset words have run for a long time (two pipelined applies, one per lane, that drew that much)
        start = [int(U32 - rng.integers(1, 300)) for _ in range(9)]
        assert m.apply(True, True, 1, bufs[0], bufs[1], start)["lane"] == lane
        plan.xq[lane], plan.sumq[lane] = start[:8], start[8]
    plan.done[0], plan.summed = [2 * c for c in plan.contrib], [2] * plan.tiles
    wrapped = False
    for k in range(60):
        r = rng.random()
        frames = 1 if r < 0.7 else int(rng.integers(2, 9))
        persist = rng.random() < 0.8
        fused = rng.random() < 0.95
        inp = launch_input(N, n, frames, int(rng.integers(16, 257)), reserved=int(rng.integers(0, 129)), head_patches=int(rng.integers(2)), persist=persist,
                           tiles=plan.tiles, fused=int(fused))
        if frames > 1 and N == 256 and rng.random() < 0.5:
            inp["frame_major_opt"] = 2
        d = decide(lib, inp)
        gated = fused and d["form"] == PERSISTENT and N == 256
        i, o = rng.choice(len(bufs), 2, replace=False)
        a = m.apply(gated and frames == 1, gated, frames, bufs[i], bufs[o], d["xq_draws"] + [d["sum_queue_draws"]], fused=fused)
        assert a["base"][:8] == plan.xq[a["lane"]] and a["base"][8] == plan.sumq[a["lane"]], f"launch {k}: the bases are not where the queue words stand"
        if not fused:
            assert d["form"] == GEN2 and d["xq_draws"] == [0] * 8 and d["sum_queue_draws"] == 0
            continue
        if a["restart"]:
            plan.restart()
        # (one launch at a time here: the previous one has ended, so the gate finds every tile published)
        L = Launch(plan, inp, d, epoch=a["epoch"], lane=a["lane"], xq_base=a["base"][:8], sum_base=a["base"][8],
                   gate_want=a["want"] if a["gate"] else None, seq=a["seq"] if gated else 0)
        assert simulate([L], places_of(inp)) is None, (k, inp, d)
        check_accounting(L)
        wrapped = wrapped or any((b + dr) >= U32 for b, dr in zip(a["base"], a["draws"]))
    lane_check(m)
    assert wrapped and (N == 128 or sum(1 for a in m.applies if a["lane"] == 1) > 2)


@pytest.mark.parametrize("cus", [8, 9, 16, 40, 248, 256])
@pytest.mark.parametrize("n", [81, 520, 1100, 2100])
def test_two_gated_launches_in_flight_finish(lib, cus, n):
    """Two applies of a 256-pixel plan in flight at once (rpsf_lanes.hpp): the second one's patches wait for the first one's sum of every tile
    they write.  Dispatched one behind the other, with the second taking the places the first leaves, both run to completion, the counters end at
    two epochs and each lane's word at its own launch's draws."""
    for head in (0, 1):
        inp = launch_input(256, n, 1, cus, head_patches=head)
        d = decide(lib, inp)
        plan = Plan(n, frames=1)
        a = Launch(plan, inp, d, epoch=1, lane=0, seq=1)
        b = Launch(plan, inp, d, epoch=2, lane=1, gate_want=1, seq=2)
        if not has_room(inp, d):  # (test_the_decision_stalls_under_tight_masks)
            assert simulate([a, b], places_of(inp)) is not None
            continue
        assert simulate([a, b], places_of(inp)) is None
        assert plan.done[0] == [2 * c for c in plan.contrib] and plan.summed == [2] * plan.tiles
        for L in (a, b):
            assert L.xq_drawn == d["xq_draws"] and L.sum_drawn == d["sum_queue_draws"]
            assert all(v == 1 for v in L.computed.values()) and len(L.computed) == n and len(L.summed_n) == plan.tiles
        assert plan.xq[0] == d["xq_draws"] and plan.xq[1] == d["xq_draws"] and plan.sumq == [d["sum_queue_draws"]] * 2


def test_two_gated_launches_in_any_order_of_execution(lib):
    """... and with both grids resident and the next workgroup to move drawn at random."""
    rng = np.random.default_rng(5)
    for n in (9, 81, 300):
        for head in (0, 1):
            inp = launch_input(256, n, 1, 256, head_patches=head)
            d = decide(lib, inp)
            plan = Plan(n, frames=1)
            a = Launch(plan, inp, d, epoch=1, lane=0, seq=1)
            b = Launch(plan, inp, d, epoch=2, lane=1, gate_want=1, seq=2)
            assert simulate([a, b], 2 * d["grid"], rng) is None
            assert plan.done[0] == [2 * c for c in plan.contrib]
            for L in (a, b):
                assert L.xq_drawn == d["xq_draws"] and L.sum_drawn == d["sum_queue_draws"] and len(L.computed) == n and len(L.summed_n) == plan.tiles


def test_a_launch_of_more_than_2_31_workgroups_is_refused(lib):
    assert decide(lib, launch_input(256, 1 << 24, 255, 256, tiles=1))["too_large"] == 1
    assert decide(lib, launch_input(256, 1 << 20, 255, 256, tiles=1))["too_large"] == 0
    assert lib.emu_launch_chunk(256, 81) == 11 and lib.emu_launch_chunk(128, 143) == 18 and lib.emu_launch_chunk(32, 1089) == 144
