"""The launch lanes of a plan (regularizepsf_amd/csrc/rpsf_lanes.hpp), checked on the CPU.

Back-to-back persistent applies of a 256-pixel plan alternate between two streams; the header decides the lane of every apply, where the lanes
join, which queue positions each launch owns, its epoch and the sequence number its tile sums publish.  A wrong base or epoch is a wait that
never ends on the device, so the decisions are replayed here on a model of the two streams - an apply is "ordered behind" another when the
stream operations the library would issue (launch, join = record + wait, fork event) put it there - over random sequences of operations.
"""

import ctypes
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from tests import pipeline_cases as pc
from tests.lattice_cases import lattice, thinned
from tests.test_lattice_host import _build as lattice_build
from tests.test_lattice_host import lib as lattice_lib  # noqa: F401  (the fixture that builds the lattice emulator)

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "emu" / "emu_lanes.cpp"
LIB = ROOT / "tests" / "emu" / "libemu_lanes.so"
DEPS = [ROOT / "regularizepsf_amd" / "csrc" / "rpsf_lanes.hpp"]
VP = ctypes.c_void_p
U32 = 1 << 32
# width, out_row0, out_rows, origin_row, origin_col, plane stride: a whole frame, its two row windows, a shifted origin, grown planes
WHOLE = (4096, 0, 4096, 0, 0, 4096 * 4096)
LAYOUTS = [WHOLE, (4096, 0, 2048, 0, 0, 4096 * 4096), (4096, 2048, 2048, 0, 0, 4096 * 4096), (4096, 0, 4096, 128, 0, 4096 * 4096),
           (4096, 0, 4096, 0, 128, 4096 * 4096), (2048, 0, 4096, 0, 0, 4096 * 4096), (4096, 0, 4096, 0, 0, 2 * 4096 * 4096)]


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists() or LIB.stat().st_mtime < max([SRC.stat().st_mtime] + [d.stat().st_mtime for d in DEPS]):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
        if not pathlib.Path(clang).exists():
            clang = shutil.which("clang++") or shutil.which("hipcc")
        assert clang is not None, "no clang++ to build the emulator"
        subprocess.run([clang, "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(LIB), str(SRC)], check=True)
    so = ctypes.CDLL(str(LIB))
    so.emu_lanes_reset.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
    so.emu_lanes_begin.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_uint64] * 4 + [VP, VP]
    so.emu_lanes_commit.argtypes = [ctypes.c_int, VP, ctypes.c_uint32]
    so.emu_lanes_seq_reached.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    so.emu_lanes_next_epoch.argtypes = [ctypes.c_int, VP]
    so.emu_lanes_info.argtypes = [VP]
    so.emu_lanes_set_exposed.argtypes = [ctypes.c_int]
    return so


class Model:
    """The two streams as the library drives them.  A stream's clock is the set of applies everything enqueued on it next runs behind."""

    def __init__(self, lib, enabled=True, seq=0, done_epoch=0):
        self.lib = lib
        lib.emu_lanes_reset(int(enabled), seq, done_epoch)
        self.clock = [set(), set()]      # public stream, second lane
        self.fork = set()                # what the fork event stands for
        self.applies = []                # dicts: lane, pred, hot, gate, seq, want, epoch, restart, gated, img, out, xq (base, draws), sum (base, draws)
        self.lane_end = [[0] * 9, [0] * 9]  # where each lane's queue counters stand (8 XCD queues + the sum queue)
        self.first = True

    def join(self):
        """Everything that is not a pipelined apply: rpsf_detail_join_lanes."""
        if self.lib.emu_lanes_join():
            self.clock[0] |= self.clock[1]
        return set(self.clock[0])

    def other(self):
        """set_transfer, an option, a batch, a synchronise ... : joins, then works on the public stream.  Returns what it runs behind."""
        return self.join()

    def apply(self, hot, gated, frames, img, out, draws, layout=WHOLE, fused=True):
        """fused=False: a launch whose plane sum is a kernel of its own (or that has none): no tile counters, no epoch - and never the gated kernel."""
        assert fused or not (hot or gated)
        restart = fused and bool(self.lib.emu_lanes_epoch_restarts(frames))
        hot = hot and gated and frames == 1 and not restart  # (rpsf.hip, launch_apply: such a launch is never pipelined)
        k = np.zeros(16, np.int64)
        lay = np.asarray(layout, np.int64)
        self.lib.emu_lanes_begin(int(hot), int(gated), img[0], img[1], out[0], out[1], lay.ctypes.data_as(VP), k.ctypes.data_as(VP))
        lane, join, fork, wait_fork, gate, seq, want = (int(v) for v in k[:7])
        if join:
            self.clock[0] |= self.clock[1]
        if fork:
            self.fork = set(self.clock[0])
        if wait_fork:
            self.clock[1] |= self.fork
        e = np.zeros(2, np.int64)
        if fused:
            self.lib.emu_lanes_next_epoch(frames, e.ctypes.data_as(VP))
        xq = np.asarray(draws[:8], np.uint32)
        self.lib.emu_lanes_commit(lane, xq.ctypes.data_as(VP), int(draws[8]))
        me = len(self.applies)
        a = dict(lane=lane, pred=set(self.clock[lane]), hot=hot, gate=bool(gate), seq=seq, want=want, epoch=int(e[0]), restart=bool(e[1]),
                 gated=gated, img=img, out=out, layout=tuple(layout), base=[int(v) for v in k[8:16]] + [int(k[7])], draws=list(draws), joined=bool(join), frames=frames, fused=fused)
        self.applies.append(a)
        self.clock[lane] = self.clock[lane] | a["pred"] | {me}
        return a


def overlaps(a, b):
    return a[0] < b[1] and b[0] < a[1]


def check(model):
    ap = model.applies
    seen_epochs = []
    ends = [[None] * 9, [None] * 9]
    for n, a in enumerate(ap):
        before = set(range(n))
        # Never more than two applies in flight: a lane runs one launch at a time (stream order), so what apply n is not ordered behind lies on
        # the OTHER lane, where at most one launch runs at any moment; and n + 2 follows n on n's lane.  (An apply older than n - 1 that apply n
        # is not stream-ordered behind has published every tile before n starts: n starts behind n - 2, and an apply ends only after the sums of
        # all its tiles, each of which comes behind the previous apply's sum of the same tile - the gate)
        loose = before - a["pred"]
        assert all(ap[m]["lane"] != a["lane"] for m in loose), f"apply {n} is not ordered behind {sorted(loose)} of its own lane"
        assert n < 2 or (n - 2) in a["pred"], f"apply {n} may start before apply {n - 2} has ended"
        for m in loose:  # every apply in between is pipelined too, each waiting at the gate for the one before it
            assert all(ap[j]["hot"] and ap[j]["gate"] for j in range(m + 1, n + 1)), f"apply {n} beside apply {m} without a gate chain"
        prev_ordered = n == 0 or (n - 1) in a["pred"]
        if not prev_ordered:
            p = ap[n - 1]
            # ... and where n - 1 may still run, both are pipelined applies of the gated kernel on different lanes, n waits for n - 1's tile sums
            assert a["hot"] and p["hot"] and a["gated"] and p["gated"] and a["lane"] != p["lane"]
            assert a["gate"] and a["want"] == p["seq"] and a["seq"] == (p["seq"] + 1) % U32
            assert not a["restart"] and not a["joined"]
            # the caller's buffers: n reads nothing n - 1 writes and writes nothing n - 1 reads
            assert not overlaps(a["img"], p["out"]) and not overlaps(a["out"], p["img"])
            # ... and the planes of a tile lie where n - 1 has them: the gate orders tile against tile, which is memory against memory only then
            assert a["layout"] == p["layout"]
        if not a["hot"]:
            assert before <= a["pred"], "an apply that is not pipelined runs behind everything"
            assert not a["gate"] and a["lane"] == 0
        if a["gate"]:  # a gate only ever asks for a sequence number the previous launch publishes
            assert ap[n - 1]["gated"] and ap[n - 1]["seq"] == a["want"]
        # queue positions: a launch starts where the last launch ON ITS LANE ended; the lanes never share a counter
        for q in range(9):
            if ends[a["lane"]][q] is not None:
                assert a["base"][q] == ends[a["lane"]][q], f"apply {n} queue {q}"
            else:
                assert a["base"][q] == 0
            ends[a["lane"]][q] = (a["base"][q] + a["draws"][q]) % U32
        # epochs: + 1 per fused launch, a new count (the counters are cleared) only behind everything; none repeats within a count
        if not a["fused"]:
            continue
        if a["restart"]:
            assert before <= a["pred"] and a["epoch"] == 1
            seen_epochs = [1]
        else:
            assert not seen_epochs or a["epoch"] == seen_epochs[-1] + 1
            assert a["epoch"] < (1 << 29)
            seen_epochs.append(a["epoch"])


def random_run(lib, rng, steps, enabled=True, seq=0, done_epoch=0):
    m = Model(lib, enabled, seq, done_epoch)
    bufs = [(i * 1000, i * 1000 + 900) for i in range(6)]
    behind_other = []
    for _ in range(steps):
        r = rng.random()
        draws = [int(v) for v in rng.integers(1, 200, 9)]
        if r < 0.80:  # a hot apply of a frame loop: a few buffers in rotation, sometimes the last output as the next input
            i, o = rng.choice(len(bufs), 2, replace=False)
            if m.applies and rng.random() < 0.1:
                img, out = m.applies[-1]["out"], bufs[o]
            else:
                img, out = bufs[i], bufs[o]
            if img == out:
                continue
            m.apply(True, True, 1, img, out, draws, LAYOUTS[int(rng.integers(len(LAYOUTS)))] if rng.random() < 0.15 else WHOLE)
        elif r < 0.85:  # a batch (never pipelined, restarts the tile counters when the frame count changes)
            m.apply(False, True, int(rng.integers(2, 5)), bufs[0], bufs[1], draws)
        elif r < 0.88:  # one patch per workgroup (RPSF_OPT_PERSIST 0): not the gated kernel
            m.apply(False, False, 1, bufs[2], bufs[3], draws)
        elif r < 0.91:  # an apply through a view, on a caller's stream, with timing events ...: the gated kernel, not pipelined
            m.apply(False, True, 1, bufs[2], bufs[3], draws)
        elif r < 0.98:  # set_transfer, an option, synchronise, a host-array call, a download
            behind = m.other()
            assert behind == set(range(len(m.applies))), "after a join the public stream runs behind every apply"
            behind_other.append(len(m.applies))
        else:
            lib.emu_lanes_enable(int(rng.random() < 0.5))  # RPSF_OPT_PIPELINE (set_option joins first)
            m.other()
    m.other()
    assert m.clock[0] == set(range(len(m.applies)))
    return m


@pytest.mark.parametrize("seed", range(20))
def test_random_sequences_keep_the_lane_invariants(lib, seed):
    rng = np.random.default_rng(seed)
    m = random_run(lib, rng, 400)
    check(m)
    hot_pairs = sum(1 for n in range(1, len(m.applies)) if (n - 1) not in m.applies[n]["pred"])
    assert hot_pairs > 20, "the sequences must exercise overlapping applies"


def test_frame_loop_alternates_and_only_the_first_apply_forks(lib):
    m = Model(lib)
    for i in range(12):
        a = m.apply(True, True, 1, (0, 100), (200, 300), [5] * 9)
        assert a["lane"] == i % 2 and a["gate"] == (i > 0) and a["epoch"] == i + 1 and a["seq"] == i + 1
    check(m)
    assert m.other() == set(range(12))
    a = m.apply(True, True, 1, (0, 100), (200, 300), [5] * 9)
    assert a["lane"] == 0 and not a["gate"] and a["pred"] == set(range(12))  # behind a join: lane 0, nothing to wait for
    b = m.apply(True, True, 1, (0, 100), (200, 300), [5] * 9)
    assert b["lane"] == 1 and b["gate"] and set(range(12)) <= b["pred"] and 12 not in b["pred"]  # lane 1 was forked behind the join
    check(m)


def test_one_lane_when_the_option_is_off_or_the_stream_is_exposed(lib):
    for exposed in (False, True):
        m = Model(lib, enabled=exposed)
        if exposed:
            lib.emu_lanes_expose()
        for n in range(8):
            a = m.apply(True, True, 1, (0, 100), (200, 300), [3] * 9)
            assert a["lane"] == 0 and not a["gate"] and a["pred"] == set(range(n))
        check(m)


def test_chained_buffers_join(lib):
    m = Model(lib)
    m.apply(True, True, 1, (0, 100), (200, 300), [3] * 9)
    a = m.apply(True, True, 1, (250, 350), (400, 500), [3] * 9)  # reads what the previous apply writes
    assert a["joined"] is False and a["pred"] == {0} and not a["gate"]  # (lane 1 idle: nothing to record, lane 0 follows in stream order)
    m.apply(True, True, 1, (0, 100), (600, 700), [3] * 9)
    b = m.apply(True, True, 1, (800, 900), (50, 150), [3] * 9)  # writes what the previous apply reads, which runs on lane 1
    assert b["joined"] and b["pred"] == {0, 1, 2} and b["lane"] == 0
    check(m)


def test_sequence_numbers_and_the_gate_across_the_wrap(lib):
    assert lib.emu_lanes_seq_reached(5, 5) and lib.emu_lanes_seq_reached(6, 5) and not lib.emu_lanes_seq_reached(4, 5)
    assert lib.emu_lanes_seq_reached(0, U32 - 1) and lib.emu_lanes_seq_reached(1, U32 - 1) and not lib.emu_lanes_seq_reached(U32 - 1, 0)
    assert lib.emu_lanes_seq_reached(U32 - 1, U32 - 1) and not lib.emu_lanes_seq_reached(U32 - 2, U32 - 1)
    assert not lib.emu_lanes_seq_reached(0, 1) and lib.emu_lanes_seq_reached((1 << 31) - 1, 0) and not lib.emu_lanes_seq_reached(1 << 31, 0)
    m = Model(lib, seq=U32 - 3)
    published = None
    for i in range(6):  # sequence numbers 2^32 - 2, 2^32 - 1, 0, 1, 2, 3
        a = m.apply(True, True, 1, (0, 100), (200, 300), [1] * 9)
        assert a["seq"] == (U32 - 2 + i) % U32
        if a["gate"]:
            assert a["want"] == published and lib.emu_lanes_seq_reached(published, a["want"])
            assert not lib.emu_lanes_seq_reached((published - 1) % U32, a["want"]), "a tile one apply behind keeps the gate shut"
        published = a["seq"]
    check(m)


def test_epoch_restarts_before_the_counters_overflow(lib):
    m = Model(lib, done_epoch=(1 << 29) - 3)
    epochs = [m.apply(True, True, 1, (0, 100), (200, 300), [1] * 9) for _ in range(5)]
    assert [a["epoch"] for a in epochs] == [(1 << 29) - 2, (1 << 29) - 1, 1, 2, 3]
    assert epochs[2]["restart"] and not epochs[2]["hot"] and epochs[2]["pred"] == {0, 1} and not epochs[2]["gate"]
    check(m)


@pytest.mark.parametrize("other", LAYOUTS[1:])
def test_another_geometry_joins(lib, other):
    """Two row windows of a frame, another origin, another width, grown planes: tile t of the next apply is not where tile t of the last one
    is, so the applies do not overlap - whichever of the two lanes the last one took."""
    m = Model(lib)
    for i, lay in enumerate((WHOLE, WHOLE, other, other, other, WHOLE, other, WHOLE)):
        a = m.apply(True, True, 1, (0, 100), (200 + 1000 * (i & 1), 300 + 1000 * (i & 1)), [2] * 9, lay)
        if i and lay != m.applies[i - 1]["layout"]:
            assert a["pred"] == set(range(i)) and not a["gate"] and a["lane"] == 0
        elif i:
            assert a["gate"] and (i - 1) not in a["pred"]
    check(m)


def test_the_gate_guards_the_tiles_the_counters_count(lattice_lib):
    """The patches of the gated kernel compute their four tiles from the patch corner ((li + (q >> 1)) * ntj + lj + (q & 1), rpsf_kernels2.hpp,
    gate_tile); the tile counters are addressed through the quadrant words of lattice_build.  The two must name the same tiles, on full and on
    thinned lattices, whatever the processing order."""
    n, half = 256, 128
    cases = [lattice(n, nli, nlj) for nli in (1, 2, 3, 9, 17) for nlj in (1, 2, 9, 16, 33)]
    cases += [thinned(n, nli, nlj, seed) for seed, (nli, nlj) in enumerate([(3, 3), (9, 9), (9, 11), (17, 33), (33, 17)])]
    cases += [lattice(n, 9, 9, origin=(-128 + 64, -128 + 32))]
    checked = 0
    for coords in cases:
        t = lattice_build(lattice_lib, n, coords)
        if not (t["lattice"] and t["direct_ok"]):
            continue
        desc, quads = t["desc"], t["quads"]
        assert len(desc) == len(quads) == len(coords)
        li, lj = (desc[:, 0] - t["r0"]) // half, (desc[:, 1] - t["c0"]) // half
        for q in range(4):
            tile = (li + (q >> 1)) * t["ntj"] + lj + (q & 1)
            assert np.array_equal(tile, (quads[:, q] >> 8).astype(np.int64)), f"quadrant {q}"
            assert tile.min() >= 0 and tile.max() < t["nti"] * t["ntj"]
        checked += 1
    assert checked >= 25


# ---- the lane report (rpsf_plan_lane_info) and the sequences of tests/pipeline_cases.py -----------------------------------------------------
def lane_info(lib):
    v = np.zeros(6, np.int64)
    lib.emu_lanes_info(v.ctypes.data_as(VP))
    return [int(x) for x in v]


@pytest.mark.parametrize("seed", range(20))
def test_the_lane_report_counts_the_random_sequences(lib, seed):
    """Lane 0 and lane 1 sum to the pipelined applies, the gated count is the applies that may run beside their predecessor or behind it on
    the other lane, and a join is counted exactly when lane 1 held work the public stream did not wait for yet."""
    rng = np.random.default_rng(1000 + seed)
    m = Model(lib)
    bufs = [(i * 1000, i * 1000 + 900) for i in range(6)]
    want = dict(lane=[0, 0], gated=0, joins=0)
    busy = False  # lane 1 holds an apply no join has covered yet
    for _ in range(400):
        r = rng.random()
        before = lane_info(lib)
        if r < 0.75:
            i, o = rng.choice(len(bufs), 2, replace=False)
            a = m.apply(True, True, 1, bufs[i], bufs[o], [3] * 9, LAYOUTS[int(rng.integers(len(LAYOUTS)))] if rng.random() < 0.15 else WHOLE)
            pipelined = a["hot"] and bool(before[4]) and not before[5]
            if a["joined"] or not pipelined:
                want["joins"] += busy
                busy = False
            if pipelined:
                want["lane"][a["lane"]] += 1
                want["gated"] += a["gate"]
                busy = busy or a["lane"] == 1
            else:
                assert not a["gate"] and a["lane"] == 0
        elif r < 0.85:
            m.apply(False, True, int(rng.integers(1, 4)), bufs[0], bufs[1], [3] * 9)
            want["joins"] += busy
            busy = False
        elif r < 0.95:
            m.other()
            want["joins"] += busy
            busy = False
        else:
            m.other()
            want["joins"] += busy
            busy = False
            lib.emu_lanes_enable(int(rng.random() < 0.7))
        got = lane_info(lib)
        assert got[:4] == [want["lane"][0], want["lane"][1], want["gated"], want["joins"]]
        assert got[1] == sum(1 for a in m.applies if a["lane"] == 1)  # (nothing but a pipelined apply ever takes lane 1)
    check(m)
    assert want["lane"][1] > 20 and want["joins"] > 10, "the sequences must exercise lane 1 and joins that are due"


BUFFERS = {name: (i * 10000, i * 10000 + 9000) for i, name in enumerate(["f0", "f1", "f2", "f3", "top", "o0", "o1"])}
BUFFERS["o1"] = (BUFFERS["o0"][1], BUFFERS["o0"][1] + 9000)  # the two outputs are one allocation
SCRIPT_LAYOUTS = {"whole": WHOLE, "top": LAYOUTS[1]}


def replay(lib, script):
    """A script of tests/pipeline_cases.py on the model: the lane report's deltas, after the invariants of every apply have been checked."""
    m = Model(lib)
    multi = False
    for token in script:
        what = token[0]
        if what == "hot":
            m.apply(not multi, True, 1, BUFFERS[token[1]], BUFFERS[token[2]], [3] * 9, SCRIPT_LAYOUTS[token[3]])
        elif what == "cold":
            _, frames, fused, gated = token
            m.apply(False, gated, frames, (0, 1), (2, 3), [3] * 9, fused=fused)
        elif what == "join":
            m.other()
        elif what == "enable":
            lib.emu_lanes_enable(token[1])
        elif what == "expose":
            lib.emu_lanes_set_exposed(token[1])
        elif what == "multi":
            multi = True
        else:
            assert what == "nop", token
    check(m)
    return tuple(lane_info(lib)[:4])


def test_the_sequences_of_the_gpu_tests_give_the_lane_reports_they_expect(lib):
    scripts = pc.sequences()
    assert set(scripts) == set(pc.EXPECTED)
    wrong = {name: (replay(lib, script), pc.EXPECTED[name]) for name, script in scripts.items() if replay(lib, script) != pc.EXPECTED[name]}
    assert not wrong, wrong
    # by hand: forty hot applies alternate, all but the first wait at the gate, nothing joins; one operation behind a busy lane 1 joins once
    assert pc.EXPECTED["loop"] == (20, 20, 39, 0)
    assert pc.EXPECTED["set_transfer_device-k2"] == (3, 2, 3, 1) and pc.EXPECTED["set_transfer_device-k1"] == (3, 1, 2, 0)
    for k in pc.PREFIXES:  # every sandwich's prefix leaves lane 1 busy from two applies on, and its operation meets it
        for name, o in pc.OPS_BY_NAME.items():
            joins = pc.EXPECTED[f"{name}-k{k}"][3]
            if name == "setters_without_join":
                assert joins == 0
            else:
                assert joins >= (1 if k >= 2 else 0), (name, k)


def test_every_entry_point_that_takes_a_plan_is_accounted_for():
    """A new entry point cannot arrive without the decision: which case runs it behind pipelined applies, or why it touches no stream."""
    import re

    header = (ROOT / "include" / "rpsf.h").read_text()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    names = set(re.findall(r"\b(rpsf_\w+)\s*\(\s*(?:const\s+)?rpsf_plan\s*\*\s*\w", header))
    assert len(names) > 40 and "rpsf_apply_device" in names and "rpsf_plan_lane_info" in names and "rpsf_plan_create" not in names
    assert names == set(pc.COVERAGE), (sorted(names - set(pc.COVERAGE)), sorted(set(pc.COVERAGE) - names))
    known = set(pc.OPS_BY_NAME) | {"loop", "growth", "rounds", "destroy"}
    for name, (kind, value) in pc.COVERAGE.items():
        if kind == "cases":
            assert value and set(value) <= known, name
        else:
            assert kind == "no stream" and len(value) > 10, name
