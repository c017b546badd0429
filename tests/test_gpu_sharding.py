"""World-size-2 runs of the product's sharded step on ONE GPU (two processes, both on device 0).

The band compute is the HIP kernel, the stream / event choreography is ``ShardedApply.step()``'s and the seam add is K4
(``rpsf_add_rows``) in both tests; what differs is the transport of the 128 spill rows:

* ``test_sharded_step_world_2_rccl_same_device``: the product's own ``rpsf_comm_seam_exchange`` (RCCL send/recv).  RCCL
  refuses two ranks on one device in most builds ("Duplicate GPU detected"); the test then SKIPS with RCCL's own error
  string as the reason, so the log says what the hardware available here could not exercise.
* ``test_sharded_step_world_2_host_transport``: bench.py's ``GlooSeam`` (the rows travel through the host over gloo).
"""

import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, N = 1024, 1024, 256


def _case():
    from oracle import regpsf_oracle as orc

    coords = [tuple(int(v) for v in c) for c in orc.calculate_covering((H, W), N)]
    rng = np.random.default_rng(5)
    k = (rng.standard_normal((len(coords), N, N)) + 1j * rng.standard_normal((len(coords), N, N))).astype(np.complex64)
    image = (rng.standard_normal((H, W)) * 10 + 60).astype(np.float32)
    return coords, k, image


def _worker(rank, world, port, transport, overlap, queue):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as dist

    from regularizepsf_amd import _native
    from regularizepsf_amd.sharding import ShardedApply

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        comm = None
        if transport == "rccl":
            uid = torch.zeros(128, dtype=torch.uint8)
            if rank == 0:
                uid = torch.frombuffer(bytearray(_native.Comm.unique_id()), dtype=torch.uint8).clone()
            dist.broadcast(uid, 0)
            try:
                comm = _native.Comm(0, rank, world, bytes(uid.numpy().tobytes()))
            except Exception as exc:  # noqa: BLE001 - the reason goes into the skip message
                queue.put((rank, "refused", f"{type(exc).__name__}: {exc}"))
                return
        else:
            import bench

            comm = bench.GlooSeam(rank, world, 0)
        coords, k, image = _case()
        sh = ShardedApply(coords, lambda idx: k[idx], N, H, W, rank, world, 0, comm, overlap=overlap)
        b = sh.band
        sh.upload_rows(image[b.image_row0 : b.image_row0 + b.image_rows])
        outs = []
        for _ in range(3):  # repeated steps: the cross-stream ordering of step k + 1 against the add of step k
            sh.step()
            outs.append(sh.owned_rows())
        queue.put((rank, "ok", (b.out_row0, b.own_rows, outs[0], all(np.array_equal(o, outs[0]) for o in outs[1:]))))
        dist.barrier()
        if transport == "rccl":
            comm.close()
    finally:
        dist.destroy_process_group()


def _run(transport, overlap):
    import multiprocessing as mp  # (not torch.multiprocessing: torch brings its own HIP runtime, and this process may have loaded librpsf_hip.so)

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")  # no HIP call in this process before the children start
    queue = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, transport, overlap, queue)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(2):
            rank, status, payload = queue.get(timeout=600)
            results[rank] = (status, payload)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    return results


def _check(results):
    from oracle import regpsf_oracle as orc

    coords, k, image = _case()
    ref = orc.apply_transfer(image, coords, k, workers=-1)
    rows = 0
    for rank in (0, 1):
        status, (row0, own, out, same) = results[rank]
        assert status == "ok" and same
        assert np.abs(out - ref[row0 : row0 + own]).max() <= 1e-5 * np.abs(ref).max(), rank
        rows += own
    assert rows == H


@pytest.mark.timeout(900, method="thread")
@pytest.mark.parametrize("overlap", [True, False, "pipeline"])
def test_sharded_step_world_2_host_transport(overlap):
    _check(_run("gloo", overlap))


@pytest.mark.timeout(900, method="thread")
def test_sharded_step_world_2_rccl_same_device():
    results = _run("rccl", True)
    refused = [payload for status, payload in results.values() if status == "refused"]
    if refused:
        pytest.skip(f"RCCL refuses a world of two ranks on one device here: {refused[0]}")
    _check(results)


# ---- the sharded step straight behind pipelined applies of the band's plan (RPSF_OPT_PIPELINE) --------------------------------
def _pipelined_worker(rank, world, port, form, queue):
    """k = 1, 2, 3 pipelined applies of the band's main plan into two buffers in turn, then ``step()`` with no synchronise in between: the step's
    own apply, its waits, K4 and the seam exchange go onto the plan's stream handle behind an apply that is in flight on the second lane.
    Reference: the same calls with the option off and a synchronise behind each.  Everything is compared here, bit for bit; the lane report's
    deltas go back to the test."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist

    import bench
    from regularizepsf_amd import _native
    from regularizepsf_amd.sharding import ShardedApply
    from tests import pipeline_cases as pc

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        coords, k, image = _case()
        sh = ShardedApply(coords, lambda idx: k[idx], N, H, W, rank, world, 0, bench.GlooSeam(rank, world, 0), overlap=pc.SHARDED_FORMS[form])
        b, g = sh.band, sh.geometry
        rows = image[b.image_row0 : b.image_row0 + b.image_rows]
        sh.upload_rows(rows)
        others = [_native.DeviceBuffer(rows.nbytes).upload(np.ascontiguousarray(rows[::-1]) * np.float32(i + 2)) for i in range(3)]  # the prefix's frames
        outs = [_native.DeviceBuffer(g.out_rows * W * 4) for _ in range(2)]
        fill = np.full((g.out_rows, W), -1.0, np.float32)
        report = {}
        for n in (1, 2, 3):
            results = {}
            for pipelined in (False, True):
                sh.synchronize()
                for o in outs:
                    o.upload(fill)
                sh.plan.set_option("pipeline", int(pipelined))  # (1: the caller's word that nothing of theirs is on the plan's stream any more)
                before = sh.plan.lane_info()
                for i in range(n):
                    sh.plan.apply_device(others[i].ptr, outs[i & 1].ptr, g)
                    if not pipelined:
                        sh.synchronize()
                sh.step()
                info = sh.plan.lane_info()
                lanes = tuple(info[key] - before[key] for key in ("lane0", "lane1", "gated", "joins"))
                results[pipelined] = [sh.owned_rows(), sh.spill_rows()] + [o.download((g.out_rows, W)) for o in outs]
                if pipelined:
                    report[n] = {"lanes": lanes, "exposed": info["exposed"], "enabled": info["enabled"],
                                 "same": [pc.same_bytes(x, y) for x, y in zip(results[True], results[False])],
                                 "fresh": not np.array_equal(results[True][0][: min(b.own_rows, g.out_rows)], results[True][2][: min(b.own_rows, g.out_rows)])
                                 and (n < 2 or not np.array_equal(results[True][2], results[True][3])) and not np.array_equal(results[True][2], fill)}
                else:
                    report[n, "reference lanes"] = lanes
        queue.put((rank, "ok", report))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900, method="thread")
@pytest.mark.parametrize("form", ["sequence", "overlap", "pipeline"])
def test_sharded_step_behind_pipelined_applies(form):
    import multiprocessing as mp

    from tests import pipeline_cases as pc

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    procs = [ctx.Process(target=_pipelined_worker, args=(r, 2, port, form, queue)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(2):
            rank, status, payload = queue.get(timeout=600)
            results[rank] = (status, payload)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank in (0, 1):
        status, report = results[rank]
        assert status == "ok"
        for n in pc.PREFIXES:
            got, expected = report[n], pc.EXPECTED[f"sharded_{form}-r{rank}-k{n}"]
            print(f"LANES | sharded step, {form}, rank {rank}, prefix {n} | {got['lanes']} | expected {expected} | exposed {got['exposed']}, enabled {got['enabled']}")
            assert report[n, "reference lanes"] == (0, 0, 0, 0)
            assert all(got["same"]), (form, rank, n, got["same"])  # owned rows, spill, both prefix outputs
            assert got["fresh"], "the prefix outputs and the band's rows must differ from one another"
            assert got["lanes"] == expected
            assert got["exposed"] and got["enabled"] == (form != "pipeline")
