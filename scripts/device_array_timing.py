"""What a device-resident frame costs through the public API, beside the private loop it replaces:

  per call of ``transform.apply(dev, out=dev_out, stream=s)``, no host wait inside the loop, the stream drained at the end -
    zero_copy   float32 in, float32 out: the views go into rpsf_apply_device as they are
    f64_f64     float64 in, float64 out: kernels C1 and C2 around the same apply
    u16_in      uint16 in, float32 out: kernel C1
  and ``safe``, the zero-copy call with stream=None (one device wait before, one stream wait after),
  at 4096 x 4096 / 256-pixel patches and 512 x 512 / 64-pixel patches, beside rpsf_apply_device_loop_ms of the same plan (device time
  per apply between one pair of events) and a Python loop over the private ``_native.Plan.apply_device`` on raw pointers.

    python scripts/device_array_timing.py [--iters 200] [--rounds 5] [--private-only]

--private-only measures the two private figures alone: it uses nothing this feature added, so the same file times a checkout from
before it (RPSF_TREE=<that checkout> picks the package to import).  Prints one JSON line.
"""
import argparse
import json
import os
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, os.environ.get("RPSF_TREE") or str(pathlib.Path(__file__).resolve().parent.parent))
import regularizepsf_amd as rp  # noqa: E402
from regularizepsf_amd import _native  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--private-only", action="store_true")
a = ap.parse_args()


def covering_transfer(shape, n, seed):
    """The covering's corners (regularizepsf/util.py:10-53 through the package's own calculate_covering) and a random complex64 K."""
    rng = np.random.default_rng(seed)
    coords = [tuple(int(v) for v in c) for c in rp.calculate_covering(shape, n)]
    k = (rng.standard_normal((len(coords), n, n)) + 1j * rng.standard_normal((len(coords), n, n))).astype(np.complex64)
    return coords, k


def best_of(rounds, iters, call, drain):
    """ms per call: `iters` calls back to back, then `drain`; the best round."""
    best = 1e9
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
        drain()
        best = min(best, 1e3 * (time.perf_counter() - t0) / iters)
    return best


result = {"device": _native.device_info(0)[1], "iters": a.iters, "rounds": a.rounds, "private_only": bool(a.private_only), "cases": {}}
for side, n in ((4096, 256), (512, 64)):
    shape = (side, side)
    iters = a.iters if side <= 1024 else max(20, a.iters // 4)
    coords, k = covering_transfer(shape, n, 1)
    t = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))
    plan = t._device_plan()
    frame = (np.random.default_rng(2).standard_normal(shape) * 10 + 30).astype(np.float32)
    row = {}
    # ---- the private path: raw pointers and a hand-filled geometry
    img = _native.DeviceBuffer(frame.nbytes).upload(frame)
    out = _native.DeviceBuffer(frame.nbytes)
    geom = _native.Geometry.whole(*shape, _native.PAD_MODES["symmetric"])
    plan.apply_device(img.ptr, out.ptr, geom)
    plan.synchronize()
    row["rpsf_apply_device_loop_ms"] = min(plan.apply_device_loop_ms(img.ptr, out.ptr, geom, iters) for _ in range(a.rounds))
    row["private_python_loop_ms"] = best_of(a.rounds, iters, lambda: plan.apply_device(img.ptr, out.ptr, geom), plan.synchronize)
    reference = out.download(shape)
    if not a.private_only:
        s = _native.Stream()
        dev, dev_out = rp.to_device(frame), rp.device_empty(shape, np.float32)
        dev64, out64 = rp.to_device(frame.astype(np.float64)), rp.device_empty(shape, np.float64)
        dev16 = rp.to_device(np.clip(frame * 500, 0, 65535).astype(np.uint16))

        def drain(stream=s):
            _native.stream_synchronize(stream.ptr)

        for name, args in (("zero_copy", (dev, dev_out)), ("f64_f64", (dev64, out64)), ("u16_in", (dev16, dev_out))):
            t.apply(args[0], out=args[1], stream=s)
            drain()
            row[name + "_ms"] = best_of(a.rounds, iters, lambda x=args[0], o=args[1]: t.apply(x, out=o, stream=s), drain)
            row[name + "_route"] = t.last_route
        t.apply(dev, out=dev_out, stream=s)
        row["zero_copy_equals_private"] = bool(np.array_equal(dev_out.to_host(), reference))
        row["safe_ms"] = best_of(a.rounds, iters, lambda: t.apply(dev, out=dev_out), lambda: None)
        # what the zero-copy call adds to the private loop on the host: the call itself with the device out of the way
        from regularizepsf_amd.transform import _kernel_stamp

        t0 = time.perf_counter()
        for _ in range(200):
            _kernel_stamp(t._transfer_kernel)
        row["kernel_stamp_ms"] = 1e3 * (time.perf_counter() - t0) / 200
        s.close()
    img.free()
    out.free()
    result["cases"][f"{side}x{side}_n{n}"] = {key: (round(v, 5) if isinstance(v, float) else v) for key, v in row.items()}
print(json.dumps(result), flush=True)
