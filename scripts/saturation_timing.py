"""The saturation branch of apply through saturation="host" and saturation="device", one process, interleaved:

  A  the reference's example workload (docs/source/example.ipynb: 512 x 512 frames, psf_size 64, saturation_threshold=2000;
     frames by scripts/notebook_workload.py's recipe), host arrays in and out;
  B  one 4096 x 4096 frame, psf_size 256, ~200 saturated stars and one bleed column of 2000 rows;
  the device time of kernels F1 ... F5 behind both, F4's time per masked pixel of the bleed column (the serial chain),
  and rpsf_apply_device_saturated on a frame that stays on the GPU.

    python scripts/saturation_timing.py [--frames 100] [--rounds 5] [--skip-large]
"""
import argparse
import pathlib
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import regularizepsf_amd as rp  # noqa: E402
from oracle import regpsf_oracle as orc  # noqa: E402  (synthetic inputs)
from regularizepsf_amd import _native  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--skip-large", action="store_true")
a = ap.parse_args()
print(f"device: {_native.device_info(0)[1]}", flush=True)


def transforms(h, w, n):
    coords, k = orc.synthetic_transfer(h, w, n, alpha=1.0, epsilon=0.1)
    return {route: rp.ArrayPSFTransform(rp.IndexedCube(coords, k), saturation=route) for route in ("host", "device")}


def interleaved(ts, frames, rounds, **kwargs):
    """ms per frame of every route, the routes taking turns round by round; (best, median) each."""
    times = {route: [] for route in ts}
    for _ in range(rounds):
        for route, t in ts.items():
            t0 = time.perf_counter()
            for f in frames:
                t.apply(f, **kwargs)
            times[route].append(1e3 * (time.perf_counter() - t0) / len(frames))
    return {route: (min(v), statistics.median(v)) for route, v in times.items()}


def kernel_ms(t, frames, **kwargs):
    plan = t._device_plan()
    rows = []
    for f in frames:
        t.apply(f, **kwargs)
        rows.append(plan.saturation_kernel_ms())
    return np.mean(rows, axis=0), np.max(rows, axis=0)


def resident(t, frame, threshold, iters):
    """rpsf_apply_device_saturated on a frame that is on the GPU and stays there: ms per call, the stream drained at the end."""
    plan = t._device_plan()
    img = _native.DeviceBuffer(frame.nbytes).upload(frame)
    out = _native.DeviceBuffer(frame.nbytes)
    mode = _native.PAD_MODES["symmetric"]
    for _ in range(3):
        plan.apply_device_saturated(img.ptr, out.ptr, *frame.shape, mode, threshold, 1, 7)
    plan.synchronize()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(iters):
            plan.apply_device_saturated(img.ptr, out.ptr, *frame.shape, mode, threshold, 1, 7)
        plan.synchronize()
        best = min(best, 1e3 * (time.perf_counter() - t0) / iters)
    result = out.download(frame.shape)
    img.free()
    out.free()
    return best, result


def report(label, res):
    for route, (best, median) in res.items():
        print(f"  {label}, saturation={route!r}: best {best:.3f} ms per frame, median {median:.3f}", flush=True)


# ---------------------------------------------------------------------------------------------------------------- A
h = w = 512
ts = transforms(h, w, 64)
frames = [orc.starfield(h, w, 100 + i) for i in range(a.frames)]
kw = {"saturation_threshold": 2000}
hot = [int((f > 2000).sum()) for f in frames]
print(f"A: {a.frames} frames of {h}x{w} float32, N=64, saturation_threshold=2000; hot pixels per frame: mean {np.mean(hot):.1f}, max {max(hot)}")
same = all(np.array_equal(ts["host"].apply(f, **kw), ts["device"].apply(f, **kw), equal_nan=True) for f in frames[:10])
print(f"  the two routes agree bit for bit on the first 10 frames: {same}")
t_warm = time.perf_counter()
while time.perf_counter() - t_warm < 0.5:
    for t in ts.values():
        t.apply(frames[0], **kw)
report("A", interleaved(ts, frames, a.rounds, **kw))
report("A without a threshold (the default path, for scale)", interleaved({"host": ts["host"]}, frames, a.rounds))
mean, worst = kernel_ms(ts["device"], frames, **kw)
print("  A, device time of F1 .. F5 per frame, ms (F3 includes the host's one wait): mean " + " ".join(f"{x:.4f}" for x in mean)
      + " | max " + " ".join(f"{x:.4f}" for x in worst))
best, result = resident(ts["device"], frames[0], 2000.0, 200)
agree = np.array_equal(result, ts["device"].apply(frames[0], **kw).astype(np.float32), equal_nan=True)
print(f"  A, rpsf_apply_device_saturated on a resident frame: {best:.3f} ms per call (equal to the class route: {agree})", flush=True)

# ---------------------------------------------------------------------------------------------------------------- B
if not a.skip_large:
    h = w = 4096
    ts = transforms(h, w, 256)
    rng = np.random.default_rng(1)
    frame = np.minimum(orc.starfield(h, w, 7), 1500.0).astype(np.float32)
    yy, xx = np.mgrid[-3:4, -3:4]
    for r, c in zip(rng.integers(8, h - 8, 200), rng.integers(8, w - 8, 200)):  # saturated cores of 7 x 7 stars
        frame[r - 3 : r + 4, c - 3 : c + 4] = np.maximum(frame[r - 3 : r + 4, c - 3 : c + 4], 6.0e4 * np.exp(-(yy**2 + xx**2) / 4.0))
    frame[1000:3000, 2049] = 6.0e4  # the bleed column
    column_masked = 2000 * 3 + 2  # dilation 1
    print(f"B: one {h}x{w} float32 frame, N=256, {int((frame > 2000).sum())} hot pixels, bleed column of 2000 rows")
    for t in ts.values():
        t.apply(frame, **kw)
    same = np.array_equal(ts["host"].apply(frame, **kw), ts["device"].apply(frame, **kw), equal_nan=True)
    print(f"  the two routes agree bit for bit: {same}")
    report("B", interleaved(ts, [frame], max(3, a.rounds), **kw))
    mean, _ = kernel_ms(ts["device"], [frame] * 3, **kw)
    print("  B, device time of F1 .. F5, ms: " + " ".join(f"{x:.3f}" for x in mean))
    print(f"  B, F4 per masked pixel of the bleed column ({column_masked} pixels, one wave, the longest chain of the launch): "
          f"{1e3 * mean[3] / column_masked:.3f} us")
    best, _ = resident(ts["device"], frame, 2000.0, 5)
    print(f"  B, rpsf_apply_device_saturated on a resident frame: {best:.3f} ms per call", flush=True)
