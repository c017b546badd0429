"""Device time of kernels F1 ... F5 with and without a bad-pixel mask ("Bad-pixel masks"), one process, interleaved:
one resident 512 x 512 float32 frame, psf_size 64, scripts/saturation_timing.py's workload A, a frame-group of one through the batch
entry points (so that every route runs the same F4, ordering pass included):

  threshold   rpsf_apply_batch_device_saturated with saturation_threshold=2000
  as mask     rpsf_apply_batch_device_masked with threshold=+inf and the same pixels (the dilated hot mask) given as a uint8 device mask
  null mask   rpsf_apply_batch_device_masked with mask NULL and fill_nonfinite 0: the unmasked entry point's code
  nonfinite   rpsf_apply_batch_device_masked with saturation_threshold=2000 and fill_nonfinite=1, no mask (nothing is non-finite)

from rpsf_saturation_kernel_ms, mean and best over --iters calls per route and round.  On a commit without the masked entry points
only the first route runs, which gives the parent's numbers from the same script.

    python scripts/mask_timing.py [--iters 50] [--rounds 5]
"""
import argparse
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import regularizepsf_amd as rp  # noqa: E402
from oracle import regpsf_oracle as orc  # noqa: E402  (synthetic inputs)
from regularizepsf_amd import _native  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
print(f"device: {_native.device_info(0)[1]}", flush=True)

H = W = 512
N, THRESHOLD, DILATION, WIDTH = 64, 2000.0, 1, 7
coords, k = orc.synthetic_transfer(H, W, N, alpha=1.0, epsilon=0.1)
plan = rp.ArrayPSFTransform(rp.IndexedCube(coords, k))._device_plan()
frame = orc.starfield(H, W, 100).astype(np.float32)
mode = _native.PAD_MODES["symmetric"]
img = _native.DeviceBuffer(frame.nbytes).upload(frame)
outs = {}


def out_buffer(route):
    if route not in outs:
        outs[route] = _native.DeviceBuffer(frame.nbytes)
    return outs[route]


routes = {"threshold": lambda o: plan.apply_batch_device_saturated(img.ptr, o.ptr, 1, H * W, H * W, H, W, mode, THRESHOLD, DILATION, WIDTH)}
if hasattr(plan, "apply_batch_device_masked"):
    from scipy.ndimage import binary_dilation

    mask = rp.to_device(binary_dilation(frame > THRESHOLD, iterations=DILATION).astype(np.uint8))
    view = _native.View(mask.ptr, _native.DTYPES["|u1"], H, W, W, 1)
    inf = float("inf")
    routes["as mask"] = lambda o: plan.apply_batch_device_masked(img.ptr, o.ptr, 1, H * W, H * W, H, W, mode, inf, DILATION, WIDTH, [view], False)
    routes["null mask"] = lambda o: plan.apply_batch_device_masked(img.ptr, o.ptr, 1, H * W, H * W, H, W, mode, THRESHOLD, DILATION, WIDTH, None, False)
    routes["nonfinite"] = lambda o: plan.apply_batch_device_masked(img.ptr, o.ptr, 1, H * W, H * W, H, W, mode, THRESHOLD, DILATION, WIDTH, None, True)
print(f"one resident {H}x{W} float32 frame, N={N}, threshold {THRESHOLD:g}, dilation {DILATION}, width {WIDTH}; "
      f"{int((frame > THRESHOLD).sum())} hot pixels; {a.rounds} rounds of {a.iters} calls per route, interleaved", flush=True)

masked = {}
for route, call in routes.items():  # warm-up, and what every route masks
    for _ in range(3):
        masked[route] = int(call(out_buffer(route))[0])
    plan.synchronize()
results = {route: outs[route].download(frame.shape) for route in routes}
for route in routes:
    same = np.array_equal(results[route].view(np.uint32), results["threshold"].view(np.uint32))
    print(f"  {route:10s}: {masked[route]} masked pixels of the padded frame; the bits of 'threshold': {same}", flush=True)

rows = {route: [] for route in routes}
for _ in range(a.rounds):
    for route, call in routes.items():
        per_call = []
        for _ in range(a.iters):
            call(out_buffer(route))
            per_call.append(plan.saturation_kernel_ms())
        rows[route].append(np.mean(per_call, axis=0))
print("device time per call, ms:      F1      F2      F3      F4      F5   (F3 includes the host's one wait)")
for route, r in rows.items():
    r = np.array(r)
    print(f"  {route:10s} mean  " + " ".join(f"{x:7.4f}" for x in r.mean(axis=0)))
    print(f"  {route:10s} best  " + " ".join(f"{x:7.4f}" for x in r.min(axis=0)))
    print(f"  {route:10s} worst " + " ".join(f"{x:7.4f}" for x in r.max(axis=0)), flush=True)
img.free()
for o in outs.values():
    o.free()
