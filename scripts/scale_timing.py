"""What interpolation_scale costs: the two upscale passes on the device, a scaled build next to an unscaled one on the
same frames, and SciPy's RectBivariateSpline on this box's host, called as the reference calls it (image_processing.py:49-59).

    python scripts/scale_timing.py [--size 2048] [--scale 2] [--build-size 1024] [--frames 4] [--stars 500] [--n 16] [--repeats 5]

Prints one JSON line.  U1 / U2 are device times between events (rpsf_scale_kernel_ms), medians over --repeats calls after a first
call that loads the module; the call time includes the frame's upload and the scaled frame's download.  The builds run on --frames
frames of --build-size pixels with the clean-up on the device: the reference's covering of a scaled build has four times the cells of
the unscaled one, and clean_cell on the host is a millisecond per cell.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

import regularizepsf_amd as rp  # noqa: E402
from regularizepsf_amd import _native  # noqa: E402

from builder_timing import make_frame  # noqa: E402  (scripts/ is sys.path[0] when this file is run)


def kernel_ms() -> tuple[float, float]:
    u1, u2 = ctypes.c_double(0), ctypes.c_double(0)
    _native.check(_native.lib().rpsf_scale_kernel_ms(ctypes.byref(u1), ctypes.byref(u2)))
    return u1.value, u2.value


def host_upscale(frame: np.ndarray, scale: int) -> np.ndarray:
    from scipy.interpolate import RectBivariateSpline

    h, w = frame.shape
    spline = RectBivariateSpline(np.arange(h), np.arange(w), frame)
    return spline(np.linspace(0, h - 1, 1 + (h - 1) * scale), np.linspace(0, w - 1, 1 + (w - 1) * scale))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--build-size", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--stars", type=int, default=500)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    s, n = args.scale, args.n
    rng = np.random.default_rng(11)
    big, _ = make_frame(args.size, args.stars, rng)
    made = [make_frame(args.build_size, args.stars, rng) for _ in range(args.frames)]
    frames, stars = [m[0] for m in made], [m[1] for m in made]
    res: dict = {"size": args.size, "scale": s, "build_size": args.build_size, "frames": args.frames, "stars_per_frame": args.stars, "n": n}

    rp.scale_image(big[:64, :64], s)  # first launch: module load
    u1, u2, wall = [], [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        scaled = rp.scale_image(big, s)
        wall.append((time.perf_counter() - t0) * 1e3)
        a, b = kernel_ms()
        u1.append(a)
        u2.append(b)
    res["u1_kernel_ms"], res["u2_kernel_ms"] = float(np.median(u1)), float(np.median(u2))
    res["scale_image_call_ms"] = float(np.median(wall))
    # what the two passes must move: the frame read once and the scaled frame written once, float64 on the device
    res["upscale_GBps"] = (big.size * big.itemsize + scaled.size * 8) / ((res["u1_kernel_ms"] + res["u2_kernel_ms"]) * 1e-3) / 1e9

    t0 = time.perf_counter()
    want = host_upscale(big.astype(np.float64), s)
    res["host_rectbivariatespline_ms"] = (time.perf_counter() - t0) * 1e3
    res["upscale_max_err_over_peak"] = float(np.abs(scaled - want).max() / np.abs(big).max())

    # a scaled build against an unscaled one on the same frames; the scaled build's stars are the same stars in scaled-frame pixels
    scaled_stars = [p * s for p in stars]
    for cleanup in ("device",):
        rp.ArrayPSFBuilder(n, cleanup=cleanup).build(frames[:1], stars=stars[:1])
        t0 = time.perf_counter()
        rp.ArrayPSFBuilder(n, cleanup=cleanup).build(frames, stars=stars)
        res[f"build_unscaled_{cleanup}_ms"] = (time.perf_counter() - t0) * 1e3
        builder = rp.ArrayPSFBuilder(n, interpolation="device", cleanup=cleanup)
        builder.build(frames[:1], interpolation_scale=s, stars=scaled_stars[:1])
        t0 = time.perf_counter()
        _, counts = builder.build(frames, interpolation_scale=s, stars=scaled_stars)
        res[f"build_scaled_{cleanup}_ms"] = (time.perf_counter() - t0) * 1e3
        res["scaled_cells"], res["scaled_memberships"] = len(counts), int(sum(counts.values()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
