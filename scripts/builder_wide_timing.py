"""Device time of the PSF builder's per-star and per-cell kernels at N = 128 (B1, B3) and at N = 256 (B1w, B3w) in one run, and one
whole ArrayPSFBuilder(256, cleanup="device").build at the headline geometry ("Wide sizes").

    python scripts/builder_wide_timing.py [--size 4096] [--stars 512] [--repeats 5]

One frame of --size squared with --stars stars; both sizes cut their patches at the same positions.  Prints one JSON line.  The
yardstick for N = 256 is the N = 128 figure of the same run times 4, the pixel ratio; the prefilter's serial length doubles besides.
"""

from __future__ import annotations

import argparse
import json
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

import regularizepsf_amd as rp  # noqa: E402
from regularizepsf_amd import builder as bld  # noqa: E402
from scripts.builder_timing import make_frame  # noqa: E402


def stages(n: int, frame: np.ndarray, pos: np.ndarray, repeats: int) -> dict:
    corner, rounded, shift = bld.star_geometry(pos, n)
    warm = bld._Stack(n, 0, len(pos))
    warm.add_frame(frame, rounded[:2], shift[:2], np.inf, 0.0, np.inf)  # first launch: module load
    warm.close()
    b1 = []
    for k in range(repeats):  # a fresh stack every time: the same launch, and the last one is kept for the stages behind it
        stack = bld._Stack(n, 0, len(pos))
        flags = stack.add_frame(frame, rounded, shift, np.inf, 0.0, np.inf)
        b1.append(stack.kernel_ms()[0])
        if k < repeats - 1:
            stack.close()
    corners = rp.calculate_covering(frame.shape, n)
    offsets, members = bld.cell_membership(corner[flags == 1], corners, n)
    b3 = []
    for _ in range(repeats):
        flagged = stack.model("median", 50.0, offsets, members)[1]
        b3.append(stack.clean_ms())
    b2 = stack.kernel_ms()[1]
    stack.close()
    with_stars = int((np.diff(offsets) > 0).sum())
    return {"n": n, "stars": len(pos), "accepted": int((flags == 1).sum()), "b1_ms": float(np.median(b1)),
            "b1_us_per_star": float(np.median(b1)) * 1e3 / len(pos), "cells": len(corners), "cells_with_stars": with_stars,
            "b2_median_ms": b2, "b3_ms": float(np.median(b3)), "b3_us_per_cell": float(np.median(b3)) * 1e3 / len(corners),
            "b3_flagged": int(flagged.sum())}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--stars", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    frame, pos = make_frame(args.size, args.stars, np.random.default_rng(11))
    res: dict = {"size": args.size, "stars": args.stars, "repeats": args.repeats}
    res["n128"] = stages(128, frame, pos, args.repeats)
    res["n256"] = stages(256, frame, pos, args.repeats)
    res["b1_ratio"] = res["n256"]["b1_us_per_star"] / res["n128"]["b1_us_per_star"]
    res["b3_ratio"] = res["n256"]["b3_us_per_cell"] / res["n128"]["b3_us_per_cell"]
    builder = rp.ArrayPSFBuilder(256, cleanup="device")
    builder.build(frame, stars=[pos])
    t0 = time.perf_counter()
    _, counts = builder.build(frame, stars=[pos])
    res["build_256_device_cleanup_ms"] = (time.perf_counter() - t0) * 1e3
    res["build_256_patches"] = int(sum(counts.values()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
