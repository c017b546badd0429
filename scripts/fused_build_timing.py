"""What the fused star finding saves: in one process and on the same frames, the composition
``build(frames, stars=find_stars(frames))`` - two uploads per frame and the mesh's round trip to the host - next to
``ArrayPSFBuilder(n, finder="device").build(frames)``.

    python scripts/fused_build_timing.py [--repeats 5] [--stars 500] [--quick]

Three cases: 8 host frames of 2048 x 2048 with N = 32; the same frames as device arrays (the composition has to bring them to the host
first: that is part of its time); 4 host frames of 1024 x 1024 with interpolation_scale = 2 and N = 16.  Per case both routes run once to
warm up and then alternate --repeats times; the times are host clocks around calls that end with the model on the host, medians and
extremes in milliseconds.  The clean-up runs on the device on both sides (clean_cell on the host is a millisecond per cell and the same
on both).  The S1b kernel time is the device time between events around its launch (rpsf_stars_mesh_ms), next to S1's and to the host's
filter_mesh on the same mesh.  Both routes must give the same bytes; the script fails otherwise.  Prints one JSON line per case.
--quick shrinks the frames: a rehearsal of the script, not a measurement.
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
from regularizepsf_amd import stars as star_finder  # noqa: E402

from builder_timing import make_frame  # noqa: E402  (scripts/ is sys.path[0] when this file is run)

BOX = 64


def summary(ms: list[float]) -> dict:
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def same(a, b) -> bool:
    return a[0].values.tobytes() == b[0].values.tobytes() and a[1] == b[1]


def mesh_times(frame: np.ndarray, repeats: int) -> dict:
    """S1 and S1b device times of one frame on the fused route, and the host's filter_mesh on the same raw mesh."""
    finder = star_finder._Finder(frame.shape, BOX)
    s1, s1b, host = [], [], []
    for _ in range(repeats + 1):
        finder.background_device(frame, None)
        s1.append(finder.kernel_ms()[0])
        s1b.append(finder.mesh_ms())
    level, rms = finder.background(frame, None)
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        star_finder.filter_mesh(level, rms)
        host.append((time.perf_counter() - t0) * 1e3)
    finder.close()
    return {"mesh_nodes": int(level.size), "s1_kernel_ms": float(np.median(s1[1:])), "s1b_kernel_ms": float(np.median(s1b[1:])),
            "host_filter_mesh_ms": float(np.median(host[1:]))}


def run_case(name: str, composition, fused, repeats: int) -> dict:
    want, got = composition(), fused()  # warm-up: code objects, allocations
    if not same(got, want):
        raise SystemExit(f"{name}: the fused build differs from the composition")
    t_composition, t_fused = [], []
    for _ in range(repeats):
        for call, times in ((composition, t_composition), (fused, t_fused)):
            t0 = time.perf_counter()
            call()
            times.append((time.perf_counter() - t0) * 1e3)
    out = {"case": name, "composition": summary(t_composition), "fused": summary(t_fused), "same_bytes": True}
    out["fused_over_composition"] = out["fused"]["median_ms"] / out["composition"]["median_ms"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stars", type=int, default=500)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    size, small, stars = (256, 128, 20) if args.quick else (2048, 1024, args.stars)
    rng = np.random.default_rng(13)
    frames = [make_frame(size, stars, rng)[0] for _ in range(8)]
    small_frames = [make_frame(small, max(1, stars // 4), rng)[0] for _ in range(4)]

    def host_composition():
        return rp.ArrayPSFBuilder(32, cleanup="device").build(frames, stars=rp.find_stars(frames, box=BOX))

    def host_fused():
        return rp.ArrayPSFBuilder(32, cleanup="device", finder="device", finder_options={"box": BOX}).build(frames)

    res = run_case(f"8 host frames of {size} x {size}, N = 32", host_composition, host_fused, args.repeats)
    res.update(mesh_times(frames[0], args.repeats), stars_found=int(sum(len(s) for s in rp.find_stars(frames, box=BOX))))
    print(json.dumps(res), flush=True)

    device_frames = [rp.to_device(f) for f in frames]

    def device_composition():  # what a caller had to do before: bring the frames down, then the two uploads each
        host = [f.to_host() for f in device_frames]
        return rp.ArrayPSFBuilder(32, cleanup="device").build(host, stars=rp.find_stars(host, box=BOX))

    def device_fused():
        return rp.ArrayPSFBuilder(32, cleanup="device", finder="device", finder_options={"box": BOX}).build(device_frames)

    print(json.dumps(run_case(f"8 device frames of {size} x {size}, N = 32", device_composition, device_fused, args.repeats)), flush=True)

    def scaled_composition():
        found = rp.find_stars(rp.scale_image(small_frames, 2), box=BOX)
        return rp.ArrayPSFBuilder(16, interpolation="device", cleanup="device").build(small_frames, interpolation_scale=2, stars=found)

    def scaled_fused():
        builder = rp.ArrayPSFBuilder(16, interpolation="device", cleanup="device", finder="device", finder_options={"box": BOX})
        return builder.build(small_frames, interpolation_scale=2)

    print(json.dumps(run_case(f"4 host frames of {small} x {small}, interpolation_scale = 2, N = 16", scaled_composition, scaled_fused,
                              args.repeats)), flush=True)


if __name__ == "__main__":
    main()
