"""Time the weighted model-fit kernel S12 next to S8 on one large frame, at that frame's detections, with a model built from the same frame:
    python scripts/fitw_timing.py [--size 4096] [--stars 10000] [--repeats 5] [--psf-size 32] [--radius 8] [--limit 300] [--out FILE]

The frame, the stars and the model are scripts/fit_timing.py's.  The variance map is sky + max(frame, 0) / gain computed on
the host in float32 - a map that says what the noise model says, so that the two modes do the same arithmetic after the variance itself.
Medians of --repeats after one warm-up of
  * rpsf_stars_fit_weighted_ms, the device time of S12, with the map and with the noise model (finite gain, and gain = inf), with and
    without a fitted background, next to rpsf_stars_fit_ms (S8) on the same finder, model and positions in the same run; the ratio
    S12 / S8; rpsf_stars_variance_host's upload on the host clock; fit_weighted on the host clock; the distribution of the flags,
  * fit_stars_weighted end to end in both modes on host frames (host clock around the call), next to fit_stars,
  * the float64 NumPy restatement of the definition (tests/fitw_cases.ref_fit_weighted) on the same positions, once, in both modes, compared
    bit for bit.
Every step is a process of its own under `timeout -k 10 --limit`; this driver checks each exit status and stops at the first step that
fails.  The text is APPENDED to --out.  There is no pass bar.
"""

from __future__ import annotations

import argparse
import hashlib
import pathlib
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
STEPS = ("kernels", "fit_stars_weighted", "numpy")
SKY, GAIN = 4.0, 2.5


def step(args) -> None:
    sys.path.insert(0, str(ROOT / "scripts"))
    sys.path.insert(0, str(ROOT))
    from star_timing import synthetic_frame

    import regularizepsf_amd as rp
    from regularizepsf_amd import _native, stars

    frame, _ = synthetic_frame(args.size, args.stars)
    variance = (np.float32(SKY) + np.maximum(frame, np.float32(0.0)) / np.float32(GAIN)).astype(np.float32)
    cus, name = _native.device_info(0)
    lines = [f"{args.step}: frame {args.size} x {args.size} float32, {args.stars} synthetic stars, box {args.box}, threshold 3.0, model cells of "
             f"{args.psf_size}, R = {args.radius:g}, variance {SKY:g} + max(pixel, 0) / {GAIN:g}; {name}, {cus} CUs; medians of {args.repeats} "
             f"after one warm-up"]
    finder = stars._Finder(frame.shape, args.box)
    finder.background_device(frame, None)
    positions = np.ascontiguousarray(finder.detect_device(3.0, 5, None)[:, :2])
    psf, counts = rp.ArrayPSFBuilder(args.psf_size).build(frame, stars=[positions])
    coordinates, values = stars.model_cube(psf)
    cells = stars.nearest_cells(positions, coordinates, args.psf_size)
    lines.append(f"  {len(positions)} positions; the model: {len(coordinates)} cells, {sum(1 for v in counts.values() if v)} of them with stars")
    if args.step == "kernels":
        model = stars._Model(values)
        t0 = time.perf_counter()
        finder.variance(variance)
        lines.append(f"  the variance frame's upload ({variance.nbytes / 2 ** 20:.0f} MiB float32, rpsf_stars_variance_host): "
                     f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
        modes = (("map", None, np.inf), (f"model, gain {GAIN:g}", SKY, GAIN), ("model, gain inf", SKY, np.inf))
        for use_mesh in (True, False):
            for fit_background in (True, False):
                times = {label: [] for label, _, _ in modes}
                plain, host = [], {label: [] for label, _, _ in modes}
                for _ in range(args.repeats + 1):
                    finder.background_device(frame, None)
                    finder.fit(model, positions, cells, args.radius, fit_background, use_mesh)
                    plain.append(finder.fit_ms())
                    for label, sky, gain in modes:
                        t0 = time.perf_counter()
                        out = finder.fit_weighted(model, positions, cells, args.radius, fit_background, use_mesh, sky, gain)
                        host[label].append((time.perf_counter() - t0) * 1e3)
                        times[label].append(finder.fit_weighted_ms())
                        if label == "map":
                            rows = out
                s8 = float(np.median(plain[1:]))
                flags = rows[:, 3].astype(int)
                lines.append(f"  background {'mesh' if use_mesh else 'none'}, {'flux and background' if fit_background else 'flux alone'}: S8 device time "
                             f"{s8:.3f} ms (min {min(plain[1:]):.3f}, max {max(plain[1:]):.3f}); " + "; ".join(
                                 f"S12 ({label}) {np.median(t[1:]):.3f} ms (min {min(t[1:]):.3f}, max {max(t[1:]):.3f}), {np.median(t[1:]) / s8:.2f} x S8, "
                                 f"fit_weighted() on the host clock {np.median(host[label][1:]):.3f} ms" for label, t in times.items())
                             + f"; flags (map) {dict(zip(*(v.tolist() for v in np.unique(flags, return_counts=True))))}; rows sha256 "
                             f"{hashlib.sha256(rows.tobytes()).hexdigest()[:16]}")
        model.close()
    finder.close()
    if args.step == "fit_stars_weighted":
        calls = (("fit_stars", lambda: rp.fit_stars(frame, [positions], psf, args.radius, box=args.box)),
                 ("fit_stars_weighted, variance map", lambda: rp.fit_stars_weighted(frame, [positions], psf, args.radius, variance=variance, box=args.box)),
                 ("fit_stars_weighted, noise model", lambda: rp.fit_stars_weighted(frame, [positions], psf, args.radius, sky_variance=SKY, gain=GAIN,
                                                                                   box=args.box)))
        for label, call in calls:
            times = []
            for _ in range(args.repeats + 1):
                t0 = time.perf_counter()
                out = call()
                times.append((time.perf_counter() - t0) * 1e3)
            good = out[0][out[0]["flags"] == 0]
            extra = ""
            if "snr" in good.dtype.names:
                extra = (f"; median snr {np.median(good['snr']):.1f}, {int((good['snr'] > 5).sum())} rows with snr > 5, median chi2_reduced "
                         f"{np.median(good['chi2_reduced']):.3f}, median flux_err / |flux| {np.median(good['flux_err'] / np.abs(good['flux'])):.2e}")
            lines.append(f"  {label}: {len(out[0])} rows, {len(good)} without a flag; end to end, ms per call: {', '.join(f'{t:.1f}' for t in times[1:])}; "
                         f"median {np.median(times[1:]):.1f}; median residual_fraction {np.median(good['residual_fraction']):.4f}{extra}")
    if args.step == "numpy":
        from tests import fitw_cases as fw

        level, rms = stars._Finder(frame.shape, args.box).background(frame, None)
        level_f = stars.filter_mesh(level, rms)[0]
        finder, model = stars._Finder(frame.shape, args.box), stars._Model(values)
        finder.background_device(frame, None)
        finder.variance(variance)
        for label, v, sky, gain in (("map", variance, None, np.inf), (f"model, gain {GAIN:g}", None, SKY, GAIN)):
            t0 = time.perf_counter()
            ref = fw.ref_fit_weighted(frame, None, args.box, level_f, values, positions, cells, args.radius, True, "mesh", v, sky, gain)
            seconds = time.perf_counter() - t0
            got = finder.fit_weighted(model, positions, cells, args.radius, True, True, sky, gain)
            differ = sum(not fw.same_bits(a, b) for a, b in zip(got, ref))
            lines.append(f"  the NumPy float64 restatement ({label}) on the same {len(positions)} positions (mesh given): {seconds * 1e3:.0f} ms on the "
                         f"host; rows that differ from S12's in any bit: {differ}")
        model.close()
        finder.close()
    print("\n".join(lines), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with args.out.open("a") as log:
        log.write("\n".join(lines) + "\n")


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--size", type=int, default=4096)
    parser.add_argument("--stars", type=int, default=10000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--box", type=int, default=64)
    parser.add_argument("--psf-size", type=int, default=32)
    parser.add_argument("--radius", type=float, default=8.0)
    parser.add_argument("--limit", type=int, default=300, help="seconds per step")
    parser.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "star_fitw_gpu.log")
    parser.add_argument("--step", choices=STEPS)
    args = parser.parse_args()
    if args.step:
        step(args)
        return
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, str(pathlib.Path(__file__).resolve()), "--step", name, "--size", str(args.size),
               "--stars", str(args.stars), "--repeats", str(args.repeats), "--box", str(args.box), "--psf-size", str(args.psf_size), "--radius",
               str(args.radius), "--out", str(args.out)]
        done = subprocess.run(cmd)
        if done.returncode != 0:
            print(f"fitw_timing: step {name} ended with status {done.returncode}; nothing more is started", flush=True)
            sys.exit(done.returncode if done.returncode > 0 else 1)


if __name__ == "__main__":
    main()
