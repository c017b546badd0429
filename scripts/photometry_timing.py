"""Time the aperture kernel S6 next to the shape kernel S5 on one large frame, at that frame's detections:
    python scripts/photometry_timing.py [--size 4096] [--stars 10000] [--repeats 5] [--radii 2,4,6,8,12] [--subpix 5] [--limit 300] [--out FILE]

The frame is scripts/star_timing.py's.  Medians of --repeats after one warm-up of
  * rpsf_stars_photometry_ms, the device time of S6, next to rpsf_stars_shape_ms (S5) and S4's from rpsf_stars_kernel_ms, on one finder
    on the fused route (background_device, detect_device, measure, photometry), with background="mesh" and "none",
  * star_photometry end to end (host clock around the call: finder created, frame uploaded, mesh kernels, S6, arrays returned),
  * the float64 NumPy restatement of the definition (tests/photometry_cases.ref_photometry) on the same positions, once.
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
STEPS = ("kernels", "star_photometry", "numpy")


def step(args) -> None:
    sys.path.insert(0, str(ROOT / "scripts"))
    sys.path.insert(0, str(ROOT))
    from star_timing import synthetic_frame

    import regularizepsf_amd as rp
    from regularizepsf_amd import _native, stars

    frame, _ = synthetic_frame(args.size, args.stars)
    radii = np.array([float(r) for r in args.radii.split(",")])
    cus, name = _native.device_info(0)
    lines = [f"{args.step}: frame {args.size} x {args.size} float32, {args.stars} synthetic stars, box {args.box}, threshold 3.0, radii "
             f"{radii.tolist()}, subpix {args.subpix}; {name}, {cus} CUs; medians of {args.repeats} after one warm-up"]
    finder = stars._Finder(frame.shape, args.box)
    finder.background_device(frame, None)
    rows = finder.detect_device(3.0, 5, None)
    positions = np.ascontiguousarray(rows[:, :2])
    if args.step == "kernels":
        for use_mesh in (True, False):
            times = []
            for _ in range(args.repeats + 1):
                finder.background_device(frame, None)
                finder.detect_device(3.0, 5, None)
                finder.measure()
                t0 = time.perf_counter()
                out = finder.photometry(positions, radii, args.subpix, use_mesh)
                times.append((finder.photometry_ms(), finder.shape_ms(), finder.kernel_ms()[3], (time.perf_counter() - t0) * 1e3))
            t = np.array(times[1:])
            lines.append(f"  background {'mesh' if use_mesh else 'none'}: {len(positions)} positions; S6 device time {np.median(t[:, 0]):.3f} ms (min "
                         f"{t[:, 0].min():.3f}, max {t[:, 0].max():.3f}); S5 {np.median(t[:, 1]):.3f} ms; S4 {np.median(t[:, 2]):.3f} ms; photometry() on "
                         f"the host clock (positions up, rows down) {np.median(t[:, 3]):.3f} ms; rows sha256 "
                         f"{hashlib.sha256(out.tobytes()).hexdigest()[:16]}")
        lines.append(f"  the mesh launches a background='none' call still makes: S1 {finder.kernel_ms()[0]:.3f} ms, S1b {finder.mesh_ms():.3f} ms")
    finder.close()
    if args.step == "star_photometry":
        for background in ("mesh", "none"):
            times = []
            for _ in range(args.repeats + 1):
                t0 = time.perf_counter()
                out = rp.star_photometry(frame, [positions], radii, box=args.box, subpix=args.subpix, background=background)[0]
                times.append((time.perf_counter() - t0) * 1e3)
            lines.append(f"  background {background}: {len(out)} rows; end to end, ms per call: {', '.join(f'{t:.1f}' for t in times[1:])}; median "
                         f"{np.median(times[1:]):.1f}; median half-light radius {np.nanmedian(out['half_light_radius']):.3f}, median coverage "
                         f"{np.median(out['coverage'][:, -1]):.3f}")
    if args.step == "numpy":
        from tests import photometry_cases as pc

        level, rms = stars._Finder(frame.shape, args.box).background(frame, None)
        level_f = stars.filter_mesh(level, rms)[0]
        t0 = time.perf_counter()
        ref = pc.ref_photometry(frame, None, args.box, level_f, positions, radii, args.subpix, "mesh")
        seconds = time.perf_counter() - t0
        finder = stars._Finder(frame.shape, args.box)
        finder.background_device(frame, None)
        got = finder.photometry(positions, radii, args.subpix, True)
        finder.close()
        m = len(radii)
        counts = slice(2 + m, 2 + 3 * m)
        lines.append(f"  the NumPy float64 restatement on the same {len(positions)} positions (mesh given): {seconds * 1e3:.0f} ms on the host; counts "
                     f"equal to S6's: {bool(np.array_equal(got[:, counts], ref['rows'][:, counts]))}; worst flux error / bound "
                     f"{float(np.max(np.abs(got[:, 2:2 + m] - ref['rows'][:, 2:2 + m]) / ref['bounds'][:, :m])):.2e}")
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
    parser.add_argument("--radii", default="2,4,6,8,12")
    parser.add_argument("--subpix", type=int, default=5)
    parser.add_argument("--limit", type=int, default=300, help="seconds per step")
    parser.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "star_photometry_gpu.log")
    parser.add_argument("--step", choices=STEPS)
    args = parser.parse_args()
    if args.step:
        step(args)
        return
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, str(pathlib.Path(__file__).resolve()), "--step", name, "--size", str(args.size),
               "--stars", str(args.stars), "--repeats", str(args.repeats), "--box", str(args.box), "--radii", args.radii, "--subpix",
               str(args.subpix), "--out", str(args.out)]
        done = subprocess.run(cmd)
        if done.returncode != 0:
            print(f"photometry_timing: step {name} ended with status {done.returncode}; nothing more is started", flush=True)
            sys.exit(done.returncode if done.returncode > 0 else 1)


if __name__ == "__main__":
    main()
