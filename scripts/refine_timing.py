"""Time the windowed-position kernel S7 next to S5 and S6 on one large frame, at that frame's detections, and say what it buys:
    python scripts/refine_timing.py [--size 4096] [--stars 10000] [--repeats 5] [--sigma 1.5] [--limit 300] [--out FILE]

The frame is scripts/star_timing.py's, whose true star positions are known.  Medians of --repeats after one warm-up of
  * rpsf_stars_refine_ms, the device time of S7, next to rpsf_stars_shape_ms (S5) and rpsf_stars_photometry_ms (S6, radii 2, 4, 6, 8, 12),
    on one finder on the fused route, with rpsf_stars_refine on the host clock (positions up, rows down) and the distribution of niter,
  * the accuracy: the RMS and the worst distance to the truth of find_stars' positions and of the refined ones, over the detections that
    lie within 0.5 px of a true position,
  * refine_stars end to end (host clock around the call: finder created, frame uploaded, mesh kernels, S7, arrays returned),
  * the float64 NumPy restatement of the definition (tests/refine_cases.ref_refine) on the same positions, once.
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
STEPS = ("kernels", "refine_stars", "numpy")


def _distances(positions: np.ndarray, truth: np.ndarray) -> np.ndarray:
    """Per position the distance to the nearest true position."""
    from scipy.spatial import cKDTree

    return cKDTree(truth).query(positions)[0]


def step(args) -> None:
    sys.path.insert(0, str(ROOT / "scripts"))
    sys.path.insert(0, str(ROOT))
    from star_timing import synthetic_frame

    import regularizepsf_amd as rp
    from regularizepsf_amd import _native, stars

    frame, truth = synthetic_frame(args.size, args.stars)
    cus, name = _native.device_info(0)
    lines = [f"{args.step}: frame {args.size} x {args.size} float32, {args.stars} synthetic stars, box {args.box}, threshold 3.0, sigma "
             f"{args.sigma}, max_iter 16, eps 1e-4, max_shift 2.0; {name}, {cus} CUs; medians of {args.repeats} after one warm-up"]
    finder = stars._Finder(frame.shape, args.box)
    finder.background_device(frame, None)
    rows = finder.detect_device(3.0, 5, None)
    positions = np.ascontiguousarray(rows[:, :2])
    if args.step == "kernels":
        radii = np.array([2.0, 4.0, 6.0, 8.0, 12.0])
        for use_mesh in (True, False):
            times = []
            for _ in range(args.repeats + 1):
                finder.background_device(frame, None)
                finder.detect_device(3.0, 5, None)
                finder.measure()
                finder.photometry(positions, radii, 5, use_mesh)
                t0 = time.perf_counter()
                out = finder.refine(positions, args.sigma, 16, 1e-4, 2.0, use_mesh)
                times.append((finder.refine_ms(), finder.shape_ms(), finder.photometry_ms(), (time.perf_counter() - t0) * 1e3))
            t = np.array(times[1:])
            lines.append(f"  background {'mesh' if use_mesh else 'none'}: {len(positions)} positions; S7 device time {np.median(t[:, 0]):.3f} ms (min "
                         f"{t[:, 0].min():.3f}, max {t[:, 0].max():.3f}); S5 {np.median(t[:, 1]):.3f} ms; S6 {np.median(t[:, 2]):.3f} ms; refine() on "
                         f"the host clock (positions up, rows down) {np.median(t[:, 3]):.3f} ms; rows sha256 "
                         f"{hashlib.sha256(out.tobytes()).hexdigest()[:16]}")
            niter, flags = out[:, 5].astype(int), out[:, 6].astype(int)
            lines.append(f"    niter: {dict(zip(*(v.tolist() for v in np.unique(niter, return_counts=True))))}; flags: "
                         f"{dict(zip(*(v.tolist() for v in np.unique(flags, return_counts=True))))}")
            if use_mesh:
                forced = []
                for _ in range(args.repeats + 1):
                    finder.refine(positions, args.sigma, 0, 1e-4, 2.0, True)
                    forced.append(finder.refine_ms())
                lines.append(f"    max_iter = 0 (one walk per position): S7 device time {np.median(forced[1:]):.3f} ms")
                refined = stars.refined_positions(positions, out)
                before, after = _distances(positions, truth), _distances(refined, truth)
                matched = before <= 0.5
                lines.append(f"    accuracy over the {int(matched.sum())} of {len(positions)} detections within 0.5 px of a true position: find_stars "
                             f"RMS {np.sqrt(np.mean(before[matched] ** 2)):.4f} px, worst {before[matched].max():.4f} px; refined RMS "
                             f"{np.sqrt(np.mean(after[matched] ** 2)):.4f} px, worst {after[matched].max():.4f} px; medians "
                             f"{np.median(before[matched]):.4f} and {np.median(after[matched]):.4f} px; "
                             f"{int(((flags & 3) != 0).sum())} detections kept their detected position")
    finder.close()
    if args.step == "refine_stars":
        for background in ("mesh", "none"):
            times = []
            for _ in range(args.repeats + 1):
                t0 = time.perf_counter()
                out = rp.refine_stars(frame, [positions], args.sigma, box=args.box, background=background)[0]
                times.append((time.perf_counter() - t0) * 1e3)
            lines.append(f"  background {background}: {len(out)} rows; end to end, ms per call: {', '.join(f'{t:.1f}' for t in times[1:])}; median "
                         f"{np.median(times[1:]):.1f}; converged {int(out['converged'].sum())}; median corrected sqrt(rr) "
                         f"{np.nanmedian(np.sqrt(out['rr'])):.3f}, median coverage {np.median(out['coverage']):.3f}")
    if args.step == "numpy":
        from tests import refine_cases as rc

        level, rms = stars._Finder(frame.shape, args.box).background(frame, None)
        level_f = stars.filter_mesh(level, rms)[0]
        t0 = time.perf_counter()
        ref = rc.ref_refine(frame, None, args.box, level_f, positions, args.sigma, "mesh")
        seconds = time.perf_counter() - t0
        finder = stars._Finder(frame.shape, args.box)
        finder.background_device(frame, None)
        got = finder.refine(positions, args.sigma)
        finder.close()
        same = np.array_equal(got[:, 5:7], ref["rows"][:, 5:7])
        lines.append(f"  the NumPy float64 restatement on the same {len(positions)} positions (mesh given): {seconds * 1e3:.0f} ms on the host; niter "
                     f"and flags equal to S7's: {bool(same)}; worst distance between the two positions "
                     f"{float(np.max(np.hypot(*(got[:, 2:4] - ref['rows'][:, 2:4]).T))):.2e} px")
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
    parser.add_argument("--sigma", type=float, default=1.5)
    parser.add_argument("--limit", type=int, default=300, help="seconds per step")
    parser.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "star_refine_gpu.log")
    parser.add_argument("--step", choices=STEPS)
    args = parser.parse_args()
    if args.step:
        step(args)
        return
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, str(pathlib.Path(__file__).resolve()), "--step", name, "--size", str(args.size),
               "--stars", str(args.stars), "--repeats", str(args.repeats), "--box", str(args.box), "--sigma", str(args.sigma), "--out",
               str(args.out)]
        done = subprocess.run(cmd)
        if done.returncode != 0:
            print(f"refine_timing: step {name} ended with status {done.returncode}; nothing more is started", flush=True)
            sys.exit(done.returncode if done.returncode > 0 else 1)


if __name__ == "__main__":
    main()
