"""Time the position-fit kernel S9 next to S7 and S8 on one large frame, at that frame's detections, with a model built from the same
frame, and say how good the fitted positions are:
    python scripts/fitpos_timing.py [--size 4096] [--stars 10000] [--repeats 5] [--psf-size 32] [--radius 8] [--limit 300] [--out FILE]

The frame is scripts/star_timing.py's, whose true positions are known.  The stars are find_stars' on it, the model is
ArrayPSFBuilder(psf_size).build(frame, stars=those).
  * kernels: medians of --repeats after one warm-up of rpsf_stars_fit_positions_ms (S9 and the S8 behind it), rpsf_stars_refine_ms (S7,
    sigma 1.5) and rpsf_stars_fit_ms (S8) in the same run, fit_positions() on the host clock, the histogram of niter and the flag counts;
  * positions: over the detections within 0.5 px of a true star, the median, RMS and worst distance to the truth of find_stars',
    refine_stars' (sigma 1.5) and fit_positions' positions;
  * loop: the median residual_fraction of fit_stars before and after one round build -> fit_positions -> build.
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
STEPS = ("kernels", "positions", "loop")


def distances(found: np.ndarray, truth: np.ndarray, within: float = 0.5) -> tuple[np.ndarray, np.ndarray]:
    """Per found position the distance to the nearest true star, and which of them lie within `within` px."""
    from scipy.spatial import cKDTree

    d = cKDTree(truth).query(found)[0]
    return d, d <= within


def step(args) -> None:
    sys.path.insert(0, str(ROOT / "scripts"))
    sys.path.insert(0, str(ROOT))
    from star_timing import synthetic_frame

    import regularizepsf_amd as rp
    from regularizepsf_amd import _native, stars

    frame, truth = synthetic_frame(args.size, args.stars)
    cus, name = _native.device_info(0)
    lines = [f"{args.step}: frame {args.size} x {args.size} float32, {args.stars} synthetic stars, box {args.box}, threshold 3.0, model cells of "
             f"{args.psf_size}, R = {args.radius:g}, max_iter 16, eps 1e-4, max_shift 2, max_step 0.5; {name}, {cus} CUs; medians of "
             f"{args.repeats} after one warm-up"]
    finder = stars._Finder(frame.shape, args.box)
    finder.background_device(frame, None)
    positions = np.ascontiguousarray(finder.detect_device(3.0, 5, None)[:, :2])
    psf, counts = rp.ArrayPSFBuilder(args.psf_size).build(frame, stars=[positions])
    coordinates, values = stars.model_cube(psf)
    cells = stars.nearest_cells(positions, coordinates, args.psf_size)
    lines.append(f"  {len(positions)} positions; the model: {len(coordinates)} cells, {sum(1 for v in counts.values() if v)} of them with stars")
    if args.step == "kernels":
        model = stars._Model(values)
        for use_mesh in (True, False):
            for fit_background in (True, False):
                times = []
                for _ in range(args.repeats + 1):
                    finder.background_device(frame, None)
                    finder.refine(positions, 1.5, 16, 1e-4, 2.0, use_mesh)
                    finder.fit(model, positions, cells, args.radius, fit_background, use_mesh)
                    t0 = time.perf_counter()
                    steps, fits = finder.fit_positions(model, positions, cells, args.radius, fit_background, 16, 1e-4, 2.0, 0.5, use_mesh)
                    times.append((finder.fit_positions_ms(), finder.refine_ms(), finder.fit_ms(), (time.perf_counter() - t0) * 1e3))
                t = np.array(times[1:])
                flags, niter = steps[:, 5].astype(int), steps[:, 4].astype(int)
                lines.append(f"  background {'mesh' if use_mesh else 'none'}, {'flux and background' if fit_background else 'flux alone'}: S9 + S8 device "
                             f"time {np.median(t[:, 0]):.3f} ms (min {t[:, 0].min():.3f}, max {t[:, 0].max():.3f}); S7 {np.median(t[:, 1]):.3f} ms; S8 "
                             f"{np.median(t[:, 2]):.3f} ms; fit_positions() on the host clock (positions and cells up, rows down) "
                             f"{np.median(t[:, 3]):.3f} ms")
                lines.append(f"    flags {dict(zip(*(v.tolist() for v in np.unique(flags, return_counts=True))))}; niter "
                             f"{dict(zip(*(v.tolist() for v in np.unique(niter, return_counts=True))))}; S8's flags "
                             f"{dict(zip(*(v.tolist() for v in np.unique(fits[:, 3].astype(int), return_counts=True))))}; rows sha256 "
                             f"{hashlib.sha256(steps.tobytes() + fits.tobytes()).hexdigest()[:16]}")
        model.close()
    finder.close()
    if args.step == "positions":
        refined = rp.refine_stars(frame, [positions], 1.5, box=args.box)[0]
        fitted = rp.fit_positions(frame, [positions], psf, args.radius, box=args.box)[0]
        _, near = distances(positions, truth)
        lines.append(f"  {int(near.sum())} of {len(positions)} detections lie within 0.5 px of a true star; over those, the distance to the truth in px:")
        for what, got, good in (("find_stars", positions, np.ones(len(positions), bool)),
                                ("refine_stars, sigma 1.5", np.stack([refined["row"], refined["col"]], axis=-1), refined["converged"]),
                                ("fit_positions", np.stack([fitted["row"], fitted["col"]], axis=-1), fitted["converged"])):
            d = distances(got, truth, np.inf)[0]
            for label, keep in (("all of them", near), ("the converged", near & good)):
                lines.append(f"    {what:24s} {label:14s} {int(keep.sum()):5d} stars: median {np.median(d[keep]):.4f}, RMS "
                             f"{np.sqrt(np.mean(d[keep] ** 2)):.4f}, worst {d[keep].max():.4f}")
        lines.append(f"    fit_positions: flags {dict(zip(*(v.tolist() for v in np.unique(fitted['flags'], return_counts=True))))}, niter "
                     f"{dict(zip(*(v.tolist() for v in np.unique(fitted['niter'], return_counts=True))))}")
    if args.step == "loop":
        before = rp.fit_stars(frame, [positions], psf, args.radius, box=args.box)[0]
        fitted = rp.fit_positions(frame, [positions], psf, args.radius, box=args.box)
        keep = fitted[0][fitted[0]["converged"]]
        rebuilt, _ = rp.ArrayPSFBuilder(args.psf_size).build(frame, stars=[keep])
        after = rp.fit_stars(frame, [keep], rebuilt, args.radius, box=args.box)[0]
        again = rp.fit_positions(frame, [keep], rebuilt, args.radius, box=args.box)[0]
        median = lambda rows: float(np.median(rows["residual_fraction"][rows["flags"] == 0]))  # noqa: E731
        lines.append(f"  median residual_fraction of fit_stars: {median(before):.4f} at find_stars' positions with the model built there ({len(before)} "
                     f"stars); {float(np.median(fitted[0]['residual_fraction'][fitted[0]['fit_flags'] == 0])):.4f} at the fitted positions with the same "
                     f"model; {median(after):.4f} after one round build -> fit_positions -> build at the {len(keep)} converged stars, with the rebuilt "
                     f"model; {float(np.median(again['residual_fraction'][again['fit_flags'] == 0])):.4f} after fitting those once more with it "
                     f"({int(again['converged'].sum())} converged)")
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
    parser.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "star_fitpos_gpu.log")
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
            print(f"fitpos_timing: step {name} ended with status {done.returncode}; nothing more is started", flush=True)
            sys.exit(done.returncode if done.returncode > 0 else 1)


if __name__ == "__main__":
    main()
