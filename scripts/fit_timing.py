"""Time the model-fit kernel S8 next to S6 and S7 on one large frame, at that frame's detections, with a model built from the same frame:
    python scripts/fit_timing.py [--size 4096] [--stars 10000] [--repeats 5] [--psf-size 32] [--radius 8] [--limit 300] [--out FILE]

The frame is scripts/star_timing.py's.  The stars are find_stars' on it, the model is ArrayPSFBuilder(psf_size).build(frame,
stars=those).  Medians of --repeats after one warm-up of
  * rpsf_stars_fit_ms, the device time of S8, with and without a fitted background and with the mesh and without, next to
    rpsf_stars_photometry_ms (S6, radii 2, 4, 6, 8, 12) and rpsf_stars_refine_ms (S7, sigma 1.5) on the same finder and positions, with
    rpsf_stars_fit on the host clock (positions and cells up, rows down), the upload of the model, and the distribution of the flags,
  * fit_stars end to end (host clock around the call: cell choice, finder and model created, frame uploaded, mesh kernels, S8, arrays
    returned) and cell_fit_summary on its result,
  * the float64 NumPy restatement of the definition (tests/fit_cases.ref_fit) on the same positions, once, compared bit for bit.
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
STEPS = ("kernels", "fit_stars", "numpy")


def step(args) -> None:
    sys.path.insert(0, str(ROOT / "scripts"))
    sys.path.insert(0, str(ROOT))
    from star_timing import synthetic_frame

    import regularizepsf_amd as rp
    from regularizepsf_amd import _native, stars

    frame, _ = synthetic_frame(args.size, args.stars)
    cus, name = _native.device_info(0)
    lines = [f"{args.step}: frame {args.size} x {args.size} float32, {args.stars} synthetic stars, box {args.box}, threshold 3.0, model cells of "
             f"{args.psf_size}, R = {args.radius:g}; {name}, {cus} CUs; medians of {args.repeats} after one warm-up"]
    finder = stars._Finder(frame.shape, args.box)
    finder.background_device(frame, None)
    positions = np.ascontiguousarray(finder.detect_device(3.0, 5, None)[:, :2])
    t0 = time.perf_counter()
    psf, counts = rp.ArrayPSFBuilder(args.psf_size).build(frame, stars=[positions])
    build_ms = (time.perf_counter() - t0) * 1e3
    coordinates, values = stars.model_cube(psf)
    t0 = time.perf_counter()
    cells = stars.nearest_cells(positions, coordinates, args.psf_size)
    choice_ms = (time.perf_counter() - t0) * 1e3
    lines.append(f"  {len(positions)} positions; the model: {len(coordinates)} cells, {sum(1 for v in counts.values() if v)} of them with stars, "
                 f"built in {build_ms:.0f} ms; the cell choice on the host {choice_ms:.1f} ms")
    if args.step == "kernels":
        t0 = time.perf_counter()
        model = stars._Model(values)
        lines.append(f"  the model's upload ({values.nbytes / 2 ** 20:.1f} MiB, once per model): {(time.perf_counter() - t0) * 1e3:.1f} ms")
        radii = np.array([2.0, 4.0, 6.0, 8.0, 12.0])
        for use_mesh in (True, False):
            for fit_background in (True, False):
                times = []
                for _ in range(args.repeats + 1):
                    finder.background_device(frame, None)
                    finder.photometry(positions, radii, 5, use_mesh)
                    finder.refine(positions, 1.5, 16, 1e-4, 2.0, use_mesh)
                    t0 = time.perf_counter()
                    out = finder.fit(model, positions, cells, args.radius, fit_background, use_mesh)
                    times.append((finder.fit_ms(), finder.photometry_ms(), finder.refine_ms(), (time.perf_counter() - t0) * 1e3))
                t = np.array(times[1:])
                flags = out[:, 3].astype(int)
                lines.append(f"  background {'mesh' if use_mesh else 'none'}, {'flux and background' if fit_background else 'flux alone'}: S8 device time "
                             f"{np.median(t[:, 0]):.3f} ms (min {t[:, 0].min():.3f}, max {t[:, 0].max():.3f}); S6 {np.median(t[:, 1]):.3f} ms; S7 "
                             f"{np.median(t[:, 2]):.3f} ms; fit() on the host clock (positions and cells up, rows down) {np.median(t[:, 3]):.3f} ms; "
                             f"flags {dict(zip(*(v.tolist() for v in np.unique(flags, return_counts=True))))}; rows sha256 "
                             f"{hashlib.sha256(out.tobytes()).hexdigest()[:16]}")
        model.close()
    finder.close()
    if args.step == "fit_stars":
        for background in ("mesh", "none"):
            times = []
            for _ in range(args.repeats + 1):
                t0 = time.perf_counter()
                out = rp.fit_stars(frame, [positions], psf, args.radius, box=args.box, background=background)
                times.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            summary = rp.cell_fit_summary(out, psf)
            summary_ms = (time.perf_counter() - t0) * 1e3
            good = out[0][out[0]["flags"] == 0]
            lines.append(f"  background {background}: {len(out[0])} rows, {len(good)} without a flag; end to end, ms per call: "
                         f"{', '.join(f'{t:.1f}' for t in times[1:])}; median {np.median(times[1:]):.1f}; median residual_fraction "
                         f"{np.median(good['residual_fraction']):.4f}, median rms / |flux| {np.median(good['rms'] / np.abs(good['flux'])):.2e}, median "
                         f"coverage {np.median(good['coverage']):.3f}; cell_fit_summary {summary_ms:.1f} ms, {int((summary['count'] > 0).sum())} "
                         f"cells with fitted stars, the worst cell's median residual_fraction {np.nanmax(summary['residual_fraction']):.4f}")
    if args.step == "numpy":
        from tests import fit_cases as fc

        level, rms = stars._Finder(frame.shape, args.box).background(frame, None)
        level_f = stars.filter_mesh(level, rms)[0]
        t0 = time.perf_counter()
        ref = fc.ref_fit(frame, None, args.box, level_f, values, positions, cells, args.radius, True, "mesh")
        seconds = time.perf_counter() - t0
        finder, model = stars._Finder(frame.shape, args.box), stars._Model(values)
        finder.background_device(frame, None)
        got = finder.fit(model, positions, cells, args.radius, True, True)
        model.close()
        finder.close()
        differ = sum(not fc.same_bits(a, b) for a, b in zip(got, ref))
        lines.append(f"  the NumPy float64 restatement on the same {len(positions)} positions (mesh given): {seconds * 1e3:.0f} ms on the host; rows "
                     f"that differ from S8's in any bit: {differ}")
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
    parser.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "star_fit_gpu.log")
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
            print(f"fit_timing: step {name} ended with status {done.returncode}; nothing more is started", flush=True)
            sys.exit(done.returncode if done.returncode > 0 else 1)


if __name__ == "__main__":
    main()
