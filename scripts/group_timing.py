"""Time the group-fit kernel S11 (with the S8 beside it) next to S8 alone on one large frame, at that frame's deblended detections, with a
model built from the same frame:
    python scripts/group_timing.py [--size 4096] [--stars 10000] [--repeats 5] [--psf-size 32] [--radius 8] [--limit 300] [--out FILE]

The frame is scripts/star_timing.py's.  The stars are the detections of the deblend option on it, the model is
ArrayPSFBuilder(psf_size).build(frame, stars=those).  Medians of --repeats after one warm-up of
  * rpsf_stars_fit_groups_ms, the device time of S11 and the S8 launch for the stars that are alone, next to rpsf_stars_fit_ms, S8 alone
    on the same positions and the same finder, with fit_groups() on the host clock (grouping, positions up, rows down), the grouping
    alone on the host, the histogram of group sizes, and S11's time per grouped star next to g times S8's per star - with max_group = 1
    (everything through S8) and a run of the pairs alone to say which part of S11 the time goes to,
  * fit_groups end to end (host clock around the call) next to fit_stars,
  * the float64 NumPy restatement (tests/group_cases.ref_fit_groups) on the first --check positions, once, compared bit for bit.
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
STEPS = ("kernels", "fit_groups", "numpy")


def step(args) -> None:
    sys.path.insert(0, str(ROOT / "scripts"))
    sys.path.insert(0, str(ROOT))
    from star_timing import synthetic_frame

    import regularizepsf_amd as rp
    from regularizepsf_amd import _native, stars

    frame, _ = synthetic_frame(args.size, args.stars)
    cus, name = _native.device_info(0)
    lines = [f"{args.step}: frame {args.size} x {args.size} float32, {args.stars} synthetic stars, box {args.box}, threshold 3.0, deblend on, model "
             f"cells of {args.psf_size}, R = {args.radius:g}, link = 2 R; {name}, {cus} CUs; medians of {args.repeats} after one warm-up"]
    finder = stars._Finder(frame.shape, args.box)
    finder.set_deblend(True)
    finder.background_device(frame, None)
    positions = np.ascontiguousarray(finder.detect_device(3.0, 5, None)[:, :2])
    psf, counts = rp.ArrayPSFBuilder(args.psf_size).build(frame, stars=[positions])
    coordinates, values = stars.model_cube(psf)
    cells = stars.nearest_cells(positions, coordinates, args.psf_size)
    lines.append(f"  {len(positions)} positions; the model: {len(coordinates)} cells, {sum(1 for v in counts.values() if v)} of them with stars")
    if args.step == "kernels":
        model = stars._Model(values)
        t0 = time.perf_counter()
        groups = stars.star_groups(positions, 2.0 * args.radius)
        grouping_ms = (time.perf_counter() - t0) * 1e3
        sizes = np.bincount(groups["group_size"][groups["group"] == np.arange(len(groups))])
        lines.append(f"  the grouping alone on the host (every star eligible): {grouping_ms:.2f} ms; components by size 1, 2, ...: {sizes[1:].tolist()}; "
                     f"{int(groups['crowded'].sum())} stars in components of more than 8 (fitted alone)")
        for use_mesh in (True, False):
            for fit_background in (True, False):
                times = []
                for _ in range(args.repeats + 1):
                    finder.background_device(frame, None)
                    finder.fit(model, positions, cells, args.radius, fit_background, use_mesh)
                    t0 = time.perf_counter()
                    out = finder.fit_groups(model, positions, cells, args.radius, fit_background, use_mesh)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    both = finder.fit_groups_ms()
                    finder.fit_groups(model, positions, cells, args.radius, fit_background, use_mesh, None, 1)  # every star through S8
                    times.append((both, finder.fit_ms(), host_ms, finder.fit_groups_ms()))
                t = np.array(times[1:])
                size = out[:, 21].astype(int)
                fitted = (size >= 2) & (size <= 8)
                stars_by_size = np.bincount(size[fitted], minlength=9)[2:9]
                flags = out[:, 3].astype(int)
                lines.append(f"  background {'mesh' if use_mesh else 'none'}, {'flux and background' if fit_background else 'flux alone'}: S11 + S8 "
                             f"under fit_groups {np.median(t[:, 0]):.3f} ms (min {t[:, 0].min():.3f}, max {t[:, 0].max():.3f}); S8 alone under fit "
                             f"{np.median(t[:, 1]):.3f} ms; fit_groups with max_group = 1 (S8 alone) {np.median(t[:, 3]):.3f} ms; fit_groups() on "
                             f"the host clock {np.median(t[:, 2]):.3f} ms; {int(fitted.sum())} stars in groups of 2 ... 8 (stars by group size: "
                             f"{stars_by_size.tolist()}), {int((~fitted).sum())} alone; flags {dict(zip(*(v.tolist() for v in np.unique(flags, return_counts=True))))}; "
                             f"rows sha256 {hashlib.sha256(out.tobytes()).hexdigest()[:16]}")
        # which part: the grouped stars alone through S11 (no S8 launch beside it), and the same stars through S8
        finder.background_device(frame, None)
        out = finder.fit_groups(model, positions, cells, args.radius, True, True)
        size = out[:, 21].astype(int)
        for g in range(2, 9):
            pick = np.flatnonzero(size == g)
            if len(pick) == 0:
                continue
            t11, t8 = [], []
            for _ in range(args.repeats + 1):
                finder.fit_groups(model, positions[pick], cells[pick], args.radius, True, True)
                t11.append(finder.fit_groups_ms())
                finder.fit(model, positions[pick], cells[pick], args.radius, True, True)
                t8.append(finder.fit_ms())
            a, b = float(np.median(t11[1:])), float(np.median(t8[1:]))
            lines.append(f"  groups of {g} alone: {len(pick)} stars in {len(pick) // g} groups: S11 {a:.3f} ms = {1e6 * a / len(pick):.0f} ns per star; S8 on "
                         f"the same stars {b:.3f} ms = {1e6 * b / len(pick):.0f} ns per star; S11 per star / (g x S8 per star) = {a / (g * b):.2f}")
        model.close()
    finder.close()
    if args.step == "fit_groups":
        for background in ("mesh", "none"):
            times, single = [], []
            for _ in range(args.repeats + 1):
                t0 = time.perf_counter()
                out = rp.fit_groups(frame, [positions], psf, args.radius, box=args.box, background=background)
                times.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                alone = rp.fit_stars(frame, [positions], psf, args.radius, box=args.box, background=background)
                single.append((time.perf_counter() - t0) * 1e3)
            good = out[0][out[0]["flags"] == 0]
            blended = (out[0]["group_size"] >= 2) & ~out[0]["crowded"] & (out[0]["flags"] == 0) & (alone[0]["flags"] == 0)
            lines.append(f"  background {background}: {len(out[0])} rows, {len(good)} without a flag; fit_groups end to end, ms per call: "
                         f"{', '.join(f'{t:.1f}' for t in times[1:])}; median {np.median(times[1:]):.1f}; fit_stars {np.median(single[1:]):.1f}; in groups: "
                         f"median residual_fraction {np.median(out[0]['residual_fraction'][blended]):.4f} (fit_stars on the same stars "
                         f"{np.median(alone[0]['residual_fraction'][blended]):.4f}), median flux / fit_stars' flux "
                         f"{np.median(out[0]['flux'][blended] / alone[0]['flux'][blended]):.4f}")
    if args.step == "numpy":
        from tests import fit_cases as fc
        from tests import group_cases as gc

        level, rms = stars._Finder(frame.shape, args.box).background(frame, None)
        level_f = stars.filter_mesh(level, rms)[0]
        p, k = positions[:args.check], cells[:args.check]
        t0 = time.perf_counter()
        ref = gc.ref_fit_groups(frame, None, args.box, level_f, values, p, k, args.radius, True, "mesh")
        seconds = time.perf_counter() - t0
        finder, model = stars._Finder(frame.shape, args.box), stars._Model(values)
        finder.background_device(frame, None)
        got = finder.fit_groups(model, p, k, args.radius, True, True)
        model.close()
        finder.close()
        differ = sum(not fc.same_bits(a, b) for a, b in zip(got, ref))
        lines.append(f"  the NumPy float64 restatement on the first {len(p)} positions (mesh given): {seconds * 1e3:.0f} ms on the host; "
                     f"{int(((ref[:, 21] >= 2) & (ref[:, 21] <= 8)).sum())} of them in groups; rows that differ from the kernels' in any bit: {differ}")
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
    parser.add_argument("--check", type=int, default=1500, help="positions of the NumPy comparison")
    parser.add_argument("--limit", type=int, default=300, help="seconds per step")
    parser.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "star_group_gpu.log")
    parser.add_argument("--step", choices=STEPS)
    args = parser.parse_args()
    if args.step:
        step(args)
        return
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, str(pathlib.Path(__file__).resolve()), "--step", name, "--size", str(args.size),
               "--stars", str(args.stars), "--repeats", str(args.repeats), "--box", str(args.box), "--psf-size", str(args.psf_size), "--radius",
               str(args.radius), "--check", str(args.check), "--out", str(args.out)]
        done = subprocess.run(cmd)
        if done.returncode != 0:
            print(f"group_timing: step {name} ended with status {done.returncode}; nothing more is started", flush=True)
            sys.exit(done.returncode if done.returncode > 0 else 1)


if __name__ == "__main__":
    main()
