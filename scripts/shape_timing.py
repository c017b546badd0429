"""Time the shape kernel S5 and star_catalog next to find_stars on one large frame:
    python scripts/shape_timing.py [--size 4096] [--stars 10000] [--repeats 5] [--tree DIR] [--label TEXT] [--limit 300] [--out FILE]

The frame is scripts/star_timing.py's.  With the deblend option off and on, medians of --repeats after one warm-up of
  * rpsf_stars_shape_ms, the device time of S5, on an existing finder (next to S4's from rpsf_stars_kernel_ms),
  * find_stars end to end and star_catalog end to end (host clock around the call: finder created, frame uploaded, arrays returned).
--tree DIR imports the package from another checkout (built there), so that find_stars of the parent commit is timed in the same
session; a tree without star_catalog reports find_stars alone.  Every step is a process of its own under `timeout -k 10 --limit`; this
driver checks each exit status and stops at the first step that fails.  The text is APPENDED to --out.  There is no pass bar.
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
STEPS = ("find_stars", "star_catalog", "shape_ms")


def step(args) -> None:
    """One step in this process: both settings of the option."""
    sys.path.insert(0, str(ROOT / "scripts"))
    from star_timing import synthetic_frame

    import regularizepsf_amd as rp
    from regularizepsf_amd import _native, stars

    frame, _ = synthetic_frame(args.size, args.stars)
    cus, name = _native.device_info(0)
    lines = [f"[{args.label}] {args.step}: frame {args.size} x {args.size} float32, {args.stars} synthetic stars, box {args.box}, threshold 3.0; "
             f"{name}, {cus} CUs; medians of {args.repeats} after one warm-up"]
    for on in (False, True):
        what = f"  deblend {'on' if on else 'off'}:"
        if args.step == "shape_ms":
            finder = stars._Finder(frame.shape, args.box)
            finder.set_deblend(on)
            times = []
            for _ in range(args.repeats + 1):
                rows = stars.frame_stars(finder, frame, None, 3.0, 5, None)
                t0 = time.perf_counter()
                shapes = finder.measure()
                times.append((finder.shape_ms(), finder.kernel_ms()[3], (time.perf_counter() - t0) * 1e3))
            finder.close()
            t = np.array(times[1:])
            lines.append(f"{what} {len(rows)} rows; S5 device time {np.median(t[:, 0]):.3f} ms (min {t[:, 0].min():.3f}, max {t[:, 0].max():.3f}); "
                         f"S4 {np.median(t[:, 1]):.3f} ms; measure() on the host clock (descriptors up, rows down) {np.median(t[:, 2]):.3f} ms; "
                         f"shapes sha256 {hashlib.sha256(shapes.tobytes()).hexdigest()[:16]}")
            continue
        call = rp.find_stars if args.step == "find_stars" else rp.star_catalog
        times = []
        for _ in range(args.repeats + 1):
            t0 = time.perf_counter()
            out = call(frame, box=args.box, deblend=on)[0]
            times.append((time.perf_counter() - t0) * 1e3)
        digest = hashlib.sha256((out if args.step == "find_stars" else np.stack([out["row"], out["col"]], axis=-1)).tobytes()).hexdigest()[:16]
        lines.append(f"{what} {len(out)} rows; end to end, ms per call: {', '.join(f'{t:.1f}' for t in times[1:])}; median "
                     f"{np.median(times[1:]):.1f}; positions sha256 {digest}")
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
    parser.add_argument("--tree", type=pathlib.Path, default=ROOT)
    parser.add_argument("--label", default="this tree")
    parser.add_argument("--limit", type=int, default=300, help="seconds per step")
    parser.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "star_shapes_gpu.log")
    parser.add_argument("--step", choices=STEPS)
    args = parser.parse_args()
    sys.path.insert(0, str(args.tree.resolve()))
    if args.step:
        step(args)
        return
    from regularizepsf_amd import stars  # (no GPU is touched by the import)

    steps = STEPS if hasattr(stars, "star_catalog") else STEPS[:1]
    for name in steps:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, str(pathlib.Path(__file__).resolve()), "--step", name, "--size", str(args.size),
               "--stars", str(args.stars), "--repeats", str(args.repeats), "--box", str(args.box), "--tree", str(args.tree), "--label", args.label,
               "--out", str(args.out)]
        done = subprocess.run(cmd)
        if done.returncode != 0:
            print(f"shape_timing: step {name} ended with status {done.returncode}; nothing more is started", flush=True)
            sys.exit(done.returncode if done.returncode > 0 else 1)


if __name__ == "__main__":
    main()
