"""Time find_stars on one large frame:  python scripts/star_timing.py [--size 4096] [--stars 10000] [--repeats 5] [--out FILE]

Reports the device time of the four kernel groups (S1 mesh, S2 detection, S3 labelling, S4 moments; rpsf_stars_kernel_ms), the
end-to-end time of find_stars (host clock around the call, which returns host arrays), and the time of the float64 NumPy / SciPy
restatement of the same definition (tests/star_cases.py) on this machine's CPU.  `sep` is not among this package's dependencies,
so the restatement is the ONLY baseline available here: it is a single-threaded, array-at-a-time reference written for clarity,
not a tuned CPU implementation, and the ratio to it says nothing about sep.  There is no pass bar.
"""

from __future__ import annotations

import argparse
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def synthetic_frame(size: int, n_stars: int, seed: int = 4096) -> tuple[np.ndarray, np.ndarray]:
    """A gently tilted background with noise of 0.3 and `n_stars` Gaussian stars (amplitude 100 ... 400, sigma 1.1 ... 1.5) stamped in
    21 x 21 windows; float32."""
    rng = np.random.default_rng(seed)
    rows, cols = np.mgrid[0:size, 0:size]
    frame = 10.0 + 0.004 * rows - 0.003 * cols + rng.normal(0.0, 0.3, (size, size))
    pos = rng.uniform(12, size - 13, (n_stars, 2))
    amp, sig = rng.uniform(100, 400, n_stars), rng.uniform(1.1, 1.5, (n_stars, 2))
    win = np.arange(-10, 11)
    for (r, c), a, (sr, sc) in zip(pos, amp, sig):
        r0, c0 = int(round(r)), int(round(c))
        gr = np.exp(-0.5 * ((r0 + win - r) / sr) ** 2)
        gc = np.exp(-0.5 * ((c0 + win - c) / sc) ** 2)
        frame[r0 - 10:r0 + 11, c0 - 10:c0 + 11] += a * np.outer(gr, gc)
    return frame.astype(np.float32), pos


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--size", type=int, default=4096)
    parser.add_argument("--stars", type=int, default=10000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--box", type=int, default=64)
    parser.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "star_finder_timing.log")
    args = parser.parse_args()

    import regularizepsf_amd as rp
    from regularizepsf_amd import _native, stars
    from tests import star_cases as sc

    lines: list[str] = []

    def say(text: str) -> None:
        print(text, flush=True)
        lines.append(text)

    frame, truth = synthetic_frame(args.size, args.stars)
    cus, name = _native.device_info(0)
    say(f"find_stars timing: frame {args.size} x {args.size} float32, {args.stars} synthetic stars, box {args.box}, threshold 3.0; {name}, {cus} CUs")

    found = rp.find_stars(frame, box=args.box)[0]  # warm-up: code objects, allocations
    end_to_end = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        found = rp.find_stars(frame, box=args.box)[0]
        end_to_end.append((time.perf_counter() - t0) * 1e3)
    say(f"find_stars end to end (finder created, frame uploaded, positions returned), ms per call: "
        f"{', '.join(f'{t:.1f}' for t in end_to_end)}; median {np.median(end_to_end):.1f}")

    finder = stars._Finder(frame.shape, args.box)
    kernel = []
    for _ in range(args.repeats + 1):
        t0 = time.perf_counter()
        rows = stars.frame_stars(finder, frame, None, 3.0, 5, None)
        kernel.append((*finder.kernel_ms(), (time.perf_counter() - t0) * 1e3))
    finder.close()
    kernel = np.array(kernel[1:])
    for i, what in enumerate(("S1 mesh", "S2 detection", "S3 labelling (tile, seam, flatten)", "S4 moments (count, scan, roots, init, accumulate, walk)",
                              "one frame on an existing finder, host clock")):
        say(f"  {what}: median {np.median(kernel[:, i]):.3f} ms (min {kernel[:, i].min():.3f}, max {kernel[:, i].max():.3f})")
    say(f"  detections: {len(rows)}")

    t0 = time.perf_counter()
    ref = sc.ref_detect(frame, None, args.box)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    say(f"NumPy / SciPy restatement of the definition on this machine's CPU (one thread, the only baseline available here; not sep): {cpu_ms:.0f} ms")
    want = ref["rows"]
    say(f"  restatement: {len(want)} detections, min |f - T| / T = {ref['gap_threshold']:.1e}, clip gap {ref['gap_clip']:.1e} sd")
    if len(want) == len(rows):
        say(f"  areas equal: {bool(np.array_equal(want[:, 3], rows[:, 3]))}; largest position difference {np.abs(want[:, :2] - rows[:, :2]).max():.2e} px")
        dist = np.sqrt(((found[:, None, :] - truth[None, :64, :]) ** 2).sum(axis=-1)).min(axis=0)
        say(f"  distance of the nearest detection to the first 64 true centres: median {np.median(dist):.3f} px")
    else:
        say("  the counts differ (a decision within rounding of a boundary, see the gaps above)")
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
