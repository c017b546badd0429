"""Time find_stars with and without the deblend option on one large frame:
    python scripts/deblend_timing.py [--size 4096] [--stars 10000] [--repeats 5] [--label TEXT] [--check] [--out FILE]

The frame is scripts/star_timing.py's.  Reports, with the option off and on, the device time of the kernel groups
(S1 - S4: rpsf_stars_kernel_ms; D1 - D4: rpsf_stars_deblend_ms), the number of detections and how many of the generated stars have a
detection within 0.5 px.  The off rows are summarised by a digest, so that two trees can be compared: on a tree without the option the
script reports the off figures alone (run it there with the same arguments).  --check also compares the rows with the float64
restatement (tests/deblend_cases.py) on this machine's CPU.  The text is APPENDED to --out.  There is no pass bar.
"""

from __future__ import annotations

import argparse
import hashlib
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

STAGES = ("S1 mesh", "S2 detection", "S3 labelling", "S4 moments", "D1 - D4 deblend", "one frame on an existing finder, host clock")


def within(found: np.ndarray, truth: np.ndarray, radius: float = 0.5) -> int:
    """How many of `truth` have a position of `found` within `radius`."""
    from scipy.spatial import cKDTree

    if len(found) == 0:
        return 0
    return int(np.count_nonzero(cKDTree(found[:, :2]).query(truth)[0] <= radius))


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--size", type=int, default=4096)
    parser.add_argument("--stars", type=int, default=10000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--box", type=int, default=64)
    parser.add_argument("--label", default="")
    parser.add_argument("--check", action="store_true")
    parser.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "deblend_gpu.log")
    args = parser.parse_args()

    from star_timing import synthetic_frame

    from regularizepsf_amd import _native, stars

    lines: list[str] = []

    def say(text: str) -> None:
        print(text, flush=True)
        lines.append(text)

    frame, truth = synthetic_frame(args.size, args.stars)
    cus, name = _native.device_info(0)
    say(f"[{args.label}] deblend timing: frame {args.size} x {args.size} float32, {args.stars} synthetic stars, box {args.box}, threshold 3.0, "
        f"min_area 5, contrast 0.005, prominence 1.0; {name}, {cus} CUs; {args.repeats} repeats after one warm-up")
    finder = stars._Finder(frame.shape, args.box)
    has_option = hasattr(finder, "set_deblend")
    rows_of = {}
    for on in ((False, True) if has_option else (False,)):
        if has_option:
            finder.set_deblend(on)
        times = []
        for _ in range(args.repeats + 1):
            t0 = time.perf_counter()
            rows = stars.frame_stars(finder, frame, None, 3.0, 5, None)
            host = (time.perf_counter() - t0) * 1e3
            times.append((*finder.kernel_ms(), finder.deblend_ms() if has_option else 0.0, host))
            assert rows_of.setdefault(on, rows).tobytes() == rows.tobytes()  # every repeat gives the same bits
        times = np.array(times[1:])
        say(f"  deblend {'on' if on else 'off'}: {len(rows)} detections, {within(rows, truth)} of {len(truth)} generated stars found within 0.5 px; "
            f"rows sha256 {hashlib.sha256(rows.tobytes()).hexdigest()[:16]}")
        if on:
            say("    components %d, basins %d, split components %d" % finder.deblend_info())
        for i, what in enumerate(STAGES):
            if i != 4 or on:
                say(f"    {what}: median {np.median(times[:, i]):.3f} ms (min {times[:, i].min():.3f}, max {times[:, i].max():.3f})")
        say(f"    S1 - S4 device time: median {np.median(times[:, :4].sum(axis=1)):.3f} ms")
    finder.close()

    if args.check and has_option:
        from tests import deblend_cases as dc

        t0 = time.perf_counter()
        ref = dc.ref_deblend(frame, None, args.box)
        say(f"  NumPy restatement of D1 - D4 on this machine's CPU: {(time.perf_counter() - t0):.1f} s; {len(ref['rows'])} rows, components "
            f"{ref['components']}, basins {ref['basins']}, split {ref['split']}; gaps: threshold {ref['gap_threshold']:.1e}, ascent "
            f"{ref['gap_ascent']:.1e}, prominence {ref['gap_prominence']:.1e}, contrast {ref['gap_contrast']:.1e}")
        got = rows_of[True]
        if len(got) == len(ref["rows"]):
            say(f"    areas and order equal: {bool(np.array_equal(got[:, 3], ref['rows'][:, 3]))}; largest position difference "
                f"{np.abs(got[:, :2] - ref['rows'][:, :2]).max():.2e} px")
        else:
            say("    the counts differ (a decision within rounding of a boundary, see the gaps above)")
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with args.out.open("a") as log:
        log.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
