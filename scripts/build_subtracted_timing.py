"""Time kernel B1n (neighbour-subtracted patches) next to plain B1 on one large frame, at that frame's deblended detections with
fit_groups' fluxes:
    python scripts/build_subtracted_timing.py [--size 4096] [--stars 10000] [--repeats 5] [--psf-size 32] [--radius 8] [--out FILE] [--b1-only]

The frame is scripts/star_timing.py's.  The stars are the detections of the deblend option on it, the model is
ArrayPSFBuilder(psf_size).build(frame, stars=those), the fluxes are fit_groups'.  Medians of --repeats after one warm-up of
  * rpsf_builder_kernel_ms' patch figure for B1n on the device-resident frame with the fitted set, for B1n with a set nobody of which is drawn
    (every flux NaN: every list is empty) and for plain B1 on the same star list, all in this process; --b1-only measures the last alone and
    uses nothing this kernel added, so the same script times B1 on an older checkout,
  * build_subtracted end to end on the host frame (host clock) next to build(stars=) on the same,
  * the NumPy restatement (tests/builder_sub_cases.py) on the first --numpy-stars patches, with its time scaled to all of them,
and the two errors of the truth test (tests/test_gpu_builder_sub.py, test 3) against their derived bound.  The text is APPENDED to --out.
There is no pass bar.
"""

from __future__ import annotations

import argparse
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--size", type=int, default=4096)
    parser.add_argument("--stars", type=int, default=10000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--psf-size", type=int, default=32)
    parser.add_argument("--radius", type=float, default=8.0)
    parser.add_argument("--box", type=int, default=64)
    parser.add_argument("--numpy-stars", type=int, default=200)
    parser.add_argument("--b1-only", action="store_true")
    parser.add_argument("--out", default=str(ROOT / "profiles" / "build_subtracted_gpu.log"))
    args = parser.parse_args()
    sys.path.insert(0, str(ROOT / "scripts"))
    sys.path.insert(0, str(ROOT))
    from star_timing import synthetic_frame

    import regularizepsf_amd as rp
    from regularizepsf_amd import _native
    from regularizepsf_amd import builder as bld

    frame, _ = synthetic_frame(args.size, args.stars)
    cus, name = _native.device_info(0)
    positions = rp.find_stars(frame, 3.0, box=args.box, deblend=True)[0]
    n = args.psf_size
    corner, rounded, shift = bld.star_geometry(positions, n)
    _, first = np.unique(corner, axis=0, return_index=True)
    first.sort()
    lines = [f"frame {args.size} x {args.size} float32, {args.stars} synthetic stars, box {args.box}, threshold 3.0, deblend on: {len(positions)} "
             f"detections, {len(first)} distinct patches of {n}; model cells of {n}, R = {args.radius:g}; {name}, {cus} CUs; medians of "
             f"{args.repeats} after one warm-up" + ("; --b1-only" if args.b1_only else "")]
    dense = rp.to_device(frame)

    def median(values):
        return statistics.median(values[1:])

    def b1_times():
        times = []
        for _ in range(args.repeats + 1):
            stack = bld._Stack(n, 0, len(first))
            stack.add_frame_device(dense.ptr, frame.shape, rounded[first], shift[first], np.inf, 0.0, np.inf)
            times.append(stack.kernel_ms()[0])
            stack.close()
        return times

    plain = b1_times()
    lines.append(f"  B1   plain, rpsf_builder_add_frame_device:            {median(plain):9.3f} ms device   (min {min(plain[1:]):.3f}, max {max(plain[1:]):.3f})")
    if not args.b1_only:
        from regularizepsf_amd import stars

        psf, _ = rp.ArrayPSFBuilder(n).build(frame, stars=[positions])
        fits = rp.fit_groups(frame, [positions], psf, args.radius, box=args.box)
        in_groups = int((fits[0]["group_size"] > 1).sum())
        flux, cells = np.ascontiguousarray(fits[0]["flux"]), np.ascontiguousarray(fits[0]["cell"])
        values = stars.model_cube(psf)[1]
        model = stars._Model(values, 0)

        def b1n_times(fluxes):
            times, accepted = [], 0
            for _ in range(args.repeats + 1):
                stack = bld._Stack(n, 0, len(first))
                flags = stack.add_frame_subtracted(dense.ptr, frame.shape, model, positions, fluxes, cells, args.radius, first, rounded[first],
                                                   shift[first], np.inf, 0.0, np.inf)
                times.append(stack.kernel_ms()[0])
                accepted = int((flags == 1).sum())
                stack.close()
            return times, accepted

        fitted, accepted = b1n_times(flux)
        empty, _ = b1n_times(np.full(len(flux), np.nan))
        again = b1_times()
        lines.append(f"  fit_groups: {in_groups} of {len(positions)} detections in groups, {int(np.isfinite(flux).sum())} with a flux")
        lines.append(f"  B1n  the fitted set, _add_frame_device_subtracted:     {median(fitted):9.3f} ms device   (min {min(fitted[1:]):.3f}, max "
                     f"{max(fitted[1:]):.3f}; {accepted} patches accepted)")
        lines.append(f"  B1n  nobody drawn (every list empty):                  {median(empty):9.3f} ms device   (min {min(empty[1:]):.3f}, max "
                     f"{max(empty[1:]):.3f})")
        lines.append(f"  B1   plain again, after the B1n runs:                  {median(again):9.3f} ms device   (min {min(again[1:]):.3f}, max "
                     f"{max(again[1:]):.3f})")
        model.close()
        builder = rp.ArrayPSFBuilder(n)
        ends, plains = [], []
        for _ in range(args.repeats + 1):
            start = time.perf_counter()
            builder.build_subtracted(frame, fits, psf, args.radius)
            ends.append((time.perf_counter() - start) * 1e3)
            start = time.perf_counter()
            builder.build(frame, stars=[positions])
            plains.append((time.perf_counter() - start) * 1e3)
        lines.append(f"  build_subtracted end to end (host frame, host clock):  {median(ends):9.1f} ms; build(stars=) on the same: {median(plains):.1f} ms")
        from tests import builder_sub_cases as bc

        case = bc._finish({"n": n, "radius": args.radius, "frame": frame, "cube": values, "pos": positions, "flux": flux, "cell": cells,
                           "own": first[:args.numpy_stars], "cut": positions[first[:args.numpy_stars]]})
        start = time.perf_counter()
        restated, restated_flags = bc.restate_case(case, bc.brute_lists(case))
        seconds = time.perf_counter() - start
        stack = bld._Stack(n, 0, len(first))
        model = stars._Model(values, 0)
        flags = stack.add_frame_subtracted(dense.ptr, frame.shape, model, positions, flux, cells, args.radius, case["own"], case["rounded"],
                                           case["shift"], np.inf, 0.0, np.inf)
        same = flags.tolist() == restated_flags.tolist() and bc.same_bits(stack.patches(), restated[restated_flags == 1])
        stack.close()
        model.close()
        lines.append(f"  NumPy restatement, {len(case['own'])} patches: {seconds:.2f} s, scaled to {len(first)}: {seconds * len(first) / len(case['own']):.0f} s; "
                     f"the kernel's patches equal it bit for bit: {same}")
        from tests.test_gpu_builder_sub import truth_on_the_gpu

        worst, worst_plain = truth_on_the_gpu(label="")
        lines.append(f"  truth test (noise-free blended stars, true fluxes, mean): largest error / derived bound over the cells with stars: "
                     f"build_subtracted {worst:.3e}, plain build {worst_plain:.3e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "a") as handle:
        handle.write(text)


if __name__ == "__main__":
    main()
