"""Time the render kernel S10 on one large frame, at that frame's detections fitted with a model built from the same frame:
    python scripts/render_timing.py [--size 4096] [--stars 10000] [--repeats 5] [--psf-size 32] [--radius 8] [--limit 300] [--out FILE]

The frame is scripts/star_timing.py's.  The stars are find_stars' on it, the model is ArrayPSFBuilder(psf_size).build(frame,
stars=those), the fluxes are fit_stars'.  Medians of --repeats after one warm-up of
  * rpsf_stars_render_ms, the device time of S10, per mode and output dtype into a device array, with render() on the host clock (tile lists
    built, records uploaded), next to the device time of a plain device-to-device copy of the float32 frame (rpsf_memcpy_d2d) in the
    same process, and S10's ratio to it,
  * subtract_stars end to end (host clock around the call: finder and model created, frame uploaded, mesh kernels, tile lists, S10, the
    frame returned) to host arrays and to a device out=, and render_stars,
  * the float64 NumPy restatement of the definition (tests/render_cases.ref_render) on the same stars, once, compared bit for bit.
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
STEPS = ("kernels", "subtract_stars", "numpy")
MODES = ((0, "MODEL"), (1, "RESIDUAL"), (2, "RESIDUAL_MESH"))


def copy_ms(frame: np.ndarray, repeats: int) -> list[float]:
    """Device time of rpsf_memcpy_d2d for the frame, per repeat, after one warm-up."""
    import ctypes

    import regularizepsf_amd as rp
    from regularizepsf_amd import _native

    src, dst, ms, times = rp.to_device(frame), rp.device_empty(frame.shape, frame.dtype), ctypes.c_double(0.0), []
    for _ in range(repeats + 1):
        _native.check(_native.lib().rpsf_memcpy_d2d(0, ctypes.c_void_p(dst.ptr), ctypes.c_void_p(src.ptr), frame.nbytes, ctypes.byref(ms)))
        times.append(ms.value)
    return times[1:]


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
    psf, counts = rp.ArrayPSFBuilder(args.psf_size).build(frame, stars=[positions])
    coordinates, values = stars.model_cube(psf)
    cells = stars.nearest_cells(positions, coordinates, args.psf_size)
    model = stars._Model(values)
    fits = stars.fit_from_sums(finder.fit(model, positions, cells, args.radius, True, True))
    flux = np.ascontiguousarray(fits["flux"])
    tile_r, tile_c, chunk = stars.render_info()
    lines.append(f"  {len(positions)} positions, {int(np.isfinite(flux).sum())} with a fitted flux; the model: {len(coordinates)} cells, "
                 f"{sum(1 for v in counts.values() if v)} of them with stars; tiles of {tile_r} x {tile_c} pixels, chunks of {chunk} records")
    if args.step == "kernels":
        copies = copy_ms(frame, args.repeats)
        copy = float(np.median(copies))
        lines.append(f"  a plain device-to-device copy of the frame ({frame.nbytes / 2 ** 20:.0f} MiB read, as much written): {copy:.4f} ms (min "
                     f"{min(copies):.4f}, max {max(copies):.4f})")
        for dtype in (np.float32, np.float64):
            target = rp.device_empty(frame.shape, dtype)
            for mode, label in MODES:
                times = []
                for _ in range(args.repeats + 1):
                    t0 = time.perf_counter()
                    _, drawn = finder.render(model, positions, flux, cells, args.radius, mode, dtype, target)
                    times.append((finder.render_ms(), (time.perf_counter() - t0) * 1e3))
                t = np.array(times[1:])
                digest = hashlib.sha256(target.to_host().tobytes()).hexdigest()[:16]
                lines.append(f"  {label}, {np.dtype(dtype).name}: S10 device time {np.median(t[:, 0]):.3f} ms (min {t[:, 0].min():.3f}, max "
                             f"{t[:, 0].max():.3f}), {np.median(t[:, 0]) / copy:.1f} times the copy; render() on the host clock (records and "
                             f"tile lists built and uploaded, the frame stays on the device) {np.median(t[:, 1]):.3f} ms; {drawn} stars drawn; "
                             f"frame sha256 {digest}")
        times, target = [], rp.device_empty(frame.shape, np.float32)
        for _ in range(args.repeats + 1):
            finder.render(model, positions[:0], flux[:0], cells[:0], args.radius, 1, np.float32, target)
            times.append(finder.render_ms())
        lines.append(f"  RESIDUAL, float32, no stars (the frame through the kernel): S10 device time {np.median(times[1:]):.3f} ms, "
                     f"{np.median(times[1:]) / copy:.1f} times the copy")
    model.close()
    finder.close()
    if args.step == "subtract_stars":
        for background in ("none", "mesh"):
            for where in ("host", "device"):
                times = []
                for _ in range(args.repeats + 1):
                    out = rp.device_empty(frame.shape, np.float32) if where == "device" else None
                    t0 = time.perf_counter()
                    got, drawn = rp.subtract_stars(frame, [fits], psf, args.radius, box=args.box, background=background, out=out, return_counts=True)
                    times.append((time.perf_counter() - t0) * 1e3)
                residual = np.asarray(got[0])
                lines.append(f"  subtract_stars, background {background}, to a {where} array: {drawn[0]} stars drawn; end to end, ms per call: "
                             f"{', '.join(f'{t:.1f}' for t in times[1:])}; median {np.median(times[1:]):.1f}; the frame's rms {frame.std():.3f}, "
                             f"the residual's {np.nanstd(residual):.3f}")
        times = []
        for _ in range(args.repeats + 1):
            t0 = time.perf_counter()
            rp.render_stars(frame.shape, [fits], None, psf, args.radius)
            times.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"  render_stars to a host array: end to end, median {np.median(times[1:]):.1f} ms")
    if args.step == "numpy":
        from tests import render_cases as rd

        t0 = time.perf_counter()
        ref = rd.ref_render(frame, args.box, None, values, positions, flux, cells, args.radius, rd.RESIDUAL, np.float32)
        seconds = time.perf_counter() - t0
        got = rp.subtract_stars(frame, [fits], psf, args.radius, box=args.box)[0]
        differ = int(np.sum(~((got == ref) | (np.isnan(got) & np.isnan(ref)))))
        lines.append(f"  the NumPy float64 restatement on the same {len(positions)} stars (RESIDUAL, float32): {seconds * 1e3:.0f} ms on the host; "
                     f"pixels that differ from S10's: {differ}; same bits: {rd.same_frame(got, ref)}")
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
    parser.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "star_render_gpu.log")
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
            print(f"render_timing: step {name} ended with status {done.returncode}; nothing more is started", flush=True)
            sys.exit(done.returncode if done.returncode > 0 else 1)


if __name__ == "__main__":
    main()
