"""Where the time of ArrayPSFBuilder.build goes (PSF builder): the three kernels, the host stages, the build with
the clean-up on the host and on the device, and the same stages done with NumPy / SciPy on this box's host the way the reference
does them.

    python scripts/builder_timing.py [--frames 16] [--size 2048] [--stars 2000] [--n 32] [--host-frames 1] [--host-cells 400]

Prints one JSON line.  The host restatement runs the per-star stage on --host-frames frames and the per-cell stage on
--host-cells cells only and scales to the workload (they are Python loops: np.nanpercentile alone makes one Python call per pixel
of a cell, minutes for the whole lattice).
"""

from __future__ import annotations

import argparse
import json
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

import regularizepsf_amd as rp  # noqa: E402
from regularizepsf_amd import builder as bld  # noqa: E402


def make_frame(size: int, stars: int, rng: np.random.Generator) -> tuple[np.ndarray, np.ndarray]:
    frame = (10.0 + rng.normal(0.0, 0.3, (size, size))).astype(np.float32)
    pos = rng.uniform(8, size - 9, (stars, 2))
    amp = rng.uniform(60, 400, stars)
    half = 8
    grid = np.arange(-half, half + 1, dtype=np.float64)
    for (r, c), a in zip(pos, amp):
        r0, c0 = int(round(r)), int(round(c))
        stamp = a * np.exp(-0.5 * (((grid + r0 - r)[:, None] / 1.3) ** 2 + ((grid + c0 - c)[None, :] / 1.3) ** 2))
        frame[r0 - half:r0 + half + 1, c0 - half:c0 + half + 1] += stamp.astype(np.float32)
    return frame, pos


def host_patches(frame: np.ndarray, positions: np.ndarray, n: int) -> list[np.ndarray]:
    """The per-star stage as the reference does it: reflect pad, slice, scipy.ndimage.shift, plane fit, subtract."""
    from scipy.ndimage import shift as nd_shift

    padded = np.pad(frame.astype(np.float64), ((n, n), (n, n)), mode="reflect")
    corner, rounded, amount = bld.star_geometry(positions, n)
    out = []
    for (r, c), s in zip(rounded, amount):
        patch = nd_shift(padded[r + n:r + 2 * n, c + n:c + 2 * n], shift=tuple(s), mode="mirror")
        out.append(patch - bld.background_plane(patch))
    return out


def host_average(stack: np.ndarray, offsets: np.ndarray, members: np.ndarray, method: str, n: int, limit: int) -> float:
    """The per-cell stage as the reference does it: a Python list of normalised patches per cell, np.nanmedian / nansum over it.
    Seconds for the whole lattice, measured on `limit` cells spread over it."""
    wide = stack.astype(np.float64)
    wide /= wide[:, n // 2, n // 2][:, None, None]
    n_cells = len(offsets) - 1
    chosen = np.unique(np.linspace(0, n_cells - 1, min(limit, n_cells)).astype(int))
    scale = float(offsets[-1]) / max(1, sum(int(offsets[c + 1] - offsets[c]) for c in chosen))  # by memberships
    t0 = time.perf_counter()
    for c in chosen:
        group = [wide[j] for j in members[offsets[c]:offsets[c + 1]]]
        if not group:
            continue
        if method == "mean":
            acc = np.zeros((n, n))
            for p in group:
                acc = np.nansum([acc, p], axis=0)
        elif method == "median":
            np.nanmedian(group, axis=0)
        else:
            np.nanpercentile(group, 30.0, axis=0)
    return (time.perf_counter() - t0) * scale


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--stars", type=int, default=2000)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--host-frames", type=int, default=1)
    ap.add_argument("--host-cells", type=int, default=400)
    args = ap.parse_args()
    n = args.n
    rng = np.random.default_rng(11)
    made = [make_frame(args.size, args.stars, rng) for _ in range(args.frames)]
    frames, stars = [m[0] for m in made], [m[1] for m in made]
    res: dict = {"frames": args.frames, "size": args.size, "stars_per_frame": args.stars, "n": n}

    # the stages one by one, on a stack of their own
    stack = bld._Stack(n, 0, args.frames * args.stars)
    geometry = [bld.star_geometry(p, n) for p in stars]
    stack.add_frame(frames[0], geometry[0][1], geometry[0][2], np.inf, 0.0, np.inf)  # first launch: module load
    stack.close()
    stack = bld._Stack(n, 0, args.frames * args.stars)
    b1_ms, b1_wall, kept = [], [], []
    for frame, (corner, rounded, shift) in zip(frames, geometry):
        t0 = time.perf_counter()
        flags = stack.add_frame(frame, rounded, shift, np.inf, 0.0, np.inf)
        b1_wall.append((time.perf_counter() - t0) * 1e3)
        b1_ms.append(stack.kernel_ms()[0])
        kept.append(corner[flags == 1])
    res["b1_kernel_ms_per_frame"] = float(np.median(b1_ms))
    res["b1_call_ms_per_frame"] = float(np.median(b1_wall))  # with the frame's upload, the flags' download and the append
    res["patches"] = len(stack)
    # what B1 must move per star: N^2 float32 gathered, N^2 float32 stored
    res["b1_GBps"] = args.stars * n * n * 4 * 2 / (res["b1_kernel_ms_per_frame"] * 1e-3) / 1e9
    corners = rp.calculate_covering(frames[0].shape, n)
    t0 = time.perf_counter()
    offsets, members = bld.cell_membership(np.concatenate(kept), corners, n)
    res["membership_ms"] = (time.perf_counter() - t0) * 1e3
    res["cells"], res["memberships"], res["max_members"] = len(corners), len(members), int(np.diff(offsets).max())
    cells = None
    for method, q in (("mean", 50.0), ("median", 50.0), ("percentile", 30.0)):
        stack.average(method, q, offsets, members)
        t0 = time.perf_counter()
        cells = stack.average(method, q, offsets, members)
        res[f"b2_{method}_call_ms"] = (time.perf_counter() - t0) * 1e3
        ms = stack.kernel_ms()[1]
        res[f"b2_{method}_kernel_ms"] = ms
        # what B2 must move: every member patch read once, every cell written once as float64; the selection re-reads the members
        # 64 (+1 or +2) times, from cache where they fit
        must = len(members) * n * n * 4 + len(corners) * n * n * 8
        res[f"b2_{method}_GBps"] = must / (ms * 1e-3) / 1e9
    t0 = time.perf_counter()
    on_host = [bld.clean_cell(cell) for cell in cells]
    res["cleanup_ms"] = (time.perf_counter() - t0) * 1e3
    # the clean-up on the device (kernel B3): alone on the cells just averaged, then behind B2 without the cells leaving the device
    stack.clean(cells)
    t0 = time.perf_counter()
    cleaned, flagged = stack.clean(cells)
    res["clean_call_ms"] = (time.perf_counter() - t0) * 1e3  # with the cells' upload and the download of the result
    res["clean_kernel_ms"] = stack.clean_ms()
    res["clean_GBps"] = 2 * len(corners) * n * n * 8 / (res["clean_kernel_ms"] * 1e-3) / 1e9  # every cell read once and written once
    res["clean_flagged"] = int(flagged.sum())
    worst = 0.0
    for got, want, flag in zip(cleaned, on_host, flagged):
        if not flag and np.isfinite(want).all():
            worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    res["clean_max_rel_err"] = worst
    stack.model("percentile", 30.0, offsets, members)
    t0 = time.perf_counter()
    stack.model("percentile", 30.0, offsets, members)
    res["model_call_ms"] = (time.perf_counter() - t0) * 1e3  # B2 (percentile) + B3 + one download
    patches = stack.patches()
    stack.close()

    t0 = time.perf_counter()
    rp.ArrayPSFBuilder(n).build(frames, stars=stars)
    res["build_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    rp.ArrayPSFBuilder(n, cleanup="device").build(frames, stars=stars)
    res["build_device_ms"] = (time.perf_counter() - t0) * 1e3

    # the same stages on the host
    t0 = time.perf_counter()
    for frame, pos in zip(frames[:args.host_frames], stars[:args.host_frames]):
        host_patches(frame, pos, n)
    res["host_patches_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / max(1, args.host_frames)
    for method in ("mean", "median", "percentile"):
        res[f"host_{method}_ms"] = host_average(patches, offsets, members, method, n, args.host_cells) * 1e3
    print(json.dumps(res))


if __name__ == "__main__":
    main()
