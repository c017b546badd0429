"""Generate the fixtures of the scaled builds (builder_scale_*.npz) by running the REAL reference builder with interpolation_scale > 1.

Import route and stubs: those of make_builder_golden.py, imported from it (``sep`` replaced by a lookup of given star positions, keyed
by the digest of the frame ``sep.extract`` is handed - here the frame the reference's own ``_scale_image`` made), plus the one thing the
reference takes from scikit-image: ``downscale_local_mean``, stubbed with NumPy's reshape-mean, which is its definition for a cell
whose side the scale divides.  Everything else (``_scale_image``, ``_find_patches``, ``_average_patches``, ``ArrayPSFBuilder.build``)
is the reference's code, unchanged.  Stored are data only: seeds, star positions (scaled-frame pixels), the reference's P x P patches,
accept flags, cell membership, and per averaging method the averaged cells after the block mean, the final ``ArrayPSF.values`` and
which cells lie near the clean-up's cut.  A case is reseeded by make_builder_golden.py's rule: no star's deciding value within 1e-3
(relative) of a threshold, at most 10 % of the cells with a pixel within 1e-5 x centre of the 0.005 x centre cut.

Usage:  python tests/golden/make_builder_scale_golden.py [reference root]
"""

from __future__ import annotations

import pathlib
import sys
import warnings

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(HERE))

from make_builder_golden import POSITIONS, _digest, load_builder  # noqa: E402
from tests.builder_cases import METHODS  # noqa: E402
from tests.scale_cases import BUILD_CASES, block_mean, make_build_case  # noqa: E402


def _downscale_local_mean(image, factors):
    assert factors[0] == factors[1] and image.shape[0] % factors[0] == 0 and image.shape[1] % factors[1] == 0
    return block_mean(image, factors[0])


def attempt(name: str, seed: int, ref, improc) -> dict | None:
    case = BUILD_CASES[name]
    n, s = case["n"], case["scale"]
    p = n * s
    frames, stars = make_build_case(name, seed)
    POSITIONS.clear()
    scaled = [improc._scale_image(frame, s, 0) for frame in frames]
    for frame, pos in zip(scaled, stars):
        POSITIONS[_digest(frame)] = pos
    out: dict[str, dict] = {"base": {}}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for method, q in METHODS:
            psf, counts, patches = ref.ArrayPSFBuilder(n).build(frames, interpolation_scale=s, average_method=method, percentile=q,
                                                                return_patches=True)
            corners = np.array(psf.coordinates, np.int64)
            big, counts2 = ref._average_patches(patches, corners, method=method, percentile=q)
            assert counts2 == counts and list(big) == [tuple(c) for c in corners]
            cells = np.stack([_downscale_local_mean(big[tuple(c)], (s, s)) for c in corners])
            excluded = np.zeros(len(corners), bool)
            for i, cell in enumerate(cells):
                pre = cell - improc.calculate_background(cell)
                centre = pre[n // 2, n // 2]
                excluded[i] = bool(np.any(np.abs(pre - 0.005 * centre) <= 1e-5 * np.abs(centre)))
            if excluded.mean() > 0.10:
                print(f"  {name} seed {seed}: {excluded.sum()} of {len(excluded)} cells near the cut for {method}, reseeding")
                return None
            out[method] = {"cells": cells, "values": psf.values, "excluded": excluded}
    # the star list in the reference's terms (image_processing.py:76-79,96,101), at P; no finite threshold is in play in these cases, so
    # the only deciding value is the centre against star_minimum = 0
    rounded, shift, accepted = [], [], []
    for i, (frame, pos) in enumerate(zip(scaled, stars)):
        one = improc._find_patches(frame, 3, None, s, n, i)
        for y, x in pos:
            c = (i, y - p / 2, x - p / 2)
            r = (int(round(c[1])), int(round(c[2])))
            rounded.append(r)
            shift.append((-c[1] + r[0] - 0.5, -c[2] + r[1] - 0.5))
            accepted.append(c in patches)
            if c in one and abs(one[c][p // 2, p // 2]) <= 1e-3 * np.nanmax(np.abs(one[c])):
                print(f"  {name} seed {seed}: a patch centre is too close to star_minimum = 0, reseeding")
                return None
    keys = list(patches)
    assert all(patches[k].shape == (p, p) for k in keys)
    x_bounds = np.stack([corners[:, 0], corners[:, 0] + p], axis=-1)
    y_bounds = np.stack([corners[:, 1], corners[:, 1] + p], axis=-1)
    matches = [ref._find_matches(key, x_bounds, y_bounds, p) for key in keys]
    offsets, members = [0], []
    for cell in range(len(corners)):
        members += [j for j, m in enumerate(matches) if cell in m]
        offsets.append(len(members))
    count_list = np.array([counts[tuple(c)] for c in corners], np.int64)
    assert np.array_equal(np.diff(offsets), count_list)
    out["base"] = {
        "seed": np.array(seed), "stars": np.concatenate(stars), "stars_per_frame": np.array([len(v) for v in stars]),
        "rounded": np.array(rounded, np.int64), "shift": np.array(shift, np.float64), "accepted": np.array(accepted, np.uint8),
        "patch_keys": np.array(keys, np.float64), "patches": np.stack([patches[k] for k in keys]),
        "corners": corners, "counts": count_list, "offsets": np.array(offsets, np.int64), "members": np.array(members, np.int32),
        "scaled_shape": np.array(scaled[0].shape),
    }
    return out


def main() -> None:
    ref, improc = load_builder(*sys.argv[1:2])
    ref.downscale_local_mean = _downscale_local_mean
    for name, case in BUILD_CASES.items():
        seed = 1000 * case["n"] + case["scale"]
        while (out := attempt(name, seed, ref, improc)) is None:
            seed += 1
        np.savez_compressed(HERE / f"builder_scale_{name}.npz", **out["base"])
        for method, _ in METHODS:
            np.savez_compressed(HERE / f"builder_scale_{name}_{method}.npz", **out[method])
        base = out["base"]
        sizes = {f.name: f.stat().st_size for f in sorted(HERE.glob(f"builder_scale_{name}*.npz"))}
        print(name, "seed", seed, "stars", len(base["stars"]), "accepted", int(base["accepted"].sum()), "patch", base["patches"].shape[1:],
              "cells", len(base["corners"]), "non-empty", int((base["counts"] > 0).sum()), "max count", int(base["counts"].max()),
              "excluded", {m: int(out[m]["excluded"].sum()) for m, _ in METHODS}, "bytes", sizes)
        assert all(v < 500_000 for v in sizes.values())


if __name__ == "__main__":
    main()
