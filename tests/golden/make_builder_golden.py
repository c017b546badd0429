"""Generate the PSF-builder fixtures (builder_*.npz) by running the REAL reference builder downstream of the star list.

Import route: the one of make_golden.py (a bare ``regularizepsf`` package whose __path__ points at the reference), with two more
stubs - ``skimage.transform`` (only needed for interpolation_scale != 1) and ``sep``, whose ``Background`` subtracts nothing and
whose ``extract`` returns the star positions tests/builder_cases.py drew for that frame.  Everything else (``_find_patches``,
``_average_patches``, ``ArrayPSFBuilder.build``) is the reference's code, unchanged.  Stored are data only: seeds, star
positions, the reference's patches, accept flags, cell membership, averaged cells per method, final ``ArrayPSF.values`` and
counts.  A case is reseeded until no star's deciding value lies within 1e-3 (relative) of a threshold and at most 10 % of the
cells have a pixel within 1e-5 x centre of the clean-up's 0.005 x centre cut.

Usage:  python tests/golden/make_builder_golden.py [reference root]
"""

from __future__ import annotations

import hashlib
import importlib
import pathlib
import sys
import types
import warnings

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(HERE))

from make_golden import load_reference  # noqa: E402
from tests.builder_cases import CASES, METHODS, make_case, thresholds  # noqa: E402

POSITIONS: dict[str, np.ndarray] = {}


def _digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


class _Background:
    globalrms = 1
    __array_ufunc__ = None  # so that `image - background` reaches __rsub__

    def __init__(self, image) -> None:
        pass

    def __rsub__(self, image):
        return image


def _extract(data, thresh, err=None, mask=None):  # noqa: ARG001
    pos = POSITIONS[_digest(data)]
    return {"y": pos[:, 0], "x": pos[:, 1]}


def load_builder(*root):
    sep = types.ModuleType("sep")
    sep.Background, sep.extract = _Background, _extract
    sys.modules["sep"] = sep
    sys.modules["skimage"] = types.ModuleType("skimage")
    sys.modules["skimage.transform"] = types.ModuleType("skimage.transform")
    sys.modules["skimage.transform"].downscale_local_mean = None
    load_reference(*root)
    return importlib.import_module("regularizepsf.builder"), importlib.import_module("regularizepsf.image_processing")


def attempt(name: str, seed: int, ref, improc) -> dict | None:
    case = CASES[name]
    n = case["n"]
    frames, stars = make_case(name, seed)
    POSITIONS.clear()
    for frame, pos in zip(frames, stars):
        POSITIONS[_digest(frame)] = pos
    kw = thresholds(name)
    out: dict[str, dict] = {"base": {}}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for method, q in METHODS:
            psf, counts, patches = ref.ArrayPSFBuilder(n).build(frames, average_method=method, percentile=q, return_patches=True, **kw)
            corners = np.array(psf.coordinates, np.int64)
            cells, counts2 = ref._average_patches(patches, corners, method=method, percentile=q)
            assert counts2 == counts and list(cells) == [tuple(c) for c in corners]
            cells = np.stack([cells[tuple(c)] for c in corners])
            excluded = np.zeros(len(corners), bool)
            for i, cell in enumerate(cells):
                pre = cell - improc.calculate_background(cell)
                centre = pre[n // 2, n // 2]
                excluded[i] = bool(np.any(np.abs(pre - 0.005 * centre) <= 1e-5 * np.abs(centre)))
            if excluded.mean() > 0.10:
                print(f"  {name} seed {seed}: {excluded.sum()} of {len(excluded)} cells near the cut for {method}, reseeding")
                return None
            out[method] = {"cells": cells, "values": psf.values, "excluded": excluded}
    # the star list in the reference's terms (image_processing.py:76-79,96,101)
    rounded, shift, accepted, deciding = [], [], [], []
    sat, smin, smax = kw.get("saturation_threshold", np.inf), kw.get("star_minimum", 0), kw.get("star_maximum", np.inf)
    for i, (frame, pos) in enumerate(zip(frames, stars)):
        one = improc._find_patches(frame, 3, None, 1, n, i)  # no thresholds: every finite patch, to see how close it is to them
        for y, x in pos:
            c = (i, y - n / 2, x - n / 2)
            r = (int(round(c[1])), int(round(c[2])))
            rounded.append(r)
            shift.append((-c[1] + r[0] - 0.5, -c[2] + r[1] - 0.5))
            accepted.append(c in patches)
            if c in one:
                deciding += [(np.max(one[c]), sat), (one[c][n // 2, n // 2], smin), (one[c][n // 2, n // 2], smax)]
    for value, limit in deciding:
        if np.isfinite(limit) and limit != 0 and abs(value - limit) <= 1e-3 * abs(limit):
            print(f"  {name} seed {seed}: a deciding value {value} is too close to {limit}, reseeding")
            return None
    keys = list(patches)
    offsets, members = [0], []
    psf_corners = corners
    x_bounds = np.stack([psf_corners[:, 0], psf_corners[:, 0] + n], axis=-1)
    y_bounds = np.stack([psf_corners[:, 1], psf_corners[:, 1] + n], axis=-1)
    matches = [ref._find_matches(key, x_bounds, y_bounds, n) for key in keys]
    for cell in range(len(psf_corners)):
        members += [p for p, m in enumerate(matches) if cell in m]
        offsets.append(len(members))
    count_list = np.array([counts[tuple(c)] for c in psf_corners], np.int64)
    assert np.array_equal(np.diff(offsets), count_list)
    out["base"] = {
        "seed": np.array(seed), "stars": np.concatenate(stars), "stars_per_frame": np.array([len(s) for s in stars]),
        "rounded": np.array(rounded, np.int64), "shift": np.array(shift, np.float64), "accepted": np.array(accepted, np.uint8),
        "patch_keys": np.array(keys, np.float64), "patches": np.stack([patches[k] for k in keys]),
        "corners": psf_corners, "counts": count_list, "offsets": np.array(offsets, np.int64), "members": np.array(members, np.int32),
    }
    return out


def main() -> None:
    ref, improc = load_builder(*sys.argv[1:2])
    for name in CASES:
        seed = 1000 * CASES[name]["n"] + 1
        while (out := attempt(name, seed, ref, improc)) is None:
            seed += 1
        np.savez_compressed(HERE / f"builder_{name}.npz", **out["base"])
        for method, _ in METHODS:
            np.savez_compressed(HERE / f"builder_{name}_{method}.npz", **out[method])
        base = out["base"]
        print(name, "seed", seed, "stars", len(base["stars"]), "accepted", int(base["accepted"].sum()), "cells", len(base["corners"]),
              "empty", int((base["counts"] == 0).sum()), "max count", int(base["counts"].max()),
              "excluded", {m: int(out[m]["excluded"].sum()) for m, _ in METHODS},
              "bytes", {p.name: p.stat().st_size for p in sorted(HERE.glob(f"builder_{name}*.npz"))})
        assert all(p.stat().st_size < 1_000_000 for p in HERE.glob(f"builder_{name}*.npz"))


if __name__ == "__main__":
    main()
