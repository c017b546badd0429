"""The built-in device PSF models (kernel K6, `rasterize_kernel`): the case table of tests/test_gpu_functional.py and its reference.

NumPy only.  The reference is the two formulas of regularizepsf_amd/functional.py on the reference's sample grid - element [i, j] of a patch is
the model at row = j, col = i - written once for any dtype: `samples(case, n)` evaluates it in float64, `samples(case, n, np.longdouble)` one
precision up, and `wanted(case, n)` is what K6 owes: the float64 samples, divided by `math.fsum` of the patch where the case normalises.

A case is a model, its parameters at patch size N and the normalize flag.  Widths and offsets scale with N, so that at every size a case keeps
its character: a Gaussian whose wings run from the peak down through float32's denormals to exact zero, a centre outside the patch on
each side that still leaves samples above the smallest denormal, or a patch flat to within a decade.  These are the two regimes a bar of
2e-7 x the cube's peak cannot tell apart; tests/test_functional_cases.py proves from NumPy alone that every finite case is in one of them,
that float64 is a reference (it agrees with long double to 1e-12 per sample), and that each non-finite case has the pattern it claims.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

SIZES = (16, 32, 64, 128, 256)  # _native.SUPPORTED_PATCH_SIZES (asserted equal in the GPU module)
MODELS = ("elliptical_gaussian", "moffat")
PARAMS = 8  # doubles per row of the parameter table (RPSF_MODEL_PARAMS, include/rpsf.h)
#: model -> parameter -> column of the table; asserted equal to what DeviceModelPSF.pack uses
SLOTS = {
    "elliptical_gaussian": {"amplitude": 0, "row0": 1, "col0": 2, "sigma_row": 3, "sigma_col": 4, "theta": 5, "background": 6},
    "moffat": {"amplitude": 0, "row0": 1, "col0": 2, "alpha": 3, "beta": 4, "background": 6},
}
TINY = 2.0 ** -149    # float32's smallest denormal
NORMAL = 2.0 ** -126  # float32's smallest normal number
EPS32 = 2.0 ** -24    # one rounding to float32
EVAL64 = 1e-12        # the float64 evaluation: about 20 x the reference's own error against long double (tests/test_functional_cases.py)
CHUNK_CROSSING = ((256, 131, 128), (128, 515, 512))  # (N, rows, rows per chunk of 64 MiB of spectra in psf_fft_impl), as K3_CHUNK_CROSSING
ISOLATION_COUNTS = (1, 2, 5, 7, 23)

#: non-finite cases: pattern -> what it claims (proved per case in tests/test_functional_cases.py)
PATTERNS = {
    "nan_cross": "NaN on the sample row and the sample column through the centre (0 / 0 in one of the two terms), the background elsewhere",
    "nan_centre": "NaN at the one sample the centre sits on (0 / 0), the background elsewhere",
    "nan_all": "NaN at every sample",
    "nan_all_but_centre": "NaN at every sample but the one the centre sits on, where pow(1, NaN) = 1 gives background + amplitude",
    "inf_all": "+Inf at every sample",
}


@dataclass(frozen=True)
class Case:
    model: str
    name: str
    items: tuple              # ((parameter, value), ...): every parameter of the model, as float
    normalize: bool = False
    pattern: str | None = None  # key of PATTERNS for a non-finite case, None for a finite one

    @property
    def params(self) -> dict:
        return dict(self.items)

    @property
    def label(self) -> str:
        return f"{self.model} {self.name}{' normalized' if self.normalize else ''}"

    def row(self) -> np.ndarray:
        """The case's row of the parameter table, as kernel K6 reads it."""
        line = np.zeros(PARAMS, np.float64)
        for name, value in self.items:
            line[SLOTS[self.model][name]] = value
        return line


def _gaussian(n, **given):
    base = {"amplitude": 1.0, "row0": n / 2 + 0.37, "col0": n / 2 - 0.21, "sigma_row": 0.05 * n, "sigma_col": 0.05 * n, "theta": 0.0, "background": 0.0}
    assert set(given) <= set(base)
    return tuple((k, float(given.get(k, v))) for k, v in base.items())


def _moffat(n, **given):
    base = {"amplitude": 1.0, "row0": n / 2 + 0.37, "col0": n / 2 - 0.21, "alpha": 0.05 * n, "beta": 12.0, "background": 0.0}
    assert set(given) <= set(base)
    return tuple((k, float(given.get(k, v))) for k, v in base.items())


def _finite_parameters(model, n):
    """name -> parameters; every entry appears in the table with normalize off and on."""
    c = n / 2
    if model == "elliptical_gaussian":
        g = functools.partial(_gaussian, n)
        wide, narrow = 0.07 * n, 0.04 * n
        return {
            "sub-pixel centre": g(),
            "centre above the patch": g(row0=-0.25 * n, sigma_row=0.06 * n, sigma_col=0.06 * n),
            "centre below the patch": g(row0=1.25 * n, sigma_row=0.06 * n, sigma_col=0.06 * n),
            "centre left of the patch": g(col0=-0.25 * n, sigma_row=0.06 * n, sigma_col=0.06 * n),
            "centre right of the patch": g(col0=1.25 * n, sigma_row=0.06 * n, sigma_col=0.06 * n),
            "elliptic, theta 0": g(sigma_row=narrow, sigma_col=wide),
            "elliptic, theta pi/2": g(sigma_row=narrow, sigma_col=wide, theta=math.pi / 2),
            "elliptic, theta -0.7": g(sigma_row=narrow, sigma_col=wide, theta=-0.7),
            "elliptic, theta 1000.4": g(sigma_row=narrow, sigma_col=wide, theta=1000.4),  # range reduction of sin / cos
            "sigma 0.3, core between samples": g(row0=c + 0.5, col0=c + 0.5, sigma_row=0.3, sigma_col=0.3),
            # (no tilted sigma 0.3: the rotated offset u = dr cos + dc sin carries an absolute error of N ulp, and u / 0.3 squared turns it into
            # 2e-13 of the value at N = 256 in the float64 formula itself - the formula's conditioning, not a kernel's precision)
            "negative amplitude": g(amplitude=-2.5, sigma_row=narrow, sigma_col=wide, theta=0.3),
            "background 1e6 x amplitude": g(amplitude=1e-3, background=1e3),
            "background 1e-30": g(background=1e-30),
        }
    m = functools.partial(_moffat, n)
    return {
        "sub-pixel centre": m(),
        "centre above the patch": m(row0=-0.05 * n, alpha=0.06 * n),
        "centre below the patch": m(row0=1.05 * n, alpha=0.06 * n),
        "centre left of the patch": m(col0=-0.05 * n, alpha=0.06 * n),
        "centre right of the patch": m(col0=1.05 * n, alpha=0.06 * n),
        "alpha 0.05, beta 12": m(row0=c + 0.1, col0=c - 0.05, alpha=0.05),
        "beta 0.5": m(alpha=float(n), beta=0.5),
        "beta 0.5, centre above the patch": m(row0=-0.25 * n, alpha=float(n), beta=0.5),
        "negative amplitude": m(amplitude=-2.5),
        "background 1e6 x amplitude": m(amplitude=1e-3, background=1e3),
        "background 1e-30": m(background=1e-30),
    }


def _non_finite(model, n):
    c = float(n // 2)  # a sample
    if model == "elliptical_gaussian":
        g = functools.partial(_gaussian, n)
        return (
            Case(model, "sigma 0, centre on a sample, theta 0", g(row0=c, col0=c, sigma_row=0.0, sigma_col=0.0, background=0.25), pattern="nan_cross"),
            Case(model, "sigma 0, centre on a sample, theta 0.5", g(row0=c, col0=c, sigma_row=0.0, sigma_col=0.0, theta=0.5), pattern="nan_centre"),
            Case(model, "theta NaN", g(theta=math.nan), pattern="nan_all"),
            Case(model, "amplitude = background = 0", g(amplitude=0.0), normalize=True, pattern="nan_all"),
            Case(model, "background +Inf", g(background=math.inf), pattern="inf_all"),
        )
    m = functools.partial(_moffat, n)
    return (
        Case(model, "alpha 0, centre on a sample", m(row0=c, col0=c, alpha=0.0, background=0.25), pattern="nan_centre"),
        Case(model, "row0 NaN", m(row0=math.nan), pattern="nan_all"),
        Case(model, "beta NaN, centre on a sample", m(row0=c, col0=c, beta=math.nan, background=0.25), pattern="nan_all_but_centre"),
        Case(model, "amplitude = background = 0", m(amplitude=0.0), normalize=True, pattern="nan_all"),
        Case(model, "background +Inf", m(background=math.inf), pattern="inf_all"),
    )


@functools.lru_cache(maxsize=None)
def finite_cases(model: str, n: int, normalize: bool | None = None) -> tuple:
    """The finite cases of one model at patch size n; normalize None: both settings, the un-normalised ones first."""
    flags = (False, True) if normalize is None else (normalize,)
    return tuple(Case(model, name, items, flag) for flag in flags for name, items in _finite_parameters(model, n).items())


@functools.lru_cache(maxsize=None)
def non_finite_cases(model: str, n: int) -> tuple:
    return _non_finite(model, n)


def table(cases) -> np.ndarray:
    return np.stack([case.row() for case in cases])


def cycle(cases, count: int) -> list:
    """count rows that cycle through the cases: no two neighbours are equal."""
    return [cases[i % len(cases)] for i in range(count)]


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def sample_grid(n: int, dtype=np.float64):
    """(row, col) as the reference hands them to a model: np.meshgrid(arange, arange), 'xy' indexing - element [i, j] is row = j, col = i."""
    row, col = np.meshgrid(np.arange(n), np.arange(n))
    return row.astype(dtype), col.astype(dtype)


def formula(model: str, row, col, q: dict, dtype=np.float64):
    """The model's formula of regularizepsf_amd/functional.py, in `dtype` throughout (the parameters are float64 values, converted exactly)."""
    q = {k: dtype(v) for k, v in q.items()}
    half, one = dtype(0.5), dtype(1.0)
    dr, dc = row - q["row0"], col - q["col0"]
    if model == "elliptical_gaussian":
        ct, st = np.cos(q["theta"]), np.sin(q["theta"])
        u = dr * ct + dc * st
        v = dc * ct - dr * st
        return q["background"] + q["amplitude"] * np.exp(-half * ((u * u) / (q["sigma_row"] * q["sigma_row"]) + (v * v) / (q["sigma_col"] * q["sigma_col"])))
    return q["background"] + q["amplitude"] * np.power(one + (dr * dr + dc * dc) / (q["alpha"] * q["alpha"]), -q["beta"])


def samples(case: Case, n: int, dtype=np.float64) -> np.ndarray:
    """The un-normalised (n, n) samples of a case in `dtype`."""
    row, col = sample_grid(n, dtype)
    with np.errstate(all="ignore"):
        out = formula(case.model, row, col, case.params, dtype)
    assert out.dtype == dtype and out.shape == (n, n)
    return out


def wanted(case: Case, n: int) -> np.ndarray:
    """What K6 owes for the case, in float64: the samples, over math.fsum of the patch (the exactly rounded sum) where it normalises."""
    out = samples(case, n)
    if case.normalize:
        total = math.fsum(out.ravel()) if np.isfinite(out).all() else float(out.sum())
        with np.errstate(all="ignore"):
            out = out / np.float64(total)
    return out


def relative_slack(case: Case, n: int) -> float:
    """The relative part of the per-sample bound: one float32 rounding + the float64 evaluation (+ the order of the float64 sum of n x n terms)."""
    return EPS32 + EVAL64 + (n * n * 2.0 ** -53 if case.normalize else 0.0)


def bound(case: Case, n: int, want: np.ndarray, floor: float = TINY) -> np.ndarray:
    """|got - want| allowed per sample; `floor` is the grid of what the device stores below float32's normal range."""
    return relative_slack(case, n) * np.abs(want) + floor


def decades(values: np.ndarray) -> tuple[float, float]:
    """(decades between the peak and the smallest sample float32 can hold, decades between the peak and the smallest sample of all)."""
    mag = np.abs(values)
    held = mag[mag >= TINY]
    with np.errstate(divide="ignore"):
        return float(np.log10(held.max() / held.min())), float(np.log10(mag.max() / mag.min()))


def claimed_pattern(case: Case, n: int) -> tuple[np.ndarray, np.ndarray, np.ndarray | None]:
    """(NaN mask, Inf mask, the finite samples' value or None) that the case's pattern claims, from the geometry alone."""
    row, col = sample_grid(n)
    q = case.params
    on_row, on_col = row == q["row0"], col == q["col0"]
    nothing, everything = np.zeros((n, n), bool), np.ones((n, n), bool)
    if case.pattern == "nan_cross":
        return on_row | on_col, nothing, np.full((n, n), q["background"])
    if case.pattern == "nan_centre":
        return on_row & on_col, nothing, np.full((n, n), q["background"])
    if case.pattern == "nan_all":
        return everything, nothing, None
    if case.pattern == "nan_all_but_centre":
        return ~(on_row & on_col), nothing, np.full((n, n), q["background"] + q["amplitude"])
    if case.pattern == "inf_all":
        return nothing, everything, None
    raise KeyError(case.pattern)


def facts(case: Case, n: int) -> dict:
    """The predicates the table must hold a case on each side of, per model and size (Moffat has no theta: EXEMPT)."""
    q = case.params
    return {"centre inside the patch": 0.0 <= q["row0"] <= n - 1 and 0.0 <= q["col0"] <= n - 1, "theta = 0": q.get("theta", 0.0) == 0.0,
            "background = 0": q["background"] == 0.0, "normalize": case.normalize}


EXEMPT = {"moffat": ("theta = 0",)}
