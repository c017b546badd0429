"""The case table of tests/test_gpu_functional.py checked without a GPU.

That module bounds every sample kernel K6 stores by one float32 rounding of the float64 formula.  Such a bound says something only if the
float64 formula is a reference to well below one float32 rounding (condition 1: it agrees with long double to 1e-12 per sample), if the cases
hold what a bar of 2e-7 x the peak hides (condition 2: wings twenty decades below the peak, or a patch flat to within a decade, where a
float evaluation of the offset-free part shows at once), if the non-finite cases are what they say (condition 3) and if the table has a case
on each side of what the formula branches on (condition 4).  NumPy only.
"""

import math

import numpy as np
import pytest

import regularizepsf_amd as rp
from tests import functional_cases as fc

WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
MODEL_OBJECTS = {"elliptical_gaussian": rp.elliptical_gaussian, "moffat": rp.moffat}


def _all_finite_cases(model):
    return [(n, case) for n in fc.SIZES for case in fc.finite_cases(model, n)]


def test_the_reference_is_the_formula_of_the_package_on_the_reference_grid():
    """samples() in float64 == the package's host formula called the way as_array_psf calls it, bit for bit; Case.row() == pack()."""
    for model, obj in MODEL_OBJECTS.items():
        assert fc.SLOTS[model] == obj._slots and set(fc.SLOTS[model]) == obj.parameters
        for n in (16, 64):
            rr, cc = np.meshgrid(np.arange(n), np.arange(n))
            for case in fc.finite_cases(model, n) + fc.non_finite_cases(model, n):
                with np.errstate(all="ignore"):
                    host = obj(rr, cc, **case.params)
                assert np.array_equal(fc.samples(case, n), host, equal_nan=True), case.label
                assert np.array_equal(case.row(), obj.pack([case.params])[0], equal_nan=True), case.label
    # [i, j] is row = j, col = i: a centre off the diagonal lands transposed
    case = fc.Case("moffat", "grid", fc._moffat(16, row0=3.0, col0=11.0, alpha=1.0))
    assert np.unravel_index(fc.samples(case, 16).argmax(), (16, 16)) == (11, 3)


@pytest.mark.parametrize("model", fc.MODELS)
def test_float64_agrees_with_long_double_per_sample(model):
    """Condition 1: |float64 - long double| <= 1e-12 |value| wherever |value| >= 2**-149, every finite case and size."""
    if not WIDER:
        pytest.skip("long double is no wider than double here: nothing to compare the float64 formula with")
    worst = 0.0
    for n, case in _all_finite_cases(model):
        if case.normalize:
            continue  # (the same samples)
        lo, hi = fc.samples(case, n), fc.samples(case, n, np.longdouble)
        assert hi.dtype == np.longdouble
        held = np.abs(hi) >= fc.TINY
        assert held.any(), (n, case.label)
        err = float((np.abs(lo - hi)[held] / np.abs(hi)[held]).max())
        worst = max(worst, err)
        assert err <= fc.EVAL64, (n, case.label, err)
    print(f"FUNCTIONAL-CASE | {model} | float64 against long double: worst {worst:.1e} of the value (slack {fc.EVAL64:.0e})")
    assert 0 < worst < fc.EVAL64 / 10  # the slack is at least ten times the reference's own error


@pytest.mark.parametrize("model", fc.MODELS)
def test_every_finite_case_is_in_one_of_the_two_regimes(model):
    """Condition 2: the samples float32 can hold span at least 20 decades below the peak, or the whole patch lies within one decade."""
    regimes = set()
    for n, case in _all_finite_cases(model):
        want = fc.wanted(case, n)
        assert np.isfinite(want).all() and (np.abs(want) >= fc.TINY).any(), (n, case.label)
        held, everything = fc.decades(want)
        regime = "wings" if held >= 20.0 else "flat" if everything <= 1.0 else None
        assert regime, (n, case.label, held, everything)
        regimes.add(regime)
        if case.normalize:
            assert abs(math.fsum(want.ravel()) - 1.0) <= 1e-13, (n, case.label)
    assert regimes == {"wings", "flat"}


@pytest.mark.parametrize("model", fc.MODELS)
def test_the_wing_cases_reach_into_float32_denormals(model):
    """At every size some un-normalised case has samples in [2**-149, 2**-126): what the GPU module counts to see whether K6 keeps them."""
    for n in fc.SIZES:
        count = sum(int(((np.abs(w) >= fc.TINY) & (np.abs(w) < fc.NORMAL)).sum()) for w in (fc.wanted(c, n) for c in fc.finite_cases(model, n, False)))
        assert count >= 4, (model, n, count)


@pytest.mark.parametrize("model", fc.MODELS)
def test_non_finite_cases_have_the_pattern_they_claim(model):
    """Condition 3, from the NumPy formula: NaN and Inf exactly where the pattern says, and the value it says at the finite samples."""
    seen = set()
    for n in fc.SIZES:
        for case in fc.non_finite_cases(model, n):
            assert case.pattern in fc.PATTERNS
            want = fc.wanted(case, n)
            nan, inf, value = fc.claimed_pattern(case, n)
            assert np.array_equal(np.isnan(want), nan) and np.array_equal(np.isinf(want), inf), (n, case.label)
            assert nan.any() or inf.any()
            finite = ~(nan | inf)
            if value is not None:
                assert finite.any() and np.array_equal(want[finite], value[finite]), (n, case.label)
            if case.pattern == "inf_all":
                assert (want > 0).all()
            seen.add(case.pattern)
    assert {"nan_centre", "nan_all", "inf_all"} <= seen
    assert any(c.normalize for c in fc.non_finite_cases(model, 16))  # 0 x Inf of the normalisation


FACTS = sorted(fc.facts(fc.finite_cases("moffat", 16)[0], 16))


@pytest.mark.parametrize("n", fc.SIZES)
@pytest.mark.parametrize("model", fc.MODELS)
def test_every_model_has_a_case_on_each_side_of_every_predicate(model, n):
    """Condition 4, by listing."""
    seen = {f: set() for f in FACTS}
    for case in fc.finite_cases(model, n):
        for f, v in fc.facts(case, n).items():
            seen[f].add(v)
    for f in FACTS:
        if f in fc.EXEMPT.get(model, ()):
            continue
        assert seen[f] == {True, False}, f"{model} N={n}: the table has only the {seen[f]} side of '{f}'"
    q = [case.params for case in fc.finite_cases(model, n, False)]
    # a centre outside on each of the four sides
    assert any(p["row0"] < 0 for p in q) and any(p["row0"] > n - 1 for p in q) and any(p["col0"] < 0 for p in q) and any(p["col0"] > n - 1 for p in q)
    assert any(p["row0"] != round(p["row0"]) and p["col0"] != round(p["col0"]) for p in q)  # sub-pixel
    assert any(p["amplitude"] < 0 for p in q) and any(p["background"] == 1e6 * p["amplitude"] for p in q)
    if model == "elliptical_gaussian":
        tilted = {p["theta"] for p in q if p["sigma_row"] != p["sigma_col"]}
        assert {0.0, math.pi / 2} <= tilted and any(t < 0 for t in tilted) and any(t > 1000 for t in tilted)
        assert any(p["sigma_row"] < 0.35 and p["sigma_col"] < 0.35 for p in q)
    else:
        assert any(p["alpha"] == 0.05 and p["beta"] == 12.0 for p in q) and any(p["beta"] == 0.5 for p in q)


def test_tables_cycle_without_equal_neighbours():
    for model in fc.MODELS:
        for n, count, chunk in fc.CHUNK_CROSSING:
            assert chunk * n * n * 8 == 64 << 20 and chunk < count
            for normalize in (False, True):
                rows = fc.table(fc.cycle(fc.finite_cases(model, n, normalize), count))
                assert rows.shape == (count, fc.PARAMS) and (rows[1:] != rows[:-1]).any(axis=1).all()
                # ... and the first row of the second chunk is not the first row of the table: a chunk rasterised from the table's start shows
                assert (rows[chunk] != rows[0]).any() and (rows[count - 1] != rows[count - 1 - chunk]).any()
