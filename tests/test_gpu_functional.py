"""Kernel K6 (`rasterize_kernel`: the built-in device PSF models) per sample, and the model route through `psf_fft_impl` per chunk.

tests/test_functional.py compares K6 with the NumPy formula at 2e-7 x the peak of a cube: a bar that sees the core of a Gaussian and nothing
of its wings, and that an evaluation in float or a float normalisation sum pass.  Here every sample is held to what
the kernel's comment promises - evaluated in float64 from float64 parameters, one rounding to float32 -

    |got - want64| <= (2**-24 + 1e-12) |want64| + FLOOR        (+ N**2 2**-53 relative with normalize: the order of the float64 sum)

on the case table of tests/functional_cases.py, whose conditions tests/test_functional_cases.py proves on the CPU: want64 is within 1e-13 of
the long-double formula, every finite case has wings twenty decades below its peak or is flat within a decade, the non-finite cases have
the patterns they claim.  FLOOR is 2**-149, float32's denormal grid: MEASURED_FLUSH below says what the device does with samples between
2**-149 and 2**-126, and the test asserts that it still does.

    1  per sample, every finite case, every N, normalize off and on; sum of a normalised patch within N**2 2**-24 of 1
    2  non-finite cases: NaN and Inf where NumPy has them, the finite samples bounded as in 1
    3  row i of a table of 1, 2, 5, 7, 23 mixed cases == the row rasterised alone, bit for bit, samples and spectra; reversed table ->
       reversed cubes; two calls -> the same bits (the normalisation sum is a fixed tree)
    4  the chunk border of 64 MiB of spectra (N = 256 x 131 rows, N = 128 x 515 rows): rows 0, chunk - 1, chunk, count - 1 as in 1 and equal
       to the row alone; spectra of the whole cube == psf_fft of the downloaded samples; keep_values=False (every chunk rasterised into a
       reused scratch buffer) == the same spectra and no sample buffer
    5  the class route: varied_functional_psf(model)(field).as_array_psf(device=0), with and without **kwargs, == psf_model_fft_device on
       model.pack of the same parameters, bit for bit

Measured on an MI355X (log: profiles/functional_models_gpu.log).  Worst |got - want64| / (2**-24 |want64|) over the samples in float32's normal
range, per model and N (1.00 would be a full half-ulp rounding plus nothing):

    model, normalize                N = 16        32            64            128           256
    elliptical_gaussian             0.935         0.994         0.993         0.998         0.999
    elliptical_gaussian, unit sum   0.994         0.999         0.996         0.999         0.999
      denormal, kept                123, 123      445, 445      1772, 1772    7006, 7006    27949, 27949
      denormal, kept (unit sum)     123, 123      468, 468      1900, 1900    7877, 7877    32804, 32804
    moffat                          0.966         0.990         0.992         0.993         0.998
    moffat, unit sum                0.993         0.997         0.999         0.997         1.000
      denormal, kept                33, 33        33, 33        33, 33        33, 33        33, 33
      denormal, kept (unit sum)     161, 161      186, 186      186, 186      186, 186      186, 186

(denormal, kept: samples with 2**-149 <= |want64| < 2**-126 over the cases of the row, and how many of them came back non-zero.)  The double ->
float conversion does not flush on gfx950, so FLOOR is the denormal grid, 2**-149.  Every bit-for-bit property held.  Seven one-line mutants,
built on a scratch copy and run once each: float expf / powf, parameters through a float cast and a float normalisation sum each fail test 1
(and 4, 5); the parameter table or the kept samples without the chunk's offset each fail test 4 alone.  tests/test_functional.py passes on all
of them but the float parameters.
"""

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd.psf import varied_functional_psf
from tests import functional_cases as fc

pytestmark = pytest.mark.gpu
MODEL_OBJECTS = {"elliptical_gaussian": rp.elliptical_gaussian, "moffat": rp.moffat}
#: what K6's double -> float conversion does with samples in [2**-149, 2**-126) on gfx950: False = it keeps them as denormals
MEASURED_FLUSH = False
FLOOR = fc.NORMAL if MEASURED_FLUSH else fc.TINY


def _rasterise(model, n, rows, normalize, keep_values=True):
    """(samples float32 or None, spectra complex64) of a parameter table through _native.psf_model_fft_device."""
    from regularizepsf_amd import _native

    rows = np.asarray(rows, np.float64)
    values, spectra = _native.psf_model_fft_device(model, n, rows, normalize, 0, keep_values=keep_values)
    try:
        assert (values is None) == (not keep_values)
        got = values.download((len(rows), n, n), np.float32) if keep_values else None
        return got, spectra.download((len(rows), n, n), np.complex64)
    finally:
        spectra.free()
        if values is not None:
            values.free()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _check_samples(case, n, got, tally=None):
    """Bound 1 on one patch; returns the worst ratio to one float32 rounding over the samples in float32's normal range."""
    want = fc.wanted(case, n)
    assert got.dtype == np.float32 and got.shape == want.shape
    nan, inf = np.isnan(want), np.isinf(want)
    assert np.array_equal(np.isnan(got), nan), (n, case.label, "NaN pattern", int(np.isnan(got).sum()), int(nan.sum()))
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf] > 0, want[inf] > 0), (n, case.label, "Inf pattern")
    finite = ~(nan | inf)
    err = np.zeros(want.shape)
    err[finite] = np.abs(got[finite].astype(np.float64) - want[finite])
    allowed = fc.bound(case, n, np.where(finite, want, 0.0), FLOOR)
    normal = finite & (np.abs(want) >= fc.NORMAL)
    ratio = float((err[normal] / (fc.EPS32 * np.abs(want[normal]))).max()) if normal.any() else 0.0
    denormal = finite & (np.abs(want) >= fc.TINY) & (np.abs(want) < fc.NORMAL)
    if tally is not None:
        tally["denormal"] += int(denormal.sum())
        tally["kept"] += int((got[denormal] != 0).sum())
        tally["ratio"] = max(tally["ratio"], ratio)
    over = err > allowed
    if over.any():
        i = np.unravel_index(int((err / allowed).argmax()), err.shape)
        raise AssertionError(f"N={n} {case.label}: {int(over.sum())} samples over the bound; worst at {i}: got {got[i]!r}, want {want[i]!r}, "
                             f"|d| = {err[i]:.3e} > {allowed[i]:.3e} (ratio to one float32 rounding {err[i] / (fc.EPS32 * abs(want[i]) + FLOOR):.2f})")
    if case.normalize and finite.all():
        total = float(got.astype(np.float64).sum())
        assert abs(total - 1.0) <= n * n * fc.EPS32, (n, case.label, total)
    return ratio


# ---- 1, 2: per sample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fc.SIZES)
@pytest.mark.parametrize("model", fc.MODELS)
def test_every_sample_is_one_float32_rounding_of_the_float64_formula(model, n):
    from regularizepsf_amd import _native

    assert fc.SIZES == _native.SUPPORTED_PATCH_SIZES and fc.PARAMS == _native.MODEL_PARAMS and set(fc.MODELS) == set(_native.MODELS)
    tally = {"denormal": 0, "kept": 0, "ratio": 0.0}
    for normalize in (False, True):
        cases = fc.finite_cases(model, n, normalize)
        got, _ = _rasterise(model, n, fc.table(cases), normalize)
        one = {"denormal": 0, "kept": 0, "ratio": 0.0}
        for case, patch in zip(cases, got):
            ratio = _check_samples(case, n, patch, one)
            print(f"FUNCTIONAL-SAMPLE | {model} | N={n} | {case.name}{' | normalize' if normalize else ''} | ratio {ratio:.3f}")
        print(f"FUNCTIONAL-RATIO | {model} | N={n} | normalize {int(normalize)} | {len(cases)} cases | worst ratio to 2**-24 |want| {one['ratio']:.3f} | "
              f"samples with 2**-149 <= |want| < 2**-126: {one['denormal']}, came back non-zero: {one['kept']}")
        for k in ("denormal", "kept"):
            tally[k] += one[k]
        tally["ratio"] = max(tally["ratio"], one["ratio"])
    assert 0 < tally["ratio"] <= 1.0 + fc.EVAL64 / fc.EPS32 + n * n * 2.0 ** -29
    assert tally["denormal"] >= 4
    # what the conversion does below the normal range is a property of the build: MEASURED_FLUSH records it, and FLOOR follows from it
    if MEASURED_FLUSH:
        assert tally["kept"] == 0, tally
    else:
        assert tally["kept"] == tally["denormal"], tally  # (|want64| >= 2**-149 is at least a whole denormal step from 0: none rounds to it)


@pytest.mark.parametrize("n", fc.SIZES)
@pytest.mark.parametrize("model", fc.MODELS)
def test_non_finite_cases_have_numpys_pattern(model, n):
    for case in fc.non_finite_cases(model, n):
        got, spectra = _rasterise(model, n, fc.table([case]), case.normalize)
        want = fc.wanted(case, n)
        _check_samples(case, n, got[0])
        print(f"FUNCTIONAL-NONFINITE | {model} | N={n} | {case.name} | {case.pattern}: NaN {int(np.isnan(got).sum())} Inf {int(np.isinf(got).sum())} of {n * n}")
        assert np.isnan(want).any() or np.isinf(want).any()
        assert not np.isfinite(spectra).all()  # and K3 carries it on: bin 0 sums every sample


# ---- 3: isolation and order ------------------------------------------------------------------------------------------------------------
def _mixed(model, n):
    """Finite and non-finite cases of one normalize setting each, interleaved so that a non-finite row has finite neighbours."""
    out = {}
    for normalize in (False, True):
        finite = list(fc.finite_cases(model, n, normalize))
        odd = [c for c in fc.non_finite_cases(model, n) if c.normalize == normalize]
        rows = []
        for i, case in enumerate(finite):
            rows.append(case)
            if i % 3 == 1 and odd:
                rows.append(odd.pop(0))
        out[normalize] = rows + odd
    return out


@pytest.mark.parametrize("n", fc.SIZES)
@pytest.mark.parametrize("model", fc.MODELS)
def test_a_row_of_a_table_is_the_row_alone_in_any_order_and_twice(model, n):
    for normalize, pool in _mixed(model, n).items():
        alone = {}
        for count in fc.ISOLATION_COUNTS:
            cases = fc.cycle(pool[count % 4:] + pool[:count % 4], count)  # (another start per count: every case of the pool is some table's row)
            rows = fc.table(cases)
            values, spectra = _rasterise(model, n, rows, normalize)
            again = _rasterise(model, n, rows, normalize)
            assert _same_bits(values, again[0]) and _same_bits(spectra, again[1]), (n, count, normalize, "two calls differ")
            back = _rasterise(model, n, rows[::-1], normalize)
            assert _same_bits(values[::-1], back[0]) and _same_bits(spectra[::-1], back[1]), (n, count, normalize, "the reversed table is not the reversed cube")
            for i, case in enumerate(cases):
                if case not in alone:
                    v, s = _rasterise(model, n, rows[i : i + 1], normalize)
                    alone[case] = (v[0], s[0])
                assert _same_bits(values[i], alone[case][0]), (n, count, i, case.label, "samples differ from the row alone")
                assert _same_bits(spectra[i], alone[case][1]), (n, count, i, case.label, "spectrum differs from the row alone")
        assert set(alone) == set(pool)
        print(f"FUNCTIONAL-ISOLATION | {model} | N={n} | normalize {int(normalize)} | tables of {fc.ISOLATION_COUNTS} rows from {len(pool)} cases: "
              f"row == row alone, reversed == reversed, twice == once, bit for bit")


def test_unused_columns_of_the_table_are_not_read():
    """Column 7 of both models and column 5 (theta) of Moffat are padding: any value there, NaN included, gives the same bits."""
    n = 32
    for model in fc.MODELS:
        cases = fc.finite_cases(model, n, True)
        rows = fc.table(cases)
        base = _rasterise(model, n, rows, True)
        rows[:, 7] = np.nan
        if model == "moffat":
            rows[:, 5] = 1e300
        got = _rasterise(model, n, rows, True)
        assert _same_bits(base[0], got[0]) and _same_bits(base[1], got[1]), model


# ---- 4: the chunk border on the model route --------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("n", "count", "chunk"), fc.CHUNK_CROSSING)
@pytest.mark.parametrize("model", fc.MODELS)
def test_model_route_across_a_chunk_border(model, n, count, chunk):
    from regularizepsf_amd import _native

    assert chunk * n * n * 8 == 64 << 20 and chunk < count
    for normalize in (False, True):
        cases = fc.cycle(fc.finite_cases(model, n, normalize), count)
        rows = fc.table(cases)
        values, spectra = _rasterise(model, n, rows, normalize)
        worst = 0.0
        for i in (0, chunk - 1, chunk, count - 1):
            worst = max(worst, _check_samples(cases[i], n, values[i]))
            v, s = _rasterise(model, n, rows[i : i + 1], normalize)
            assert _same_bits(values[i], v[0]), (n, i, cases[i].label, "samples differ from the row alone")
            assert _same_bits(spectra[i], s[0]), (n, i, cases[i].label, "spectrum differs from the row alone")
        assert _same_bits(spectra, _native.psf_fft(values)), (n, normalize, "spectra are not those of the samples kept")
        none, scratch = _rasterise(model, n, rows, normalize, keep_values=False)
        assert none is None and _same_bits(scratch, spectra), (n, normalize, "keep_values=False gives other spectra")
        print(f"FUNCTIONAL-CHUNK | {model} | N={n} | {count} rows, chunk {chunk} | normalize {int(normalize)} | rows 0, {chunk - 1}, {chunk}, {count - 1}: "
              f"worst ratio {worst:.3f}, == row alone; spectra == psf_fft(samples) == keep_values=False, bit for bit")


# ---- 5: the class route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 128])
@pytest.mark.parametrize("model", fc.MODELS)
def test_the_class_route_is_the_table_route(model, n):
    base = MODEL_OBJECTS[model]
    shape = (2 * n + 5, 3 * n)
    coords = [tuple(int(v) for v in c) for c in rp.calculate_covering(shape, n)]
    width = "sigma_row" if model == "elliptical_gaussian" else "alpha"

    def field(row, col):
        q = {"amplitude": 1.0 + row / 300, "row0": n / 2 + 0.3 * col / shape[1], "col0": n / 2 - 0.2, width: 0.05 * n + row / (8.0 * shape[0]), "background": 1e-3}
        if model == "elliptical_gaussian":
            q.update(sigma_col=0.04 * n + col / (9.0 * shape[1]), theta=0.4 + (row + col) / 700)
        else:
            q.update(beta=2.5 + col / 600)
        return q

    varied = varied_functional_psf(base)(field)
    for normalize in (False, True):
        for kwargs in ({}, {"amplitude": -3.0, width: 0.031 * n}):
            psf = varied.as_array_psf(coords, n, device=0, normalize=normalize, **kwargs)
            sets = [{**field(r, c), **kwargs} for r, c in coords]
            values, spectra = _rasterise(model, n, base.pack(sets), normalize)
            assert _same_bits(psf.values, values) and _same_bits(psf.fft_evaluations, spectra), (model, n, normalize, kwargs)
            rows = fc.table([fc.Case(model, "field", tuple(s.items()), normalize) for s in sets])
            assert np.array_equal(rows, base.pack(sets))
            for i in (0, len(coords) - 1):
                _check_samples(fc.Case(model, f"field at {coords[i]}", tuple((k, float(v)) for k, v in sets[i].items()), normalize), n, values[i])
        # the simple model: the same parameters at every coordinate
        simple = base.as_array_psf(coords[:3], n, device=0, normalize=normalize, **sets[1])
        assert _same_bits(simple.values, np.stack([values[1]] * 3)), (model, n, normalize)
    print(f"FUNCTIONAL-CLASS | {model} | N={n} | {len(coords)} patches: as_array_psf(device=0) == psf_model_fft_device(pack(...)), bit for bit, kwargs included")
