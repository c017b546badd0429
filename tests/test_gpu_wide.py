"""The star kernels at the product's model sizes, radii and frames on the GPU (tests/wide_cases.py; tests/test_wide_host.py runs the same
cases on the emulators): S6 ... S11 through regularizepsf_amd.stars._Finder and ._Model and B1n through the builder's C ABI, against the
float64 restatements by each kernel's own comparison and against the CPU emulator of the same per-thread source byte for byte; repeats on
one finder whose scratch buffers grow and are reused; one check that is no restatement (S10 draws, S8 fits, the bound from the definition);
and the Python entry points at these sizes.

Measured on an MI355X: see profiles/star_wide_gpu.log (every check prints its figures before it asserts)."""

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import stars
from tests import builder_sub_cases as bc
from tests import fit_cases as fc
from tests import render_cases as rn
from tests import wide_cases as wc

pytestmark = pytest.mark.gpu

GPU = (stars._Finder, stars._Model)
EMU = (wc.EmuFinder, wc.EmuModel)


# ------------------------------------------------------------------------------------------------------------------ the same cases
@pytest.mark.parametrize("name", tuple(wc.PHOT_CASES))
def test_apertures_to_64(name):
    assert wc.check_photometry(stars._Finder, name).tobytes() == wc.check_photometry(wc.EmuFinder, name).tobytes()


@pytest.mark.parametrize("name", tuple(wc.REFINE_CASES))
def test_windows_of_sigma_16(name):
    assert wc.check_refine(stars._Finder, name).tobytes() == wc.check_refine(wc.EmuFinder, name).tobytes()


def test_fits_at_every_model_size_and_every_flag():
    rows = {name: wc.check_fit(*GPU, name) for name in wc.FIT_CASES}
    wc.check_fit_flags(rows)
    for name, got in rows.items():
        assert got.tobytes() == wc.check_fit(*EMU, name).tobytes(), name


def test_fitted_positions_at_every_model_size():
    rows = {name: wc.check_fitpos(*GPU, name) for name in wc.FITPOS_CASES}
    wc.check_fitpos_ends({name: steps for name, (steps, _) in rows.items()})
    for name, (steps, fits) in rows.items():
        emu_steps, emu_fits = wc.check_fitpos(*EMU, name)
        assert steps.tobytes() == emu_steps.tobytes() and fits.tobytes() == emu_fits.tobytes(), name


def test_the_library_and_the_emulator_share_the_tile_and_the_chunk_and_the_lists_reach_three_chunks():
    assert stars.render_info() == rn.emulator_info()[:3]
    wc.check_render_lists()


@pytest.mark.parametrize("name", tuple(wc.RENDER_CASES))
def test_model_and_residual_frames(name):
    frames, emulated = wc.check_render(*GPU, name), wc.check_render(*EMU, name)
    for key, got in frames.items():
        assert rn.same_frame(got, emulated[key]), (name, key)


@pytest.mark.parametrize("name", tuple(wc.GROUP_CASES))
def test_group_fits(name):
    assert wc.check_group(*GPU, name).tobytes() == wc.check_group(*EMU, name).tobytes()


def test_neighbour_subtracted_patches_of_64_with_a_model_of_130():
    """Each patch equals the composition S10 (RESIDUAL, float32) then B1, in flag and bits, and the restatement."""
    case = wc.builder_case()
    flags, patches, ms = bc.gpu_subtracted(case)
    want_flags, want_patches = bc.gpu_composed(case)
    restated_patches, restated_flags = wc.builder_expected()
    print(f"B1n on the wide frame: {len(flags)} patches of 64, a model of 130, R = 64: flags {flags.tolist()}, {ms:.3f} ms")
    assert flags.tolist() == want_flags.tolist() == restated_flags.tolist() and ms > 0.0
    assert bc.same_bits(patches, want_patches) and len(patches) == int((flags == bc.ACCEPTED).sum()) >= 3
    assert bc.same_bits(patches, restated_patches[restated_flags == bc.ACCEPTED])
    device_flags, device_patches, _ = bc.gpu_subtracted(case, on_device=True)
    assert device_flags.tolist() == flags.tolist() and bc.same_bits(device_patches, patches)


# ------------------------------------------------------------------------------------------------------------------ repeats
def test_a_second_call_and_a_small_call_in_between_change_nothing():
    """On one finder: every kernel's wide call twice, then a small call (R = 2, N = 9, three stars) of every kernel, then the wide calls
    again - the scratch buffers have grown and are reused, and every wide result is the first one's bytes."""
    c = wc.fit_case("N = 256, R = 64")
    p = wc.phot_case("eight apertures to 64, s = 8, mesh")
    r = wc.refine_case("sigmas 16 to 0.5, max_iter 16, mesh")
    s = wc.fitpos_case("N = 256, R = 64")
    d = wc.render_case("N = 256, R = 64")
    g = wc.group_case("N = 130, R = 64, mesh, flux and background")
    finder, model, middle, small = stars._Finder(wc.SHAPE, wc.BOX), stars._Model(c["cube"]), stars._Model(g["cube"]), stars._Model(fc.model(9))
    three, cells3 = np.ascontiguousarray(wc.STARS[:3]), np.zeros(3, np.int32)

    def wide():
        out = [finder.photometry(p["positions"], p["radii"], p["subpix"], True),
               finder.refine(r["positions"], r["sigma"], 16, r["eps"], r["max_shift"], True),
               finder.fit(model, c["positions"], c["cells"], 64.0, True, True),
               *finder.fit_positions(model, s["positions"], s["cells"], 64.0, True),
               finder.fit_groups(middle, g["positions"], g["cells"], 64.0, True, True, wc.LINK)]
        out += [finder.render(model, d["positions"], d["flux"], d["cells"], 64.0, mode, dtype)[0] for mode, dtype in wc.ALL_OUTPUTS]
        return [a.tobytes() for a in out]

    def little():
        finder.photometry(three, (2.0,), 1, True)
        finder.refine(three, 0.5, 2)
        finder.fit(small, three, cells3, 2.0)
        finder.fit_positions(small, three, cells3, 2.0)
        finder.fit_groups(small, three, cells3, 2.0)
        return finder.render(small, three, np.ones(3), cells3, 2.0, rn.MODEL, np.float64)[0].tobytes()

    try:
        finder.background_device(c["frame"], None)
        first = wide()
        assert wide() == first
        one = little()
        assert wide() == first
        assert little() == one
    finally:
        for m in (model, middle, small):
            m.close()
        finder.close()


# ------------------------------------------------------------------------------------------------------------------ not a restatement
ROUND_TRIP_SHAPE = (400, 400)  # the smallest square that holds four discs of R = 64 more than 2 R apart (the wide frame holds one)
ROUND_TRIP_STARS = np.array([(70.3, 68.6), (72.0, 330.5), (331.5, 70.0), (200.2, 203.7)])
ROUND_TRIP_FLUX = np.array([1000.0, 37.5, 2.0e5, 640.25])


def test_what_s10_draws_s8_fits_within_the_rounding_of_the_frame():
    """S10 draws four isolated stars with the broad positive cell (N = 130, R = 64) into a float64 MODEL frame, which is rounded once to
    float32; S8 without a fitted constant and without the mesh fits them at the same positions.  Both sides are GPU kernels of different
    structure (a thread per pixel, a wave per star), and the bound comes from the definition: every pixel of a disc is flux x m rounded
    once, relative error 2^-24; Sdm / Smm is a mean of d / m with the positive weights m m, so it is off by at most 2^-24 of the flux, and a
    factor 2 covers the float64 sums: |f / flux - 1| <= 2^-23.  The residual is at most 2^-24 of a pixel each, and the fitted flux moves
    it by as much again: chi2 < N_use (2^-24 peak pixel)^2 4."""
    R, u32 = 64.0, 2.0 ** -24
    cube = wc.cube(130)
    cells = np.full(len(ROUND_TRIP_STARS), wc.BROAD, np.int32)
    gaps = np.linalg.norm(ROUND_TRIP_STARS[:, None] - ROUND_TRIP_STARS[None], axis=2) + 1e9 * np.eye(len(ROUND_TRIP_STARS))
    assert gaps.min() > 2 * R and np.all(ROUND_TRIP_STARS - R >= 0) and np.all(ROUND_TRIP_STARS + R <= np.array(ROUND_TRIP_SHAPE) - 1)
    finder, model = stars._Finder(ROUND_TRIP_SHAPE, wc.BOX), stars._Model(cube)
    try:
        drawn, count = finder.render(model, ROUND_TRIP_STARS, ROUND_TRIP_FLUX, cells, R, rn.MODEL, np.float64)
        assert count == 4 and drawn.dtype == np.float64
        frame = drawn.astype(np.float32)
        assert np.all((frame == 0.0) | (np.abs(frame) >= 2 * float(np.finfo(np.float32).tiny))), "a pixel is subnormal in float32"
        finder.background_device(frame, None)
        fits = finder.fit(model, ROUND_TRIP_STARS, cells, R, False, False)
    finally:
        model.close()
        finder.close()
    ratio = np.abs(fits[:, fc.F] / ROUND_TRIP_FLUX - 1.0)
    peak = np.array([frame[int(round(y)) - 2:int(round(y)) + 3, int(round(x)) - 2:int(round(x)) + 3].max() for y, x in ROUND_TRIP_STARS])
    limit = fits[:, fc.N_USE] * (u32 * peak) ** 2 * 4.0
    print(f"round trip at R = 64, N = 130: N_use {fits[:, fc.N_USE].astype(int).tolist()}, |f / flux - 1| = {ratio.tolist()} (the bound: 2^-23 = "
          f"{2.0 ** -23:.3e}), chi2 {fits[:, fc.CHI2].tolist()} (the bounds: {limit.tolist()})")
    assert np.all(fits[:, fc.FLAGS] == 0) and np.all(fits[:, fc.N_USE] == fits[:, fc.N_ALL]) and np.all(fits[:, fc.N_USE] >= 12000)
    assert np.all(ratio <= 2.0 ** -23)
    assert np.all(fits[:, fc.CHI2] < limit)


# ------------------------------------------------------------------------------------------------------------------ the Python entry points
def test_the_python_entry_points_on_the_wide_frame():
    """star_photometry, refine_stars, fit_stars, fit_positions, fit_groups, subtract_stars and build_subtracted with the default box: the
    host frame and the device frame give the same bytes, and the structured rows are *_from_sums of the C ABI's rows."""
    frame = wc.field()["frame"].astype(np.float32)
    on_device = rp.to_device(frame)
    coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering(wc.SHAPE, 130)]
    psf = rp.IndexedCube(coordinates, np.stack([wc.cube(130)[k % 4] for k in range(len(coordinates))]))
    everywhere, near = wc.positions(), wc.positions()[:10]  # (without the far position for the iteration: a start stays inside 2^20)
    crowd = wc.crowd()[0]
    radii, sigma = (1.0, 16.0, 64.0), np.resize(np.array([16.0, 12.0, 8.0, 0.5]), len(everywhere))
    cells = {id(p): stars.nearest_cells(p, coordinates, 130) for p in (everywhere, near, crowd)}
    assert len(coordinates) >= 4 and len({int(k) % 4 for p in (everywhere, crowd) for k in cells[id(p)]}) >= 2
    finder, model = stars._Finder(wc.SHAPE, 64), stars._Model(np.asarray(psf.values))
    try:
        finder.background_device(frame, None)
        want = {
            "star_photometry": stars.photometry_from_sums(finder.photometry(everywhere, radii, 8, True), radii, 8),
            "refine_stars": stars.refine_from_sums(finder.refine(everywhere, sigma)),
            "fit_stars": stars.fit_from_sums(finder.fit(model, everywhere, cells[id(everywhere)], 64.0), True),
            "fit_positions": stars.fitpos_from_sums(*finder.fit_positions(model, near, cells[id(near)], 64.0), True),
            "fit_groups": stars.group_fit_from_sums(finder.fit_groups(model, crowd, cells[id(crowd)], 64.0, True, True, wc.LINK), True),
        }
        residual = finder.render(model, crowd, want["fit_groups"]["flux"], cells[id(crowd)], 64.0, rn.RESIDUAL, np.float32)[0]
    finally:
        model.close()
        finder.close()
    for image in (frame, on_device):
        got = {
            "star_photometry": rp.star_photometry(image, everywhere, radii, subpix=8),
            "refine_stars": rp.refine_stars(image, everywhere, sigma),
            "fit_stars": rp.fit_stars(image, everywhere, psf, 64.0),
            "fit_positions": rp.fit_positions(image, near, psf, 64.0),
            "fit_groups": rp.fit_groups(image, crowd, psf, 64.0, link=wc.LINK),
        }
        for name, rows in got.items():
            assert len(rows) == 1 and rows[0].dtype == want[name].dtype and rows[0].tobytes() == want[name].tobytes(), name
        taken = rp.subtract_stars(image, got["fit_groups"], psf, 64.0)
        assert len(taken) == 1 and taken[0].dtype == np.float32 and rn.same_frame(np.asarray(taken[0]), residual)
    fitted = want["fit_groups"]
    print(f"entry points: fit_stars flags {want['fit_stars']['flags'].tolist()}, fit_positions niter {want['fit_positions']['niter'].tolist()}, "
          f"fit_groups sizes {fitted['group_size'].tolist()}, {int(np.isfinite(fitted['flux']).sum())} of {len(fitted)} stars drawn")
    assert fitted["group_size"].tolist() == wc.GROUP_SIZES and np.isfinite(fitted["flux"]).sum() >= 10
    builder = rp.ArrayPSFBuilder(64)
    keep = np.zeros(len(fitted), bool)
    keep[[0, 2, 3, 4, 22]] = True  # of the pair, the three, the star alone: a patch of the chain or the pile has no ring below its centre
    host = builder.build_subtracted(frame, [fitted], psf, 64.0, keep=[keep], average_method="mean", return_patches=True)
    device = builder.build_subtracted(on_device, [fitted], psf, 64.0, keep=[keep], average_method="mean", return_patches=True)
    assert host[1] == device[1] and sum(host[1].values()) >= 3 and list(host[2]) == list(device[2]) and len(host[2]) >= 3
    assert bc.same_bits(np.asarray(host[0].values), np.asarray(device[0].values)) and all(bc.same_bits(host[2][k], device[2][k]) for k in host[2])
