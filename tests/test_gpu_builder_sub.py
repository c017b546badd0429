"""Neighbour-subtracted patches on the GPU (kernel B1n; the cases of tests/builder_sub_cases.py, which
tests/test_builder_sub_host.py runs on the emulator).

1. composition, bitwise: every patch of every case equals the project's own two steps - S10's float32 residual frame with the patch's own
   star left out, then B1 on that frame - in flag and bits; and equals the restatement;
2. nothing to subtract: build_subtracted is build, bit for bit, for every averaging method, host and device frames;
3. the point of it: on noise-free blended stars with their true fluxes every cell lies within the derived bound of the same stars built
   alone, and the plain build violates that bound;
4. keep: rows that are not kept give no patch and are still subtracted;
5. build_iterative is the loop written out with the public calls;
6. two runs give the same bits;
7. what only a real handle can refuse.
"""

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from regularizepsf_amd import builder as bld
from regularizepsf_amd.device_array import device_empty, to_device
from tests import builder_sub_cases as bc

pytestmark = pytest.mark.gpu


_subtracted, _composed = bc.gpu_subtracted, bc.gpu_composed


# ------------------------------------------------------------------------------------------------------------------ 1. composition
@pytest.mark.parametrize("name", bc.CASES)
def test_patches_equal_the_composition_of_s10_and_b1_bit_for_bit(name):
    case = bc.case(name)
    flags, patches, ms = _subtracted(case)
    want_flags, want_patches = _composed(case)
    assert flags.tolist() == want_flags.tolist()
    assert bc.same_bits(patches, want_patches) and len(patches) == int((flags == bc.ACCEPTED).sum())
    assert ms > 0.0
    restated_patches, restated_flags = bc.expected(name)
    assert flags.tolist() == restated_flags.tolist() and bc.same_bits(patches, restated_patches[restated_flags == bc.ACCEPTED])
    device_flags, device_patches, _ = _subtracted(case, on_device=True)
    assert device_flags.tolist() == flags.tolist() and bc.same_bits(device_patches, patches)


# ------------------------------------------------------------------------------------------------------------------ 2. nothing to subtract
def _lonely_field():
    rng = np.random.default_rng([67, 21])
    pos = np.array([(14.3, 15.8), (16.6, 60.1), (50.2, 20.4), (52.9, 62.7), (33.5, 40.5), (70.4, 41.2)])  # 30 pixels apart: no disc of 3 pixels reaches another star's 16-pixel patch
    flux = 50.0 * (1.0 + rng.random(len(pos)))
    frames = np.stack([bc.star_frame((88, 80), pos, flux, rng), bc.star_frame((88, 80), pos[:4], flux[:4], rng)])
    frames[1, 80, 70] = np.nan  # outside every patch
    coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering((88, 80), 16)]
    psf = rp.IndexedCube(coordinates, np.broadcast_to(bc.gaussian_cube(1, 16, rng)[0], (len(coordinates), 16, 16)).copy())
    return frames, [pos, pos[:4]], [flux, flux[:4]], psf


@pytest.mark.parametrize("method, percentile", [("mean", 50), ("median", 50), ("percentile", 30)])
@pytest.mark.parametrize("on_device", [False, True])
def test_nothing_to_subtract_is_build_bit_for_bit(method, percentile, on_device):
    frames, positions, fluxes, psf = _lonely_field()
    images = to_device(frames) if on_device else frames
    builder = rp.ArrayPSFBuilder(16)
    want = builder.build(images, stars=positions, average_method=method, percentile=percentile, return_patches=True)
    got = builder.build_subtracted(images, positions, psf, 3.0, flux=fluxes, average_method=method, percentile=percentile, return_patches=True)
    assert got[1] == want[1] and sum(want[1].values()) > 10 and any(v == 0 for v in want[1].values())
    assert got[0].coordinates == want[0].coordinates
    assert bc.same_bits(np.asarray(got[0].values), np.asarray(want[0].values))  # the NaN pattern included
    assert list(got[2]) == list(want[2]) and all(bc.same_bits(got[2][key], want[2][key]) for key in want[2])
    if not on_device:  # the function of the same name: psf_size=None is the size of the model's cells, 16
        again = rp.build_subtracted(images, positions, psf, 3.0, flux=fluxes, average_method=method, percentile=percentile, return_patches=True)
        assert again[1] == got[1] and bc.same_bits(np.asarray(again[0].values), np.asarray(got[0].values))
        assert list(again[2]) == list(got[2]) and all(bc.same_bits(again[2][key], got[2][key]) for key in got[2])


# ------------------------------------------------------------------------------------------------------------------ 3. the point of it
def _as_check(result):
    psf, counts, patches = result
    return {tuple(c): np.asarray(v) for c, v in zip(psf.coordinates, np.asarray(psf.values))}, {tuple(k): v for k, v in counts.items()}, patches


def truth_on_the_gpu(label="GPU: "):
    truth = bc.truth_case()
    psf = rp.IndexedCube(truth["coordinates"], truth["cube"])
    n = len(truth["pos"])
    frame = rp.render_stars(bc.TRUTH_SHAPE, [truth["pos"]], [truth["flux"]], psf, bc.TRUTH_R)[0]
    alone = rp.render_stars(bc.TRUTH_SHAPE, [truth["pos"][i:i + 1] for i in range(n)], [truth["flux"][i:i + 1] for i in range(n)], psf, bc.TRUTH_R)
    assert bc.same_bits(frame, bc.host_render(truth["pos"], truth["flux"], psf))  # the frame the CPU test checked the bound on
    builder = rp.ArrayPSFBuilder(bc.TRUTH_N)
    subtracted = builder.build_subtracted(frame, [truth["pos"]], psf, bc.TRUTH_R, flux=[truth["flux"]], average_method="mean", return_patches=True)
    reference = builder.build(np.stack(alone), stars=[truth["pos"][i:i + 1] for i in range(n)], average_method="mean", return_patches=True)
    plain = builder.build(frame, stars=[truth["pos"]], average_method="mean", return_patches=True)
    return bc.check_truth(_as_check(subtracted), _as_check(reference), _as_check(plain), float(frame.max()), label)


def test_with_the_true_fluxes_every_cell_is_the_stars_built_alone_within_the_bound():
    """Measured on the MI355X (profiles/build_subtracted_gpu.log): the largest error / bound over the cells with stars is 1.7e-04 for
    build_subtracted and 5.9e+02 for the plain build."""
    worst, worst_plain = truth_on_the_gpu()
    assert worst <= 1.0
    assert worst_plain > 1.0  # the case is contaminated: plain build does not get there


# ------------------------------------------------------------------------------------------------------------------ 4. keep
def test_rows_that_are_not_kept_give_no_patch_and_are_still_subtracted():
    case = bc.case("n16, model 16, R = 7, folds at every edge")
    n_set = len(case["pos"])
    keep = np.ones(n_set, bool)
    keep[[1, 3, 8]] = False
    coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering(case["frame"].shape, 16)]
    psf = rp.IndexedCube(coordinates, np.broadcast_to(np.asarray(case["cube"])[0], (len(coordinates), 16, 16)).copy())
    cells = np.zeros(n_set, np.int32)
    builder = rp.ArrayPSFBuilder(16)
    frame = np.asarray(case["frame"])
    _, counts, patches = builder.build_subtracted(frame, [np.asarray(case["pos"])], psf, 7.0, flux=[np.asarray(case["flux"])], cells=[cells],
                                                  keep=[keep], return_patches=True)
    out = device_empty(frame.shape, np.float32, 0)
    want = {}
    for i in np.flatnonzero(keep):
        flux = np.array(case["flux"])
        flux[i] = np.nan
        rp.subtract_stars(frame, [np.asarray(case["pos"])], psf, 7.0, flux=[flux], cells=[cells], out=out)
        want.update(builder.build(out, stars=[np.asarray(case["pos"])[i:i + 1]], return_patches=True)[2])
    assert len(want) == int(keep.sum()) == sum(1 for _ in patches) and list(patches) == list(want)
    assert all(bc.same_bits(patches[key], want[key]) for key in want)
    everybody = builder.build_subtracted(frame, [np.asarray(case["pos"])], psf, 7.0, flux=[np.asarray(case["flux"])], cells=[cells], return_patches=True)[2]
    assert len(everybody) == n_set and all(bc.same_bits(everybody[key], patches[key]) for key in patches)  # a row's patch does not depend on who else is cut


# ------------------------------------------------------------------------------------------------------------------ 5. build_iterative
@pytest.mark.parametrize("fit", ["groups", "stars"])
@pytest.mark.parametrize("iterations", [1, 2])
def test_build_iterative_is_the_loop_written_out(fit, iterations):
    truth = bc.truth_case()
    rng = np.random.default_rng([67, 31])
    frame = bc.star_frame(bc.TRUTH_SHAPE, truth["pos"], truth["flux"], rng, sigma=1.5)
    positions = [truth["pos"]]
    builder = rp.ArrayPSFBuilder(bc.TRUTH_N)

    def keep(fits):
        return [f["flux"] > np.nanmedian(f["flux"]) for f in fits]

    got_psf, got_counts, got_fits = builder.build_iterative(frame, positions, 5.0, iterations=iterations, fit=fit, keep=keep, average_method="mean")
    psf, counts = builder.build(frame, stars=positions, average_method="mean")
    for _ in range(iterations):
        fits = (rp.fit_groups if fit == "groups" else rp.fit_stars)(frame, positions, psf, 5.0)
        psf, counts = builder.build_subtracted(frame, fits, psf, 5.0, keep=keep(fits), average_method="mean")
    assert got_counts == counts and got_psf.coordinates == psf.coordinates
    assert bc.same_bits(np.asarray(got_psf.values), np.asarray(psf.values))
    assert len(got_fits) == 1 and got_fits[0].dtype == fits[0].dtype and got_fits[0].tobytes() == fits[0].tobytes()
    assert 0 < sum(counts.values()) and not all(keep(fits)[0])
    if iterations == 1:  # the function of the same name makes the same builder
        psf_f, counts_f, fits_f = rp.build_iterative(frame, positions, 5.0, psf_size=bc.TRUTH_N, iterations=1, fit=fit, keep=keep, average_method="mean")
        assert counts_f == counts and bc.same_bits(np.asarray(psf_f.values), np.asarray(psf.values)) and fits_f[0].tobytes() == fits[0].tobytes()


# ------------------------------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("name", ("n128, model 128, R = 63, 130 neighbours", "n16, model 8, R = 3, a list of 65"))
def test_two_runs_give_the_same_bits(name):
    case = bc.case(name)
    one, two = _subtracted(case), _subtracted(case)  # a fresh builder and a fresh model each
    assert one[0].tolist() == two[0].tolist() and bc.same_bits(one[1], two[1]) and len(one[1]) > 0


# ------------------------------------------------------------------------------------------------------------------ 7. real handles
def test_what_only_a_real_handle_can_refuse():
    lib = _native.lib()
    case = bc.case("n16, model 8, R = 3, a list of 1")
    model = stars._Model(np.asarray(case["cube"]), 0)
    frame = np.asarray(case["frame"])
    flags = np.full(1, 7, np.uint8)

    def call(handle, radius=3.0, n_all=2, own=case["own"]):
        return lib.rpsf_builder_add_frame_subtracted(handle, _native._ptr(frame), 0, frame.shape[0], frame.shape[1], model._handle, n_all,
                                                     _native._ptr(case["pos"]), _native._ptr(case["flux"]), _native._ptr(case["cell"]), radius, 1,
                                                     _native._ptr(own), _native._ptr(case["rounded"]),
                                                     _native._ptr(np.ascontiguousarray(case["shift"])), np.inf, 0.0, np.inf, _native._ptr(flags))

    wide, scaled, plain = bld._Stack(129, 0, 1), bld._Stack(8, 0, 1, 2), bld._Stack(16, 0, 1)
    try:
        assert call(wide._handle) == _native.E_UNSUPPORTED and b"wide" in lib.rpsf_last_error()
        assert call(scaled._handle) == _native.E_UNSUPPORTED and b"scaled" in lib.rpsf_last_error()
        assert call(wide._handle, radius=3.5) == _native.E_UNSUPPORTED  # what the builder cannot do at all comes first
        assert call(plain._handle, radius=3.5) == _native.E_BADARG and b"above min(64, N / 2 - 1)" in lib.rpsf_last_error()
        assert flags[0] == 7 and len(plain) == 0
        # n_all == 0 is plain B1
        assert call(plain._handle, n_all=0, own=np.array([-1], np.int32)) == 0
        b1 = bld._Stack(16, 0, 1)
        want = b1.add_frame(frame, case["rounded"], case["shift"], np.inf, 0.0, np.inf)
        assert flags.tolist() == want.tolist() and bc.same_bits(plain.patches(), b1.patches())
        b1.close()
    finally:
        for stack in (wide, scaled, plain):
            stack.close()
        model.close()
