"""Neighbour-subtracted patches (kernel B1n) without a GPU: the kernel's phases on the CPU emulator (tests/emu/emu_builder_sub.cpp)
against the float64 / NumPy restatement (tests/builder_sub_cases.py) bit for bit, the host's neighbour lists against the all-pairs rule, the
same code under the host sanitizers as a program of its own, and what is host code in the product: the two new methods' argument checks and
the C ABI's return codes.  tests/test_gpu_builder_sub.py runs the same cases on the GPU."""

import ctypes
import inspect
import subprocess

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native
from regularizepsf_amd import builder as bld
from tests import builder_sub_cases as bc

NEW_SYMBOLS = ("rpsf_builder_add_frame_subtracted", "rpsf_builder_add_frame_device_subtracted", "rpsf_builder_subtract_info")
FAKE = 0x7F0000000000  # a handle nobody dereferences


# ------------------------------------------------------------------------------------------------------------------ emulator and lists
def test_the_case_table_holds_what_it_must():
    """A check of the case table itself (the restatement and the all-pairs lists), not of the product - but the chunk borders it is laid out
    around are the product's, asked of the library."""
    chunk = ctypes.c_int(0)
    assert _native.lib().rpsf_builder_subtract_info(ctypes.byref(chunk), None, None) == 0 and chunk.value == bc.CHUNK
    assert set(bc.COUNTS) == {0, 1, chunk.value, chunk.value + 1, 2 * chunk.value + 2}
    bc.check_well_posed()


@pytest.mark.parametrize("name", bc.CASES)
def test_the_neighbour_lists_equal_the_all_pairs_rule(name):
    case = bc.case(name)
    brute, lists = bc.brute_lists(case), bc.emu_lists(case)
    assert len(brute) == len(lists) == len(case["own"])
    for k, (want, got) in enumerate(zip(brute, lists)):
        assert got.dtype == np.int32 and np.array_equal(got, want), (k, got, want)


def test_the_lists_on_a_field_of_many_buckets():
    """A frame of 9 x 7 buckets with 2 000 stars and patches that fold over every edge: the grid finds what all pairs find."""
    rng = np.random.default_rng([67, 5])
    shape = (9 * bc.BUCKET - 5, 7 * bc.BUCKET - 11)
    pos = rng.random((2000, 2)) * (np.array(shape) + 40.0) - 20.0  # some off the frame
    flux = np.where(rng.random(2000) < 0.1, np.nan, 1.0)
    case = {"n": 33, "radius": 11.5, "frame": np.zeros(shape, np.float32), "cube": np.zeros((3, 24, 24)), "pos": pos, "flux": flux,
            "cell": rng.integers(-1, 4, 2000), "own": np.concatenate([np.arange(0, 2000, 7), [-1, -1]]),
            "cut": np.concatenate([pos[::7], [(0.0, 0.0), (shape[0] - 1.0, shape[1] - 1.0)]])}
    case = bc._finish(case)
    for want, got in zip(bc.brute_lists(case), bc.emu_lists(case)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("name", bc.CASES)
def test_the_emulator_matches_the_restatement_bit_for_bit(name):
    case = bc.case(name)
    patches, flags = bc.emu_patches(case, bc.emu_lists(case))
    want_patches, want_flags = bc.expected(name)
    assert flags.tolist() == want_flags.tolist()
    assert bc.same_bits(patches, want_patches)


@pytest.mark.parametrize("name", ("n5, model 8, R = 3, the odd rows", "n16, model 16, R = 7, folds at every edge", "n16, model 8, R = 3, a list of 65"))
def test_any_superset_in_ascending_order_gives_the_same_patches(name):
    """The result must not depend on the lists being minimal: with every other drawn star on every list the bits are the same."""
    case = bc.case(name)
    drawn = np.flatnonzero(bc.star_drawn(case["flux"], case["cell"], len(case["cube"]))).astype(np.int32)
    everybody = [drawn[drawn != own] for own in case["own"]]
    patches, flags = bc.emu_patches(case, everybody)
    assert flags.tolist() == bc.expected(name)[1].tolist() and bc.same_bits(patches, bc.expected(name)[0])


def test_an_empty_set_is_kernel_b1():
    from tests import builder_cases

    case = bc.case("n33, model 16, R = 7, a patch as wide as the frame")
    patches, flags = bc.emu_patches(case, [np.zeros(0, np.int32)] * len(case["own"]))
    b1_patches, b1_flags = builder_cases.emu_patches(case["frame"], case["n"], case["rounded"], case["shift"])
    assert flags.tolist() == b1_flags.tolist() and bc.same_bits(patches, b1_patches)


def test_the_emulator_under_the_host_sanitizers(tmp_path):
    """The lists and the phases as a plain program with a main of its own (EMU_BUILDER_SUB_MAIN) under -fsanitize=address,undefined, on the
    same inputs; nothing that is loaded into Python is touched by a sanitizer."""
    program = tmp_path / "emu_builder_sub_sanitized"
    built = subprocess.run([bc._clang(), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-DEMU_BUILDER_SUB_MAIN", str(bc.ROOT / "tests" / "emu" / "emu_builder_sub.cpp"), "-o", str(program)],
                           capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitizer" in built.stderr):
        pytest.skip("the host compiler cannot link the sanitizers' runtimes: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr[-2000:]
    for name in bc.CASES:
        case = bc.case(name)
        (tmp_path / "in.bin").write_bytes(bc.case_file(case))
        done = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
        assert done.returncode == 0, (name, done.returncode, done.stdout[-500:], done.stderr[-3000:])
        patches, flags, lists = bc.read_result(case, (tmp_path / "out.bin").read_bytes())
        assert flags.tolist() == bc.expected(name)[1].tolist() and bc.same_bits(patches, bc.expected(name)[0]), name
        assert all(np.array_equal(a, b) for a, b in zip(lists, bc.brute_lists(case))), name


def test_the_chunk_fits_behind_the_block_of_b1():
    chunk, bucket, size = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    assert _native.lib().rpsf_builder_subtract_info(ctypes.byref(chunk), ctypes.byref(bucket), ctypes.byref(size)) == 0
    assert (chunk.value, bucket.value) == (bc.CHUNK, bc.BUCKET) == (64, 32)
    assert size.value == 144480 + 64 * (3 * 8 + 4) == 146272 <= 160 * 1024 and 144480 % 8 == 0
    assert _native.lib().rpsf_builder_subtract_info(None, None, None) == 0


# ------------------------------------------------------------------------------------------------------------------ the point of it, on the CPU
def test_the_bound_holds_on_the_restatement_and_the_plain_build_violates_it():
    from regularizepsf_amd.stars import nearest_cells

    truth = bc.truth_case()
    frame, alone = bc.truth_frames(bc.host_render)
    # (the bound is checked here on the test's own restatement, before the GPU test holds the product to it; what ties the restatement to the
    # product is the emulator: the blended frame's patches through the product's phases are the restatement's, bit for bit)
    n = len(truth["pos"])
    blended = bc._finish({"n": bc.TRUTH_N, "radius": bc.TRUTH_R, "frame": frame, "cube": truth["cube"], "pos": truth["pos"], "flux": truth["flux"],
                          "cell": nearest_cells(truth["pos"], truth["coordinates"], bc.TRUTH_N), "own": np.arange(n), "cut": truth["pos"]})
    emulated, emulated_flags = bc.emu_patches(blended, bc.emu_lists(blended))
    restated, restated_flags = bc.restate_case(blended, bc.brute_lists(blended))
    assert emulated_flags.tolist() == restated_flags.tolist() == [bc.ACCEPTED] * n and bc.same_bits(emulated, restated)
    cells = nearest_cells(truth["pos"], truth["coordinates"], bc.TRUTH_N)
    subtracted = bc.restated_build([frame], [truth["pos"]], ([truth["flux"]], [cells], truth["cube"], bc.TRUTH_R))
    reference = bc.restated_build(alone, [truth["pos"][i:i + 1] for i in range(len(truth["pos"]))])
    plain = bc.restated_build([frame], [truth["pos"]])
    worst, worst_plain = bc.check_truth(subtracted, reference, plain, float(frame.max()), "restatement: ")
    assert worst <= 1.0 < worst_plain
    assert 1.0 <= bc.plane_gain(bc.TRUTH_N) <= 5.0  # by hand: 1 for the mean and at most 2 per slope


# ------------------------------------------------------------------------------------------------------------------ the Python interface
def test_the_methods_are_exported_and_build_is_unchanged():
    assert "build_subtracted" in rp.__all__ and "build_iterative" in rp.__all__
    assert rp.build_subtracted is bld.build_subtracted and rp.build_iterative is bld.build_iterative
    pos, kw = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    names = [(p.name, p.default, p.kind) for p in inspect.signature(rp.ArrayPSFBuilder.build_subtracted).parameters.values()][1:]
    empty = inspect.Parameter.empty
    assert names == [("images", empty, pos), ("fits", empty, pos), ("psf", empty, pos), ("radius", empty, pos), ("flux", None, kw),
                     ("cells", None, kw), ("keep", None, kw), ("average_method", "median", kw), ("percentile", 50, kw),
                     ("saturation_threshold", np.inf, kw), ("star_minimum", 0, kw), ("star_maximum", np.inf, kw), ("return_patches", False, kw)]
    names = [(p.name, p.default, p.kind) for p in inspect.signature(rp.ArrayPSFBuilder.build_iterative).parameters.values()][1:]
    assert names == [("images", empty, pos), ("stars", empty, pos), ("radius", empty, pos), ("iterations", 2, kw), ("fit", "groups", kw),
                     ("keep", None, kw), ("build_keywords", empty, inspect.Parameter.VAR_KEYWORD)]
    build = [(p.name, p.default) for p in inspect.signature(rp.ArrayPSFBuilder.build).parameters.values()][1:]
    assert build == [("images", empty), ("sep_mask", None), ("hdu_choice", 0), ("num_workers", None), ("interpolation_scale", 1),
                     ("star_threshold", 3), ("average_method", "median"), ("percentile", 50), ("saturation_threshold", np.inf),
                     ("image_mask", None), ("star_minimum", 0), ("star_maximum", np.inf), ("sqrt_compressed", False), ("return_patches", False),
                     ("stars", None)]
    text = rp.ArrayPSFBuilder.build_subtracted.__doc__
    assert "bit for bit" in text and "keep" in text and "bilinear" in text


def test_argument_errors_of_the_two_methods():
    frame, positions = np.zeros((40, 48), np.float32), np.array([[10.0, 12.0], [13.0, 15.0]])
    psf = rp.IndexedCube([(0, 0)], np.ones((1, 8, 8)))
    b = rp.ArrayPSFBuilder(8)
    flux = [np.array([1.0, 2.0])]
    for radius in (0.0, -1.0, 3.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="radius must lie in 0 < R <= min\\(64, N / 2 - 1\\) = 3 for cells of 8"):
            b.build_subtracted(frame, [positions], psf, radius, flux=flux)
    with pytest.raises(TypeError, match="radius must be a number"):
        b.build_subtracted(frame, [positions], psf, "wide", flux=flux)
    with pytest.raises(ValueError, match="flux= is needed"):
        b.build_subtracted(frame, [positions], psf, 2.0)
    with pytest.raises(ValueError, match="flux\\[0\\] has shape \\(1,\\) for the 2 stars"):
        b.build_subtracted(frame, [positions], psf, 2.0, flux=[np.array([1.0])])
    with pytest.raises(ValueError, match="cells\\[0\\] has shape \\(3,\\) for the 2 stars"):
        b.build_subtracted(frame, [positions], psf, 2.0, flux=flux, cells=[np.zeros(3, np.int32)])
    with pytest.raises(ValueError, match="the stars have 2 entries for 1 frames"):
        b.build_subtracted(frame, [positions, positions], psf, 2.0, flux=flux * 2)
    with pytest.raises(ValueError, match="keep\\[0\\] has shape \\(3,\\) for the 2 stars"):
        b.build_subtracted(frame, [positions], psf, 2.0, flux=flux, keep=[np.ones(3, bool)])
    with pytest.raises(ValueError, match="keep has 2 entries for 1 frames"):
        b.build_subtracted(frame, [positions], psf, 2.0, flux=flux, keep=[np.ones(2, bool)] * 2)
    with pytest.raises(TypeError, match="keep\\[0\\] must be booleans"):
        b.build_subtracted(frame, [positions], psf, 2.0, flux=flux, keep=[np.array([0, 1])])
    with pytest.raises(ValueError, match="not finite or not inside"):
        b.build_subtracted(frame, [np.array([[10.0, np.nan]])], psf, 2.0, flux=[np.array([1.0])])
    with pytest.raises(rp.PSFBuilderError, match="Unknown method mode"):
        b.build_subtracted(frame, [positions], psf, 2.0, flux=flux, average_method="mode")
    with pytest.raises(rp.IncorrectShapeError, match="the model must be a cube"):
        b.build_subtracted(frame, [positions], rp.IndexedCube([(0, 0)], np.ones((1, 3, 3))), 1.0, flux=flux)
    with pytest.raises(rp.IncorrectShapeError, match="must be 3D"):
        b.build_subtracted(np.zeros(10), [positions], psf, 2.0, flux=flux)
    # a wide builder, a scaled build, a model on another device
    for method, args in ((rp.ArrayPSFBuilder(129).build_subtracted, (frame, [positions], psf, 2.0)),
                         (rp.ArrayPSFBuilder(200).build_iterative, (frame, [positions], 2.0))):
        with pytest.raises(NotImplementedError, match="stops at 128 pixels"):
            method(*args)
    for scale in (2, 1):  # the keyword itself is refused, whatever its value
        with pytest.raises(NotImplementedError, match="interpolation_scale"):
            rp.ArrayPSFBuilder(8, interpolation="device").build_iterative(frame, [positions], 2.0, interpolation_scale=scale)
    # the functions of the same names make the builder themselves: the same checks through them
    with pytest.raises(ValueError, match="keep has 2 entries for 1 frames"):
        rp.build_subtracted(frame, [positions], psf, 2.0, flux=flux, keep=[np.ones(2, bool)] * 2)
    with pytest.raises(NotImplementedError, match="stops at 128 pixels"):
        rp.build_subtracted(frame, [positions], psf, 2.0, flux=flux, psf_size=130)
    with pytest.raises(ValueError, match='fit must be "groups" or "stars"'):
        rp.build_iterative(frame, [positions], 2.0, psf_size=8, fit="positions")
    with pytest.raises(TypeError, match="build_iterative takes the build keywords"):
        b.build_iterative(frame, [positions], 2.0, sep_mask=None)

    class Elsewhere(rp.IndexedCube):  # an ArrayPSF keeps its samples' device beside them
        _fft_dev = (None, 3)

    with pytest.raises(ValueError, match="psf lives on device 3, the builder on device 0"):
        b.build_subtracted(frame, [positions], Elsewhere([(0, 0)], np.ones((1, 8, 8))), 2.0, flux=flux)
    for iterations in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="iterations must be an integer of at least 1"):
            b.build_iterative(frame, [positions], 2.0, iterations=iterations)
    with pytest.raises(ValueError, match='fit must be "groups" or "stars"'):
        b.build_iterative(frame, [positions], 2.0, fit="positions")


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_exist_and_are_in_the_table():
    lib = _native.lib()
    header = (bc.ROOT / "include" / "rpsf.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in _native._PROTOTYPES and getattr(lib, name).argtypes is not None
        assert f" {name}(" in header
    assert "image_processing.py:82-121" in header[header.index("NEIGHBOUR-SUBTRACTED PATCHES"):]


def test_new_entry_points_check_their_arguments_before_the_handles():
    lib = _native.lib()
    fake, model = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + 4096)  # must not be looked at before the other arguments are
    frame = np.zeros((8, 8), np.float32)
    pos, flux, cells = np.array([[3.0, 4.0]]), np.array([1.0]), np.array([0], np.int32)
    own, corners, frac, flags = np.array([0], np.int32), np.array([[0, 0]], np.int32), np.zeros((1, 2)), np.full(1, 7, np.uint8)
    f, p, x, c, o, k, s, a = (_native._ptr(v) for v in (frame, pos, flux, cells, own, corners, frac, flags))

    def host(b=fake, image=f, h=8, w=8, m=model, n_all=1, pp=p, xx=x, cc=c, radius=2.0, n=1, oo=o, kk=k, ss=s, aa=a):
        return lib.rpsf_builder_add_frame_subtracted(b, image, 0, h, w, m, n_all, pp, xx, cc, radius, n, oo, kk, ss, np.inf, 0.0, np.inf, aa)

    def device(b=fake, image=fake, h=8, w=8, m=model, n_all=1, pp=p, xx=x, cc=c, radius=2.0, n=1, oo=o, kk=k, ss=s, aa=a):
        return lib.rpsf_builder_add_frame_device_subtracted(b, image, h, w, m, n_all, pp, xx, cc, radius, n, oo, kk, ss, np.inf, 0.0, np.inf, aa)

    calls = []
    for call in (host, device):
        calls += [call(b=None), call(image=None), call(m=None), call(pp=None), call(xx=None), call(cc=None), call(oo=None), call(kk=None),
                  call(ss=None), call(aa=None), call(h=1), call(w=1), call(n=-1),
                  *(call(radius=radius) for radius in (0.0, -2.0, 64.5, np.nan, np.inf)),
                  *(call(pp=_native._ptr(np.array([[3.0, bad]]))) for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20)),
                  *(call(oo=_native._ptr(np.array([bad], np.int32))) for bad in (1, -2, 2 ** 31 - 1))]
    assert calls == [_native.E_BADARG] * len(calls)
    assert b"own[0]" in lib.rpsf_last_error() and flags[0] == 7
