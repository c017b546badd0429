"""Group fits (DESIGN.md 3.7 "Group fits", kernel S11) without a GPU: the host grouping (csrc/rpsf_core_stars_group.hpp) against SciPy,
the kernel's driver (csrc/rpsf_core_stars_fit_group.hpp) on the CPU emulator against the float64 restatement (tests/group_cases.py), bit
for bit - the cases and checks tests/test_gpu_group.py runs on the GPU - plus what is host code in the product: fit_groups, star_groups,
the derived fields and the C ABI's return codes."""

import ctypes
import inspect
import pathlib
import shutil
import struct
import subprocess

import numpy as np
import pytest

import regularizepsf_amd as rp
from regularizepsf_amd import _native, stars
from tests import fit_cases as fc
from tests import group_cases as gc

NEW_SYMBOLS = ("rpsf_stars_link_groups", "rpsf_stars_fit_groups", "rpsf_stars_fit_groups_ms", "rpsf_stars_fit_groups_info")
NEW_FUNCTIONS = (stars.fit_groups, stars.star_groups, stars.group_fit_dtype, stars.group_fit_from_sums, stars.fit_groups_info)
FAKE = 0x7F0000000000  # a handle nobody dereferences


# ------------------------------------------------------------------------------------------------------------------ the grouping
def _library_groups(positions, eligible, link, max_group):
    got = stars.star_groups(np.asarray(positions, np.float64).reshape(-1, 2), link, max_group=max_group, eligible=eligible)
    return got["group"], got["group_size"], got["crowded"]


def test_the_grouping_matches_scipy_on_the_emulator():
    gc.check_grouping(gc.emu_link)


def test_the_grouping_matches_scipy_in_the_library():
    gc.check_grouping(_library_groups)


def test_the_grouping_under_the_host_sanitizers(tmp_path):
    """The grouping code and the driver of S11 as a plain program with a main of its own (tests/emu/emu_group.cpp, EMU_GROUP_MAIN) under
    -fsanitize=address,undefined, on check_grouping's inputs; it also runs a small group fit, whose flags it checks itself."""
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not pathlib.Path(clang).exists():
        clang = shutil.which("clang++") or shutil.which("hipcc")
    assert clang is not None
    program = tmp_path / "emu_group_sanitized"
    built = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DEMU_GROUP_MAIN",
                            str(gc.ROOT / "tests" / "emu" / "emu_group.cpp"), "-o", str(program)], capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitizer" in built.stderr):
        pytest.skip("the host compiler cannot link the sanitizers' runtimes: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr[-2000:]
    runs = []

    def sanitized(positions, eligible, link, max_group):
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        n = len(positions)
        flags = np.ones(n, np.uint8) if eligible is None else np.ascontiguousarray(np.asarray(eligible, bool), np.uint8)
        (tmp_path / "in.bin").write_bytes(struct.pack("<qdqq", n, float(link), int(max_group), int(eligible is not None)) + positions.tobytes()
                                          + flags.tobytes())
        done = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
        assert done.returncode == 0, (done.returncode, done.stdout[-500:], done.stderr[-3000:])
        runs.append(done.stdout)
        raw = (tmp_path / "out.bin").read_bytes()
        assert len(raw) == 9 * n
        return np.frombuffer(raw[:4 * n], np.int32), np.frombuffer(raw[4 * n:8 * n], np.int32), np.frombuffer(raw[8 * n:], np.uint8) != 0

    gc.check_grouping(sanitized)
    assert runs and all("1 grouping problems" in out and "flags seen 23" in out for out in runs)


def test_star_groups_is_exported_and_checks_its_arguments():
    assert "star_groups" in rp.__all__ and rp.star_groups is stars.star_groups
    parameters = inspect.signature(rp.star_groups).parameters
    assert list(parameters)[:3] == ["stars", "link", "max_group"] and parameters["max_group"].default == 8
    assert parameters["max_group"].kind is inspect.Parameter.KEYWORD_ONLY
    got = rp.star_groups(np.array([(0.0, 0.0), (3.0, 4.0), (9.0, 9.0)]), 5.0)
    assert got.dtype == stars.GROUP_DTYPE and got["group"].tolist() == [0, 0, 2] and got["group_size"].tolist() == [2, 2, 1] and not got["crowded"].any()
    catalogue = np.zeros(3, [("row", np.float64), ("col", np.float64), ("flux", np.float64)])
    catalogue["row"], catalogue["col"] = [0.0, 3.0, 9.0], [0.0, 4.0, 9.0]
    assert rp.star_groups(catalogue, 5.0).tobytes() == got.tobytes()  # catalogues are taken by row / col
    assert rp.star_groups(np.zeros((0, 2)), 1.0).shape == (0,)
    assert rp.star_groups(np.zeros((3, 2)), 1.0, max_group=2)["crowded"].all()
    for link in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="link must be positive and finite"):
            rp.star_groups(np.zeros((2, 2)), link)
    with pytest.raises(TypeError, match="link must be a number"):
        rp.star_groups(np.zeros((2, 2)), "near")
    for max_group in (0, 9, -1):
        with pytest.raises(ValueError, match="max_group must lie in 1 ... 8"):
            rp.star_groups(np.zeros((2, 2)), 1.0, max_group=max_group)
    for max_group in (2.0, True, "8"):
        with pytest.raises(TypeError, match="max_group must be an integer"):
            rp.star_groups(np.zeros((2, 2)), 1.0, max_group=max_group)
    with pytest.raises(ValueError, match="not finite or not inside"):
        rp.star_groups(np.array([(0.0, 2.0 ** 20)]), 1.0)
    with pytest.raises(ValueError, match="eligible has 1 entries for 2 stars"):
        rp.star_groups(np.zeros((2, 2)), 1.0, eligible=[True])


# ------------------------------------------------------------------------------------------------------------------ S11 on the emulator
@pytest.mark.parametrize("name", tuple(gc.CROWD_CASES) + tuple(gc.MASKED_CASES) + tuple(gc.OTHER_CASES) + tuple(gc.COUNT_CASES))
def test_the_group_fit_matches_the_restatement_bit_for_bit(name):
    gc.check_case(gc.EmuFinder, gc.EmuModel, name)


def test_the_crowd_is_grouped_as_laid_out():
    gc.check_crowd_groups(gc.EmuFinder, gc.EmuModel)


def test_every_flag_fires():
    gc.check_every_flag_fires(gc.EmuFinder, gc.EmuModel)


def test_group_counts_around_a_workgroup():
    gc.check_group_counts(gc.EmuFinder, gc.EmuModel, gc.emulator_info()[0])


def test_the_members_sums_are_fit_stars_and_stars_alone_are_its_rows():
    gc.check_against_fit(gc.EmuFinder, gc.EmuModel)


def test_the_residual_is_subtract_stars():
    gc.check_against_render(gc.EmuFinder, gc.EmuModel)


def test_the_fluxes_against_an_independent_solve():
    assert gc.check_against_lstsq(gc.EmuFinder, gc.EmuModel) <= 1.0


@pytest.mark.parametrize("name", ("crowd, N = 16, mesh, flux and background", "masked crowd, mesh, flux alone", "9 groups"))
def test_repeats_are_bit_equal(name):
    gc.check_reproducible(gc.EmuFinder, gc.EmuModel, name)


def test_the_other_kernels_are_untouched_and_a_model_serves_two_finders():
    gc.check_isolation(gc.EmuFinder, gc.EmuModel)


def test_state_and_argument_errors():
    gc.check_errors(gc.EmuFinder, gc.EmuModel, gc.EmuError)


def test_the_records_fit_the_lds_of_a_plain_launch():
    """s11_lds_bytes(): 256 lane records and 32 group records of 18 doubles (pass 1's 54 sums fold 18 at a time), one 64-bit index and two
    ints, then per wave 54 totals, the 9 x 9 matrix, the right-hand side, the unknowns and the constant, and four ints."""
    waves, _, _, size, max_group, columns = gc.emulator_info()
    assert (waves, max_group, columns) == (4, 8, 25)
    state = (waves * ((54 + 81 + 9 + 9 + 1) * 8 + 4 * 4) + 15) // 16 * 16
    assert size == (256 + 8 * waves) * (18 * 8 + 8 + 2 * 4) + state == 51072 and size % 16 == 0 and size <= 64 * 1024
    assert stars.fit_groups_info() == (columns, max_group, waves)  # (host code of the library: no GPU needed)


def test_the_ordered_sum_runs_on_across_boxes():
    rng = np.random.default_rng([14, 67])
    one, two = rng.normal(0.0, 1.0, 90) * 10.0 ** rng.uniform(-8, 8, 90), rng.normal(0.0, 1.0, 70)
    assert gc.ordered_sum_boxes([one]) == fc.ordered_sum(one) and gc.ordered_sum_boxes([]) == 0.0
    lanes = np.zeros(64)
    for terms in (one, two):
        padded = np.zeros(128)
        padded[:len(terms)] = terms
        lanes = lanes + padded[:64]
        lanes = lanes + padded[64:]
    want = np.float64(0.0)
    for group in lanes.reshape(8, 8):  # 8 groups of 8 lanes, each in lane order, then the 8 in order
        partial = np.float64(0.0)
        for value in group:
            partial = partial + value
        want = want + partial
    assert gc.ordered_sum_boxes([one, two]) == want
    # not the sum of the boxes laid end to end: a second box starts at lane 0 again.  Lane 0 takes 1e16, then the second box's 1.0, which
    # is lost; laid end to end the 1.0 falls to lane 90 % 64 = 26 and survives, and - 1e16 (index 128) meets 1e16 in lane 0
    one, two = np.zeros(90), np.zeros(39)
    one[0], two[0], two[38] = 1e16, 1.0, -1e16
    assert gc.ordered_sum_boxes([one, two]) == 0.0 and fc.ordered_sum(np.concatenate([one, two])) == 1.0


def test_the_joint_fit_recovers_what_the_single_fit_does_not():
    """The truth test, on the restatement alone: the figures the bounds were fixed from (group_cases.MEASURED_*), to their printed
    precision."""
    error, factor = gc.check_truth()
    assert abs(error - gc.MEASURED_GROUP_ERROR) <= 5e-6 and abs(factor - gc.MEASURED_SINGLE_FACTOR) <= 0.05


def test_the_truth_on_the_emulator(monkeypatch):
    monkeypatch.setattr(stars, "_Finder", gc.EmuFinder)
    monkeypatch.setattr(stars, "_Model", gc.EmuModel)
    gc.check_truth(rp.fit_groups, rp.fit_stars, "fit_groups on the emulator")


# ------------------------------------------------------------------------------------------------------------------ host derivations
def test_derived_fields_on_hand_made_rows():
    s8 = [10.0, 20.0, 3, 0, 6, 9, 0.5, 0.625, 0.0625, 30.0, 4.0, 200.0, -8.0, 1.5, 16.0, 2.0, 1.25, -1.25, 11.0, 19.0]
    rows = np.array([s8 + [4, 3, 20, 64.0, 7.0], s8 + [1, 1, 6, 16.0, 2.0], s8 + [0, 9, 6, 16.0, 2.0]])
    got = stars.group_fit_from_sums(rows)
    assert got.dtype == stars.group_fit_dtype() and got.shape == (3,)
    single = stars.fit_from_sums(rows[:, :20])
    for name in stars.FIT_FIELDS:
        assert got[name].tobytes() == single[name].tobytes(), name
    assert got["group"].tolist() == [4, 1, 0] and got["group_size"].tolist() == [3, 1, 9] and got["group_n"].tolist() == [20, 6, 6]
    assert got["group_dof"].tolist() == [16, 4, 4] and got["crowded"].tolist() == [False, False, True]  # 20 - (3 + 1); alone: S8's dof
    assert got["group_chi2"].tolist() == [64.0, 16.0, 16.0] and got["group_rms"].tolist() == [2.0, 2.0, 2.0] and got["group_abs_res"].tolist() == [7.0, 2.0, 2.0]
    assert got["dof"].tolist() == [4, 4, 4]  # the per-star dof stays S8's nominal n_use - 2
    alone = stars.group_fit_from_sums(rows, fit_background=False, max_group=2)
    assert alone["group_dof"].tolist() == [19, 5, 5] and alone["crowded"].tolist() == [True, False, True] and alone["dof"].tolist() == [5, 5, 5]
    few = stars.group_fit_from_sums(np.array([s8 + [0, 2, 3, np.nan, np.nan]]))
    assert few["group_dof"][0] == 0 and np.isnan(few["group_rms"][0])
    empty = stars.group_fit_from_sums(np.zeros((0, len(stars.GROUP_COLUMNS))))
    assert empty.shape == (0,) and empty.dtype == stars.group_fit_dtype()


def test_fit_groups_is_exported_and_says_what_it_is_not():
    assert "fit_groups" in rp.__all__ and rp.fit_groups is stars.fit_groups
    parameters = inspect.signature(rp.fit_groups).parameters
    assert list(parameters) == ["images", "stars", "psf", "radius", "mask", "background", "box", "fit_background", "cells", "link", "max_group",
                                "device"]
    assert [parameters[n].default for n in ("mask", "background", "box", "fit_background", "cells", "link", "max_group", "device")] == [
        None, "mesh", 64, True, None, None, 8, 0]
    assert all(parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("background", "box", "fit_background", "cells", "link", "max_group", "device"))
    text = stars.fit_groups.__doc__
    assert "NOT a PSF-photometry" in text and "uniform" in text and "positions are fixed" in text and "bilinear" in text
    assert "cut at ``R``" in text and "cell of a star is fixed" in text and "near-singular" in text and "opposite sign" in text
    assert "``DEGENERATE`` at a non-positive pivot" in text and "nominal ``n_use - 2``" in text
    dtype = stars.group_fit_dtype()
    assert dtype.names[:len(stars.FIT_FIELDS)] == stars.FIT_FIELDS and all(dtype[n] == stars.fit_dtype()[n] for n in stars.FIT_FIELDS)
    assert dtype.names[len(stars.FIT_FIELDS):] == ("group", "group_size", "group_n", "group_dof", "group_chi2", "group_rms", "group_abs_res", "crowded")
    assert all(dtype[n] == np.int32 for n in ("group", "group_size", "group_n", "group_dof")) and dtype["crowded"] == np.bool_
    assert len(stars.GROUP_COLUMNS) == gc.COLUMNS and (stars.CROWDED, stars.MAX_GROUP) == (gc.CROWDED, gc.MAX_GROUP) == (16, 8)


def test_fit_groups_on_the_emulator(monkeypatch):
    """fit_groups with the emulator behind it: the forms of its arguments, its relation to fit_stars, and subtract_stars and
    cell_fit_summary on its result."""
    monkeypatch.setattr(stars, "_Finder", gc.EmuFinder)
    monkeypatch.setattr(stars, "_Model", gc.EmuModel)
    frame = fc.field()["frame"]
    positions, cells = gc.crowd()
    positions, cells = positions[:18], cells[:18]  # the pairs, the chain, the group of 8 and three more
    coordinates = [tuple(int(v) for v in c) for c in rp.calculate_covering(fc.SHAPE, 8)]
    cube = np.broadcast_to(fc.model(8)[fc.GAUSSIAN], (len(coordinates), 8, 8)).copy()
    psf = rp.IndexedCube(coordinates, cube)
    one = rp.fit_groups(frame, positions, psf, 2.5, box=16)
    assert isinstance(one, list) and len(one) == 1 and one[0].dtype == stars.group_fit_dtype() and one[0].shape == (18,)
    assert one[0]["group_size"].tolist() == gc.CROWD_SIZES[:18] and np.all(one[0]["flags"] == 0) and not one[0]["crowded"].any()
    assert one[0]["cell"].tolist() == stars.nearest_cells(positions, coordinates, 8).tolist()
    single = rp.fit_stars(frame, positions, psf, 2.5, box=16)[0]
    for name in ("row", "col", "cell", "n_use", "n_all", "coverage", "sm", "sm_all", "smm", "sd", "sdm", "sdd", "dof"):
        assert one[0][name].tobytes() == single[name].tobytes(), name
    alone = one[0]["group_size"] == 1
    assert all(one[0][name][alone].tobytes() == single[name][alone].tobytes() for name in stars.FIT_FIELDS)
    assert np.all(one[0]["flux"][~alone] != single["flux"][~alone])
    assert np.all(one[0]["group_dof"] == one[0]["group_n"] - one[0]["group_size"] - 1) and np.all(one[0]["dof"] == one[0]["n_use"] - 2)
    for options in ({"max_group": 1}, {"link": 0.25}):  # every star alone: fit_stars, field for field
        lonely = rp.fit_groups(frame, positions, psf, 2.5, box=16, **options)[0]
        assert all(lonely[name].tobytes() == single[name].tobytes() for name in stars.FIT_FIELDS), options
        assert np.all(lonely["crowded"] == (lonely["group_size"] > 1)) and np.all(lonely["group_n"] == lonely["n_use"])
    for form in ([positions], [positions.tolist()], np.ascontiguousarray(positions)):
        assert rp.fit_groups(frame, form, psf, 2.5, box=16)[0].tobytes() == one[0].tobytes()
    assert rp.fit_groups(frame, positions, psf, 2.5, box=16, link=5.0)[0].tobytes() == one[0].tobytes()  # link=None is 2 R
    assert rp.fit_groups(frame, one, psf, 2.5, box=16)[0].tobytes() == one[0].tobytes()  # its own output is taken by row / col
    stack = rp.fit_groups(np.stack([frame, frame]), [positions, positions[:0]], psf, 2.5, box=16)
    assert stack[0].tobytes() == one[0].tobytes() and stack[1].shape == (0,) and stack[1].dtype == stars.group_fit_dtype()
    # subtract_stars and cell_fit_summary take the new array as it is
    flat = rp.fit_groups(frame, positions, psf, 2.5, box=16, background="none", fit_background=False)
    residual = rp.subtract_stars(frame, flat, psf, 2.5, dtype=np.float64)[0]
    at = (flat[0]["peak_row"].astype(int), flat[0]["peak_col"].astype(int))
    assert fc.same_bits(residual[at], flat[0]["peak_e"])
    summary = rp.cell_fit_summary(one, psf)
    assert summary["count"].sum() == 18 and summary.tobytes() == rp.cell_fit_summary([stars.fit_from_sums(np.zeros((0, 20)))] + one, psf).tobytes()


def test_argument_errors():
    frame, stars_ = np.zeros((40, 48), np.float32), [np.array([[10.0, 12.0], [11.0, 13.0]])]
    psf = rp.IndexedCube([(0, 0)], np.ones((1, 8, 8)))
    for radius in (0.0, -1.0, 3.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="radius must lie in 0 < R <= min\\(64, N / 2 - 1\\) = 3 for cells of 8"):
            rp.fit_groups(frame, stars_, psf, radius)
    for link in (0.0, -1.0, 6.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="link must lie in 0 < link <= 2 R = 6"):
            rp.fit_groups(frame, stars_, psf, 3.0, link=link)
    with pytest.raises(TypeError, match="link must be a number"):
        rp.fit_groups(frame, stars_, psf, 3.0, link="wide")
    for max_group in (0, 9, -3):
        with pytest.raises(ValueError, match="max_group must lie in 1 ... 8"):
            rp.fit_groups(frame, stars_, psf, 3.0, max_group=max_group)
    for max_group in (4.0, None, False):
        with pytest.raises(TypeError, match="max_group must be an integer"):
            rp.fit_groups(frame, stars_, psf, 3.0, max_group=max_group)
    with pytest.raises(TypeError, match="fit_background must be True or False"):
        rp.fit_groups(frame, stars_, psf, 1.0, fit_background=1)
    with pytest.raises(ValueError, match='background must be "mesh" or "none"'):
        rp.fit_groups(frame, stars_, psf, 1.0, background="annulus")
    with pytest.raises(ValueError, match="stars has 2 entries for 1 frames"):
        rp.fit_groups(frame, stars_ * 2, psf, 1.0)
    with pytest.raises(ValueError, match="not finite or not inside"):
        rp.fit_groups(frame, [np.array([[10.0, np.nan]])], psf, 1.0)
    with pytest.raises(ValueError, match="cells\\[0\\] has shape \\(1,\\) for the 2 stars"):
        rp.fit_groups(frame, stars_, psf, 1.0, cells=[[0]])
    with pytest.raises(rp.IncorrectShapeError, match="the model must be a cube"):
        rp.fit_groups(frame, stars_, rp.IndexedCube([(0, 0)], np.ones((1, 3, 3))), 1.0)


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_exist_and_are_in_the_table():
    lib = _native.lib()
    header = (gc.ROOT / "include" / "rpsf.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in _native._PROTOTYPES and getattr(lib, name).argtypes is not None
        assert f" {name}(" in header
    for line in ("#define RPSF_STARS_FIT_GROUPS_COLUMNS 25\n", "#define RPSF_STARS_MAX_GROUP 8\n", "#define RPSF_STARS_FIT_CROWDED 16\n"):
        assert line in header


def test_new_entry_points_check_their_arguments_before_the_handles():
    lib = _native.lib()
    fake, fake_model = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + 4096)  # must not be looked at before the other arguments are
    pos, cells, out, ms = np.array([[3.0, 4.0]]), np.array([0], np.int32), np.full(gc.COLUMNS, -1.0), ctypes.c_double(-1.0)
    p, c, o = _native._ptr(pos), _native._ptr(cells), _native._ptr(out)
    labels, sizes, crowded = np.full(1, -1, np.int32), np.full(1, -1, np.int32), np.full(1, 7, np.uint8)
    l, s, w = _native._ptr(labels), _native._ptr(sizes), _native._ptr(crowded)
    calls = [
        lib.rpsf_stars_fit_groups(None, fake_model, 1, p, c, 2.0, 1, 1, 4.0, 8, o),
        lib.rpsf_stars_fit_groups(fake, None, 1, p, c, 2.0, 1, 1, 4.0, 8, o),
        lib.rpsf_stars_fit_groups(None, None, 0, None, None, 2.0, 1, 1, 4.0, 8, None),
        lib.rpsf_stars_fit_groups(fake, fake_model, 1, None, c, 2.0, 1, 1, 4.0, 8, o),
        lib.rpsf_stars_fit_groups(fake, fake_model, 1, p, None, 2.0, 1, 1, 4.0, 8, o),
        lib.rpsf_stars_fit_groups(fake, fake_model, 1, p, c, 2.0, 1, 1, 4.0, 8, None),
        *(lib.rpsf_stars_fit_groups(fake, fake_model, 1, p, c, radius, 1, 1, 1.0, 8, o) for radius in (0.0, -2.0, 64.5, np.nan, np.inf)),
        *(lib.rpsf_stars_fit_groups(fake, fake_model, 1, p, c, 2.0, fit_background, 1, 4.0, 8, o) for fit_background in (2, -1)),
        *(lib.rpsf_stars_fit_groups(fake, fake_model, 1, p, c, 2.0, 1, 1, link, 8, o) for link in (0.0, -1.0, 4.5, np.nan, np.inf)),
        *(lib.rpsf_stars_fit_groups(fake, fake_model, 1, p, c, 2.0, 1, 1, 4.0, max_group, o) for max_group in (0, 9, -1)),
        *(lib.rpsf_stars_fit_groups(fake, fake_model, 1, _native._ptr(np.array([[3.0, bad]])), c, 2.0, 0, 0, 4.0, 8, o)
          for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20)),
        lib.rpsf_stars_fit_groups_ms(None, ctypes.byref(ms)),
        lib.rpsf_stars_fit_groups_ms(fake, None),
        lib.rpsf_stars_link_groups(1, None, None, 1.0, 8, l, s, w),
        lib.rpsf_stars_link_groups(1, p, None, 1.0, 8, None, s, w),
        lib.rpsf_stars_link_groups(1, p, None, 1.0, 8, l, None, w),
        lib.rpsf_stars_link_groups(1, p, None, 1.0, 8, l, s, None),
        *(lib.rpsf_stars_link_groups(1, p, None, link, 8, l, s, w) for link in (0.0, -1.0, np.nan, np.inf)),
        *(lib.rpsf_stars_link_groups(1, p, None, 1.0, max_group, l, s, w) for max_group in (0, 9)),
        lib.rpsf_stars_link_groups(1, _native._ptr(np.array([[np.nan, 0.0]])), None, 1.0, 8, l, s, w),
    ]
    assert calls == [_native.E_BADARG] * len(calls)
    assert np.all(out == -1.0) and ms.value == -1.0 and labels[0] == -1 and sizes[0] == -1 and crowded[0] == 7
    assert lib.rpsf_stars_link_groups(0, None, None, 1.0, 8, None, None, None) == 0  # nothing to group needs no pointers
    assert lib.rpsf_stars_link_groups(1, p, None, 1.0, 8, l, s, w) == 0 and (labels[0], sizes[0], crowded[0]) == (0, 1, 0)
    assert lib.rpsf_stars_fit_groups_info(None, None, None) == 0
