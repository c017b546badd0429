"""bench.py's command line: `--dump-outputs` (the output of the last timed step) and the split between a plain run and `--full`."""

import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import bench
from tests.helpers import GOLDEN

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _bench(*args, timeout=600):
    done = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, timeout=timeout, cwd=str(ROOT))
    return done


def test_dump_outputs_writes_small_outputs_whole(tmp_path):
    out = np.arange(512 * 512, dtype=np.float64).reshape(512, 512)
    bench.dump_outputs(str(tmp_path / "d"), "output", out)
    got = np.load(tmp_path / "d" / "output.npy")
    assert got.dtype == np.float32 and got.shape == out.shape and np.array_equal(got, out.astype(np.float32))


def test_dump_outputs_samples_large_outputs_within_the_budget(tmp_path):
    out = np.random.default_rng(1).standard_normal((4096, 4096)).astype(np.float32)  # 67 MB: over the budget
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "output", out)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["output_sample.npy", "output_sample_index.npy"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64_000_000
    values, index = np.load(tmp_path / "a" / "output_sample.npy"), np.load(tmp_path / "a" / "output_sample_index.npy")
    assert values.dtype == np.float32 and index.dtype == np.float64 and values.shape == index.shape
    assert np.all(np.diff(index) > 0) and index[0] >= 0 and index[-1] < out.size
    assert np.array_equal(values, out.reshape(-1)[index.astype(np.int64)])
    for name in files:  # the same pixels every run
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))
    bench.dump_outputs(str(tmp_path / "r"), "output_rank0", out, share=8)  # N ranks share the budget
    assert sum(p.stat().st_size for p in (tmp_path / "r").iterdir()) <= 64_000_000 // 8


def test_steps_and_warmup_are_checked_before_any_work():
    done = _bench("--steps", "0", timeout=120)
    assert done.returncode == 2 and "--steps" in done.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_output(tmp_path):
    """Config 1 (512^2 / 32, BASELINE configs[0]): the line of a plain run carries the headline fields and none of the --full legs, and the
    dumped output is the product's result on the benchmark's inputs - the reference's own pixels (every 8th, tests/golden) within 1e-5."""
    done = _bench("--config", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"))
    assert done.returncode == 0, done.stderr[-2000:]
    line = json.loads(done.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["roofline"]["frac"] > 0
    assert not {"cpu_baseline", "parity", "verify", "e2e", "value_new_frames"} & set(line)
    out = np.load(tmp_path / "out" / "output.npy")
    assert out.dtype == np.float32 and out.shape == (512, 512)
    ref = np.load(GOLDEN / "config1_512_n32.npz")["sample"]
    assert np.abs(out[::8, ::8] - ref).max() <= 1e-5 * np.abs(ref).max()


@pytest.mark.gpu
def test_full_run_keeps_the_checks_and_extra_legs():
    done = _bench("--config", "1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu")
    assert done.returncode == 0, done.stderr[-2000:]
    line = json.loads(done.stdout.strip().splitlines()[-1])
    assert line["parity"]["max_rel"] <= 1e-5 and line["verify"]["max_error"] <= 1e-5
    assert "ms_per_step_new_frames" in line["roofline"] and "kernel_launches" in line["roofline"] and "e2e" in line
