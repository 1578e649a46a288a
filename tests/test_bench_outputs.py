"""bench.py's command line without a GPU: the plain run's result line (--dry-run stands in for the launches) and --dump-outputs' files,
which two builds of the project are compared by: float32 / float64 arrays, at most 64 MB in all, the same rays' records every time."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_module():
    spec = importlib.util.spec_from_file_location("rc_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run_bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=300, env=env)


def test_plain_line_carries_the_headline_keys():
    r = run_bench("--gpus", "1", "--dry-run", "--steps", "5", "--warmup", "2", "--res", "64")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 5 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["metric"] == bench_module().METRIC


def test_full_and_dump_outputs_are_options():
    r = run_bench("--help")
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    assert run_bench("--steps", "0", "--dry-run").returncode != 0


def test_dump_outputs_is_a_fixed_sample_within_64_mb(tmp_path):
    b = bench_module()
    import raycore_jl_amd as rc
    n = 2048 * 2048   # the default batch: above the sample size
    g = np.random.default_rng(3)
    hits = np.zeros(n, dtype=rc.HIT_DT)
    hits["hit"] = g.integers(0, 2, n)
    hits["t"] = g.random(n, dtype=np.float32)
    hits["primitive_id"] = np.where(hits["hit"] == 1, g.integers(0, 4096, n), 0xFFFFFFFF)
    hits["instance_id"] = g.integers(0, 256, n)
    hits["bary_u"] = g.random(n, dtype=np.float32)
    hits["bary_v"] = g.random(n, dtype=np.float32)
    first, second = tmp_path / "a", tmp_path / "b"
    b.dump_outputs(str(first), hits)
    b.dump_outputs(str(second), hits)
    names = sorted(os.listdir(first))
    assert names == sorted(os.listdir(second)) and "ray_index.npy" in names and "t.npy" in names
    assert sum(os.path.getsize(first / f) for f in names) <= 64 * 2**20
    idx = np.load(first / "ray_index.npy")
    assert len(idx) == b.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < n
    idx = idx.astype(np.int64)
    for f in names:
        a = np.load(first / f)
        assert a.dtype in (np.float32, np.float64), f
        assert np.array_equal(a, np.load(second / f)), f
        if f != "ray_index.npy":   # exactly the records of the sampled rays (u32 ids included: float64 holds them)
            assert np.array_equal(a, hits[f[:-4]][idx].astype(a.dtype)), f
    # a batch no larger than the sample is written whole
    small = hits[:1000]
    b.dump_outputs(str(tmp_path / "c"), small)
    assert np.array_equal(np.load(tmp_path / "c" / "ray_index.npy"), np.arange(1000))
    assert np.array_equal(np.load(tmp_path / "c" / "primitive_id.npy"), small["primitive_id"].astype(np.float64))
