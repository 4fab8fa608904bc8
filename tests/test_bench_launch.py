"""bench.py's launch contract on a box without GPUs: `--gpus N` never silently runs fewer ranks."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LAUNCH_ENV = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "CPPF_BENCH_BACKEND", "CPPF_DIST_FORCE_COLLECTIVE")


def _run(argv, **env_add):
    env = {k: v for k, v in os.environ.items() if k not in _LAUNCH_ENV}
    env.update(env_add)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True,
                          timeout=300)


def test_plain_multi_gpu_invocation_fails_loudly_without_the_gpus():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("this box has the GPUs")
    r = _run(["--gpus", "2"])
    assert r.returncode == 2 and "GPU(s) are visible" in r.stderr and "{" not in r.stdout


def test_world_size_must_equal_gpus():
    r = _run(["--gpus", "1"], WORLD_SIZE="2", RANK="0")
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr and "{" not in r.stdout
    r = _run(["--gpus", "4"], WORLD_SIZE="2", RANK="1")
    assert r.returncode == 2 and "{" not in r.stdout


def test_steps_must_be_positive():
    r = _run(["--gpus", "1", "--steps", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr and "{" not in r.stdout


def test_dump_outputs_writes_every_record_field(tmp_path):
    """--dump-outputs DIR: one DIR/<field>.npy per field of the 160-byte scene record, float32 or float64, values exact."""
    import importlib.util
    import numpy as np
    from cppf2_amd.pipeline import RESULT_DTYPE
    spec = importlib.util.spec_from_file_location("bench_for_dump_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(0)
    rec = np.zeros(5, RESULT_DTYPE)
    for name in RESULT_DTYPE.names:
        a = rec[name]
        rec[name] = rng.standard_normal(a.shape) if a.dtype.kind == "f" else rng.integers(0, 1 << 24, a.shape)
    for workload in ("shot", "ensemble"):
        d = tmp_path / workload
        bench.dump_outputs(str(d), rec, workload)
        want = [n for n in RESULT_DTYPE.names if n != "pad_"] + (["pick"] if workload == "ensemble" else [])
        assert sorted(f.name for f in d.iterdir()) == sorted(n + ".npy" for n in want)
        for n in want:
            got = np.load(d / (n + ".npy"))
            src = rec["pad_"][:, 0] if n == "pick" else rec[n]
            assert got.dtype in (np.float32, np.float64) and got.shape == src.shape
            assert np.array_equal(got, src) and got.dtype == (np.float32 if src.dtype == np.float32 else np.float64)
