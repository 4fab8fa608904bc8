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


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_plain_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_switches_off_every_leg_beside_the_headline_loop():
    """Without --full, bench.py runs the headline loop alone: every leg with a --no-* switch is off and the CPU legs take no scenes;
    --full leaves the defaults (every leg on) as they were."""
    from cppf2_amd.benchlib import launch
    bench = _bench_module()
    legs = ("no_reference_order", "no_native_arith", "no_f16x2", "no_evidence", "no_counters", "no_voxel_density", "no_prior_variants",
            "no_launch_power")
    full = launch.parse(["--full"])
    assert full.full and not any(getattr(full, k) for k in legs) and full.cpu_scenes == 3
    a = launch.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full
    bench.plain_run(a)
    assert all(getattr(a, k) for k in legs) and a.cpu_scenes == 0
    # the headline loop itself is untouched: its workload, stream mode and K / W
    assert (a.steps, a.warmup, a.scenes_per_gpu, a.single_stream, a.streams, a.workload) == (7, 2, 64, False, 2, "shot")


def test_plain_line_holds_the_contract_fields():
    """report.report_plain: the contract fields as the --full line states them (value = scenes of the K timed steps / their seconds,
    ms_per_step, metric, unit, dtype), the records' hash and the poses against the ground truth -- and none of the figures that take
    runs of their own."""
    import hashlib
    import types
    import numpy as np
    from cppf2_amd.benchlib import launch, report
    from cppf2_amd.pipeline import RESULT_DTYPE
    B, world, steps = 3, 1, 5
    rec = np.zeros(B, RESULT_DTYPE)
    rec["R"] = np.eye(3)
    rec["t"] = [[0.0, 0.0, 0.8], [0.1, 0.0, 0.9], [0.0, 0.3, 0.7]]
    scenes = [{"t": rec["t"][b] + (0.001 if b < 2 else 0.2), "R": np.eye(3)} for b in range(B)]     # the third one is 20 cm off
    pipe = types.SimpleNamespace(results_to_numpy=lambda r=None: rec.copy())
    step = types.SimpleNamespace(B=B, N=4096, T=20000, cloud="synthetic", scenes=scenes, pipe=pipe, all_records=object())
    args = launch.parse(["--steps", str(steps), "--warmup", "0"])
    dt = 0.125
    line = report.report_plain(args, step, world, None, dt, {"median": 12.5}, {"gather": 0.01})
    assert line == {**report.headline_fields(args, step, world, dt), **line}
    assert line["metric"] == "scenes/sec (1/2/4/8 GPU) at 4096 pts x 20k tuples; 5deg5cm match vs ref"
    assert line["value"] == B * world * steps / dt and line["ms_per_step"] == 1e3 * dt / steps
    assert (line["unit"], line["higher_is_better"], line["dtype"], line["steps"], line["warmup"]) == ("scenes/s", True, "f32", steps, 0)
    assert line["full"] is False and line["records_gathered"] == B and line["step_interval_ms"] == {"median": 12.5}
    assert line["records_sha256"] == hashlib.sha256(rec.tobytes()).hexdigest() == line["collective"]["records_sha256"]
    assert line["pose_5deg5cm_vs_gt"] == 2 / 3
    assert not {"roofline", "cpu_baseline", "oracle_agreement", "two_streams", "value_single_stream", "ok"} & set(line)
