"""bench.py contract pieces that need no GPU: the metric matches BASELINE.json, the byte
accounting behind roofline.achieved, the CLI parses."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_metric_is_baseline_metric():
    with open(os.path.join(REPO, "BASELINE.json")) as f:
        assert bench.METRIC == json.load(f)["metric"]


def test_algorithmic_bytes():
    step_b, obs_b = bench.algorithmic_bytes(4, 2, 32 * 32)       # C3
    assert obs_b == 4 * 2 * 1024 + 20 and step_b == 205
    assert bench.algorithmic_bytes(4, 2, 1024, obs_bytes=2)[1] == 2 * 2 * 1024 + 20
    assert bench.algorithmic_bytes(8, 2, 64 * 64)[1] == 4 * 2 * 4096 + 20   # C4


def test_configs_name_the_baseline_workloads():
    assert {"c1", "c2", "c3", "c4", "c5"} <= set(bench.CONFIGS)
    c3 = bench.CONFIGS["c3"]
    assert c3["envs"] == 65536 and c3["scenario"] == "grid32" and c3["fear"]


def test_cli_help_without_gpu():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--steps" in r.stdout and "--obs-dtype" in r.stdout
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_dump_outputs_formats_and_budget(tmp_path):
    """--dump-outputs: float64 stays float64, integers of 32 bits or more become float64 (exact),
    everything else float32; None entries are the caller's to drop; an array above its share of
    the budget is cut to the same seeded sample of its envs on every call, indices beside it."""
    import numpy as np
    import torch
    E, K = 4096, 2
    g = torch.Generator().manual_seed(3)
    obs = torch.randint(-2, 3, (K, E, 8, 8), generator=g).to(torch.bfloat16)
    tensors = {"obs": obs,
               "reward": torch.randn(E, K, generator=g, dtype=torch.float64),
               "done": torch.randint(0, 2, (E,), generator=g).to(torch.uint8),
               "mask": torch.randint(0, 512, (E, K), generator=g).to(torch.int16),
               "desc_copy": torch.randint(-2 ** 31, 2 ** 31 - 1, (E, 12), generator=g).to(torch.int32)}
    budget = 1 << 20  # obs alone is 2 MB as float32: it is the only array sampled
    shapes = bench.dump_outputs(str(tmp_path / "a"), tensors, E, budget=budget)
    again = bench.dump_outputs(str(tmp_path / "b"), tensors, E, budget=budget)
    assert shapes == again
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted([n + ".npy" for n in tensors] + ["obs_envs.npy"])
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert sum(a.nbytes for a in got.values()) <= budget
    for f in files:
        assert np.array_equal(got[f[:-4]], np.load(tmp_path / "b" / f))
    assert {n: a.dtype.name for n, a in got.items()} == {
        "obs": "float32", "obs_envs": "float64", "reward": "float64", "done": "float32", "mask": "float32",
        "desc_copy": "float64"}
    for n in ("reward", "done", "mask", "desc_copy"):  # whole and exact
        assert np.array_equal(got[n], tensors[n].numpy().astype(got[n].dtype)), n
    envs = got["obs_envs"].astype(np.int64)
    assert 0 < len(envs) < E and np.all(np.diff(envs) > 0) and shapes["obs"] == [K, len(envs), 8, 8]
    assert np.array_equal(got["obs"], obs.float().numpy()[:, envs])


def test_profiled_steps_need_full():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--profile-steps", "8"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr


def test_launch_plan_one_rank_per_gpu():
    """`bench.py --gpus N` without a launcher starts N copies of itself with torchrun's variables
    (the plan only: nothing is started and no GPU is touched here)."""
    argv = ["--gpus", "4", "--steps", "20", "--warmup", "5"]
    plans = bench.launch_plan(4, argv, {"PATH": "/bin", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}, 29511)
    assert len(plans) == 4
    for r, (cmd, env) in enumerate(plans):
        assert cmd[0] == sys.executable and cmd[1] == os.path.join(REPO, "bench.py") and cmd[2:] == argv
        assert (env["RANK"], env["LOCAL_RANK"], env["WORLD_SIZE"]) == (str(r), str(r), "4")
        assert env["MASTER_ADDR"] == "127.0.0.1" and env["MASTER_PORT"] == "29511"
        assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and env["PATH"] == "/bin"


def test_busy_time_merges_overlapping_launches():
    spans = [(1, 0.0, 1.4), (1, 1.0, 2.4), (0, 0.0, 0.2), (1, 2.0, 3.4), (1, 5.0, 6.0)]
    total, n = bench.busy_ms(spans, 1)
    assert n == 4 and abs(total - (3.4 + 1.0)) < 1e-12
    assert bench.busy_ms(spans, 0) == (0.2, 1)
    assert bench.busy_ms([], 1) == (0.0, 0)
