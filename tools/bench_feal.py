"""Armed cost of the per-agent FeAL output (gw_set_feal) at bench.py's C3 shape: 65,536 envs of grid32
(32 x 32, N = 4, K = 2), FeAR on, random RL policy, the obs writer pipelined as bench.py runs it.

One process, one env: the step time unarmed, armed, unarmed again (HIP events around >= 200 timed
steps after a warm-up, no host sync inside), then feal_kernel's busy time from the per-launch
profiling spans (GW_SPAN_FEAL) and its world updates per second from gw_count_sims.  One JSON line:

    python tools/bench_feal.py [--steps 300] [--warmup 50] [--envs 65536] [--scenario grid32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-responsible-nav_amd")]

import torch  # noqa: E402

GW_SPAN_FEAL = 10


def timed_steps(env, n):
    """us per step over n steps between two HIP events on the current stream."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(n):
        env.step()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1e3 / n


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--scenario", default="grid32")
    ap.add_argument("--profiled", type=int, default=20)
    args = ap.parse_args(argv)
    assert args.steps >= 200, "at least 200 timed steps"

    from marlnav.vec_env import VecGridEnv
    E = args.envs
    env = VecGridEnv(args.scenario, num_envs=E, fear=True, fear_weight=-5.0, max_steps=150, auto_reset=True, seed=42,
                     stats=True)
    feal = torch.zeros((E, env.N), dtype=torch.float64, device=env.device)
    sets = torch.zeros((E, env.N, 2), dtype=torch.int16, device=env.device)
    env.set_obs_async(True)
    env.reset()
    env.set_feal(feal, sets)  # the record buffer and both code paths exist before anything is timed
    for _ in range(args.warmup):
        env.step()
    env.set_feal(None, None)
    for _ in range(args.warmup):
        env.step()

    us = {}
    for name, armed in (("unarmed", False), ("armed", True), ("unarmed_again", False)):
        env.set_feal(feal if armed else None, sets if armed else None)
        for _ in range(10):
            env.step()
        us[name] = timed_steps(env, args.steps)

    # the kernel alone: per-launch spans and the sim counter over a few profiled armed steps
    env.set_feal(feal, sets)
    env.obs_fence()
    n_prof = args.profiled
    env.profile(True, reserve=16 * (n_prof + 2))
    env.profile(False)
    ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
    env.count_sims(ctr)
    before = int(ctr.item())
    env.set_feal(None, None)  # the step's own FeAR sims over the same number of steps, to subtract
    for _ in range(n_prof):
        env.step()
    env.obs_fence()
    torch.cuda.synchronize()
    fear_only = int(ctr.item()) - before
    env.set_feal(feal, sets)
    env.profile(True)
    for _ in range(n_prof):
        env.step()
    env.obs_fence()
    torch.cuda.synchronize()
    env.profile(False)
    env.count_sims(None)
    with_feal = int(ctr.item()) - before - fear_only
    spans = env.profile_spans()
    env.profile_read()
    k = spans[spans[:, 0] == GW_SPAN_FEAL]
    busy_us = float((k[:, 2] - k[:, 1]).sum()) * 1e3 / max(len(k), 1)
    # the two runs of n_prof steps see different worlds, so the step's own sims differ slightly between
    # them; feal_kernel's exact count is bounded by 9 (N + 1) .. 18 N per env
    mean_feal = float(feal.mean().item())
    env.close()
    out = {"tool": "bench_feal", "scenario": args.scenario, "envs": E, "agents": env.N, "kernel_path": env.kernel_path,
           "timed_steps": args.steps, "us_per_step_unarmed": us["unarmed"], "us_per_step_armed": us["armed"],
           "us_per_step_unarmed_again": us["unarmed_again"],
           "armed_minus_unarmed_us": us["armed"] - 0.5 * (us["unarmed"] + us["unarmed_again"]),
           "feal_kernel_launches_profiled": int(len(k)), "feal_kernel_busy_us": busy_us,
           "sims_per_step_fear_only": fear_only / n_prof, "sims_per_step_with_feal": with_feal / n_prof,
           "feal_sims_per_step": (with_feal - fear_only) / n_prof,
           "feal_sims_per_s_at_kernel_busy": ((with_feal - fear_only) / n_prof) / (busy_us * 1e-6) if busy_us else None,
           "mean_feal_last_step": mean_feal}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
