"""Armed cost of the N x N responsibility matrix output (gw_set_fear_full) at bench.py's C3 shape:
65,536 envs of grid32 (32 x 32, N = 4, K = 2), FeAR on, random RL policy, the obs writer pipelined as bench.py runs it.

One process, one env: the step time unarmed, armed, unarmed again (HIP events around >= 200 timed
steps after a warm-up, no host sync inside), then fear_full_kernel's busy time from the per-launch
profiling spans (GW_SPAN_FEAR_FULL) and its world updates per second from gw_count_sims.  One JSON line:

    python tools/bench_fear_full.py [--steps 300] [--warmup 50] [--envs 65536] [--scenario grid32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-responsible-nav_amd")]

import torch  # noqa: E402

GW_SPAN_FEAR_FULL = 11


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
    resp = torch.zeros((E, env.N, env.N), dtype=torch.float64, device=env.device)
    sets = torch.zeros((E, env.N, env.N, 2), dtype=torch.int16, device=env.device)
    env.set_obs_async(True)
    env.reset()
    env.set_fear_full(resp, sets)  # the record buffer and both code paths exist before anything is timed
    for _ in range(args.warmup):
        env.step()
    env.set_fear_full(None, None)
    for _ in range(args.warmup):
        env.step()

    us = {}
    for name, armed in (("unarmed", False), ("armed", True), ("unarmed_again", False)):
        env.set_fear_full(resp if armed else None, sets if armed else None)
        for _ in range(10):
            env.step()
        us[name] = timed_steps(env, args.steps)

    # the kernel alone: per-launch spans and the sim counter over a few profiled armed steps
    env.set_fear_full(resp, sets)
    env.obs_fence()
    n_prof = args.profiled
    env.profile(True, reserve=16 * (n_prof + 2))
    env.profile(False)
    ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
    env.count_sims(ctr)
    before = int(ctr.item())
    env.set_fear_full(None, None)  # the step's own FeAR sims over the same number of steps, to subtract
    for _ in range(n_prof):
        env.step()
    env.obs_fence()
    torch.cuda.synchronize()
    fear_only = int(ctr.item()) - before
    env.set_fear_full(resp, sets)
    env.profile(True)
    for _ in range(n_prof):
        env.step()
    env.obs_fence()
    torch.cuda.synchronize()
    env.profile(False)
    env.count_sims(None)
    with_full = int(ctr.item()) - before - fear_only
    spans = env.profile_spans()
    env.profile_read()
    k = spans[spans[:, 0] == GW_SPAN_FEAR_FULL]
    busy_us = float((k[:, 2] - k[:, 1]).sum()) * 1e3 / max(len(k), 1)
    # the two runs of n_prof steps see different worlds, so the step's own sims differ slightly between
    # them; fear_full_kernel's exact count is bounded by 9 N .. 9 N^2 per env
    resp_sum = resp.sum(0).cpu().tolist()
    env.close()
    out = {"tool": "bench_fear_full", "scenario": args.scenario, "envs": E, "agents": env.N,
           "kernel_path": env.kernel_path,
           "timed_steps": args.steps, "us_per_step_unarmed": us["unarmed"], "us_per_step_armed": us["armed"],
           "us_per_step_unarmed_again": us["unarmed_again"],
           "armed_minus_unarmed_us": us["armed"] - 0.5 * (us["unarmed"] + us["unarmed_again"]),
           "fear_full_kernel_launches_profiled": int(len(k)), "fear_full_kernel_busy_us": busy_us,
           "sims_per_step_fear_only": fear_only / n_prof, "sims_per_step_with_full": with_full / n_prof,
           "fear_full_sims_per_step": (with_full - fear_only) / n_prof,
           "fear_full_sims_per_s_at_kernel_busy": (((with_full - fear_only) / n_prof) / (busy_us * 1e-6)
                                                   if busy_us else None),
           "resp_full_sum_last_step": resp_sum}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
