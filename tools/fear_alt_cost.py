#!/usr/bin/env python3
"""Per-step cost of the per-action FeAR table (VecGridEnv(fear_alt=True), gw_set_fear_alt).

For each batch size: the same env (grid32, FeAR on, random RL policy on device, pipelined obs as
bench.py's C3 line) stepped with the table off and on, timed with HIP events around ``--steps``
steps after ``--warmup`` steps, and the FeAR sims per second from gw_count_sims over a second,
equally long run (the counter's atomics stay out of the timed one).  One JSON line per run.

  python tools/fear_alt_cost.py [--envs 65536 4096] [--steps 100] [--warmup 20] [--scenario grid32]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "marl-responsible-nav_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from marlnav.vec_env import VecGridEnv  # noqa: E402


def run(scenario, E, table, steps, warmup):
    env = VecGridEnv(scenario, num_envs=E, fear=True, fear_weight=-5.0, max_steps=150, seed=42, fear_alt=table)
    env.set_obs_async(True)
    env.reset()
    for _ in range(warmup):
        env.step()
    env.obs_fence()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        env.step()
    env.obs_fence()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    counter = torch.zeros(1, dtype=torch.int64, device=env.device)
    env.count_sims(counter)
    for _ in range(steps):
        env.step()
    env.obs_fence()
    torch.cuda.synchronize()
    env.count_sims(None)
    sims = int(counter[0])
    out = dict(scenario=scenario, envs=E, fear_alt=bool(table), kernel_path=env.kernel_path, steps=steps,
               us_per_step=round(1e3 * ms / steps, 2), sims_per_step=round(sims / steps, 1),
               sims_per_s=round(sims / steps / (1e-3 * ms / steps), 1))
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--scenario", default="grid32")
    args = ap.parse_args()
    assert args.steps >= 1 and torch.cuda.is_available()
    for E in args.envs:
        for table in (False, True):
            print(json.dumps(run(args.scenario, E, table, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
