"""Cost of the responsibility-map fold (gw_resp_map_accum) at bench.py's C3 shape: 65,536 envs of grid32
(32 x 32, N = 4, K = 2), FeAR on with the N x N matrix armed (gw_set_fear_full), random RL policy, the obs
writer pipelined as bench.py runs it.

One process, one env.  The step alone and the step with the fold (the pre-move cells copied before it,
``VecGridEnv.copy_pos``, and the op after it) alternate, --runs times each of --steps steps between two HIP
events with no host sync inside; then the op alone, back to back on the last step's data.  One JSON line with
the median [min, max] of each:

    python tools/bench_resp_map.py [--steps 300] [--runs 5] [--warmup 50] [--envs 65536] [--scenario grid32]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-responsible-nav_amd")]

import torch  # noqa: E402


def timed(n, body):
    """us per call of body() over n calls between two HIP events on the current stream."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(n):
        body()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1e3 / n


def mmm(xs):
    return [statistics.median(xs), min(xs), max(xs)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--scenario", default="grid32")
    args = ap.parse_args(argv)

    from marlnav.vec_env import VecGridEnv
    E = args.envs
    env = VecGridEnv(args.scenario, num_envs=E, fear=True, fear_weight=-5.0, max_steps=150, auto_reset=True, seed=42,
                     stats=True, fear_full=True)
    hw = env.H * env.W
    counts = torch.zeros((2, hw, 10, 10), dtype=torch.int64, device=env.device)
    visits = torch.zeros(hw, dtype=torch.int64, device=env.device)
    cells = torch.empty((env.N, E), dtype=torch.int32, device=env.device)
    env.set_obs_async(True)
    env.reset()

    def plain():
        env.step()

    def folded():
        env.copy_pos(cells)
        r = env.step()
        env.resp_map_accum(r.resp_valid, cells, counts, visits)

    for _ in range(args.warmup):
        folded()
    for _ in range(args.warmup):
        plain()
    us_plain, us_fold = [], []
    for _ in range(args.runs):
        us_plain.append(timed(args.steps, plain))
        us_fold.append(timed(args.steps, folded))
    env.obs_fence()
    rv = env.out["resp_valid"]
    us_op = [timed(args.steps, lambda: env.resp_map_accum(rv, cells, counts, visits)) for _ in range(args.runs)]
    us_copy = [timed(args.steps, lambda: env.copy_pos(cells)) for _ in range(args.runs)]
    torch.cuda.synchronize()
    bins_hit = int((counts != 0).sum())
    pairs = int(counts[0].sum())
    env.close()
    out = {"tool": "bench_resp_map", "scenario": args.scenario, "envs": E, "agents": env.N, "cells": hw,
           "kernel_path": env.kernel_path, "steps_per_run": args.steps, "runs": args.runs,
           "us_per_step_armed_med_min_max": mmm(us_plain), "us_per_step_with_fold_med_min_max": mmm(us_fold),
           "fold_minus_armed_us_median": statistics.median(us_fold) - statistics.median(us_plain),
           "us_op_alone_back_to_back_med_min_max": mmm(us_op), "us_copy_pos_alone_med_min_max": mmm(us_copy),
           "atomics_per_launch": E * env.N * (2 * (env.N - 1) + 1), "pair_steps_counted_plane0": pairs,
           "nonzero_bins": bins_hit}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
