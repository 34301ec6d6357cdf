"""Cost of the responsibility-footprint fold (gw_resp_footprint_accum) at bench.py's C3 shape: 65,536 envs of
grid32 (32 x 32, N = 4, K = 2), FeAR on with the N x N matrix armed (gw_set_fear_full) and the step's actions
and crash bits reported (debug=True), random RL policy, the obs writer pipelined as bench.py runs it.

One process, one env.  The step alone and the step with the fold (the pre-move cells copied before it,
``VecGridEnv.copy_pos``, and the op after it) alternate, --runs times each of --steps steps between two HIP
events with no host sync inside; then the op alone, back to back on the last step's data.  A last pass folds
--share-steps steps at R = 15 and reports what the footprint shows: the share of the absolute Resp beyond each
radius.  One JSON line with the median [min, max] of each:

    python tools/bench_resp_footprint.py [--steps 300] [--runs 5] [--warmup 50] [--envs 65536] [--radius 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-responsible-nav_amd")]

import numpy as np  # noqa: E402
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


def far_shares(counts15):
    """counts [2, 9, O(15), 10, 10] -> the share of the absolute Resp beyond Chebyshev radius r, r = 0..15."""
    from marlnav.resp_footprint import resp_footprint_from_counts
    from marlnav.resp_map import resp_table
    mag = resp_footprint_from_counts(counts15, np.abs(resp_table()))[0][0].numpy().sum(0)  # [O]: over the actions
    near, far = mag[:-1].reshape(31, 31), float(mag[-1])
    d = np.maximum(np.abs(np.arange(31) - 15)[:, None], np.abs(np.arange(31) - 15)[None, :])
    total = float(near.sum()) + far
    return [(float(near[d > r].sum()) + far) / total if total else 0.0 for r in range(16)], total


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--scenario", default="grid32")
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--share-steps", type=int, default=100)
    args = ap.parse_args(argv)

    from marlnav.vec_env import VecGridEnv
    E, R = args.envs, args.radius
    env = VecGridEnv(args.scenario, num_envs=E, fear=True, fear_weight=-5.0, max_steps=150, auto_reset=True, seed=42,
                     stats=True, fear_full=True, debug=True)
    dev = env.device
    counts = torch.zeros((2, 9, (2 * R + 1) ** 2 + 1, 10, 10), dtype=torch.int64, device=dev)
    visits = torch.zeros(9, dtype=torch.int64, device=dev)
    cells = torch.empty((env.N, E), dtype=torch.int32, device=dev)
    env.set_obs_async(True)
    env.reset()
    out = env.out

    def plain():
        env.step()

    def fold(c=counts, v=visits, radius=R):
        env.resp_footprint_accum(out["resp_valid"], cells, out["actions"], c, v, crash_bits=out["crash_bits"],
                                 radius=radius)

    def folded():
        env.copy_pos(cells)
        env.step()
        fold()

    for _ in range(args.warmup):
        folded()
    for _ in range(args.warmup):
        plain()
    us_plain, us_fold = [], []
    for _ in range(args.runs):
        us_plain.append(timed(args.steps, plain))
        us_fold.append(timed(args.steps, folded))
    env.obs_fence()
    us_op = [timed(args.steps, fold) for _ in range(args.runs)]
    torch.cuda.synchronize()
    bins_hit = [int((counts[p] != 0).sum()) for p in range(2)]
    pairs, crashed = int(counts[0].sum()), int(counts[1].sum())
    launches = args.warmup + 2 * args.runs * args.steps
    # what the footprint shows: a fold at R = 15, the largest radius
    c15 = torch.zeros((2, 9, 31 * 31 + 1, 10, 10), dtype=torch.int64, device=dev)
    for _ in range(args.share_steps):
        env.copy_pos(cells)
        env.step()
        fold(c15, None, 15)
    torch.cuda.synchronize()
    shares, total = far_shares(c15.cpu())
    r99 = next((r for r in range(16) if shares[r] <= 0.01), None)
    env.close()
    res = {"tool": "bench_resp_footprint", "scenario": args.scenario, "envs": E, "agents": env.N, "radius": R,
           "kernel_path": env.kernel_path, "steps_per_run": args.steps, "runs": args.runs,
           "us_per_step_armed_med_min_max": mmm(us_plain), "us_per_step_with_fold_med_min_max": mmm(us_fold),
           "fold_minus_armed_us_median": statistics.median(us_fold) - statistics.median(us_plain),
           "us_op_alone_back_to_back_med_min_max": mmm(us_op),
           "increments_per_launch_plane0_and_visits": E * env.N * env.N,
           "increments_per_launch_crash_plane_mean": crashed / launches, "pair_steps_counted_plane0": pairs,
           "nonzero_bins_plane0_plane1": bins_hit, "bins_per_plane": counts[0].numel(),
           "share_steps": args.share_steps, "abs_resp_total_share_steps": total,
           "far_share_of_abs_resp_beyond_radius_0_to_15": shares, "far_share_at_radius": shares[R],
           "smallest_radius_holding_99_percent": r99}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
