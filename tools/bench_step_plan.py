"""The reward horizon (gw_step_plan) measured: uniform-random policy.

1. Behaviour on Level 3 (--envs envs x --steps steps): the RL agents' own crashes and the apples caught per 1,000
   RL-agent-steps with no shield, the horizon shield (step_horizon's horizon_mask handed to fear_shield on a zero
   table) and the plan shield (step_plan's plan_mask in its place), at H = 3 and 4, all in one run from the same
   seed.  Each shielded run also counts the replaced proposals.
2. One step_plan call beside one step_horizon call at the same H (2, 3, 4) in the same session, at Level 3 with
   --envs envs and at the headline shape (grid32, --big-envs envs): HIP events around the call, warm, the median and
   the spread of --reps calls, and the world updates per env of each from gw_count_sims.

Prints one JSON line.

    python tools/bench_step_plan.py [--envs 4096] [--steps 300] [--reps 30] [--big-envs 65536]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-responsible-nav_amd")]

import torch  # noqa: E402

from bench_step_lookahead import timed  # noqa: E402


def rates(mode, H, E, steps, seed=0):
    """mode: "none", "horizon" or "plan"."""
    from marlnav.vec_env import VecGridEnv
    env = VecGridEnv("level3", num_envs=E, fear=False, seed=seed, debug=True)
    env.reset()
    K, dev = env.K, env.device
    kk = torch.arange(K, device=dev).unsqueeze(0)
    zero = torch.zeros((E, K, 9), dtype=torch.float64, device=dev)
    tot = dict(rl_crashes=0, apples=0, replaced=0)
    for _ in range(steps):
        mask = env.out["mask"]
        if mode == "none":
            r = env.step()
        else:
            if mode == "horizon":
                sp = env.step_horizon(None, None, mask=mask, horizon=H)
                allowed = sp["horizon_mask"]
            else:
                sp = env.step_plan(None, None, mask=mask, horizon=H)
                allowed = sp["plan_mask"]
            prop = sp["actions"][:, :K].contiguous()
            out, _ = env.fear_shield(zero, prop, mask=allowed, tau=0.0)
            tot["replaced"] += int((out != prop).sum())
            r = env.step(out)
        tot["rl_crashes"] += int(((r.crash_bits.long().unsqueeze(1) >> kk) & 1).sum())
        tot["apples"] += int(r.apples.sum())
    env.close()
    tot["crashes_per_1000"] = round(1000.0 * tot["rl_crashes"] / (E * steps * K), 2)
    tot["apples_per_1000"] = round(1000.0 * tot["apples"] / (E * steps * K), 2)
    return tot


def call_times(scenario, E, reps):
    from marlnav.vec_env import VecGridEnv
    env = VecGridEnv(scenario, num_envs=E, fear=False, seed=0)
    env.reset()
    for _ in range(20):  # a world in mid-episode
        env.step()
    mask = env.out["mask"]
    ctr = torch.zeros(1, dtype=torch.int64, device=env.device)

    def sims(fn):
        ctr.zero_()
        env.count_sims(ctr)
        fn()
        env.count_sims(None)
        torch.cuda.synchronize()
        return round(int(ctr) / E, 1)

    res = dict(envs=E, N=env.N, K=env.K, H=env.H, W=env.W)
    for H in (2, 3, 4):
        hz = lambda: env.step_horizon(None, None, mask=mask, horizon=H)  # noqa: E731
        pl = lambda: env.step_plan(None, None, mask=mask, horizon=H)  # noqa: E731
        res[f"step_horizon_{H}"] = dict(timed(hz, reps), updates_per_env=sims(hz))
        res[f"step_plan_{H}"] = dict(timed(pl, reps), updates_per_env=sims(pl))
    env.close()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--big-envs", type=int, default=65536)
    args = ap.parse_args(argv)
    res = {"tool": "bench_step_plan", "scenario": "level3", "envs": args.envs, "steps": args.steps, "rates": {},
           "call_us": {}}
    res["rates"]["none"] = rates("none", 0, args.envs, args.steps)
    for H in (3, 4):
        for mode in ("horizon", "plan"):
            res["rates"][f"{mode}_{H}"] = rates(mode, H, args.envs, args.steps)
    res["call_us"]["level3"] = call_times("level3", args.envs, args.reps)
    if args.big_envs > 0:
        res["call_us"]["grid32"] = call_times("grid32", args.big_envs, args.reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
