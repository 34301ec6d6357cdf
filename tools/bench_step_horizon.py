"""The crash horizon (gw_step_horizon) measured: uniform-random policy.

1. Crash rates on Level 3 (--envs envs x --steps steps), the RL agents' own crashes per 1,000 RL-agent-steps, with
   no shield, the unilateral crash shield (step_preview's safe mask handed to fear_shield on a zero table), the
   lookahead shield (step_lookahead's ahead_mask) and the horizon shield at H = 2, 3 and 4 (step_horizon's
   horizon_mask), all in one run from the same seed.  Horizon 2 hands out the lookahead shield's masks, so its
   trajectory and crash count must be the lookahead run's exactly: asserted here.  Each horizon run also counts the
   doomed proposals, the agent-steps without a viable action in the mask, and the agent-steps in which the mask
   had to fall back below depth H.
2. One step_horizon call at H = 2, 3, 4 beside one step_lookahead call in the same session, at Level 3 with --envs
   envs and at the headline shape (grid32, --big-envs envs): HIP events around the call, warm, the median and the
   spread of --reps calls, and the world updates per env of each from gw_count_sims.

Prints one JSON line.

    python tools/bench_step_horizon.py [--envs 4096] [--steps 300] [--reps 30] [--big-envs 65536]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-responsible-nav_amd")]

import torch  # noqa: E402

from bench_step_lookahead import timed  # noqa: E402

ALL = 0x1FF


def rates(mode, E, steps, seed=0):
    """mode: "none", "unilateral", "lookahead" or an int H (the horizon shield)."""
    from marlnav.vec_env import VecGridEnv
    env = VecGridEnv("level3", num_envs=E, fear=False, seed=seed, debug=True)
    env.reset()
    K, dev = env.K, env.device
    kk = torch.arange(K, device=dev).unsqueeze(0)
    zero = torch.zeros((E, K, 9), dtype=torch.float64, device=dev)
    tot = dict(rl_crashes=0, replaced=0, doomed_proposed=0, no_viable=0)
    for _ in range(steps):
        mask = env.out["mask"]
        if mode == "none":
            r = env.step()
        else:
            mm = mask.long() & ALL
            if mode == "unilateral":
                sp = env.step_preview(None, None, mask=mask, reward=False)
                allowed = sp["safe_mask"]
            elif mode == "lookahead":
                sp = env.step_lookahead(None, None, mask=mask)
                allowed = sp["ahead_mask"]
            else:
                sp = env.step_horizon(None, None, mask=mask, horizon=mode)
                allowed = sp["horizon_mask"]
                some = (sp["viable9"].long() & mm) != 0
                prop_ok = ((sp["viable9"].long() >> sp["actions"][:, :K].long()) & 1) != 0
                tot["doomed_proposed"] += int((some & ~prop_ok).sum())
                tot["no_viable"] += int((~some).sum())
            prop = sp["actions"][:, :K].contiguous()
            out, _ = env.fear_shield(zero, prop, mask=allowed, tau=0.0)
            tot["replaced"] += int((out != prop).sum())
            r = env.step(out)
        tot["rl_crashes"] += int(((r.crash_bits.long().unsqueeze(1) >> kk) & 1).sum())
    pos = env.positions().clone()
    env.close()
    tot["rl_per_1000"] = round(1000.0 * tot["rl_crashes"] / (E * steps * K), 2)
    return tot, pos


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
    la = lambda: env.step_lookahead(None, None, mask=mask)  # noqa: E731
    res["step_lookahead"] = dict(timed(la, reps), updates_per_env=sims(la))
    for H in (2, 3, 4):
        hz = lambda: env.step_horizon(None, None, mask=mask, horizon=H)  # noqa: E731
        res[f"step_horizon_{H}"] = dict(timed(hz, reps), updates_per_env=sims(hz))
    assert torch.equal(env.step_horizon(None, None, mask=mask, horizon=2)["horizon_mask"],
                       env.step_lookahead(None, None, mask=mask)["ahead_mask"])
    env.close()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--big-envs", type=int, default=65536)
    args = ap.parse_args(argv)
    res = {"tool": "bench_step_horizon", "scenario": "level3", "envs": args.envs, "steps": args.steps, "rates": {},
           "call_us": {}}
    final = {}
    for mode in ("none", "unilateral", "lookahead", 2, 3, 4):
        name = mode if isinstance(mode, str) else f"horizon_{mode}"
        res["rates"][name], final[name] = rates(mode, args.envs, args.steps)
    # the same masks, so the same trajectory
    assert res["rates"]["horizon_2"]["rl_crashes"] == res["rates"]["lookahead"]["rl_crashes"], res["rates"]
    assert torch.equal(final["horizon_2"], final["lookahead"])
    res["call_us"]["level3"] = call_times("level3", args.envs, args.reps)
    if args.big_envs > 0:
        res["call_us"]["grid32"] = call_times("grid32", args.big_envs, args.reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
