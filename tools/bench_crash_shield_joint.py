"""The coordinated crash-aware shield (gw_crash_shield_joint) measured: Level 3, 4,096 envs, uniform-random policy.

1. Crash rates over --steps steps (default 300), one run: no shield, the unilateral crash shield (step_preview's
   safe mask handed to fear_shield on a zero table), and joint_crash at 1, 2 and 4 sweeps.  Per setting: the RL
   agents' own crashes per 1,000 RL-agent-steps, all agents' crashes per 1,000 world-agent-steps, and for the
   shields the unavoidable agent-steps (every masked action crashes the agent) and, unilateral, how many of the
   crashes left were of the both-moved kind (the agent was moved, could have avoided the crash, and another RL
   agent of the env was moved too); joint_crash: unconverged env-steps.
2. One crash_shield_joint call against the composition from today's entry points (fear_preview, step_preview,
   fear_shield(agents=1 << k) per visit, then a final step_preview and fear_preview), crash-only and with FeAR at
   tau = 0, two sweeps: HIP events around each call, warm, the median and the spread of --reps calls.
One JSON line:

    python tools/bench_crash_shield_joint.py [--envs 4096] [--steps 300] [--reps 30]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-responsible-nav_amd")]

import torch  # noqa: E402

ALL = 0x1FF


def rates(mode, E, steps, sweeps=2, seed=0):
    from marlnav.vec_env import VecGridEnv
    env = VecGridEnv("level3", num_envs=E, fear=False, seed=seed, debug=True)
    _, mask = env.reset()
    K, N, dev = env.K, env.N, env.device
    kk = torch.arange(K, device=dev).unsqueeze(0)
    zero = torch.zeros((E, K, 9), dtype=torch.float64, device=dev)
    tot = dict(rl_crashes=0, all_crashes=0, unavoidable=0, both_moved=0, replaced=0, unconverged=0)
    for _ in range(steps):
        mask = env.out["mask"]
        if mode == "none":
            r = env.step()
            unav = moved = None
        elif mode == "unilateral":
            sp = env.step_preview(None, None, mask=mask, reward=False)
            prop = sp["actions"][:, :K].contiguous()
            out, _ = env.fear_shield(zero, prop, mask=sp["safe_mask"], tau=0.0)
            mm = mask.long() & ALL
            unav = (mm != 0) & ((mm & ~sp["crash9"].long()) == 0)
            moved = out != prop
            r = env.step(out)
        else:
            g = env.crash_shield_joint(None, None, mask=mask, sweeps=sweeps)
            unav, moved = (g["flags"] & 32) != 0, (g["flags"] & 1) != 0
            tot["unconverged"] += int((g["flags"][:, 0] & 8 != 0).sum())
            r = env.step(g["actions"])
        own = ((r.crash_bits.long().unsqueeze(1) >> kk) & 1).bool()
        tot["rl_crashes"] += int(own.sum())
        tot["all_crashes"] += int(sum(((r.crash_bits.long() >> n) & 1).sum() for n in range(N)))
        if unav is not None:
            tot["unavoidable"] += int(unav.sum())
            tot["replaced"] += int(moved.sum())
            others = moved.sum(1, keepdim=True) - moved.long() > 0
            tot["both_moved"] += int((own & moved & ~unav & others).sum())
    env.close()
    tot["rl_per_1000"] = round(1000.0 * tot["rl_crashes"] / (E * steps * K), 2)
    tot["all_per_1000"] = round(1000.0 * tot["all_crashes"] / (E * steps * N), 2)
    return tot


def composed(env, mask, tau, sweeps):
    """The rule on today's entry points (three calls per visit), as tests/test_gpu_crash_shield_joint.py composes it."""
    E, K, dev = env.E, env.K, env.device
    sp = env.step_preview(None, None, mask=mask, reward=False)
    cur = sp["actions"][:, :K].contiguous()
    zero = torch.zeros((E, K, 9), dtype=torch.float64, device=dev)
    for _ in range(sweeps):
        changed = torch.zeros(E, dtype=torch.bool, device=dev)
        for k in range(K):
            t = env.fear_preview(cur) if tau is not None else zero
            sp = env.step_preview(cur, None, mask=mask, reward=False)
            out, _ = env.fear_shield(t, cur, mask=sp["safe_mask"], tau=0.0 if tau is None else tau, agents=1 << k)
            changed |= out[:, k] != cur[:, k]
            cur = out
        if not bool(changed.any()):
            break
    env.step_preview(cur, None, mask=mask, reward=False)
    if tau is not None:
        env.fear_preview(cur)
    return cur


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) * 1e3)
    ms.sort()
    return dict(median_us=round(ms[len(ms) // 2], 1), min_us=round(ms[0], 1), max_us=round(ms[-1], 1), reps=reps)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args(argv)
    from marlnav.vec_env import VecGridEnv
    res = {"tool": "bench_crash_shield_joint", "scenario": "level3", "envs": args.envs, "steps": args.steps, "rates": {},
           "call_us": {}}
    for name, mode, sweeps in (("none", "none", 0), ("unilateral", "unilateral", 0), ("joint_crash_1", "joint", 1),
                               ("joint_crash_2", "joint", 2), ("joint_crash_4", "joint", 4)):
        res["rates"][name] = rates(mode, args.envs, args.steps, sweeps)
    env = VecGridEnv("level3", num_envs=args.envs, fear=False, seed=0, debug=True)
    _, mask = env.reset()
    for _ in range(20):  # a world in mid-episode
        env.step()
    mask = env.out["mask"]
    for name, tau in (("crash_only", None), ("fear_tau0", 0.0)):
        one = env.crash_shield_joint(None, None, mask=mask, tau=tau, sweeps=2)["actions"].clone()
        assert torch.equal(one, composed(env, mask, tau, 2)), name
        res["call_us"][name] = {
            "one_call": timed(lambda: env.crash_shield_joint(None, None, mask=mask, tau=tau, sweeps=2), args.reps),
            "composed": timed(lambda: composed(env, mask, tau, 2), args.reps)}
    env.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
