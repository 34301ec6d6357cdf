"""The two-step crash lookahead (gw_step_lookahead) measured: uniform-random policy.

1. Crash rates on Level 3 over --steps steps (default 300), one run: no shield, the unilateral crash shield
   (step_preview's safe mask handed to fear_shield on a zero table) and the lookahead shield (step_lookahead's
   ahead_mask in its place).  Per setting: the RL agents' own crashes per 1,000 RL-agent-steps and all agents'
   crashes per 1,000 world-agent-steps; for the shields the replaced agent-steps, the unavoidable agent-steps
   (every masked action crashes the agent), the own crashes in such agent-steps, and how many of THOSE were
   preceded by a trap action: the action the same agent applied one step earlier, in the same episode, was in that
   step's trap9.  The lookahead run also counts the trap proposals and the agent-steps in which every crash-free
   masked action was a trap (the mask fell back to the safe mask).
2. One step_lookahead call beside one step_preview call in the same session, at Level 3 with --envs envs and at
   the headline shape (grid32: 32 x 32, N = 4, K = 2) with --big-envs envs: HIP events around each call, warm, the
   median and the spread of --reps calls.  No composition of the lookahead from step_preview and forced steps on
   a scratch env exists, so there is no composed baseline.
One JSON line:

    python tools/bench_step_lookahead.py [--envs 4096] [--steps 300] [--reps 30] [--big-envs 65536]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-responsible-nav_amd")]

import torch  # noqa: E402

ALL = 0x1FF


def rates(mode, E, steps, seed=0):
    from marlnav.vec_env import VecGridEnv
    env = VecGridEnv("level3", num_envs=E, fear=False, seed=seed, debug=True)
    env.reset()
    K, N, dev = env.K, env.N, env.device
    kk = torch.arange(K, device=dev).unsqueeze(0)
    zero = torch.zeros((E, K, 9), dtype=torch.float64, device=dev)
    tot = dict(rl_crashes=0, all_crashes=0, replaced=0, unavoidable=0, unavoidable_crashes=0, after_trap=0,
               trap_proposed=0, trap_only=0)
    prev_trap = torch.zeros((E, K), dtype=torch.bool, device=dev)  # the action applied one step earlier was a trap
    for _ in range(steps):
        mask = env.out["mask"]
        if mode == "none":
            r = env.step()
            own = ((r.crash_bits.long().unsqueeze(1) >> kk) & 1).bool()
        else:
            la = env.step_lookahead(None, None, mask=mask)  # (the unilateral run reads its trap sets only)
            prop = la["actions"][:, :K].contiguous()
            crash9, trap9 = la["crash9"].long(), la["trap9"].long()
            mm = mask.long() & ALL
            if mode == "lookahead":
                allowed = la["ahead_mask"]
                tot["trap_proposed"] += int(((trap9 >> prop.long()) & 1).sum())
                tot["trap_only"] += int((((mm & ~crash9) != 0) & ((mm & ~crash9 & ~trap9) == 0)).sum())
            else:
                allowed = env.step_preview(None, None, mask=mask, reward=False)["safe_mask"]
            out, _ = env.fear_shield(zero, prop, mask=allowed, tau=0.0)
            unav = (mm != 0) & ((mm & ~crash9) == 0)
            r = env.step(out)
            own = ((r.crash_bits.long().unsqueeze(1) >> kk) & 1).bool()
            tot["replaced"] += int((out != prop).sum())
            tot["unavoidable"] += int(unav.sum())
            tot["unavoidable_crashes"] += int((own & unav).sum())
            tot["after_trap"] += int((own & unav & prev_trap).sum())
            prev_trap = (((trap9 >> out.long()) & 1) != 0) & (r.done == 0).unsqueeze(1)
        tot["rl_crashes"] += int(own.sum())
        tot["all_crashes"] += int(sum(((r.crash_bits.long() >> n) & 1).sum() for n in range(N)))
    env.close()
    tot["rl_per_1000"] = round(1000.0 * tot["rl_crashes"] / (E * steps * K), 2)
    tot["all_per_1000"] = round(1000.0 * tot["all_crashes"] / (E * steps * N), 2)
    return tot


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


def call_times(scenario, E, reps):
    from marlnav.vec_env import VecGridEnv
    env = VecGridEnv(scenario, num_envs=E, fear=False, seed=0)
    env.reset()
    for _ in range(20):  # a world in mid-episode
        env.step()
    mask = env.out["mask"]
    la = env.step_lookahead(None, None, mask=mask)
    pv = env.step_preview(None, None, mask=mask, reward=False)
    assert torch.equal(la["crash9"], pv["crash9"])
    going = 9 * env.K * E - int(sum(((la["ends"].long() >> a) & 1).sum() for a in range(9)))
    res = dict(envs=E, N=env.N, K=env.K, H=env.H, W=env.W, second_steps_per_env=round(9.0 * going / E, 1),
               step_lookahead=timed(lambda: env.step_lookahead(None, None, mask=mask), reps),
               step_preview=timed(lambda: env.step_preview(None, None, mask=mask, reward=False), reps))
    env.close()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--big-envs", type=int, default=65536)
    args = ap.parse_args(argv)
    res = {"tool": "bench_step_lookahead", "scenario": "level3", "envs": args.envs, "steps": args.steps, "rates": {},
           "call_us": {}}
    for mode in ("none", "unilateral", "lookahead"):
        res["rates"][mode] = rates(mode, args.envs, args.steps)
    res["call_us"]["level3"] = call_times("level3", args.envs, args.reps)
    if args.big_envs > 0:
        res["call_us"]["grid32"] = call_times("grid32", args.big_envs, args.reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
