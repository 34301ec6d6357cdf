"""Cost of the FeAR preview + responsibility shield (gw_fear_preview, gw_fear_shield) at bench.py's C3 shape:
65,536 envs of grid32 (32 x 32, N = 4, K = 2), FeAR on, the obs writer pipelined as bench.py runs it.

One process, one env: the step alone (device-random RL policy), then preview + shield + step (the same random
proposals, taken from the preview's joint action; tau = 0, the env's action mask, every RL agent shielded), then
the step alone again: HIP events around >= 200 timed steps after a warm-up, no host sync inside.  Then the two
preview launches' busy time from the per-launch profiling spans (GW_SPAN_FEAR_PREVIEW) and the preview's world
updates per step from gw_count_sims.  One JSON line:

    python tools/bench_fear_preview.py [--steps 300] [--warmup 50] [--envs 65536] [--scenario grid32]

--mode joint [--sweeps N] [--repeats 5]: the coordinated shield (gw_fear_shield_joint) against the same rule
composed from the two entry points above, on one fixed world in the same run (joint_mode below).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-responsible-nav_amd")]

import torch  # noqa: E402

GW_SPAN_FEAR_PREVIEW = 12


class Shielded:
    """preview -> shield -> step with preallocated buffers (what Rollout(shield=tau) does per step)."""

    def __init__(self, env, tau):
        E, K, N, dev = env.E, env.K, env.N, env.device
        self.env, self.tau = env, tau
        self.table = torch.empty((E, K, 9), dtype=torch.float64, device=dev)
        self.joint = torch.empty((E, N), dtype=torch.int32, device=dev)
        self.prop = torch.empty((E, K), dtype=torch.int32, device=dev)
        self.out = torch.empty((E, K), dtype=torch.int32, device=dev)
        self.flags = torch.zeros((E, K), dtype=torch.uint8, device=dev)

    def step(self):
        env = self.env
        env.fear_preview(None, out=self.table, actions=self.joint)
        self.prop.copy_(self.joint[:, :env.K])
        env.fear_shield(self.table, self.prop, mask=env.out["mask"], tau=self.tau, out=self.out, flags=self.flags)
        return env.step(self.out)


def timed(fn, n):
    """us per call over n calls between two HIP events on the current stream."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(n):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1e3 / n


def joint_mode(env, args):
    """--mode joint: on one fixed world (the env after the warm-up steps, the random policy's proposals, the env's
    action mask, every RL agent shielded) time, in this same run, (a) the rule of gw_fear_shield_joint composed
    from gw_fear_preview + gw_fear_shield(agents = 1 << k) with one sweep: K previews, K shields and the final
    preview (two launches per preview); (b) the one joint call at sweeps = 1, 2, 4 (and --sweeps); (c) the share of envs
    with flag bits 0, 2 and 3.  Each figure: `repeats` runs of `steps` calls between two HIP events after a
    warm-up; median, min and max over the runs in us per call."""
    import statistics
    E, K, N, dev = env.E, env.K, env.N, env.device
    table = torch.empty((E, K, 9), dtype=torch.float64, device=dev)
    joint = torch.empty((E, N), dtype=torch.int32, device=dev)
    env.obs_fence()
    env.fear_preview(None, out=table, actions=joint)
    prop = joint[:, :K].contiguous()
    scripted = joint[:, K:].contiguous()
    mask = env.out["mask"]
    cur = torch.empty_like(prop)
    flags = torch.zeros((E, K), dtype=torch.uint8, device=dev)
    out = torch.empty_like(prop)

    def composed():
        cur.copy_(prop)
        for k in range(K):
            env.fear_preview(cur, scripted, out=table)
            env.fear_shield(table, cur, mask=mask, tau=args.tau, agents=1 << k, out=cur, flags=flags)
        env.fear_preview(cur, scripted, out=table)

    def joint_call(sweeps):
        return lambda: env.fear_shield_joint(prop, scripted, mask=mask, tau=args.tau, sweeps=sweeps, out=out,
                                             flags=flags, table=table)

    def spread(fn):
        for _ in range(args.warmup):
            fn()
        runs = sorted(timed(fn, args.steps) for _ in range(args.repeats))
        return {"median_us": statistics.median(runs), "min_us": runs[0], "max_us": runs[-1], "runs": len(runs)}

    res = {"composed_one_sweep": spread(composed)}
    composed()
    torch.cuda.synchronize()
    want_actions, want_table = cur.clone(), table.clone()
    for sweeps in sorted({1, 2, 4, args.sweeps}):
        res[f"joint_sweeps_{sweeps}"] = spread(joint_call(sweeps))
        torch.cuda.synchronize()
        share = lambda b: float(((flags >> b) & 1).any(1).float().mean())  # noqa: E731
        res[f"joint_sweeps_{sweeps}"].update(share_replaced=share(0), share_over=share(2), share_unconverged=share(3))
        if sweeps == 1:  # the same rule: the same answer
            assert torch.equal(out, want_actions) and torch.equal(table, want_table)
    res["composed_again"] = spread(composed)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    env.count_sims(ctr)
    joint_call(args.sweeps)()
    env.count_sims(None)
    torch.cuda.synchronize()
    res["joint_sims_per_call"] = int(ctr.item())
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["unilateral", "joint"], default="unilateral")
    ap.add_argument("--sweeps", type=int, default=2, help="--mode joint: the sweep count timed beside 1, 2 and 4")
    ap.add_argument("--repeats", type=int, default=5, help="--mode joint: timed runs per figure")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--scenario", default="grid32")
    ap.add_argument("--profiled", type=int, default=20)
    ap.add_argument("--tau", type=float, default=0.0)
    args = ap.parse_args(argv)
    assert args.steps >= 200, "at least 200 timed steps"

    from marlnav.vec_env import VecGridEnv
    E = args.envs
    env = VecGridEnv(args.scenario, num_envs=E, fear=True, fear_weight=-5.0, max_steps=150, auto_reset=True, seed=42,
                     stats=True)
    sh = Shielded(env, args.tau)
    env.set_obs_async(True)
    env.reset()
    for _ in range(args.warmup):  # the preview's record buffer and both code paths exist before anything is timed
        sh.step()
    for _ in range(args.warmup):
        env.step()

    if args.mode == "joint":
        res = joint_mode(env, args)
        env.close()
        print(json.dumps({"tool": "bench_fear_preview", "mode": "joint", "scenario": args.scenario, "envs": E,
                          "agents": env.N, "rl_agents": env.K, "tau": args.tau, "calls_per_run": args.steps, **res}),
              flush=True)
        return

    us = {}
    for name, fn in (("step", env.step), ("shielded", sh.step), ("step_again", env.step)):
        for _ in range(10):
            fn()
        us[name] = timed(fn, args.steps)

    # the preview alone: per-call spans and the sim counter over a few profiled calls on the current world
    env.obs_fence()
    n_prof = args.profiled
    env.profile(True, reserve=16 * (n_prof + 2))
    env.profile(False)
    ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
    env.count_sims(ctr)
    env.profile(True)
    for _ in range(n_prof):
        env.fear_preview(None, out=sh.table)
    torch.cuda.synchronize()
    env.profile(False)
    env.count_sims(None)
    sims = int(ctr.item())
    spans = env.profile_spans()
    env.profile_read()
    k = spans[spans[:, 0] == GW_SPAN_FEAR_PREVIEW]
    busy_us = float((k[:, 2] - k[:, 1]).sum()) * 1e3 / max(len(k), 1)
    replaced = (sh.flags & 1).sum(0).cpu().tolist()
    stuck = (sh.flags >> 1).sum(0).cpu().tolist()
    env.close()
    out = {"tool": "bench_fear_preview", "scenario": args.scenario, "envs": E, "agents": env.N, "tau": args.tau,
           "kernel_path": env.kernel_path, "timed_steps": args.steps,
           "us_per_step": us["step"], "us_per_step_shielded": us["shielded"], "us_per_step_again": us["step_again"],
           "shielded_minus_step_us": us["shielded"] - 0.5 * (us["step"] + us["step_again"]),
           "preview_spans_profiled": int(len(k)), "preview_span_us": busy_us,
           "preview_sims_per_call": sims / n_prof,
           "preview_sims_per_s_at_span": (sims / n_prof) / (busy_us * 1e-6) if busy_us else None,
           "replaced_last_step": replaced, "stuck_last_step": stuck}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
