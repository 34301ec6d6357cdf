"""us per step of ``evaluate`` with the responsibility shield on: Level 3, 4,096 episodes, random-initialised MLP
actors; the whole call (env creation included) over the steps its loop took, five calls per setting.  One JSON line:

    python tools/bench_eval_shield.py [--episodes 4096] [--runs 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-responsible-nav_amd")]

import torch  # noqa: E402

SETTINGS = (("plain", {}), ("shield0", dict(shield=0.0)), ("shield0_crash", dict(shield=0.0, shield_crash=True)),
            ("crash", dict(shield_crash=True)), ("joint0", dict(shield=0.0, shield_mode="joint")),
            ("joint_crash", dict(shield_mode="joint_crash")), ("joint0_crash", dict(shield=0.0, shield_mode="joint_crash")))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args(argv)

    from marlnav import scenario as S
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    from marlnav.vec_env import VecGridEnv

    calls = [0]
    env_step = VecGridEnv.step

    def counted(self, *a, **k):  # the loop's steps (the result's "steps" are active env-steps)
        calls[0] += 1
        return env_step(self, *a, **k)

    VecGridEnv.step = counted
    sc = S.builtin("level3")
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=0)
    res = {"tool": "bench_eval_shield", "scenario": "level3", "episodes": args.episodes}
    for name, kw in SETTINGS:
        runs = []
        for _ in range(args.runs):
            calls[0] = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = evaluate(actors, sc, episodes=args.episodes, max_steps=150, **kw)
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) * 1e6 / calls[0])
        res[name] = {"us_per_step_runs": [round(x, 1) for x in runs], "loop_steps": calls[0], "steps": r["steps"],
                     "crashes": r["crashes"],
                     "shield": {k: v.tolist() if hasattr(v, "tolist") else v for k, v in r.items()
                                if k.startswith("shield")}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
