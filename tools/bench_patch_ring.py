"""A/B of the window rollout's replay ring at c5patch's shape (65,536 envs, grid32, P = 11, FeAR on, the fused
MLP window actor): the dense window ring (the step also writes 2 K P^2 floats per env) against the
descriptor-only ring (``Rollout(patch=P, desc_ring="only")``: 48 bytes per env, no window writer).

Both rollouts live in one process and their runs alternate (dense, desc, dense, desc, ...): --runs runs of
--steps steps each after a warm-up, timed with a host clock around work that ends in a device synchronise;
reported as median [min, max] us per step.  Rollout-only steps replay as ring-phase graphs of 16 steps, as
bench.py's c5patch line does; with --updates-per-step N every step is eager and followed by N batch-128
updates (the dense fused learner, recorded launches) sampled from that ring.

    python tools/bench_patch_ring.py [--updates-per-step 1] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "marl-responsible-nav_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GRAPH_N = 16


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--scenario", default="grid32")
    ap.add_argument("--patch", type=int, default=11)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--updates-per-step", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import torch
    from marlnav.maddpg import MADDPG
    from marlnav.rollout import Rollout
    from marlnav.vec_env import VecGridEnv

    if not torch.cuda.is_available():
        raise SystemExit("bench_patch_ring: needs the GPU (a timing on the CPU says nothing)")
    E, P, ups = args.envs, args.patch, args.updates_per_step
    slots = -(-max(-(-200_000 // E) + 1, 2) // GRAPH_N) * GRAPH_N  # bench.py's ring, rounded to the graph length

    class Side:
        def __init__(self, mode):
            self.mode = mode
            self.env = VecGridEnv(args.scenario, num_envs=E, fear=True, fear_weight=-5.0, max_steps=150,
                                  auto_reset=True, seed=42, stats=True, obs=False)
            self.learner = MADDPG(self.env.K, P, P, device=self.env.device, seed=0, capturable=True, batch_size=128)
            self.ro = Rollout(self.env, self.learner.actors, replay_slots=slots, training=True, seed=42, patch=P,
                              desc_ring="only" if mode == "desc" else False)
            assert self.ro.fused and self.ro.desc_only == (mode == "desc")
            self.ro.reset()
            self.graph = None

        def eager(self, n):
            ro, m = self.ro, self.learner
            for _ in range(n):
                ro.step()
                if ups and ro.replay.t >= 2:
                    ro.learn_fence()
                    if m._graph is None:
                        m.capture(ro.replay, launches=True)
                    for _ in range(ups):
                        m.replay_learn()

        def run(self, n):
            """n steps; rollout-only: whole graphs first, the remainder eagerly, then untimed steps back to a
            graph boundary.  -> seconds for the n steps."""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if self.graph is not None:
                for _ in range(n // GRAPH_N):
                    self.graph.replay()
                self.eager(n % GRAPH_N)
            else:
                self.eager(n)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if self.graph is not None and n % GRAPH_N:
                self.eager(GRAPH_N - n % GRAPH_N)
                torch.cuda.synchronize()
            return dt

    sides = [Side("dense"), Side("desc")]
    for s in sides:
        s.eager(args.warmup - args.warmup % GRAPH_N or GRAPH_N)
        torch.cuda.synchronize()
        if not ups:
            s.graph = s.ro.capture(GRAPH_N)
        s.run(GRAPH_N * 4)  # the timed path itself, warm
    times = {s.mode: [] for s in sides}
    for _ in range(args.runs):
        for s in sides:  # alternating
            times[s.mode].append(s.run(args.steps) / args.steps * 1e6)
    K = sides[0].env.K
    common = K * 9 * 4 + K * 8 + K + 1  # probs, reward, term, done per env and slot
    res = dict(envs=E, scenario=args.scenario, patch=P, steps=args.steps, runs=args.runs, updates_per_step=ups,
               slots=slots, graph_steps=0 if ups else GRAPH_N,
               ring_bytes_per_env_slot=dict(dense_obs=2 * K * P * P * 4, desc_obs=48, other=common))
    for mode, v in times.items():
        res[mode] = dict(us_per_step=[round(x, 2) for x in v], median=round(statistics.median(v), 2),
                         min=round(min(v), 2), max=round(max(v), 2))
    res["ring_alloc_bytes"] = {s.mode: int(sum(t.numel() * t.element_size() for t in
                                                (getattr(s.ro.replay, n) for n in ("obs", "final_obs", "desc"))
                                                if t is not None)) for s in sides}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for s in sides:
        s.env.close()


if __name__ == "__main__":
    main()
