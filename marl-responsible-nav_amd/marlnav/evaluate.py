"""Evaluation driver: ``customeval.py:70-133`` batched.

The reference evaluates a trained MADDPG for ``eval_episodes = 100`` episodes, one env at a
time: every episode runs at most TRAIN_STEPS steps (``configs/custom.yaml``) and stops when all
RL agents are terminated or all are truncated; it sums ``info["agent_crashes"]`` and
``info["apples_caught"]`` over all steps taken and counts the steps.  Here the episodes run as
E = episodes envs in parallel (auto-reset off, step cap = TRAIN_STEPS); an env stops counting
after its episode ends, so the totals are the same sums.  Actions: ``training=False`` (no
Gumbel noise), the env's action mask, argmax — agilerl's eval-mode ``get_action`` restated.
With the fused actor the env writes no dense obs (the actor reads the obs descriptors).
Weights come from this package's safetensors checkpoints (marlnav/maddpg.py ``MADDPG.save``) or
from the reference's shipped agilerl ``.pt`` checkpoints, read without unpickling by
marlnav/checkpoint.py (``agents.load_wo_memory``, maddpg/agent.py:279-281); those are
single-agent actors (obs 160 = Level 3's 10 x 16), evaluated on the single-agent CustomEnv
(``variant=1``, custom/customenv.py:78-183).
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import _lib
from .actor import MultiAgentActors
from .resp_folds import Shield, build_folds, check_shield_args, fold_parts, fold_results
from .scenario import builtin
from .vec_env import VecGridEnv

# the folds' totals that evaluate reports as means per active env-step, under these names; the counts it drops
_MEANS = {"resp": "resp", "fear_regret": "fear_regret", "fear_best": "fear_best_frac", "feal_sum": "feal"}
_UNUSED = ("resp_steps", "fear_regret_steps", "feal_envs", "feal_steps")


@torch.no_grad()
def evaluate(actors: MultiAgentActors, scenario="level3", episodes: int = 100, max_steps: int = 150,
             fear: bool = False, seed: int = 42, record_actions: bool = False, fused: bool | None = None,
             variant: int = 0, resp_matrix: bool = False, fear_regret: bool = False,
             feal: bool = False, resp_full: bool = False, shield: float | None = None,
             shield_mode: str = "unilateral", shield_sweeps: int = 2, resp_map: bool = False,
             resp_footprint: int | None = None, shield_crash: bool = False,
             shield_lookahead: bool = False, shield_horizon: int | None = None,
             shield_plan: int | None = None) -> dict:
    """The responsibility folds (marlnav/resp_folds.py: each class says what it sums), over the episodes still
    running; all but ``resp_matrix`` raise ValueError without ``fear=True``.  f64 / int64 CPU tensors:
      resp_matrix: "resp" [K, N], the summed rows divided by "steps".
      fear_regret: "fear_regret" [K] and "fear_best_frac" [K] (how often agent k's action was FeAR-minimal),
        per active env-step.
      feal: "feal" [N], the mean FeAL of every world agent per active env-step.
      resp_full: "resp_full" [N, N] (the sum: divide by "steps" for the mean) and "resp_full_steps", the batched
        steps it covers.
      resp_map: "resp_map" [2, H, W], "resp_map_counts", "resp_map_visits"
        (``resp_map.reshape(2, -1) / resp_map_visits`` is the mean per visit).
      resp_footprint (a radius R in 1..15): "resp_footprint" [2, 9, O], "resp_footprint_counts",
        "resp_footprint_visits".
    The responsibility shield at inference time (``resp_folds.Shield`` has the pipelines), counted over the
    episodes still running; works with ``fear=False`` (the reference's evaluation configuration); recorded
    actions are the ones applied:
      shield (a float tau; None: off): "shield_replaced" [K], "shield_stuck" [K].
      shield_mode: "unilateral" or "joint" (at most ``shield_sweeps`` sweeps); joint: also "shield_over" [K]
        and "shield_unconverged".
      shield_crash: the crash-aware shield, alone or with ``shield``; also "shield_crash_proposed" [K] and
        "shield_crash_replaced" [K].  Unilateral: ValueError with ``shield_mode="joint"``.
      shield_mode="joint_crash": the coordinated crash-aware shield (``VecGridEnv.crash_shield_joint``: the crash
        preview inside the joint sweeps); ``shield=None`` is crash-only, a tau adds FeAR; ``shield_crash`` is
        implied.  The joint mode's counts, "shield_crash_proposed" [K] (the proposal would have crashed the agent),
        "shield_crash_final" [K] (the applied joint action does) and "shield_unavoidable" [K].
      shield_lookahead: the lookahead shield (``VecGridEnv.step_lookahead``): the crash-aware shield that also keeps
        off trap actions; ``shield_crash`` is implied; also "shield_trap_proposed" [K] and "shield_trap_replaced"
        [K].  Unilateral: ValueError with ``shield_mode="joint"`` or ``"joint_crash"``.
      shield_horizon: the horizon shield (``VecGridEnv.step_horizon``, an int H in 2..4): the crash-aware shield that
        picks among the masked actions that keep the agent alive longest over H steps; ``shield_crash`` is implied;
        also "shield_doomed_proposed" [K] (the proposal's depth was below H while a viable action existed),
        "shield_doomed_replaced" [K] and "shield_no_viable" [K].  Unilateral: ValueError with a joint mode or
        with ``shield_lookahead=True``.
      shield_plan: the plan shield (``VecGridEnv.step_plan``, an int H in 2..4): the crash-aware shield that picks
        among the masked actions that keep the agent alive longest over H steps and, of those, collect the most
        env reward ("plan_mask"); ``shield_crash`` is implied; also "shield_plan_proposed_off" [K] (the proposal
        was not in the plan mask) and "shield_plan_replaced" [K].  Unilateral: ValueError with a joint mode, with
        ``shield_lookahead=True`` or with ``shield_horizon``.  ``actors=None`` with ``shield_plan=H`` is the
        policy-free planner, a model-predictive baseline: every RL agent proposes 0 and takes the lowest action of
        its plan mask, re-planned every step (``actors=None`` without ``shield_plan`` is a ValueError)."""
    check_shield_args(shield_mode, shield_crash, "evaluate", shield_lookahead, shield_horizon, shield_plan)
    if actors is None and shield_plan is None:
        raise ValueError("evaluate(actors=None) needs shield_plan=H: the policy-free planner")
    for kw, on in (("fear_regret=True", fear_regret), ("feal=True", feal), ("resp_full=True", resp_full),
                   ("resp_map=True", resp_map), ("resp_footprint=R", resp_footprint is not None)):
        if on and not fear:
            raise ValueError(f"evaluate({kw}) needs fear=True")
    footprint = resp_footprint is not None
    sc = builtin(scenario) if isinstance(scenario, str) else scenario
    if actors is None:
        fused = False
    if fused is None:
        fused = actors.fusable(SimpleNamespace(K=sc.K, H=sc.H, W=sc.W))
    # the fused actor reads the obs descriptors: no dense obs is written at all
    env = VecGridEnv(sc, num_envs=episodes, fear=fear, max_steps=max_steps, auto_reset=False, seed=seed,
                     obs=not fused and actors is not None, variant=variant, fear_rows=resp_matrix, fear_alt=fear_regret, feal=feal,
                     fear_full=resp_full or resp_map or footprint, debug=footprint)
    try:
        obs, mask = env.reset()
        dev = env.device
        active = torch.ones(episodes, dtype=torch.uint8, device=dev)
        counts = torch.zeros(3, dtype=torch.int64, device=dev)       # crashes, apples, steps
        fear_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        lib = _lib.load()
        folds, cells = build_folds(env, "evaluate", resp_matrix, fear_regret, feal, resp_full, resp_map, resp_footprint)
        guard = None
        if (shield is not None or shield_crash or shield_lookahead or shield_horizon is not None
                or shield_plan is not None or shield_mode == "joint_crash"):
            guard = Shield(env, shield, shield_mode, shield_sweeps, shield_crash, count_crash=True, who="evaluate",
                           lookahead=shield_lookahead, horizon=shield_horizon, plan=shield_plan)
        stay = torch.zeros((episodes, env.K), dtype=torch.int32, device=dev) if actors is None else None
        recorded = []
        alive = torch.zeros(max_steps, dtype=torch.bool, device=dev) if record_actions else None
        for i in range(max_steps):
            if actors is None:  # the policy-free planner: the shield alone decides
                actions, probs = stay, None
            elif fused:  # one kernel over the obs descriptors (include/actor_ops.h)
                actions, probs = actors.act_env(env, env.out["mask"], training=False)
            else:
                actions, probs = actors.act(env.out["obs"], env.out["mask"], training=False)
            if guard is not None:  # actor -> preview(s) -> shield -> step
                actions = guard.apply(env, actions, None if probs is None else probs.contiguous(), env.out["mask"],
                                      active=active)
            if record_actions:
                recorded.append(actions.clone())
            if cells is not None:  # the step's pre-move cells
                env.copy_pos(cells)
            r = env.step(actions)
            for f in folds:  # the active envs' outputs, before gw_eval_accum retires the done ones
                f.fold(env, env.out, active=active)
            # the active envs' crashes, apples, steps and FeAR summed, then the done ones retired
            _lib.check(lib.gw_eval_accum(r.crashes.data_ptr(), r.apples.data_ptr(), r.fear.data_ptr(),
                                         r.done.data_ptr(), active.data_ptr(), counts.data_ptr(), fear_sum.data_ptr(),
                                         episodes, env.K, torch.cuda.current_stream(dev).cuda_stream),
                       "gw_eval_accum")
            if record_actions:
                alive[i] = active.any()  # device-side: is any episode still running after step i
            # a host sync every 8 steps: stepping envs whose episode ended changes no total
            # (they are masked out), so checking late only costs the few extra steps
            if i % 8 == 7 and not bool(active.any()):
                break
        c = counts.tolist()
        out = {"episodes": episodes, "crashes": c[0], "apples_caught": c[1], "steps": c[2], "fear": float(fear_sum)}
        parts, widths = fold_parts(folds)
        for key, v in fold_results(folds, widths, torch.cat(parts) if parts else None).items():
            if key in _MEANS:  # per active env-step
                out[_MEANS[key]] = v / max(c[2], 1)
            elif key not in _UNUSED:
                out[key] = v
        if guard is not None:
            out.update(guard.totals())
        if record_actions:
            # the early-stop check runs every 8 steps: keep the actions up to the first step after
            # which every episode had ended (the steps an env-at-a-time loop would have taken)
            n = len(recorded)
            dead = (~alive[:n]).nonzero()
            if dead.numel():
                n = int(dead[0, 0]) + 1
            out["actions"] = torch.stack(recorded[:n])
        return out
    finally:
        env.close()
