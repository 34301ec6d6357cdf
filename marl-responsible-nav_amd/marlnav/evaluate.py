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
from .scenario import builtin
from .vec_env import VecGridEnv


@torch.no_grad()
def evaluate(actors: MultiAgentActors, scenario="level3", episodes: int = 100, max_steps: int = 150,
             fear: bool = False, seed: int = 42, record_actions: bool = False, fused: bool | None = None,
             variant: int = 0, resp_matrix: bool = False, fear_regret: bool = False,
             feal: bool = False, resp_full: bool = False, shield: float | None = None,
             shield_mode: str = "unilateral", shield_sweeps: int = 2, resp_map: bool = False,
             resp_footprint: int | None = None, shield_crash: bool = False) -> dict:
    """resp_matrix (with ``fear=True``): the result also carries "resp", the [K, N] responsibility
    matrix (f64 CPU tensor): every step's per-pair rows (StepResult.fear_row: how much RL agent k
    restricted agent j) summed over the episodes still running and divided by "steps".
    fear_regret (with ``fear=True``): the result also carries "fear_regret" [K], the policy's hindsight
    FeAR regret fear[e, k] - min_a fear_alt[e, k, a] (StepResult.fear_alt, the minimum over all nine
    actions) per active env-step, and "fear_best_frac" [K], how often agent k's action was
    FeAR-minimal (f64 CPU tensors).
    feal (with ``fear=True``): the result also carries "feal" [N], the mean Responsibility.FeAL of every
    world agent (StepResult.feal) per active env-step (f64 CPU tensor).
    resp_full (with ``fear=True``): the result also carries "resp_full", the [N, N] sum of every step's
    responsibility matrix with every world agent as actor (StepResult.resp_full: how much agent i, RL or
    scripted, restricted agent j) over the episodes still running (f64 CPU tensor; divide by "steps" for
    the mean per env-step), and "resp_full_steps", the batched steps it covers.
    resp_map (with ``fear=True``): the result also carries the responsibility maps of the episodes still
    running (gw_resp_map_accum with the ``active`` mask of the other folds, on the cells copied before each
    step): "resp_map" [2, H, W] f64 (plane 0: the Resp summed at the cell of the agent that caused it, plane
    1: at the cell of the agent that received it), "resp_map_counts" (int64 [2, H*W, 10, 10], the exact counts
    per cell and valid-action counts (vm, va) the map is formed from) and "resp_map_visits" (int64 [H*W],
    agent-steps per cell): ``resp_map.reshape(2, -1) / resp_map_visits`` is the mean per visit.
    resp_footprint (a radius R in 1..15, with ``fear=True``): the result also carries the responsibility
    footprint of the episodes still running (gw_resp_footprint_accum with the ``active`` mask, on the cells
    copied before each step, the step's joint action and its crash bits): "resp_footprint" [2, 9, O] f64 (per
    action of the actor and offset of the affected agent from it, O = (2R + 1)^2 + 1 with the far bin last, the
    Resp summed; plane 1: the affected agents that crashed in the step), "resp_footprint_counts" (int64
    [2, 9, O, 10, 10]) and "resp_footprint_visits" (int64 [9], actor-steps per action).
    shield (a float tau; None: off): the responsibility shield at inference time.  Every step runs actor,
    ``env.fear_preview`` of the proposed actions, ``env.fear_shield`` (the env's action mask, the actor's
    probabilities, every RL agent shielded), then ``env.step`` with the shielded actions; works with
    ``fear=False`` (the reference's evaluation configuration).  The result also carries "shield_replaced" [K]
    and "shield_stuck" [K] (int64 CPU tensors): the agent-steps of the episodes still running whose action
    was replaced / that had no allowed action.  Recorded actions are the ones applied.
    shield_mode: "unilateral" (the default, the two calls above) or "joint": the one call
    ``env.fear_shield_joint`` with at most ``shield_sweeps`` sweeps (the agents visited one after the other, each
    on the actions fixed so far).  The result then also carries "shield_over" [K] (the agent-steps, counted as
    the other two, whose applied action's FeAR exceeds tau: flag bit 2) and "shield_unconverged" (the env-steps
    whose last sweep still changed an action: flag bit 3).
    shield_crash (default off): the crash-aware shield.  The loop becomes actor -> (``env.fear_preview``) ->
    ``env.step_preview`` -> ``env.fear_shield`` -> ``env.step``, the shield called with the preview's "safe_mask"
    (the action mask without the actions under which the agent itself would crash) in the action mask's place.
    With ``shield=None`` the FeAR table is a zero table allocated once and tau = 0: only crashing proposals are
    replaced, by the most probable safe action.  The result also carries "shield_crash_proposed" [K] and
    "shield_crash_replaced" [K] (int64 CPU tensors): the agent-steps of the episodes still running whose proposed
    action would have crashed the agent itself / of those, the ones the shield replaced, beside
    "shield_replaced" and "shield_stuck".  Unilateral like the FeAR shield: an agent moved to a safe action is
    crash-free only in envs where every other agent's action was kept.  With ``shield_mode="joint"`` it raises
    ValueError."""
    if shield_crash and shield_mode == "joint":
        raise ValueError('evaluate(shield_crash=True) with shield_mode="joint": the crash-aware shield is unilateral')
    if shield_mode not in ("unilateral", "joint"):
        raise ValueError('evaluate(shield_mode=...): "unilateral" or "joint"')
    joint_mode = shield is not None and shield_mode == "joint"
    if fear_regret and not fear:
        raise ValueError("evaluate(fear_regret=True) needs fear=True")
    if feal and not fear:
        raise ValueError("evaluate(feal=True) needs fear=True")
    if resp_full and not fear:
        raise ValueError("evaluate(resp_full=True) needs fear=True")
    if resp_map and not fear:
        raise ValueError("evaluate(resp_map=True) needs fear=True")
    footprint = resp_footprint is not None
    if footprint and not fear:
        raise ValueError("evaluate(resp_footprint=R) needs fear=True")
    if footprint and not 1 <= int(resp_footprint) <= 15:
        raise ValueError("evaluate(resp_footprint=R): R in 1..15")
    sc = builtin(scenario) if isinstance(scenario, str) else scenario
    if fused is None:
        fused = actors.fusable(SimpleNamespace(K=sc.K, H=sc.H, W=sc.W))
    # the fused actor reads the obs descriptors: no dense obs is written at all
    env = VecGridEnv(sc, num_envs=episodes, fear=fear, max_steps=max_steps, auto_reset=False, seed=seed,
                     obs=not fused, variant=variant, fear_rows=resp_matrix, fear_alt=fear_regret, feal=feal,
                     fear_full=resp_full or resp_map or footprint, debug=footprint)
    try:
        obs, mask = env.reset()
        dev = env.device
        active = torch.ones(episodes, dtype=torch.uint8, device=dev)
        counts = torch.zeros(3, dtype=torch.int64, device=dev)       # crashes, apples, steps
        fear_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        lib = _lib.load()
        resp = torch.zeros((env.K, env.N), dtype=torch.float64, device=dev) if resp_matrix else None
        resp_calls = torch.zeros((), dtype=torch.int64, device=dev)
        regret = torch.zeros((env.K, 2), dtype=torch.float64, device=dev) if fear_regret else None
        regret_calls = torch.zeros((), dtype=torch.int64, device=dev)
        feal_sum = torch.zeros(env.N, dtype=torch.float64, device=dev) if feal else None
        feal_cnt = torch.zeros(2, dtype=torch.int64, device=dev)  # calls, env-steps
        full = torch.zeros((env.N, env.N), dtype=torch.float64, device=dev) if resp_full else None
        full_calls = torch.zeros((), dtype=torch.int64, device=dev)
        hw = env.H * env.W
        map_counts = torch.zeros((2, hw, 10, 10), dtype=torch.int64, device=dev) if resp_map else None
        map_visits = torch.zeros(hw, dtype=torch.int64, device=dev) if resp_map else None
        map_cells = torch.empty((env.N, episodes), dtype=torch.int32, device=dev) if resp_map or footprint else None
        if footprint:
            fp_counts = torch.zeros((2, 9, (2 * int(resp_footprint) + 1) ** 2 + 1, 10, 10), dtype=torch.int64, device=dev)
            fp_visits = torch.zeros(9, dtype=torch.int64, device=dev)
        table = torch.empty((episodes, env.K, 9), dtype=torch.float64, device=dev) if shield is not None else None
        if shield_crash and shield is None:  # a zero table under tau = 0: only the safe mask decides
            table = torch.zeros((episodes, env.K, 9), dtype=torch.float64, device=dev)
        crash_cnt = torch.zeros((2, env.K), dtype=torch.int64, device=dev)  # crashing proposals, of those replaced
        # replaced, stuck; joint mode: over tau, unconverged (bit 3 is the same for an env's K entries)
        shield_cnt = torch.zeros((4 if joint_mode else 2, env.K), dtype=torch.int64, device=dev)
        recorded = []
        alive = torch.zeros(max_steps, dtype=torch.bool, device=dev) if record_actions else None
        for i in range(max_steps):
            if fused:  # one kernel over the obs descriptors (include/actor_ops.h)
                actions, probs = actors.act_env(env, env.out["mask"], training=False)
            else:
                actions, probs = actors.act(env.out["obs"], env.out["mask"], training=False)
            if joint_mode:  # actor -> the coordinated shield (one call) -> step
                actions, flags, _ = env.fear_shield_joint(actions, None, mask=env.out["mask"], probs=probs.contiguous(),
                                                          tau=float(shield), sweeps=shield_sweeps, table=table)
                on = active.to(torch.int64).unsqueeze(1)
                for b in range(4):
                    shield_cnt[b] += (((flags >> b) & 1) * on).sum(0)
            elif shield is not None or shield_crash:
                # actor -> preview(s) -> shield -> step; the episodes still running are counted
                on = active.to(torch.int64).unsqueeze(1)
                amask, proposed = env.out["mask"], actions
                if shield is not None:
                    env.fear_preview(actions, out=table)
                if shield_crash:  # the shield picks among the actions under which the agent itself does not crash
                    sp = env.step_preview(actions, None, mask=amask, reward=False)
                    amask = sp["safe_mask"]
                    bad = (sp["crash9"].to(torch.int64) >> proposed.to(torch.int64)) & 1
                actions, flags = env.fear_shield(table, actions, mask=amask, probs=probs.contiguous(),
                                                 tau=0.0 if shield is None else float(shield))
                if shield_crash:
                    crash_cnt[0] += (bad * on).sum(0)
                    crash_cnt[1] += (bad * (actions != proposed).to(torch.int64) * on).sum(0)
                shield_cnt[0] += ((flags & 1) * on).sum(0)
                shield_cnt[1] += ((flags >> 1) * on).sum(0)
            if record_actions:
                recorded.append(actions.clone())
            if map_cells is not None:  # the step's pre-move cells
                env.copy_pos(map_cells)
            r = env.step(actions)
            if resp_map:  # the active envs' sets binned by cell, likewise before the done ones are retired
                env.resp_map_accum(r.resp_valid, map_cells, map_counts, map_visits, active=active)
            if footprint:  # and by the actor's action and the affected agent's offset, likewise
                env.resp_footprint_accum(r.resp_valid, map_cells, r.actions, fp_counts, fp_visits,
                                         crash_bits=r.crash_bits, active=active, radius=int(resp_footprint))
            if resp_matrix:  # the active envs' Resp rows, before gw_eval_accum retires the done ones
                _lib.check(lib.gw_fear_row_accum(r.fear_row.data_ptr(), active.data_ptr(), episodes, env.K, env.N,
                                                 resp.data_ptr(), resp_calls.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "gw_fear_row_accum")
            if fear_regret:  # the active envs' regret, likewise before the done ones are retired
                _lib.check(lib.gw_fear_regret_accum(r.fear_alt.data_ptr(), r.fear.data_ptr(), active.data_ptr(),
                                                    episodes, env.K, regret.data_ptr(), regret_calls.data_ptr(),
                                                    torch.cuda.current_stream(dev).cuda_stream),
                           "gw_fear_regret_accum")
            if feal:  # the active envs' FeAL, likewise
                _lib.check(lib.gw_feal_accum(r.feal.data_ptr(), active.data_ptr(), episodes, env.N, feal_sum.data_ptr(),
                                             feal_cnt.data_ptr(), feal_cnt.data_ptr() + 8,
                                             torch.cuda.current_stream(dev).cuda_stream), "gw_feal_accum")
            if resp_full:  # the active envs' N x N matrices: the row fold with every agent an actor
                _lib.check(lib.gw_fear_row_accum(r.resp_full.data_ptr(), active.data_ptr(), episodes, env.N, env.N,
                                                 full.data_ptr(), full_calls.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "gw_fear_row_accum")
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
        if resp_matrix:
            out["resp"] = (resp / max(c[2], 1)).cpu()
        if fear_regret:
            reg = (regret / max(c[2], 1)).cpu()
            out["fear_regret"], out["fear_best_frac"] = reg[:, 0].clone(), reg[:, 1].clone()
        if feal:
            out["feal"] = (feal_sum / max(c[2], 1)).cpu()
        if resp_full:
            out["resp_full"], out["resp_full_steps"] = full.cpu(), int(full_calls)
        if resp_map:
            from .resp_map import resp_map_from_counts
            out["resp_map_counts"], out["resp_map_visits"] = map_counts.cpu(), map_visits.cpu()
            out["resp_map"] = resp_map_from_counts(out["resp_map_counts"])[0].reshape(2, env.H, env.W)
        if footprint:
            from .resp_footprint import resp_footprint_from_counts
            out["resp_footprint_counts"], out["resp_footprint_visits"] = fp_counts.cpu(), fp_visits.cpu()
            out["resp_footprint"] = resp_footprint_from_counts(out["resp_footprint_counts"])[0]
        if shield_crash:
            out["shield_crash_proposed"], out["shield_crash_replaced"] = crash_cnt[0].cpu(), crash_cnt[1].cpu()
        if shield is not None or shield_crash:
            out["shield_replaced"], out["shield_stuck"] = shield_cnt[0].cpu(), shield_cnt[1].cpu()
            if joint_mode:
                out["shield_over"], out["shield_unconverged"] = shield_cnt[2].cpu(), int(shield_cnt[3, 0])
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
