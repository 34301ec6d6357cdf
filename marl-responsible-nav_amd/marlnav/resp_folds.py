"""The responsibility folds and the responsibility shield that ``Rollout`` and ``evaluate`` share.

A fold sums one of the step's FeAR outputs over the envs into a running total, one launch per step (also
inside ``Rollout.capture`` graphs), optionally over the envs of an ``active`` mask only (``evaluate``: the
episodes still running).  Every fold has the same four parts:
  ``Fold(env, who, ...)``         checks the ``env.out`` keys it reads (ValueError naming the caller ``who`` and
                                  its keyword) and allocates its buffers;
  ``fold(env, out, active=None)`` the step's launch on the current stream; ``out`` is ``env.out``;
  ``parts()``                     the 1-D float64 tensors it adds to the caller's one float64 all-reduce;
  ``results(flat, all_reduce)``   its result keys from its slice ``flat`` of that vector (the parts
                                  concatenated, summed over the ranks); int64 counts are all-reduced here,
                                  in collectives of their own.
``build_folds`` arms them from the keywords, ``fold_parts`` / ``fold_results`` cut the vector by the parts'
own sizes.  A new fold is a class with these four parts and a line in ``build_folds``.
"""
from __future__ import annotations

import torch

from . import _lib


def _stream(env):
    return torch.cuda.current_stream(env.device).cuda_stream


def _need(env, who: str, kw: str, flag: str, *keys: str, why: str = ""):
    if any(env.out.get(k) is None for k in keys):
        raise ValueError(f"{who}({kw}) needs VecGridEnv({flag})" + why)


def _summed(t: torch.Tensor, all_reduce) -> torch.Tensor:
    """An int64 device buffer on the host, summed over the ranks first if there are several (exact)."""
    if all_reduce is None:
        return t.cpu()
    t = t.clone()  # (the all-reduce is in place)
    all_reduce(t)
    return t.cpu()


class RowFold:
    """``resp_matrix`` (an env with ``fear_rows=True``): every step's per-pair responsibility rows
    (StepResult.fear_row: how much RL agent k restricted agent j) summed over the envs into a [K, N] total;
    keys "resp", "resp_steps".
    ``resp_full`` (``fear_full=True``): the same fold with every world agent, RL or scripted, as actor
    (StepResult.resp_full, K = N) into an [N, N] total; keys "resp_full", "resp_full_steps".
    gw_fear_row_accum: a fixed summation order, so a graph replay equals the eager run bit for bit.  The step
    counts are this rank's (the ranks step in lockstep) and are not summed over them."""

    def __init__(self, env, who: str, full: bool = False):
        self.src, self.key = ("resp_full", "resp_full") if full else ("fear_row", "resp")
        _need(env, who, "resp_full=True" if full else "resp_matrix=True",
              "fear_full=True" if full else "fear_rows=True", self.src)
        self.rows = env.N if full else env.K
        self.total = torch.zeros((self.rows, env.N), dtype=torch.float64, device=env.device)
        self.steps = torch.zeros((), dtype=torch.int64, device=env.device)

    def fold(self, env, out, active=None):
        _lib.check(env.lib.gw_fear_row_accum(out[self.src].data_ptr(), None if active is None else active.data_ptr(),
                                             env.E, self.rows, env.N, self.total.data_ptr(), self.steps.data_ptr(),
                                             _stream(env)), "gw_fear_row_accum")

    def parts(self):
        return [self.total.reshape(-1)]

    def results(self, flat, all_reduce=None):
        return {self.key: flat.reshape(self.total.shape).cpu(), self.key + "_steps": int(self.steps)}


class RegretFold:
    """``fear_regret`` (an env with ``fear_alt=True``): every step's hindsight FeAR regret, fear[e, k] -
    min_a fear_alt[e, k, a] (the minimum over all nine actions), and the count of envs whose agent k took a
    FeAR-minimal action, summed over the envs (gw_fear_regret_accum); keys "fear_regret" [K], "fear_best" [K]
    (env-steps) and "fear_regret_steps"."""

    def __init__(self, env, who: str):
        _need(env, who, "fear_regret=True", "fear_alt=True", "fear_alt")
        self.total = torch.zeros((env.K, 2), dtype=torch.float64, device=env.device)
        self.steps = torch.zeros((), dtype=torch.int64, device=env.device)

    def fold(self, env, out, active=None):
        _lib.check(env.lib.gw_fear_regret_accum(out["fear_alt"].data_ptr(), out["fear"].data_ptr(),
                                                None if active is None else active.data_ptr(), env.E, env.K,
                                                self.total.data_ptr(), self.steps.data_ptr(), _stream(env)),
                   "gw_fear_regret_accum")

    def parts(self):
        return [self.total.reshape(-1)]

    def results(self, flat, all_reduce=None):
        reg = flat.reshape(self.total.shape).cpu()
        return {"fear_regret": reg[:, 0].clone(), "fear_best": reg[:, 1].clone(),
                "fear_regret_steps": int(self.steps)}


class FealFold:
    """``feal`` (an env with ``feal=True``): every step's per-agent FeAL (StepResult.feal) summed over the envs
    into an [N] total, with the env-steps summed (gw_feal_accum); keys "feal_sum" [N], "feal_envs" (over all
    ranks: feal_sum / feal_envs is the mean FeAL) and "feal_steps"."""

    def __init__(self, env, who: str):
        _need(env, who, "feal=True", "feal=True", "feal")
        self.total = torch.zeros(env.N, dtype=torch.float64, device=env.device)
        self.cnt = torch.zeros(2, dtype=torch.int64, device=env.device)  # steps, env-steps

    def fold(self, env, out, active=None):
        cnt = self.cnt.data_ptr()
        _lib.check(env.lib.gw_feal_accum(out["feal"].data_ptr(), None if active is None else active.data_ptr(),
                                         env.E, env.N, self.total.data_ptr(), cnt, cnt + 8, _stream(env)),
                   "gw_feal_accum")

    def parts(self):  # the env-step count rides along as a double (exact below 2^53)
        return [self.total, self.cnt[1:2].to(torch.float64)]

    def results(self, flat, all_reduce=None):
        return {"feal_sum": flat[:-1].cpu(), "feal_envs": int(flat[-1]), "feal_steps": int(self.cnt[0])}


class MapFold:
    """``resp_map`` (an env with ``fear_full=True``; arms ``resp_full``): where on the grid the agents restrict
    each other.  The step's valid-action sets are binned by the agents' pre-move cells (``cells``, filled by
    ``env.copy_pos`` before the step; gw_resp_map_accum); keys "resp_map_counts" (int64 [2, H*W, 10, 10]: plane
    0 caused at the actor's cell, plane 1 received at the affected agent's cell), "resp_map_visits" (int64
    [H*W], agent-steps per cell) and the derived "resp_map" ([2, H, W] f64, the summed Resp per cell:
    ``marlnav.resp_map_from_counts``).  The device keeps integer counts, so the totals are the same bit for
    bit eager or replayed, and several ranks all-reduce the integers."""

    def __init__(self, env, who: str, cells: torch.Tensor):
        _need(env, who, "resp_map=True", "fear_full=True", "resp_valid")
        hw = env.H * env.W
        self.cells, self.hw = cells, (env.H, env.W)
        self.counts = torch.zeros((2, hw, 10, 10), dtype=torch.int64, device=env.device)
        self.visits = torch.zeros(hw, dtype=torch.int64, device=env.device)

    def fold(self, env, out, active=None):
        env.resp_map_accum(out["resp_valid"], self.cells, self.counts, self.visits, active=active)

    def parts(self):
        return []

    def results(self, flat=None, all_reduce=None):
        from .resp_map import resp_map_from_counts
        cnt, vis = _summed(self.counts, all_reduce), _summed(self.visits, all_reduce)
        return {"resp_map_counts": cnt, "resp_map_visits": vis,
                "resp_map": resp_map_from_counts(cnt)[0].reshape(2, *self.hw)}


class FootprintFold:
    """``resp_footprint`` (a radius R in 1..15; an env with ``fear_full=True`` and ``debug=True``, whose steps
    report ``actions`` and ``crash_bits``): how far, and in which direction, an action restricts others.  The
    step's sets are binned by the actor's action and the affected agent's offset from it (on the cells
    ``MapFold`` uses), the affected agents that crashed in the step into a second plane
    (gw_resp_footprint_accum); keys "resp_footprint_counts" (int64 [2, 9, O, 10, 10], O = (2R + 1)^2 + 1: the
    near offsets row-major, then the far bin), "resp_footprint_visits" (int64 [9], actor-steps per action) and
    the derived "resp_footprint" ([2, 9, O] f64: ``marlnav.resp_footprint_from_counts``).  Integer counts,
    all-reduced as integers."""

    def __init__(self, env, who: str, cells: torch.Tensor, radius: int):
        _need(env, who, "resp_footprint=R", "fear_full=True", "resp_valid")
        _need(env, who, "resp_footprint=R", "debug=True", "actions", "crash_bits",
              why=" (the step's actions and crash_bits)")
        self.cells, self.radius = cells, int(radius)
        if not 1 <= self.radius <= 15:
            raise ValueError(f"{who}(resp_footprint=R): R in 1..15")
        n_off = (2 * self.radius + 1) ** 2 + 1
        self.counts = torch.zeros((2, 9, n_off, 10, 10), dtype=torch.int64, device=env.device)
        self.visits = torch.zeros(9, dtype=torch.int64, device=env.device)

    def fold(self, env, out, active=None):
        env.resp_footprint_accum(out["resp_valid"], self.cells, out["actions"], self.counts, self.visits,
                                 crash_bits=out["crash_bits"], active=active, radius=self.radius)

    def parts(self):
        return []

    def results(self, flat=None, all_reduce=None):
        from .resp_footprint import resp_footprint_from_counts
        cnt, vis = _summed(self.counts, all_reduce), _summed(self.visits, all_reduce)
        return {"resp_footprint_counts": cnt, "resp_footprint_visits": vis,
                "resp_footprint": resp_footprint_from_counts(cnt)[0]}


def build_folds(env, who: str, resp_matrix: bool = False, fear_regret: bool = False, feal: bool = False,
                resp_full: bool = False, resp_map: bool = False, resp_footprint: int | None = None):
    """-> (the armed folds in the order they are launched and reduced: rows, regret, FeAL, full, map,
    footprint; the [N, E] int32 cells buffer the caller fills with ``env.copy_pos`` before every step, or None).
    ``resp_map`` arms ``resp_full``; map and footprint share the cells buffer.  ``who`` is the caller's name in
    the ValueErrors ("Rollout", "evaluate")."""
    cells = None
    if resp_map or resp_footprint is not None:
        cells = torch.empty((env.N, env.E), dtype=torch.int32, device=env.device)
    folds = [cls(env, who) for on, cls in ((resp_matrix, RowFold), (fear_regret, RegretFold), (feal, FealFold)) if on]
    binned = [MapFold(env, who, cells)] if resp_map else []
    if resp_footprint is not None:
        binned.append(FootprintFold(env, who, cells, resp_footprint))
    if resp_full or resp_map:
        folds.append(RowFold(env, who, full=True))
    return folds + binned, cells


def fold_parts(folds):
    """-> (every fold's float64 parts in order, as one list for ``torch.cat``; each fold's width in it)."""
    parts = [f.parts() for f in folds]
    return [p for ps in parts for p in ps], [sum(p.numel() for p in ps) for ps in parts]


GW_HORIZON_MAX = 4  # include/gridenv.h


def fold_results(folds, widths, flat, all_reduce=None) -> dict:
    """Every fold's result keys: fold i reads the next ``widths[i]`` doubles of ``flat`` (``fold_parts``
    concatenated and summed over the ranks).  ``all_reduce`` (several ranks: an in-place sum, None otherwise) is
    called on a copy of each int64 count, in fold order after the caller's float64 all-reduce."""
    out, off = {}, 0
    for f, n in zip(folds, widths):
        out.update(f.results(flat[off:off + n] if n else None, all_reduce))
        off += n
    return out


def check_shield_args(shield_mode: str, shield_crash: bool, who: str = "Rollout", shield_lookahead: bool = False,
                      shield_horizon: int | None = None, shield_plan: int | None = None):
    """The shield keywords' checks (no device needed)."""
    if shield_plan is not None:
        if isinstance(shield_plan, bool) or not 2 <= int(shield_plan) <= GW_HORIZON_MAX:
            raise ValueError(f"{who}(shield_plan=...): None or an int in 2..{GW_HORIZON_MAX}")
        if shield_lookahead or shield_horizon is not None:
            raise ValueError(f"{who}(shield_plan={shield_plan}) with shield_lookahead or shield_horizon: the plan shield "
                             "looks ahead itself; pick one")
        if shield_mode in ("joint", "joint_crash"):
            raise ValueError(f'{who}(shield_plan={shield_plan}) with shield_mode="{shield_mode}": the plan shield is '
                             "unilateral")
    if shield_horizon is not None:
        if isinstance(shield_horizon, bool) or not 2 <= int(shield_horizon) <= GW_HORIZON_MAX:
            raise ValueError(f"{who}(shield_horizon=...): None or an int in 2..{GW_HORIZON_MAX}")
        if shield_lookahead:
            raise ValueError(f"{who}(shield_horizon={shield_horizon}) with shield_lookahead=True: the horizon shield at "
                             "horizon 2 is the lookahead shield; pick one")
        if shield_mode in ("joint", "joint_crash"):
            raise ValueError(f'{who}(shield_horizon={shield_horizon}) with shield_mode="{shield_mode}": the horizon '
                             "shield is unilateral")
    if shield_mode not in ("unilateral", "joint", "joint_crash"):
        raise ValueError(f'{who}(shield_mode=...): "unilateral", "joint" or "joint_crash"')
    if shield_lookahead and shield_mode != "unilateral":
        raise ValueError(f'{who}(shield_lookahead=True) with shield_mode="{shield_mode}": the lookahead shield is '
                         "unilateral")
    if shield_crash and shield_mode == "joint":
        raise ValueError(f'{who}(shield_crash=True) with shield_mode="joint": the crash-aware shield is unilateral')


class Shield:
    """The responsibility shield between the actor and the step (eager only), with preallocated buffers.
    ``apply`` runs one of three pipelines and returns the actions to step with:
      unilateral (``tau`` a float): ``env.fear_preview`` of the proposed actions, then ``env.fear_shield`` (the
        env's action mask, the actor's probabilities, every RL agent shielded); each agent's row assumes that
        the others keep their proposed actions;
      joint (``mode="joint"``): the one call ``env.fear_shield_joint`` (the agents visited one after the other,
        at most ``sweeps`` sweeps); ``table`` then holds the [E, K, 9] FeAR table of the joint action the step
        applies and ``flags`` carries bits 2 (over tau) and 3 (unconverged) too;
      crash-aware (``crash=True``, unilateral only): ``env.step_preview`` after the FeAR preview, and the shield
        called with its "safe_mask" (the action mask without the actions under which the agent itself would
        crash) in the action mask's place; ``crash9`` holds the last step's [E, K] own-crash sets.  With
        ``tau=None`` the table is a zero table under tau = 0: only crashing proposals are replaced, by the most
        probable safe action.  An agent moved to a safe action is crash-free only in envs where every other
        agent's action was kept.
      coordinated crash-aware (``mode="joint_crash"``; ``crash`` is implied): the one call
        ``env.crash_shield_joint``, the crash preview inside the joint sweeps: every visit previews the agent's nine
        actions against the actions fixed so far.  ``tau=None`` is crash-only, a float adds FeAR (``table`` is then
        set); ``crash9`` holds the own-crash sets under the applied joint action, ``flags`` carries bits 4 (the
        agent crashes in the step) and 5 (its last visit had no crash-free masked action) too.
      lookahead (``lookahead=True``, unilateral only; ``crash`` is implied): the crash-aware pipeline with
        ``env.step_lookahead`` in ``step_preview``'s place and its "ahead_mask" in the safe mask's: the trap actions
        (after which every action the agent's new cell allows crashes it in the step after, the other RL agents
        staying) are taken out too.  ``trap9`` holds the last step's [E, K] trap sets.
      horizon (``horizon=H``, unilateral only; ``crash`` is implied): the crash-aware pipeline with
        ``env.step_horizon(horizon=H)`` in ``step_preview``'s place and its "horizon_mask" (the masked actions that
        keep the agent alive longest over H steps, the other RL agents staying after the first) in the safe
        mask's.  ``depth`` / ``viable9`` hold the last step's [E, K, 9] depths and [E, K] viable sets.
      plan (``plan=H``, unilateral only, not with lookahead or horizon; ``crash`` is implied): the crash-aware
        pipeline with ``env.step_plan(horizon=H)`` in ``step_preview``'s place and its "plan_mask" (of the masked
        actions that keep the agent alive longest over H steps, the ones whose best continuation collects the most
        env reward) in the safe mask's.  ``depth`` / ``ret`` / ``plan_mask`` hold the last step's tables.  With
        ``probs=None`` or one-hot probabilities ``env.fear_shield`` picks the lowest action of the plan mask:
        the policy-free planner.
    ``flags`` holds the last step's [E, K] uint8 flags.  ``totals()``: "shield_replaced" [K] and "shield_stuck"
    [K] (int64 CPU tensors: the agent-steps whose action was replaced, flag bit 0 / that had no allowed action,
    bit 1); joint: also "shield_over" [K] (the applied action's FeAR exceeds tau, bit 2) and
    "shield_unconverged" (env-steps whose last sweep still changed an action, bit 3); ``count_crash``: also
    "shield_crash_proposed" [K] and "shield_crash_replaced" [K] (the agent-steps whose proposed action would
    have crashed the agent itself / of those, the ones replaced); joint_crash: the joint mode's four counts,
    "shield_crash_proposed" [K] (agent k crashes in the step the proposal would have run), "shield_crash_final" [K]
    (it crashes in the step that was run, bit 4) and "shield_unavoidable" [K] (bit 5); lookahead: also
    "shield_trap_proposed" [K] and "shield_trap_replaced" [K] (the agent-steps whose proposed action was a trap
    action / of those, the ones replaced); horizon: also "shield_doomed_proposed" [K] (the proposal's depth was
    below H while some action of the mask was viable), "shield_doomed_replaced" [K] (of those, the ones replaced)
    and "shield_no_viable" [K] (no action of the mask was viable); plan: also "shield_plan_proposed_off" [K] (the
    proposal was not in the plan mask) and "shield_plan_replaced" [K] (of those, the ones replaced)."""

    def __init__(self, env, tau: float | None, mode: str = "unilateral", sweeps: int = 2, crash: bool = False,
                 count_crash: bool = False, who: str = "Rollout", lookahead: bool = False, horizon: int | None = None,
                 plan: int | None = None):
        check_shield_args(mode, crash, who, lookahead, horizon, plan)
        self.lookahead = bool(lookahead)
        self.horizon = None if horizon is None else int(horizon)
        self.plan = None if plan is None else int(plan)
        crash = bool(crash) or self.lookahead or self.horizon is not None or self.plan is not None
        E, K, dev = env.E, env.K, env.device
        self.tau = None if tau is None else float(tau)
        self.joint_crash = mode == "joint_crash"
        self.joint, self.sweeps = mode == "joint" or self.joint_crash, int(sweeps)
        self.crash = bool(crash) or self.joint_crash
        # replaced, stuck; joint mode: over tau, unconverged (bit 3 is the same for an env's K entries)
        self.cnt = torch.zeros((4 if self.joint else 2, K), dtype=torch.int64, device=dev)
        # crashing proposals, of those replaced
        self.crash_cnt = torch.zeros((2, K), dtype=torch.int64, device=dev) if crash and count_crash else None
        # trap proposals, of those replaced
        self.trap_cnt = torch.zeros((2, K), dtype=torch.int64, device=dev) if self.lookahead else None
        self.trap9 = None
        # doomed proposals, of those replaced, agent-steps without a viable action
        self.doomed_cnt = torch.zeros((3, K), dtype=torch.int64, device=dev) if self.horizon is not None else None
        self.depth = self.viable9 = None
        # proposals outside the plan mask, of those replaced
        self.plan_cnt = torch.zeros((2, K), dtype=torch.int64, device=dev) if self.plan is not None else None
        self.ret = self.plan_mask = None
        if self.joint_crash:  # proposal crashes, final crashes, unavoidable
            self.crash_cnt = torch.zeros((3, K), dtype=torch.int64, device=dev)
            self._outcome_prop = torch.empty(E, dtype=torch.int16, device=dev)
            self._agent_bit = torch.arange(K, dtype=torch.int64, device=dev).unsqueeze(0)
            self._flag_bit = torch.arange(6, dtype=torch.uint8, device=dev).reshape(6, 1, 1)
        # the crash shield alone: a zero table under tau = 0, so that only the safe mask decides
        self._table = (torch.zeros if tau is None else torch.empty)((E, K, 9), dtype=torch.float64, device=dev)
        self._out = torch.empty((E, K), dtype=torch.int32, device=dev)
        self.flags = torch.zeros((E, K), dtype=torch.uint8, device=dev)
        self.table = self._table if self.joint and not (self.joint_crash and tau is None) else None
        self.crash9 = torch.empty((E, K), dtype=torch.int16, device=dev) if self.joint_crash else None
        if not self.joint:  # the preview's joint action: the random policy's proposals are read from it
            self._joint = torch.empty((E, env.N), dtype=torch.int32, device=dev)

    def apply(self, env, actions, probs, mask, active=None):
        """actor -> preview(s) -> shield: the actions the step will apply, and the flags into the counts
        (weighted by ``active`` [E] uint8 if given).  ``actions=None``: the device-random policy, whose
        proposals are the draws the step would make."""
        on = None if active is None else active.to(torch.int64).unsqueeze(1)

        def count(cnt, bits):
            cnt += (bits if on is None else bits * on).sum(0)

        if self.joint_crash:
            r = env.crash_shield_joint(actions, None, mask=mask, probs=probs, tau=self.tau, sweeps=self.sweeps,
                                       out=self._out, flags=self.flags, table=self.table,
                                       outcome_prop=self._outcome_prop, crash9=self.crash9)
            bits = ((r["flags"].unsqueeze(0) >> self._flag_bit) & 1).to(torch.int64)  # [6, E, K], one pass
            per_bit = (bits if on is None else bits * on).sum(1)
            self.cnt += per_bit[:4]
            self.crash_cnt[1:] += per_bit[4:]
            count(self.crash_cnt[0], (self._outcome_prop.to(torch.int64).unsqueeze(1) >> self._agent_bit) & 1)
            return r["actions"]
        if self.joint:
            out, flags, _ = env.fear_shield_joint(actions, None, mask=mask, probs=probs, tau=self.tau,
                                                  sweeps=self.sweeps, out=self._out, flags=self.flags,
                                                  table=self._table)
            for b in range(4):
                count(self.cnt[b], (flags >> b) & 1)
            return out
        if self.tau is not None:
            if actions is None:  # the preview reports the actions the step would draw
                env.fear_preview(None, out=self._table, actions=self._joint)
                actions = self._joint[:, :env.K].contiguous()
            else:
                env.fear_preview(actions, out=self._table)
        if self.crash:  # the shield picks among the actions under which the agent itself does not crash
            m_in = mask
            if self.plan is not None:  # ... that keeps the agent alive longest and collects the most reward
                sp = env.step_plan(actions, None, mask=mask, horizon=self.plan)
                self.depth, self.ret, self.plan_mask = sp["depth"], sp["ret"], sp["plan_mask"]
            elif self.horizon is not None:  # ... and that keeps the agent alive longest
                sp = env.step_horizon(actions, None, mask=mask, horizon=self.horizon)
                self.depth, self.viable9 = sp["depth"], sp["viable9"]
            elif self.lookahead:  # ... and that is no trap action
                sp = env.step_lookahead(actions, None, mask=mask)
            else:
                sp = env.step_preview(actions, None, mask=mask, reward=False)
            if actions is None:
                actions = sp["actions"][:, :env.K].contiguous()
            which = ("plan_mask" if self.plan is not None else "horizon_mask" if self.horizon is not None else
                     "ahead_mask" if self.lookahead else "safe_mask")
            mask, self.crash9 = sp[which], sp["crash9"]
            self.trap9 = sp.get("trap9")
        out, flags = env.fear_shield(self._table, actions, mask=mask, probs=probs,
                                     tau=0.0 if self.tau is None else self.tau, out=self._out, flags=self.flags)
        if self.crash_cnt is not None:
            bad = (self.crash9.to(torch.int64) >> actions.to(torch.int64)) & 1
            count(self.crash_cnt[0], bad)
            count(self.crash_cnt[1], bad * (out != actions).to(torch.int64))
        if self.trap_cnt is not None:
            trap = (self.trap9.to(torch.int64) >> actions.to(torch.int64)) & 1
            count(self.trap_cnt[0], trap)
            count(self.trap_cnt[1], trap * (out != actions).to(torch.int64))
        if self.doomed_cnt is not None:
            via = self.viable9.to(torch.int64) & (0x1FF if m_in is None else m_in.to(torch.int64) & 0x1FF)
            some = (via != 0).to(torch.int64)
            doomed = (1 - ((self.viable9.to(torch.int64) >> actions.to(torch.int64)) & 1)) * some
            count(self.doomed_cnt[0], doomed)
            count(self.doomed_cnt[1], doomed * (out != actions).to(torch.int64))
            count(self.doomed_cnt[2], 1 - some)
        if self.plan_cnt is not None:
            off = 1 - ((self.plan_mask.to(torch.int64) >> actions.to(torch.int64)) & 1)
            count(self.plan_cnt[0], off)
            count(self.plan_cnt[1], off * (out != actions).to(torch.int64))
        count(self.cnt[0], flags & 1)
        count(self.cnt[1], flags >> 1)
        return out

    def totals(self, all_reduce=None) -> dict:
        """The counts as CPU tensors (several ranks: summed in one integer all-reduce of their own)."""
        out = {}
        if self.joint_crash:
            cc = _summed(self.crash_cnt, all_reduce)
            out["shield_crash_proposed"], out["shield_crash_final"], out["shield_unavoidable"] = cc[0], cc[1], cc[2]
        elif self.crash_cnt is not None:
            cc = _summed(self.crash_cnt, all_reduce)
            out["shield_crash_proposed"], out["shield_crash_replaced"] = cc[0], cc[1]
        if self.trap_cnt is not None:
            tc = _summed(self.trap_cnt, all_reduce)
            out["shield_trap_proposed"], out["shield_trap_replaced"] = tc[0], tc[1]
        if self.doomed_cnt is not None:
            dc = _summed(self.doomed_cnt, all_reduce)
            out["shield_doomed_proposed"], out["shield_doomed_replaced"], out["shield_no_viable"] = dc[0], dc[1], dc[2]
        if self.plan_cnt is not None:
            pc = _summed(self.plan_cnt, all_reduce)
            out["shield_plan_proposed_off"], out["shield_plan_replaced"] = pc[0], pc[1]
        cnt = _summed(self.cnt, all_reduce)
        out["shield_replaced"], out["shield_stuck"] = cnt[0], cnt[1]
        if self.joint:
            out["shield_over"], out["shield_unconverged"] = cnt[2], int(cnt[3, 0])
        return out
