"""The two-step crash lookahead's reference (gw_step_lookahead): the C oracle stepped twice per (env, RL agent,
first action, second action) on copies of its state, as tests/_step_preview_ref.oracle_tables does once, and the
trap, mask and sim-count rules of include/gridenv.h restated in numpy.  The cases are _step_preview_ref.CASES'
shapes with seeds and step caps chosen here, on the CPU (tests/test_step_lookahead_cpu.py proves their coverage
from the oracle's own tables before any GPU run)."""
import dataclasses
import functools

import numpy as np

import _step_preview_ref as P
from oracle import oracle as O

NA, ALL = 9, 0x1FF

# max_steps = 7: the cap is reached inside the 16 steps of the run (all nine ends bits set at t = 6)
CASES = [dataclasses.replace(c, max_steps=7) for c in P.CASES]
CASE_IDS = [c.name for c in CASES]
STEPS = 16
COMPARE_AT = (0, 1, 3, 6, 9, 13)  # the steps compared (device-random RL actions at the odd ones); 6, 13: the cap
REPLAY_ROUNDS = 2
scenario_of, make_oracle, oracle_joint = P.scenario_of, P.make_oracle, P.oracle_joint
clustered_spawn = P.clustered_spawn


def _copy(env):
    return type(env).from_buffer_copy(env)


def oracle_lookahead(orc, sc, joint):
    """For every (e, k, a): the oracle env stepped once on a copy of its state with the joint action ``joint[e]``
    except that RL agent k plays a (auto_reset off): its ``done`` is the ends bit, ``mask[k]`` is mask2, bit k of
    its crash bits the crash9 bit.  Where it is not done, for each b one more step from there with RL actions zero
    except k playing b and the oracle's own scripted draws: bit k of its crash bits is bit b of crash2.  The
    oracle's state is left as it was.  -> dict of int64 arrays: crash2 [E, K, 9], ends / crash9 [E, K],
    mask2 [E, K, 9], scripted2 [E, K, 9, N - K] (the second step's scripted actions; -1 where the step ends) and
    the counts of how a step ended: "end_eaten" (every apple gone, no RL crash), "end_cap" (the step cap alone),
    "end_other" (k itself fine, another RL agent crashed), "cap_all_nine" (the (e, k) at the step cap: all nine
    bits set)."""
    E, K, N = orc.E, sc.K, sc.N
    crash2 = np.zeros((E, K, NA), np.int64)
    mask2 = np.zeros((E, K, NA), np.int64)
    ends = np.zeros((E, K), np.int64)
    crash9 = np.zeros((E, K), np.int64)
    scripted2 = np.full((E, K, NA, N - K), -1, np.int64)
    kinds = dict(end_eaten=0, end_cap=0, end_other=0, cap_all_nine=0)
    all_k = (1 << K) - 1
    fear, orc.world.fear = orc.world.fear, 0  # neither crashes nor dones depend on FeAR: the trials skip it
    try:
        for e in range(E):
            saved = _copy(orc.envs[e])
            scripted = joint[e, K:].copy() if N > K else None
            for k in range(K):
                for a in range(NA):
                    rl = joint[e, :K].copy()
                    rl[k] = a
                    out = orc.step_one(e, rl, scripted, auto_reset=False)[2]
                    own = (out.crash_bits >> k) & 1
                    crash9[e, k] |= own << a
                    mask2[e, k, a] = out.mask[k]
                    if out.done:
                        ends[e, k] |= 1 << a
                        rl_crash = out.crash_bits & all_k
                        capped = orc.world.max_steps > 0 and orc.envs[e].t >= orc.world.max_steps
                        kinds["end_eaten"] += int(not rl_crash and saved.apples != 0 and orc.envs[e].apples == 0)
                        kinds["end_cap"] += int(capped and not rl_crash and orc.envs[e].apples != 0)
                        kinds["end_other"] += int(not own and rl_crash != 0)
                    else:
                        after = _copy(orc.envs[e])
                        for b in range(NA):
                            rl2 = np.zeros(K, np.int32)
                            rl2[k] = b
                            out2 = orc.step_one(e, rl2, None, auto_reset=False)[2]
                            crash2[e, k, a] |= ((out2.crash_bits >> k) & 1) << b
                            scripted2[e, k, a] = list(out2.actions)[K:N]
                            orc.envs[e] = _copy(after)
                    orc.envs[e] = _copy(saved)
                capped = orc.world.max_steps > 0 and saved.t + 1 >= orc.world.max_steps
                kinds["cap_all_nine"] += int(capped and ends[e, k] == ALL)
    finally:
        orc.world.fear = fear
    return dict(crash2=crash2, ends=ends, crash9=crash9, mask2=mask2, scripted2=scripted2, **kinds)


def derived(tab, mask):
    """(trap9 [E, K], safe_mask [E, K], ahead_mask [E, K], sims) from the oracle's tables by the stated rules; mask
    None: all nine.  sims: 9 K + 9 x (the (k, a) whose step does not end), summed over the envs."""
    crash2, ends, crash9, mask2 = tab["crash2"], tab["ends"], tab["crash9"], tab["mask2"]
    E, K, _ = crash2.shape
    goes_on = ((ends[:, :, None] >> np.arange(NA)) & 1) == 0                     # [E, K, 9]
    trap = goes_on & (mask2 != 0) & ((mask2 & ~crash2) == 0)
    trap9 = (trap.astype(np.int64) << np.arange(NA)).sum(-1)
    m = np.full((E, K), ALL, np.int64) if mask is None else (mask.astype(np.int64) & ALL)
    safe = m & ~crash9
    safe = np.where(safe != 0, safe, m)
    ahead = m & ~crash9 & ~trap9
    ahead = np.where(ahead != 0, ahead, safe)
    sims = NA * K * E + NA * int(goes_on.sum())
    return trap9, safe, ahead, sims


def coverage(tab, mask):
    """What one comparison's oracle tables show, as counts (the conditions tests/test_step_lookahead_cpu.py
    asserts): trap bits; non-zero crash2 entries that are no trap; ahead_mask != safe_mask; ends bits of actions
    under which k itself does not crash; (e, k) whose second-step scripted actions differ between two first
    actions (see test_step_lookahead_cpu.py: always 0); and how steps ended."""
    trap9, safe, ahead, _ = derived(tab, mask)
    no_trap = ((trap9[:, :, None] >> np.arange(NA)) & 1) == 0
    s2 = tab["scripted2"]
    differs = 0
    if s2.shape[-1]:
        for e in range(s2.shape[0]):
            for k in range(s2.shape[1]):
                rows = {tuple(r) for r in s2[e, k].tolist() if r[0] >= 0}
                differs += int(len(rows) > 1)
    return dict(trap=int((trap9 != 0).sum()), crash2_no_trap=int(((tab["crash2"] != 0) & no_trap).sum()),
                ahead_differs=int((ahead != safe).sum()), ends_not_own=int(((tab["ends"] & ~tab["crash9"]) != 0).sum()),
                scripted2_differs=differs, end_eaten=tab["end_eaten"], end_cap=tab["end_cap"],
                end_other=tab["end_other"], cap_all_nine=tab["cap_all_nine"])


def masks_of(orc, sc):
    return np.asarray(sc.action_mask)[orc.positions()[:, :sc.K]].astype(np.uint16)


@functools.lru_cache(maxsize=None)
def reference_run(name: str):
    """The oracle's own run of a case, computed once per session and never modified: a list of comparisons, each a
    dict with "where", "rl" ([E, K] int32 or None: the step's own draws), "scripted" (None or [E, N - K]),
    "spawn" (None, or the replayed reset's [E, N] before it), "joint" [E, N], "mask" [E, K] uint16, "pos" [E, N]
    (the oracle's cells), "step" (how many of the steps ran before it), "tab" (oracle_lookahead) and "cov"
    (coverage).  The steps between the comparisons are in "rl_steps": the [E, K] actions (or None) of each of the
    STEPS steps."""
    case = CASES[CASE_IDS.index(name)]
    sc, orc = make_oracle(case)
    E, K = case.E, sc.K
    rng = np.random.default_rng(200 + case.seed)
    obs = np.zeros((K, E, sc.HW), np.float32)
    outs = (O.StepOut * E)()
    comps, rl_steps = [], []

    def compare(where, rl, scripted, spawn):
        joint = oracle_joint(orc, sc, rl)
        if scripted is not None:
            joint = np.concatenate([rl, scripted], 1).astype(np.int32)
        mask = masks_of(orc, sc)
        tab = oracle_lookahead(orc, sc, joint)
        comps.append(dict(where=where, rl=rl, scripted=scripted, spawn=spawn, joint=joint, mask=mask, tab=tab,
                          pos=orc.positions(),
                          cov=coverage(tab, mask), step=len(rl_steps)))

    for t in range(STEPS):
        rl = rng.integers(0, NA, (E, K)).astype(np.int32) if t % 2 == 0 else None
        if t in COMPARE_AT:
            compare(f"{name} step {t}", rl, None, None)
        rl_steps.append(rl)
        orc.vec_step(rl, obs=obs, outs=outs)
    for rnd in range(REPLAY_ROUNDS):
        spawn, rl, scripted = clustered_spawn(sc, E, rng)
        for e in range(E):
            orc.reset_one(e, spawn=spawn[e], episode=orc.envs[e].episode + 1)  # gw_reset starts a new episode
        compare(f"{name} replay {rnd}", rl, scripted if sc.N > K else None, spawn)
    return dict(case=case, comps=comps, rl_steps=rl_steps)


def summed_coverage(name: str) -> dict:
    total = {}
    for c in reference_run(name)["comps"]:
        for n, v in c["cov"].items():
            total[n] = total.get(n, 0) + v
    return total
