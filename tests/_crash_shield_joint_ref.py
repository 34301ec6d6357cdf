"""A numpy restatement of the coordinated crash-aware shield (include/gridenv.h gw_crash_shield_joint), written from
the rule's wording, one env at a time: tests/_fear_shield_ref.pick_one for the pick, tests/_fear_shield_joint_ref
.table_row for the FeAR rows, and for the crash bits the C oracle stepped on a copy of the env's state (the way
tests/_step_preview_ref.oracle_tables does).  The reference of the CPU and GPU tests of gw_crash_shield_joint, with
the sim count from the header's wording and the seeded clustered cases both use."""
import functools

import numpy as np

import _fear_shield_joint_ref as R
from _fear_shield_ref import pick_one
from oracle import oracle as O

NA = 9
ALL = 0x1FF
E0 = R.E0


class CrashOracle:
    """The C oracle's envs reset on given spawns (FeAR off: only the world update is asked for);
    ``outcome(e, joint)``: crash bits | restricted bits << 8 of one step of env e under the joint action, on a copy
    of its state."""

    def __init__(self, sc, spawn):
        self.sc = sc
        self.orc = O.OracleEnvs(sc, spawn.shape[0], fear=False, max_steps=1000, seed=1, reset=False)
        for e in range(spawn.shape[0]):
            self.orc.reset_one(e, spawn[e])
        self._memo = {}

    def outcome(self, e, joint):
        key = (e, np.asarray(joint, np.int32).tobytes())
        if key not in self._memo:
            K, N = self.sc.K, self.sc.N
            env = self.orc.envs[e]
            saved = type(env).from_buffer_copy(env)
            out = self.orc.step_one(e, np.array(joint[:K], np.int32), np.array(joint[K:], np.int32) if N > K else None,
                                    auto_reset=False)[2]
            self.orc.envs[e] = saved
            self._memo[key] = (out.crash_bits & 0xFF) | ((out.restricted_bits & 0xFF) << 8)
        return self._memo[key]

    def crash9(self, e, joint, k):
        """bit a: agent k itself crashes under `joint` with k playing a"""
        c9 = 0
        j = np.array(joint, np.int32)
        for a in range(NA):
            j[k] = a
            c9 |= ((self.outcome(e, j) >> k) & 1) << a
        return c9


def safe_mask(has_mask, m, crash9):
    """csrc/step_preview.h as include/gridenv.h states it: m & ~crash9 (no mask: all nine); empty -> m unchanged."""
    m = (int(m) & ALL) if has_mask else ALL
    safe = m & ~crash9
    return safe if safe else m


def visit_one(t, cur, has_mask, m, crash9, pr, tau):
    """One visit (tau None: no FeAR, nine zeros under tau = 0) -> (action, pick flags, unavoidable)."""
    use_fear = tau is not None
    safe = safe_mask(has_mask, m, crash9)
    a, f = pick_one(t if use_fear else np.zeros(NA), cur, safe, pr, tau if use_fear else 0.0, True)
    mm = (int(m) & ALL) if has_mask else ALL
    return a, f, int(mm != 0 and (mm & ~crash9) == 0)


def crash_one(orc, e, loc, prop, scripted, mask, probs, tau, agents, sweeps, want_table=False):
    """One env.  loc [N] cells, prop [K], scripted [N - K], mask [K] or None, probs [K, 9] f32 or None, tau a float
    or None (use_fear = 0).  -> dict: actions, flags, table (None when no table is computed), joint, outcome,
    outcome_prop, crash9, sims / fear_sims (world updates the kernel's schedule runs, all / the FeAR ones), changed
    (per sweep run), why (per visit that replaced: "crash" the current action was not in the safe mask, "fear" it
    was)."""
    sc = orc.sc
    K, N = sc.K, sc.N
    use_fear = tau is not None
    loc = np.asarray(loc, np.int32)
    clamp = lambda a: int(a) if 0 <= int(a) < NA else 0  # noqa: E731  (what gw_step applies for it)
    prop = np.array([clamp(a) for a in prop], np.int32)
    joint = np.concatenate([prop, [clamp(a) for a in scripted]]).astype(np.int32)
    bits = ((1 << K) - 1) if agents is None else int(agents) & ((1 << K) - 1)
    per_actor = [NA * (1 + 8 * (int(R._close(loc.astype(np.int64), sc.W, k).sum()) - 1)) for k in range(K)]
    rows = {}

    def row(k):
        key = (k, joint.tobytes())
        if key not in rows:
            rows[key] = R.table_row(sc, loc, joint, k)
        return rows[key]

    o_prop = orc.outcome(e, joint)
    stuck, unav = [0] * K, [0] * K
    changed_log, why, sims, fear_sims = [], [], 0, 0
    if bits:
        for _ in range(sweeps):
            changed = False
            for k in range(K):
                if not (bits >> k) & 1:
                    continue
                sims += NA                       # a visit: 9 real updates ...
                if use_fear:
                    fear_sims += per_actor[k]    # ... and with use_fear the joint shield's visit
                c9 = orc.crash9(e, joint, k)
                m = 0 if mask is None else int(mask[k]) & 0xFFFF
                a, f, u = visit_one(row(k) if use_fear else None, int(joint[k]), mask is not None, m, c9,
                                    None if probs is None else probs[k], tau)
                stuck[k], unav[k] = (f >> 1) & 1, u
                if a != joint[k]:
                    why.append("crash" if not (safe_mask(mask is not None, m, c9) >> int(joint[k])) & 1 else "fear")
                    joint[k] = a
                    changed = True
            changed_log.append(changed)
            if not changed:
                break
    unconverged = bool(changed_log and changed_log[-1])
    sims += NA * K                               # the final outcome and crash9: 9 K real updates, always
    o_fin = orc.outcome(e, joint)
    crash9 = np.array([orc.crash9(e, joint, k) for k in range(K)], np.uint16)
    table = None
    if use_fear or want_table:                   # the final table, with the joint shield's economy
        have = bits if (use_fear and changed_log and not unconverged) else 0
        fear_sims += sum(per_actor[k] for k in range(K) if not (have >> k) & 1)
        table = np.stack([row(k) for k in range(K)])
    flags = np.zeros(K, np.uint8)
    for k in range(K):
        sh = (bits >> k) & 1
        over = bool(use_fear and sh and np.float64(table[k, joint[k]]) > np.float64(tau))
        flags[k] = (int(joint[k] != prop[k]) | (stuck[k] << 1) | (int(over) << 2) | (int(unconverged) << 3) |
                    (((o_fin >> k) & 1) << 4) | (unav[k] << 5))
    return dict(actions=joint[:K].copy(), flags=flags, table=table, joint=joint.copy(), outcome=np.uint16(o_fin),
                outcome_prop=np.uint16(o_prop), crash9=crash9, sims=sims + fear_sims, fear_sims=fear_sims,
                changed=changed_log, why=why)


def crash_ref(sc, spawn, rl, scripted, mask=None, probs=None, tau=None, agents=None, sweeps=2, want_table=False,
              orc=None):
    """All envs -> dict of stacked outputs (sims / fear_sims summed, changed / why a list per env)."""
    orc = orc or CrashOracle(sc, spawn)
    E = spawn.shape[0]
    outs = [crash_one(orc, e, spawn[e], rl[e], scripted[e], None if mask is None else mask[e],
                      None if probs is None else probs[:, e], tau, agents, sweeps, want_table) for e in range(E)]
    r = {n: np.stack([o[n] for o in outs]) for n in ("actions", "flags", "joint", "outcome", "outcome_prop", "crash9")}
    r["table"] = None if outs[0]["table"] is None else np.stack([o["table"] for o in outs])
    r["sims"] = int(sum(o["sims"] for o in outs))
    r["fear_sims"] = int(sum(o["fear_sims"] for o in outs))
    r["changed"] = [o["changed"] for o in outs]
    r["why"] = [o["why"] for o in outs]
    return r


def unilateral_ref(sc, spawn, rl, scripted, mask=None, probs=None, tau=None, orc=None):
    """The unilateral crash-aware shield of all K agents at once (gw_fear_preview, gw_step_preview's safe_mask,
    gw_fear_shield; tau None: a zero table under tau = 0) -> (actions [E, K], outcome [E] of the step applying them)."""
    orc = orc or CrashOracle(sc, spawn)
    E, K = spawn.shape[0], sc.K
    out = np.zeros((E, K), np.int32)
    oc = np.zeros(E, np.uint16)
    for e in range(E):
        joint = np.concatenate([rl[e], scripted[e]]).astype(np.int32)
        for k in range(K):
            t = R.table_row(sc, spawn[e].astype(np.int32), joint, k) if tau is not None else None
            out[e, k] = visit_one(t, int(joint[k]), mask is not None, 0 if mask is None else int(mask[e, k]),
                                  orc.crash9(e, joint, k), None if probs is None else probs[k, e], tau)[0]
        oc[e] = orc.outcome(e, np.concatenate([out[e], scripted[e]]))
    return out, oc


# ---- the seeded cases ------------------------------------------------------------------------------------

# name -> (scenario, seed of _fear_shield_joint_ref.clustered, tau; None: the crash shield alone).  The spawns are
# clustered so that agents meet.  tests/test_crash_shield_joint_cpu.py holds the floors these seeds meet on the
# reference alone
CASES = {"level3_crash": ("level3", 3101, None), "level3_fear": ("level3", 3125, 0.0),
         "3x4_n7_k7_crash": ("3x4_n7_k7", 3121, None), "3x4_n7_k7_fear": ("3x4_n7_k7", 3131, 0.0)}
FLOOR_SWEEPS = 4  # the "higher count" of the convergence floor, and the coordinated side of the both-moved floor


@functools.lru_cache(maxsize=None)
def case(name, E=E0):
    """-> (scenario, spawn [E, N], rl [E, K], scripted [E, N - K], mask [E, K] u16, probs [K, E, 9] f32, tau), never
    modified."""
    scen, seed, tau = CASES[name]
    sc = R.scenario(scen)
    arrs = R.clustered(sc, seed, E)
    for a in arrs:
        a.setflags(write=False)
    return (sc,) + arrs + (tau,)


@functools.lru_cache(maxsize=None)
def case_oracle(name, E=E0):
    sc, spawn = case(name, E)[:2]
    return CrashOracle(sc, spawn)


@functools.lru_cache(maxsize=None)
def case_ref(name, sweeps, E=E0):
    """crash_ref of a seeded case (computed once per session and shared; never modified)."""
    sc, spawn, rl, scripted, mask, probs, tau = case(name, E)
    return crash_ref(sc, spawn, rl, scripted, mask, probs, tau, None, sweeps, orc=case_oracle(name, E))


@functools.lru_cache(maxsize=None)
def case_unilateral(name, E=E0):
    sc, spawn, rl, scripted, mask, probs, tau = case(name, E)
    return unilateral_ref(sc, spawn, rl, scripted, mask, probs, tau, orc=case_oracle(name, E))


def floors(name):
    """What the reference alone shows on a seeded case, as counts of envs (visits for the last two):
    both_moved: the unilateral crash shield leaves two moved RL agents crashing and the coordinated one (FLOOR_SWEEPS
      sweeps) leaves no RL agent of the env crashing;
    unavoidable: an entry with flag bit 5 (two sweeps);
    late: unconverged at one sweep and converged at FLOOR_SWEEPS;
    for_crash / for_fear: visits (two sweeps) that replaced an action outside / inside the safe mask."""
    sc, spawn, rl = case(name)[:3]
    K = sc.K
    uni, uni_oc = case_unilateral(name)
    r1, r2, r4 = case_ref(name, 1), case_ref(name, 2), case_ref(name, FLOOR_SWEEPS)
    kbits = (uni_oc.astype(np.int64)[:, None] >> np.arange(K)[None, :]) & 1
    two_moved = ((kbits == 1) & (uni != rl)).sum(1) >= 2
    co_clean = (r4["flags"] & 16).sum(1) == 0
    why = [w for ws in r2["why"] for w in ws]
    return dict(both_moved=int((two_moved & co_clean).sum()), unavoidable=int(((r2["flags"] & 32) != 0).any(1).sum()),
                late=int((((r1["flags"][:, 0] & 8) != 0) & ((r4["flags"][:, 0] & 8) == 0)).sum()),
                for_crash=why.count("crash"), for_fear=why.count("fear"))
