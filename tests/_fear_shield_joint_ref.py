"""A numpy restatement of the coordinated responsibility shield (include/gridenv.h gw_fear_shield_joint), written
from the rule's wording on tests/_fear_shield_ref.pick_one and the C oracle's fear_one_actor rows, one env at a
time: the reference of the CPU and GPU tests of the joint shield, and the seeded cases both use."""
import functools

import numpy as np

from _fear_shield_ref import pick_one, shield_ref
from marlnav import scenario as S
from oracle import oracle as O

NA = 9
E0 = 203


def _close(loc, W, k):
    """[N] bool: within Manhattan distance 5 of agent k, itself included (CustomMAEnv.close_agents)."""
    r, c = loc // W, loc % W
    return (np.abs(r - r[k]) + np.abs(c - c[k])) <= 5


def table_row(sc, loc, joint, k):
    """[9] f64: row k of the preview table of (loc, joint): the oracle's np.sum(Resp) for actor k over its close
    list, k playing a (the way tests/test_gpu_fear_preview._oracle_rows builds a table)."""
    region = sc.region.reshape(sc.H, sc.W)
    mdr = sc.mdr[loc].astype(np.int32)
    ids = np.flatnonzero(_close(loc.astype(np.int64), sc.W, k)).astype(np.int32)
    acts = joint[ids].astype(np.int32)
    at = int(np.flatnonzero(ids == k)[0])
    out = np.zeros(NA)
    for a in range(NA):
        acts[at] = a
        out[a] = O.fear_one_actor(sc.H, sc.W, region, loc, ids, acts, mdr, k)[0]
    return out


def joint_one(sc, loc, prop, scripted, mask, probs, tau, agents, sweeps):
    """One env.  loc [N] cells, prop [K], scripted [N - K], mask [K] or None, probs [K, 9] f32 or None.
    -> dict: actions [K], flags [K], table [K, 9], joint [N], sims (world updates the kernel's schedule runs),
    changed (per sweep run: did it change an action)."""
    K, N = sc.K, sc.N
    loc = np.asarray(loc, np.int32)
    clamp = lambda a: int(a) if 0 <= int(a) < NA else 0  # noqa: E731  (what gw_step applies for it)
    prop = np.array([clamp(a) for a in prop], np.int32)
    joint = np.concatenate([prop, [clamp(a) for a in scripted]]).astype(np.int32)
    bits = ((1 << K) - 1) if agents is None else int(agents) & ((1 << K) - 1)
    per_actor = [NA * (1 + 8 * (int(_close(loc.astype(np.int64), sc.W, k).sum()) - 1)) for k in range(K)]
    rows = {}

    def row(k):
        key = (k, joint.tobytes())
        if key not in rows:
            rows[key] = table_row(sc, loc, joint, k)
        return rows[key]

    stuck = [0] * K
    changed_log, sims = [], 0
    if bits:
        for _ in range(sweeps):
            changed = False
            for k in range(K):
                if not (bits >> k) & 1:
                    continue
                sims += per_actor[k]
                m = 0x1FF if mask is None else int(mask[k]) & 0xFFFF
                a, f = pick_one(row(k), joint[k], m, None if probs is None else probs[k], tau, True)
                stuck[k] = (f >> 1) & 1
                if a != joint[k]:
                    joint[k] = a
                    changed = True
            changed_log.append(changed)
            if not changed:
                break
    unconverged = bool(changed_log and changed_log[-1])
    # the final table: after an unchanged last sweep the shielded agents' rows are the visits'
    have = bits if (bits and not unconverged) else 0
    sims += sum(per_actor[k] for k in range(K) if not (have >> k) & 1)
    table = np.stack([row(k) for k in range(K)])
    flags = np.zeros(K, np.uint8)
    for k in range(K):
        sh = (bits >> k) & 1
        flags[k] = (int(joint[k] != prop[k]) | (stuck[k] << 1) |
                    (int(bool(sh) and np.float64(table[k, joint[k]]) > np.float64(tau)) << 2) | (int(unconverged) << 3))
    return dict(actions=joint[:K].copy(), flags=flags, table=table, joint=joint.copy(), sims=sims, changed=changed_log)


def joint_ref(sc, spawn, rl, scripted, mask=None, probs=None, tau=0.0, agents=None, sweeps=2):
    """All envs.  spawn [E, N], rl [E, K], scripted [E, N - K], mask [E, K] or None, probs [K, E, 9] or None
    -> dict of stacked outputs (sims summed, changed a list per env)."""
    E = spawn.shape[0]
    outs = [joint_one(sc, spawn[e], rl[e], scripted[e], None if mask is None else mask[e],
                      None if probs is None else probs[:, e], tau, agents, sweeps) for e in range(E)]
    r = {n: np.stack([o[n] for o in outs]) for n in ("actions", "flags", "table", "joint")}
    r["sims"] = int(sum(o["sims"] for o in outs))
    r["changed"] = [o["changed"] for o in outs]
    return r


def unilateral_ref(sc, spawn, rl, scripted, mask=None, probs=None, tau=0.0):
    """The unilateral shield of all K agents at once (gw_fear_preview + gw_fear_shield): -> actions [E, K]."""
    E = spawn.shape[0]
    joint = np.concatenate([rl, scripted], 1).astype(np.int32)
    table = np.stack([np.stack([table_row(sc, spawn[e].astype(np.int32), joint[e], k) for k in range(sc.K)])
                      for e in range(E)])
    return shield_ref(table, rl, mask, probs, tau, None)[0]


# ---- the seeded cases ------------------------------------------------------------------------------------

def scenario(name):
    """A built-in by name, or a row of tests/_shapes.py by its id."""
    import _shapes
    return _shapes.scenario(name) if name in _shapes.BY_ID else S.builtin(name)


# scenario -> (seed, tau, spawn among the `near` road cells nearest a random one): clustered spawns so that agents
# meet.  tests/test_fear_shield_joint_cpu.py holds the floors these seeds meet on the CPU reference
CASES = {"level3": (715, -0.5, 8), "grid64_n8": (729, 0.0, 24), "3x4_n7_k7": (713, 0.0, 24)}


@functools.lru_cache(maxsize=None)
def case(name, E=E0):
    """-> (scenario, spawn [E, N], rl [E, K], scripted [E, N - K], mask [E, K] u16, probs [K, E, 9] f32, tau).
    Spawns: N road cells drawn among the `near` nearest a random road cell, sorted (as the unilateral shield's test).
    Mask: the cells' action masks, except that a fifth of the entries forbid the cell's MdR, a tenth are a random
    9-bit set and a few are 0.  Probabilities from four values, so maxima tie."""
    seed, tau, n_near = CASES[name]
    sc = scenario(name)
    rng = np.random.default_rng(seed)
    free = sc.free_cells.astype(np.int64)
    fr, fc = free // sc.W, free % sc.W
    spawn = np.zeros((E, sc.N), np.int32)
    for e in range(E):
        c = int(rng.integers(0, free.size))
        near = np.argsort(np.abs(fr - fr[c]) + np.abs(fc - fc[c]), kind="stable")[:n_near]
        spawn[e] = np.sort(free[rng.choice(near, sc.N, replace=False)])
    rl = rng.integers(0, NA, (E, sc.K)).astype(np.int32)
    scripted = rng.integers(0, NA, (E, sc.N - sc.K)).astype(np.int32)
    cells = spawn[:, :sc.K]
    mask = sc.action_mask[cells].astype(np.uint16)
    u = rng.random((E, sc.K))
    no_mdr = mask & ~(1 << sc.mdr[cells].astype(np.uint16))
    mask = np.where(u < 0.2, no_mdr, mask)
    mask = np.where((u >= 0.2) & (u < 0.3), rng.integers(0, 0x200, (E, sc.K)).astype(np.uint16), mask)
    mask = np.where(u > 0.98, 0, mask).astype(np.uint16)
    probs = rng.choice(np.array([0.05, 0.1, 0.2, 0.3], np.float32), (sc.K, E, NA)).astype(np.float32)
    for a in (spawn, rl, scripted, mask, probs):
        a.setflags(write=False)
    return sc, spawn, rl, scripted, mask, probs, tau


def clustered(sc, seed, E):
    """-> (spawn [E, N], rl [E, K], scripted [E, N - K], mask [E, K] u16, probs [K, E, 9] f32): spawns drawn among
    the 24 road cells nearest a random one (sorted), uniform RL and scripted actions, a mask with zero,
    MdR-forbidding and random entries, probabilities with tied maxima."""
    rng = np.random.default_rng(seed)
    free = sc.free_cells.astype(np.int64)
    fr, fc = free // sc.W, free % sc.W
    spawn = np.zeros((E, sc.N), np.int32)
    for e in range(E):
        c = int(rng.integers(0, free.size))
        near = np.argsort(np.abs(fr - fr[c]) + np.abs(fc - fc[c]), kind="stable")[:24]
        spawn[e] = np.sort(free[rng.choice(near, sc.N, replace=False)])
    rl = rng.integers(0, NA, (E, sc.K)).astype(np.int32)
    scripted = rng.integers(0, NA, (E, sc.N - sc.K)).astype(np.int32)
    cells = spawn[:, :sc.K]
    mask = sc.action_mask[cells].astype(np.uint16)
    u = rng.random((E, sc.K))
    mask = np.where(u < 0.25, mask & ~(1 << sc.mdr[cells].astype(np.uint16)), mask)
    mask = np.where((u >= 0.25) & (u < 0.4), rng.integers(0, 0x200, (E, sc.K)).astype(np.uint16), mask)
    mask = np.where(u > 0.95, 0, mask).astype(np.uint16)
    probs = rng.choice(np.array([0.05, 0.1, 0.2, 0.3], np.float32), (sc.K, E, NA)).astype(np.float32)
    return spawn, rl, scripted, mask, probs


# The case sets of the GPU tests that compare against the composition on the GPU (no CPU reference there):
# "<scenario>" the sets of test_equals_the_composition at E0 envs, "<scenario>@E" those of the dead-wave test.
# tests/test_fear_shield_joint_cpu.py holds the floors they meet on the CPU reference (FLOOR_SETTING below).
COMPOSITION_SCENARIOS = ["level3", "grid64_n8", "7x9_n3_k3", "2x2_n4_k2", "3x4_n7_k7", "4x6_n6_k6", "5x5_n6_k4",
                         "64x64_n8_k8"]
DEAD_WAVE_SCENARIO = "3x4_n7_k7"
COMPOSITION_SEEDS = {"level3": 900, "grid64_n8": 901, "7x9_n3_k3": 1001, "2x2_n4_k2": 903, "3x4_n7_k7": 904,
                     "4x6_n6_k6": 905, "5x5_n6_k4": 906, "64x64_n8_k8": 907}
DEAD_WAVE_SEEDS = {1: 951, 3: 957, 5: 950, 257: 950}
FLOOR_SETTING = dict(tau=0.0, agents=None)  # with the set's own mask and probabilities: one of the tests' combinations


@functools.lru_cache(maxsize=None)
def clustered_set(key):
    """-> (scenario, spawn, rl, scripted, mask, probs) of a key of the table above (never modified)."""
    name, _, e = key.partition("@")
    sc = scenario(name)
    if e:
        arrs = clustered(sc, DEAD_WAVE_SEEDS[int(e)], int(e))
    else:
        arrs = clustered(sc, COMPOSITION_SEEDS[name], E0)
    for a in arrs:
        a.setflags(write=False)
    return (sc,) + arrs


@functools.lru_cache(maxsize=None)
def case_ref(name, sweeps, E=E0):
    """joint_ref of a seeded case (computed once per session and shared; never modified)."""
    sc, spawn, rl, scripted, mask, probs, tau = case(name, E)
    return joint_ref(sc, spawn, rl, scripted, mask, probs, tau, None, sweeps)
