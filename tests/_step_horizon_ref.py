"""The crash horizon's reference (gw_step_horizon): the C oracle stepped on copies of its state.

Two forms, which must agree wherever both are run (tests/test_step_horizon_cpu.py):
  plain     per (env, RL agent k, first action a) a depth-first search with no memoisation: step 1 under the
            proposed joint action with k playing a, then ``apples = 0`` on the copy, then steps with every other RL
            agent playing 0, the oracle's own scripted draws, and k's actions limited to the mask the step before
            returned for it.  A branch stops as soon as depth H is reached;
  memoised  per (env, k) level by level: level h is the set of distinct cells k can stand in after h survived
            steps, each with the oracle state of the first path that reached it.  One oracle step per (level,
            cell, allowed action), then a backward pass.  This is what the kernel does, and its count of oracle
            steps is the sim count of include/gridenv.h.
They agree because, as long as k has not crashed, the world differs between k's choices in k's own cell only;
``path_backgrounds`` records the other agents' cells and the scripted actions on every surviving path so that the
test can assert that directly.  The viable set and the mask rule are restated in numpy (``derived``).
The cases are _step_preview_ref.CASES' shapes and one open map whose H * W is no multiple of 4 (tests/_shapes.py's
13 x 3 row), with the step cap chosen here."""
import dataclasses
import functools

import numpy as np

import _step_lookahead_ref as L
import _step_preview_ref as P
from oracle import oracle as O

NA, ALL = 9, 0x1FF
HORIZONS = (2, 3, 4)
CRASH, END = -1, -2  # transition codes beside a cell

# max_steps = 7: the cap is reached inside the run, and inside the horizon at the steps before it
CASES = [dataclasses.replace(c, max_steps=7) for c in P.CASES] + [P.Case("open13x3_k1", "open:13,3,3,1", 23, max_steps=7)]
CASE_IDS = [c.name for c in CASES]
STEPS = 7
COMPARE_AT = (1, 3, 4, 5, 6)  # the steps compared (device-random RL actions at the odd ones); 4-6: the cap within 3, 2, 1
REPLAY_ROUNDS = 2
scenario_of, make_oracle, oracle_joint = P.scenario_of, P.make_oracle, P.oracle_joint
clustered_spawn = P.clustered_spawn


def _copy(env):
    return type(env).from_buffer_copy(env)


def _first_step(orc, sc, joint, e, k, a):
    """The oracle env e stepped once under joint[e] with k playing a (auto_reset off) -> its StepOut; the env is
    left in the state after the step."""
    K, N = sc.K, sc.N
    rl = joint[e, :K].copy()
    rl[k] = a
    return orc.step_one(e, rl, joint[e, K:].copy() if N > K else None, auto_reset=False)[2]


def _later_step(orc, e, k, K, b):
    rl = np.zeros(K, np.int32)
    rl[k] = b
    return orc.step_one(e, rl, None, auto_reset=False)[2]


def _plain_from(orc, e, k, K, mask, h, H):
    """k has survived h steps and the episode goes on -> the largest depth reachable from the oracle's present
    state (H: the horizon or an episode end is reached, or k stands in a cell that allows nothing)."""
    if h == H or mask == 0:
        return H
    saved, best = _copy(orc.envs[e]), h
    for b in range(NA):
        if not (mask >> b) & 1:
            continue
        out = _later_step(orc, e, k, K, b)
        if (out.crash_bits >> k) & 1:
            d = h
        elif out.done:
            d = H
        else:
            d = _plain_from(orc, e, k, K, int(out.mask[k]), h + 1, H)
        orc.envs[e] = _copy(saved)
        best = max(best, d)
        if best == H:
            break
    return best


def oracle_horizon_plain(orc, sc, joint, H):
    """depth [E, K, 9] int64 by the plain search.  The oracle's state is left as it was."""
    E, K = orc.E, sc.K
    depth = np.zeros((E, K, NA), np.int64)
    fear, orc.world.fear = orc.world.fear, 0  # neither crashes nor dones depend on FeAR: the trials skip it
    try:
        for e in range(E):
            saved = _copy(orc.envs[e])
            for k in range(K):
                for a in range(NA):
                    out = _first_step(orc, sc, joint, e, k, a)
                    if (out.crash_bits >> k) & 1:
                        d = 0
                    elif out.done:
                        d = H
                    else:
                        orc.envs[e].apples = 0
                        d = _plain_from(orc, e, k, K, int(out.mask[k]), 1, H)
                    depth[e, k, a] = d
                    orc.envs[e] = _copy(saved)
    finally:
        orc.world.fear = fear
    return depth


def oracle_horizon(orc, sc, joint, H):
    """The memoised form.  -> dict: depth [E, K, 9], ends / crash9 [E, K] (int64), sims (9 K E + the oracle steps
    of the levels >= 1), paths[e][k][a] (the actions after a of one continuation that reaches depth[e, k, a]:
    it stops at an episode end, at the horizon, or where every allowed action crashes k), and counts of what the
    levels >= 1 met: "cap_inside" ((e, k) whose forward pass the step cap ended before level H - 1),
    "other_crash_later" (updates of a step >= 2 that k survives while another RL agent's crash ends the episode),
    "empty_mask" (nodes whose cell allows nothing).  The oracle's state is left as it was."""
    E, K, N = orc.E, sc.K, sc.N
    amask = np.asarray(sc.action_mask).astype(np.int64)
    depth = np.zeros((E, K, NA), np.int64)
    ends = np.zeros((E, K), np.int64)
    crash9 = np.zeros((E, K), np.int64)
    paths = [[[None] * NA for _ in range(K)] for _ in range(E)]
    counts = dict(cap_inside=0, other_crash_later=0, empty_mask=0)
    sims = NA * K * E
    cap = orc.world.max_steps
    fear, orc.world.fear = orc.world.fear, 0
    try:
        for e in range(E):
            saved = _copy(orc.envs[e])
            for k in range(K):
                first, level = [None] * NA, {}
                for a in range(NA):
                    out = _first_step(orc, sc, joint, e, k, a)
                    own = (out.crash_bits >> k) & 1
                    crash9[e, k] |= own << a
                    ends[e, k] |= int(out.done) << a
                    if own:
                        first[a] = CRASH
                    elif out.done:
                        first[a] = END
                    else:
                        first[a] = int(orc.envs[e].pos[k])
                        orc.envs[e].apples = 0
                        level.setdefault(first[a], _copy(orc.envs[e]))
                    orc.envs[e] = _copy(saved)
                trans, h = [], 1
                while h < H and level:
                    nxt, tr = {}, {}
                    for cell in sorted(level):
                        tr[cell] = {}
                        counts["empty_mask"] += int(amask[cell] & ALL == 0)
                        for b in range(NA):
                            if not (amask[cell] >> b) & 1:
                                continue
                            orc.envs[e] = _copy(level[cell])
                            out = _later_step(orc, e, k, K, b)
                            sims += 1
                            if (out.crash_bits >> k) & 1:
                                code = CRASH
                            elif out.done:
                                code = END
                                counts["other_crash_later"] += int((out.crash_bits & ((1 << K) - 1)) != 0)
                            else:
                                code = int(orc.envs[e].pos[k])
                                if h + 1 < H:
                                    nxt.setdefault(code, _copy(orc.envs[e]))
                            tr[cell][b] = code
                    trans.append(tr)
                    level, h = nxt, h + 1
                orc.envs[e] = _copy(saved)
                counts["cap_inside"] += int(cap > 0 and 1 < cap - saved.t < H and len(trans) == cap - saved.t - 1
                                            and any(END in row.values() for row in trans[-1].values()))
                dep, best = {}, {}
                for h in range(len(trans), 0, -1):
                    for cell, row in trans[h - 1].items():
                        d_best, b_best = (H, None) if not row else (-1, None)
                        for b, code in row.items():
                            d = h if code == CRASH else H if (code == END or h + 1 >= H) else dep[(h + 1, code)]
                            if d > d_best:
                                d_best, b_best = d, b
                        dep[(h, cell)], best[(h, cell)] = d_best, b_best
                for a in range(NA):
                    code = first[a]
                    depth[e, k, a] = 0 if code == CRASH else H if (code == END or H == 1) else dep[(1, code)]
                    path, h = [], 1
                    while code >= 0 and h < H and depth[e, k, a] > h:
                        b = best[(h, code)]
                        if b is None:  # a cell that allows nothing
                            break
                        path.append(b)
                        code, h = trans[h - 1][code][b], h + 1
                    paths[e][k][a] = path
    finally:
        orc.world.fear = fear
    return dict(depth=depth, ends=ends, crash9=crash9, sims=sims, paths=paths, **counts)


def path_backgrounds(orc, sc, joint, e, k, H):
    """Every path of (e, k) on which k survives, searched in full (no early stop): -> {level h: the set of
    (the other agents' cells, the scripted agents' actions of step h) over the paths that survived h steps with
    the episode going on}.  The invariance claim is that every set has one element."""
    K, N = sc.K, sc.N
    seen = {}
    saved = _copy(orc.envs[e])
    fear, orc.world.fear = orc.world.fear, 0

    def note(h, out):
        cells = tuple(int(orc.envs[e].pos[n]) for n in range(N) if n != k)
        seen.setdefault(h, set()).add((cells, tuple(list(out.actions)[K:N])))

    def walk(mask, h):
        if h == H:
            return
        here = _copy(orc.envs[e])
        for b in range(NA):
            if (mask >> b) & 1:
                out = _later_step(orc, e, k, K, b)
                if not (out.crash_bits >> k) & 1 and not out.done:
                    note(h + 1, out)
                    walk(int(out.mask[k]), h + 1)
                orc.envs[e] = _copy(here)

    try:
        for a in range(NA):
            out = _first_step(orc, sc, joint, e, k, a)
            if not (out.crash_bits >> k) & 1 and not out.done:
                note(1, out)
                orc.envs[e].apples = 0
                walk(int(out.mask[k]), 1)
            orc.envs[e] = _copy(saved)
    finally:
        orc.world.fear = fear
    return seen


def derived(depth, mask, H):
    """(viable9 [E, K], horizon_mask [E, K]) int64 from the depth table by the stated rules; mask None: all nine."""
    E, K, _ = depth.shape
    bit = 1 << np.arange(NA)
    viable9 = ((depth == H) * bit).sum(-1)
    m = np.full((E, K), ALL, np.int64) if mask is None else (mask.astype(np.int64) & ALL)
    in_m = ((m[:, :, None] >> np.arange(NA)) & 1) == 1
    top = np.where(in_m, depth, -1).max(-1, keepdims=True)
    return viable9, ((in_m & (depth == top)) * bit).sum(-1)


def _walk(name: str, visit):
    """The oracle's own run of a case: ``visit(orc, sc, comp)`` at every comparison, comp holding "where", "rl"
    ([E, K] int32 or None: the step's own draws), "scripted" (None or [E, N - K]), "spawn" (None, or the replayed
    reset's [E, N] before it), "joint" [E, N], "mask" [E, K] uint16, "pos" [E, N] and "step" (how many of the steps
    ran before it).  -> (case, the comps, the [E, K] actions (or None) of each of the STEPS steps)."""
    case = CASES[CASE_IDS.index(name)]
    sc, orc = make_oracle(case)
    E, K = case.E, sc.K
    rng = np.random.default_rng(300 + case.seed)
    obs = np.zeros((K, E, sc.HW), np.float32)
    outs = (O.StepOut * E)()
    comps, rl_steps = [], []

    def compare(where, rl, scripted, spawn):
        joint = oracle_joint(orc, sc, rl)
        if scripted is not None:
            joint = np.concatenate([rl, scripted], 1).astype(np.int32)
        comps.append(dict(where=where, rl=rl, scripted=scripted, spawn=spawn, joint=joint, mask=L.masks_of(orc, sc),
                          pos=orc.positions(), step=len(rl_steps)))
        visit(orc, sc, comps[-1])

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
    return case, comps, rl_steps


@functools.lru_cache(maxsize=None)
def reference_run(name: str):
    """The memoised reference of a case, computed once per session and never modified: _walk's comparisons, each
    with "tab" ({H: oracle_horizon's dict} for H in HORIZONS) and "la" (_step_lookahead_ref.oracle_lookahead's
    tables of the same state), and "rl_steps"."""
    def visit(orc, sc, c):
        c["tab"] = {H: oracle_horizon(orc, sc, c["joint"], H) for H in HORIZONS}
        c["la"] = L.oracle_lookahead(orc, sc, c["joint"])

    case, comps, rl_steps = _walk(name, visit)
    return dict(case=case, comps=comps, rl_steps=rl_steps)


@functools.lru_cache(maxsize=None)
def plain_run(name: str):
    """The plain search over the same run (CPU tests only): per comparison "plain" ({H: depth [E, K, 9]}) and, at
    the replayed resets, "backgrounds" ({(e, k): path_backgrounds at H = HORIZONS[-1]} for every (e, k))."""
    def visit(orc, sc, c):
        c["plain"] = {H: oracle_horizon_plain(orc, sc, c["joint"], H) for H in HORIZONS}
        if c["spawn"] is not None:
            c["backgrounds"] = {(e, k): path_backgrounds(orc, sc, c["joint"], e, k, HORIZONS[-1])
                                for e in range(orc.E) for k in range(sc.K)}

    return _walk(name, visit)[1]


def depth_histogram(name: str, H: int) -> list:
    """How many (e, k, a) entries of the case's comparisons have each depth 0..H."""
    hist = np.zeros(H + 1, np.int64)
    for c in reference_run(name)["comps"]:
        hist += np.bincount(c["tab"][H]["depth"].ravel(), minlength=H + 1)
    return hist.tolist()
