"""The reward horizon's reference (gw_step_plan): the C oracle stepped on copies of its state, its apples left
as they are, ``StepOut.reward[k]`` times 10 rounded to an int as the step's reward.

Two forms, which must agree wherever both are run (tests/test_step_plan_cpu.py):
  plain     per (env, RL agent k, first action a) a depth-first search with no memoisation and no early stop:
            step 1 under the proposed joint action with k playing a, then steps with every other RL agent playing
            0, the oracle's own scripted draws, and k's actions limited to the mask the step before returned for
            it.  The lexicographic maximum of (depth, return), the lowest action on ties;
  memoised  per (env, k) level by level: level h is the set of distinct (cell, is k's apple still there) states
            k can be in after h survived steps, each with the oracle state of the first path that reached it.
            One oracle step per state and allowed action, then a backward pass.  The sim count is one per (level,
            distinct CELL, allowed action), as include/gridenv.h counts; the paths come from this form.
The cases are _step_horizon_ref.CASES (the shapes, the step cap inside the horizon) walked through the same
steps and the clustered replayed reset, then a "near apple" replayed reset (every RL agent within Manhattan
distance 3 of its own apple) and, where K >= 2, a reset whose first step lets every RL agent but the last eat, so
that the last agent's apple is the env's last one at the comparison after it."""
import ctypes as C
import functools

import numpy as np

import _step_horizon_ref as R
import _step_lookahead_ref as L
from oracle import oracle as O

NA, ALL = 9, 0x1FF
HORIZONS = R.HORIZONS
HORIZON_MAX = 4
CRASH, END = -1, -2  # transition codes beside a cell
NO_ACTION = 0xFF
CRASH_TENTHS = -100
CASES, CASE_IDS = R.CASES, R.CASE_IDS
STEPS = R.STEPS
COMPARE_AT = (1, 4, 5, 6)  # the steps compared (device-random RL actions at the odd ones); 4-6: the cap within 3, 2, 1
scenario_of, make_oracle, oracle_joint = R.scenario_of, R.make_oracle, R.oracle_joint
_copy = R._copy


def tenths(x) -> int:
    return int(round(10.0 * float(x)))


class _Stepper:
    """orc.step_one without its per-call allocations (the plain search steps the oracle millions of times)."""

    def __init__(self, orc, sc):
        self.orc, self.K, self.N = orc, sc.K, sc.N
        self.obs = np.zeros((sc.K, sc.HW), np.float32)
        self.final = np.zeros((sc.K, sc.HW), np.float32)
        self.rl = np.zeros(sc.K, np.int32)
        self.sa = np.zeros(max(sc.N - sc.K, 1), np.int32)
        self.out = O.StepOut()
        self.fn = O.lib().orc_env_step
        self.p = [a.ctypes.data_as(C.c_void_p) for a in (self.obs, self.final, self.rl, self.sa)]

    def first(self, joint, e, k, a):
        """env e stepped once under joint[e] with k playing a (auto_reset off) -> the StepOut (reused)."""
        self.rl[:] = joint[e, :self.K]
        self.rl[k] = a
        if self.N > self.K:
            self.sa[:self.N - self.K] = joint[e, self.K:]
        return self._run(e, self.p[3] if self.N > self.K else None)

    def later(self, e, k, b):
        self.rl[:] = 0
        self.rl[k] = b
        return self._run(e, None)

    def _run(self, e, sa):
        orc = self.orc
        self.fn(C.byref(orc.world), orc.env_offset + e, C.byref(orc.envs[e]), self.p[2], sa, None, 0, self.p[0],
                self.p[1], C.byref(self.out))
        return self.out


def _better(a, b):
    return a[0] > b[0] or (a[0] == b[0] and a[1] > b[1])


def _plain_from(st, e, k, mask, h, H):
    """k has survived h steps and the episode goes on -> (depth, return from here on, actions) of the best
    continuation from the oracle's present state."""
    if h == H or mask == 0:
        return H, 0, []
    orc = st.orc
    saved, best = _copy(orc.envs[e]), None
    for b in range(NA):
        if not (mask >> b) & 1:
            continue
        out = st.later(e, k, b)
        rw = tenths(out.reward[k])
        if (out.crash_bits >> k) & 1:
            v = (h, rw, [b])
        elif out.done:
            v = (H, rw, [b])
        else:
            d, r, p = _plain_from(st, e, k, int(out.mask[k]), h + 1, H)
            v = (d, rw + r, [b] + p)
        orc.envs[e] = _copy(saved)
        if best is None or _better(v, best):
            best = v
    return best


def oracle_plan_plain(orc, sc, joint, H):
    """(depth [E, K, 9], ret [E, K, 9] int64, paths[e][k][a]) by the plain search.  The oracle's state is left as it
    was."""
    E, K = orc.E, sc.K
    depth = np.zeros((E, K, NA), np.int64)
    ret = np.zeros((E, K, NA), np.int64)
    paths = [[[None] * NA for _ in range(K)] for _ in range(E)]
    st = _Stepper(orc, sc)
    fear, orc.world.fear = orc.world.fear, 0  # neither crashes, dones nor env rewards depend on FeAR
    try:
        for e in range(E):
            saved = _copy(orc.envs[e])
            for k in range(K):
                for a in range(NA):
                    out = st.first(joint, e, k, a)
                    rw = tenths(out.reward[k])
                    if (out.crash_bits >> k) & 1:
                        v = (0, rw, [])
                    elif out.done:
                        v = (H, rw, [])
                    else:
                        d, r, p = _plain_from(st, e, k, int(out.mask[k]), 1, H)
                        v = (d, rw + r, p)
                    depth[e, k, a], ret[e, k, a], paths[e][k][a] = v
                    orc.envs[e] = _copy(saved)
    finally:
        orc.world.fear = fear
    return depth, ret, paths


def oracle_plan(orc, sc, joint, H):
    """The memoised form.  -> dict: depth / ret [E, K, 9], path [E, K, 9, 3] (0xFF past the end), ends / crash9
    [E, K] (int64), sims, and counts over the (e, k, a) entries' best continuations: "eat_later" (k eats its apple at
    a step >= 2), "last_later" (... and that ends the episode: the env's last apple), "crash_in_ret" (depth < H: the
    return includes the crash's -100).  The oracle's state is left as it was."""
    E, K = orc.E, sc.K
    amask = np.asarray(sc.action_mask).astype(np.int64)
    depth = np.zeros((E, K, NA), np.int64)
    ret = np.zeros((E, K, NA), np.int64)
    path = np.full((E, K, NA, HORIZON_MAX - 1), NO_ACTION, np.int64)
    ends = np.zeros((E, K), np.int64)
    crash9 = np.zeros((E, K), np.int64)
    counts = dict(eat_later=0, last_later=0, crash_in_ret=0)
    sims = NA * K * E
    st = _Stepper(orc, sc)
    fear, orc.world.fear = orc.world.fear, 0
    try:
        for e in range(E):
            saved = _copy(orc.envs[e])
            for k in range(K):
                first, level = [None] * NA, {}
                for a in range(NA):
                    out = st.first(joint, e, k, a)
                    own, rw = (out.crash_bits >> k) & 1, tenths(out.reward[k])
                    crash9[e, k] |= own << a
                    ends[e, k] |= int(out.done) << a
                    if own:
                        first[a] = (CRASH, False, rw)
                    elif out.done:
                        first[a] = (END, False, rw)
                    else:
                        cell, there = int(orc.envs[e].pos[k]), bool((orc.envs[e].apples >> k) & 1)
                        first[a] = (cell, there, rw)
                        level.setdefault(cell, {}).setdefault(there, _copy(orc.envs[e]))
                    orc.envs[e] = _copy(saved)
                trans, h = [], 1
                while h < H and level:
                    nxt, tr = {}, {}
                    for cell in sorted(level):
                        for there in level[cell]:
                            tr[(cell, there)] = {}
                        for b in range(NA):
                            if not (amask[cell] >> b) & 1:
                                continue
                            sims += 1  # the kernel's one update serves both of the cell's states
                            for there, state in level[cell].items():
                                orc.envs[e] = _copy(state)
                                out = st.later(e, k, b)
                                after = bool((orc.envs[e].apples >> k) & 1)
                                eat = there and not after
                                last = eat and orc.envs[e].apples == 0
                                if (out.crash_bits >> k) & 1:
                                    code = CRASH
                                elif out.done:
                                    code = END
                                else:
                                    code = int(orc.envs[e].pos[k])
                                    if h + 1 < H:
                                        nxt.setdefault(code, {}).setdefault(after, _copy(orc.envs[e]))
                                tr[(cell, there)][b] = (code, after, tenths(out.reward[k]), eat, last)
                    trans.append(tr)
                    level, h = nxt, h + 1
                orc.envs[e] = _copy(saved)
                val = {}  # (h, cell, there) -> (depth, return, best action or None)
                for h in range(len(trans), 0, -1):
                    for (cell, there), row in trans[h - 1].items():
                        best = (H, 0, None) if not row else None
                        for b, (code, after, rw, _, _) in row.items():
                            if code == CRASH:
                                v = (h, rw, b)
                            elif code == END or h + 1 >= H:
                                v = (H, rw, b)
                            else:
                                d, r, _ = val[(h + 1, code, after)]
                                v = (d, rw + r, b)
                            if best is None or _better(v, best):
                                best = v
                        val[(h, cell, there)] = best
                for a in range(NA):
                    code, there, rw = first[a]
                    if code == CRASH:
                        depth[e, k, a], ret[e, k, a] = 0, rw
                        counts["crash_in_ret"] += 1
                        continue
                    if code == END:
                        depth[e, k, a], ret[e, k, a] = H, rw
                        continue
                    d, r, _ = val[(1, code, there)]
                    depth[e, k, a], ret[e, k, a] = d, rw + r
                    h, crashed = 1, False
                    while h < H:
                        b = val[(h, code, there)][2]
                        if b is None:  # a cell that allows nothing
                            break
                        path[e, k, a, h - 1] = b
                        code, there, _, eat, last = trans[h - 1][(code, there)][b]
                        counts["eat_later"] += int(eat)
                        counts["last_later"] += int(last and code == END)
                        crashed = code == CRASH
                        if code < 0:
                            break
                        h += 1
                    assert crashed == (d < H), (e, k, a, d, H)
                    counts["crash_in_ret"] += int(crashed)
    finally:
        orc.world.fear = fear
    return dict(depth=depth, ret=ret, path=path, ends=ends, crash9=crash9, sims=sims, **counts)


def plan_mask(depth, ret, mask):
    """plan_mask [E, K] int64 from the tables by the stated rule; mask None: all nine."""
    E, K, _ = depth.shape
    bit = 1 << np.arange(NA)
    m = np.full((E, K), ALL, np.int64) if mask is None else (mask.astype(np.int64) & ALL)
    in_m = ((m[:, :, None] >> np.arange(NA)) & 1) == 1
    key = depth * 100000 + (ret + 50000)  # lexicographic (depth, ret): |ret| is far below 50000
    top = np.where(in_m, key, -1).max(-1, keepdims=True)
    return ((in_m & (key == top)) * bit).sum(-1)


def paths_array(paths):
    """oracle_plan_plain's path lists as oracle_plan's [E, K, 9, 3] array."""
    E, K = len(paths), len(paths[0])
    out = np.full((E, K, NA, HORIZON_MAX - 1), NO_ACTION, np.int64)
    for e in range(E):
        for k in range(K):
            for a in range(NA):
                out[e, k, a, :len(paths[e][k][a])] = paths[e][k][a]
    return out


def near_apple_spawn(sc, E, rng, eat_first=False):
    """(spawn [E, N], rl [E, K], scripted [E, N - K]) int32 for a replayed reset: every RL agent within Manhattan
    distance 3 of its own apple (2 or 3 where the map allows, so that the apple is eaten at a step >= 2), the
    scripted agents among the road cells nearest to an apple, all cells distinct and off the RL agents' apples.
    eat_first: every RL agent but the last stands next to its apple and proposes the unit move onto it, the last
    one proposes 0: after that step its apple is the env's last one wherever the others' moves went through."""
    N, K, W = sc.N, sc.K, sc.W
    free = sc.free_cells.astype(np.int64)
    fr, fc = free // W, free % W
    apples = [int(x) for x in sc.apples[:K]]
    spawn = np.zeros((E, N), np.int32)
    rl = rng.integers(0, NA, (E, K)).astype(np.int32)
    for e in range(E):
        taken = set(apples)
        for k in range(K):
            ap = apples[k]
            dist = np.abs(fr - ap // W) + np.abs(fc - ap % W)
            want = (1,) if eat_first and k < K - 1 else (2, 3)
            cand = [int(c) for c, d in zip(free, dist) if d in want and int(c) not in taken]
            if not cand:
                cand = [int(c) for c, d in zip(free, dist) if 1 <= d <= 3 and int(c) not in taken]
            if not cand:
                cand = [int(free[i]) for i in np.argsort(dist, kind="stable") if int(free[i]) not in taken][:1]
            c = cand[int(rng.integers(0, len(cand)))]
            taken.add(c)
            spawn[e, k] = c
            dr, dc = ap // W - c // W, ap % W - c % W
            if eat_first:
                rl[e, k] = 0
                if k < K - 1 and abs(dr) + abs(dc) == 1:
                    rl[e, k] = 1 if dr == -1 else 2 if dr == 1 else 3 if dc == -1 else 4  # U, D, L, R
        centre = apples[int(rng.integers(0, K))]
        order = np.argsort(np.abs(fr - centre // W) + np.abs(fc - centre % W), kind="stable")
        rest = [int(free[i]) for i in order if int(free[i]) not in taken]
        near = rest[: max(N - K + 4, 6)]
        pick = rng.choice(len(near), N - K, replace=False) if N > K else []
        for j, i in enumerate(pick):
            spawn[e, K + j] = near[int(i)]
    scripted = rng.integers(0, NA, (E, N - K)).astype(np.int32)
    return spawn, rl, scripted


def _walk(name: str, visit):
    """The oracle's own run of a case as a list of ops, in order: {"op": "step", "rl", "scripted"} (None: the step's
    own draws), {"op": "reset", "spawn"} and {"op": "compare", ...} with "where", "rl" ([E, K] int32 or None),
    "scripted" (None or [E, N - K]), "joint" [E, N], "mask" [E, K] uint16, "pos" [E, N]; ``visit(orc, sc, comp)`` is
    called at every comparison.  -> (case, ops)."""
    case = CASES[CASE_IDS.index(name)]
    sc, orc = make_oracle(case)
    E, K, N = case.E, sc.K, sc.N
    rng = np.random.default_rng(500 + case.seed)
    obs = np.zeros((K, E, sc.HW), np.float32)
    outs = (O.StepOut * E)()
    ops = []

    def compare(where, rl, scripted):
        joint = oracle_joint(orc, sc, rl)
        if scripted is not None:
            joint = np.concatenate([rl, scripted], 1).astype(np.int32)
        ops.append(dict(op="compare", where=where, rl=rl, scripted=scripted, joint=joint, mask=L.masks_of(orc, sc),
                        pos=orc.positions()))
        visit(orc, sc, ops[-1])

    def step(rl):
        ops.append(dict(op="step", rl=rl, scripted=None))
        orc.vec_step(rl, obs=obs, outs=outs)

    def reset(spawn):
        ops.append(dict(op="reset", spawn=spawn))
        for e in range(E):
            orc.reset_one(e, spawn=spawn[e], episode=orc.envs[e].episode + 1)  # gw_reset starts a new episode

    for t in range(STEPS):
        rl = rng.integers(0, NA, (E, K)).astype(np.int32) if t % 2 == 0 else None
        if t in COMPARE_AT:
            compare(f"{name} step {t}", rl, None)
        step(rl)
    spawn, rl, scripted = R.clustered_spawn(sc, E, rng)
    reset(spawn)
    compare(f"{name} clustered", rl, scripted if N > K else None)
    spawn, rl, scripted = near_apple_spawn(sc, E, rng)
    reset(spawn)
    compare(f"{name} near apple", rl, scripted if N > K else None)
    if K >= 2:
        spawn, rl, _ = near_apple_spawn(sc, E, rng, eat_first=True)
        reset(spawn)
        step(rl)
        compare(f"{name} last apple", rng.integers(0, NA, (E, K)).astype(np.int32), None)
    return case, ops


@functools.lru_cache(maxsize=None)
def reference_run(name: str):
    """The memoised reference of a case, computed once per session and never modified: "case", "ops" (_walk's) and
    "comps" (the compare ops), each with "tab" ({H: oracle_plan's dict} for H in HORIZONS) and "hz" ({H: the depth
    table of _step_horizon_ref.oracle_horizon, the world without apples after step 1})."""
    def visit(orc, sc, c):
        c["tab"] = {H: oracle_plan(orc, sc, c["joint"], H) for H in HORIZONS}
        c["hz"] = {H: R.oracle_horizon(orc, sc, c["joint"], H)["depth"] for H in HORIZONS}

    case, ops = _walk(name, visit)
    return dict(case=case, ops=ops, comps=[o for o in ops if o["op"] == "compare"])


@functools.lru_cache(maxsize=None)
def plain_run(name: str):
    """The plain search over the same run (CPU tests only): per comparison "plain" ({H: (depth, ret, path array)})."""
    def visit(orc, sc, c):
        c["plain"] = {}
        for H in HORIZONS:
            d, r, p = oracle_plan_plain(orc, sc, c["joint"], H)
            c["plain"][H] = (d, r, paths_array(p))

    return [o for o in _walk(name, visit)[1] if o["op"] == "compare"]
