"""The step outcome preview's reference: the C oracle stepped once per (env, RL agent, action) on a copy of the
env's state, and the cases tests/test_gpu_step_preview.py runs (chosen here, on the CPU, so that the oracle's own
tables reach every kind of entry the test's coverage condition names)."""
import dataclasses

import numpy as np

from _shapes import open_scenario
from marlnav import scenario as S
from oracle import oracle as O

NA = 9
ALL = 0x1FF


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    scen: str          # a built-in, or "open:H,W,N,K" (tests/_shapes.open_scenario)
    E: int
    fear: bool = True
    variant: int = 0
    seed: int = 3
    max_steps: int = 12


# E = 37 is no multiple of the kernel's 4 envs per block; N = 5 is the first size on the per-lane pair lists;
# N = K = 8 has 72 tasks per env, so lanes 0-7 take a second turn
CASES = [
    Case("level3", "level3", 37),
    Case("n5_k5", "open:5,8,5,5", 14),
    Case("n8_k2", "open:6,6,8,2", 18),
    Case("n8_k8_fear_off", "open:6,6,8,8", 9, fear=False),  # (the oracle's FeAR at K = N = 8 would take most of the time)
    Case("single_k1", "level3_single", 21, variant=1),
]
CASE_IDS = [c.name for c in CASES]
STEPS = 30
PREVIEW_AT = (0, 1, 2, 5, 9, 13, 20, 29)  # the steps previewed and compared (device-random RL actions at the odd ones)
REPLAY_ROUNDS = 2


def scenario_of(case: Case):
    if case.scen.startswith("open:"):
        return open_scenario(*[int(x) for x in case.scen[5:].split(",")])
    return S.builtin(case.scen)


def make_oracle(case: Case):
    sc = scenario_of(case)
    orc = O.OracleEnvs(sc, case.E, fear=case.fear, fear_weight=-5.0, max_steps=case.max_steps, seed=case.seed,
                       reset=False, variant=case.variant)
    orc.reset_all(obs=np.zeros((sc.K, case.E, sc.HW), np.float32))
    return sc, orc


def oracle_joint(orc, sc, rl):
    """[E, N] int32: the joint action the oracle's next step applies (its own Philox draws for what is not given),
    read from a trial step on a copy of each env's state."""
    E = orc.E
    joint = np.zeros((E, sc.N), np.int32)
    for e in range(E):
        saved = type(orc.envs[e]).from_buffer_copy(orc.envs[e])
        out = orc.step_one(e, None if rl is None else rl[e], None, auto_reset=False)[2]
        joint[e] = list(out.actions)[: sc.N]
        orc.envs[e] = saved
    return joint


def oracle_tables(orc, sc, joint):
    """(outcome [E, K, 9] uint16, reward_alt [E, K, 9] f64): for every (e, k, a) the oracle env stepped once on a
    copy of its state with the joint action ``joint[e]`` except that RL agent k plays a, auto_reset off:
    crash_bits | restricted_bits << 8 and reward[k].  The oracle's state is left as it was."""
    E, K, N = orc.E, sc.K, sc.N
    outcome = np.zeros((E, K, NA), np.uint16)
    reward = np.zeros((E, K, NA), np.float64)
    for e in range(E):
        saved = type(orc.envs[e]).from_buffer_copy(orc.envs[e])
        scripted = joint[e, K:].copy() if N > K else None
        for k in range(K):
            for a in range(NA):
                rl = joint[e, :K].copy()
                rl[k] = a
                out = orc.step_one(e, rl, scripted, auto_reset=False)[2]
                outcome[e, k, a] = (out.crash_bits & 0xFF) | ((out.restricted_bits & 0xFF) << 8)
                reward[e, k, a] = out.reward[k]
                orc.envs[e] = type(saved).from_buffer_copy(saved)
    return outcome, reward


def derived(outcome, mask):
    """(crash9 [E, K], safe_mask [E, K]) uint16 from the outcome table by the stated rule; mask None: all nine."""
    E, K, _ = outcome.shape
    own = (outcome.astype(np.int64) >> np.arange(K)[None, :, None]) & 1           # bit k of entry (e, k, a)
    crash9 = (own << np.arange(NA)[None, None, :]).sum(-1)
    m = np.full((E, K), ALL, np.int64) if mask is None else (mask.astype(np.int64) & ALL)
    safe = m & ~crash9
    return crash9.astype(np.uint16), np.where(safe != 0, safe, m).astype(np.uint16)


def coverage(outcome, reward, mask, K, variant):
    """What one comparison's oracle tables show, as counts: own crashes, restricted bits, the closer reward
    (+1, or +0.1 in the single-agent variant: an entry whose reward is none of the sums of -10, 20, 40),
    safe_mask != mask, apple rewards (>= 20), the all-eaten bonus (>= 40)."""
    crash9, safe = derived(outcome, mask)
    m = np.full(crash9.shape, ALL, np.int64) if mask is None else (mask.astype(np.int64) & ALL)
    step = 0.1 if variant == 1 else 1.0
    base = reward - np.round(reward / 10.0) * 10.0  # what is left beside the multiples of ten
    return dict(own_crash=int((crash9 != 0).sum()), restricted=int(((outcome >> 8) != 0).sum()),
                closer=int(np.isclose(base, step).sum()), safe_differs=int((safe.astype(np.int64) != m).sum()),
                apple=int((reward >= 20).sum()), all_eaten=int((reward >= 40).sum()))


def clustered_spawn(sc, E, rng):
    """(spawn [E, N], rl [E, K], scripted [E, N-K]) int32 for a replayed reset: RL agent k one or two cells from
    its own apple where the map allows, everybody else among the road cells nearest to the apples, all cells
    distinct; in the even envs the RL agents propose the unit move towards their apple, else a uniform action."""
    N, K, W = sc.N, sc.K, sc.W
    free = sc.free_cells.astype(np.int64)
    fr, fc = free // W, free % W
    spawn = np.zeros((E, N), np.int32)
    rl = rng.integers(0, NA, (E, K)).astype(np.int32)
    for e in range(E):
        taken = set()
        for k in range(K):
            ap = int(sc.apples[k])
            order = np.argsort(np.abs(fr - ap // W) + np.abs(fc - ap % W), kind="stable")
            cand = [int(free[i]) for i in order[1:7] if int(free[i]) not in taken and int(free[i]) not in
                    [int(x) for x in sc.apples[:K]]] or [int(free[i]) for i in order if int(free[i]) not in taken]
            c = cand[int(rng.integers(0, len(cand)))]
            taken.add(c)
            spawn[e, k] = c
            dr, dc = ap // W - c // W, ap % W - c % W
            if e % 2 == 0 and abs(dr) + abs(dc) == 1:
                rl[e, k] = 1 if dr == -1 else 2 if dr == 1 else 3 if dc == -1 else 4  # U, D, L, R
        centre = int(sc.apples[int(rng.integers(0, K))])
        order = np.argsort(np.abs(fr - centre // W) + np.abs(fc - centre % W), kind="stable")
        rest = [int(free[i]) for i in order if int(free[i]) not in taken]
        near = rest[: max(N - K + 4, 6)]
        pick = rng.choice(len(near), N - K, replace=False) if N > K else []
        for j, i in enumerate(pick):
            spawn[e, K + j] = near[int(i)]
    scripted = rng.integers(0, NA, (E, N - K)).astype(np.int32)
    return spawn, rl, scripted
