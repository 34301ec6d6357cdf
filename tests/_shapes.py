"""Open-map scenarios at the agent counts and map shapes where the step, FeAR and obs kernels branch.

Every rollout fixture of the suite before this file was a one-cell-wide ring road (level3_like) with
W in {16, 32, 64}, N in {4, 5, 8} and K in {1, 2, 3}.  ``SHAPES`` walks the template parameters
(N, KMAX), the obs writer's store paths and the divisions by W, H*W/4 and H*W/8; each row names the
branch it is there for.  ``open_scenario`` is the one builder shared by the golden recorder
(tests/golden/make_golden_shapes.py), the CPU pins (tests/test_shapes_cpu.py) and the GPU sweep
(tests/test_gpu_shapes.py)."""
import functools
import os

import numpy as np

from marlnav import scenario as S

# (H, W, N, K, holes, the branch the row reaches)
SHAPES = [
    (7, 9, 3, 3, ((3, 4),), "HW=63: scalar obs path, odd W, KMAX=N at N<=4"),
    (9, 7, 2, 2, ((4, 3),), "transpose of the above, N=2"),
    (5, 5, 6, 4, ((0, 0), (2, 2)), "HW=25 scalar path, N>4 pair lists, K=4"),
    (3, 4, 7, 7, (), "HW4=3, N=7, K=N, more than half the map occupied"),
    (1, 8, 2, 1, (), "H=1, HW4=2, HW8==1"),
    (2, 2, 4, 2, (), "HW4==1, free cells == N"),
    (2, 2, 2, 2, (), "HW4==1 with room to move"),
    (6, 6, 7, 3, (), "N=7 with uint32_t tasks"),
    (4, 6, 6, 6, ((1, 1),), "N=6, K=N"),
    (5, 8, 5, 5, (), "HW%8==0: the bf16 writer is legal, K=5"),
    (13, 3, 3, 1, (), "W=3, HW=39"),
    (64, 64, 8, 8, ((10, 10),), "HW=4096 at K=8: tables exceed OBS_TAB_MAX, largest LDS"),
]


def shape_id(row) -> str:
    H, W, N, K = row[:4]
    return f"{H}x{W}_n{N}_k{K}"


SHAPE_IDS = [shape_id(r) for r in SHAPES]
BY_ID = dict(zip(SHAPE_IDS, SHAPES))


def open_scenario_dict(H, W, N, K, holes=()) -> dict:
    """The scenario in the reference's JSON schema: all road but ``holes``, three overlapping policies
    (one- and two-step, every direction) and three MdR regions (stay, Down2, Left1)."""
    region = np.ones((H, W))
    for r, c in holes:
        region[r, c] = 0
    road = np.argwhere(region == 1)
    whole = {"slicex": [0, H, 0], "slicey": [0, W, 0]}
    policies = {
        "00": dict(stepWeights=[1, 1, 1], directionWeights=[1, 1, 1, 1], **whole),
        "01": dict(stepWeights=[0, 2, 1], directionWeights=[0, 1, 0, 3], slicex=[0, H, 2], slicey=[0, W, 0]),
        "02": dict(stepWeights=[1, 0, 3], directionWeights=[2, 0, 1, 0], slicex=[0, H, 0], slicey=[1, W, 3]),
    }
    mdrs = {
        "00": dict(mdr=0, **whole),
        "01": dict(mdr=6, slicex=[0, H, 0], slicey=[0, W, 2]),
        "02": dict(mdr=3, slicex=[1, H, 2], slicey=[0, W, 0]),
    }
    apples = {f"apple_{k}": [int(x) for x in road[(7 * k + 3) % len(road)]] for k in range(K)}
    return {"AgentLocations": [], "Map": {"Region": region.tolist(), "Walls": [], "OneWays": []}, "MdRs": mdrs,
            "N_Agents": N, "N_Intelligent": K, "Policies": policies, "SpecificAction4Agents": [],
            "defaultAction": "random", "Apples": apples}


def open_scenario(H, W, N, K, holes=()) -> S.CompiledScenario:
    return S.compile_scenario(open_scenario_dict(H, W, N, K, holes), name=f"open{H}x{W}_n{N}_k{K}")


@functools.lru_cache(maxsize=None)
def scenario(sid: str) -> S.CompiledScenario:
    """The compiled scenario of a table row, by its id (compiled once per session; never modified)."""
    return open_scenario(*BY_ID[sid][:5])


# What the C oracle's own FeAR-on rollout of each row holds at the sweep's parameters (E = 33, 20 steps,
# max_steps = 12, seed = 7): episodes done, crashes, non-zero (env, k) FeAR values, restricted moves.
# tests/test_shapes_cpu.py pins the oracle to these numbers; the GPU sweep asserts that none is zero, so
# no row can pass by doing nothing.
ORACLE_COUNTS = {
    "7x9_n3_k3": (78, 112, 447, 408), "9x7_n2_k2": (43, 22, 139, 258), "5x5_n6_k4": (450, 927, 1601, 1135),
    "3x4_n7_k7": (647, 2772, 2710, 1351), "1x8_n2_k1": (128, 39, 111, 687), "2x2_n4_k2": (587, 945, 654, 975),
    "2x2_n2_k2": (206, 384, 529, 713), "6x6_n7_k3": (336, 546, 1228, 1043), "4x6_n6_k6": (486, 1360, 2417, 1170),
    "5x8_n5_k5": (246, 545, 1624, 742), "13x3_n3_k1": (97, 50, 208, 688), "64x64_n8_k8": (41, 16, 96, 121),
}
SWEEP = dict(E=33, steps=20, max_steps=12, seed=7)


@functools.lru_cache(maxsize=None)
def oracle_counts(sid: str):
    """(episodes done, crashes, non-zero (env, k) FeAR, restricted moves) of the oracle's FeAR-on rollout of
    the row at SWEEP's parameters (CPU only; computed once per session)."""
    from oracle import oracle as O
    sc, E = scenario(sid), SWEEP["E"]
    orc = O.OracleEnvs(sc, E, fear=True, fear_weight=-5.0, max_steps=SWEEP["max_steps"], seed=SWEEP["seed"], reset=False)
    obs = np.zeros((sc.K, E, sc.HW), np.float32)
    orc.reset_all(obs=obs)
    outs = (O.StepOut * E)()
    done = crashes = nonzero = restricted = 0
    for _ in range(SWEEP["steps"]):
        orc.vec_step(None, obs=obs, outs=outs)
        for e in range(E):
            done += int(outs[e].done)
            crashes += int(outs[e].crashes)
            nonzero += sum(outs[e].fear[k] != 0 for k in range(sc.K))
            restricted += bin(outs[e].restricted_bits).count("1")
    return done, crashes, nonzero, restricted


TRAJ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes_traj.npz")


def traj_cases():
    """[(row id, seed)] of tests/golden/shapes_traj.npz (make_golden_shapes.py)."""
    z = np.load(TRAJ)
    return [(str(sid), int(s)) for sid in z["rows"] for s in z[f"{sid}/seeds"]]


def load_traj(sid: str, seed: int):
    """-> (the trajectory in _replay.replay's form, FeAR on?, fear_weight)."""
    z = np.load(TRAJ)
    pre = f"{sid}/s{seed}/"
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    return d, bool(d.pop("fear_on")), float(d.pop("fear_weight"))
