"""Record tests/golden/shapes_traj.npz: CustomMAEnv trajectories from the REFERENCE Python on the open
maps of tests/_shapes.py (every row of SHAPES but 64x64), in the replay form of the traj_*.npz files.

Runs where make_golden.py runs (the reference checkout beside the repository; its stand-ins for
pettingzoo / gymnasium / pygame are make_golden.install_stubs, nothing is added here).  The scenario
goes to the reference as the JSON dict tests/_shapes.open_scenario_dict builds, the one
marlnav.scenario.compile_scenario compiles for the oracle and the kernels.

Per row two trajectories of STEPS steps: FeAR on (fear_weight -5.0) and FeAR off.  Even seeds drive the
RL agents with uniform actions, odd seeds with masked ones (make_golden.run_traj).  The seeds are chosen
so that every row ends an episode, every row with N >= 2 crashes and every FeAR-on trajectory has a
non-zero FeAR (tests/test_shapes_cpu.py asserts all three on the file).

Layout: "<row id>/s<seed>/<key>" for the keys of run_traj plus fear and fear_weight; "rows" lists the
row ids recorded, "<row id>/seeds" that row's seeds.

Rows the reference cannot run: none.  (2x2 with N = 4 spawns through rng.choice without replacement,
custom/ma_customenv.py:376, so a full map ends at once.)  64x64 is left out for size: one K = 8 obs
there is 32 KB per step; that row rests on the oracle's piecewise pins and on grid64_n8's trajectories.

usage:  python tests/golden/make_golden_shapes.py
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
from make_golden import import_reference, install_stubs, make_env_factory, run_traj  # noqa: E402
import _shapes  # noqa: E402

STEPS = 40
FEAR_WEIGHT = -5.0
# row id -> (FeAR-on seed, FeAR-off seed)
SEEDS = {sid: (2 * i, 2 * i + 1) for i, sid in enumerate(_shapes.SHAPE_IDS)}
SEEDS["9x7_n2_k2"] = (38, 27)  # two agents on 62 cells: seeds 2 and 3 neither crash nor end an episode in 40 steps


def main():
    install_stubs()
    G, CA, R, M = import_reference()
    flat, rows = {}, []
    for row in _shapes.SHAPES:
        H, W, N, K, holes = row[:5]
        sid = _shapes.shape_id(row)
        if H * W == 4096:
            continue
        fac = make_env_factory(G, M, _shapes.open_scenario_dict(H, W, N, K, holes), sid)
        for fear, seed in zip((True, False), SEEDS[sid]):
            d = run_traj(fac, W, N, K, fear, FEAR_WEIGHT, seed, STEPS, "uniform" if seed % 2 == 0 else "masked")
            for k, v in d.items():
                flat[f"{sid}/s{seed}/{k}"] = v
            flat[f"{sid}/s{seed}/fear_on"] = np.array(int(fear))
            flat[f"{sid}/s{seed}/fear_weight"] = np.array(FEAR_WEIGHT)
            print(f"{sid} seed {seed} fear {int(fear)}: {int(d['done'].sum())} episodes, "
                  f"{int(d['crashes'].sum())} crashes, {int((d['fear'] != 0).sum())} non-zero FeAR")
        flat[f"{sid}/seeds"] = np.array(SEEDS[sid])
        rows.append(sid)
        R.CountValidMovesOfAffected_tuple.cache_clear()
    flat["rows"] = np.array(rows)
    path = os.path.join(OUT, "shapes_traj.npz")
    np.savez_compressed(path, **flat)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(rows)} rows")


if __name__ == "__main__":
    main()
