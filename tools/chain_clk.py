"""Measurement only: phase durations of the defer path's two launches per step, step_v2<.., DEFER>
(step_v2_block, slots 0-6) and fear_v2 (fear_block, slots 8-13), thread 0 of blocks 0-63, from the
GW_STEP_CLK build (tools/step_clk.sh; loaded through MARLNAV_LIB, never by the product path).

Usage: MARLNAV_LIB=.../libgridenv_clk.so GW_KERNEL=defer python tools/chain_clk.py [envs] [steps] [scenario]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marl-responsible-nav_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from marlnav import _lib  # noqa: E402
from marlnav import scenario as S  # noqa: E402
from marlnav.vec_env import VecGridEnv  # noqa: E402

STEP = ["loads+fill+sync", "draws", "world update", "finish_env", "to stats", "block stats"]
FEAR = ["loads+fill+sync", "A plan", "B sims", "C values+tail", "block stats"]


def table(title, d, names):
    ph = np.diff(d, axis=1)
    print(f"{title}: {d.shape[0]} blocks, cycles per phase (median / max over blocks), ~us at 2.4 GHz")
    for i, n in enumerate(names):
        print(f"  {n:16s} {int(np.median(ph[:, i])):7d} {int(ph[:, i].max()):7d}  {np.median(ph[:, i]) / 2400:6.2f}")
    tot = d[:, -1] - d[:, 0]
    print(f"  {'total':16s} {int(np.median(tot)):7d} {int(tot.max()):7d}  {np.median(tot) / 2400:6.2f}")


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    scen = sys.argv[3] if len(sys.argv) > 3 else "grid32"
    assert os.environ.get("MARLNAV_LIB"), "needs the measurement build (tools/step_clk.sh)"
    lib = _lib.load()
    lib.gw_step_debug_clocks.argtypes = [C.c_void_p]
    env = VecGridEnv(S.builtin(scen), num_envs=E, fear=True, fear_weight=-5.0, seed=42, stats=True)
    assert env.kernel_path == "defer", env.kernel_path
    env.set_obs_async(True)
    env.reset()
    for _ in range(steps):
        env.step()
    torch.cuda.synchronize()
    buf = np.zeros((64, 16), dtype=np.uint64)
    assert lib.gw_step_debug_clocks(buf.ctypes.data) == 0
    d = buf.astype(np.int64)
    table("step_v2<DEFER>", d[:, 0:7], STEP)
    table("fear_v2", d[:, 8:14], FEAR)
    env.close()


if __name__ == "__main__":
    main()
