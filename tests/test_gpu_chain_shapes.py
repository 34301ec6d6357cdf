"""Block geometry of the defer path's two launches per step: step_v2<.., DEFER> (32-env blocks with
lane-parallel draws for N <= 4, 128-env blocks above) and fear_v2 (one lane per (env, actor) in
phases A and C, 9-bit valid sets for the V counts).

Every comparison is bit-exact against the C oracle (tests/test_gpu_parity.py's rollout check plus
the state, the statistics rows' integer fields and, per step, the Resp rows from the oracle's
FeAR_4_one_actor on the pre-step snapshot)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu
STEPS = 20
INT_FIELDS = {1: "episodes", 3: "crashes", 4: "apples", 6: "done_len", 7: "env_steps"}


def _close(sc, loc, k):
    r, c = loc // sc.W, loc % sc.W
    return (np.abs(r - r[k]) + np.abs(c - c[k])) <= 5


def _oracle_rows(sc, loc, act, mdr):
    """[K, N] Resp rows and [K] sums of one env: FeAR_4_one_actor over each actor's close set."""
    rows, sums = np.zeros((sc.K, sc.N)), np.zeros(sc.K)
    for k in range(sc.K):
        ids = np.flatnonzero(_close(sc, loc, k)).astype(np.int32)
        s, resp, _, _ = O.fear_one_actor(sc.H, sc.W, sc.region, loc, ids, act[ids], mdr, k)
        rows[k], sums[k] = resp[k], s
    return rows, sums


def _outs(outs, name, n, E):
    return np.array([list(getattr(outs[e], name))[:n] for e in range(E)])


def _rollout(sc, E, steps=STEPS, variant=0, seed=7, rows=True, expect_fear=True):
    """Native-RNG rollout with auto-reset on the GPU == the oracle's, every step; -> per-step (fear, fear_row)."""
    env = VecGridEnv(sc, num_envs=E, fear=True, fear_weight=-5.0, max_steps=12, auto_reset=True, seed=seed,
                     final_obs=True, debug=True, stats=True, fear_rows=True, variant=variant)
    orc = O.OracleEnvs(sc, E, fear=True, fear_weight=-5.0, max_steps=12, seed=seed, reset=False, variant=variant)
    K, N = sc.K, sc.N
    obs_o = np.zeros((K, E, sc.HW), np.float32)
    fin_o = np.zeros((K, E, sc.HW), np.float32)
    orc.reset_all(obs=obs_o)
    obs_g, _ = env.reset()
    np.testing.assert_array_equal(obs_g.reshape(K, E, -1).cpu().numpy(), obs_o)
    outs = (O.StepOut * E)()
    trace, done_total, nonzero = [], 0, 0
    for t in range(steps):
        pre = orc.positions()
        env.out["fear_row"].fill_(float("nan"))
        r = env.step()
        orc.vec_step(None, obs=obs_o, outs=outs, final_obs=fin_o)
        torch.cuda.synchronize()
        for name, field, n in (("actions", "actions", N), ("mdr", "mdr", N), ("final_pos", "final_pos", N),
                               ("reward", "reward", K), ("fear", "fear", K), ("shaped", "shaped", K),
                               ("term", "term", K), ("trunc", "trunc", K)):
            np.testing.assert_array_equal(getattr(r, name).cpu().numpy(), _outs(outs, field, n, E), err_msg=f"t={t} {name}")
        np.testing.assert_array_equal(r.mask.cpu().numpy().astype(np.uint16), _outs(outs, "mask", K, E), err_msg=f"t={t} mask")
        for name, field in (("crash_bits", "crash_bits"), ("restr_bits", "restricted_bits"), ("done", "done"),
                            ("ep_return", "ep_return"), ("ep_fear", "ep_fear"), ("ep_len", "ep_len"),
                            ("apples", "apples_caught"), ("crashes", "crashes")):
            np.testing.assert_array_equal(getattr(r, name).cpu().numpy(), np.array([getattr(outs[e], field) for e in range(E)]),
                                          err_msg=f"t={t} {name}")
        np.testing.assert_array_equal(r.obs.reshape(K, E, -1).cpu().numpy(), obs_o, err_msg=f"t={t} obs")
        dn = np.array([outs[e].done for e in range(E)])
        ended = np.flatnonzero(dn)
        np.testing.assert_array_equal(r.final_obs.reshape(K, E, -1)[:, ended].cpu().numpy(), fin_o[:, ended])
        # the statistics rows: as many as the block geometry says, integer fields exact
        st = r.stats.cpu().numpy()
        assert st.shape[0] == env.lib.gw_stats_rows(env.handle)
        want = {1: dn.sum(), 3: sum(outs[e].crashes for e in range(E)), 4: sum(outs[e].apples_caught for e in range(E)),
                6: sum(outs[e].ep_len for e in range(E) if outs[e].done), 7: E}
        for i, name in INT_FIELDS.items():
            assert st[:, i].sum() == want[i], (t, name)
        # the state
        gs = {n: v.cpu().numpy() for n, v in env.state().items()}
        np.testing.assert_array_equal(gs["pos"].T, orc.positions(), err_msg=f"t={t} state pos")
        for n, f in (("t", "t"), ("episode", "episode"), ("score", "score"), ("fear_score", "fear_score")):
            np.testing.assert_array_equal(gs[n], np.array([getattr(orc.envs[e], f) for e in range(E)]).astype(gs[n].dtype),
                                          err_msg=f"t={t} state {n}")
        fr = r.fear_row.cpu().numpy()
        assert not np.isnan(fr).any()
        if rows:
            acts, mdr, fe = r.actions.cpu().numpy(), r.mdr.cpu().numpy(), r.fear.cpu().numpy()
            for e in range(E):
                wr, ws = _oracle_rows(sc, pre[e], acts[e], mdr[e])
                np.testing.assert_array_equal(fr[e], wr, err_msg=f"t={t} e={e} fear_row")
                np.testing.assert_array_equal(fe[e], ws, err_msg=f"t={t} e={e} fear")
        nonzero += int((fr != 0).sum())
        done_total += int(dn.sum())
        trace.append((r.fear.cpu().numpy().copy(), fr.copy()))
    env.close()
    assert done_total > 0  # auto-resets happened
    assert nonzero > 0 or not expect_fear or E < 8  # FeAR was not trivially zero
    return trace


@pytest.fixture
def defer(monkeypatch):
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    monkeypatch.setenv("GW_KERNEL", "defer")


@pytest.mark.parametrize("E", [1, 31, 32, 33, 63, 64, 65, 129])
@pytest.mark.parametrize("name", ["grid32", "level3"])
def test_env_counts_around_block_edges(name, E, defer):
    _rollout(S.builtin(name), E)


def test_n8_pair_lists(defer):
    sc = S.builtin("grid64_n8")
    assert sc.N == 8 and sc.K == 2
    _rollout(sc, 17)


def test_single_rl_agent_variant(defer):
    """K = 1 (variant = 1, the single-agent env on its own scenario): every output, the state and the
    statistics; the Resp rows where the scenario has a second agent."""
    sc = S.builtin("level3_single")
    assert sc.K == 1
    _rollout(sc, 33, variant=1, rows=sc.N > 1, expect_fear=False)


def _crowded(sc, E):
    """E spawns with all four agents pairwise within Manhattan distance 5 on free cells, and joint actions
    that all differ from the cells' MdR."""
    free = set(int(c) for c in sc.free_cells)
    spawns = []
    for c in sorted(free):
        r0, c0 = divmod(c, sc.W)
        near = sorted(x for x in free if abs(x // sc.W - r0) + abs(x % sc.W - c0) <= 2)
        if len(near) >= sc.N:
            spawns.append(near[: sc.N])
        if len(spawns) == E:
            break
    assert len(spawns) == E, "the map has too few crowded neighbourhoods"
    loc = np.array(spawns, np.int32)
    mdr = np.asarray(sc.mdr)[loc].astype(np.int32)
    act = (mdr + 1 + (np.arange(E)[:, None] + np.arange(sc.N)[None, :]) % 8) % 9  # never the MdR
    return loc, act.astype(np.int32), mdr


def test_crowded_block_fills_the_task_lists(defer):
    sc = S.builtin("grid32")
    E, K, N = 64, sc.K, sc.N
    loc, act, mdr = _crowded(sc, E)
    assert (act != mdr).all()
    for e in range(E):  # on the CPU: every actor's close set is full
        for k in range(K):
            assert _close(sc, loc[e], k).all(), (e, k)
    env = VecGridEnv(sc, num_envs=E, fear=True, fear_weight=-5.0, max_steps=1000, debug=True, fear_rows=True)
    env.reset(spawn=torch.as_tensor(loc))
    env.out["fear_row"].fill_(float("nan"))
    r = env.step(act[:, :K].copy(), act[:, K:].copy())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(r.actions.cpu().numpy(), act)
    np.testing.assert_array_equal(r.mdr.cpu().numpy(), mdr)
    fr, fe = r.fear_row.cpu().numpy(), r.fear.cpu().numpy()
    env.close()
    for e in range(E):
        wr, ws = _oracle_rows(sc, loc[e], act[e], mdr[e])
        np.testing.assert_array_equal(fr[e], wr, err_msg=f"e={e} fear_row")
        np.testing.assert_array_equal(fe[e], ws, err_msg=f"e={e} fear")
    assert (fr != 0).any()


def _fear_trace(E, steps, patch):
    """fear / fear_row per step of a grid32 rollout; patch: every step is a gw_step_patch_next step."""
    env = VecGridEnv("grid32", num_envs=E, fear=True, fear_weight=-5.0, max_steps=12, seed=7, debug=True,
                     fear_rows=True, obs=not patch)
    env.reset()
    out = []
    for _ in range(steps):
        if patch:
            win = torch.empty((env.K, E, patch, patch), device=env.device)
            env.patch_next(patch, win)
        r = env.step()
        torch.cuda.synchronize()
        out.append((r.fear.cpu().numpy().copy(), r.fear_row.cpu().numpy().copy()))
    env.close()
    return out


def test_merged_and_window_writer_launch_agree_with_defer(monkeypatch):
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    monkeypatch.setenv("GW_KERNEL", "defer")
    ref = _fear_trace(33, 12, 0)
    rows = _fear_trace(36, 12, 11)  # fear_rows_kernel (E % 4 == 0 for the window writer); envs 0-32 are the same envs
    monkeypatch.setenv("GW_KERNEL", "merged")
    merged = _fear_trace(33, 12, 0)
    assert any((fr != 0).any() for _, fr in ref)
    for t, ((f0, r0), (f1, r1), (f2, r2)) in enumerate(zip(ref, merged, rows)):
        np.testing.assert_array_equal(f0, f1, err_msg=f"t={t} merged fear")
        np.testing.assert_array_equal(r0, r1, err_msg=f"t={t} merged fear_row")
        np.testing.assert_array_equal(f0, f2[:33], err_msg=f"t={t} fear_rows_kernel fear")
        np.testing.assert_array_equal(r0, r2[:33], err_msg=f"t={t} fear_rows_kernel fear_row")
