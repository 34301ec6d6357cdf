"""Per-agent FeAR responsibility rows from the step (gw_step_out.fear_row, VecGridEnv(fear_rows=True)).

1. The reference's own FeAR_4_one_actor known-answer cases (tests/golden/fear.npz, recorded from
   custom/Responsibility.py:135-210) run through the STEP kernels -- fear_v2 wide / narrow (defer
   path) and step_v2's inline FeAR (merged path) -- one case per env, one step: the Resp row and its
   np.sum bit for bit, no case left out.  Only the actor's MdR enters FeAR_4_one_actor and half the
   cases draw it at random, so each group is split by that value and every split runs on a
   scenario whose MdR table is that constant.
2. The same through fear_rows_kernel (the FeAR launch that carries the window writer).
3. Native Philox rollouts: every step's rows == gw_fear_matrix's on the pre-step snapshot.
4. The new output is result-neutral.  5. FeAR off / actor plays its MdR: explicit zero rows.
6. gw_fear_row_accum and Rollout(resp_matrix=True), eager and graph-replayed.  7. evaluate().

Summation bound (6, 7): any order of summing n f64 terms x_i differs from the exact sum by at most
(n - 1) u sum|x_i| (1 + O(n u)), u = 2^-53; the tests allow n * 2^-53 * sum|x_i| between the
kernel's fixed tree and numpy's pairwise sum, computed from the data."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = {"level3": 1200, "grid32": 400, "grid64_n8": 250, "open6_n8": 250}
KERNEL_PATHS = {
    "defer": {"GW_KERNEL": "defer"},
    "defer_narrow": {"GW_KERNEL": "defer", "GW_FEAR_BE": "narrow"},
    "merged": {"GW_KERNEL": "merged"},
}
K = 2
U = 2.0 ** -53


def _set_path(monkeypatch, path):
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    for k, v in KERNEL_PATHS[path].items():
        monkeypatch.setenv(k, v)


def _group(name):
    z = np.load(os.path.join(GOLD, "fear.npz"))
    return {k.split("/", 1)[1]: np.asarray(z[k]) for k in z.files if k.startswith(name + "/")}


def _scenario(region2d: np.ndarray, N: int, mdr_value: int) -> S.CompiledScenario:
    """A scenario on the case's map (as test_gpu_world_kats._scenario) with K = 2 RL agents and the
    constant MdR ``mdr_value`` in every cell."""
    base = S.builtin("level3")
    H, W = region2d.shape
    free = np.flatnonzero(region2d.reshape(-1) == 1).astype(np.int32)
    return dataclasses.replace(
        base, name="fear_kat", H=H, W=W, N=N, K=K, region=(region2d != 0).astype(np.uint8).reshape(-1),
        policy_id=np.zeros(H * W, np.uint8), policy_keys=base.policy_keys[:1], policy_p=base.policy_p[:1],
        policy_cdf=base.policy_cdf[:1], mdr=np.full(H * W, mdr_value, np.uint8), apples=free[:K].copy(),
        free_cells=free, okmask=S.okmask_table(region2d), action_mask=S.action_mask_table(region2d))


def _manhattan_close(loc, W, who):
    """[n, N] bool: agent j within Manhattan distance 5 of agent who[i] (itself included):
    CustomMAEnv.close_agents (custom/ma_customenv.py:456-464)."""
    r, c = loc // W, loc % W
    ar = np.arange(loc.shape[0])
    return (np.abs(r - r[ar, who][:, None]) + np.abs(c - c[ar, who][:, None])) <= 5


def _check_fixture(g, name):
    n, N = g["act"].shape
    ar = np.arange(n)
    actor = g["actor"]
    assert n == GROUPS[name] and actor.min() >= 0 and actor.max() < K
    W = g["region"].shape[1]
    # the fixture's in_list is exactly the actor's close set, which is what the step builds
    np.testing.assert_array_equal(g["in_list"] != 0, _manhattan_close(g["loc"].astype(np.int64), W, actor))
    assert (g["act"][ar, actor] == g["mdr"][ar, actor]).any(), "no actor == MdR case"
    assert (g["in_list"] == 0).any(), "no agent outside in_list"
    assert (g["resp"] != 0).any(), "no non-zero Resp entry"


def _run_kats(g, patch=0):
    """Every case of the group through one step; -> (cases compared, fear_row [n, N], fear [n]) of the
    case's actor, NaN where no env ran the case.  patch > 0: the step carries the window writer
    (patch_next armed, no dense obs, E padded to a multiple of 4 with repeated cases)."""
    n, N = g["act"].shape
    actor = g["actor"]
    v_all = g["mdr"][np.arange(n), actor]
    rows = np.full((n, N), np.nan)
    fear = np.full(n, np.nan)
    compared = 0
    for v in np.unique(v_all):
        idx = np.flatnonzero(v_all == v)
        real = idx.size
        if patch and idx.size % 4:
            idx = np.concatenate([idx, idx[: 4 - idx.size % 4]])
        E = idx.size
        env = VecGridEnv(_scenario(g["region"], N, int(v)), num_envs=E, fear=True, fear_weight=-5.0,
                         max_steps=1000, debug=True, fear_rows=True, obs=not patch)
        try:
            env.reset(spawn=torch.as_tensor(g["loc"][idx].astype(np.int32)))
            if patch:
                assert env.kernel_path == "defer" and E % 4 == 0
                win = torch.full((K, E, patch, patch), float("nan"), device=env.device)
                env.patch_next(patch, win)
            env.out["fear_row"].fill_(float("nan"))
            act = g["act"][idx].astype(np.int32)
            r = env.step(act[:, :K].copy(), act[:, K:].copy())
            torch.cuda.synchronize()
            if patch:  # the writer ran inside the step
                assert torch.equal(win, env.obs_patch(patch))
            np.testing.assert_array_equal(r.actions.cpu().numpy(), act)
            assert (r.mdr.cpu().numpy() == v).all()
            fr = r.fear_row.cpu().numpy()
            assert fr.shape == (E, K, N) and not np.isnan(fr).any()
            fe = r.fear.cpu().numpy()
            a = actor[idx]
            rows[idx] = fr[np.arange(E), a]
            fear[idx] = fe[np.arange(E), a]
            compared += real
        finally:
            env.close()
    return compared, rows, fear


def _assert_kats(g, name, compared, rows, fear):
    n = GROUPS[name]
    assert compared == n and not np.isnan(rows).any() and not np.isnan(fear).any()
    ar = np.arange(n)
    np.testing.assert_array_equal(rows, g["resp"][ar, g["actor"]], err_msg=f"{name}: Resp row")
    np.testing.assert_array_equal(fear, g["sum"], err_msg=f"{name}: np.sum(Resp)")


@pytest.mark.parametrize("path", sorted(KERNEL_PATHS))
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_reference_kats_through_the_step_kernels(group, path, monkeypatch):
    _set_path(monkeypatch, path)
    g = _group(group)
    _check_fixture(g, group)
    _assert_kats(g, group, *_run_kats(g))


@pytest.mark.parametrize("be", ["wide", "narrow"])
def test_reference_kats_through_the_window_writer_launch(be, monkeypatch):
    """grid32 once more with patch_next(11, ...) armed and FeAR on: the step is fear_rows_kernel."""
    monkeypatch.setenv("GW_KERNEL", "defer")
    monkeypatch.setenv("GW_FEAR_BE", be)
    g = _group("grid32")
    _assert_kats(g, "grid32", *_run_kats(g, patch=11))


@pytest.mark.parametrize("scen,E", [("grid32", 256), ("grid64_n8", 64)])
def test_native_rollout_rows_match_fear_matrix(scen, E):
    sc = S.builtin(scen)
    N, W = sc.N, sc.W
    env = VecGridEnv(sc, num_envs=E, fear=True, fear_weight=-5.0, seed=5, debug=True, fear_rows=True)
    env.reset()
    nonzero = 0
    for t in range(8):
        cells = env.positions().cpu().numpy().astype(np.int64)  # pre-step
        r = env.step()
        torch.cuda.synchronize()
        acts = r.actions.cpu().numpy()
        fr, fe = r.fear_row.cpu().numpy(), r.fear.cpu().numpy()
        for k in range(sc.K):
            close = _manhattan_close(cells, W, np.full(E, k))
            bits = (close.astype(np.int64) << np.arange(N)).sum(1).astype(np.uint8)
            want = env.fear_matrix(cells.astype(np.int32), acts, in_list=bits)["resp"].cpu().numpy()[:, k, :]
            np.testing.assert_array_equal(fr[:, k, :], want, err_msg=f"step {t} agent {k}")
            for e in range(E):  # numpy's own pairwise order over the N x N matrix
                m = np.zeros((N, N))
                m[k] = want[e]
                assert fe[e, k] == np.sum(m), (t, e, k)
        nonzero += int((fr != 0).sum())
    assert nonzero > 0
    env.close()


def _neutral_run(rows, fear_async):
    env = VecGridEnv("grid32", num_envs=512, fear=True, fear_weight=-5.0, seed=9, max_steps=12, debug=True,
                     stats=True, fear_rows=rows)
    if fear_async:
        assert env.kernel_path == "defer"
        env.set_obs_async(True, fear_async=True)
    env.reset()
    steps = []
    for _ in range(16):
        r = env.step()
        env.fear_fence()
        env.obs_fence()
        steps.append({f.name: getattr(r, f.name).clone() for f in dataclasses.fields(r)
                      if f.name != "fear_row" and getattr(r, f.name) is not None})
    st = env.state()
    torch.cuda.synchronize()
    env.close()
    return steps, st


@pytest.mark.parametrize("path,fear_async", [("defer", False), ("merged", False), ("defer", True)])
def test_fear_rows_are_result_neutral(path, fear_async, monkeypatch):
    _set_path(monkeypatch, path)
    (a, sa), (b, sb) = _neutral_run(True, fear_async), _neutral_run(False, fear_async)
    for t, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for n in x:
            assert torch.equal(x[n], y[n]), (t, n)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n


@pytest.mark.parametrize("path", ["defer", "merged"])
def test_zero_rows_fear_off_and_actor_on_its_mdr(path, monkeypatch):
    _set_path(monkeypatch, path)
    for scen in ("grid32", "grid64_n8"):
        off = VecGridEnv(scen, num_envs=96, fear=False, seed=3, fear_rows=True)
        off.reset()
        off.out["fear_row"].fill_(float("nan"))
        r = off.step()
        assert bool((r.fear_row == 0).all()) and bool((r.fear == 0).all())
        off.close()
        on = VecGridEnv(scen, num_envs=512, fear=True, seed=3, debug=True, fear_rows=True)
        on.reset()
        seen = 0
        for _ in range(4):
            on.out["fear_row"].fill_(float("nan"))
            r = on.step()
            assert not bool(torch.isnan(r.fear_row).any())
            same = r.actions[:, : on.K] == r.mdr[:, : on.K]  # [E, K]
            assert bool((r.fear_row[same] == 0).all())
            seen += int(same.sum())
            idx = torch.arange(on.K, device=on.device)
            assert bool((r.fear_row[:, idx, idx] == 0).all())  # j == k
        assert seen > 0
        on.close()


def _bound(n_terms, x):
    return n_terms * U * np.abs(x).sum(0)


def _accum(rows, active, totals, steps):
    E, Kk, N = rows.shape
    _lib.check(_lib.load().gw_fear_row_accum(rows.data_ptr(), active.data_ptr() if active is not None else None,
                                             E, Kk, N, totals.data_ptr(), steps.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "gw_fear_row_accum")


def test_fear_row_accum_op():
    E, N = 4096, 4
    rng = np.random.default_rng(0)
    x = rng.uniform(-1.0, 1.0, (E, K, N))
    act = (rng.random(E) < 0.6).astype(np.uint8)
    rows, active = torch.as_tensor(x).cuda(), torch.as_tensor(act).cuda()
    got = []
    for _ in range(2):
        totals = torch.zeros((K, N), dtype=torch.float64, device="cuda")
        steps = torch.zeros((), dtype=torch.int64, device="cuda")
        _accum(rows, active, totals, steps)
        assert int(steps) == 1
        got.append(totals.cpu().numpy().copy())
        _accum(rows, None, totals, steps)  # += on top, every env
        assert int(steps) == 2
        got.append(totals.cpu().numpy().copy())
    np.testing.assert_array_equal(got[0], got[2])  # deterministic
    np.testing.assert_array_equal(got[1], got[3])
    xa = x[act != 0]
    assert (np.abs(got[0] - xa.sum(0)) <= _bound(E, xa)).all()
    both = np.concatenate([xa, x])
    assert (np.abs(got[1] - both.sum(0)) <= _bound(2 * E, both)).all()
    assert np.abs(got[0]).min() > 0
    assert torch.equal(active.cpu(), torch.as_tensor(act))  # the mask is read only


def _window_rollout(graph, steps_eager=10):
    """The c5patch-style rollout (MLP actors on 11 x 11 windows, FeAR on, no dense obs) with the
    responsibility total on; graph: 2 eager steps, then ring-phase graphs of 8 steps."""
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    E, P, slots, G = 1024, 11, 16, 8
    env = VecGridEnv("grid32", num_envs=E, fear=True, fear_weight=-5.0, max_steps=40, seed=42, stats=True,
                     obs=False, fear_rows=True)
    actors = MultiAgentActors(env.K, P, P, arch="mlp", device=env.device, seed=0)
    ro = Rollout(env, actors, replay_slots=slots, training=True, seed=42, patch=P, resp_matrix=True)
    assert ro.fused
    ro.reset()
    per_step = []
    if graph:
        for _ in range(2):
            ro.step()
        graphs = ro.capture(G)
        graphs.replay()
    else:
        for _ in range(steps_eager):
            per_step.append(ro.step().fear_row.cpu().numpy().copy())
    ro.fence()
    tot = ro.totals()
    torch.cuda.synchronize()
    env.close()
    return tot, per_step, E


def test_rollout_resp_total_and_graph_replay():
    tot, per_step, E = _window_rollout(False)
    assert tot["resp_steps"] == 10 and tuple(tot["resp"].shape) == (K, 4)
    x = np.concatenate(per_step)  # [10 E, K, N]
    got = tot["resp"].numpy()
    assert (np.abs(got - x.sum(0)) <= _bound(E, x)).all()  # (narrower than the 10 E terms allow)
    assert np.abs(got).sum() > 0
    # each agent's row total is its FeAR total (the statistics' fear field sums both agents)
    assert abs(got.sum() - tot["fear"]) <= 2 * _bound(x.shape[0] * 4, x).sum()
    tot_g, _, _ = _window_rollout(True)
    assert tot_g["resp_steps"] == 10
    assert torch.equal(tot_g["resp"], tot["resp"])  # graph replay == eager, bit for bit
    assert tot_g["fear"] == tot["fear"]


def test_evaluate_resp_matrix():
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("grid32")
    E, T = 64, 40
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    r = evaluate(actors, sc, episodes=E, max_steps=T, fear=True, seed=11, record_actions=True, resp_matrix=True)
    resp = r["resp"].numpy()
    assert resp.shape == (sc.K, sc.N) and resp.dtype == np.float64
    assert "resp" not in evaluate(actors, sc, episodes=E, max_steps=8, fear=True, seed=11)
    # each agent's accumulated FeAR over the episodes still running: the recorded actions replayed
    env = VecGridEnv(sc, num_envs=E, fear=True, max_steps=T, auto_reset=False, seed=11, fear_rows=True)
    env.reset()
    active = np.ones(E, bool)
    fear_k, abs_k, terms, steps = np.zeros(sc.K), np.zeros(sc.K), 0, 0
    for a in r["actions"]:
        s = env.step(a)
        fe, fr = s.fear.cpu().numpy(), s.fear_row.cpu().numpy()
        fear_k += fe[active].sum(0)
        abs_k += np.abs(fr[active]).sum((0, 2))
        terms += int(active.sum()) * sc.N
        steps += int(active.sum())
        active &= s.done.cpu().numpy() == 0
    env.close()
    assert steps == r["steps"] and abs_k.sum() > 0
    assert abs(fear_k.sum() - r["fear"]) <= (terms + 2) * U * abs_k.sum()
    # n = the row's terms, + 2 for the division by steps and the multiplication back
    assert (np.abs(resp.sum(1) * r["steps"] - fear_k) <= (terms + 2) * U * abs_k).all(), (resp, fear_k)
