"""Per-action counterfactual FeAR table from the step (gw_set_fear_alt, VecGridEnv(fear_alt=True)).

1. The reference's FeAR_4_one_actor known-answer cases (tests/golden/fear.npz) through fear_alt_kernel,
   one case per env and one step, on the defer (wide / narrow) and merged paths: for both RL agents of
   every case and all nine actions a, fear_alt[e][k][a] bit for bit against oracle.fear_one_actor
   called with k's Manhattan-5 close list and k's entry replaced by a; at the case's own actor and
   a == its action also against the fixture's recorded np.sum, the reference's own number.  As in
   test_gpu_fear_rows, each group is split by the case actor's MdR and every split runs on a scenario
   whose MdR table is that constant (only the actor's MdR enters FeAR_4_one_actor).
2. Native Philox rollouts on both kernel paths, auto-resets included: fear_alt[:, k, action] == fear,
   fear_alt[:, k, MdR] == 0 bit for bit every step, and a seeded sample of entries against
   gw_fear_matrix on the pre-step cells with k's action replaced.  Built-ins (N = 4, 8) and level3
   with N = 3 and N = 5 world agents.
3. The table is result-neutral; NULL switches it off again.  4. FeAR off: zeros; the single-agent env.
5. gw_fear_regret_accum against numpy.  6. Rollout(fear_regret=True) eager == graph replay; evaluate().

Summation bound (5): any order of summing n f64 terms x_i differs from the exact sum by at most
(n - 1) u sum|x_i| (1 + O(n u)), u = 2^-53; the test allows n * 2^-53 * sum|x_i| between the kernel's
fixed tree and math.fsum (the form test_gpu_fear_rows.test_fear_row_accum_op uses), from the data."""
import dataclasses
import functools
import math
import os

import numpy as np
import pytest
import torch

from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv
from oracle import oracle as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = {"level3": 1200, "grid32": 400, "grid64_n8": 250, "open6_n8": 250}
KERNEL_PATHS = {
    "defer": {"GW_KERNEL": "defer"},
    "defer_narrow": {"GW_KERNEL": "defer", "GW_FEAR_BE": "narrow"},
    "merged": {"GW_KERNEL": "merged"},
}
K = 2
NA = 9
U = 2.0 ** -53


def _set_path(monkeypatch, path):
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    for k, v in KERNEL_PATHS[path].items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def _group(name):
    z = np.load(os.path.join(GOLD, "fear.npz"))
    return {k.split("/", 1)[1]: np.asarray(z[k]) for k in z.files if k.startswith(name + "/")}


def _scenario(region2d: np.ndarray, N: int, mdr_value: int) -> S.CompiledScenario:
    """A scenario on the case's map with K = 2 RL agents and the constant MdR ``mdr_value``."""
    base = S.builtin("level3")
    H, W = region2d.shape
    free = np.flatnonzero(region2d.reshape(-1) == 1).astype(np.int32)
    return dataclasses.replace(
        base, name="fear_alt_kat", H=H, W=W, N=N, K=K, region=(region2d != 0).astype(np.uint8).reshape(-1),
        policy_id=np.zeros(H * W, np.uint8), policy_keys=base.policy_keys[:1], policy_p=base.policy_p[:1],
        policy_cdf=base.policy_cdf[:1], mdr=np.full(H * W, mdr_value, np.uint8), apples=free[:K].copy(),
        free_cells=free, okmask=S.okmask_table(region2d), action_mask=S.action_mask_table(region2d))


def _manhattan_close(loc, W, who):
    """[n, N] bool: agent j within Manhattan distance 5 of agent who[i] (itself included):
    CustomMAEnv.close_agents (custom/ma_customenv.py:456-464)."""
    r, c = loc // W, loc % W
    ar = np.arange(loc.shape[0])
    return (np.abs(r - r[ar, who][:, None]) + np.abs(c - c[ar, who][:, None])) <= 5


@functools.lru_cache(maxsize=None)
def _oracle_table(name):
    """[n, K, 9] f64: the oracle's np.sum(Resp) of FeAR_4_one_actor(actor = k) with k playing a, k's
    MdR = the case actor's (the constant of the scenario the case runs on).  Computed once per group
    and shared by the kernel paths; never modified."""
    g = _group(name)
    n, N = g["act"].shape
    H, W = g["region"].shape
    loc = g["loc"].astype(np.int64)
    v_all = g["mdr"][np.arange(n), g["actor"]]
    want = np.full((n, K, NA), np.nan)
    for k in range(K):
        close = _manhattan_close(loc, W, np.full(n, k))
        for i in range(n):
            ids = np.flatnonzero(close[i]).astype(np.int32)
            acts = g["act"][i][ids].astype(np.int32)
            at = int(np.flatnonzero(ids == k)[0])
            mdr = np.full(N, v_all[i], np.int32)
            for a in range(NA):
                acts[at] = a
                want[i, k, a] = O.fear_one_actor(H, W, g["region"], g["loc"][i], ids, acts, mdr, k)[0]
    assert not np.isnan(want).any()
    want.setflags(write=False)
    return want


def _run_kats(g):
    """Every case of the group through one step; -> (cases compared, fear_alt [n, K, 9], fear [n, K])."""
    n, N = g["act"].shape
    v_all = g["mdr"][np.arange(n), g["actor"]]
    alt = np.full((n, K, NA), np.nan)
    fear = np.full((n, K), np.nan)
    compared = 0
    for v in np.unique(v_all):
        idx = np.flatnonzero(v_all == v)
        E = idx.size
        env = VecGridEnv(_scenario(g["region"], N, int(v)), num_envs=E, fear=True, fear_weight=-5.0,
                         max_steps=1000, debug=True, fear_alt=True)
        try:
            env.reset(spawn=torch.as_tensor(g["loc"][idx].astype(np.int32)))
            env.out["fear_alt"].fill_(float("nan"))
            act = g["act"][idx].astype(np.int32)
            r = env.step(act[:, :K].copy(), act[:, K:].copy())
            torch.cuda.synchronize()
            np.testing.assert_array_equal(r.actions.cpu().numpy(), act)
            assert (r.mdr.cpu().numpy() == v).all()
            fa = r.fear_alt.cpu().numpy()
            assert fa.shape == (E, K, NA) and not np.isnan(fa).any()
            alt[idx] = fa
            fear[idx] = r.fear.cpu().numpy()
            compared += E
        finally:
            env.close()
    return compared, alt, fear


@pytest.mark.parametrize("path", sorted(KERNEL_PATHS))
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_reference_kats_through_fear_alt_kernel(group, path, monkeypatch):
    _set_path(monkeypatch, path)
    g = _group(group)
    n = GROUPS[group]
    assert g["act"].shape[0] == n and g["actor"].min() >= 0 and g["actor"].max() < K
    compared, alt, fear = _run_kats(g)
    assert compared == n and not np.isnan(alt).any() and not np.isnan(fear).any()
    want = _oracle_table(group)
    print(f"{group}/{path}: {compared} cases, {int((alt != want).sum())} of {alt.size} entries differ, "
          f"{int((want != 0).sum())} non-zero")
    np.testing.assert_array_equal(alt, want, err_msg=f"{group}: fear_alt vs oracle.fear_one_actor")
    ar, actor = np.arange(n), g["actor"]
    own = alt[ar, actor, g["act"][ar, actor]]
    np.testing.assert_array_equal(own, g["sum"], err_msg=f"{group}: a == act vs the reference's np.sum(Resp)")
    np.testing.assert_array_equal(own, fear[ar, actor])
    assert (want != 0).any()


def _rollout_scenario(scen):
    """A built-in, or "<built-in>@N": that built-in with N world agents (its map, policies and K)."""
    name, _, n = scen.partition("@")
    sc = S.builtin(name)
    return dataclasses.replace(sc, name=f"{name}_n{n}", N=int(n)) if n else sc


# level3@3: fewer agents than any built-in; level3@5: the first N of the kernels' LIST world update.
# Their six steps end episodes through max_steps = 3; gw_fear_matrix, the comparison, is pinned at
# N = 3 and N = 5 by the reference-recorded cases of tests/golden/fear_matrix.npz.
@pytest.mark.parametrize("path", ["defer", "merged"])
@pytest.mark.parametrize("scen,E,steps,max_steps", [
    pytest.param("grid32", 256, 20, 7, id="grid32-256"), pytest.param("grid64_n8", 64, 20, 7, id="grid64_n8-64"),
    pytest.param("level3@3", 7, 6, 3, id="level3@3-7"), pytest.param("level3@5", 7, 6, 3, id="level3@5-7")])
def test_native_rollout_identities_and_fear_matrix(scen, E, steps, max_steps, path, monkeypatch):
    _set_path(monkeypatch, path)
    sc = _rollout_scenario(scen)
    N, W, Kk = sc.N, sc.W, sc.K
    env = VecGridEnv(sc, num_envs=E, fear=True, fear_weight=-5.0, seed=5, max_steps=max_steps, debug=True,
                     fear_alt=True)
    assert env.kernel_path == KERNEL_PATHS[path]["GW_KERNEL"]
    env.reset()
    assert tuple(env.positions().shape) == (E, N)
    rng = np.random.default_rng(17)
    ar = torch.arange(E, device=env.device)
    resets = nonzero = sampled = 0
    for t in range(steps):
        cells = env.positions().cpu().numpy().astype(np.int64)  # pre-step (pre-reset) world
        env.out["fear_alt"].fill_(float("nan"))
        r = env.step()
        torch.cuda.synchronize()
        fa = r.fear_alt
        assert not bool(torch.isnan(fa).any())
        for k in range(Kk):
            assert torch.equal(fa[ar, k, r.actions[:, k].long()], r.fear[:, k]), (t, k)
            assert bool((fa[ar, k, r.mdr[:, k].long()] == 0).all()), (t, k)
        resets += int(r.done.sum())
        nonzero += int((fa != 0).sum())
        # a seeded sample of (env, k, a) against gw_fear_matrix with k's action replaced
        S_ = 24
        es, ks, as_ = rng.integers(0, E, S_), rng.integers(0, Kk, S_), rng.integers(0, NA, S_)
        acts = r.actions.cpu().numpy()[es].copy()
        acts[np.arange(S_), ks] = as_
        close = _manhattan_close(cells[es], W, ks)
        bits = (close.astype(np.int64) << np.arange(N)).sum(1).astype(np.uint8)
        resp = env.fear_matrix(cells[es].astype(np.int32), acts, in_list=bits)["resp"].cpu().numpy()
        got = fa.cpu().numpy()
        for i in range(S_):
            m = np.zeros((N, N))
            m[ks[i]] = resp[i, ks[i]]
            assert got[es[i], ks[i], as_[i]] == O.np_sum(m), (t, es[i], ks[i], as_[i])
        sampled += S_
    assert resets > 0, "no env auto-reset in the run"
    assert nonzero > 0 and sampled == 24 * steps
    env.close()


def _neutral_run(alt, fear_async):
    env = VecGridEnv("grid32", num_envs=512, fear=True, fear_weight=-5.0, seed=9, max_steps=6, debug=True,
                     stats=True, fear_alt=alt)
    if fear_async:
        assert env.kernel_path == "defer"
        env.set_obs_async(True, fear_async=True)
    env.reset()
    steps = []
    for _ in range(10):
        r = env.step()
        env.fear_fence()
        env.obs_fence()
        steps.append({f.name: getattr(r, f.name).clone() for f in dataclasses.fields(r)
                      if f.name != "fear_alt" and getattr(r, f.name) is not None})
        if alt:  # the FeAR-owned table is ordered by the fence as well
            for k in range(env.K):
                ar = torch.arange(env.E, device=env.device)
                assert torch.equal(r.fear_alt[ar, k, r.actions[:, k].long()], r.fear[:, k])
    st = env.state()
    torch.cuda.synchronize()
    env.close()
    return steps, st


@pytest.mark.parametrize("path,fear_async", [("defer", False), ("merged", False), ("defer", True)])
def test_fear_alt_is_result_neutral(path, fear_async, monkeypatch):
    _set_path(monkeypatch, path)
    (a, sa), (b, sb) = _neutral_run(True, fear_async), _neutral_run(False, fear_async)
    assert len(a) == len(b) == 10
    for t, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for n in x:
            assert torch.equal(x[n], y[n]), (t, n)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n


@pytest.mark.parametrize("path", ["defer", "merged"])
def test_null_switches_the_table_off_again(path, monkeypatch):
    _set_path(monkeypatch, path)
    env = VecGridEnv("grid32", num_envs=96, fear=True, seed=3, fear_alt=True)
    env.reset()
    env.out["fear_alt"].fill_(float("nan"))
    r = env.step()
    assert not bool(torch.isnan(r.fear_alt).any())
    _lib.check(env.lib.gw_set_fear_alt(env.handle, None), "gw_set_fear_alt")
    env.out["fear_alt"].fill_(float("nan"))
    for _ in range(2):
        env.step()
    torch.cuda.synchronize()
    assert bool(torch.isnan(env.out["fear_alt"]).all())
    assert env.lib.gw_set_fear_alt(None, None) == -1  # GW_ERR_ARG on a null env
    env.close()


@pytest.mark.parametrize("path", ["defer", "merged"])
def test_fear_off_gives_zeros(path, monkeypatch):
    _set_path(monkeypatch, path)
    for scen in ("grid32", "grid64_n8"):
        off = VecGridEnv(scen, num_envs=96, fear=False, seed=3, fear_alt=True)
        off.reset()
        off.out["fear_alt"].fill_(float("nan"))
        r = off.step()
        assert bool((r.fear_alt == 0).all()) and bool((r.fear == 0).all())
        off.close()


def test_single_agent_variant_identity():
    env = VecGridEnv("level3_single", num_envs=64, fear=True, fear_weight=-5.0, variant=1, seed=4, debug=True,
                     fear_alt=True)
    assert env.K == 1
    env.reset()
    ar = torch.arange(64, device=env.device)
    nonzero = 0
    for _ in range(12):
        env.out["fear_alt"].fill_(float("nan"))
        r = env.step()
        assert not bool(torch.isnan(r.fear_alt).any())
        assert torch.equal(r.fear_alt[ar, 0, r.actions[:, 0].long()], r.fear[:, 0])
        assert bool((r.fear_alt[ar, 0, r.mdr[:, 0].long()] == 0).all())
        nonzero += int((r.fear_alt != 0).sum())
    assert nonzero > 0
    env.close()


def _regret(alt, fear, active, totals, steps):
    E, Kk, _ = alt.shape
    _lib.check(_lib.load().gw_fear_regret_accum(alt.data_ptr(), fear.data_ptr(),
                                                active.data_ptr() if active is not None else None, E, Kk,
                                                totals.data_ptr(), steps.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "gw_fear_regret_accum")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 1000])
def test_fear_regret_accum_op(E, masked):
    rng = np.random.default_rng(E)
    # a table like the kernel's: few distinct values, so ties at the minimum are common
    x = rng.choice(np.array([-1.0, -0.5, -0.125, 0.0, 0.25, 1.0 / 3.0, 0.7]), (E, K, NA))
    pick = rng.integers(0, NA, (E, K))
    f = np.take_along_axis(x, pick[..., None], 2)[..., 0]
    act = (rng.random(E) < 0.6).astype(np.uint8) if masked else None
    if masked:
        act[0] = 1
    alt, fear = torch.as_tensor(x).cuda(), torch.as_tensor(f).cuda()
    active = torch.as_tensor(act).cuda() if masked else None
    got = []
    for _ in range(2):
        totals = torch.zeros((K, 2), dtype=torch.float64, device="cuda")
        steps = torch.zeros((), dtype=torch.int64, device="cuda")
        _regret(alt, fear, active, totals, steps)
        assert int(steps) == 1
        got.append(totals.cpu().numpy().copy())
    np.testing.assert_array_equal(got[0], got[1])  # two launches: identical bits
    keep = np.ones(E, bool) if act is None else act != 0
    m = x.min(2)
    d = (f - m)[keep]  # [n, K] the per-env regrets, the same f64 subtraction
    for k in range(K):
        assert got[0][k, 1] == float((f[keep, k] == m[keep, k]).sum())  # the count column is exact
        exact = math.fsum(d[:, k])
        bound = d.shape[0] * U * np.abs(d[:, k]).sum()
        print(f"E={E} masked={masked} k={k}: |err| {abs(got[0][k, 0] - exact):.3e} bound {bound:.3e}")
        assert abs(got[0][k, 0] - exact) <= bound
    assert (d >= 0).all() and (E < 63 or d.sum() > 0)
    if masked:
        assert torch.equal(active.cpu(), torch.as_tensor(act))  # the mask is read only


def _window_rollout(graph, steps_eager=10):
    """The rollout of test_gpu_fear_rows._window_rollout (MLP actors on 11 x 11 windows, FeAR on, no
    dense obs, ring 16) at E = 256 with the regret total on; graph: 2 eager steps + one 8-step graph."""
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    E, P, slots, G = 256, 11, 16, 8
    env = VecGridEnv("grid32", num_envs=E, fear=True, fear_weight=-5.0, max_steps=40, seed=42, stats=True,
                     obs=False, fear_alt=True)
    assert env.kernel_path == "merged"
    actors = MultiAgentActors(env.K, P, P, arch="mlp", device=env.device, seed=0)
    ro = Rollout(env, actors, replay_slots=slots, training=True, seed=42, patch=P, fear_regret=True)
    assert ro.fused
    ro.reset()
    if graph:
        for _ in range(2):
            ro.step()
        graphs = ro.capture(G)
        graphs.replay()
    else:
        for _ in range(steps_eager):
            ro.step()
    ro.fence()
    tot = ro.totals()
    torch.cuda.synchronize()
    env.close()
    return tot, E


def test_rollout_regret_total_and_graph_replay(monkeypatch):
    _set_path(monkeypatch, "merged")
    tot, E = _window_rollout(False)
    assert tot["fear_regret_steps"] == 10
    assert tuple(tot["fear_regret"].shape) == (K,) and tuple(tot["fear_best"].shape) == (K,)
    assert bool((tot["fear_regret"] >= 0).all()) and float(tot["fear_regret"].sum()) > 0
    assert bool((tot["fear_best"] >= 0).all()) and bool((tot["fear_best"] <= 10 * E).all())
    assert bool((tot["fear_best"] == tot["fear_best"].round()).all())
    tot_g, _ = _window_rollout(True)
    assert tot_g["fear_regret_steps"] == 10
    assert torch.equal(tot_g["fear_regret"], tot["fear_regret"])  # graph replay == eager, bit for bit
    assert torch.equal(tot_g["fear_best"], tot["fear_best"])
    assert tot_g["fear"] == tot["fear"]


def test_evaluate_fear_regret():
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("grid32")
    E, T = 64, 24
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    r = evaluate(actors, sc, episodes=E, max_steps=T, fear=True, seed=11, fear_regret=True)
    for name in ("fear_regret", "fear_best_frac"):
        assert tuple(r[name].shape) == (sc.K,) and r[name].dtype == torch.float64
    assert bool((r["fear_regret"] >= 0).all())
    assert bool((r["fear_best_frac"] >= 0).all()) and bool((r["fear_best_frac"] <= 1).all())
    plain = evaluate(actors, sc, episodes=E, max_steps=8, fear=True, seed=11)
    assert "fear_regret" not in plain and "fear_best_frac" not in plain
    with pytest.raises(ValueError):
        evaluate(actors, sc, episodes=E, max_steps=8, fear=False, fear_regret=True)
