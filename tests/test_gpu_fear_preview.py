"""FeAR preview before the step (gw_fear_preview) and the responsibility shield (gw_fear_shield).

1. The preview equals the next step, bit for bit: before every step of a native Philox rollout (max_steps = 5,
   12 steps: every env auto-resets at least twice) the previewed table equals that step's fear_alt, the previewed
   joint action its actions and the previewed MdR its mdr; device-random and given RL actions; the defer (wide /
   narrow) and merged paths; built-ins (N = 4, 8) and level3 with N = 3 and N = 5; once under the rollouts'
   pipeline (lazy async obs, unjoined FeAR), where the previous step's fear_alt kernel may still be reading the
   steps' record buffer while the preview writes its own.
2. The reference's FeAR_4_one_actor known-answer cases (tests/golden/fear.npz, level3 and open6_n8) WITHOUT a
   step: reset(spawn = the case's cells), fear_preview(the case's actions), against oracle.fear_one_actor for
   both RL agents and all nine actions, formed as tests/test_gpu_fear_alt.py forms its table.
3. Neutrality: an env that previews twice before every step (same table both times) and its twin that never
   does agree in every StepResult field, the state snapshot and the obs writers' counts.
4. FeAR-off envs: the preview on fear=False equals the fear_alt of a fear=True twin, step for step.
5. The shield op against the numpy restatement of its rule (tests/_fear_shield_ref.py).
6. The unilateral guarantee through a real step, with a floor on how often the shield acted (confirmed on the
   CPU oracle inside the test, from the same spawns and actions).
7. evaluate(shield=...), Rollout(shield=...) totals, capture raises.

E = 203 is a multiple of neither 4 (envs per fear_alt_kernel block) nor 64, and not of 256 (preview_rec_kernel)."""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from _fear_shield_ref import shield_ref
from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv
from oracle import oracle as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KERNEL_PATHS = {
    "defer": {"GW_KERNEL": "defer"},
    "defer_narrow": {"GW_KERNEL": "defer", "GW_FEAR_BE": "narrow"},
    "merged": {"GW_KERNEL": "merged"},
}
E0 = 203
K = 2
NA = 9


def _set_path(monkeypatch, path):
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    for k, v in KERNEL_PATHS[path].items():
        monkeypatch.setenv(k, v)


def _rollout_scenario(scen):
    """A built-in, or "<built-in>@N": that built-in with N world agents (its map, policies and K)."""
    name, _, n = scen.partition("@")
    sc = S.builtin(name)
    return dataclasses.replace(sc, name=f"{name}_n{n}", N=int(n)) if n else sc


def _i32(E, N, dev):
    return torch.full((E, N), -7, dtype=torch.int32, device=dev)


# ---- 1. preview == the next step -------------------------------------------------------------------------

@pytest.mark.parametrize("path", sorted(KERNEL_PATHS))
@pytest.mark.parametrize("scen", ["level3", "grid32", "grid64_n8", "level3@3", "level3@5"])
def test_preview_equals_the_next_step(scen, path, monkeypatch):
    _set_path(monkeypatch, path)
    sc = _rollout_scenario(scen)
    for given in (False, True):
        env = VecGridEnv(sc, num_envs=E0, fear=True, fear_weight=-5.0, seed=5, max_steps=5, debug=True, fear_alt=True)
        assert env.kernel_path == KERNEL_PATHS[path]["GW_KERNEL"]
        env.reset()
        gen = torch.Generator(device=env.device).manual_seed(31)
        acts, mdr = _i32(E0, sc.N, env.device), _i32(E0, sc.N, env.device)
        resets = nonzero = 0
        for t in range(12):
            rl = torch.randint(0, NA, (E0, sc.K), generator=gen, device=env.device, dtype=torch.int32) if given else None
            acts.fill_(-7)
            mdr.fill_(-7)
            tab = env.fear_preview(rl, None, actions=acts, mdr=mdr)
            env.out["fear_alt"].fill_(float("nan"))
            r = env.step(rl)
            torch.cuda.synchronize()
            assert torch.equal(tab, r.fear_alt), (scen, path, given, t)  # bit for bit (no NaN: equal() is exact)
            assert torch.equal(acts, r.actions), (scen, path, given, t)
            assert torch.equal(mdr, r.mdr), (scen, path, given, t)
            if given:
                assert torch.equal(acts[:, :sc.K], rl)
            resets += int(r.done.sum())
            nonzero += int((tab != 0).sum())
        assert resets >= 2 * E0 and nonzero > 0
        env.close()


def test_preview_beside_the_unjoined_fear_kernels(monkeypatch):
    """The rollouts' pipeline: lazy async obs and unjoined FeAR (| 4).  Step t's fear_alt kernel runs on the aux
    stream from the steps' record buffer; the preview of step t + 1 is enqueued on the caller's stream with no
    fence in between and must neither disturb it nor be disturbed: both tables are compared after the fence."""
    _set_path(monkeypatch, "defer")
    env = VecGridEnv("grid32", num_envs=E0, fear=True, fear_weight=-5.0, seed=8, max_steps=5, debug=True,
                     fear_alt=True)
    assert env.kernel_path == "defer"
    env.set_obs_async("lazy", fear_async=True)
    env.reset()
    last = None
    nonzero = 0
    for t in range(13):
        acts, mdr = _i32(E0, env.N, env.device), _i32(E0, env.N, env.device)
        tab = env.fear_preview(None, None, actions=acts, mdr=mdr) if t < 12 else None
        if last is not None:  # step t - 1, whose FeAR-owned outputs are ordered by the fence
            env.fear_fence()
            torch.cuda.synchronize()
            ptab, pacts, pmdr, r = last
            assert torch.equal(ptab, r.fear_alt), t - 1
            assert torch.equal(pacts, r.actions) and torch.equal(pmdr, r.mdr), t - 1
            nonzero += int((ptab != 0).sum())
        if t < 12:
            last = (tab, acts, mdr, env.step())
    env.obs_fence()
    torch.cuda.synchronize()
    assert nonzero > 0
    env.close()


# ---- 2. reference cases without a step -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _group(name):
    z = np.load(os.path.join(GOLD, "fear.npz"))
    return {k.split("/", 1)[1]: np.asarray(z[k]) for k in z.files if k.startswith(name + "/")}


def _kat_scenario(region2d, N, mdr_value):
    """A scenario on the case's map with K = 2 RL agents and the constant MdR ``mdr_value``."""
    base = S.builtin("level3")
    H, W = region2d.shape
    free = np.flatnonzero(region2d.reshape(-1) == 1).astype(np.int32)
    return dataclasses.replace(
        base, name="fear_preview_kat", H=H, W=W, N=N, K=K, region=(region2d != 0).astype(np.uint8).reshape(-1),
        policy_id=np.zeros(H * W, np.uint8), policy_keys=base.policy_keys[:1], policy_p=base.policy_p[:1],
        policy_cdf=base.policy_cdf[:1], mdr=np.full(H * W, mdr_value, np.uint8), apples=free[:K].copy(),
        free_cells=free, okmask=S.okmask_table(region2d), action_mask=S.action_mask_table(region2d))


def _close(loc, W, k):
    """[N] bool: within Manhattan distance 5 of agent k, itself included (CustomMAEnv.close_agents)."""
    r, c = loc // W, loc % W
    return (np.abs(r - r[k]) + np.abs(c - c[k])) <= 5


def _oracle_rows(H, W, region, loc, joint, mdr, ks):
    """[len(ks), 9] f64: oracle.fear_one_actor's np.sum(Resp) for actor k over its close list, k playing a."""
    out = np.full((len(ks), NA), np.nan)
    for i, k in enumerate(ks):
        ids = np.flatnonzero(_close(loc.astype(np.int64), W, k)).astype(np.int32)
        acts = joint[ids].astype(np.int32)
        at = int(np.flatnonzero(ids == k)[0])
        for a in range(NA):
            acts[at] = a
            out[i, a] = O.fear_one_actor(H, W, region, loc, ids, acts, mdr, k)[0]
    return out


@pytest.mark.parametrize("group,n", [("level3", 1200), ("open6_n8", 250)])
def test_reference_cases_without_a_step(group, n):
    g = _group(group)
    assert g["act"].shape[0] == n
    N = g["act"].shape[1]
    H, W = g["region"].shape
    v_all = g["mdr"][np.arange(n), g["actor"]]  # only the actor's MdR enters FeAR_4_one_actor: split by it
    want = np.stack([_oracle_rows(H, W, g["region"], g["loc"][i], g["act"][i], np.full(N, v_all[i], np.int32),
                                  range(K)) for i in range(n)])
    got = np.full((n, K, NA), np.nan)
    for v in np.unique(v_all):
        idx = np.flatnonzero(v_all == v)
        env = VecGridEnv(_kat_scenario(g["region"], N, int(v)), num_envs=idx.size, fear=True, max_steps=1000)
        try:
            env.reset(spawn=torch.as_tensor(g["loc"][idx].astype(np.int32)))
            act = g["act"][idx].astype(np.int32)
            acts, mdr = _i32(idx.size, N, env.device), _i32(idx.size, N, env.device)
            tab = env.fear_preview(act[:, :K].copy(), act[:, K:].copy(), actions=acts, mdr=mdr)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(acts.cpu().numpy(), act)
            assert bool((mdr == int(v)).all())
            np.testing.assert_array_equal(env.positions().cpu().numpy(), g["loc"][idx])  # the world did not move
            got[idx] = tab.cpu().numpy()
        finally:
            env.close()
    print(f"{group}: {int((got != want).sum())} of {got.size} entries differ, {int((want != 0).sum())} non-zero")
    np.testing.assert_array_equal(got, want)
    ar, actor = np.arange(n), g["actor"]
    np.testing.assert_array_equal(got[ar, actor, g["act"][ar, actor]], g["sum"])  # the reference's own number
    assert (want != 0).any()


# ---- 3. neutrality ---------------------------------------------------------------------------------------

def _neutral_run(preview, path):
    env = VecGridEnv("grid32", num_envs=E0, fear=True, fear_weight=-5.0, seed=9, max_steps=5, debug=True, stats=True,
                     fear_rows=True, fear_alt=True, final_obs=True)
    assert env.kernel_path == KERNEL_PATHS[path]["GW_KERNEL"]
    env.reset()
    steps = []
    for _ in range(12):
        if preview:
            a = env.fear_preview()
            b = env.fear_preview()
            assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
        r = env.step()
        torch.cuda.synchronize()
        steps.append({f.name: getattr(r, f.name).clone() for f in dataclasses.fields(r)
                      if getattr(r, f.name) is not None})
    st = env.state()
    counts = env.obs_delta_counts()
    torch.cuda.synchronize()
    env.close()
    return steps, st, counts


@pytest.mark.parametrize("path", ["defer", "merged"])
def test_preview_is_result_neutral(path, monkeypatch):
    _set_path(monkeypatch, path)
    (a, sa, ca), (b, sb, cb) = _neutral_run(True, path), _neutral_run(False, path)
    assert len(a) == len(b) == 12 and ca == cb
    for t, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys() and {"obs", "final_obs", "fear_alt", "fear_row", "stats"} <= x.keys()
        for n in x:
            # final_obs starts as NaN and is written for done envs only: NaN compares as a value here
            assert torch.equal(torch.nan_to_num(x[n], nan=-9.0), torch.nan_to_num(y[n], nan=-9.0)), (t, n)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n


def test_status_codes_and_sim_count():
    env = VecGridEnv("grid32", num_envs=E0, fear=True, seed=3)
    with pytest.raises(_lib.GwError, match="before gw_reset"):
        env.fear_preview()
    env.reset()
    out = torch.empty((E0, K, NA), dtype=torch.float64, device=env.device)
    s = torch.cuda.current_stream().cuda_stream
    assert env.lib.gw_fear_preview(None, None, None, out.data_ptr(), None, None, s) == -1   # null env
    assert env.lib.gw_fear_preview(env.handle, None, None, None, None, None, s) == -1       # null table
    ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
    env.count_sims(ctr)
    env.fear_preview(out=out)
    env.count_sims(None)
    torch.cuda.synchronize()
    # per actor 9 (1 + 8 (c - 1)) world updates with close count c in 1..N: between 9 K and 9 K (8 N - 7) per env
    assert 9 * K * E0 <= int(ctr) <= 9 * K * (8 * env.N - 7) * E0
    env.close()


# ---- 4. FeAR-off envs ------------------------------------------------------------------------------------

@pytest.mark.parametrize("scen,variant", [("grid32", 0), ("level3_single", 1)])
def test_preview_on_a_fear_off_env(scen, variant):
    kw = dict(num_envs=E0, fear_weight=-5.0, seed=4, max_steps=5, debug=True, variant=variant)
    off = VecGridEnv(scen, fear=False, **kw)
    on = VecGridEnv(scen, fear=True, fear_alt=True, **kw)
    assert off.K == (1 if variant else 2)
    off.reset()
    on.reset()
    nonzero = 0
    for t in range(12):
        acts = _i32(E0, off.N, off.device)
        tab = off.fear_preview(actions=acts)
        ro, rn = off.step(), on.step()
        torch.cuda.synchronize()
        assert torch.equal(ro.final_pos, rn.final_pos) and torch.equal(ro.actions, rn.actions), t
        assert torch.equal(tab, rn.fear_alt) and torch.equal(acts, rn.actions), t
        assert bool((ro.fear == 0).all())
        nonzero += int((tab != 0).sum())
    assert nonzero > 0
    off.close()
    on.close()


# ---- 5. the shield op ------------------------------------------------------------------------------------

VALUES = np.array([-1.0, -0.5, 0.0, 0.5, 1.0, 2.0])


def _shield(table, actions, mask, probs, E, Kk, tau, agents, out, flags):
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(_lib.load().gw_fear_shield(p(table), p(actions), p(mask), p(probs), E, Kk, tau, agents, p(out), p(flags),
                                          torch.cuda.current_stream().cuda_stream), "gw_fear_shield")


@pytest.mark.parametrize("Kk", [1, 2])
@pytest.mark.parametrize("E", [1, 63, 257])
def test_shield_op_against_numpy(E, Kk):
    rng = np.random.default_rng(100 * E + Kk)
    table = rng.choice(VALUES, (E, Kk, NA))
    acts = rng.integers(0, NA, (E, Kk)).astype(np.int32)
    mask = rng.integers(0, 0x200, (E, Kk)).astype(np.int16)
    mask[rng.random((E, Kk)) < 0.3] = 0x1FF
    mask.reshape(-1)[0] = 0
    probs = rng.choice(np.array([0.05, 0.1, 0.2, 0.3], np.float32), (Kk, E, NA)).astype(np.float32)  # tied maxima
    dev = "cuda"
    t_d, a_d = torch.as_tensor(table).to(dev), torch.as_tensor(acts).to(dev)
    m_d, p_d = torch.as_tensor(mask).to(dev), torch.as_tensor(probs).to(dev)
    seen = set()
    for tau in (-0.5, 0.0, 0.5, 8.0):
        for use_mask, use_probs in ((True, True), (True, False), (False, True), (False, False)):
            for agents in sorted({0, 1, (1 << Kk) - 1, 1 << (Kk - 1)}):
                want_a, want_f = shield_ref(table, acts, mask.view(np.uint16) if use_mask else None,
                                            probs if use_probs else None, tau, agents)
                out = torch.full((E, Kk), -3, dtype=torch.int32, device=dev)
                flags = torch.full((E, Kk), 77, dtype=torch.uint8, device=dev)
                _shield(t_d, a_d, m_d if use_mask else None, p_d if use_probs else None, E, Kk, tau, agents, out, flags)
                np.testing.assert_array_equal(out.cpu().numpy(), want_a)
                np.testing.assert_array_equal(flags.cpu().numpy(), want_f)
                seen |= set(want_f.reshape(-1).tolist())
                # actions_out aliasing actions_in, flags NULL
                alias = a_d.clone()
                _shield(t_d, alias, m_d if use_mask else None, p_d if use_probs else None, E, Kk, tau, agents, alias, None)
                np.testing.assert_array_equal(alias.cpu().numpy(), want_a)
    assert torch.equal(a_d.cpu(), torch.as_tensor(acts))  # inputs are read only
    assert E == 1 or seen == {0, 1, 2, 3}


# ---- 6. the unilateral guarantee -------------------------------------------------------------------------

def _unilateral_case(scen, seed):
    """Seeded spawns (N road cells drawn among the 24 nearest a random road cell, sorted, so that agents meet),
    proposed RL actions and scripted actions, all uniform."""
    sc = S.builtin(scen)
    rng = np.random.default_rng(seed)
    free = sc.free_cells.astype(np.int64)
    fr, fc = free // sc.W, free % sc.W
    spawn = np.zeros((E0, sc.N), np.int32)
    for e in range(E0):
        c = int(rng.integers(0, free.size))
        near = np.argsort(np.abs(fr - fr[c]) + np.abs(fc - fc[c]), kind="stable")[:24]
        spawn[e] = np.sort(free[rng.choice(near, sc.N, replace=False)])
    rl = rng.integers(0, NA, (E0, sc.K)).astype(np.int32)
    scripted = rng.integers(0, NA, (E0, sc.N - sc.K)).astype(np.int32)
    return sc, spawn, rl, scripted


UNILATERAL_SEEDS = {"level3": 611, "grid64_n8": 612}


@pytest.mark.parametrize("scen", sorted(UNILATERAL_SEEDS))
def test_unilateral_guarantee_through_a_step(scen):
    sc, spawn, rl, scripted = _unilateral_case(scen, UNILATERAL_SEEDS[scen])
    joint = np.concatenate([rl, scripted], 1)
    region = sc.region.reshape(sc.H, sc.W)
    # the CPU oracle over the same spawns and actions: the proposed action's FeAR, and the floor it implies
    # (tau = 0: an agent whose proposed action has FeAR > 0 must be replaced)
    want = np.stack([_oracle_rows(sc.H, sc.W, region, spawn[e], joint[e], sc.mdr[spawn[e]].astype(np.int32),
                                  range(sc.K)) for e in range(E0)])  # [E, K, 9]
    prop = np.take_along_axis(want, rl[..., None].astype(np.int64), 2)[..., 0]
    floor = (prop > 0).mean(0)
    print(f"{scen}: oracle FeAR(proposed) > 0 in {floor} of the envs per RL agent")
    assert (floor >= 0.01).all(), "the seeded spawns and actions do not reach the 1 % floor on the CPU oracle"
    env = VecGridEnv(sc, num_envs=E0, fear=True, fear_weight=-5.0, seed=6, max_steps=1000, debug=True)
    ar = torch.arange(E0, device=env.device)
    rl_d = torch.as_tensor(rl).to(env.device)
    replaced = 0
    for k in range(sc.K):
        _, mask = env.reset(spawn=torch.as_tensor(spawn))
        table = env.fear_preview(rl_d, scripted)
        chosen, flags = env.fear_shield(table, rl_d, mask=mask, tau=0.0, agents=1 << k)
        r = env.step(chosen, scripted)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(table.cpu().numpy(), want)  # the preview is the oracle's table
        other = [j for j in range(sc.K) if j != k]
        assert torch.equal(chosen[:, other], rl_d[:, other]) and bool((flags[:, other] == 0).all())
        assert torch.equal(r.actions[:, :sc.K], chosen)
        assert torch.equal(r.fear[:, k], table[ar, k, chosen[:, k].long()]), k  # bit for bit
        ok = (flags[:, k] & 2) == 0
        assert bool((r.fear[:, k][ok] <= 0.0).all())
        assert bool(((flags[:, k] & 1) == (chosen[:, k] != rl_d[:, k]).to(torch.uint8)).all())
        frac = float((flags[:, k] & 1).float().mean())
        print(f"{scen} k={k}: replaced {frac:.3f}, stuck {float((flags[:, k] >> 1).float().mean()):.3f}")
        assert frac >= 0.01
        replaced += int((flags[:, k] & 1).sum())
    assert replaced >= 0.01 * E0 * sc.K
    env.close()


# ---- 7. evaluation and rollouts --------------------------------------------------------------------------

def test_evaluate_with_a_shield():
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("grid32")
    E, T = 64, 24
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    plain = evaluate(actors, sc, episodes=E, max_steps=T, fear=True, seed=11, record_actions=True)
    # every row sum is at most N - 1: tau = N can never replace an action
    loose = evaluate(actors, sc, episodes=E, max_steps=T, fear=True, seed=11, record_actions=True, shield=float(sc.N))
    for name in ("crashes", "apples_caught", "steps", "fear"):
        assert plain[name] == loose[name], name
    assert torch.equal(plain["actions"], loose["actions"])
    assert int(loose["shield_replaced"].sum()) == 0 and int(loose["shield_stuck"].sum()) == 0
    assert "shield_replaced" not in plain
    r = evaluate(actors, sc, episodes=E, max_steps=T, fear=False, seed=11, shield=0.0)  # the reference's eval config
    for name in ("shield_replaced", "shield_stuck"):
        assert tuple(r[name].shape) == (sc.K,) and r[name].dtype == torch.int64
        assert bool((r[name] >= 0).all()) and bool((r[name] <= r["steps"]).all())


@pytest.mark.parametrize("policy", ["actors", "random"])
def test_rollout_shield_totals(policy):
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    env = VecGridEnv("grid32", num_envs=E0, fear=True, fear_weight=-5.0, max_steps=40, seed=42, stats=True)
    actors = MultiAgentActors(env.K, env.H, env.W, arch="mlp", device=env.device, seed=0) if policy == "actors" else None
    ro = Rollout(env, actors, replay_slots=16 if actors is not None else 0, training=True, seed=42, shield=0.0)
    ro.reset()
    rep = torch.zeros(env.K, dtype=torch.int64)
    stuck = torch.zeros(env.K, dtype=torch.int64)
    for t in range(10):
        r = ro.step()
        f = ro.shield_flags.cpu().to(torch.int64)
        rep += (f & 1).sum(0)
        stuck += (f >> 1).sum(0)
        if actors is not None:  # the ring keeps the actor's probabilities: rows of a distribution, not one-hot picks
            p = ro.replay.probs[t % 16]
            assert tuple(p.shape) == (env.K, E0, NA) and bool(((p.sum(-1) - 1).abs() < 1e-4).all())
    ro.fence()
    tot = ro.totals()
    torch.cuda.synchronize()
    assert torch.equal(tot["shield_replaced"], rep) and torch.equal(tot["shield_stuck"], stuck)
    assert tot["env_steps"] == 10 * E0
    if policy == "random":
        assert int(rep.sum()) > 0  # random proposals do get replaced at tau = 0
    if actors is not None:
        with pytest.raises(ValueError):
            ro.capture(8)
    env.close()
    plain = Rollout(VecGridEnv("grid32", num_envs=8, fear=True, stats=True), None)
    assert plain.shield is None and "shield_replaced" not in plain.totals()
    plain.env.close()
