"""Step outcome preview (gw_step_preview) and the crash-aware shield.

1. Against the C oracle, bit for bit: an OracleEnvs twin in native-RNG mode with the same seed; before a handful
   of the 30 steps the preview's outcome / reward_alt tables equal the oracle stepped once per (e, k, a) on a copy
   of its state (tests/_step_preview_ref.py), crash9 and safe_mask follow by the stated rule, the previewed joint
   action is the oracle's own; then both twins step (auto-resets included: max_steps = 12).  After that two
   replayed resets with clustered spawns beside the apples.  Cases (tests/_step_preview_ref.CASES): Level 3 with
   E = 37, N = 5 (the first LIST size), N = 8 with K = 2, N = K = 8 (72 tasks: two turns; FeAR off), the
   single-agent variant with K = 1.  Every case asserts from the ORACLE's tables that they hold an own crash, a
   restricted bit, a closer reward and a safe_mask != mask; the run as a whole an apple reward and the all-eaten
   bonus (test_coverage_of_the_whole_run, from the same cached oracle tables).
2. Consistency with the step on both kernel paths.  3. No side effects.  4. Graph capture.  5. The promise of the
   crash-aware shield, exact.  6. evaluate(shield_crash=True) against the same loop driven by hand.
7. Status codes, the span, the sim count."""
import dataclasses

import numpy as np
import pytest
import torch

import _step_preview_ref as R
from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv
from oracle import oracle as O

pytestmark = pytest.mark.gpu
NA = 9
GW_ERR_ARG, GW_ERR_STATE = -1, -4
GW_SPAN_STEP_PREVIEW = 14
_COVERAGE = {}  # case name -> summed coverage counts of the oracle's tables (filled by test 1)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _compare(env, orc, sc, rl, scripted, where, cov):
    """One preview against the oracle; returns the previewed joint action (numpy)."""
    K = sc.K
    mask_t = env.out["mask"]
    pv = env.step_preview(rl, scripted, mask=mask_t)
    torch.cuda.synchronize()
    joint = pv["actions"].cpu().numpy()
    want_joint = R.oracle_joint(orc, sc, None if rl is None else np.asarray(rl))
    if scripted is None:
        np.testing.assert_array_equal(joint, want_joint, err_msg=f"{where}: joint action")
    else:
        np.testing.assert_array_equal(joint, np.concatenate([rl, scripted], 1), err_msg=f"{where}: joint action")
    outcome, reward = R.oracle_tables(orc, sc, joint)  # the scripted actions from the preview's `actions`
    mask = np.asarray(sc.action_mask)[orc.positions()[:, :K]].astype(np.uint16)
    np.testing.assert_array_equal(_u16(mask_t), mask, err_msg=f"{where}: action mask")
    crash9, safe = R.derived(outcome, mask)
    got_o, got_r = _u16(pv["outcome"]), pv["reward_alt"].cpu().numpy()
    print(f"{where}: {int((got_o != outcome).sum())} outcome and {int((got_r != reward).sum())} reward entries of "
          f"{outcome.size} differ")
    np.testing.assert_array_equal(got_o, outcome, err_msg=f"{where}: outcome")
    assert got_r.dtype == np.float64 and np.array_equal(got_r, reward), f"{where}: reward_alt"  # exact f64 equality
    np.testing.assert_array_equal(_u16(pv["crash9"]), crash9, err_msg=f"{where}: crash9")
    np.testing.assert_array_equal(_u16(pv["safe_mask"]), safe, err_msg=f"{where}: safe_mask")
    for n, v in R.coverage(outcome, reward, mask, K, orc.world.variant).items():
        cov[n] = cov.get(n, 0) + v
    return joint


# ---- 1. against the oracle -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_preview_equals_the_oracle(case):
    sc, orc = R.make_oracle(case)
    E, K = case.E, sc.K
    env = VecGridEnv(sc, num_envs=E, fear=case.fear, fear_weight=-5.0, seed=case.seed, max_steps=case.max_steps,
                     variant=case.variant, debug=True)
    env.reset()
    rng = np.random.default_rng(100 + case.seed)
    obs = np.zeros((K, E, sc.HW), np.float32)
    outs = (O.StepOut * E)()
    cov, dones = {}, 0
    for t in range(R.STEPS):
        rl = rng.integers(0, NA, (E, K)).astype(np.int32) if t % 2 == 0 else None  # odd steps: device-random
        if t in R.PREVIEW_AT:
            _compare(env, orc, sc, rl, None, f"{case.name} step {t}", cov)
        r = env.step(rl)
        orc.vec_step(rl, obs=obs, outs=outs)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(env.positions().cpu().numpy(), orc.positions(), err_msg=f"twins at step {t}")
        np.testing.assert_array_equal(r.reward.cpu().numpy(), np.array([list(outs[e].reward)[:K] for e in range(E)]))
        dones += int(r.done.sum())
    assert dones >= E  # auto-resets were part of the run
    for rnd in range(R.REPLAY_ROUNDS):  # replayed resets: agents clustered beside the apples
        spawn, rl, scripted = R.clustered_spawn(sc, E, rng)
        env.reset(spawn=torch.as_tensor(spawn))
        for e in range(E):
            orc.reset_one(e, spawn=spawn[e])
        _compare(env, orc, sc, rl, scripted if sc.N > K else None, f"{case.name} replay {rnd}", cov)
    env.close()
    print(f"{case.name}: oracle coverage {cov}")
    _COVERAGE[case.name] = cov
    for n in ("own_crash", "restricted", "closer", "safe_differs"):  # a condition on the oracle's tables
        assert cov[n] > 0, (case.name, n, cov)


def test_coverage_of_the_whole_run():
    """At least one case shows an apple reward (>= 20) and one the all-eaten bonus (>= 40 for one agent), in the
    oracle's tables (the cases ran above; run alone, this test runs the two cases that carry them on the CPU)."""
    for name in ("level3", "n8_k2"):
        if name not in _COVERAGE:
            test_preview_equals_the_oracle(R.CASES[R.CASE_IDS.index(name)])
    assert any(c["apple"] > 0 for c in _COVERAGE.values())
    assert any(c["all_eaten"] > 0 for c in _COVERAGE.values())


# ---- 2. consistency with the step ------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["defer", "merged"])
@pytest.mark.parametrize("name", ["level3", "n5_k5", "n8_k8_fear_off"])
def test_preview_entry_of_the_applied_action_is_the_step(name, path, monkeypatch):
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    monkeypatch.setenv("GW_KERNEL", path)
    case = R.CASES[R.CASE_IDS.index(name)]
    sc = R.scenario_of(case)
    E, K = 41, sc.K
    env = VecGridEnv(sc, num_envs=E, fear=case.fear, seed=5, max_steps=5, debug=True)
    assert env.kernel_path == path
    env.reset()
    gen = torch.Generator(device=env.device).manual_seed(17)
    ar = torch.arange(E, device=env.device)
    crashes = dones = 0
    for t in range(12):
        rl = torch.randint(0, NA, (E, K), generator=gen, device=env.device, dtype=torch.int32) if t % 2 else None
        pv = {n: v.clone() for n, v in env.step_preview(rl).items()}
        r = env.step(rl)
        torch.cuda.synchronize()
        assert torch.equal(pv["actions"], r.actions), t
        want = r.crash_bits.to(torch.int32) | (r.restr_bits.to(torch.int32) << 8)
        for k in range(K):
            a = r.actions[:, k].long()
            assert torch.equal(pv["outcome"][ar, k, a].to(torch.int32) & 0xFFFF, want), (t, k)
            assert torch.equal(pv["reward_alt"][ar, k, a], r.reward[:, k]), (t, k)  # bit for bit
        crashes += int((r.crash_bits != 0).sum())
        dones += int(r.done.sum())
    assert crashes > 0 and dones >= E
    env.close()


# ---- 3. no side effects ----------------------------------------------------------------------------------

def _trajectory(preview):
    env = VecGridEnv("level3", num_envs=37, fear=True, fear_weight=-5.0, seed=9, max_steps=6, debug=True)
    env.reset()
    steps = []
    for _ in range(20):
        if preview:
            before = {n: v.clone() for n, v in env.state().items()}
            env.step_preview(mask=env.out["mask"])
            after = env.state()
            torch.cuda.synchronize()
            for n in before:
                assert torch.equal(before[n], after[n]), n
        r = env.step()
        torch.cuda.synchronize()
        steps.append({n: getattr(r, n).clone() for n in ("obs", "reward", "fear", "shaped", "done", "term", "trunc",
                                                          "mask", "final_pos", "ep_return")})
    st, counts = env.state(), env.obs_delta_counts()
    torch.cuda.synchronize()
    env.close()
    return steps, st, counts


def test_preview_has_no_side_effects():
    (a, sa, ca), (b, sb, cb) = _trajectory(True), _trajectory(False)
    assert len(a) == len(b) == 20 and ca == cb
    for t, (x, y) in enumerate(zip(a, b)):
        for n in x:
            assert torch.equal(x[n], y[n]), (t, n)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n


# ---- 4. graph capture ------------------------------------------------------------------------------------

def test_graph_capture():
    env = VecGridEnv("level3", num_envs=37, fear=True, seed=4, debug=True)
    E, K, N = env.E, env.K, env.N
    env.reset()
    env.step()
    dev = env.device
    buf = dict(outcome=torch.full((E, K, NA), -3, dtype=torch.int16, device=dev),
               reward=torch.full((E, K, NA), -3.0, dtype=torch.float64, device=dev),
               crash9=torch.full((E, K), -3, dtype=torch.int16, device=dev),
               safe=torch.full((E, K), -3, dtype=torch.int16, device=dev),
               actions=torch.full((E, N), -3, dtype=torch.int32, device=dev))
    mask = env.out["mask"]
    stream = torch.cuda.Stream()
    args = (env.handle, None, None, mask.data_ptr(), buf["outcome"].data_ptr(), buf["reward"].data_ptr(),
            buf["crash9"].data_ptr(), buf["safe"].data_ptr(), buf["actions"].data_ptr())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        buf["actions"].fill_(-3)  # (so that the capture is not empty)
        first = env.lib.gw_step_preview(*args, stream.cuda_stream)  # it would have to allocate
    assert first == GW_ERR_STATE
    eager = {n: v.clone() for n, v in env.step_preview(mask=mask).items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        status = env.lib.gw_step_preview(*args, stream.cuda_stream)
    assert status == 0
    torch.cuda.synchronize()
    assert bool((buf["outcome"] == -3).all())  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    for got, name in ((buf["outcome"], "outcome"), (buf["reward"], "reward_alt"), (buf["crash9"], "crash9"),
                      (buf["safe"], "safe_mask"), (buf["actions"], "actions")):
        assert torch.equal(got, eager[name]), name
    env.close()


# ---- 5. the promise --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["level3", "n8_k2"])
def test_a_safe_pick_does_not_crash(name):
    case = R.CASES[R.CASE_IDS.index(name)]
    sc = R.scenario_of(case)
    E, K = 203, sc.K
    rng = np.random.default_rng(77)
    env = VecGridEnv(sc, num_envs=E, fear=False, seed=6, max_steps=1000, debug=True)
    dev = env.device
    zero = torch.zeros((E, K, NA), dtype=torch.float64, device=dev)
    probs = torch.as_tensor(rng.random((K, E, NA)).astype(np.float32)).to(dev)
    replaced = kept_subset = 0
    for agents in [1 << k for k in range(K)] + [(1 << K) - 1]:
        spawn, rl, scripted = R.clustered_spawn(sc, E, rng)
        mask = env.reset(spawn=torch.as_tensor(spawn))[1].clone()  # (the step below rewrites the env's own)
        rl_d = torch.as_tensor(rl).to(dev)
        pv = env.step_preview(rl_d, scripted, mask=mask)
        chosen, flags = env.fear_shield(zero, rl_d, mask=pv["safe_mask"], probs=probs, tau=0.0, agents=agents)
        r = env.step(chosen, scripted)
        torch.cuda.synchronize()
        avoidable = (mask.to(torch.int32) & ~pv["crash9"].to(torch.int32) & 0x1FF) != 0  # [E, K]
        kept = chosen == rl_d
        for k in range(K):
            if not (agents >> k) & 1:
                assert torch.equal(chosen[:, k], rl_d[:, k])
                continue
            others = [j for j in range(K) if j != k]
            sel = avoidable[:, k] & kept[:, others].all(1)  # one agent shielded: the others are all kept
            if agents == 1 << k:
                assert bool(kept[:, others].all())
            crashed = (r.crash_bits.to(torch.int32) >> k) & 1
            assert int(crashed[sel].sum()) == 0, (name, agents, k)  # exact, not statistical
            bad = (pv["crash9"][:, k].to(torch.int64) >> rl_d[:, k].long()) & 1
            assert bool((chosen[:, k] != rl_d[:, k])[(bad == 1) & avoidable[:, k]].all())  # crashing proposals go
            replaced += int((chosen[:, k] != rl_d[:, k]).sum())
            kept_subset += int(sel.sum())
    assert replaced > 0 and kept_subset > 0
    env.close()


# ---- 6. driver level -------------------------------------------------------------------------------------

def test_evaluate_with_the_crash_shield_equals_the_loop_by_hand():
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("level3")
    E, T = 256, 24
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    res = evaluate(actors, sc, episodes=E, max_steps=T, fear=False, seed=11, shield_crash=True, fused=False)
    for n in ("shield_crash_proposed", "shield_crash_replaced", "shield_replaced", "shield_stuck"):
        assert tuple(res[n].shape) == (sc.K,) and res[n].dtype == torch.int64, n
    assert bool((res["shield_crash_replaced"] <= res["shield_crash_proposed"]).all())
    assert bool((res["shield_crash_replaced"] <= res["shield_replaced"]).all())
    # the same actor -> preview -> shield -> step sequence on a VecGridEnv driven by hand
    env = VecGridEnv(sc, num_envs=E, fear=False, max_steps=T, auto_reset=False, seed=11, obs=True)
    obs, mask = env.reset()
    zero = torch.zeros((E, sc.K, NA), dtype=torch.float64, device=env.device)
    active = torch.ones(E, dtype=torch.bool, device=env.device)
    crashes = steps = 0
    for _ in range(T):
        actions, probs = actors.act(env.out["obs"], env.out["mask"], training=False)
        pv = env.step_preview(actions, None, mask=env.out["mask"], reward=False)
        chosen, _ = env.fear_shield(zero, actions, mask=pv["safe_mask"], probs=probs.contiguous(), tau=0.0)
        r = env.step(chosen)
        crashes += int(r.crashes[active].sum())
        steps += int(active.sum())
        active &= r.done == 0
    env.close()
    print(f"evaluate(shield_crash=True): crashes {res['crashes']} in {res['steps']} env-steps, crashing proposals "
          f"{res['shield_crash_proposed'].tolist()}, replaced {res['shield_crash_replaced'].tolist()}")
    assert res["steps"] == steps and res["crashes"] == crashes
    with pytest.raises(ValueError):
        evaluate(actors, sc, episodes=8, shield=0.0, shield_mode="joint", shield_crash=True)


def test_rollout_with_the_crash_shield():
    from marlnav.rollout import Rollout
    env = VecGridEnv("level3", num_envs=203, fear=True, max_steps=40, seed=42, stats=True)
    ro = Rollout(env, None, seed=42, shield_crash=True)  # the device-random policy, no FeAR shield: zero table
    ro.reset()
    rep = torch.zeros(env.K, dtype=torch.int64)
    bad_total = 0
    for _ in range(10):
        ro.step()
        f = ro.shield_flags.cpu().to(torch.int64)
        rep += (f & 1).sum(0)
        bad_total += int((ro.shield_crash9 != 0).sum())
    ro.fence()
    tot = ro.totals()
    torch.cuda.synchronize()
    assert torch.equal(tot["shield_replaced"], rep) and int(tot["shield_stuck"].sum()) == 0  # tau = 0 on a zero table
    assert bad_total > 0
    with pytest.raises(ValueError):
        Rollout(env, None, shield=0.0, shield_mode="joint", shield_crash=True)
    env.close()


# ---- 7. status codes, span, sims -------------------------------------------------------------------------

def test_status_codes_span_and_sim_count():
    E = 37
    env = VecGridEnv("level3", num_envs=E, fear=False, seed=3)
    K = env.K
    out = torch.zeros((E, K, NA), dtype=torch.int16, device=env.device)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda h, o: env.lib.gw_step_preview(h, None, None, None, o, None, None, None, None, s)  # noqa: E731
    assert call(env.handle, out.data_ptr()) == GW_ERR_STATE  # before the first reset
    with pytest.raises(_lib.GwError, match="before gw_reset"):
        env.step_preview()
    env.reset()
    assert call(None, out.data_ptr()) == GW_ERR_ARG
    assert call(env.handle, None) == GW_ERR_ARG
    ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
    env.count_sims(ctr)
    env.profile(True, reserve=8)
    a = env.step_preview()
    assert call(env.handle, out.data_ptr()) == 0  # every optional output NULL
    env.count_sims(None)
    torch.cuda.synchronize()
    assert int(ctr) == 2 * NA * K * E  # 9 K world updates per env and call
    assert torch.equal(out, a["outcome"])
    spans = env.profile_spans()
    assert spans[:, 0].tolist() == [GW_SPAN_STEP_PREVIEW] * 2 and bool((spans[:, 2] > spans[:, 1]).all())
    env.profile(False)
    b = env.step_preview(reward=False)
    assert "reward_alt" not in b and b["outcome"].data_ptr() == a["outcome"].data_ptr()  # allocated once, reused
    with pytest.raises(ValueError):
        env.step_preview(mask=torch.zeros((E, K), dtype=torch.int32, device=env.device))
    env.close()
