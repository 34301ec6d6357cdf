"""Crash horizon (gw_step_horizon) and the horizon shield.

1. Against the C oracle, exact integer equality: a VecGridEnv twin of tests/_step_horizon_ref.reference_run (the
   oracle searched level by level on copies of its state; coverage and the equality with the plain depth-first
   search proven on the CPU by tests/test_step_horizon_cpu.py).  Before a handful of the run's steps (device-random
   proposals at the odd ones, auto-resets included) and after two clustered replayed resets every output equals the
   reference at H = 2, 3 and 4, and the sim count is the reference's.
2. H = 2 against step_lookahead_kernel.  3. The promise through real steps on both kernel paths (K = 1, where the
   stay assumption is exact).  4. No side effects.  5. Graph capture.  6. The shield: evaluate(shield_horizon=3)
   against the loop by hand; an agent moved off a doomed proposal has a viable action at the next step.
7. Status codes and the span kind."""
import numpy as np
import pytest
import torch

import _step_horizon_ref as R
from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu
NA, ALL = 9, 0x1FF
GW_ERR_ARG, GW_ERR_STATE = -1, -4
GW_SPAN_STEP_HORIZON, GW_HORIZON_MAX = 17, 4
NAMES = ("depth", "ends", "crash9", "viable9", "horizon_mask")


def _i64(t):
    a = t.cpu().numpy()
    return (a.view(np.uint16) if a.dtype == np.int16 else a).astype(np.int64)


def _twin(run, upto=None):
    """A VecGridEnv twin of the reference run and a generator of (comparison, env) with the env brought to the
    comparison's state (``upto``: stop after that comparison index)."""
    case = run["case"]
    sc = R.scenario_of(case)
    env = VecGridEnv(sc, num_envs=case.E, fear=case.fear, fear_weight=-5.0, seed=case.seed, max_steps=case.max_steps,
                     variant=case.variant, debug=True)
    env.reset()

    def walk():
        done_steps = 0
        for i, c in enumerate(run["comps"]):
            for rl in run["rl_steps"][done_steps:c["step"]]:
                env.step(rl)
            done_steps = c["step"]
            if c["spawn"] is not None:
                env.reset(spawn=torch.as_tensor(c["spawn"]))
            yield c
            if upto is not None and i == upto:
                return

    return env, walk()


# ---- 1. against the oracle -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.CASE_IDS)
def test_horizon_equals_the_oracle(name):
    run = R.reference_run(name)
    env, comps = _twin(run)
    ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
    for c in comps:
        torch.cuda.synchronize()
        np.testing.assert_array_equal(env.positions().cpu().numpy(), c["pos"], err_msg=f"{c['where']}: twins")
        mask_t = env.out["mask"]
        np.testing.assert_array_equal(mask_t.cpu().numpy().view(np.uint16), c["mask"], err_msg=c["where"])
        for H in R.HORIZONS:
            ctr.zero_()
            env.count_sims(ctr)
            hz = env.step_horizon(c["rl"], c["scripted"], mask=mask_t, horizon=H)
            env.count_sims(None)
            torch.cuda.synchronize()
            tab = c["tab"][H]
            viable9, hmask = R.derived(tab["depth"], c["mask"], H)
            want = dict(depth=tab["depth"], ends=tab["ends"], crash9=tab["crash9"], viable9=viable9, horizon_mask=hmask)
            np.testing.assert_array_equal(hz["actions"].cpu().numpy(), c["joint"], err_msg=f"{c['where']}: joint action")
            for n in NAMES:
                got = _i64(hz[n])
                print(f"{c['where']} H {H}: {int((got != want[n]).sum())} of {got.size} {n} entries differ")
                np.testing.assert_array_equal(got, want[n], err_msg=f"{c['where']} H {H}: {n}")
            assert int(ctr) == tab["sims"], (c["where"], H, int(ctr), tab["sims"])
            no_mask = env.step_horizon(c["rl"], c["scripted"], mask=None, horizon=H)["horizon_mask"]
            np.testing.assert_array_equal(_i64(no_mask), R.derived(tab["depth"], None, H)[1], err_msg=c["where"])
    env.close()


# ---- 2. H = 2 against the existing kernel ----------------------------------------------------------------

@pytest.mark.parametrize("name", ["level3", "n8_k2", "n5_k5", "open13x3_k1"])
def test_horizon_two_is_the_lookahead(name):
    env, comps = _twin(R.reference_run(name))
    traps = 0
    for c in comps:
        mask_t = env.out["mask"]
        la = {n: v.clone() for n, v in env.step_lookahead(c["rl"], c["scripted"], mask=mask_t).items()}
        hz = env.step_horizon(c["rl"], c["scripted"], mask=mask_t, horizon=2)
        torch.cuda.synchronize()
        bit = (1 << torch.arange(NA, device=env.device)).to(torch.int64)
        for d, n in ((1, "trap9"), (0, "crash9")):
            got = ((hz["depth"] == d).to(torch.int64) * bit).sum(-1)
            assert torch.equal(got, la[n].to(torch.int64) & 0xFFFF), (c["where"], n)
        assert torch.equal(hz["horizon_mask"], la["ahead_mask"]), c["where"]
        assert torch.equal(hz["ends"], la["ends"]) and torch.equal(hz["crash9"], la["crash9"]), c["where"]
        assert torch.equal(hz["actions"], la["actions"]), c["where"]
        traps += int((la["trap9"] != 0).sum())
    assert traps > 0 or name == "n5_k5"  # (N == K has no trap)
    env.close()


# ---- 3. the promise through real steps -------------------------------------------------------------------

# (the 13 x 3 map's H * W is no multiple of 4: its env has no merged path)
@pytest.mark.parametrize("name,path", [("single_k1", "defer"), ("single_k1", "merged"), ("open13x3_k1", "defer")])
def test_depth_holds_through_real_steps(name, path, monkeypatch):
    """K = 1: the stay assumption is exact.  In every env the agent is driven along the reference's path from a
    first action with depth == H (even envs, where one exists) or with 1 <= depth < H (odd envs): it does not
    crash on the path; at the end of a doomed path every action its cell allows is in step_preview's crash9."""
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    monkeypatch.setenv("GW_KERNEL", path)
    run = R.reference_run(name)
    sc = R.scenario_of(run["case"])
    amask = torch.as_tensor(np.asarray(sc.action_mask).astype(np.int64))
    E = run["case"].E
    survived = doomed_checked = 0
    for ci in (0, 1, len(run["comps"]) - 2, len(run["comps"]) - 1):
        for H in (3, 4):
            env, comps = _twin(run, upto=ci)
            assert env.kernel_path == path
            for c in comps:
                pass
            tab = c["tab"][H]
            depth, seqs, kinds = tab["depth"][:, 0], [], []
            for e in range(E):
                full = [a for a in range(NA) if depth[e, a] == H]
                short = [a for a in range(NA) if 1 <= depth[e, a] < H]
                pick = (full or short) if e % 2 == 0 else (short or full)
                if not pick:  # every first action crashes the agent: nothing to drive
                    seqs.append([])
                    kinds.append(H)
                    continue
                a = pick[0]
                seqs.append([a] + list(tab["paths"][e][0][a]))
                kinds.append(int(depth[e, a]))
                assert len(seqs[e]) <= kinds[e]  # (shorter only where the episode ends on the way)
            alive = np.array([len(q) > 0 for q in seqs])
            zeros = torch.zeros((E, 1), dtype=torch.int32, device=env.device)
            for i in range(H + 1):
                at_end = np.array([alive[e] and kinds[e] < H and i == kinds[e] and len(seqs[e]) == kinds[e] for e in range(E)])
                if at_end.any():
                    c9 = env.step_preview(zeros, reward=False)["crash9"][:, 0].to(torch.int64).cpu()
                    m = amask[env.positions()[:, 0].long().cpu()] & ALL
                    sel = torch.as_tensor(at_end)
                    assert bool((m[sel] != 0).all()) and bool(((m & ~c9)[sel] == 0).all()), (c["where"], H, i)
                    doomed_checked += int(at_end.sum())
                    alive &= ~at_end
                if i == H or not alive.any():
                    break
                act = np.array([[seqs[e][i] if alive[e] and i < len(seqs[e]) else 0] for e in range(E)], np.int32)
                alive &= np.array([i < len(seqs[e]) for e in range(E)])
                r = env.step(torch.as_tensor(act), c["scripted"] if i == 0 else None)
                torch.cuda.synchronize()
                crashed = ((r.crash_bits.cpu().numpy().astype(np.int64) & 1) != 0)
                assert not (crashed & alive).any(), (c["where"], H, i)
                alive &= r.done.cpu().numpy() == 0
                if i == H - 1:
                    survived += int(alive.sum())
            env.close()
    print(f"{name} on {path}: {survived} agents survived H steps, {doomed_checked} doomed agents checked")
    assert survived > 0 and doomed_checked > 0


# ---- 4. no side effects ----------------------------------------------------------------------------------

def _trajectory(horizon):
    env = VecGridEnv("level3", num_envs=37, fear=True, fear_weight=-5.0, seed=9, max_steps=6, debug=True)
    env.reset()
    steps = []
    for i in range(20):
        if horizon:
            before = {n: v.clone() for n, v in env.state().items()}
            env.step_horizon(mask=env.out["mask"], horizon=2 + i % 3)
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


def test_horizon_has_no_side_effects():
    (a, sa, ca), (b, sb, cb) = _trajectory(True), _trajectory(False)
    assert len(a) == len(b) == 20 and ca == cb
    for t, (x, y) in enumerate(zip(a, b)):
        for n in x:
            assert torch.equal(x[n], y[n]), (t, n)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n


# ---- 5. graph capture ------------------------------------------------------------------------------------

def test_graph_capture():
    env = VecGridEnv("level3", num_envs=37, fear=True, seed=4, debug=True)
    E, K, N = env.E, env.K, env.N
    env.reset()
    env.step()
    dev = env.device
    i16 = dict(dtype=torch.int16, device=dev)
    buf = dict(depth=torch.full((E, K, NA), 77, dtype=torch.uint8, device=dev), ends=torch.full((E, K), -3, **i16),
               crash9=torch.full((E, K), -3, **i16), viable9=torch.full((E, K), -3, **i16),
               horizon_mask=torch.full((E, K), -3, **i16), actions=torch.full((E, N), -3, dtype=torch.int32, device=dev))
    mask = env.out["mask"]
    stream = torch.cuda.Stream()
    args = (env.handle, None, None, mask.data_ptr(), 4) + tuple(buf[n].data_ptr() for n in NAMES) + (
        buf["actions"].data_ptr(), None)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        buf["actions"].fill_(-3)  # (so that the capture is not empty)
        first = env.lib.gw_step_horizon(*args, stream.cuda_stream)  # it would have to allocate
    assert first == GW_ERR_STATE
    env.step_horizon(mask=mask, horizon=4)  # one eager call
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        status = env.lib.gw_step_horizon(*args, stream.cuda_stream)
    assert status == 0
    torch.cuda.synchronize()
    assert bool((buf["depth"] == 77).all())  # captured, not run
    for _ in range(3):  # the world moves on: the replay reads the state of its own time
        env.step()
    eager = {n: v.clone() for n, v in env.step_horizon(mask=mask, horizon=4).items()}
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for n in NAMES + ("actions",):
        assert torch.equal(buf[n], eager[n]), n
    env.close()


# ---- 6. the shield ---------------------------------------------------------------------------------------

def test_evaluate_with_the_horizon_shield_equals_the_loop_by_hand():
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("level3")
    E, T, H = 256, 24, 3
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    res = evaluate(actors, sc, episodes=E, max_steps=T, fear=False, seed=11, shield_horizon=H, fused=False)
    names = ("shield_doomed_proposed", "shield_doomed_replaced", "shield_no_viable", "shield_crash_proposed",
             "shield_crash_replaced", "shield_replaced", "shield_stuck")
    for n in names:
        assert tuple(res[n].shape) == (sc.K,) and res[n].dtype == torch.int64, n
    assert "shield_trap_proposed" not in res
    env = VecGridEnv(sc, num_envs=E, fear=False, max_steps=T, auto_reset=False, seed=11, obs=True)
    env.reset()
    zero = torch.zeros((E, sc.K, NA), dtype=torch.float64, device=env.device)
    active = torch.ones(E, dtype=torch.bool, device=env.device)
    crashes = steps = agent_steps = 0
    hand = {n: torch.zeros(sc.K, dtype=torch.int64) for n in names}
    for _ in range(T):
        actions, probs = actors.act(env.out["obs"], env.out["mask"], training=False)
        m = env.out["mask"].to(torch.int64) & ALL
        hz = env.step_horizon(actions, None, mask=env.out["mask"], horizon=H)
        chosen, flags = env.fear_shield(zero, actions, mask=hz["horizon_mask"], probs=probs.contiguous(), tau=0.0)
        on = active.to(torch.int64).unsqueeze(1)
        a64 = actions.to(torch.int64)
        some = ((hz["viable9"].to(torch.int64) & m) != 0).to(torch.int64)
        doomed = (hz["depth"].gather(2, a64.unsqueeze(2)).squeeze(2) < H).to(torch.int64) * some
        bad = (hz["crash9"].to(torch.int64) >> a64) & 1
        moved = (chosen != actions).to(torch.int64)
        for n, v in zip(names, (doomed, doomed * moved, 1 - some, bad, bad * moved, flags.to(torch.int64) & 1,
                                (flags.to(torch.int64) >> 1) & 1)):
            hand[n] += (v * on).sum(0).cpu()
        agent_steps += int(active.sum())
        r = env.step(chosen)
        crashes += int(r.crashes[active].sum())
        steps += int(active.sum())
        active &= r.done == 0
    env.close()
    print(f"evaluate(shield_horizon={H}): crashes {res['crashes']} in {res['steps']} env-steps, doomed proposals "
          f"{res['shield_doomed_proposed'].tolist()}, replaced {res['shield_doomed_replaced'].tolist()}, no viable "
          f"action {res['shield_no_viable'].tolist()}")
    assert res["steps"] == steps and res["crashes"] == crashes
    for n in names:  # every count of Shield.apply against the same sums taken by hand
        assert torch.equal(res[n], hand[n]), (n, res[n].tolist(), hand[n].tolist())
    # the counters add up: replaced doomed proposals are doomed proposals, crashing proposals with a viable
    # alternative are doomed, and doomed + no-viable agent-steps are agent-steps
    assert bool((hand["shield_doomed_replaced"] <= hand["shield_doomed_proposed"]).all())
    assert bool((hand["shield_doomed_proposed"] + hand["shield_no_viable"] <= agent_steps).all())
    assert int(hand["shield_doomed_proposed"].sum()) > 0 and int(hand["shield_doomed_replaced"].sum()) > 0
    for mode in ("joint", "joint_crash"):
        with pytest.raises(ValueError, match="shield_horizon"):
            evaluate(actors, sc, episodes=8, shield_mode=mode, shield_horizon=3)
    with pytest.raises(ValueError, match="shield_horizon"):
        evaluate(actors, sc, episodes=8, shield_lookahead=True, shield_horizon=3)


@pytest.mark.parametrize("name", ["level3", "n8_k2"])
def test_an_agent_moved_off_a_doomed_proposal_has_a_viable_action(name):
    """Exact, where the horizon's one assumption holds: the others' actions were kept in the step, and no other RL
    agent moves in the steps after (they all propose 0 at the next step).  An action of depth 3 at H = 3 leaves the
    agent, one step later, with an allowed action of depth 2 at H = 2."""
    from marlnav.rollout import Rollout
    case = R.CASES[R.CASE_IDS.index(name)]
    sc = R.scenario_of(case)
    E, K, H = 203, sc.K, 3
    rng = np.random.default_rng(78)
    env = VecGridEnv(sc, num_envs=E, fear=False, seed=6, max_steps=1000, debug=True)
    dev = env.device
    zero = torch.zeros((E, K, NA), dtype=torch.float64, device=dev)
    zeros = torch.zeros((E, K), dtype=torch.int32, device=dev)
    probs = torch.as_tensor(rng.random((K, E, NA)).astype(np.float32)).to(dev)
    bit = (1 << torch.arange(NA, device=dev)).to(torch.int64)
    moved_off = checked = 0
    for rnd in range(6):
        spawn, rl, scripted = R.clustered_spawn(sc, E, rng)
        mask = env.reset(spawn=torch.as_tensor(spawn))[1].clone()
        rl_d = torch.as_tensor(rl).to(dev)
        k = rnd % K  # one agent shielded at a time: the others are all kept
        # k proposes its lowest doomed action where it has one (its own proposal does not enter its own rows)
        d0 = env.step_horizon(rl_d, scripted, mask=mask, horizon=H)["depth"][:, k]
        low9 = ((d0 < H).to(torch.int64) * bit).sum(-1) & mask[:, k].to(torch.int64)
        low = torch.log2((low9 & -low9).clamp(min=1).to(torch.float64)).round().to(torch.int32)
        rl_d[:, k] = torch.where(low9 != 0, low, rl_d[:, k])
        hz = {n: v.clone() for n, v in env.step_horizon(rl_d, scripted, mask=mask, horizon=H).items()}
        assert torch.equal(hz["depth"][:, k], d0)
        chosen, _ = env.fear_shield(zero, rl_d, mask=hz["horizon_mask"], probs=probs, tau=0.0, agents=1 << k)
        chosen = chosen.clone()
        was_doomed = ((hz["viable9"][:, k].to(torch.int64) >> rl_d[:, k].long()) & 1) == 0
        room = (mask[:, k].to(torch.int64) & hz["viable9"][:, k].to(torch.int64) & ALL) != 0
        sel = was_doomed & room
        assert bool((chosen[:, k] != rl_d[:, k])[sel].all())  # a doomed proposal goes where a viable action is left
        assert bool((((hz["viable9"][:, k].to(torch.int64) >> chosen[:, k].long()) & 1) == 1)[sel].all())
        r = env.step(chosen, scripted)
        alive = r.done.clone() == 0
        m2 = env.out["mask"][:, k].to(torch.int64) & ALL
        nxt = env.step_horizon(zeros, None, mask=env.out["mask"], horizon=H - 1)  # the RL agents proposing 0
        ok = (m2 == 0) | ((nxt["viable9"][:, k].to(torch.int64) & m2) != 0)
        torch.cuda.synchronize()
        assert bool(ok[sel & alive].all()), (name, rnd, k)
        moved_off += int(sel.sum())
        checked += int((sel & alive).sum())
    print(f"{name}: {moved_off} agents moved off a doomed proposal, {checked} checked at the next step")
    assert moved_off > 0 and checked > 0
    with pytest.raises(ValueError, match="shield_horizon"):
        Rollout(env, None, shield_mode="joint_crash", shield_horizon=3)
    env.close()


def test_rollout_with_the_horizon_shield():
    from marlnav.rollout import Rollout
    env = VecGridEnv("level3", num_envs=203, fear=True, max_steps=40, seed=42, stats=True)
    ro = Rollout(env, None, seed=42, shield_horizon=4)  # the device-random policy
    ro.reset()
    short = 0
    for _ in range(10):
        ro.step()
        short += int((ro.shield_depth < 4).sum())
        assert ro.shield_viable9 is not None
    ro.fence()
    tot = ro.totals()
    torch.cuda.synchronize()
    assert short > 0 and int(tot["shield_doomed_proposed"].sum()) >= int(tot["shield_doomed_replaced"].sum()) > 0
    assert int(tot["shield_stuck"].sum()) == 0
    env.close()


# ---- 7. status codes, span -------------------------------------------------------------------------------

def test_status_codes_and_span():
    E = 37
    env = VecGridEnv("level3", num_envs=E, fear=False, seed=3)
    K = env.K
    out = torch.zeros((E, K, NA), dtype=torch.uint8, device=env.device)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda h, H, o: env.lib.gw_step_horizon(h, None, None, None, H, o, *[None] * 6, s)  # noqa: E731
    assert call(env.handle, 3, out.data_ptr()) == GW_ERR_STATE  # before the first reset
    with pytest.raises(_lib.GwError, match="before gw_reset"):
        env.step_horizon()
    env.reset()
    assert call(None, 3, out.data_ptr()) == GW_ERR_ARG
    for H in (1, GW_HORIZON_MAX + 1, 0, -1):
        assert call(env.handle, H, out.data_ptr()) == GW_ERR_ARG, H
        with pytest.raises(ValueError, match="horizon"):
            env.step_horizon(horizon=H)
    u16 = torch.zeros((E, K + 1), dtype=torch.int16, device=env.device)
    assert env.lib.gw_step_horizon(env.handle, None, None, None, 3, None, u16.data_ptr() + 1, *[None] * 5, s) == GW_ERR_ARG
    env.profile(True, reserve=8)
    a = env.step_horizon(horizon=3)
    assert call(env.handle, 3, out.data_ptr()) == 0  # every other output NULL
    assert env.lib.gw_step_horizon(env.handle, None, None, None, 4, *[None] * 7, s) == 0  # every output NULL
    torch.cuda.synchronize()
    assert torch.equal(out, a["depth"]) and int(a["depth"].max()) <= 3
    spans = env.profile_spans()
    assert spans[:, 0].tolist() == [GW_SPAN_STEP_HORIZON] * 3 and bool((spans[:, 2] > spans[:, 1]).all())
    env.profile(False)
    b = env.step_horizon(horizon=3)
    assert b["depth"].data_ptr() == a["depth"].data_ptr()  # allocated once, reused
    with pytest.raises(ValueError):
        env.step_horizon(mask=torch.zeros((E, K), dtype=torch.int32, device=env.device))
    env.close()
