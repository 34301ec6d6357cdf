"""Two-step crash lookahead (gw_step_lookahead) and the lookahead shield.

1. Against the C oracle, exact integer equality: a VecGridEnv twin of tests/_step_lookahead_ref.reference_run (the
   oracle stepped twice per (e, k, a, b) on copies of its state; coverage proven on the CPU by
   tests/test_step_lookahead_cpu.py).  Before a handful of the run's steps (device-random proposals at the odd
   ones, auto-resets included) and after two clustered replayed resets every output equals the reference, crash9
   equals step_preview's, and the sim count is the reference's.
2. The promise through real steps on both kernel paths.  3. No side effects.  4. Graph capture.
5. The shield: evaluate(shield_lookahead=True) against the loop by hand; an agent moved off a trap action is not
   trapped at the next step; the ValueError cases.  6. Status codes, the span kind, the sim count."""
import numpy as np
import pytest
import torch

import _step_lookahead_ref as R
from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu
NA, ALL = 9, 0x1FF
GW_ERR_ARG, GW_ERR_STATE = -1, -4
GW_SPAN_STEP_LOOKAHEAD = 16
NAMES = ("crash2", "ends", "crash9", "trap9", "ahead_mask")


def _i64(t):
    return t.cpu().numpy().view(np.uint16).astype(np.int64)


# ---- 1. against the oracle -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.CASE_IDS)
def test_lookahead_equals_the_oracle(name):
    run = R.reference_run(name)
    case = run["case"]
    sc = R.scenario_of(case)
    E, K = case.E, sc.K
    env = VecGridEnv(sc, num_envs=E, fear=case.fear, fear_weight=-5.0, seed=case.seed, max_steps=case.max_steps,
                     variant=case.variant, debug=True)
    env.reset()
    ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
    done_steps = 0
    for c in run["comps"]:
        for rl in run["rl_steps"][done_steps:c["step"]]:
            env.step(rl)
        done_steps = c["step"]
        if c["spawn"] is not None:
            env.reset(spawn=torch.as_tensor(c["spawn"]))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(env.positions().cpu().numpy(), c["pos"], err_msg=f"{c['where']}: twins")
        mask_t = env.out["mask"]
        np.testing.assert_array_equal(mask_t.cpu().numpy().view(np.uint16), c["mask"], err_msg=c["where"])
        ctr.zero_()
        env.count_sims(ctr)
        la = env.step_lookahead(c["rl"], c["scripted"], mask=mask_t)
        env.count_sims(None)
        pv = env.step_preview(c["rl"], c["scripted"], mask=mask_t, reward=False)
        torch.cuda.synchronize()
        tab = c["tab"]
        trap9, _, ahead, sims = R.derived(tab, c["mask"])
        want = dict(crash2=tab["crash2"], ends=tab["ends"], crash9=tab["crash9"], trap9=trap9, ahead_mask=ahead)
        np.testing.assert_array_equal(la["actions"].cpu().numpy(), c["joint"], err_msg=f"{c['where']}: joint action")
        for n in NAMES:
            got = _i64(la[n])
            print(f"{c['where']}: {int((got != want[n]).sum())} of {got.size} {n} entries differ")
            np.testing.assert_array_equal(got, want[n], err_msg=f"{c['where']}: {n}")
        assert torch.equal(la["crash9"], pv["crash9"]), c["where"]
        assert int(ctr) == sims, (c["where"], int(ctr), sims)
    env.close()


# ---- 2. the promise through real steps -------------------------------------------------------------------

@pytest.mark.parametrize("path", ["defer", "merged"])
@pytest.mark.parametrize("name", ["level3", "n8_k2", "single_k1"])
def test_crash2_of_the_applied_action_is_the_next_crash9(name, path, monkeypatch):
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    monkeypatch.setenv("GW_KERNEL", path)
    case = R.CASES[R.CASE_IDS.index(name)]
    sc = R.scenario_of(case)
    E, K = 41, sc.K
    env = VecGridEnv(sc, num_envs=E, fear=case.fear, seed=5, max_steps=5, variant=case.variant, debug=True)
    assert env.kernel_path == path
    env.reset()
    gen = torch.Generator(device=env.device).manual_seed(17)
    ar = torch.arange(E, device=env.device)
    zeros = torch.zeros((E, K), dtype=torch.int32, device=env.device)
    crashes = dones = rows = compared = 0
    for t in range(12):
        rl = torch.randint(0, NA, (E, K), generator=gen, device=env.device, dtype=torch.int32) if t % 2 else None
        la = {n: v.clone() for n, v in env.step_lookahead(rl).items()}
        r = env.step(rl)
        done = r.done.clone().bool()
        assert torch.equal(la["actions"], r.actions), t
        nxt = env.step_preview(zeros, reward=False)["crash9"]
        torch.cuda.synchronize()
        for k in range(K):
            a = r.actions[:, k].long()
            assert torch.equal(((la["ends"][:, k].to(torch.int64) >> a) & 1).bool(), done), (t, k)
            assert torch.equal((la["crash9"][:, k].to(torch.int64) >> a) & 1,
                               (r.crash_bits.to(torch.int64) >> k) & 1), (t, k)
            assert torch.equal(la["crash2"][ar, k, a][~done], nxt[:, k][~done]), (t, k)
            rows += int((la["crash2"][ar, k, a][~done] != 0).sum())
            compared += int((~done).sum())
        crashes += int((r.crash_bits != 0).sum())
        dones += int(done.sum())
    assert crashes > 0 and dones >= E and rows > 0 and compared > 0
    env.close()


# ---- 3. no side effects ----------------------------------------------------------------------------------

def _trajectory(lookahead):
    env = VecGridEnv("level3", num_envs=37, fear=True, fear_weight=-5.0, seed=9, max_steps=6, debug=True)
    env.reset()
    steps = []
    for _ in range(20):
        if lookahead:
            before = {n: v.clone() for n, v in env.state().items()}
            env.step_lookahead(mask=env.out["mask"])
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


def test_lookahead_has_no_side_effects():
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
    i16 = dict(dtype=torch.int16, device=dev)
    buf = dict(crash2=torch.full((E, K, NA), -3, **i16), ends=torch.full((E, K), -3, **i16),
               crash9=torch.full((E, K), -3, **i16), trap9=torch.full((E, K), -3, **i16),
               ahead_mask=torch.full((E, K), -3, **i16), actions=torch.full((E, N), -3, dtype=torch.int32, device=dev))
    mask = env.out["mask"]
    stream = torch.cuda.Stream()
    args = (env.handle, None, None, mask.data_ptr()) + tuple(buf[n].data_ptr() for n in NAMES) + (
        buf["actions"].data_ptr(), None)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        buf["actions"].fill_(-3)  # (so that the capture is not empty)
        first = env.lib.gw_step_lookahead(*args, stream.cuda_stream)  # it would have to allocate
    assert first == GW_ERR_STATE
    env.step_lookahead(mask=mask)  # one eager call
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        status = env.lib.gw_step_lookahead(*args, stream.cuda_stream)
    assert status == 0
    torch.cuda.synchronize()
    assert bool((buf["crash2"] == -3).all())  # captured, not run
    for _ in range(3):  # the world moves on: the replay reads the state of its own time
        env.step()
    eager = {n: v.clone() for n, v in env.step_lookahead(mask=mask).items()}
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for n in NAMES + ("actions",):
        assert torch.equal(buf[n], eager[n]), n
    env.close()


# ---- 5. the shield ---------------------------------------------------------------------------------------

def test_evaluate_with_the_lookahead_shield_equals_the_loop_by_hand():
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("level3")
    E, T = 256, 24
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    res = evaluate(actors, sc, episodes=E, max_steps=T, fear=False, seed=11, shield_lookahead=True, fused=False)
    for n in ("shield_trap_proposed", "shield_trap_replaced", "shield_crash_proposed", "shield_crash_replaced",
              "shield_replaced", "shield_stuck"):
        assert tuple(res[n].shape) == (sc.K,) and res[n].dtype == torch.int64, n
    assert bool((res["shield_trap_replaced"] <= res["shield_trap_proposed"]).all())
    env = VecGridEnv(sc, num_envs=E, fear=False, max_steps=T, auto_reset=False, seed=11, obs=True)
    env.reset()
    zero = torch.zeros((E, sc.K, NA), dtype=torch.float64, device=env.device)
    active = torch.ones(E, dtype=torch.bool, device=env.device)
    crashes = steps = 0
    names = ("shield_trap_proposed", "shield_trap_replaced", "shield_crash_proposed", "shield_crash_replaced",
             "shield_replaced", "shield_stuck")
    hand = {n: torch.zeros(sc.K, dtype=torch.int64) for n in names}
    for _ in range(T):
        actions, probs = actors.act(env.out["obs"], env.out["mask"], training=False)
        la = env.step_lookahead(actions, None, mask=env.out["mask"])
        chosen, flags = env.fear_shield(zero, actions, mask=la["ahead_mask"], probs=probs.contiguous(), tau=0.0)
        on = active.to(torch.int64).unsqueeze(1)
        trap = (la["trap9"].to(torch.int64) >> actions.to(torch.int64)) & 1
        bad = (la["crash9"].to(torch.int64) >> actions.to(torch.int64)) & 1
        moved = (chosen != actions).to(torch.int64)
        for n, v in zip(names, (trap, trap * moved, bad, bad * moved, flags.to(torch.int64) & 1,
                                (flags.to(torch.int64) >> 1) & 1)):
            hand[n] += (v * on).sum(0).cpu()
        r = env.step(chosen)
        crashes += int(r.crashes[active].sum())
        steps += int(active.sum())
        active &= r.done == 0
    env.close()
    print(f"evaluate(shield_lookahead=True): crashes {res['crashes']} in {res['steps']} env-steps, trap proposals "
          f"{res['shield_trap_proposed'].tolist()}, replaced {res['shield_trap_replaced'].tolist()}")
    assert res["steps"] == steps and res["crashes"] == crashes
    for n in names:  # every count of Shield.apply against the same sums taken by hand
        assert torch.equal(res[n], hand[n]), (n, res[n].tolist(), hand[n].tolist())
    assert int(hand["shield_trap_proposed"].sum()) > 0 and int(hand["shield_trap_replaced"].sum()) > 0
    for mode in ("joint", "joint_crash"):
        with pytest.raises(ValueError, match="shield_lookahead"):
            evaluate(actors, sc, episodes=8, shield_mode=mode, shield_lookahead=True)


@pytest.mark.parametrize("name", ["level3", "n8_k2"])
def test_an_agent_moved_off_a_trap_is_not_trapped(name):
    """Exact, where the lookahead's one assumption holds: the others' actions were kept in the step, and no other
    RL agent moves in the step after (they all propose 0 there; K = 1 needs nothing)."""
    from marlnav.rollout import Rollout
    case = R.CASES[R.CASE_IDS.index(name)]
    sc = R.scenario_of(case)
    E, K = 203, sc.K
    rng = np.random.default_rng(78)
    env = VecGridEnv(sc, num_envs=E, fear=False, seed=6, max_steps=1000, debug=True)
    dev = env.device
    zero = torch.zeros((E, K, NA), dtype=torch.float64, device=dev)
    zeros = torch.zeros((E, K), dtype=torch.int32, device=dev)
    probs = torch.as_tensor(rng.random((K, E, NA)).astype(np.float32)).to(dev)
    moved_off = checked = 0
    for rnd in range(6):
        spawn, rl, scripted = R.clustered_spawn(sc, E, rng)
        mask = env.reset(spawn=torch.as_tensor(spawn))[1].clone()
        rl_d = torch.as_tensor(rl).to(dev)
        for k in range(K):  # one agent shielded at a time: the others are all kept
            if rnd % K != k:
                continue
            # k proposes its lowest trap action where it has one (its own proposal does not enter its own rows)
            t9 = env.step_lookahead(rl_d, scripted, mask=mask)["trap9"][:, k].to(torch.int64)
            low = torch.log2((t9 & -t9).clamp(min=1).to(torch.float64)).round().to(torch.int32)
            rl_d[:, k] = torch.where(t9 != 0, low, rl_d[:, k])
            la = {n: v.clone() for n, v in env.step_lookahead(rl_d, scripted, mask=mask).items()}
            assert torch.equal(la["trap9"][:, k].to(torch.int64), t9)
            chosen, _ = env.fear_shield(zero, rl_d, mask=la["ahead_mask"], probs=probs, tau=0.0, agents=1 << k)
            chosen = chosen.clone()
            was_trap = ((la["trap9"][:, k].to(torch.int64) >> rl_d[:, k].long()) & 1).bool()
            room = (mask[:, k].to(torch.int64) & ~la["crash9"][:, k].to(torch.int64)
                    & ~la["trap9"][:, k].to(torch.int64) & ALL) != 0
            sel = was_trap & room
            assert bool((chosen[:, k] != rl_d[:, k])[sel].all())  # a trap proposal goes where anything else is left
            r = env.step(chosen, scripted)
            alive = r.done.clone() == 0
            nxt = env.step_preview(zeros, reward=False)  # the next step, the RL agents proposing 0
            m2 = env.out["mask"][:, k].to(torch.int64) & ALL
            trapped_now = (m2 != 0) & ((m2 & ~nxt["crash9"][:, k].to(torch.int64)) == 0)
            torch.cuda.synchronize()
            assert int(trapped_now[sel & alive].sum()) == 0, (name, rnd, k)
            moved_off += int(sel.sum())
            checked += int((sel & alive).sum())
    print(f"{name}: {moved_off} agents moved off a trap action, {checked} checked at the next step")
    assert moved_off > 0 and checked > 0
    with pytest.raises(ValueError, match="shield_lookahead"):
        Rollout(env, None, shield_mode="joint_crash", shield_lookahead=True)
    env.close()


def test_rollout_with_the_lookahead_shield():
    from marlnav.rollout import Rollout
    env = VecGridEnv("level3", num_envs=203, fear=True, max_steps=40, seed=42, stats=True)
    ro = Rollout(env, None, seed=42, shield_lookahead=True)  # the device-random policy
    ro.reset()
    traps = 0
    for _ in range(10):
        ro.step()
        traps += int((ro.shield_trap9 != 0).sum())
    ro.fence()
    tot = ro.totals()
    torch.cuda.synchronize()
    assert traps > 0 and int(tot["shield_trap_proposed"].sum()) >= int(tot["shield_trap_replaced"].sum())
    assert int(tot["shield_stuck"].sum()) == 0
    env.close()


# ---- 6. status codes, span, sims -------------------------------------------------------------------------

def test_status_codes_span_and_sim_count():
    E = 37
    env = VecGridEnv("level3", num_envs=E, fear=False, seed=3)
    K = env.K
    out = torch.zeros((E, K, NA), dtype=torch.int16, device=env.device)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda h, o: env.lib.gw_step_lookahead(h, None, None, None, o, *[None] * 6, s)  # noqa: E731
    assert call(env.handle, out.data_ptr()) == GW_ERR_STATE  # before the first reset
    with pytest.raises(_lib.GwError, match="before gw_reset"):
        env.step_lookahead()
    env.reset()
    assert call(None, out.data_ptr()) == GW_ERR_ARG
    assert call(env.handle, out.data_ptr() + 1) == GW_ERR_ARG  # a u16 array at an odd address
    ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
    env.count_sims(ctr)
    env.profile(True, reserve=8)
    a = env.step_lookahead()
    assert call(env.handle, out.data_ptr()) == 0  # every other output NULL
    assert env.lib.gw_step_lookahead(env.handle, *[None] * 10, s) == 0  # every output NULL
    env.count_sims(None)
    torch.cuda.synchronize()
    goes_on = NA * K * E - int(sum(bin(int(v) & ALL).count("1") for v in a["ends"].flatten().tolist()))
    assert int(ctr) == 3 * (NA * K * E + NA * goes_on)
    assert torch.equal(out, a["crash2"])
    spans = env.profile_spans()
    assert spans[:, 0].tolist() == [GW_SPAN_STEP_LOOKAHEAD] * 3 and bool((spans[:, 2] > spans[:, 1]).all())
    env.profile(False)
    b = env.step_lookahead()
    assert b["crash2"].data_ptr() == a["crash2"].data_ptr()  # allocated once, reused
    with pytest.raises(ValueError):
        env.step_lookahead(mask=torch.zeros((E, K), dtype=torch.int32, device=env.device))
    env.close()
