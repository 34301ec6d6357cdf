"""Reward horizon (gw_step_plan) and the plan shield.

1. Against the C oracle, exact integer equality: a VecGridEnv twin of tests/_step_plan_ref.reference_run (the
   oracle searched level by level on copies of its state with its apples left as they are; coverage and the
   equality with the plain depth-first search proven on the CPU by tests/test_step_plan_cpu.py).  Before a handful
   of the run's steps and after the replayed resets (clustered, near apple, last apple) every output equals the
   reference at H = 2, 3 and 4, and the sim count is the reference's.
2. ends / crash9 against step_horizon_kernel and step_preview_kernel.  3. ret of a first action that crashes the
   agent or ends the episode is round(10 * reward_alt).  4. The promise through real steps on both kernel paths
   (K = 1, where the stay assumption is exact), each in a child process.  5. No side effects.  6. Graph capture.
7. The shield: evaluate(shield_plan=3) against the loop by hand, and the policy-free planner.  8. Status codes and
   the span kind."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _step_plan_ref as P
from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu
NA, ALL = 9, 0x1FF
GW_ERR_ARG, GW_ERR_STATE = -1, -4
GW_SPAN_STEP_PLAN, GW_HORIZON_MAX = 18, 4
NAMES = ("depth", "ret", "path", "ends", "crash9", "plan_mask")


def _i64(t):
    return t.cpu().numpy().astype(np.int64)


def _u16(t):
    return t.cpu().numpy().view(np.uint16).astype(np.int64)


def _twin(run, upto=None):
    """A VecGridEnv twin of the reference run and a generator of (comparison, env) with the env brought to the
    comparison's state by the run's own ops (``upto``: stop after that comparison index)."""
    case = run["case"]
    sc = P.scenario_of(case)
    env = VecGridEnv(sc, num_envs=case.E, fear=case.fear, fear_weight=-5.0, seed=case.seed, max_steps=case.max_steps,
                     variant=case.variant, debug=True)
    env.reset()

    def walk():
        i = 0
        for op in run["ops"]:
            if op["op"] == "step":
                env.step(op["rl"], op["scripted"])
            elif op["op"] == "reset":
                env.reset(spawn=torch.as_tensor(op["spawn"]))
            else:
                yield op
                if upto is not None and i == upto:
                    return
                i += 1

    return env, walk()


# ---- 1. against the oracle -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.CASE_IDS)
def test_plan_equals_the_oracle(name):
    run = P.reference_run(name)
    env, comps = _twin(run)
    ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
    for c in comps:
        torch.cuda.synchronize()
        np.testing.assert_array_equal(env.positions().cpu().numpy(), c["pos"], err_msg=f"{c['where']}: twins")
        mask_t = env.out["mask"]
        np.testing.assert_array_equal(mask_t.cpu().numpy().view(np.uint16), c["mask"], err_msg=c["where"])
        for H in P.HORIZONS:
            ctr.zero_()
            env.count_sims(ctr)
            pl = env.step_plan(c["rl"], c["scripted"], mask=mask_t, horizon=H)
            env.count_sims(None)
            torch.cuda.synchronize()
            tab = c["tab"][H]
            want = dict(depth=tab["depth"], ret=tab["ret"], path=tab["path"], ends=tab["ends"], crash9=tab["crash9"],
                        plan_mask=P.plan_mask(tab["depth"], tab["ret"], c["mask"]))
            np.testing.assert_array_equal(pl["actions"].cpu().numpy(), c["joint"], err_msg=f"{c['where']}: joint action")
            for n in NAMES:
                got = _i64(pl[n]) if n in ("depth", "ret", "path") else _u16(pl[n])
                print(f"{c['where']} H {H}: {int((got != want[n]).sum())} of {got.size} {n} entries differ")
                np.testing.assert_array_equal(got, want[n], err_msg=f"{c['where']} H {H}: {n}")
            assert int(ctr) == tab["sims"], (c["where"], H, int(ctr), tab["sims"])
            no_mask = env.step_plan(c["rl"], c["scripted"], mask=None, horizon=H)["plan_mask"]
            np.testing.assert_array_equal(_u16(no_mask), P.plan_mask(tab["depth"], tab["ret"], None), err_msg=c["where"])
    env.close()


# ---- 2., 3. against the existing kernels -----------------------------------------------------------------

@pytest.mark.parametrize("name", ["level3", "n8_k2", "single_k1", "open13x3_k1"])
def test_first_step_is_the_previews(name):
    env, comps = _twin(P.reference_run(name))
    ended = 0
    for c in comps:
        mask_t = env.out["mask"]
        sp = {n: v.clone() for n, v in env.step_preview(c["rl"], c["scripted"], mask=mask_t).items()}
        for H in P.HORIZONS:
            hz = {n: v.clone() for n, v in env.step_horizon(c["rl"], c["scripted"], mask=mask_t, horizon=H).items()}
            pl = env.step_plan(c["rl"], c["scripted"], mask=mask_t, horizon=H)
            torch.cuda.synchronize()
            assert torch.equal(pl["ends"], hz["ends"]) and torch.equal(pl["crash9"], hz["crash9"]), c["where"]
            assert torch.equal(pl["crash9"], sp["crash9"]) and torch.equal(pl["actions"], hz["actions"]), c["where"]
            assert bool((pl["depth"] >= hz["depth"]).all()), c["where"]  # the apples only add episode ends
            # a first action that crashes the agent or ends the episode: its return is the step's reward
            bit = torch.arange(NA, device=env.device)
            over = (((pl["ends"].to(torch.int64) | pl["crash9"].to(torch.int64)).unsqueeze(-1) >> bit) & 1) == 1
            want = torch.round(sp["reward_alt"] * 10.0).to(torch.int16)
            assert torch.equal(pl["ret"][over], want[over]), (c["where"], H)
            assert bool((pl["path"][over] == 0xFF).all()), (c["where"], H)
            ended += int(over.sum())
    assert ended > 0
    env.close()


# ---- 4. the promise through real steps -------------------------------------------------------------------

def _promise(name, path):
    """K = 1: the stay assumption is exact.  In every env the agent plays a first action a (a different one per env
    and round) and then path[e, 0, a] through env.step: it survives exactly depth steps (its crash, if depth < H,
    comes at step depth + 1, the path's last entry; the episode ends no earlier than the path does), and the sum
    of out["reward"] times 10 over those steps equals ret."""
    run = P.reference_run(name)
    E = run["case"].E
    n_comps = len(run["comps"])
    checked = short = ate = 0
    for ci in (0, n_comps - 2, n_comps - 1):
        for H in (3, 4):
            for off in (0, 4):
                env, comps = _twin(run, upto=ci)
                assert env.kernel_path == path, (env.kernel_path, path)
                for c in comps:
                    pass
                pl = env.step_plan(c["rl"], c["scripted"], mask=env.out["mask"], horizon=H)
                torch.cuda.synchronize()
                first = (np.arange(E) + off) % NA
                depth = pl["depth"].cpu().numpy().astype(np.int64)[np.arange(E), 0, first]
                ret = pl["ret"].cpu().numpy().astype(np.int64)[np.arange(E), 0, first]
                pth = pl["path"].cpu().numpy().astype(np.int64)[np.arange(E), 0, first]
                seqs = [[int(first[e])] + [int(b) for b in pth[e] if b != 0xFF] for e in range(E)]
                total = np.zeros(E, np.int64)
                for i in range(H):
                    playing = np.array([i < len(q) for q in seqs])
                    if not playing.any():
                        break
                    act = np.array([[seqs[e][i] if playing[e] else 0] for e in range(E)], np.int32)
                    r = env.step(torch.as_tensor(act), c["scripted"] if i == 0 else None)
                    torch.cuda.synchronize()
                    crashed = (r.crash_bits.cpu().numpy().astype(np.int64) & 1) != 0
                    done = r.done.cpu().numpy() != 0
                    total += np.where(playing, np.round(r.reward.cpu().numpy()[:, 0] * 10.0).astype(np.int64), 0)
                    is_last = np.array([i == len(q) - 1 for q in seqs])
                    # the crash comes at step depth + 1 and nowhere else; nothing ends before the path does
                    assert (crashed[playing] == ((depth == i) & (depth < H))[playing]).all(), (c["where"], H, off, i)
                    assert not (done & playing & ~is_last).any(), (c["where"], H, off, i)
                    ate += int((playing & (r.apples.cpu().numpy() > 0) & (i > 0)).sum())
                lens = np.array([len(q) for q in seqs])
                assert (lens[depth < H] == depth[depth < H] + 1).all(), (c["where"], H, off)
                np.testing.assert_array_equal(total, ret, err_msg=f"{c['where']} H {H} off {off}")
                checked += E
                short += int((depth < H).sum())
                env.close()
    print(f"promise {name} on {path}: {checked} continuations, {short} below H, {ate} apples at a step >= 2")
    assert checked > 0 and short > 0 and ate > 0


# (the 13 x 3 map's H * W is no multiple of 4: its env has no merged path)
@pytest.mark.parametrize("name,path", [("single_k1", "defer"), ("single_k1", "merged"), ("open13x3_k1", "defer")])
def test_depth_and_return_hold_through_real_steps(name, path):
    env = dict(os.environ, GW_KERNEL=path, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    env.pop("GW_FEAR_BE", None)
    code = f"import test_gpu_step_plan as T; T._promise({name!r}, {path!r})"
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], env=env, cwd=os.path.dirname(os.path.abspath(__file__)),
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert f"promise {name} on {path}" in r.stdout


# ---- 5. no side effects ----------------------------------------------------------------------------------

def _trajectory(plan):
    env = VecGridEnv("level3", num_envs=37, fear=True, fear_weight=-5.0, seed=9, max_steps=6, debug=True)
    env.reset()
    steps = []
    for i in range(20):
        if plan:
            before = {n: v.clone() for n, v in env.state().items()}
            env.step_plan(mask=env.out["mask"], horizon=2 + i % 3)
            after = env.state()
            torch.cuda.synchronize()
            for n in before:  # positions, flags, t, episode, prev_dist, scores
                assert torch.equal(before[n], after[n]), n
        r = env.step()
        torch.cuda.synchronize()
        steps.append({n: getattr(r, n).clone() for n in ("obs", "reward", "fear", "shaped", "done", "term", "trunc",
                                                          "mask", "final_pos", "ep_return")})
    st, counts = env.state(), env.obs_delta_counts()
    torch.cuda.synchronize()
    env.close()
    return steps, st, counts


def test_plan_has_no_side_effects():
    (a, sa, ca), (b, sb, cb) = _trajectory(True), _trajectory(False)
    assert len(a) == len(b) == 20 and ca == cb
    for t, (x, y) in enumerate(zip(a, b)):
        for n in x:
            assert torch.equal(x[n], y[n]), (t, n)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n


# ---- 6. graph capture ------------------------------------------------------------------------------------

def test_graph_capture():
    env = VecGridEnv("level3", num_envs=37, fear=True, seed=4, debug=True)
    E, K, N = env.E, env.K, env.N
    env.reset()
    env.step()
    dev = env.device
    i16 = dict(dtype=torch.int16, device=dev)
    buf = dict(depth=torch.full((E, K, NA), 77, dtype=torch.uint8, device=dev), ret=torch.full((E, K, NA), -3, **i16),
               path=torch.full((E, K, NA, 3), 77, dtype=torch.uint8, device=dev), ends=torch.full((E, K), -3, **i16),
               crash9=torch.full((E, K), -3, **i16), plan_mask=torch.full((E, K), -3, **i16),
               actions=torch.full((E, N), -3, dtype=torch.int32, device=dev))
    mask = env.out["mask"]
    stream = torch.cuda.Stream()
    args = (env.handle, None, None, mask.data_ptr(), 4) + tuple(buf[n].data_ptr() for n in NAMES) + (
        buf["actions"].data_ptr(), None)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        buf["actions"].fill_(-3)  # (so that the capture is not empty)
        first = env.lib.gw_step_plan(*args, stream.cuda_stream)  # it would have to allocate
    assert first == GW_ERR_STATE
    env.step_plan(mask=mask, horizon=4)  # one eager call
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        status = env.lib.gw_step_plan(*args, stream.cuda_stream)
    assert status == 0
    torch.cuda.synchronize()
    assert bool((buf["depth"] == 77).all())  # captured, not run
    for _ in range(3):  # the world moves on: the replay reads the state of its own time
        env.step()
    eager = {n: v.clone() for n, v in env.step_plan(mask=mask, horizon=4).items()}
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for n in NAMES + ("actions",):
        assert torch.equal(buf[n], eager[n]), n
    env.close()


# ---- 7. the shield ---------------------------------------------------------------------------------------

def test_evaluate_with_the_plan_shield_equals_the_loop_by_hand():
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("level3")
    E, T, H = 256, 24, 3
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    res = evaluate(actors, sc, episodes=E, max_steps=T, fear=False, seed=11, shield_plan=H, fused=False)
    names = ("shield_plan_proposed_off", "shield_plan_replaced", "shield_crash_proposed", "shield_crash_replaced",
             "shield_replaced", "shield_stuck")
    for n in names:
        assert tuple(res[n].shape) == (sc.K,) and res[n].dtype == torch.int64, n
    assert "shield_doomed_proposed" not in res and "shield_trap_proposed" not in res
    env = VecGridEnv(sc, num_envs=E, fear=False, max_steps=T, auto_reset=False, seed=11, obs=True)
    env.reset()
    zero = torch.zeros((E, sc.K, NA), dtype=torch.float64, device=env.device)
    active = torch.ones(E, dtype=torch.bool, device=env.device)
    crashes = apples = steps = agent_steps = 0
    hand = {n: torch.zeros(sc.K, dtype=torch.int64) for n in names}
    for _ in range(T):
        actions, probs = actors.act(env.out["obs"], env.out["mask"], training=False)
        pl = env.step_plan(actions, None, mask=env.out["mask"], horizon=H)
        chosen, flags = env.fear_shield(zero, actions, mask=pl["plan_mask"], probs=probs.contiguous(), tau=0.0)
        on = active.to(torch.int64).unsqueeze(1)
        a64 = actions.to(torch.int64)
        off = 1 - ((pl["plan_mask"].to(torch.int64) >> a64) & 1)
        bad = (pl["crash9"].to(torch.int64) >> a64) & 1
        moved = (chosen != actions).to(torch.int64)
        for n, v in zip(names, (off, off * moved, bad, bad * moved, flags.to(torch.int64) & 1,
                                (flags.to(torch.int64) >> 1) & 1)):
            hand[n] += (v * on).sum(0).cpu()
        agent_steps += int(active.sum())
        r = env.step(chosen)
        crashes += int(r.crashes[active].sum())
        apples += int(r.apples[active].sum())
        steps += int(active.sum())
        active &= r.done == 0
    env.close()
    print(f"evaluate(shield_plan={H}): crashes {res['crashes']}, apples {res['apples_caught']} in {res['steps']} env-steps, "
          f"proposals off the plan mask {res['shield_plan_proposed_off'].tolist()}, replaced "
          f"{res['shield_plan_replaced'].tolist()}")
    assert res["steps"] == steps and res["crashes"] == crashes and res["apples_caught"] == apples
    for n in names:  # every count of Shield.apply against the same sums taken by hand
        assert torch.equal(res[n], hand[n]), (n, res[n].tolist(), hand[n].tolist())
    # the counters add up: a proposal off a non-empty plan mask is replaced by an action of it, a kept proposal
    # was on it; a crashing proposal with a crash-free masked action is off the mask
    assert torch.equal(hand["shield_plan_replaced"], hand["shield_replaced"])
    assert bool((hand["shield_plan_replaced"] <= hand["shield_plan_proposed_off"]).all())
    assert bool((hand["shield_plan_proposed_off"] <= agent_steps).all())
    assert bool((hand["shield_crash_replaced"] <= hand["shield_plan_replaced"]).all())
    assert int(hand["shield_plan_proposed_off"].sum()) > 0 and int(hand["shield_plan_replaced"].sum()) > 0
    for mode in ("joint", "joint_crash"):
        with pytest.raises(ValueError, match="shield_plan"):
            evaluate(actors, sc, episodes=8, shield_mode=mode, shield_plan=3)
    with pytest.raises(ValueError, match="shield_plan"):
        evaluate(actors, sc, episodes=8, shield_horizon=3, shield_plan=3)


def test_the_policy_free_planner_and_the_rollout_keyword():
    """evaluate(None, shield_plan=H): every RL agent proposes 0 and takes the lowest action of its plan mask.  Against
    the same loop by hand; the planner catches apples, which staying never does."""
    from marlnav.evaluate import evaluate
    from marlnav.rollout import Rollout
    sc = S.builtin("level3")
    E, T, H = 128, 16, 4
    res = evaluate(None, sc, episodes=E, max_steps=T, fear=False, seed=3, shield_plan=H)
    env = VecGridEnv(sc, num_envs=E, fear=False, max_steps=T, auto_reset=False, seed=3, obs=False)
    env.reset()
    stay = torch.zeros((E, sc.K), dtype=torch.int32, device=env.device)
    active = torch.ones(E, dtype=torch.bool, device=env.device)
    crashes = apples = steps = 0
    for _ in range(T):
        pm = env.step_plan(stay, None, mask=env.out["mask"], horizon=H)["plan_mask"].to(torch.int64) & ALL
        low = torch.log2((pm & -pm).clamp(min=1).to(torch.float64)).round().to(torch.int32)  # its lowest action
        keep = ((pm & 1) == 1) | (pm == 0)
        r = env.step(torch.where(keep, stay, low))
        crashes += int(r.crashes[active].sum())
        apples += int(r.apples[active].sum())
        steps += int(active.sum())
        active &= r.done == 0
    env.close()
    print(f"planner H = {H}: {res['apples_caught']} apples, {res['crashes']} crashes in {res['steps']} env-steps")
    assert (res["steps"], res["crashes"], res["apples_caught"]) == (steps, crashes, apples)
    assert res["apples_caught"] > 0
    env = VecGridEnv("level3", num_envs=203, fear=True, max_steps=40, seed=42, stats=True)
    ro = Rollout(env, None, seed=42, shield_plan=3)  # the device-random policy
    ro.reset()
    for _ in range(10):
        ro.step()
        assert ro.shield_ret is not None and ro.shield_plan_mask is not None and ro.shield_depth is not None
    ro.fence()
    tot = ro.totals()
    torch.cuda.synchronize()
    assert int(tot["shield_plan_proposed_off"].sum()) >= int(tot["shield_plan_replaced"].sum()) > 0
    assert int(tot["shield_stuck"].sum()) == 0
    with pytest.raises(ValueError, match="shield_plan"):
        Rollout(env, None, shield_mode="joint_crash", shield_plan=3)
    env.close()


# ---- 8. status codes, span -------------------------------------------------------------------------------

def test_status_codes_and_span():
    E = 37
    env = VecGridEnv("level3", num_envs=E, fear=False, seed=3)
    K = env.K
    out = torch.zeros((E, K, NA), dtype=torch.uint8, device=env.device)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda h, H, o: env.lib.gw_step_plan(h, None, None, None, H, o, *[None] * 7, s)  # noqa: E731
    assert call(env.handle, 3, out.data_ptr()) == GW_ERR_STATE  # before the first reset
    with pytest.raises(_lib.GwError, match="before gw_reset"):
        env.step_plan()
    env.reset()
    assert call(None, 3, out.data_ptr()) == GW_ERR_ARG
    for H in (1, GW_HORIZON_MAX + 1, 0, -1):
        assert call(env.handle, H, out.data_ptr()) == GW_ERR_ARG, H
        with pytest.raises(ValueError, match="horizon"):
            env.step_plan(horizon=H)
    u16 = torch.zeros((E, K * NA + 1), dtype=torch.int16, device=env.device)
    for slot in (1, 3, 4, 5):  # ret, ends, crash9, plan_mask
        ptrs = [None] * 6
        ptrs[slot] = u16.data_ptr() + 1
        assert env.lib.gw_step_plan(env.handle, None, None, None, 3, *ptrs, None, None, s) == GW_ERR_ARG, slot
    assert env.lib.gw_step_plan(env.handle, None, None, u16.data_ptr() + 1, 3, *[None] * 8, s) == GW_ERR_ARG  # mask
    env.profile(True, reserve=8)
    a = env.step_plan(horizon=3)
    assert call(env.handle, 3, out.data_ptr()) == 0  # every other output NULL
    assert env.lib.gw_step_plan(env.handle, None, None, None, 4, *[None] * 8, s) == 0  # every output NULL
    torch.cuda.synchronize()
    assert torch.equal(out, a["depth"]) and int(a["depth"].max()) <= 3
    spans = env.profile_spans()
    assert spans[:, 0].tolist() == [GW_SPAN_STEP_PLAN] * 3 and bool((spans[:, 2] > spans[:, 1]).all())
    env.profile(False)
    b = env.step_plan(horizon=3)
    assert b["depth"].data_ptr() == a["depth"].data_ptr()  # allocated once, reused
    with pytest.raises(ValueError):
        env.step_plan(mask=torch.zeros((E, K), dtype=torch.int32, device=env.device))
    env.close()
