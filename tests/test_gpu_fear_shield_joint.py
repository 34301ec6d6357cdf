"""The coordinated responsibility shield on the GPU (gw_fear_shield_joint, csrc/fear_shield_joint.hip).

1. One call equals the rule composed on the GPU from env.fear_preview + env.fear_shield(agents=1 << k): actions,
   flag bits 0-3, table and joint bit for bit, over built-ins and the shape sweep's rows, sweeps 1 / 2 / 4 / 8,
   tau -0.5 / 0 / 0.5, the env's mask / none / a mask with zero and MdR-forbidding entries, probabilities none /
   with tied maxima, agents all / none / a proper subset, RL and scripted actions given or drawn, actions_out
   aliasing rl_actions.  Every factor's every value occurs in each scenario's combination list.
2. Equals the CPU reference (tests/_fear_shield_joint_ref.py) on the seeded clustered cases, whose floors
   tests/test_fear_shield_joint_cpu.py holds.
3. Through a step on the defer, defer_narrow and merged paths.  The shield's table with nobody shielded, the
   preview's and the step's fear_alt are one table (csrc/fear_alt_core.h from both kernels) at N = 2, 5, 8, E = 5.
4. sweeps = 1, agents = 1 << k equals gw_fear_shield on the same preview table.
5. It changes nothing: twin env, two calls in a row, beside the unjoined FeAR kernels, FeAR-off env.
6. Edges: E in {1, 3, 5, 257}; envs that converge after different sweep counts inside one block; an out-of-range
   proposed action.
7. Graph capture.  8. Argument errors, the span, the sim count.  9. evaluate and Rollout with shield_mode="joint".

E = 203 is a multiple of neither 4 (envs per block) nor 64."""
import numpy as np
import pytest
import torch

import _fear_shield_joint_ref as R
from marlnav import _lib
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu
E0 = R.E0
NA = 9
GW_ERR_ARG, GW_ERR_STATE = -1, -4
GW_SPAN_FEAR_SHIELD = 13
KERNEL_PATHS = {
    "defer": {"GW_KERNEL": "defer"},
    "defer_narrow": {"GW_KERNEL": "defer", "GW_FEAR_BE": "narrow"},
    "merged": {"GW_KERNEL": "merged"},
}


def _set_path(monkeypatch, path):
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    for k, v in KERNEL_PATHS[path].items():
        monkeypatch.setenv(k, v)


def _dev(a, dev):
    if a is None:
        return None
    a = np.array(a.view(np.int16) if a.dtype == np.uint16 else a)  # a copy: the cached case arrays are read-only
    return torch.as_tensor(a).to(dev).contiguous()


def _composed(env, rl, scripted, mask, probs, tau, agents, sweeps):
    """The rule of include/gridenv.h on today's entry points, all envs at once.  An env that has converged is
    swept again with the others: a sweep over an unchanged joint action changes nothing and repeats its answers."""
    E, K, N, dev = env.E, env.K, env.N, env.device
    first = torch.empty((E, N), dtype=torch.int32, device=dev)
    env.fear_preview(rl, scripted, actions=first)
    prop = first[:, :K].contiguous()  # the proposed actions as the step reads them (drawn if rl is None)
    cur = prop.clone()
    stuck = torch.zeros((E, K), dtype=torch.uint8, device=dev)
    changed = torch.zeros(E, dtype=torch.bool, device=dev)
    bits = ((1 << K) - 1 if agents is None else agents) & ((1 << K) - 1)
    if bits:
        for _ in range(sweeps):
            changed = torch.zeros(E, dtype=torch.bool, device=dev)
            for k in range(K):
                if not (bits >> k) & 1:
                    continue
                t = env.fear_preview(cur, scripted)
                out, fl = env.fear_shield(t, cur, mask=mask, probs=probs, tau=tau, agents=1 << k)
                stuck[:, k] = (fl[:, k] >> 1) & 1
                changed |= out[:, k] != cur[:, k]
                cur = out
            if not bool(changed.any()):
                break
    joint = torch.empty((E, N), dtype=torch.int32, device=dev)
    table = env.fear_preview(cur, scripted, actions=joint)
    at = table.gather(2, cur.long().unsqueeze(2))[..., 0]
    sh = torch.tensor([(bits >> k) & 1 for k in range(K)], dtype=torch.bool, device=dev)
    flags = ((cur != prop).to(torch.uint8) | (stuck << 1) | ((sh.unsqueeze(0) & (at > tau)).to(torch.uint8) << 2) |
             (changed.to(torch.uint8).unsqueeze(1) << 3))
    return cur, flags, table, joint


def _poison(env):
    E, K, N, dev = env.E, env.K, env.N, env.device
    return dict(out=torch.full((E, K), -3, dtype=torch.int32, device=dev),
                flags=torch.full((E, K), 0x77, dtype=torch.uint8, device=dev),
                table=torch.full((E, K, NA), float("nan"), dtype=torch.float64, device=dev),
                joint=torch.full((E, N), -3, dtype=torch.int32, device=dev))


def _assert_same(got, want, what):
    for name, g, w in zip(("actions", "flags", "table", "joint"), got, want):
        assert torch.equal(g, w), (what, name, int((g != w).sum()))


# ---- 1. the composition ----------------------------------------------------------------------------------

# (sweeps, tau, mask kind, probs given, agents kind, rl given, scripted given, alias): every value of every factor
COMBOS = [
    (1, 0.0, "env", False, "all", True, True, False),
    (2, 0.0, "odd", True, "all", True, True, True),
    (4, -0.5, "odd", False, "all", True, False, False),
    (8, -0.5, None, True, "all", True, True, False),
    (2, 0.5, "env", True, "subset", False, True, False),
    (8, 0.0, "odd", True, "subset", True, True, True),
    (2, 0.0, None, False, "none", True, True, False),
    (4, 0.5, "odd", True, "all", False, False, False),
    (1, -0.5, "env", True, "all", False, True, False),
]
SCENARIOS = R.COMPOSITION_SCENARIOS  # their case sets and the floors they meet: tests/_fear_shield_joint_ref.py


@pytest.mark.parametrize("scen", SCENARIOS)
def test_equals_the_composition(scen):
    sc, spawn, rl, scripted, odd, probs = R.clustered_set(scen)
    env = VecGridEnv(sc, num_envs=E0, fear=True, fear_weight=-5.0, seed=12, max_steps=1000, debug=True)
    dev = env.device
    _, env_mask = env.reset(spawn=torch.as_tensor(spawn.copy()))
    rl_d, sa_d, odd_d, pr_d = _dev(rl, dev), _dev(scripted, dev), _dev(odd, dev), _dev(probs, dev)
    subset = 0b10 if sc.K == 2 else (0b101 | (1 << (sc.K - 1)))  # a proper subset of the K agents
    seen = 0
    for sweeps, tau, mk, use_p, ak, give_rl, give_sa, alias in COMBOS:
        mask = {"env": env_mask, "odd": odd_d, None: None}[mk]
        agents = {"all": None, "none": 0, "subset": subset}[ak]
        a = rl_d.clone() if give_rl else None
        s = sa_d if give_sa else None
        p = pr_d if use_p else None
        want = _composed(env, a, s, mask, p, tau, agents, sweeps)
        buf = _poison(env)
        if alias and a is not None:
            buf["out"] = a
        got = env.fear_shield_joint(a, s, mask=mask, probs=p, tau=tau, agents=agents, sweeps=sweeps, **buf)
        torch.cuda.synchronize()
        _assert_same((got[0], got[1], got[2], buf["joint"]), want, (scen, sweeps, tau, mk, use_p, ak, give_rl, give_sa))
        if give_rl and not alias:
            assert torch.equal(a, rl_d)  # the inputs are read only
        seen += int((got[1] & 1).sum())  # actions replaced
        if agents == 0:
            assert bool((got[1] == 0).all()) and torch.equal(got[0], want[3][:, :sc.K])
    assert seen
    env.close()


# ---- 2. the CPU reference --------------------------------------------------------------------------------

def _case_env(name, E=E0, **kw):
    sc, spawn, rl, scripted, mask, probs, tau = R.case(name, E)
    env = VecGridEnv(sc, num_envs=E, fear_weight=-5.0, seed=6, max_steps=1000, debug=True, **{"fear": True, **kw})
    env.reset(spawn=torch.as_tensor(spawn.copy()))  # (the cached case arrays are read-only)
    dev = env.device
    return env, (_dev(rl, dev), _dev(scripted, dev), _dev(mask, dev), _dev(probs, dev), tau)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_equals_the_cpu_reference(name):
    env, (rl, scripted, mask, probs, tau) = _case_env(name)
    for sweeps in (1, 2):
        want = R.case_ref(name, sweeps)
        buf = _poison(env)
        ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
        env.count_sims(ctr)
        env.fear_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau, sweeps=sweeps, **buf)
        env.count_sims(None)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(buf["out"].cpu().numpy(), want["actions"])
        np.testing.assert_array_equal(buf["flags"].cpu().numpy(), want["flags"])
        np.testing.assert_array_equal(buf["table"].cpu().numpy(), want["table"])
        np.testing.assert_array_equal(buf["joint"].cpu().numpy(), want["joint"])
        assert int(ctr) == want["sims"]  # every world update it ran, the reference's task count
    env.close()


# ---- 3. through a step -----------------------------------------------------------------------------------

@pytest.mark.parametrize("path", sorted(KERNEL_PATHS))
def test_through_a_step(path, monkeypatch):
    _set_path(monkeypatch, path)
    for name in ("level3", "3x4_n7_k7"):
        env, (rl, scripted, mask, probs, tau) = _case_env(name)
        assert env.kernel_path == KERNEL_PATHS[path]["GW_KERNEL"]
        K = env.K
        joint = torch.full((E0, env.N), -3, dtype=torch.int32, device=env.device)
        out, flags, table = env.fear_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau, sweeps=2, joint=joint)
        r = env.step(out, scripted)
        torch.cuda.synchronize()
        assert torch.equal(r.actions[:, :K], out) and torch.equal(joint, r.actions)
        at = table.gather(2, out.long().unsqueeze(2))[..., 0]
        assert torch.equal(r.fear, at), (name, path)  # every k, bit for bit
        ok = (flags & 4) == 0
        assert bool((r.fear[ok] <= tau).all()) and bool(ok.any()) and bool((~ok).any())
        env.close()


# The table code the shield and fear_alt_kernel share (csrc/fear_alt_core.h), from both kernels on one state, at
# the smallest shapes where it branches: N = 2 on H*W = 4; N = K = 5, the first agent count with pair lists;
# N = K = 8, the largest sets.  E = 5: one full block and a block whose last three waves are past the env range.
# Seeds: clustered spawns (tests/_fear_shield_joint_ref.clustered) whose tables are not all zero.
CORE_CASES = {"2x2_n2_k2": 921, "5x8_n5_k5": 922, "64x64_n8_k8": 923}


@pytest.mark.parametrize("sid", sorted(CORE_CASES))
def test_shield_preview_and_step_give_one_table(sid):
    sc = R.scenario(sid)
    E = 5
    spawn, rl, scripted, _, _ = R.clustered(sc, CORE_CASES[sid], E)
    env = VecGridEnv(sc, num_envs=E, fear=True, fear_weight=-5.0, seed=3, max_steps=1000, debug=True, fear_alt=True)
    dev = env.device
    env.reset(spawn=torch.as_tensor(spawn.copy()))
    rl_d, sa_d = _dev(rl, dev), _dev(scripted, dev)
    buf = _poison(env)
    out, _, table = env.fear_shield_joint(rl_d, sa_d, agents=0, sweeps=1, **buf)  # the shield's run(all) and row
    preview = env.fear_preview(rl_d, sa_d).clone()                               # fear_alt_kernel on the same record
    env.out["fear_alt"].fill_(float("nan"))
    r = env.step(out, sa_d)
    torch.cuda.synchronize()
    assert torch.equal(out, rl_d)
    assert not bool(torch.isnan(table).any()) and bool((table != 0).any())
    assert torch.equal(table, preview), sid
    assert torch.equal(table, r.fear_alt), sid
    env.close()


# ---- 4. one agent, one sweep -----------------------------------------------------------------------------

def test_one_agent_one_sweep_is_gw_fear_shield():
    env, (rl, scripted, mask, probs, tau) = _case_env("3x4_n7_k7")
    table = env.fear_preview(rl, scripted)
    acted = 0
    for k in range(env.K):
        want_a, want_f = env.fear_shield(table, rl, mask=mask, probs=probs, tau=tau, agents=1 << k)
        out, flags, _ = env.fear_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau, agents=1 << k, sweeps=1)
        torch.cuda.synchronize()
        assert torch.equal(out, want_a) and torch.equal(flags & 3, want_f), k
        acted += int((want_f != 0).sum())
    assert acted > 0
    env.close()


# ---- 5. it changes nothing -------------------------------------------------------------------------------

def _twin_run(call):
    env = VecGridEnv("grid32", num_envs=E0, fear=True, fear_weight=-5.0, seed=9, max_steps=5, debug=True, stats=True,
                     fear_alt=True)
    env.reset()
    steps = []
    for _ in range(8):
        if call:
            a = env.fear_shield_joint(tau=0.0, sweeps=2)
            b = env.fear_shield_joint(tau=0.0, sweeps=2)
            for x, y in zip(a, b):
                assert torch.equal(x, y) and x.data_ptr() != y.data_ptr()
        r = env.step()
        torch.cuda.synchronize()
        steps.append({n: getattr(r, n).clone() for n in ("actions", "fear", "fear_alt", "reward", "done", "final_pos",
                                                         "stats")})
    st = env.state()
    torch.cuda.synchronize()
    env.close()
    return steps, st


def test_the_call_is_result_neutral():
    (a, sa), (b, sb) = _twin_run(True), _twin_run(False)
    for t, (x, y) in enumerate(zip(a, b)):
        for n in x:
            assert torch.equal(x[n], y[n]), (t, n)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n


def test_beside_the_unjoined_fear_kernels(monkeypatch):
    """The pattern of test_preview_beside_the_unjoined_fear_kernels: step t's fear_alt kernel may still read the
    steps' record buffer on the aux stream while the call of step t + 1 writes the preview's own."""
    _set_path(monkeypatch, "defer")
    env = VecGridEnv("grid32", num_envs=E0, fear=True, fear_weight=-5.0, seed=8, max_steps=5, debug=True,
                     fear_alt=True)
    env.set_obs_async("lazy", fear_async=True)
    env.reset()
    last = None
    for t in range(9):
        cur = env.fear_shield_joint(tau=float(env.N), sweeps=2) if t < 8 else None  # tau = N: nothing is replaced
        if last is not None:
            env.fear_fence()
            torch.cuda.synchronize()
            (out, flags, table), r = last
            assert torch.equal(table, r.fear_alt) and torch.equal(out, r.actions[:, :env.K]), t - 1
            assert bool((flags == 0).all())
        if t < 8:
            last = (cur, env.step())
    env.obs_fence()
    torch.cuda.synchronize()
    env.close()


def test_on_a_fear_off_env():
    on, args = _case_env("level3")
    off, _ = _case_env("level3", fear=False)
    rl, scripted, mask, probs, tau = args
    a = on.fear_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau)
    b = off.fear_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau)
    torch.cuda.synchronize()
    _assert_same(b, a, "fear off")
    assert bool((a[2] != 0).any())
    on.close()
    off.close()


# ---- 6. edges --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [1, 3, 5, 257])
def test_dead_waves_in_the_last_block(E):
    sc, spawn, rl, scripted, odd, probs = R.clustered_set(f"{R.DEAD_WAVE_SCENARIO}@{E}")
    env = VecGridEnv(sc, num_envs=E, fear=True, seed=2, max_steps=1000, debug=True)
    env.reset(spawn=torch.as_tensor(spawn.copy()))
    dev = env.device
    rl_d, sa_d, odd_d, pr_d = _dev(rl, dev), _dev(scripted, dev), _dev(odd, dev), _dev(probs, dev)
    want = _composed(env, rl_d, sa_d, odd_d, pr_d, 0.0, None, 4)
    buf = _poison(env)
    got = env.fear_shield_joint(rl_d, sa_d, mask=odd_d, probs=pr_d, tau=0.0, sweeps=4, **buf)
    torch.cuda.synchronize()
    _assert_same((got[0], got[1], got[2], buf["joint"]), want, E)
    env.close()


def test_envs_of_one_block_converge_after_different_sweeps():
    env, (rl, scripted, mask, probs, tau) = _case_env("3x4_n7_k7")
    need = torch.full((E0,), 9, dtype=torch.int64, device=env.device)  # the first sweep count with bit 3 clear
    for sweeps in (8, 4, 3, 2, 1):
        want = _composed(env, rl, scripted, mask, probs, tau, None, sweeps)
        got = env.fear_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau, sweeps=sweeps, joint=None)
        torch.cuda.synchronize()
        _assert_same(got, want[:3], sweeps)
        need[(got[1][:, 0] & 8) == 0] = sweeps
    blocks = need[:E0 - E0 % 4].reshape(-1, 4)  # four waves of a block are four consecutive envs
    mixed = int((blocks.min(1).values != blocks.max(1).values).sum())
    print(f"sweeps to converge: {torch.bincount(need).tolist()}, blocks with different counts: {mixed}")
    assert mixed >= 1 and int(need.max()) >= 3
    env.close()


def test_an_out_of_range_proposal_is_read_as_stay():
    env, (rl, scripted, mask, probs, tau) = _case_env("level3")
    bad = rl.clone()
    bad[::3, 0] = 17
    bad[1::3, 1] = -4
    zero = torch.where((bad < 0) | (bad >= NA), torch.zeros_like(bad), bad)
    for agents in (None, 0):
        a = env.fear_shield_joint(bad, scripted, mask=mask, probs=probs, tau=tau, agents=agents)
        b = env.fear_shield_joint(zero, scripted, mask=mask, probs=probs, tau=tau, agents=agents)
        torch.cuda.synchronize()
        _assert_same(a, b, agents)
        assert bool(((a[0] >= 0) & (a[0] < NA)).all())
    r = env.step(bad, scripted)  # the step applies the same 0
    torch.cuda.synchronize()
    assert torch.equal(r.actions[:, :env.K], zero)
    env.close()


# ---- 7. graph capture ------------------------------------------------------------------------------------

def test_graph_capture():
    env, (rl, scripted, mask, probs, tau) = _case_env("level3")
    buf = _poison(env)
    stream = torch.cuda.Stream()
    args = (env.handle, rl.data_ptr(), scripted.data_ptr(), mask.data_ptr(), probs.data_ptr(), tau, 3, 2,
            buf["out"].data_ptr(), buf["flags"].data_ptr(), buf["table"].data_ptr(), buf["joint"].data_ptr())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        buf["joint"].fill_(-3)  # (so that the capture is not empty)
        first = env.lib.gw_fear_shield_joint(*args, stream.cuda_stream)  # it would have to allocate
    assert first == GW_ERR_STATE
    eager = env.fear_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau, sweeps=2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        status = env.lib.gw_fear_shield_joint(*args, stream.cuda_stream)
    assert status == 0
    torch.cuda.synchronize()
    assert bool((buf["out"] == -3).all())  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    _assert_same((buf["out"], buf["flags"], buf["table"]), eager, "replay")
    env.close()


# ---- 8. errors, span, sims -------------------------------------------------------------------------------

def test_argument_errors_and_the_span():
    env = VecGridEnv("level3", num_envs=5, fear=True, seed=3)
    out = torch.zeros((5, env.K), dtype=torch.int32, device=env.device)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda h, o, sw: env.lib.gw_fear_shield_joint(h, None, None, None, None, 0.0, 3, sw, o, None, None, None, s)  # noqa: E731
    assert call(env.handle, out.data_ptr(), 2) == GW_ERR_STATE  # before the first reset
    env.reset()
    assert call(None, out.data_ptr(), 2) == GW_ERR_ARG
    assert call(env.handle, None, 2) == GW_ERR_ARG
    assert call(env.handle, out.data_ptr(), 0) == GW_ERR_ARG and call(env.handle, out.data_ptr(), 9) == GW_ERR_ARG
    with pytest.raises(ValueError):
        env.fear_shield_joint(sweeps=0)
    with pytest.raises(ValueError):
        env.fear_shield_joint(flags=torch.zeros((5, env.K), dtype=torch.int32, device=env.device))
    env.profile(True, reserve=8)
    env.fear_shield_joint(sweeps=8)
    env.fear_shield_joint(sweeps=1, flags=None, table=None)
    assert call(env.handle, out.data_ptr(), 1) == 0  # flags, table and joint NULL
    torch.cuda.synchronize()
    spans = env.profile_spans()
    assert spans[:, 0].tolist() == [GW_SPAN_FEAR_SHIELD] * 3 and bool((spans[:, 2] > spans[:, 1]).all())
    env.profile(False)
    env.close()


# ---- 9. evaluate and Rollout -----------------------------------------------------------------------------

def test_evaluate_in_joint_mode():
    from marlnav import scenario as S
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("grid32")
    E, T = 64, 24
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    plain = evaluate(actors, sc, episodes=E, max_steps=T, fear=True, seed=11, record_actions=True)
    # every row sum is at most N - 1: tau = N can never replace an action
    loose = evaluate(actors, sc, episodes=E, max_steps=T, fear=True, seed=11, record_actions=True, shield=float(sc.N),
                     shield_mode="joint", shield_sweeps=3)
    for name in ("crashes", "apples_caught", "steps", "fear"):
        assert plain[name] == loose[name], name
    assert torch.equal(plain["actions"], loose["actions"])
    for name in ("shield_replaced", "shield_stuck", "shield_over"):
        assert tuple(loose[name].shape) == (sc.K,) and int(loose[name].sum()) == 0
    assert loose["shield_unconverged"] == 0
    uni = evaluate(actors, sc, episodes=E, max_steps=T, fear=False, seed=11, shield=0.0)
    assert "shield_over" not in uni and "shield_over" not in plain
    # Non-zero counts with a known answer.  Every table entry is at least -(N - 1), so at tau = -N no action is
    # allowed: every agent (the env's masks are never 0) is stuck and over tau at every step of every episode still
    # running, which is what "steps" counts.  With one sweep an env is unconverged where an action was replaced.
    low = evaluate(actors, sc, episodes=E, max_steps=T, fear=False, seed=11, shield=-float(sc.N), shield_mode="joint",
                   shield_sweeps=1)
    assert 0 < low["steps"] <= E * T  # (the episodes still running alone are counted)
    assert low["shield_over"].tolist() == [low["steps"]] * sc.K == low["shield_stuck"].tolist()
    rep_k = low["shield_replaced"]
    assert int(rep_k.max()) > 0 and int(rep_k.max()) <= low["shield_unconverged"] <= min(int(rep_k.sum()), low["steps"])
    with pytest.raises(ValueError):
        evaluate(actors, sc, episodes=E, max_steps=T, shield=0.0, shield_mode="both")


@pytest.mark.parametrize("policy,scen,sweeps", [("actors", "grid32", 2), ("random", "grid32", 2),
                                                ("random", "3x4_n7_k7", 1)])
def test_rollout_in_joint_mode(policy, scen, sweeps):
    """The dense map at one sweep is where bits 2 and 3 are common: there the compared counts must be non-zero."""
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    env = VecGridEnv(R.scenario(scen), num_envs=E0, fear=True, fear_weight=-5.0, max_steps=40, seed=42, stats=True,
                     debug=True)
    actors = MultiAgentActors(env.K, env.H, env.W, arch="mlp", device=env.device, seed=0) if policy == "actors" else None
    ro = Rollout(env, actors, replay_slots=16 if actors is not None else 0, training=True, seed=42, shield=0.0,
                 shield_mode="joint", shield_sweeps=sweeps)
    ro.reset()
    cnt = torch.zeros((4, env.K), dtype=torch.int64)
    for t in range(10):
        r = ro.step()
        torch.cuda.synchronize()
        f = ro.shield_flags.cpu().to(torch.int64)
        for b in range(4):
            cnt[b] += (f >> b & 1).sum(0)
        ok = (ro.shield_flags & 4) == 0
        assert bool((r.fear[ok] <= 0.0).all()), t  # the step's FeAR of every agent without bit 2
        at = ro.shield_table.gather(2, r.actions[:, :env.K].long().unsqueeze(2))[..., 0]
        assert torch.equal(r.fear, at), t
    ro.fence()
    tot = ro.totals()
    assert torch.equal(tot["shield_replaced"], cnt[0]) and torch.equal(tot["shield_stuck"], cnt[1])
    assert torch.equal(tot["shield_over"], cnt[2]) and tot["shield_unconverged"] == int(cnt[3, 0])
    assert tot["env_steps"] == 10 * E0
    if policy == "random":
        assert int(cnt[0].sum()) > 0
    if scen == "3x4_n7_k7":
        print(f"over {cnt[2].tolist()}, unconverged {int(cnt[3, 0])}, stuck {cnt[1].tolist()}")
        # at one sweep an agent is over tau where a later visit changed the world under it (or where it was stuck):
        # the last agent visited saw the final joint action, so it is over only where it was stuck
        assert int(cnt[2].sum()) > 0 and int(cnt[3, 0]) > 0
        assert int(cnt[2, -1]) <= int(cnt[1, -1])
    if actors is not None:
        with pytest.raises(ValueError):
            ro.capture(8)
    with pytest.raises(ValueError):
        Rollout(env, None, shield=0.0, shield_mode="both")
    env.close()
