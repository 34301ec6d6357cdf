"""The coordinated crash-aware shield on the GPU (gw_crash_shield_joint, csrc/crash_shield_joint.hip).

1. One call equals the rule composed on the GPU from today's entry points per visit (env.fear_preview,
   env.step_preview(mask), env.fear_shield(mask=safe_mask, agents=1 << k), then a final step_preview and
   fear_preview): actions, flags, table, joint, outcome, outcome_prop and crash9 bit for bit, on level3, 2x2_n2_k2
   (N = 2, H*W = 4), 5x8_n5_k5 (the first size with pair lists) and 64x64_n8_k8 (72 final tasks, a second turn);
   sweeps 1 / 2 / 4 / 8, tau None / -0.5 / 0 / 0.5, the env's mask / none / a mask with zero and MdR-forbidding
   entries, probabilities none / tied, agents all / none / a proper subset, actions given / drawn, `out` aliasing
   the input.  Every factor's every value occurs in each scenario's combination list.
2. Equals the CPU reference (tests/_crash_shield_joint_ref.py) on the seeded cases at sweeps 1 and 2, with the
   gw_count_sims count; tau=None, table=None runs no FeAR world update.
3. Through a step on the defer, defer_narrow and merged paths: outcome, table[actions], the bit 3 / 5 / 4 promise and
   the bit 2 promise, both sides of each condition occurring.
4. sweeps = 1, agents = 1 << k equals the unilateral pipeline for every k.
5. It changes nothing: twin env, two calls in a row, FeAR-off env.
6. Edges: E in {1, 3, 5, 257}; envs of one block that converge after different sweep counts; an out-of-range proposal.
7. Graph capture, argument errors, the span kind, every optional output NULL.
8. evaluate and Rollout with shield_mode="joint_crash".

E = 203 is a multiple of neither 4 (envs per block) nor 64."""
import numpy as np
import pytest
import torch

import _crash_shield_joint_ref as CR
import _fear_shield_joint_ref as R
from marlnav import _lib
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu
E0 = R.E0
NA = 9
ALL = 0x1FF
GW_ERR_ARG, GW_ERR_STATE = -1, -4
GW_SPAN_CRASH_SHIELD = 15
NAMES = ("actions", "flags", "table", "joint", "outcome", "outcome_prop", "crash9")
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


def _full_outcome(sp, cur):
    """[E] int16: the outcome of the joint action itself, entry (k = 0, a = cur[:, 0]) of a step_preview of it."""
    return sp["outcome"][:, 0].gather(1, cur[:, :1].long())[:, 0].clone()


def _composed(env, rl, scripted, mask, probs, tau, agents, sweeps, want_table=True):
    """The rule of include/gridenv.h on today's entry points, all envs at once: three calls per visit.  An env that
    has converged is swept again with the others: a sweep over an unchanged joint action changes nothing and
    repeats its answers."""
    E, K, N, dev = env.E, env.K, env.N, env.device
    use_fear = tau is not None
    first = torch.empty((E, N), dtype=torch.int32, device=dev)
    env.fear_preview(rl, scripted, actions=first)
    prop = first[:, :K].contiguous()  # the proposed actions as the step reads them (drawn if rl is None)
    o_prop = _full_outcome(env.step_preview(prop, scripted, reward=False), prop)
    cur = prop.clone()
    stuck = torch.zeros((E, K), dtype=torch.uint8, device=dev)
    unav = torch.zeros((E, K), dtype=torch.uint8, device=dev)
    changed = torch.zeros(E, dtype=torch.bool, device=dev)
    zero = torch.zeros((E, K, NA), dtype=torch.float64, device=dev)
    bits = ((1 << K) - 1 if agents is None else agents) & ((1 << K) - 1)
    if bits:
        for _ in range(sweeps):
            changed = torch.zeros(E, dtype=torch.bool, device=dev)
            for k in range(K):
                if not (bits >> k) & 1:
                    continue
                t = env.fear_preview(cur, scripted) if use_fear else zero
                sp = env.step_preview(cur, scripted, mask=mask, reward=False)
                out, fl = env.fear_shield(t, cur, mask=sp["safe_mask"], probs=probs, tau=tau if use_fear else 0.0,
                                          agents=1 << k)
                mm = torch.full((E,), ALL, dtype=torch.int64, device=dev) if mask is None else mask[:, k].long() & ALL
                stuck[:, k] = (fl[:, k] >> 1) & 1
                unav[:, k] = ((mm != 0) & ((mm & ~sp["crash9"][:, k].long()) == 0)).to(torch.uint8)
                changed |= out[:, k] != cur[:, k]
                cur = out
            if not bool(changed.any()):
                break
    joint = torch.empty((E, N), dtype=torch.int32, device=dev)
    table = env.fear_preview(cur, scripted, actions=joint)
    sp = env.step_preview(cur, scripted, mask=mask, reward=False)
    crash9, o_fin = sp["crash9"].clone(), _full_outcome(sp, cur)
    at = table.gather(2, cur.long().unsqueeze(2))[..., 0]
    sh = torch.tensor([(bits >> k) & 1 for k in range(K)], dtype=torch.bool, device=dev)
    kk = torch.arange(K, device=dev).unsqueeze(0)
    over = (sh.unsqueeze(0) & (at > tau)) if use_fear else torch.zeros((E, K), dtype=torch.bool, device=dev)
    flags = ((cur != prop).to(torch.uint8) | (stuck << 1) | (over.to(torch.uint8) << 2) |
             (changed.to(torch.uint8).unsqueeze(1) << 3) | ((((o_fin.long().unsqueeze(1) & 0xFF) >> kk) & 1).to(torch.uint8) << 4) |
             (unav << 5))
    return dict(actions=cur, flags=flags, table=table if (use_fear or want_table) else None, joint=joint,
                outcome=o_fin, outcome_prop=o_prop, crash9=crash9)


def _poison(env, table=True):
    E, K, N, dev = env.E, env.K, env.N, env.device
    i16 = dict(dtype=torch.int16, device=dev)
    return dict(out=torch.full((E, K), -3, dtype=torch.int32, device=dev),
                flags=torch.full((E, K), 0x77, dtype=torch.uint8, device=dev),
                table=torch.full((E, K, NA), float("nan"), dtype=torch.float64, device=dev) if table else None,
                joint=torch.full((E, N), -3, dtype=torch.int32, device=dev),
                outcome=torch.full((E,), -3, **i16), outcome_prop=torch.full((E,), -3, **i16),
                crash9=torch.full((E, K), -3, **i16))


def _assert_same(got, want, what):
    for name in NAMES:
        g, w = got.get(name), want.get(name)
        if w is None:
            assert g is None, (what, name)
            continue
        assert torch.equal(g, w), (what, name, int((g != w).sum()))


# ---- 1. the composition ----------------------------------------------------------------------------------

# (sweeps, tau, mask kind, probs given, agents kind, rl given, scripted given, alias): every value of every factor
COMBOS = [
    (1, None, "env", False, "all", True, True, False),
    (2, 0.0, "odd", True, "all", True, True, True),
    (4, -0.5, "odd", False, "all", True, False, False),
    (8, None, None, True, "all", True, True, False),
    (2, 0.5, "env", True, "subset", False, True, False),
    (8, 0.0, "odd", True, "subset", True, True, True),
    (2, None, None, False, "none", True, True, False),
    (4, 0.5, "odd", True, "all", False, False, False),
    (1, -0.5, "env", True, "all", False, True, False),
    (2, None, "odd", True, "all", False, True, False),
]
# clustered spawns (tests/_fear_shield_joint_ref.clustered): agents meet
SCENARIOS = {"level3": 3201, "2x2_n2_k2": 3202, "5x8_n5_k5": 3203, "64x64_n8_k8": 3204}


@pytest.mark.parametrize("scen", sorted(SCENARIOS))
def test_equals_the_composition(scen):
    sc = R.scenario(scen)
    spawn, rl, scripted, odd, probs = R.clustered(sc, SCENARIOS[scen], E0)
    env = VecGridEnv(sc, num_envs=E0, fear=True, fear_weight=-5.0, seed=12, max_steps=1000, debug=True)
    dev = env.device
    _, env_mask = env.reset(spawn=torch.as_tensor(spawn.copy()))
    rl_d, sa_d, odd_d, pr_d = _dev(rl, dev), _dev(scripted, dev), _dev(odd, dev), _dev(probs, dev)
    subset = 0b10 if sc.K == 2 else (0b101 | (1 << (sc.K - 1)))  # a proper subset of the K agents
    replaced = crashing = unavoidable = 0
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
        got = env.crash_shield_joint(a, s, mask=mask, probs=p, tau=tau, agents=agents, sweeps=sweeps, **buf)
        torch.cuda.synchronize()
        assert got["actions"] is buf["out"] and got["table"] is buf["table"]
        _assert_same(got, want, (scen, sweeps, tau, mk, use_p, ak, give_rl, give_sa))
        if give_rl and not alias:
            assert torch.equal(a, rl_d)  # the inputs are read only
        f = got["flags"]
        replaced += int((f & 1).sum())
        crashing += int(((f >> 4) & 1).sum())
        unavoidable += int(((f >> 5) & 1).sum())
        if agents == 0:
            assert bool(((f & 0x2F) == 0).all()) and torch.equal(got["actions"], want["joint"][:, :sc.K])
            assert torch.equal(got["outcome"], got["outcome_prop"])
    assert replaced and crashing and unavoidable
    env.close()


# ---- 2. the CPU reference --------------------------------------------------------------------------------

def _case_env(name, E=E0, **kw):
    sc, spawn, rl, scripted, mask, probs, tau = CR.case(name, E)
    env = VecGridEnv(sc, num_envs=E, fear_weight=-5.0, seed=6, max_steps=1000, debug=True, **{"fear": True, **kw})
    env.reset(spawn=torch.as_tensor(spawn.copy()))  # (the cached case arrays are read-only)
    dev = env.device
    return env, (_dev(rl, dev), _dev(scripted, dev), _dev(mask, dev), _dev(probs, dev), tau)


def _assert_ref(buf, want, what):
    for name in NAMES:
        key = "out" if name == "actions" else name
        if want[name] is None:
            continue
        got = buf[key].cpu().numpy()
        ref = want[name].view(np.int16) if want[name].dtype == np.uint16 else want[name]
        np.testing.assert_array_equal(got, ref, err_msg=str((what, name)))


@pytest.mark.parametrize("name", sorted(CR.CASES))
def test_equals_the_cpu_reference(name):
    env, (rl, scripted, mask, probs, tau) = _case_env(name)
    for sweeps in (1, 2):
        want = CR.case_ref(name, sweeps)
        buf = _poison(env, table=tau is not None)
        ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
        env.count_sims(ctr)
        env.crash_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau, sweeps=sweeps, **buf)
        env.count_sims(None)
        torch.cuda.synchronize()
        _assert_ref(buf, want, (name, sweeps))
        assert int(ctr) == want["sims"]  # every world update it ran, the count the header states
        visits = sum(len(c) for c in want["changed"]) * env.K
        if tau is None:  # tau=None, table=None: nine real updates per visit and 9 K at the end, no FeAR update at all
            assert want["fear_sims"] == 0 and int(ctr) == NA * visits + NA * env.K * E0
        else:
            assert want["fear_sims"] > 0
    env.close()


def test_a_table_without_fear_costs_only_the_final_table():
    name = "level3_crash"
    sc, spawn, rl_h, sa_h, mask_h, probs_h, _ = CR.case(name)
    env, (rl, scripted, mask, probs, _) = _case_env(name)
    want = CR.crash_ref(sc, spawn, rl_h, sa_h, mask_h, probs_h, None, None, 2, want_table=True, orc=CR.case_oracle(name))
    buf = _poison(env)
    ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
    env.count_sims(ctr)
    got = env.crash_shield_joint(rl, scripted, mask=mask, probs=probs, tau=None, sweeps=2, **buf)
    env.count_sims(None)
    torch.cuda.synchronize()
    _assert_ref(buf, want, name)
    assert (got["flags"] & 4).sum() == 0  # bit 2 only with use_fear
    assert int(ctr) == want["sims"] and want["fear_sims"] > 0
    assert want["sims"] - want["fear_sims"] == CR.case_ref(name, 2)["sims"]
    env.close()


# ---- 3. through a step -----------------------------------------------------------------------------------

@pytest.mark.parametrize("path", sorted(KERNEL_PATHS))
def test_through_a_step(path, monkeypatch):
    _set_path(monkeypatch, path)
    seen = {k: 0 for k in ("held", "not_held", "crash", "no_crash", "under", "over")}
    for name in ("level3_fear", "3x4_n7_k7_fear", "3x4_n7_k7_crash"):
        env, (rl, scripted, mask, probs, tau) = _case_env(name)
        assert env.kernel_path == KERNEL_PATHS[path]["GW_KERNEL"]
        K = env.K
        joint = torch.full((E0, env.N), -3, dtype=torch.int32, device=env.device)
        g = env.crash_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau, sweeps=2, joint=joint)
        out, flags = g["actions"], g["flags"]
        r = env.step(out, scripted)
        torch.cuda.synchronize()
        assert torch.equal(r.actions[:, :K], out) and torch.equal(joint, r.actions)
        step_outcome = r.crash_bits.to(torch.int16) | (r.restr_bits.to(torch.int16) << 8)
        assert torch.equal(g["outcome"], step_outcome), (name, path)
        crashed = ((r.crash_bits.long().unsqueeze(1) >> torch.arange(K, device=env.device).unsqueeze(0)) & 1).bool()
        assert torch.equal(crashed, (flags & 16) != 0)
        # bit 3 clear, a non-zero mask, bit 5 clear: bit 4 clear, and the agent does not crash in the step
        held = ((flags[:, :1] & 8) == 0) & ((mask & ALL) != 0) & ((flags & 32) == 0)
        assert not bool(crashed[held].any()), (name, path)
        seen["held"] += int(held.sum())
        seen["not_held"] += int((~held).sum())
        seen["crash"] += int(crashed.sum())
        seen["no_crash"] += int((~crashed).sum())
        if tau is not None:
            at = g["table"].gather(2, out.long().unsqueeze(2))[..., 0]
            assert torch.equal(r.fear, at), (name, path)  # every k, bit for bit
            ok = (flags & 4) == 0
            assert bool((r.fear[ok] <= tau).all())
            seen["under"] += int(ok.sum())
            seen["over"] += int((~ok).sum())
        else:
            assert "table" not in g and not bool((flags & 4).any())
        env.close()
    assert all(seen.values()), seen


# ---- 4. one agent, one sweep -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["3x4_n7_k7_fear", "3x4_n7_k7_crash"])
def test_one_agent_one_sweep_is_the_unilateral_pipeline(name):
    env, (rl, scripted, mask, probs, tau) = _case_env(name)
    E, K = env.E, env.K
    table = env.fear_preview(rl, scripted) if tau is not None else \
        torch.zeros((E, K, NA), dtype=torch.float64, device=env.device)
    safe = env.step_preview(rl, scripted, mask=mask, reward=False)["safe_mask"].clone()
    acted = 0
    for k in range(K):
        want_a, want_f = env.fear_shield(table, rl, mask=safe, probs=probs, tau=0.0 if tau is None else tau,
                                         agents=1 << k)
        g = env.crash_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau, agents=1 << k, sweeps=1)
        torch.cuda.synchronize()
        assert torch.equal(g["actions"], want_a) and torch.equal(g["flags"] & 3, want_f), k
        acted += int((want_f != 0).sum())
    assert acted > 0
    env.close()


# ---- 5. it changes nothing -------------------------------------------------------------------------------

def _twin_run(call):
    """call: None a plain run; "beside" two calls before every step, their answers not used; "through" the step
    applies the answer of a call that shields nobody, which is the step's own draw."""
    env = VecGridEnv("grid32", num_envs=E0, fear=True, fear_weight=-5.0, seed=9, max_steps=5, debug=True, stats=True,
                     fear_alt=True)
    env.reset()
    steps = []
    for _ in range(8):
        acts = None
        if call == "beside":
            a = env.crash_shield_joint(tau=0.0, sweeps=2)
            b = env.crash_shield_joint(tau=0.0, sweeps=2)
            assert sorted(a) == sorted(b) == sorted(["actions", "flags", "table", "outcome", "outcome_prop", "crash9"])
            for n in a:
                assert torch.equal(a[n], b[n]) and a[n].data_ptr() != b[n].data_ptr(), n
        elif call == "through":
            g = env.crash_shield_joint(tau=float(env.N), agents=0, sweeps=2)
            assert not bool((g["flags"] & 0x2F).any())
            acts = g["actions"]
        r = env.step(acts)
        torch.cuda.synchronize()
        steps.append({n: getattr(r, n).clone() for n in ("actions", "fear", "fear_alt", "reward", "done", "final_pos",
                                                         "stats", "crash_bits")})
    st = env.state()
    torch.cuda.synchronize()
    env.close()
    return steps, st


def test_the_call_is_result_neutral():
    plain, sp = _twin_run(None)
    for kind in ("beside", "through"):
        a, sa = _twin_run(kind)
        for t, (x, y) in enumerate(zip(a, plain)):
            for n in x:
                assert torch.equal(x[n], y[n]), (kind, t, n)
        for n in sa:
            assert torch.equal(sa[n], sp[n]), (kind, n)


def test_on_a_fear_off_env():
    on, args = _case_env("level3_fear")
    off, _ = _case_env("level3_fear", fear=False)
    rl, scripted, mask, probs, tau = args
    a = on.crash_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau)
    b = off.crash_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau)
    torch.cuda.synchronize()
    _assert_same(b, a, "fear off")
    assert bool((a["table"] != 0).any()) and bool((a["flags"] & 1).any())
    on.close()
    off.close()


# ---- 6. edges --------------------------------------------------------------------------------------------

DEAD_WAVE_SEEDS = {1: 3301, 3: 3302, 5: 3303, 257: 3304}


@pytest.mark.parametrize("E", [1, 3, 5, 257])
def test_dead_waves_in_the_last_block(E):
    sc = R.scenario("3x4_n7_k7")
    spawn, rl, scripted, odd, probs = R.clustered(sc, DEAD_WAVE_SEEDS[E], E)
    env = VecGridEnv(sc, num_envs=E, fear=True, seed=2, max_steps=1000, debug=True)
    env.reset(spawn=torch.as_tensor(spawn.copy()))
    dev = env.device
    rl_d, sa_d, odd_d, pr_d = _dev(rl, dev), _dev(scripted, dev), _dev(odd, dev), _dev(probs, dev)
    for tau in (0.0, None):
        want = _composed(env, rl_d, sa_d, odd_d, pr_d, tau, None, 4)
        buf = _poison(env)
        got = env.crash_shield_joint(rl_d, sa_d, mask=odd_d, probs=pr_d, tau=tau, sweeps=4, **buf)
        torch.cuda.synchronize()
        _assert_same(got, want, (E, tau))
    env.close()


def test_envs_of_one_block_converge_after_different_sweeps():
    env, (rl, scripted, mask, probs, tau) = _case_env("3x4_n7_k7_fear")
    need = torch.full((E0,), 9, dtype=torch.int64, device=env.device)  # the first sweep count with bit 3 clear
    for sweeps in (8, 4, 3, 2, 1):
        want = _composed(env, rl, scripted, mask, probs, tau, None, sweeps)
        got = env.crash_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau, sweeps=sweeps)
        torch.cuda.synchronize()
        want["joint"] = None
        _assert_same(got, want, sweeps)
        need[(got["flags"][:, 0] & 8) == 0] = sweeps
    blocks = need[:E0 - E0 % 4].reshape(-1, 4)  # four waves of a block are four consecutive envs
    mixed = int((blocks.min(1).values != blocks.max(1).values).sum())
    print(f"sweeps to converge: {torch.bincount(need).tolist()}, blocks with different counts: {mixed}")
    assert mixed >= 1 and int(need.max()) >= 3
    env.close()


def test_an_out_of_range_proposal_is_read_as_stay():
    env, (rl, scripted, mask, probs, tau) = _case_env("level3_fear")
    bad = rl.clone()
    bad[::3, 0] = 17
    bad[1::3, 1] = -4
    zero = torch.where((bad < 0) | (bad >= NA), torch.zeros_like(bad), bad)
    for agents in (None, 0):
        for t in (tau, None):
            a = env.crash_shield_joint(bad, scripted, mask=mask, probs=probs, tau=t, agents=agents)
            b = env.crash_shield_joint(zero, scripted, mask=mask, probs=probs, tau=t, agents=agents)
            torch.cuda.synchronize()
            _assert_same(a, b, (agents, t))
            assert bool(((a["actions"] >= 0) & (a["actions"] < NA)).all())
    env.close()


# ---- 7. graph capture, errors, the span ------------------------------------------------------------------

def test_graph_capture():
    env, (rl, scripted, mask, probs, tau) = _case_env("level3_fear")
    buf = _poison(env)
    stream = torch.cuda.Stream()
    args = (env.handle, rl.data_ptr(), scripted.data_ptr(), mask.data_ptr(), probs.data_ptr(), 1, tau, 3, 2,
            buf["out"].data_ptr(), buf["flags"].data_ptr(), buf["table"].data_ptr(), buf["joint"].data_ptr(),
            buf["outcome"].data_ptr(), buf["outcome_prop"].data_ptr(), buf["crash9"].data_ptr())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        buf["joint"].fill_(-3)  # (so that the capture is not empty)
        first = env.lib.gw_crash_shield_joint(*args, stream.cuda_stream)  # it would have to allocate
    assert first == GW_ERR_STATE
    eager = env.crash_shield_joint(rl, scripted, mask=mask, probs=probs, tau=tau, sweeps=2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g, stream=stream):
        status = env.lib.gw_crash_shield_joint(*args, stream.cuda_stream)
    assert status == 0
    torch.cuda.synchronize()
    assert bool((buf["out"] == -3).all())  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    got = dict(buf, actions=buf["out"], joint=None)
    _assert_same(got, dict(eager, joint=None), "replay")
    env.close()


def test_argument_errors_the_span_and_null_outputs():
    env = VecGridEnv("level3", num_envs=5, fear=True, seed=3)
    out = torch.zeros((5, env.K), dtype=torch.int32, device=env.device)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda h, o, sw, uf=0: env.lib.gw_crash_shield_joint(h, None, None, None, None, uf, 0.0, 3, sw, o,  # noqa: E731
                                                                *[None] * 6, s)
    assert call(env.handle, out.data_ptr(), 2) == GW_ERR_STATE  # before the first reset
    env.reset()
    assert call(None, out.data_ptr(), 2) == GW_ERR_ARG
    assert call(env.handle, None, 2) == GW_ERR_ARG
    assert call(env.handle, out.data_ptr(), 0) == GW_ERR_ARG and call(env.handle, out.data_ptr(), 9) == GW_ERR_ARG
    with pytest.raises(ValueError):
        env.crash_shield_joint(sweeps=0)
    with pytest.raises(ValueError):
        env.crash_shield_joint(flags=torch.zeros((5, env.K), dtype=torch.int32, device=env.device))
    with pytest.raises(ValueError):
        env.crash_shield_joint(outcome=torch.zeros(5, dtype=torch.int16))  # not on the device
    env.profile(True, reserve=8)
    full = env.crash_shield_joint(tau=0.0, sweeps=8)
    assert call(env.handle, out.data_ptr(), 8, 1) == 0  # every optional output NULL, with FeAR
    torch.cuda.synchronize()
    assert torch.equal(out, full["actions"])
    crash_only = env.crash_shield_joint(sweeps=8)
    assert call(env.handle, out.data_ptr(), 8, 0) == 0  # ... and without
    torch.cuda.synchronize()
    assert torch.equal(out, crash_only["actions"]) and "table" not in crash_only
    spans = env.profile_spans()
    assert spans[:, 0].tolist() == [GW_SPAN_CRASH_SHIELD] * 4
    assert bool((spans[:, 2] > spans[:, 1]).all())
    env.profile(False)
    env.close()


# ---- 8. evaluate and Rollout -----------------------------------------------------------------------------

def test_evaluate_in_joint_crash_mode():
    from marlnav import scenario as S
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("grid32")
    E, T = 64, 24
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    counts = ("shield_replaced", "shield_stuck", "shield_over", "shield_crash_proposed", "shield_crash_final",
              "shield_unavoidable")
    for kw in (dict(), dict(shield=0.0), dict(shield=0.0, shield_crash=True)):
        r = evaluate(actors, sc, episodes=E, max_steps=T, fear=False, seed=11, shield_mode="joint_crash",
                     shield_sweeps=3, **kw)
        for name in counts:
            assert tuple(r[name].shape) == (sc.K,) and r[name].dtype == torch.int64, name
        assert isinstance(r["shield_unconverged"], int) and "shield_crash_replaced" not in r
        assert 0 < r["steps"] <= E * T and int(r["shield_replaced"].max()) <= r["steps"]
        if "shield" not in kw:  # crash-only: nobody is stuck or over tau, and only crashing proposals move
            assert int(r["shield_stuck"].sum()) == 0 == int(r["shield_over"].sum())
    plain = evaluate(actors, sc, episodes=E, max_steps=T, fear=False, seed=11)
    assert not any(k.startswith("shield") for k in plain)
    with pytest.raises(ValueError):
        evaluate(actors, sc, episodes=E, max_steps=T, shield_mode="joint", shield_crash=True)


@pytest.mark.parametrize("tau,sweeps", [(None, 1), (0.0, 1), (None, 4)])
def test_rollout_in_joint_crash_mode(tau, sweeps):
    """The random policy on the dense map: totals are the per-step sums of the flags; at one sweep envs stay
    unconverged and agents still crash; at four sweeps, in the converged envs, the RL agents' own crashes are
    exactly the unavoidable ones (the env's masks are never 0)."""
    from marlnav.rollout import Rollout
    env = VecGridEnv(R.scenario("3x4_n7_k7"), num_envs=E0, fear=True, fear_weight=-5.0, max_steps=40, seed=42,
                     stats=True, debug=True)
    ro = Rollout(env, None, replay_slots=0, training=True, seed=42, shield=tau, shield_mode="joint_crash", shield_sweeps=sweeps)
    ro.reset()
    K = env.K
    cnt = torch.zeros((6, K), dtype=torch.int64)
    conv_crash = conv_unav = 0
    kk = torch.arange(K, device=env.device).unsqueeze(0)
    for t in range(10):
        r = ro.step()
        torch.cuda.synchronize()
        f = ro.shield_flags.to(torch.int64)
        for b in range(6):
            cnt[b] += ((f >> b) & 1).sum(0).cpu()
        crashed = (r.crash_bits.long().unsqueeze(1) >> kk) & 1
        assert torch.equal(crashed, (f >> 4) & 1), t  # bit 4 is the step's own crash bit
        sp9 = ro.shield_crash9.long()
        assert torch.equal((sp9 >> r.actions[:, :K].long()) & 1, crashed), t  # crash9 of the applied joint action
        conv = (f[:, :1] & 8) == 0
        both = conv.expand(-1, K)
        assert torch.equal(((f >> 4) & 1)[both], ((f >> 5) & 1)[both]), t
        conv_crash += int(((f >> 4) & 1)[both].sum())
        conv_unav += int(((f >> 5) & 1)[both].sum())
        if tau is not None:
            at = ro.shield_table.gather(2, r.actions[:, :K].long().unsqueeze(2))[..., 0]
            assert torch.equal(r.fear, at), t
        else:
            assert ro.shield_table is None
    ro.fence()
    tot = ro.totals()
    assert torch.equal(tot["shield_replaced"], cnt[0]) and torch.equal(tot["shield_stuck"], cnt[1])
    assert torch.equal(tot["shield_over"], cnt[2]) and tot["shield_unconverged"] == int(cnt[3, 0])
    assert torch.equal(tot["shield_crash_final"], cnt[4]) and torch.equal(tot["shield_unavoidable"], cnt[5])
    assert int(tot["shield_crash_proposed"].sum()) > int(tot["shield_crash_final"].sum())
    assert tot["env_steps"] == 10 * E0 and int(cnt[0].sum()) > 0
    print(f"tau {tau}, sweeps {sweeps}: unconverged {int(cnt[3, 0])}, crash_final {cnt[4].tolist()}, "
          f"unavoidable {cnt[5].tolist()}, converged: crashes {conv_crash}, unavoidable {conv_unav}")
    if sweeps == 1:
        assert tot["shield_unconverged"] > 0 and int(tot["shield_crash_final"].sum()) > 0
    else:
        assert conv_crash == conv_unav > 0
    with pytest.raises(ValueError):
        Rollout(env, None, shield_mode="joint_crashes")
    env.close()
