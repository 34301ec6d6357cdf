"""Per-agent FeAL and valid-action sets from the step (gw_set_feal, VecGridEnv(feal=True)).

1. The reference's own Responsibility.FeAL known-answer cases (tests/golden/fear_matrix.npz, recorded from
   custom/Responsibility.py:213-303) through the STEP and feal_kernel, one case per env and one step, on
   the defer (wide / narrow FeAR blocks) and merged paths: the cases whose in_list is all ones (the
   step lists every agent) and whose MdR row is one constant, split by that constant, each split on a
   scenario whose MdR table is that constant (as test_gpu_fear_rows._scenario).  feal bit for bit, the
   popcounts of feal_valid against feal_vm / feal_va, for every agent; all 118 cases, none left out.
2. Native Philox rollouts (grid32 N = 4, grid64_n8 N = 8: the pair-list world; E = 7: a partial last
   block, E = 1: a one-env grid; auto-reset on, the step cap 4 makes every env reset at step 4 of 6):
   every step against gw_fear_matrix and the C oracle on the pre-step snapshot.
3. The reference's invariant: the others-actual variant with b = the agent's own action is the step's
   own world update, so that bit of feal_valid[..., 1] is "neither crashed nor restricted" of the step.
4. Result-neutral; disarming stops the writes; one pointer alone.  5. FeAR off: GW_ERR_STATE.
6. Ordering: unjoined FeAR (fear_fence) and captured steps on the merged path.
7. gw_feal_accum, Rollout(feal=True) eager == graph replay, evaluate(feal=True).
8. The facade's info["feal"] and customeval.py --feal.

Summation bound (7): any order of summing n f64 terms x_i differs from the exact sum by at most
(n - 1) u sum|x_i| (1 + O(n u)), u = 2^-53 (derived in test_gpu_fear_rows' header); the tests allow
n * 2^-53 * sum|x_i| between the kernel's fixed tree and numpy's sum, computed from the data."""
import dataclasses
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
KAT_GROUPS = {"grid32": 25, "level3": 9, "open5x8_n5": 22, "open6_n3": 50, "open6_n8": 12}
KERNEL_PATHS = {
    "defer": {"GW_KERNEL": "defer"},
    "defer_narrow": {"GW_KERNEL": "defer", "GW_FEAR_BE": "narrow"},
    "merged": {"GW_KERNEL": "merged"},
}
K = 2
U = 2.0 ** -53
GW_ERR_STATE = -4


def _set_path(monkeypatch, path):
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    for k, v in KERNEL_PATHS[path].items():
        monkeypatch.setenv(k, v)


def _popcount(x):
    x = np.asarray(x).astype(np.int64) & 0xFFFF
    return sum((x >> b) & 1 for b in range(16))


def _sets(t: torch.Tensor) -> np.ndarray:
    """feal_valid (int16 views of the u16 bit sets) as non-negative ints [E, N, 2]."""
    return t.cpu().numpy().view(np.uint16).astype(np.int64)


def _scenario(region2d: np.ndarray, N: int, mdr_value: int) -> S.CompiledScenario:
    """A scenario on the case's map with K = 2 RL agents and the constant MdR ``mdr_value`` in every
    cell (as test_gpu_fear_rows._scenario)."""
    base = S.builtin("level3")
    H, W = region2d.shape
    free = np.flatnonzero(region2d.reshape(-1) == 1).astype(np.int32)
    return dataclasses.replace(
        base, name="feal_kat", H=H, W=W, N=N, K=K, region=(region2d != 0).astype(np.uint8).reshape(-1),
        policy_id=np.zeros(H * W, np.uint8), policy_keys=base.policy_keys[:1], policy_p=base.policy_p[:1],
        policy_cdf=base.policy_cdf[:1], mdr=np.full(H * W, mdr_value, np.uint8), apples=free[:K].copy(),
        free_cells=free, okmask=S.okmask_table(region2d), action_mask=S.action_mask_table(region2d))


def _kat_cases(name):
    z = np.load(os.path.join(GOLD, "fear_matrix.npz"))
    d = {k.split("/", 1)[1]: np.asarray(z[k]) for k in z.files if k.startswith(name + "/")}
    sel = (d["in_list"] != 0).all(1) & (d["mdr"] == d["mdr"][:, :1]).all(1)
    return d, np.flatnonzero(sel)


@pytest.mark.parametrize("path", sorted(KERNEL_PATHS))
def test_reference_kats_through_the_step(path, monkeypatch):
    _set_path(monkeypatch, path)
    compared = below_one = 0
    values = set()
    for name, count in sorted(KAT_GROUPS.items()):
        d, sel = _kat_cases(name)
        assert sel.size == count, (name, sel.size)
        N = d["loc"].shape[1]
        v_all = d["mdr"][sel, 0]
        for v in np.unique(v_all):
            idx = sel[v_all == v]
            E = idx.size
            env = VecGridEnv(_scenario(d["region"], N, int(v)), num_envs=E, fear=True, fear_weight=-5.0,
                             max_steps=1000, debug=True, feal=True)
            try:
                assert env.kernel_path == KERNEL_PATHS[path]["GW_KERNEL"]
                env.reset(spawn=torch.as_tensor(d["loc"][idx].astype(np.int32)))
                env.out["feal"].fill_(float("nan"))
                env.out["feal_valid"].fill_(-1)
                act = d["act"][idx].astype(np.int32)
                r = env.step(act[:, :K].copy(), act[:, K:].copy())
                torch.cuda.synchronize()
                np.testing.assert_array_equal(r.actions.cpu().numpy(), act)
                assert (r.mdr.cpu().numpy() == v).all()
                fe, fv = r.feal.cpu().numpy(), _sets(r.feal_valid)
                assert fe.shape == (E, N) and fv.shape == (E, N, 2) and (fv < 512).all()
                print(f"{name} mdr {v}: {E} cases, feal differs in {int((fe != d['feal'][idx]).sum())} of {fe.size}")
                np.testing.assert_array_equal(fe, d["feal"][idx], err_msg=f"{name} mdr {v}: feal")
                np.testing.assert_array_equal(_popcount(fv[..., 0]), d["feal_vm"][idx], err_msg=f"{name}: feal_vm")
                np.testing.assert_array_equal(_popcount(fv[..., 1]), d["feal_va"][idx], err_msg=f"{name}: feal_va")
                compared += E
                below_one += int((fe < 1).sum())
                values.add(int(v))
            finally:
                env.close()
    assert compared == 118, compared
    assert below_one > 0
    assert values == {0, 1, 2, 3, 4, 8}


def _rollout_checks(scen, E, path_env):
    """6 native steps; every step's feal / feal_valid against gw_fear_matrix and the C oracle on the
    pre-step snapshot, and the invariant of the agent's own action (test 3).  -> done envs seen."""
    sc = S.builtin(scen)
    N, H, W = sc.N, sc.H, sc.W
    region = np.asarray(sc.region).reshape(H, W)
    env = VecGridEnv(sc, num_envs=E, fear=True, fear_weight=-5.0, seed=5, max_steps=4, auto_reset=True,
                     debug=True, feal=True)
    assert env.kernel_path == path_env
    env.reset()
    resets = own_invalid = 0
    try:
        for t in range(6):
            cells = env.positions().cpu().numpy().astype(np.int32)  # the pre-step (pre-reset) world
            env.out["feal"].fill_(float("nan"))
            env.out["feal_valid"].fill_(-1)
            r = env.step()
            torch.cuda.synchronize()
            acts, mdr = r.actions.cpu().numpy(), r.mdr.cpu().numpy()
            fe, fv = r.feal.cpu().numpy(), _sets(r.feal_valid)
            vm, va = _popcount(fv[..., 0]), _popcount(fv[..., 1])
            assert not np.isnan(fe).any() and (fv < 512).all()
            fm = {k: v.cpu().numpy() for k, v in env.fear_matrix(cells, acts, mdr, None).items()}
            np.testing.assert_array_equal(fe, fm["feal"], err_msg=f"step {t}: feal vs gw_fear_matrix")
            np.testing.assert_array_equal(vm, fm["feal_vm"], err_msg=f"step {t}")
            np.testing.assert_array_equal(va, fm["feal_va"], err_msg=f"step {t}")
            for e in range(E):
                o = O.fear_matrix(H, W, region, cells[e], acts[e], mdr[e], None)
                np.testing.assert_array_equal(fe[e], o["feal"], err_msg=f"step {t} env {e}: feal vs oracle")
                np.testing.assert_array_equal(vm[e], o["feal_vm"], err_msg=f"step {t} env {e}")
                np.testing.assert_array_equal(va[e], o["feal_va"], err_msg=f"step {t} env {e}")
            # 3: bit actions[e][i] of the others-actual set is the step's own validity of agent i
            bad = (r.crash_bits.cpu().numpy().astype(np.int64) | r.restr_bits.cpu().numpy().astype(np.int64))
            for i in range(N):
                own = (fv[:, i, 1] >> acts[:, i]) & 1
                np.testing.assert_array_equal(own, 1 - ((bad >> i) & 1), err_msg=f"step {t} agent {i}")
                own_invalid += int((own == 0).sum())
            resets += int(r.done.sum())
    finally:
        env.close()
    return resets, own_invalid


@pytest.mark.parametrize("path", ["defer", "merged"])
@pytest.mark.parametrize("scen,E", [("grid32", 7), ("grid32", 1), ("grid64_n8", 7), ("grid64_n8", 1)])
def test_native_rollout_matches_fear_matrix_and_oracle(scen, E, path, monkeypatch):
    _set_path(monkeypatch, path)
    resets, _ = _rollout_checks(scen, E, KERNEL_PATHS[path]["GW_KERNEL"])
    assert resets >= E, "no env auto-reset within the 6 steps"  # the step cap is 4: the pre-reset rule ran


NEUTRAL_SKIP = ("feal", "feal_valid")


def _neutral_run(feal, fear_async):
    env = VecGridEnv("grid32", num_envs=512, fear=True, fear_weight=-5.0, seed=9, max_steps=6, debug=True,
                     stats=True, feal=feal)
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
                      if f.name not in NEUTRAL_SKIP and getattr(r, f.name) is not None})
    st = env.state()
    counts = env.obs_delta_counts()
    torch.cuda.synchronize()
    env.close()
    return steps, st, counts


@pytest.mark.parametrize("path,fear_async", [("defer", False), ("merged", False), ("defer", True)])
def test_feal_is_result_neutral(path, fear_async, monkeypatch):
    _set_path(monkeypatch, path)
    (a, sa, ca), (b, sb, cb) = _neutral_run(True, fear_async), _neutral_run(False, fear_async)
    assert len(a) == len(b) == 10
    for t, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys() and "obs" in x
        for n in x:
            assert torch.equal(x[n], y[n]), (t, n)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n
    assert ca == cb and sum(ca) >= 10  # gw_obs_delta_counts: the same writers wrote the same obs


@pytest.mark.parametrize("path", ["defer", "merged"])
def test_disarming_and_single_pointers(path, monkeypatch):
    _set_path(monkeypatch, path)
    env = VecGridEnv("grid32", num_envs=96, fear=True, seed=3, feal=True)
    fe, fv = env.out["feal"], env.out["feal_valid"]
    env.reset()

    def poison():
        fe.fill_(float("nan"))
        fv.fill_(-1)

    poison()
    r = env.step()
    assert r.feal is fe and r.feal_valid is fv
    assert not bool(torch.isnan(fe).any()) and not bool((fv == -1).any())
    env.set_feal(fe, None)  # feal alone
    poison()
    r = env.step()
    assert r.feal_valid is None
    assert not bool(torch.isnan(fe).any()) and bool((fv == -1).all())
    env.set_feal(None, fv)  # the sets alone
    poison()
    r = env.step()
    assert r.feal is None
    assert bool(torch.isnan(fe).all()) and not bool((fv == -1).any())
    env.set_feal(None, None)  # off again
    poison()
    for _ in range(2):
        r = env.step()
    torch.cuda.synchronize()
    assert r.feal is None and r.feal_valid is None
    assert bool(torch.isnan(fe).all()) and bool((fv == -1).all())
    assert env.lib.gw_set_feal(None, None, None) == -1  # GW_ERR_ARG on a null env
    env.close()


@pytest.mark.parametrize("path", ["defer", "merged"])
def test_fear_off_is_an_error_and_weight_zero_works(path, monkeypatch):
    _set_path(monkeypatch, path)
    off = VecGridEnv("grid32", num_envs=8, fear=False, seed=3)
    buf = torch.full((8, off.N), float("nan"), dtype=torch.float64, device=off.device)
    sets = torch.full((8, off.N, 2), -1, dtype=torch.int16, device=off.device)
    assert off.lib.gw_set_feal(off.handle, buf.data_ptr(), sets.data_ptr()) == GW_ERR_STATE
    msg = off.lib.gw_last_error().decode()
    assert "FeAR" in msg and "fear_weight" in msg, msg
    assert off.lib.gw_set_feal(off.handle, None, None) == 0  # disarming is always fine
    off.reset()
    off.step()
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and bool((sets == -1).all())  # nothing that reads as "no agency"
    off.close()
    with pytest.raises(_lib.GwError, match="FeAR"):
        VecGridEnv("grid32", num_envs=8, fear=False, seed=3, feal=True)
    on = VecGridEnv("grid32", num_envs=64, fear=True, fear_weight=0.0, seed=3, feal=True)
    on.reset()
    on.out["feal"].fill_(float("nan"))
    for _ in range(3):
        r = on.step()
        assert torch.equal(r.shaped, r.reward)
    assert not bool(torch.isnan(r.feal).any())
    on.close()


def test_unjoined_fear_is_ordered_by_the_fear_fence(monkeypatch):
    _set_path(monkeypatch, "defer")
    env = VecGridEnv("grid32", num_envs=300, fear=True, seed=21, max_steps=5, debug=True, feal=True)
    assert env.kernel_path == "defer"
    env.set_obs_async(True, fear_async=True)
    env.reset()
    for t in range(7):
        cells = env.positions()
        env.out["feal"].fill_(float("nan"))
        r = env.step()
        env.fear_fence()
        want = env.fear_matrix(cells, r.actions, r.mdr, None)
        assert torch.equal(r.feal, want["feal"]), t
        sets = r.feal_valid.to(torch.int32) & 0xFFFF
        pc = sum((sets >> b) & 1 for b in range(9))
        assert torch.equal(pc[..., 0].to(torch.int32), want["feal_vm"]), t
        assert torch.equal(pc[..., 1].to(torch.int32), want["feal_va"]), t
    env.obs_fence()
    torch.cuda.synchronize()
    env.close()


def _captured_steps(graph):
    """1 eager step + 4 more (eager, or two replays of a 2-step capture) on the merged path with async
    obs; -> the feal / feal_valid of every step after the first, read after each step or replay."""
    env = VecGridEnv("grid32", num_envs=130, fear=True, seed=33, max_steps=3, feal=True)
    assert env.kernel_path == "merged"
    env.set_obs_async(True)
    env.reset()
    env.step()
    seen = []

    def grab():
        torch.cuda.synchronize()
        seen.append((env.out["feal"].clone(), env.out["feal_valid"].clone()))
        env.out["feal"].fill_(float("nan"))
        env.out["feal_valid"].fill_(-1)
        torch.cuda.synchronize()

    grab()
    if graph:
        g = env.capture_steps(2)
        for _ in range(2):
            g.replay()
            grab()
    else:
        for _ in range(2):
            env.step()
            env.step()
            grab()
    env.obs_fence()
    st = env.state()
    torch.cuda.synchronize()
    env.close()
    return seen, st


def test_captured_steps_replay_the_writes(monkeypatch):
    _set_path(monkeypatch, "merged")
    (a, sa), (b, sb) = _captured_steps(False), _captured_steps(True)
    assert len(a) == len(b) == 3
    for t, ((fa, va), (fb, vb)) in enumerate(zip(a, b)):
        assert not bool(torch.isnan(fb).any()) and not bool((vb == -1).any()), t  # the replay wrote them
        assert torch.equal(fa, fb) and torch.equal(va, vb), t
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n
    assert bool((a[-1][0] < 1).any())


def _accum(feal, active, totals, cnt):
    E, N = feal.shape
    _lib.check(_lib.load().gw_feal_accum(feal.data_ptr(), active.data_ptr() if active is not None else None, E, N,
                                         totals.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 8,
                                         torch.cuda.current_stream().cuda_stream), "gw_feal_accum")


@pytest.mark.parametrize("N", [3, 4, 8])
@pytest.mark.parametrize("E", [1, 255, 4096])
def test_feal_accum_op(E, N):
    rng = np.random.default_rng(E + N)
    x = rng.choice(np.arange(10.0) / (9 + 1e-6), (E, N))  # values like the kernel's
    act = (rng.random(E) < 0.6).astype(np.uint8)
    act[0] = 1
    feal, active = torch.as_tensor(x).cuda(), torch.as_tensor(act).cuda()
    got = []
    for _ in range(2):
        totals = torch.zeros(N, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        _accum(feal, active, totals, cnt)
        assert cnt.tolist() == [1, int(act.sum())]
        got.append(totals.cpu().numpy().copy())
        _accum(feal, None, totals, cnt)  # += on top, every env
        assert cnt.tolist() == [2, int(act.sum()) + E]
        got.append(totals.cpu().numpy().copy())
    np.testing.assert_array_equal(got[0], got[2])  # two launches: identical bits
    np.testing.assert_array_equal(got[1], got[3])
    xa = x[act != 0]
    err, bound = np.abs(got[0] - xa.sum(0)), xa.shape[0] * U * np.abs(xa).sum(0)
    print(f"E={E} N={N} masked: max |err| {err.max():.3e} bound {bound.min():.3e}")
    assert (err <= bound).all()
    both = np.concatenate([xa, x])
    assert (np.abs(got[1] - both.sum(0)) <= both.shape[0] * U * np.abs(both).sum(0)).all()
    assert torch.equal(active.cpu(), torch.as_tensor(act))  # the mask is read only


def test_feal_accum_graph_replay_equals_eager():
    E, N = 1000, 4
    rng = np.random.default_rng(7)
    feal = torch.as_tensor(rng.choice(np.arange(10.0) / (9 + 1e-6), (E, N))).cuda()
    active = torch.as_tensor((rng.random(E) < 0.5).astype(np.uint8)).cuda()
    eager_t = torch.zeros(N, dtype=torch.float64, device="cuda")
    eager_c = torch.zeros(2, dtype=torch.int64, device="cuda")
    for _ in range(3):
        _accum(feal, active, eager_t, eager_c)
    graph_t, graph_c = torch.zeros_like(eager_t), torch.zeros_like(eager_c)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _accum(feal, active, graph_t, graph_c)
    torch.cuda.synchronize()
    assert graph_c.tolist() == [0, 0]  # nothing ran at capture time
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(graph_t, eager_t) and torch.equal(graph_c, eager_c)
    assert eager_c.tolist() == [3, 3 * int(active.sum())]


def _window_rollout(graph, steps_eager=10):
    """The rollout of test_gpu_fear_alt._window_rollout (MLP actors on 11 x 11 windows, FeAR on, no dense
    obs, ring 16, E = 256, merged path) with the FeAL total on; graph: 2 eager steps + one 8-step graph."""
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    E, P, slots, G = 256, 11, 16, 8
    env = VecGridEnv("grid32", num_envs=E, fear=True, fear_weight=-5.0, max_steps=40, seed=42, stats=True,
                     obs=False, feal=True)
    assert env.kernel_path == "merged"
    actors = MultiAgentActors(env.K, P, P, arch="mlp", device=env.device, seed=0)
    ro = Rollout(env, actors, replay_slots=slots, training=True, seed=42, patch=P, feal=True)
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
            per_step.append(ro.step().feal.cpu().numpy().copy())
    ro.fence()
    tot = ro.totals()
    torch.cuda.synchronize()
    env.close()
    return tot, per_step, E


def test_rollout_feal_total_and_graph_replay(monkeypatch):
    _set_path(monkeypatch, "merged")
    tot, per_step, E = _window_rollout(False)
    assert tot["feal_steps"] == 10 and tot["feal_envs"] == 10 * E and tuple(tot["feal_sum"].shape) == (4,)
    x = np.concatenate(per_step)  # [10 E, N]
    got = tot["feal_sum"].numpy()
    err, bound = np.abs(got - x.sum(0)), x.shape[0] * U * np.abs(x).sum(0)
    print(f"rollout: max |err| {err.max():.3e} bound {bound.min():.3e} mean FeAL {got / tot['feal_envs']}")
    assert (err <= bound).all()
    assert (got > 0).all() and (got < 10 * E).all()
    tot_g, _, _ = _window_rollout(True)
    assert tot_g["feal_steps"] == 10 and tot_g["feal_envs"] == 10 * E
    assert torch.equal(tot_g["feal_sum"], tot["feal_sum"])  # graph replay == eager, bit for bit
    assert tot_g["fear"] == tot["fear"]
    from marlnav.rollout import Rollout
    plain = VecGridEnv("grid32", num_envs=8, fear=True, seed=1)
    with pytest.raises(ValueError):
        Rollout(plain, None, feal=True)
    plain.close()


def test_evaluate_feal():
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("grid32")
    E, T = 64, 24
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    r = evaluate(actors, sc, episodes=E, max_steps=T, fear=True, seed=11, record_actions=True, feal=True)
    mean = r["feal"].numpy()
    assert mean.shape == (sc.N,) and mean.dtype == np.float64
    assert "feal" not in evaluate(actors, sc, episodes=E, max_steps=8, fear=True, seed=11)
    with pytest.raises(ValueError):
        evaluate(actors, sc, episodes=E, max_steps=8, fear=False, feal=True)
    # the recorded actions replayed, FeAL folded on the host over the episodes still running
    env = VecGridEnv(sc, num_envs=E, fear=True, max_steps=T, auto_reset=False, seed=11, feal=True)
    env.reset()
    active = np.ones(E, bool)
    total, abs_total, terms = np.zeros(sc.N), np.zeros(sc.N), 0
    for a in r["actions"]:
        s = env.step(a)
        fe = s.feal.cpu().numpy()
        total += fe[active].sum(0)
        abs_total += np.abs(fe[active]).sum(0)
        terms += int(active.sum())
        active &= s.done.cpu().numpy() == 0
    env.close()
    assert terms == r["steps"] and (abs_total > 0).all()
    # n = the env-steps summed, + 2 for the division by steps and the multiplication back
    err = np.abs(mean * r["steps"] - total)
    print(f"evaluate: mean FeAL {mean}, max |err| {err.max():.3e}, bound {((terms + 2) * U * abs_total).min():.3e}")
    assert (err <= (terms + 2) * U * abs_total).all()
    assert (mean > 0).all() and (mean <= 1).all()


def test_facade_info_and_customeval_flag(tmp_path, capsys):
    """CustomMAEnv(feal=True): info["feal"] is the step's FeAL of the N world agents; the default dict
    is unchanged.  customeval.py --feal prints the mean FeAL per agent under the reference's totals,
    which FeAR on / off does not change."""
    from custom.ma_customenv import CustomMAEnv
    env = CustomMAEnv(render=False, fear=True, seed=123, feal=True)
    plain = CustomMAEnv(render=False, fear=True, seed=123)
    env.reset()
    plain.reset()
    N = env.scenario.N
    for t in range(5):
        pos = env._env.positions()
        _, rew, _, _, info = env.step([t % 9, (2 * t + 1) % 9])
        _, rew_p, _, _, info_p = plain.step([t % 9, (2 * t + 1) % 9])
        assert isinstance(info["feal"], list) and len(info["feal"]) == N
        act = [a for _, a in env.Action4Agents]
        mdr = [m for _, m in env.MdR4Agents]
        want = env._env.fear_matrix(pos, [act], [mdr], None)["feal"][0].cpu().tolist()
        assert info["feal"] == want, t
        assert "feal" not in info_p and rew == rew_p
        assert {k: v for k, v in info.items() if k not in ("feal",) and not k.startswith("agent_")} == \
               {k: v for k, v in info_p.items() if not k.startswith("agent_")}
    with pytest.raises(ValueError):
        CustomMAEnv(render=False, fear=False, feal=True)

    import customeval
    from marlnav.maddpg import MADDPG
    sc = S.builtin("grid32")
    ck = str(tmp_path / "m.safetensors")
    MADDPG(sc.K, sc.H, sc.W, device=torch.device("cuda"), seed=3).save(ck)
    args = ["--checkpoint", ck, "--scenario", "grid32", "--episodes", "16", "--train-steps", "12"]
    customeval.main(args)
    base = capsys.readouterr().out.strip().splitlines()
    customeval.main(args + ["--feal"])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(base) == 3 and out[:3] == base
    assert out[3].startswith("Mean FeAL per agent: ")
    vals = [float(v) for v in out[3].split(": ")[1].split()]
    assert len(vals) == sc.N and all(0 < v <= 1 for v in vals)
