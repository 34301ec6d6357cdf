"""The full N x N responsibility matrix from the step (gw_set_fear_full, VecGridEnv(fear_full=True)).

1. The reference's own Responsibility.FeAR known-answer cases (tests/golden/fear_matrix.npz, recorded from
   custom/Responsibility.py:57-132) through the STEP and fear_full_kernel, one case per env and one step,
   on the defer (wide / narrow FeAR blocks) and merged paths: the cases whose in_list is all ones and
   whose MdR row is one constant, split by that constant, each split on a scenario whose MdR table is that
   constant (as test_gpu_feal._scenario).  resp bit for bit, the popcounts of resp_valid against vm / va,
   the diagonal zero; all 118 cases, none left out; negative and positive entries both compared.
2. Native Philox rollouts (grid32 N = 4, grid64_n8 N = 8: the pair-list world; E = 7: a partial last
   block, E = 1; auto-reset on, the step cap 4 makes every env reset inside the 6 steps): every step
   against gw_fear_matrix(in_list = NULL) and the C oracle on the pre-step snapshot.
3. Invariants: the action sets are FeAL's others-actual sets of the affected agent; an actor on its MdR
   has a zero row and equal sets; an RL actor with every agent within Manhattan 5 has the step's
   fear_row as its row.
4. Result-neutral; disarming stops the writes; one pointer alone; FeAR off: GW_ERR_STATE; unjoined FeAR
   (fear_fence); captured steps on the merged path; gw_count_sims rises by 9 N + 9 (N - 1) popc(diff).
5. Rollout(resp_full=True) eager == graph replay, evaluate(resp_full=True), the facade's
   info["fear_matrix"] and customeval.py --resp-full.

Summation bound (5): any order of summing n f64 terms x_i differs from the exact sum by at most
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
    """resp_valid / feal_valid (int16 views of the u16 bit sets) as non-negative ints."""
    return t.cpu().numpy().view(np.uint16).astype(np.int64)


def _scenario(region2d: np.ndarray, N: int, mdr_value: int) -> S.CompiledScenario:
    """A scenario on the case's map with K = 2 RL agents and the constant MdR ``mdr_value`` in every
    cell (as test_gpu_feal._scenario)."""
    base = S.builtin("level3")
    H, W = region2d.shape
    free = np.flatnonzero(region2d.reshape(-1) == 1).astype(np.int32)
    return dataclasses.replace(
        base, name="fear_full_kat", H=H, W=W, N=N, K=K, region=(region2d != 0).astype(np.uint8).reshape(-1),
        policy_id=np.zeros(H * W, np.uint8), policy_keys=base.policy_keys[:1], policy_p=base.policy_p[:1],
        policy_cdf=base.policy_cdf[:1], mdr=np.full(H * W, mdr_value, np.uint8), apples=free[:K].copy(),
        free_cells=free, okmask=S.okmask_table(region2d), action_mask=S.action_mask_table(region2d))


def _kat_cases(name):
    z = np.load(os.path.join(GOLD, "fear_matrix.npz"))
    d = {k.split("/", 1)[1]: np.asarray(z[k]) for k in z.files if k.startswith(name + "/")}
    sel = (d["in_list"] != 0).all(1) & (d["mdr"] == d["mdr"][:, :1]).all(1)
    return d, np.flatnonzero(sel)


def _poison(env):
    env.out["resp_full"].fill_(float("nan"))
    env.out["resp_valid"].fill_(-1)


@pytest.mark.parametrize("path", sorted(KERNEL_PATHS))
def test_reference_kats_through_the_step(path, monkeypatch):
    _set_path(monkeypatch, path)
    compared = negative = positive = 0
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
                             max_steps=1000, debug=True, fear_full=True)
            try:
                assert env.kernel_path == KERNEL_PATHS[path]["GW_KERNEL"]
                env.reset(spawn=torch.as_tensor(d["loc"][idx].astype(np.int32)))
                _poison(env)
                act = d["act"][idx].astype(np.int32)
                r = env.step(act[:, :K].copy(), act[:, K:].copy())
                torch.cuda.synchronize()
                np.testing.assert_array_equal(r.actions.cpu().numpy(), act)
                assert (r.mdr.cpu().numpy() == v).all()
                rf, rv = r.resp_full.cpu().numpy(), _sets(r.resp_valid)
                assert rf.shape == (E, N, N) and rv.shape == (E, N, N, 2) and (rv < 512).all()
                print(f"{name} mdr {v}: {E} cases, resp differs in {int((rf != d['resp'][idx]).sum())} of {rf.size}")
                np.testing.assert_array_equal(rf, d["resp"][idx], err_msg=f"{name} mdr {v}: resp")
                np.testing.assert_array_equal(_popcount(rv[..., 0]), d["vm"][idx], err_msg=f"{name}: vm")
                np.testing.assert_array_equal(_popcount(rv[..., 1]), d["va"][idx], err_msg=f"{name}: va")
                dg = np.arange(N)
                assert (rf[:, dg, dg] == 0.0).all() and not np.signbit(rf[:, dg, dg]).any()
                assert (rv[:, dg, dg] == 0).all()
                compared += E
                negative += int((rf < 0).sum())
                positive += int((rf > 0).sum())
                values.add(int(v))
            finally:
                env.close()
    assert compared == 118, compared
    assert negative == 75 and positive > 0, (negative, positive)
    assert values == {0, 1, 2, 3, 4, 8}


def _rollout_checks(scen, E, path_env):
    """6 native steps; every step's resp_full / resp_valid against gw_fear_matrix and the C oracle on
    the pre-step snapshot.  -> done envs seen, non-zero entries seen."""
    sc = S.builtin(scen)
    N, H, W = sc.N, sc.H, sc.W
    region = np.asarray(sc.region).reshape(H, W)
    env = VecGridEnv(sc, num_envs=E, fear=True, fear_weight=-5.0, seed=5, max_steps=4, auto_reset=True,
                     debug=True, fear_full=True)
    assert env.kernel_path == path_env
    env.reset()
    resets = nonzero = 0
    dg = np.arange(N)
    try:
        for t in range(6):
            cells = env.positions().cpu().numpy().astype(np.int32)  # the pre-step (pre-reset) world
            _poison(env)
            r = env.step()
            torch.cuda.synchronize()
            acts, mdr = r.actions.cpu().numpy(), r.mdr.cpu().numpy()
            rf, rv = r.resp_full.cpu().numpy(), _sets(r.resp_valid)
            vm, va = _popcount(rv[..., 0]), _popcount(rv[..., 1])
            assert not np.isnan(rf).any() and (rv < 512).all()
            assert (rf[:, dg, dg] == 0.0).all() and (rv[:, dg, dg] == 0).all()
            fm = {k: v.cpu().numpy() for k, v in env.fear_matrix(cells, acts, mdr, None).items()}
            np.testing.assert_array_equal(rf, fm["resp"], err_msg=f"step {t}: resp vs gw_fear_matrix")
            np.testing.assert_array_equal(vm, fm["vm"], err_msg=f"step {t}")
            np.testing.assert_array_equal(va, fm["va"], err_msg=f"step {t}")
            for e in range(E):
                o = O.fear_matrix(H, W, region, cells[e], acts[e], mdr[e], None)
                np.testing.assert_array_equal(rf[e], o["resp"], err_msg=f"step {t} env {e}: resp vs oracle")
                np.testing.assert_array_equal(vm[e], o["vm"], err_msg=f"step {t} env {e}")
                np.testing.assert_array_equal(va[e], o["va"], err_msg=f"step {t} env {e}")
            resets += int(r.done.sum())
            nonzero += int((rf != 0).sum())
    finally:
        env.close()
    return resets, nonzero


@pytest.mark.parametrize("path", ["defer", "merged"])
@pytest.mark.parametrize("scen,E", [("grid32", 7), ("grid32", 1), ("grid64_n8", 7), ("grid64_n8", 1)])
def test_native_rollout_matches_fear_matrix_and_oracle(scen, E, path, monkeypatch):
    _set_path(monkeypatch, path)
    resets, _ = _rollout_checks(scen, E, KERNEL_PATHS[path]["GW_KERNEL"])
    assert resets >= E, "no env auto-reset within the 6 steps"  # the step cap is 4: the pre-reset rule ran


@pytest.mark.parametrize("path", ["defer", "merged"])
@pytest.mark.parametrize("scen", ["level3", "grid64_n8"])
def test_invariants(scen, path, monkeypatch):
    """level3 (10 x 16, N = 4), seed 11, E = 64: the C oracle's rollout of this seed has RL actors with
    every agent within Manhattan 5 in its first 6 steps, so the fear_row comparison runs there (asserted
    below).  On grid64_n8 (64 x 64, N = 8) eight agents within distance 5 of one of them are not to be
    expected: that case runs the other two invariants on the pair-list world, and the fear_row comparison
    only for the rows that happen to qualify, possibly none."""
    _set_path(monkeypatch, path)
    sc = S.builtin(scen)
    N, W, E = sc.N, sc.W, 64
    env = VecGridEnv(sc, num_envs=E, fear=True, fear_weight=-5.0, seed=11, max_steps=4, auto_reset=True,
                     debug=True, feal=True, fear_full=True, fear_rows=True)
    env.reset()
    on_mdr = full_rows = 0
    off = ~np.eye(N, dtype=bool)
    try:
        for t in range(6):
            cells = env.positions().cpu().numpy().astype(np.int64)
            _poison(env)
            r = env.step()
            torch.cuda.synchronize()
            acts, mdr = r.actions.cpu().numpy(), r.mdr.cpu().numpy()
            rf, rv = r.resp_full.cpu().numpy(), _sets(r.resp_valid)
            fv = _sets(r.feal_valid)
            # the action sets are those of FeAL's others-actual variant of the affected agent, for every actor
            want = np.broadcast_to(fv[:, None, :, 1], (E, N, N))
            np.testing.assert_array_equal(rv[..., 1][:, off], want[:, off], err_msg=f"step {t}")
            # an actor on its MdR: a zero row and equal sets
            same = acts == mdr  # [E, N]
            assert (rf[same] == 0.0).all() and not np.signbit(rf[same]).any(), t
            np.testing.assert_array_equal(rv[same][..., 0], rv[same][..., 1], err_msg=f"step {t}")
            on_mdr += int(same.sum())
            # an RL actor with every agent within Manhattan 5: the step's close set is full
            row, col = cells // W, cells % W
            fr = r.fear_row.cpu().numpy()
            for k in range(sc.K):
                dist = np.abs(row - row[:, k:k + 1]) + np.abs(col - col[:, k:k + 1])
                full = (dist <= 5).all(1)
                np.testing.assert_array_equal(rf[full, k], fr[full, k], err_msg=f"step {t} actor {k}")
                full_rows += int(full.sum())
    finally:
        env.close()
    assert on_mdr > 0
    if scen == "level3":  # the map chosen for it; see the docstring for grid64_n8
        assert full_rows > 0, "no RL actor had a full close set: the fear_row comparison did not run"


NEUTRAL_SKIP = ("resp_full", "resp_valid")


def _neutral_run(fear_full, fear_async):
    env = VecGridEnv("grid32", num_envs=512, fear=True, fear_weight=-5.0, seed=9, max_steps=6, debug=True,
                     stats=True, fear_full=fear_full)
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
def test_fear_full_is_result_neutral(path, fear_async, monkeypatch):
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
    env = VecGridEnv("grid32", num_envs=96, fear=True, seed=3, fear_full=True)
    rf, rv = env.out["resp_full"], env.out["resp_valid"]
    env.reset()

    def poison():
        rf.fill_(float("nan"))
        rv.fill_(-1)

    poison()
    r = env.step()
    assert r.resp_full is rf and r.resp_valid is rv
    assert not bool(torch.isnan(rf).any()) and not bool((rv == -1).any())
    env.set_fear_full(rf, None)  # the matrix alone
    poison()
    r = env.step()
    assert r.resp_valid is None
    assert not bool(torch.isnan(rf).any()) and bool((rv == -1).all())
    env.set_fear_full(None, rv)  # the sets alone
    poison()
    r = env.step()
    assert r.resp_full is None
    assert bool(torch.isnan(rf).all()) and not bool((rv == -1).any())
    env.set_fear_full(None, None)  # off again
    poison()
    for _ in range(2):
        r = env.step()
    torch.cuda.synchronize()
    assert r.resp_full is None and r.resp_valid is None
    assert bool(torch.isnan(rf).all()) and bool((rv == -1).all())
    assert env.lib.gw_set_fear_full(None, None, None) == -1  # GW_ERR_ARG on a null env
    env.close()


@pytest.mark.parametrize("path", ["defer", "merged"])
def test_fear_off_is_an_error(path, monkeypatch):
    _set_path(monkeypatch, path)
    off = VecGridEnv("grid32", num_envs=8, fear=False, seed=3)
    N = off.N
    buf = torch.full((8, N, N), float("nan"), dtype=torch.float64, device=off.device)
    sets = torch.full((8, N, N, 2), -1, dtype=torch.int16, device=off.device)
    assert off.lib.gw_set_fear_full(off.handle, buf.data_ptr(), sets.data_ptr()) == GW_ERR_STATE
    msg = off.lib.gw_last_error().decode()
    assert "FeAR" in msg and "fear_weight" in msg, msg
    assert off.lib.gw_set_fear_full(off.handle, None, None) == 0  # disarming is always fine
    off.reset()
    off.step()
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and bool((sets == -1).all())
    off.close()
    with pytest.raises(_lib.GwError, match="FeAR"):
        VecGridEnv("grid32", num_envs=8, fear=False, seed=3, fear_full=True)


def test_unjoined_fear_is_ordered_by_the_fear_fence(monkeypatch):
    _set_path(monkeypatch, "defer")
    env = VecGridEnv("grid32", num_envs=300, fear=True, seed=21, max_steps=5, debug=True, fear_full=True)
    assert env.kernel_path == "defer"
    env.set_obs_async(True, fear_async=True)
    env.reset()
    for t in range(7):
        cells = env.positions()
        env.out["resp_full"].fill_(float("nan"))
        r = env.step()
        env.fear_fence()
        want = env.fear_matrix(cells, r.actions, r.mdr, None)
        assert torch.equal(r.resp_full, want["resp"]), t
        sets = r.resp_valid.to(torch.int32) & 0xFFFF
        pc = sum((sets >> b) & 1 for b in range(9))
        assert torch.equal(pc[..., 0].to(torch.int32), want["vm"]), t
        assert torch.equal(pc[..., 1].to(torch.int32), want["va"]), t
    env.obs_fence()
    torch.cuda.synchronize()
    env.close()


def _captured_steps(graph):
    """1 eager step + 4 more (eager, or two replays of a 2-step capture) on the merged path with async
    obs; -> the resp_full / resp_valid of every step after the first, read after each step or replay."""
    env = VecGridEnv("grid32", num_envs=130, fear=True, seed=33, max_steps=3, fear_full=True)
    assert env.kernel_path == "merged"
    env.set_obs_async(True)
    env.reset()
    env.step()
    seen = []

    def grab():
        torch.cuda.synchronize()
        seen.append((env.out["resp_full"].clone(), env.out["resp_valid"].clone()))
        _poison(env)
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
    assert bool((a[-1][0] != 0).any())


@pytest.mark.parametrize("path", ["defer", "merged"])
@pytest.mark.parametrize("scen,E", [("grid32", 133), ("grid64_n8", 9)])
def test_sims_count_is_the_deduplicated_task_set(scen, E, path, monkeypatch):
    """Two envs of one seed, one armed: the armed one's gw_count_sims counter runs ahead by exactly
    sum_e 9 N + 9 (N - 1) popc(diff_e), diff_e = the agents whose action is not their MdR (host)."""
    _set_path(monkeypatch, path)
    counts, want = {}, 0
    for armed in (False, True):
        env = VecGridEnv(scen, num_envs=E, fear=True, seed=17, max_steps=4, debug=True, fear_full=armed)
        ctr = torch.zeros(1, dtype=torch.int64, device=env.device)
        env.reset()
        env.count_sims(ctr)
        for _ in range(5):
            r = env.step()
            if armed:
                d = (r.actions != r.mdr).sum(1).cpu().numpy().astype(np.int64)  # popc(diff) per env
                want += int((9 * env.N + 9 * (env.N - 1) * d).sum())
                assert (d >= 0).all() and (d <= env.N).all()
        torch.cuda.synchronize()
        env.count_sims(None)
        counts[armed] = int(ctr.item())
        N = env.N
        env.close()
    got = counts[True] - counts[False]
    print(f"{scen} E={E}: {got} sims over 5 steps, {got / (5 * E):.1f} per env (at most {9 * N * N})")
    assert got == want
    assert 9 * N * 5 * E <= got <= 9 * N * N * 5 * E


def _window_rollout(graph, steps_eager=10):
    """The rollout of test_gpu_feal._window_rollout (MLP actors on 11 x 11 windows, FeAR on, no dense obs,
    ring 16, E = 256, merged path) with the N x N total on; graph: 2 eager steps + one 8-step graph."""
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    E, P, slots, G = 256, 11, 16, 8
    env = VecGridEnv("grid32", num_envs=E, fear=True, fear_weight=-5.0, max_steps=40, seed=42, stats=True,
                     obs=False, fear_full=True)
    assert env.kernel_path == "merged"
    actors = MultiAgentActors(env.K, P, P, arch="mlp", device=env.device, seed=0)
    ro = Rollout(env, actors, replay_slots=slots, training=True, seed=42, patch=P, resp_full=True)
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
            per_step.append(ro.step().resp_full.cpu().numpy().copy())
    ro.fence()
    tot = ro.totals()
    torch.cuda.synchronize()
    env.close()
    return tot, per_step, E


def test_rollout_total_and_graph_replay(monkeypatch):
    _set_path(monkeypatch, "merged")
    tot, per_step, E = _window_rollout(False)
    assert tot["resp_full_steps"] == 10 and tuple(tot["resp_full"].shape) == (4, 4)
    x = np.concatenate(per_step)  # [10 E, N, N]
    got = tot["resp_full"].numpy()
    err, bound = np.abs(got - x.sum(0)), x.shape[0] * U * np.abs(x).sum(0)
    print(f"rollout: max |err| {err.max():.3e}, bound (off-diagonal min) {bound[~np.eye(4, dtype=bool)].min():.3e}")
    assert (err <= bound).all()
    assert (np.diag(got) == 0).all() and (got != 0).any()
    tot_g, _, _ = _window_rollout(True)
    assert tot_g["resp_full_steps"] == 10
    assert torch.equal(tot_g["resp_full"], tot["resp_full"])  # graph replay == eager, bit for bit
    assert tot_g["fear"] == tot["fear"]
    from marlnav.rollout import Rollout
    plain = VecGridEnv("grid32", num_envs=8, fear=True, seed=1)
    with pytest.raises(ValueError):
        Rollout(plain, None, resp_full=True)
    plain.close()


def test_evaluate_resp_full():
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("grid32")
    E, T = 64, 24
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    r = evaluate(actors, sc, episodes=E, max_steps=T, fear=True, seed=11, record_actions=True, resp_full=True)
    got = r["resp_full"].numpy()
    assert got.shape == (sc.N, sc.N) and got.dtype == np.float64
    assert r["resp_full_steps"] >= len(r["actions"])  # the early-stop check runs every 8 steps
    assert "resp_full" not in evaluate(actors, sc, episodes=E, max_steps=8, fear=True, seed=11)
    with pytest.raises(ValueError):
        evaluate(actors, sc, episodes=E, max_steps=8, fear=False, resp_full=True)
    # the recorded actions replayed, the matrices folded on the host over the episodes still running
    env = VecGridEnv(sc, num_envs=E, fear=True, max_steps=T, auto_reset=False, seed=11, fear_full=True)
    env.reset()
    active = np.ones(E, bool)
    total, abs_total, terms = np.zeros((sc.N, sc.N)), np.zeros((sc.N, sc.N)), 0
    for a in r["actions"]:
        s = env.step(a)
        m = s.resp_full.cpu().numpy()
        total += m[active].sum(0)
        abs_total += np.abs(m[active]).sum(0)
        terms += int(active.sum())
        active &= s.done.cpu().numpy() == 0
    env.close()
    assert terms == r["steps"] and (abs_total[~np.eye(sc.N, dtype=bool)] > 0).all()
    err = np.abs(got - total)
    print(f"evaluate: sum\n{got}\nmax |err| {err.max():.3e}, bound max {(terms * U * abs_total).max():.3e}")
    assert (err <= terms * U * abs_total).all()
    assert (np.diag(got) == 0).all()


def test_facade_info_and_customeval_flag(tmp_path, capsys):
    """CustomMAEnv(fear_full=True): info["fear_matrix"] is the step's N x N matrix; the default dict is
    unchanged.  customeval.py --resp-full prints the matrix under the reference's totals."""
    from custom.ma_customenv import CustomMAEnv
    env = CustomMAEnv(render=False, fear=True, seed=123, fear_full=True)
    plain = CustomMAEnv(render=False, fear=True, seed=123)
    env.reset()
    plain.reset()
    N = env.scenario.N
    for t in range(5):
        pos = env._env.positions()
        _, rew, _, _, info = env.step([t % 9, (2 * t + 1) % 9])
        _, rew_p, _, _, info_p = plain.step([t % 9, (2 * t + 1) % 9])
        m = info["fear_matrix"]
        assert isinstance(m, list) and len(m) == N and all(isinstance(row, list) and len(row) == N for row in m)
        act = [a for _, a in env.Action4Agents]
        mdr = [x for _, x in env.MdR4Agents]
        want = env._env.fear_matrix(pos, [act], [mdr], None)["resp"][0].cpu().tolist()
        assert m == want, t
        assert "fear_matrix" not in info_p and rew == rew_p
        assert {k: v for k, v in info.items() if k != "fear_matrix" and not k.startswith("agent_")} == \
               {k: v for k, v in info_p.items() if not k.startswith("agent_")}
    with pytest.raises(ValueError):
        CustomMAEnv(render=False, fear=False, fear_full=True)

    import customeval
    from marlnav.maddpg import MADDPG
    sc = S.builtin("grid32")
    ck = str(tmp_path / "m.safetensors")
    MADDPG(sc.K, sc.H, sc.W, device=torch.device("cuda"), seed=3).save(ck)
    args = ["--checkpoint", ck, "--scenario", "grid32", "--episodes", "16", "--train-steps", "12"]
    customeval.main(args)
    base = capsys.readouterr().out.strip().splitlines()
    customeval.main(args + ["--resp-full"])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(base) == 3 and out[:3] == base
    assert out[3].startswith("Responsibility matrix") and len(out) == 4 + sc.N
    rows = [[float(v) for v in line.split()] for line in out[4:]]
    assert all(len(row) == sc.N for row in rows)
    assert all(rows[i][i] == 0.0 for i in range(sc.N)) and any(v != 0.0 for row in rows for v in row)
