"""Responsibility footprints on the GPU (gw_resp_footprint_accum, csrc/resp_footprint.hip; include/rollout_ops.h).

Shapes, the smallest at which the kernel can go wrong: grid32 with E = 37 and R = 5 (N = 4; 592 threads: a tail
block, waves that straddle a pair boundary), grid64_n8 with E = 5 and R = 15 (N = 8: the largest count array and
the largest R), the 2 x 2, N = 2 open map of tests/_shapes.py with E = 33 and R = 1 (every offset is near: the
far bin stays 0) and the 13 x 3 open map with R = 2 (W taken for H shows).  Six native steps each with
fear_full=True, debug=True (the step's actions and crash_bits) and a step cap of 4, so that auto-resets fall
inside the run; one run per case, shared by the tests and never modified.

1. counts / visits equal np.add.at of the rule (tests/_resp_footprint_ref.py) exactly; the kept steps folded
   twice give exactly twice that; plane 0 over action and offset equals gw_resp_map_accum's plane 0 over cells.
2. Orientation on the 13 x 3 and 1 x 8 maps, synthetic N = 2 inputs.
3. The far bin: a second fold of grid32 with R = 1.
4. The crash plane; crash_bits NULL leaves plane 1 alone.
5. The active mask.  6. Clamped cells and actions.
7. The derived footprint against math.fsum of the steps' resp_full within n * 2^-53 * sum|x|.
8. Argument errors.  9. Rollout(resp_footprint=5): eager joined = the host fold, unjoined = joined, a graph
   replay = the eager run.  10. evaluate(resp_footprint=5) and customeval.py --resp-footprint."""
import functools
import math

import numpy as np
import pytest
import torch

import marlnav
from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv

import _resp_footprint_ref as F
import _shapes
from test_resp_footprint_cpu import check_orientation, orientation_inputs

pytestmark = pytest.mark.gpu
CASES = {"grid32": ("grid32", 37, 5), "grid64_n8": ("grid64_n8", 5, 15), "open2x2_n2": ("2x2_n2_k2", 33, 1),
         "open13x3_n3": ("13x3_n3_k1", 33, 2)}
STEPS = 6
GW_ERR_ARG = -1


def _scenario(name):
    return _shapes.scenario(name) if name in _shapes.BY_ID else S.builtin(name)


def _sets(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint16).astype(np.int64)


def _rv(sets, dev):
    return torch.from_numpy(sets.astype(np.uint16).view(np.int16)).to(dev)


def _buffers(dev, R, fill=0):
    return (torch.full((2, 9, F.n_offsets(R), 10, 10), fill, dtype=torch.int64, device=dev),
            torch.full((9,), fill, dtype=torch.int64, device=dev))


@functools.lru_cache(maxsize=None)
def _run(case):
    """-> dict: per-step host copies (cells, sets, resp_full, actions, crash_bits), the device folds' results."""
    name, E, R = CASES[case]
    sc = _scenario(name)
    env = VecGridEnv(sc, num_envs=E, fear=True, fear_weight=-5.0, seed=5, max_steps=4, auto_reset=True,
                     fear_full=True, debug=True)
    try:
        HW, N, dev = sc.H * sc.W, sc.N, env.device
        env.reset()
        counts, visits = _buffers(dev, R)
        m_counts, m_visits = _buffers(dev, R)
        z_counts, z_visits = _buffers(dev, R, fill=7)
        n_counts, n_visits = _buffers(dev, R)
        n_counts[1] = 7  # crash_bits NULL: this plane must stay as it is
        map_counts = torch.zeros((2, HW, 10, 10), dtype=torch.int64, device=dev)
        mask = (torch.arange(E, device=dev) % 2 == 0).to(torch.uint8)
        none = torch.zeros(E, dtype=torch.uint8, device=dev)
        cells_dev = torch.empty((N, E), dtype=torch.int32, device=dev)
        steps, resets = [], 0
        for _ in range(STEPS):
            env.copy_pos(cells_dev)
            r = env.step()
            a = (r.resp_valid, cells_dev, r.actions)
            env.resp_footprint_accum(*a, counts, visits, crash_bits=r.crash_bits, radius=R)
            env.resp_footprint_accum(*a, m_counts, m_visits, crash_bits=r.crash_bits, active=mask, radius=R)
            env.resp_footprint_accum(*a, z_counts, z_visits, crash_bits=r.crash_bits, active=none, radius=R)
            env.resp_footprint_accum(*a, n_counts, n_visits, radius=R)
            env.resp_map_accum(r.resp_valid, cells_dev, map_counts)
            torch.cuda.synchronize()
            steps.append((cells_dev.cpu().numpy().copy(), _sets(r.resp_valid), r.resp_full.cpu().numpy().copy(),
                          r.actions.cpu().numpy().copy(), r.crash_bits.cpu().numpy().copy()))
            resets += int(r.done.sum())
        # the kept steps uploaded again, each folded twice into zeroed buffers, with crash bits set by hand
        # (every agent of every third env, then one agent per env) so that the plane is exercised in any case
        hand = [((np.arange(E) % 3 == 0) * ((1 << N) - 1) | (1 << (np.arange(E) + t) % N)).astype(np.uint8)
                for t in range(STEPS)]
        d_counts, d_visits = _buffers(dev, R)
        r1_counts, r1_visits = _buffers(dev, 1)
        for (cells, sets, _, acts, crash), hb in zip(steps, hand):
            up = (_rv(sets, dev), torch.from_numpy(cells).to(dev), torch.from_numpy(acts).to(dev))
            for _ in range(2):
                env.resp_footprint_accum(*up, d_counts, d_visits, crash_bits=torch.from_numpy(hb).to(dev), radius=R)
            env.resp_footprint_accum(*up, r1_counts, r1_visits, crash_bits=torch.from_numpy(crash).to(dev), radius=1)
        # the clamp call: cells of -1 and HW, actions of -1, 9 and 2^31 - 1
        cells, sets, _, acts, crash = steps[-1]
        bad_cells, bad_acts = cells.copy(), acts.copy()
        bad_cells.reshape(-1)[::3] = -1
        bad_cells.reshape(-1)[1::3] = HW
        bad_acts.reshape(-1)[::4] = -1
        bad_acts.reshape(-1)[1::4] = 9
        bad_acts.reshape(-1)[2::4] = 2 ** 31 - 1
        c_counts, c_visits = _buffers(dev, R)
        env.resp_footprint_accum(_rv(sets, dev), torch.from_numpy(bad_cells).to(dev), torch.from_numpy(bad_acts).to(dev),
                                 c_counts, c_visits, crash_bits=torch.from_numpy(crash).to(dev), radius=R)
        torch.cuda.synchronize()
        g = lambda t: t.cpu().numpy()  # noqa: E731
        return dict(sc=sc, E=E, N=N, R=R, W=sc.W, HW=HW, steps=steps, resets=resets, hand=hand,
                    mask=g(mask).astype(bool), counts=g(counts), visits=g(visits), m_counts=g(m_counts),
                    m_visits=g(m_visits), z_counts=g(z_counts), z_visits=g(z_visits), n_counts=g(n_counts),
                    n_visits=g(n_visits), d_counts=g(d_counts), d_visits=g(d_visits), r1_counts=g(r1_counts),
                    r1_visits=g(r1_visits), map_counts=g(map_counts), bad_cells=bad_cells, bad_acts=bad_acts,
                    c_counts=g(c_counts), c_visits=g(c_visits))
    finally:
        env.close()


@functools.lru_cache(maxsize=None)
def _host_fold(case, masked=False, hand=False, R=None):
    d = _run(case)
    R = d["R"] if R is None else R
    counts, visits = np.zeros((2, 9, F.n_offsets(R), 10, 10), np.int64), np.zeros(9, np.int64)
    for t, (cells, sets, _, acts, crash) in enumerate(d["steps"]):
        c, v = F.fold(sets, cells, acts, d["W"], d["HW"], R, crash_bits=d["hand"][t] if hand else crash,
                      active=d["mask"] if masked else None)
        counts += c
        visits += v
    return counts, visits


@pytest.mark.parametrize("case", sorted(CASES))
def test_counts_and_visits(case):
    d = _run(case)
    E, N = d["E"], d["N"]
    assert d["resets"] >= E, "no env auto-reset within the run"  # the step cap is 4
    want_c, want_v = _host_fold(case)
    np.testing.assert_array_equal(d["counts"], want_c)
    np.testing.assert_array_equal(d["visits"], want_v)
    assert d["counts"][0].sum() == STEPS * E * N * (N - 1) and d["visits"].sum() == STEPS * E * N
    assert (d["visits"] > 0).sum() >= 2, "the run reached a single action"
    hand_c, hand_v = _host_fold(case, hand=True)
    np.testing.assert_array_equal(d["d_counts"], 2 * hand_c, err_msg="folding twice is not twice the fold")
    np.testing.assert_array_equal(d["d_visits"], 2 * hand_v)
    np.testing.assert_array_equal(d["counts"][0].sum((0, 1)), d["map_counts"][0].sum(0),
                                  err_msg="(vm, va) totals differ from gw_resp_map_accum's")
    if case == "open2x2_n2":  # every offset of a 2 x 2 map is within R = 1
        assert (want_c[:, :, -1] == 0).all() and (d["counts"][:, :, -1] == 0).all()


@pytest.mark.parametrize("H,W", [(13, 3), (1, 8)])
def test_orientation(H, W):
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    E, R = 5, 2
    sets, cells, actions, off = orientation_inputs(H, W, E)
    counts, visits = _buffers(dev, R)
    rv, cd, ad = _rv(sets, dev), torch.from_numpy(cells).to(dev), torch.from_numpy(actions).to(dev)
    st = lib.gw_resp_footprint_accum(rv.data_ptr(), cd.data_ptr(), ad.data_ptr(), None, None, counts.data_ptr(),
                                     visits.data_ptr(), E, 2, H, W, R, torch.cuda.current_stream(dev).cuda_stream)
    assert st == 0, lib.gw_last_error()
    torch.cuda.synchronize()
    check_orientation(counts.cpu().numpy(), visits.cpu().numpy(), E, R, off)
    assert int(counts[1].sum()) == 0


def test_far_bin():
    d = _run("grid32")
    want5, _ = _host_fold("grid32")
    want1, want1_v = _host_fold("grid32", R=1)
    # the seed gives both kinds of pair at R = 1 (asserted on the reference fold, not on the kernel's output)
    assert want1[0, :, :-1].sum() > 0 and want1[0, :, -1].sum() > 0 and want5[0, :, -1].sum() > 0
    np.testing.assert_array_equal(d["r1_counts"], want1)
    np.testing.assert_array_equal(d["r1_visits"], want1_v)
    np.testing.assert_array_equal(d["r1_counts"].sum(2), d["counts"].sum(2))  # near + far per (plane, action, vm, va)


@pytest.mark.parametrize("case", sorted(CASES))
def test_crash_plane(case):
    d = _run(case)
    want_c, _ = _host_fold(case)
    np.testing.assert_array_equal(d["counts"][1], want_c[1])
    assert (d["counts"][1] <= d["counts"][0]).all() and (d["d_counts"][1] <= d["d_counts"][0]).all()
    # crash_bits NULL: plane 0 as before, plane 1 untouched
    np.testing.assert_array_equal(d["n_counts"][0], want_c[0])
    assert (d["n_counts"][1] == 7).all()
    np.testing.assert_array_equal(d["n_visits"], d["visits"])
    recorded = any(c.any() for *_, c in d["steps"])
    hand_c, _ = _host_fold(case, hand=True)  # (compared in test_counts_and_visits)
    assert all(h.any() for h in d["hand"]) and 0 < hand_c[1].sum() < hand_c[0].sum()
    print(f"{case}: recorded crashes {'yes' if recorded else 'none'}, crash-plane pairs {want_c[1].sum()}, "
          f"with the hand-set bits {hand_c[1].sum()}")
    if case == "open2x2_n2":  # (two agents on four cells: tests/_shapes.py counts 384 crashes in 660 env-steps)
        assert recorded and want_c[1].sum() > 0, "six steps of the 2 x 2 map held no crash"


@pytest.mark.parametrize("case", sorted(CASES))
def test_active_mask(case):
    d = _run(case)
    want_c, want_v = _host_fold(case, masked=True)
    assert 0 < want_v.sum() < d["visits"].sum()
    np.testing.assert_array_equal(d["m_counts"], want_c)
    np.testing.assert_array_equal(d["m_visits"], want_v)
    assert (d["z_counts"] == 7).all() and (d["z_visits"] == 7).all()  # all-zero mask: untouched


@pytest.mark.parametrize("case", sorted(CASES))
def test_cells_and_actions_are_clamped(case):
    d = _run(case)
    E, N, HW = d["E"], d["N"], d["HW"]
    assert (d["bad_cells"] == -1).any() and (d["bad_cells"] == HW).any()
    assert all((d["bad_acts"] == v).any() for v in (-1, 9, 2 ** 31 - 1))
    _, sets, _, _, crash = d["steps"][-1]
    want_c, want_v = F.fold(sets, d["bad_cells"], d["bad_acts"], d["W"], HW, d["R"], crash_bits=crash)
    np.testing.assert_array_equal(d["c_counts"], want_c)
    np.testing.assert_array_equal(d["c_visits"], want_v)
    assert d["c_counts"][0].sum() == E * N * (N - 1) and d["c_visits"].sum() == E * N  # every increment lands


@pytest.mark.parametrize("case", sorted(CASES))
def test_derived_footprint_against_resp_full(case):
    d = _run(case)
    T, N = marlnav.resp_table(), d["N"]
    off = ~np.eye(N, dtype=bool)
    for _, sets, resp, _, _ in d["steps"]:  # the order of the two sets: [0] the actor on its MdR (vm), [1] actual (va)
        np.testing.assert_array_equal(resp[:, off], T[F.popcount9(sets[..., 0]), F.popcount9(sets[..., 1])][:, off])
    fp, pairs, (near, far) = marlnav.resp_footprint_from_counts(torch.from_numpy(d["counts"]), T)
    got = fp[0].numpy()
    exact, mag, n = F.bin_resp([(resp, cells, acts) for cells, _, resp, acts, _ in d["steps"]], d["W"], d["HW"], d["R"])
    np.testing.assert_array_equal(pairs[0].numpy(), n)
    err, bound = np.abs(got - exact), n * F.U * mag
    print(f"{case}: terms per bin up to {n.max()}, non-empty bins {(n > 0).sum()}, max |err| {err.max():.3e}, "
          f"bound max {bound.max():.3e}")
    assert (err <= bound).all()
    assert (got[n == 0] == 0.0).all()
    S = 2 * d["R"] + 1
    assert tuple(near.shape) == (2, 9, S, S) and torch.equal(far, fp[:, :, -1])


def test_argument_errors():
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    E, N, H, W, R = 8, 4, 4, 4, 2
    rv = torch.zeros((E, N, N, 2), dtype=torch.int16, device=dev)
    cells = torch.zeros((N, E), dtype=torch.int32, device=dev)
    acts = torch.zeros((E, N), dtype=torch.int32, device=dev)
    counts, visits = _buffers(dev, R)
    s = torch.cuda.current_stream(dev).cuda_stream

    def call(rv_p, cells_p, acts_p, counts_p, e, n, h, w, r, visits_p=None):
        return lib.gw_resp_footprint_accum(rv_p, cells_p, acts_p, None, None, counts_p, visits_p, e, n, h, w, r, s)

    p = (rv.data_ptr(), cells.data_ptr(), acts.data_ptr(), counts.data_ptr())
    good = (E, N, H, W, R)
    bad = [(None, p[1], p[2], p[3], *good), (p[0], None, p[2], p[3], *good), (p[0], p[1], None, p[3], *good),
           (p[0], p[1], p[2], None, *good), (*p, E, 1, H, W, R), (*p, E, 9, H, W, R), (*p, 0, N, H, W, R),
           (*p, E, N, 0, W, R), (*p, E, N, H, 0, R), (*p, E, N, H, W, 0), (*p, E, N, H, W, 16),
           (p[0] + 2, p[1], p[2], p[3], *good), (p[0], p[1] + 2, p[2], p[3], *good), (p[0], p[1], p[2] + 1, p[3], *good),
           (p[0], p[1], p[2], p[3] + 4, *good), (*p, *good, visits.data_ptr() + 4)]
    for args in bad:
        assert call(*args) == GW_ERR_ARG, args
        assert b"gw_resp_footprint_accum" in lib.gw_last_error()
    assert call(*p, *good, visits.data_ptr()) == 0
    torch.cuda.synchronize()
    # all cells 0, all words 0, all actions 0: one bin, the centre offset
    centre = R * (2 * R + 1) + R
    assert int(counts.sum()) == E * N * (N - 1) == int(counts[0, 0, centre, 0, 0]) and int(visits[0]) == E * N

    from marlnav.rollout import Rollout
    plain = VecGridEnv("grid32", num_envs=E, fear=True, seed=1, debug=True)
    try:
        with pytest.raises(ValueError):  # no fear_full
            plain.resp_footprint_accum(rv, cells, acts, *_buffers(dev, 5))
        with pytest.raises(ValueError):
            Rollout(plain, None, resp_footprint=5)
    finally:
        plain.close()
    armed = VecGridEnv("grid32", num_envs=E, fear=True, seed=1, fear_full=True)
    try:
        a = (armed.out["resp_valid"], armed.copy_pos(), acts)
        with pytest.raises(ValueError):  # counts of the wrong dtype
            armed.resp_footprint_accum(*a, torch.zeros((2, 9, 122, 10, 10), dtype=torch.int32, device=dev))
        with pytest.raises(ValueError):  # counts sized for another radius
            armed.resp_footprint_accum(*a, _buffers(dev, 5)[0], radius=4)
        with pytest.raises(ValueError):
            armed.resp_footprint_accum(*a, _buffers(dev, 5)[0], radius=16)
        with pytest.raises(ValueError):  # actions of the wrong size
            armed.resp_footprint_accum(a[0], a[1], acts[:, :2].contiguous(), _buffers(dev, 5)[0])
        with pytest.raises(ValueError):  # the step's actions and crash_bits need debug=True
            Rollout(armed, None, resp_footprint=5)
    finally:
        armed.close()


def _random_rollout(fear_async):
    """Random RL policy, no ring: 7 steps; -> (totals, the host fold of the same steps or None)."""
    from marlnav.rollout import Rollout
    E, R = 96, 5
    env = VecGridEnv("grid32", num_envs=E, fear=True, fear_weight=-5.0, max_steps=5, seed=9, stats=True,
                     fear_full=True, debug=True)
    try:
        ro = Rollout(env, None, resp_footprint=R, obs_async=fear_async, fear_async=fear_async)
        ro.reset()
        counts, visits = np.zeros((2, 9, F.n_offsets(R), 10, 10), np.int64), np.zeros(9, np.int64)
        for _ in range(7):
            cells = None if fear_async else env.copy_pos().cpu().numpy()
            r = ro.step()
            if not fear_async:
                torch.cuda.synchronize()
                c, v = F.fold(_sets(r.resp_valid), cells, r.actions.cpu().numpy(), env.W, env.H * env.W, R,
                              crash_bits=r.crash_bits.cpu().numpy())
                counts += c
                visits += v
        ro.fence()
        tot = ro.totals()
        torch.cuda.synchronize()
        return tot, (None if fear_async else (counts, visits))
    finally:
        env.close()


def test_rollout_totals(monkeypatch):
    monkeypatch.setenv("GW_KERNEL", "defer")  # (the path whose FeAR can stay unjoined)
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    tot, (counts, visits) = _random_rollout(False)
    assert tot["resp_footprint_counts"].dtype == torch.int64
    assert tuple(tot["resp_footprint_counts"].shape) == (2, 9, 122, 10, 10)
    np.testing.assert_array_equal(tot["resp_footprint_counts"].numpy(), counts)
    np.testing.assert_array_equal(tot["resp_footprint_visits"].numpy(), visits)
    assert visits.sum() == 7 * 96 * 4 and counts[0].sum() == 7 * 96 * 12
    assert tuple(tot["resp_footprint"].shape) == (2, 9, 122) and tot["resp_footprint"].dtype == torch.float64
    assert torch.equal(tot["resp_footprint"], marlnav.resp_footprint_from_counts(counts)[0])
    assert "resp_map" not in tot and "resp_full" not in tot  # the footprint turns neither on
    # the unjoined FeAR folds each step one step late, on the cells copied before it: the same integers
    tot_a, _ = _random_rollout(True)
    for k in ("resp_footprint_counts", "resp_footprint_visits", "resp_footprint"):
        assert torch.equal(tot_a[k], tot[k]), k


def _window_rollout(graph):
    """test_gpu_resp_map._window_rollout with the footprint on: 10 eager steps, or 2 eager + one 8-step graph."""
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    E, P, slots, G = 256, 11, 16, 8
    env = VecGridEnv("grid32", num_envs=E, fear=True, fear_weight=-5.0, max_steps=40, seed=42, stats=True,
                     obs=False, fear_full=True, debug=True)
    try:
        actors = MultiAgentActors(env.K, P, P, arch="mlp", device=env.device, seed=0)
        ro = Rollout(env, actors, replay_slots=slots, training=True, seed=42, patch=P, resp_footprint=5)
        ro.reset()
        if graph:
            for _ in range(2):
                ro.step()
            ro.capture(G).replay()
        else:
            for _ in range(10):
                ro.step()
        ro.fence()
        tot = ro.totals()
        torch.cuda.synchronize()
        return tot
    finally:
        env.close()


def test_graph_replay_equals_eager(monkeypatch):
    monkeypatch.setenv("GW_KERNEL", "merged")
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    eager, replayed = _window_rollout(False), _window_rollout(True)
    assert int(eager["resp_footprint_visits"].sum()) == 10 * 256 * 4
    assert int(eager["resp_footprint_counts"][0].sum()) == 10 * 256 * 12
    for k in ("resp_footprint_counts", "resp_footprint_visits", "resp_footprint"):
        assert torch.equal(eager[k], replayed[k]), k


def test_evaluate_and_customeval(tmp_path, capsys):
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("grid32")
    E, T = 32, 16
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    r = evaluate(actors, sc, episodes=E, max_steps=T, fear=True, seed=11, resp_footprint=5)
    assert tuple(r["resp_footprint"].shape) == (2, 9, 122) and r["resp_footprint"].dtype == torch.float64
    cnt, vis = r["resp_footprint_counts"].numpy(), r["resp_footprint_visits"].numpy()
    # the episodes still running: "steps" active env-steps, N actor-steps and N (N - 1) pairs each
    assert vis.sum() == r["steps"] * sc.N and cnt[0].sum() == r["steps"] * sc.N * (sc.N - 1)
    assert (cnt[1] <= cnt[0]).all()
    assert "resp_footprint" not in evaluate(actors, sc, episodes=E, max_steps=8, fear=True, seed=11)
    with pytest.raises(ValueError):
        evaluate(actors, sc, episodes=E, max_steps=8, fear=False, resp_footprint=5)

    import customeval
    from marlnav.maddpg import MADDPG
    ck, out_file = str(tmp_path / "m.safetensors"), str(tmp_path / "fp.npz")
    MADDPG(sc.K, sc.H, sc.W, device=torch.device("cuda"), seed=3).save(ck)
    args = ["--checkpoint", ck, "--scenario", "grid32", "--episodes", "16", "--train-steps", "12"]
    customeval.main(args)
    base = capsys.readouterr().out.strip().splitlines()
    customeval.main(args + ["--resp-footprint", "--resp-footprint-file", out_file])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(base) == 3 and out[:3] == base
    assert len(out) == 3 + 9 * (1 + 11) + 2
    for a in range(9):
        head = out[3 + 12 * a]
        assert head.startswith(f"Action {a}: ") and all(len(ln.split()) == 11 for ln in out[4 + 12 * a:15 + 12 * a])
    assert out[-2].startswith("Far share of the absolute Resp (beyond radius 5): ")
    share = float(out[-2].split(": ")[1].split()[0])
    assert 0.0 <= share <= 1.0
    z = np.load(out_file)
    assert z["counts"].shape == (2, 9, 122, 10, 10) and z["visits"].shape == (9,) and z["footprint"].shape == (2, 9, 122)
    assert z["counts"][0].sum() > 0 and z["visits"].sum() * (sc.N - 1) == z["counts"][0].sum()
    customeval.main(args + ["--resp-footprint", "2"])  # another radius, no file
    assert len(capsys.readouterr().out.strip().splitlines()) == 3 + 9 * (1 + 5) + 1
