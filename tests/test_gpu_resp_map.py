"""Responsibility maps on the GPU (gw_resp_map_accum, csrc/resp_map.hip; include/rollout_ops.h).

Shapes, the smallest at which the kernel can go wrong: grid32 with E = 37 (N = 4; 592 threads: no multiple of
4, 64 or 256, a tail block, waves that straddle a pair boundary), grid64_n8 with E = 5 (N = 8: 64 pairs per env,
HW = 4096, the 6.5 MB count array), and the smallest N = 2 open map of tests/_shapes.py (2 x 2, HW = 4).  Six
native steps each with fear_full=True and a step cap of 4, so that auto-resets fall inside the run; one run per
case, shared by the tests and never modified.

1. counts / visits equal np.add.at of the popcounts (tests/_resp_map_ref.py) exactly; folding the kept steps
   twice into a zeroed buffer gives exactly twice that (the op adds).
2. The active mask: every other env masked = the numpy fold of the unmasked envs; an all-zero mask leaves the
   buffers as they were.
3. resp_map_from_counts of the counts against the steps' resp_full, in total and per cell, within the derived
   bound n * 2^-53 * sum|x| (derivation in tests/_resp_map_ref.py; the reference sum is math.fsum, numpy's own
   sequential binning is held to the same bound).  resp_full == T[vm][va] entry by entry pins the order of the sets.
4. Cells of -1 and HW are clamped: every increment lands in a valid cell, E N (N - 1) per plane.  The kernel
   forms no address from an unclamped value (csrc/resp_map.h), so this run is a check of the clamp's result.
5. Argument errors; the Python surface: Rollout(resp_map=True) eager (FeAR joined and unjoined) and as a
   graph replay, evaluate(resp_map=True), customeval.py --resp-map, VecGridEnv without fear_full."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import marlnav
from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv

import _resp_map_ref as R
import _shapes

pytestmark = pytest.mark.gpu
CASES = {"grid32": ("grid32", 37), "grid64_n8": ("grid64_n8", 5), "open2x2_n2": ("2x2_n2_k2", 33)}
STEPS = 6
GW_ERR_ARG = -1


def _scenario(name):
    return _shapes.scenario(name) if name in _shapes.BY_ID else S.builtin(name)


def _sets(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint16).astype(np.int64)


def _buffers(env, fill=0):
    hw = env.H * env.W
    return (torch.full((2, hw, 10, 10), fill, dtype=torch.int64, device=env.device),
            torch.full((hw,), fill, dtype=torch.int64, device=env.device))


@functools.lru_cache(maxsize=None)
def _run(case):
    """-> dict: per-step host copies (cells, resp_valid, resp_full), the device folds' results."""
    name, E = CASES[case]
    sc = _scenario(name)
    env = VecGridEnv(sc, num_envs=E, fear=True, fear_weight=-5.0, seed=5, max_steps=4, auto_reset=True,
                     fear_full=True)
    try:
        HW, N = sc.H * sc.W, sc.N
        env.reset()
        counts, visits = _buffers(env)
        m_counts, m_visits = _buffers(env)
        z_counts, z_visits = _buffers(env, fill=7)
        mask = (torch.arange(E, device=env.device) % 2 == 0).to(torch.uint8)
        none = torch.zeros(E, dtype=torch.uint8, device=env.device)
        cells_dev = torch.empty((N, E), dtype=torch.int32, device=env.device)
        steps, resets = [], 0
        for _ in range(STEPS):
            env.copy_pos(cells_dev)
            r = env.step()
            env.resp_map_accum(r.resp_valid, cells_dev, counts, visits)
            env.resp_map_accum(r.resp_valid, cells_dev, m_counts, m_visits, active=mask)
            env.resp_map_accum(r.resp_valid, cells_dev, z_counts, z_visits, active=none)
            torch.cuda.synchronize()
            steps.append((cells_dev.cpu().numpy().copy(), _sets(r.resp_valid), r.resp_full.cpu().numpy().copy()))
            resets += int(r.done.sum())
        # the kept steps uploaded again, each folded twice into zeroed buffers; then the clamp call
        d_counts, d_visits = _buffers(env)
        for cells, sets, _ in steps:
            rv = torch.from_numpy(sets.astype(np.uint16).view(np.int16)).to(env.device)
            cd = torch.from_numpy(cells).to(env.device)
            for _ in range(2):
                env.resp_map_accum(rv, cd, d_counts, d_visits)
        bad_cells = steps[-1][0].copy()
        bad_cells.reshape(-1)[::3] = -1
        bad_cells.reshape(-1)[1::3] = HW
        c_counts, c_visits = _buffers(env)
        env.resp_map_accum(torch.from_numpy(steps[-1][1].astype(np.uint16).view(np.int16)).to(env.device),
                           torch.from_numpy(bad_cells).to(env.device), c_counts, c_visits)
        torch.cuda.synchronize()
        return dict(sc=sc, E=E, N=N, HW=HW, steps=steps, resets=resets, mask=mask.cpu().numpy().astype(bool),
                    counts=counts.cpu().numpy(), visits=visits.cpu().numpy(),
                    m_counts=m_counts.cpu().numpy(), m_visits=m_visits.cpu().numpy(),
                    z_counts=z_counts.cpu().numpy(), z_visits=z_visits.cpu().numpy(),
                    d_counts=d_counts.cpu().numpy(), d_visits=d_visits.cpu().numpy(),
                    bad_cells=bad_cells, c_counts=c_counts.cpu().numpy(), c_visits=c_visits.cpu().numpy())
    finally:
        env.close()


@functools.lru_cache(maxsize=None)
def _host_fold(case, masked=False):
    d = _run(case)
    counts, visits = np.zeros((2, d["HW"], 10, 10), np.int64), np.zeros(d["HW"], np.int64)
    for cells, sets, _ in d["steps"]:
        c, v = R.fold(sets, cells, d["HW"], d["mask"] if masked else None)
        counts += c
        visits += v
    return counts, visits


@pytest.mark.parametrize("case", sorted(CASES))
def test_counts_and_visits(case):
    d = _run(case)
    E, N = d["E"], d["N"]
    assert d["resets"] >= E, "no env auto-reset within the run"  # the step cap is 4
    assert all((c >= 0).all() and (c < d["HW"]).all() for c, _, _ in d["steps"])
    want_c, want_v = _host_fold(case)
    np.testing.assert_array_equal(d["counts"], want_c)
    np.testing.assert_array_equal(d["visits"], want_v)
    assert d["counts"][0].sum() == d["counts"][1].sum() == STEPS * E * N * (N - 1)
    assert d["visits"].sum() == STEPS * E * N
    assert (d["counts"].sum((0, 1)) > 0).sum() >= 2, "the run reached a single (vm, va) bin"
    np.testing.assert_array_equal(d["d_counts"], 2 * want_c, err_msg="folding twice is not twice the fold")
    np.testing.assert_array_equal(d["d_visits"], 2 * want_v)


@pytest.mark.parametrize("case", sorted(CASES))
def test_active_mask(case):
    d = _run(case)
    want_c, want_v = _host_fold(case, masked=True)
    assert 0 < want_v.sum() < d["visits"].sum()
    np.testing.assert_array_equal(d["m_counts"], want_c)
    np.testing.assert_array_equal(d["m_visits"], want_v)
    assert (d["z_counts"] == 7).all() and (d["z_visits"] == 7).all()  # all-zero mask: untouched


@pytest.mark.parametrize("case", sorted(CASES))
def test_derived_map_against_resp_full(case):
    d = _run(case)
    T, N = marlnav.resp_table(), d["N"]
    off = ~np.eye(N, dtype=bool)
    for _, sets, resp in d["steps"]:  # the order of the two sets: [0] the actor on its MdR (vm), [1] actual (va)
        vm, va = R.popcount9(sets[..., 0]), R.popcount9(sets[..., 1])
        np.testing.assert_array_equal(resp[:, off], T[vm, va][:, off])
    allx = np.concatenate([resp[:, off].reshape(-1) for _, _, resp in d["steps"]])
    print(f"{case}: {allx.size} entries, {(allx < 0).sum()} negative, {(allx > 0).sum()} positive")
    if case == "grid32":  # T[va][vm] != T[vm][va] wherever vm != va: a swapped read cannot pass the line above
        assert (allx != 0).any()
    got, pairs = marlnav.resp_map_from_counts(torch.from_numpy(d["counts"]), T)
    got = got.numpy()
    exact, mag, n, seq = R.bin_resp([(resp, cells, None) for cells, _, resp in d["steps"]], d["HW"])
    np.testing.assert_array_equal(pairs.numpy(), n)
    # in total (plane 0; plane 1 holds the same terms in other cells)
    total_ref, total_mag = math.fsum(allx.tolist()), math.fsum(np.abs(allx).tolist())
    for p in range(2):
        err = abs(math.fsum(got[p].tolist()) - total_ref)
        print(f"{case} plane {p}: total {total_ref:.6f}, |err| {err:.3e}, bound {allx.size * R.U * total_mag:.3e}")
        assert err <= allx.size * R.U * total_mag
    # per cell
    bound = n * R.U * mag
    err, err_np = np.abs(got - exact), np.abs(got - seq)
    print(f"{case}: terms per cell up to {n.max()}, max |err| {err.max():.3e} (vs numpy's binning {err_np.max():.3e}), "
          f"bound max {bound.max():.3e}")
    assert (err <= bound).all() and (err_np <= bound).all()
    assert (got[n == 0] == 0.0).all()


@pytest.mark.parametrize("case", sorted(CASES))
def test_cells_are_clamped(case):
    d = _run(case)
    E, N, HW = d["E"], d["N"], d["HW"]
    assert (d["bad_cells"] == -1).any() and (d["bad_cells"] == HW).any()
    want_c, want_v = R.fold(d["steps"][-1][1], d["bad_cells"], HW)  # (the restatement clamps as the header does)
    np.testing.assert_array_equal(d["c_counts"], want_c)
    np.testing.assert_array_equal(d["c_visits"], want_v)
    assert d["c_counts"][0].sum() == d["c_counts"][1].sum() == E * N * (N - 1) and d["c_visits"].sum() == E * N


def test_argument_errors():
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    E, N, HW = 8, 4, 16
    rv = torch.zeros((E, N, N, 2), dtype=torch.int16, device=dev)
    cells = torch.zeros((N, E), dtype=torch.int32, device=dev)
    counts = torch.zeros((2, HW, 10, 10), dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def call(rv_p, cells_p, counts_p, e, n, hw):
        return lib.gw_resp_map_accum(rv_p, cells_p, None, counts_p, None, e, n, hw, s)

    good = (rv.data_ptr(), cells.data_ptr(), counts.data_ptr())
    for args in ((*good, E, 1, HW), (*good, E, 9, HW), (good[0], good[1], None, E, N, HW), (*good, 0, N, HW),
                 (*good, E, N, 0), (None, good[1], good[2], E, N, HW), (good[0], None, good[2], E, N, HW)):
        assert call(*args) == GW_ERR_ARG, args
        assert b"gw_resp_map_accum" in lib.gw_last_error()
    assert call(*good, E, N, HW) == 0
    torch.cuda.synchronize()
    assert int(counts.sum()) == 2 * E * N * (N - 1) and int(counts[0, 0, 0, 0]) == E * N * (N - 1)

    plain = VecGridEnv("grid32", num_envs=E, fear=True, seed=1)
    try:
        with pytest.raises(ValueError):
            plain.resp_map_accum(rv, cells, torch.zeros((2, 1024, 10, 10), dtype=torch.int64, device=dev))
        from marlnav.rollout import Rollout
        with pytest.raises(ValueError):
            Rollout(plain, None, resp_map=True)
    finally:
        plain.close()
    armed = VecGridEnv("grid32", num_envs=E, fear=True, seed=1, fear_full=True)
    try:
        with pytest.raises(ValueError):  # counts of the wrong dtype
            armed.resp_map_accum(armed.out["resp_valid"], armed.copy_pos(),
                                 torch.zeros((2, 1024, 10, 10), dtype=torch.int32, device=dev))
    finally:
        armed.close()


def _random_rollout(fear_async):
    """Random RL policy, no ring: 7 steps; -> (totals, the host fold of the same steps or None)."""
    from marlnav.rollout import Rollout
    E = 96
    env = VecGridEnv("grid32", num_envs=E, fear=True, fear_weight=-5.0, max_steps=5, seed=9, stats=True,
                     fear_full=True)
    try:
        ro = Rollout(env, None, resp_map=True, obs_async=fear_async, fear_async=fear_async)
        ro.reset()
        HW = env.H * env.W
        counts, visits = np.zeros((2, HW, 10, 10), np.int64), np.zeros(HW, np.int64)
        for _ in range(7):
            cells = None if fear_async else env.copy_pos().cpu().numpy()
            r = ro.step()
            if not fear_async:
                torch.cuda.synchronize()
                c, v = R.fold(_sets(r.resp_valid), cells, HW)
                counts += c
                visits += v
        ro.fence()
        tot = ro.totals()
        torch.cuda.synchronize()
        return tot, (None if fear_async else (counts, visits)), env
    finally:
        env.close()


def test_rollout_totals(monkeypatch):
    monkeypatch.setenv("GW_KERNEL", "defer")  # (the path whose FeAR can stay unjoined)
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    tot, (counts, visits), env = _random_rollout(False)
    assert tot["resp_map_counts"].dtype == torch.int64 and tuple(tot["resp_map_counts"].shape) == (2, 1024, 10, 10)
    np.testing.assert_array_equal(tot["resp_map_counts"].numpy(), counts)
    np.testing.assert_array_equal(tot["resp_map_visits"].numpy(), visits)
    assert tuple(tot["resp_map"].shape) == (2, env.H, env.W) and tot["resp_map"].dtype == torch.float64
    want, _ = marlnav.resp_map_from_counts(counts)
    assert torch.equal(tot["resp_map"].reshape(2, -1), want)
    assert tot["resp_full_steps"] == 7  # resp_map turns the matrix total on
    # the unjoined FeAR folds each step one step late, on the cells copied before it: the same integers
    tot_a, _, _ = _random_rollout(True)
    assert torch.equal(tot_a["resp_map_counts"], tot["resp_map_counts"])
    assert torch.equal(tot_a["resp_map_visits"], tot["resp_map_visits"])
    assert torch.equal(tot_a["resp_map"], tot["resp_map"])


def _window_rollout(graph):
    """test_gpu_fear_full._window_rollout with the maps on: 10 eager steps, or 2 eager + one 8-step graph."""
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    E, P, slots, G = 256, 11, 16, 8
    env = VecGridEnv("grid32", num_envs=E, fear=True, fear_weight=-5.0, max_steps=40, seed=42, stats=True,
                     obs=False, fear_full=True)
    try:
        actors = MultiAgentActors(env.K, P, P, arch="mlp", device=env.device, seed=0)
        ro = Rollout(env, actors, replay_slots=slots, training=True, seed=42, patch=P, resp_map=True)
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
    assert int(eager["resp_map_visits"].sum()) == 10 * 256 * 4
    for k in ("resp_map_counts", "resp_map_visits", "resp_map", "resp_full"):
        assert torch.equal(eager[k], replayed[k]), k


def test_evaluate_and_customeval(tmp_path, capsys):
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("grid32")
    E, T = 32, 16
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    r = evaluate(actors, sc, episodes=E, max_steps=T, fear=True, seed=11, resp_map=True)
    assert tuple(r["resp_map"].shape) == (2, sc.H, sc.W) and r["resp_map"].dtype == torch.float64
    cnt, vis = r["resp_map_counts"].numpy(), r["resp_map_visits"].numpy()
    # the episodes still running: "steps" active env-steps, N visits and N (N - 1) pairs each
    assert vis.sum() == r["steps"] * sc.N and cnt[0].sum() == cnt[1].sum() == r["steps"] * sc.N * (sc.N - 1)
    assert "resp_map" not in evaluate(actors, sc, episodes=E, max_steps=8, fear=True, seed=11)
    with pytest.raises(ValueError):
        evaluate(actors, sc, episodes=E, max_steps=8, fear=False, resp_map=True)

    import customeval
    from marlnav.maddpg import MADDPG
    ck, out_file = str(tmp_path / "m.safetensors"), str(tmp_path / "maps.npz")
    MADDPG(sc.K, sc.H, sc.W, device=torch.device("cuda"), seed=3).save(ck)
    args = ["--checkpoint", ck, "--scenario", "grid32", "--episodes", "16", "--train-steps", "12"]
    customeval.main(args)
    base = capsys.readouterr().out.strip().splitlines()
    customeval.main(args + ["--resp-map", out_file])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(base) == 3 and out[:3] == base
    assert out[3].startswith("Mean Resp caused per visit") and out[4 + sc.H].startswith("Mean Resp received per visit")
    assert len(out) == 3 + 2 * (1 + sc.H) + 1 and all(len(ln.split()) == sc.W for ln in out[4:4 + sc.H])
    z = np.load(out_file)
    assert z["counts"].shape == (2, sc.HW, 10, 10) and z["visits"].shape == (sc.H, sc.W)
    assert z["resp_map"].shape == (2, sc.H, sc.W) and z["counts"].sum() > 0
    customeval.main(args + ["--resp-map"])  # no file: the maps are printed only
    assert len(capsys.readouterr().out.strip().splitlines()) == 3 + 2 * (1 + sc.H)
