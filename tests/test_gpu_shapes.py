"""The shape sweep: every agent count and map shape of tests/_shapes.SHAPES through the step, FeAR and obs
kernels, on every kernel path, bit for bit against the C oracle.

The rows are open maps (two-dimensional moves, two-step MdRs under live scripted policies) at the N, K and
H x W where the kernels take another template instantiation or another branch; each row names its branch in
the table.  The oracle is pinned to the reference on the same rows by tests/test_shapes_cpu.py.

a. FeAR-on native rollouts: test_gpu_chain_shapes._rollout (every output, the state, the integer statistics,
   per step the Resp rows of every env from FeAR_4_one_actor on the pre-step snapshot).
b. FeAR-off native rollouts: test_gpu_parity._compare_native (the FeAR-off step kernels are instantiations
   of their own).
c. The reference's recorded trajectories (tests/golden/shapes_traj.npz) through GpuStepper.
d. fear_alt, feal, fear_full armed together, and fear_preview on FeAR-on and FeAR-off twins.
e. The obs writers: the delta writer, bf16 where H*W % 8 == 0 (the predicate is computed), the windows.

Sizes: E = 33 is one full 32-env block plus a ragged one, two 16-env blocks plus one and nine 4-env blocks;
E = 36 where the window writer of the FeAR launch needs E % 4 == 0.  max_steps = 12 ends episodes at the cap
inside every run.  On rows with H*W % 4 != 0 gw_create keeps the defer path whatever GW_KERNEL says (the
merged launch needs float4 rows), so "merged" runs the defer kernels there; the cases run all the same."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from marlnav import _lib
from marlnav.vec_env import VecGridEnv

from _replay import replay
from _shapes import SHAPE_IDS, SWEEP, load_traj, oracle_counts, scenario, traj_cases
from test_gpu_chain_shapes import _rollout
from test_gpu_fear_full import _popcount, _sets
from test_gpu_fear_preview import _oracle_rows as _alt_rows
from test_gpu_obs_patch import crop
from test_gpu_parity import KERNEL_PATHS, GpuStepper, _compare_native

pytestmark = pytest.mark.gpu
E = SWEEP["E"]


def _set_path(monkeypatch, path):
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    monkeypatch.delenv("GW_OBS_DELTA", raising=False)
    for k, v in KERNEL_PATHS[path].items():
        monkeypatch.setenv(k, v)


# ---- a. FeAR on ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", sorted(KERNEL_PATHS))
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_fear_on_rollout_matches_oracle(sid, path, monkeypatch):
    _set_path(monkeypatch, path)
    done, crashes, nonzero, restricted = oracle_counts(sid)  # over the oracle's own outputs
    assert done > 0 and crashes > 0 and nonzero > 0 and restricted > 0, (sid, done, crashes, nonzero, restricted)
    trace = _rollout(scenario(sid), E, steps=SWEEP["steps"], seed=SWEEP["seed"])
    assert len(trace) == SWEEP["steps"]
    assert sum(int((fear != 0).sum()) for fear, _ in trace) == nonzero  # the GPU's FeAR is the counted one


# ---- b. FeAR off -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", sorted(KERNEL_PATHS))
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_fear_off_rollout_matches_oracle(sid, path, monkeypatch):
    _set_path(monkeypatch, path)
    done = _compare_native(scenario(sid), E, False, 30, max_steps=12, offset=12345)
    assert done > 0


# ---- c. reference trajectories ---------------------------------------------------------------------------

@pytest.mark.parametrize("path", sorted(KERNEL_PATHS))
@pytest.mark.parametrize("sid,seed", traj_cases())
def test_gpu_replays_reference_trajectory(sid, seed, path, monkeypatch):
    _set_path(monkeypatch, path)
    d, fear, weight = load_traj(sid, seed)
    sc = scenario(sid)
    st = GpuStepper(sc, fear, weight)
    try:
        T, err = replay(st, d, sc.K, sc.N)
    finally:
        st.env.close()
    assert T == len(d["rl"]) > 0 and err == 0.0


# ---- d. the optional outputs -----------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["defer", "merged"])
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_optional_outputs_match_oracle(sid, path, monkeypatch):
    """fear_alt, feal and fear_full armed together, 12 steps with auto-resets; fear_preview of a FeAR-on and a
    FeAR-off twin (same seed: the world does not depend on FeAR) before every step."""
    _set_path(monkeypatch, path)
    sc = scenario(sid)
    N, K, H, W = sc.N, sc.K, sc.H, sc.W
    region = np.asarray(sc.region).reshape(H, W)
    kw = dict(num_envs=E, fear_weight=-5.0, seed=SWEEP["seed"], max_steps=SWEEP["max_steps"], auto_reset=True, debug=True)
    env = VecGridEnv(sc, fear=True, fear_alt=True, feal=True, fear_full=True, **kw)
    twins = [VecGridEnv(sc, fear=True, **kw), VecGridEnv(sc, fear=False, **kw)]
    ar, dg = np.arange(E), np.arange(N)
    resets = nz_alt = nz_full = below_one = 0
    try:
        for e in [env] + twins:
            e.reset()
        for t in range(12):
            cells = env.positions().cpu().numpy().astype(np.int32)  # the pre-step (pre-reset) world
            tabs = [tw.fear_preview() for tw in twins]
            for name, v in (("fear_alt", float("nan")), ("feal", float("nan")), ("resp_full", float("nan")),
                            ("feal_valid", -1), ("resp_valid", -1)):
                env.out[name].fill_(v)
            r = env.step()
            for tw in twins:
                tw.step()
            torch.cuda.synchronize()
            acts, mdr, fear = r.actions.cpu().numpy(), r.mdr.cpu().numpy(), r.fear.cpu().numpy()
            fa = r.fear_alt.cpu().numpy()
            rf, rv = r.resp_full.cpu().numpy(), _sets(r.resp_valid)
            fe, fv = r.feal.cpu().numpy(), _sets(r.feal_valid)
            assert fa.shape == (E, K, 9) and rf.shape == (E, N, N) and rv.shape == (E, N, N, 2)
            assert fe.shape == (E, N) and fv.shape == (E, N, 2)
            assert not np.isnan(fa).any() and not np.isnan(rf).any() and not np.isnan(fe).any()
            assert (rv < 512).all() and (fv < 512).all()
            assert (rf[:, dg, dg] == 0.0).all() and (rv[:, dg, dg] == 0).all()
            # gw_fear_matrix on the same snapshot
            fm = {k: v.cpu().numpy() for k, v in env.fear_matrix(cells, acts, mdr, None).items()}
            np.testing.assert_array_equal(rf, fm["resp"], err_msg=f"t={t} resp_full vs gw_fear_matrix")
            np.testing.assert_array_equal(_popcount(rv[..., 0]), fm["vm"], err_msg=f"t={t} vm vs gw_fear_matrix")
            np.testing.assert_array_equal(_popcount(rv[..., 1]), fm["va"], err_msg=f"t={t} va vs gw_fear_matrix")
            for e in range(E):
                o = O.fear_matrix(H, W, region, cells[e], acts[e], mdr[e], None)
                np.testing.assert_array_equal(rf[e], o["resp"], err_msg=f"t={t} e={e} resp_full")
                np.testing.assert_array_equal(_popcount(rv[e, ..., 0]), o["vm"], err_msg=f"t={t} e={e} vm")
                np.testing.assert_array_equal(_popcount(rv[e, ..., 1]), o["va"], err_msg=f"t={t} e={e} va")
                np.testing.assert_array_equal(fe[e], o["feal"], err_msg=f"t={t} e={e} feal")
                np.testing.assert_array_equal(_popcount(fv[e, :, 0]), o["feal_vm"], err_msg=f"t={t} e={e} feal_vm")
                np.testing.assert_array_equal(_popcount(fv[e, :, 1]), o["feal_va"], err_msg=f"t={t} e={e} feal_va")
                # FeAR_4_one_actor over k's close set with k's action replaced by a, all nine a
                want = _alt_rows(H, W, region, cells[e], acts[e], mdr[e], range(K))
                np.testing.assert_array_equal(fa[e], want, err_msg=f"t={t} e={e} fear_alt")
            for k in range(K):
                np.testing.assert_array_equal(fa[ar, k, acts[:, k]], fear[:, k], err_msg=f"t={t} k={k} own action")
                assert (fa[ar, k, mdr[:, k]] == 0).all(), (t, k)
            for tab, tw in zip(tabs, twins):
                assert torch.equal(tab, r.fear_alt), (t, "preview", tw.fear_enabled)  # bit for bit, no NaN
            resets += int(r.done.sum())
            nz_alt += int((fa != 0).sum())
            nz_full += int((rf != 0).sum())
            below_one += int((fe < 1).sum())
    finally:
        for e in [env] + twins:
            e.close()
    assert resets > 0 and nz_alt > 0 and nz_full > 0 and below_one > 0, (resets, nz_alt, nz_full, below_one)


# ---- e. the obs writers ----------------------------------------------------------------------------------

E4 = 36


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_delta_writer_equals_full_writer(sid, monkeypatch):
    """A ring of two destinations: the first step into each is a full write, every later one the delta
    writer's (gw_obs_delta_counts); obs and final_obs bit for bit those of a twin with the table off.  On the
    defer path, the one the delta writer covers."""
    _set_path(monkeypatch, "defer")
    sc = scenario(sid)
    kw = dict(num_envs=E4, fear=True, fear_weight=-5.0, seed=SWEEP["seed"], max_steps=SWEEP["max_steps"],
              auto_reset=True, final_obs=True)
    env, ref = VecGridEnv(sc, **kw), VecGridEnv(sc, **kw)
    try:
        assert env.kernel_path == "defer" and env.obs_delta
        ref.set_obs_delta(False)
        ring = [torch.full_like(env.out["obs"], float("nan")) for _ in range(2)]
        a, b = env.reset()[0], ref.reset()[0]
        assert torch.equal(_bits(a), _bits(b))
        base, base_ref = env.obs_delta_counts(), ref.obs_delta_counts()
        ended = 0
        for t in range(12):
            c0 = env.obs_delta_counts()
            r, q = env.step(obs_out=ring[t % 2]), ref.step()
            torch.cuda.synchronize()
            c1 = env.obs_delta_counts()
            assert (c1[0] - c0[0], c1[1] - c0[1]) == ((1, 0) if t < 2 else (0, 1)), (t, c0, c1)
            assert r.obs is ring[t % 2]
            assert torch.equal(_bits(r.obs), _bits(q.obs)), t
            assert torch.equal(_bits(r.final_obs), _bits(q.final_obs)), t  # NaN rows (never ended) compare as bits
            assert torch.equal(r.done, q.done) and torch.equal(r.reward, q.reward), t
            ended += int(r.done.sum())
        assert ref.obs_delta_counts() == (base_ref[0] + 12, 0)  # the twin never took the delta writer
        assert env.obs_delta_counts() == (base[0] + 2, base[1] + 10)
        assert ended > 0
    finally:
        env.close()
        ref.close()


@pytest.mark.parametrize("path", ["defer", "merged"])
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_bf16_obs_equal_f32_or_are_rejected(sid, path, monkeypatch):
    _set_path(monkeypatch, path)
    sc = scenario(sid)
    kw = dict(num_envs=E4, fear=True, fear_weight=-5.0, seed=SWEEP["seed"], max_steps=SWEEP["max_steps"],
              auto_reset=True, final_obs=True)
    if sc.HW % 8 != 0:
        with pytest.raises(_lib.GwError, match=r"bf16 obs needs H\*W % 8 == 0"):
            VecGridEnv(sc, obs_dtype=torch.bfloat16, **kw)
        return
    a, b = VecGridEnv(sc, **kw), VecGridEnv(sc, obs_dtype=torch.bfloat16, **kw)
    try:
        assert b.out["obs"].dtype == torch.bfloat16
        oa, ob = a.reset()[0], b.reset()[0]
        assert torch.equal(oa, ob.float())
        ended = 0
        for t in range(12):
            r, q = a.step(), b.step()
            torch.cuda.synchronize()
            assert torch.equal(r.obs, q.obs.float()), t
            d = r.done != 0
            assert torch.equal(r.final_obs[:, d], q.final_obs[:, d].float()), t
            assert torch.equal(r.done, q.done) and torch.equal(r.reward, q.reward) and torch.equal(r.fear, q.fear), t
            ended += int(d.sum())
        assert ended > 0
    finally:
        a.close()
        b.close()


def test_bf16_predicate_splits_the_table():
    legal = sorted(sid for sid in SHAPE_IDS if scenario(sid).HW % 8 == 0)
    assert legal == sorted(["1x8_n2_k1", "4x6_n6_k6", "5x8_n5_k5", "64x64_n8_k8"])


@pytest.mark.parametrize("path", ["defer", "merged"])
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_windows_equal_cropped_obs(sid, path, monkeypatch):
    """obs_patch(P, final=True) after every step, and patch_next(11) before every step of a twin without dense
    obs (FeAR on and E % 4 == 0: the windows come from the FeAR launch), against the -1-padded crop of the
    dense obs.  P = 1, odd, even, and wider than the map on both sides."""
    _set_path(monkeypatch, path)
    sc = scenario(sid)
    K, W = sc.K, sc.W
    sizes = sorted({1, 3, 8, min(129, 2 * max(sc.H, sc.W) + 1)})
    kw = dict(num_envs=E4, fear=True, fear_weight=-5.0, seed=SWEEP["seed"], max_steps=SWEEP["max_steps"], auto_reset=True)
    env = VecGridEnv(sc, final_obs=True, debug=True, **kw)
    twin = VecGridEnv(sc, obs=False, **kw)
    PN = 11
    nxt = [torch.full((K, E4, PN, PN), float("nan"), device=env.device) for _ in range(2)]
    try:
        env.reset()
        twin.reset()
        pos = env.state()["pos"]  # [N, E]
        def nan(P):  # a cell the writer skips must not pass on what the allocator left there
            return torch.full((K, E4, P, P), float("nan"), device=env.device)

        for P in sizes:
            p = env.obs_patch(P, out=nan(P))
            for k in range(K):
                assert torch.equal(p[k], crop(env.out["obs"][k], pos[k], P, W)), ("reset", P, k)
        ended = 0
        for t in range(12):
            twin.patch_next(PN, nxt[0], nxt[1])
            r, q = env.step(), twin.step()
            pos = env.state()["pos"]
            d = r.done != 0
            ended += int(d.sum())
            assert torch.equal(r.fear, q.fear) and torch.equal(r.done, q.done), t
            for P in sizes + [PN]:
                if P == PN:
                    patch, fin = nxt
                else:
                    patch, fin = env.obs_patch(P, final=True, out=nan(P))
                for k in range(K):
                    assert torch.equal(patch[k], crop(r.obs[k], pos[k], P, W)), (t, P, k)
                    want = crop(r.final_obs[k], r.final_pos[:, k].contiguous(), P, W)
                    assert torch.equal(fin[k][d], want[d]), (t, P, k, "final")
                    if P != PN:
                        assert bool(torch.isnan(fin[k][~d]).all()), (t, P, k)  # terminal windows of done envs only
        assert ended > 0
    finally:
        env.close()
        twin.close()
