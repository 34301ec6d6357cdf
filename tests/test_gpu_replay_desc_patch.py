"""The descriptor-only replay ring of the local-window rollouts (``ReplayRing(patch=P, desc="only")``,
``Rollout(patch=P, desc_ring="only")``, ``MADDPGTrainer(patch=P)``; gw_replay_gather_desc_patch,
include/rollout_ops.h): the ring holds 48-byte obs descriptors and no windows, the step runs no window
writer, and the sampled P x P rows expanded from the descriptors are bit for bit gw_obs_patch's windows.

Every comparison is ``torch.equal``.  The reference is a dense window ring the TEST keeps: after the reset and
after every step it calls ``env.obs_patch(P, final=True)`` itself and stores the windows in mirror tensors
[S, K, E, P, P] at the slots the step filled; the rows are then sampled exhaustively (every stored transition
of every env) with gw_replay_gather on the mirror and with the new entry point on the descriptor ring."""
import ctypes as C

import numpy as np
import pytest
import torch

import _desc_patch as DP
import _shapes as SH
from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu

GW_ERR_ARG = -1
GW_SPAN_WINDOW = 7
SLOTS = 6


def _gather(rp, P, mirror=None, u=None, env=None, B=None, seed=0, ctr=None, rows_only=False):
    """One gather launch with explicit (u, env) or in-kernel draws (seed, ctr): on the descriptor ring
    (mirror None: gw_replay_gather_desc_patch) or on the test's dense mirror (obs, final): gw_replay_gather."""
    L, K, PP, dev = _lib.load(), rp.K, P * P, rp.probs.device
    B = int(u.numel()) if B is None else B
    o = dict(state=torch.full((K, B, P, P), 7.0, device=dev), next=torch.full((K, B, P, P), 7.0, device=dev),
             probs=torch.empty((K, B, 9), device=dev), reward=torch.empty((B, K), dtype=torch.float64, device=dev),
             term=torch.empty((B, K), dtype=torch.uint8, device=dev),
             tr=torch.empty((B,), dtype=torch.int64, device=dev),
             x=torch.empty((B, K * PP + 9 * K), device=dev), xn=torch.zeros((B, K * PP + 9 * K), device=dev))
    outs = (None if rows_only else o["state"].data_ptr(), None if rows_only else o["next"].data_ptr(),
            o["probs"].data_ptr(), o["reward"].data_ptr(), o["term"].data_ptr(), o["tr"].data_ptr(),
            o["x"].data_ptr(), o["xn"].data_ptr(), seed, ctr.data_ptr() if ctr is not None else None,
            torch.cuda.current_stream(dev).cuda_stream)
    up = u.data_ptr() if u is not None else None
    ep = env.data_ptr() if env is not None else None
    ring = (rp.probs.data_ptr(), rp.reward.data_ptr(), rp.term.data_ptr(), rp.done.data_ptr(), rp.t_dev.data_ptr())
    if mirror is None:
        _lib.check(L.gw_replay_gather_desc_patch(C.byref(rp._src), rp.desc.data_ptr(), *ring, up, ep, rp.S, B, P,
                                                 *outs), "gw_replay_gather_desc_patch")
    else:
        obs_m, fin_m = mirror
        _lib.check(L.gw_replay_gather(obs_m.data_ptr(), fin_m.data_ptr(), 0, *ring, up, ep, rp.S, K, rp.E, PP, B,
                                      *outs), "gw_replay_gather")
    o["xn"] = o["xn"][:, :K * PP]  # x_next's action slots are left to the caller
    return o


def _exhaustive_draws(rp, steps=None):
    """(u, env) that pick every stored transition of every env: u = (step + 0.5) / n for every step < n."""
    n = min(max(rp.t, 1), rp.S - 1)
    steps = list(range(n)) if steps is None else sorted({s for s in steps if s < n})
    dev = rp.probs.device
    u = torch.tensor([(s + 0.5) / n for s in steps], dtype=torch.float32, device=dev).repeat_interleave(rp.E)
    env = torch.arange(rp.E, dtype=torch.int64, device=dev).repeat(len(steps))
    return u, env


def _assert_equal(a, b, skip=()):
    for name in a:
        if name not in skip:
            assert torch.equal(a[name], b[name]), name


def _compare(rp, P, mirror, steps=None, other=None):
    """The exhaustive sample on the descriptor ring == on the mirror (or on another descriptor ring)."""
    u, env = _exhaustive_draws(rp, steps)
    a = _gather(rp, P, u=u, env=env)
    b = _gather(rp, P, mirror=mirror, u=u, env=env)
    torch.cuda.synchronize()
    _assert_equal(a, b)
    assert not torch.isnan(a["state"]).any() and not torch.isnan(a["next"]).any()
    rows = _gather(rp, P, u=u, env=env, rows_only=True)  # state / next_state NULL: the critic rows alone
    _assert_equal(rows, a, skip=("state", "next"))
    assert (rows["state"] == 7.0).all() and (rows["next"] == 7.0).all()
    if other is not None:
        _assert_equal(_gather(other, P, u=u, env=env), a)
    return a["tr"].cpu().numpy(), env.cpu().numpy()


class _Cover:
    """Which branches the sampled rows reached, decided from the agents' cells in the descriptors."""

    def __init__(self, H, W, N, K, P):
        self.H, self.W, self.N, self.K, self.P = H, W, N, K, P
        self.done = self.reset_state = self.reset_next = self.inside = self.outside = 0
        self.over = np.zeros(4, bool)

    def add(self, rp, tr, env):
        desc = rp.desc.cpu().numpy()
        done = rp.done.cpu().numpy()[tr, env] != 0
        nx = (tr + 1) % rp.S
        d0, d1 = desc[tr, env], desc[nx, env]
        self.done += int(done.sum())
        self.reset_state += int(DP.half_flags(d0, 0)[0].sum())
        self.reset_next += int(DP.half_flags(d1, 0)[0].sum())
        nxt = np.where(done[:, None], DP.half_cells(d1, 1, self.N), DP.half_cells(d1, 0, self.N))
        for cells in (DP.half_cells(d0, 0, self.N), nxt):
            for k in range(self.K):
                over, ins, out = DP.coverage(cells[:, k], cells, self.H, self.W, self.P)
                self.over |= np.array(over)
                self.inside += ins
                self.outside += out

    def check(self):
        assert self.done > 0, "no done row sampled"
        assert self.reset_state > 0 and self.reset_next > 0, "no reset-encoded obs sampled"
        if self.H > self.P and self.W > self.P:  # a map larger than the window
            assert self.over.all(), f"no window overhangs every edge (top, bottom, left, right): {self.over}"
            assert self.inside > 0 and self.outside > 0, (self.inside, self.outside)


COMPARE_AT = (1, 2, 4, 5, 6, 7, 13, 20)  # before / at / after the ring of 6 slots wraps

ROLLOUT_CASES = [("grid32", 11, 256, True), ("grid64_n8", 16, 64, False)]


@pytest.mark.parametrize("scen,P,E,fear", ROLLOUT_CASES, ids=[c[0] for c in ROLLOUT_CASES])
def test_rows_equal_obs_patch_windows_rollout(scen, P, E, fear):
    """Rollout(patch=P, desc_ring="only") with the fused MLP window actor: c5patch's own shape (grid32, P = 11,
    FeAR on) and P % 4 == 0 with N = 8 (grid64_n8, P = 16)."""
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    sc = S.builtin(scen)
    env = VecGridEnv(sc, num_envs=E, fear=fear, fear_weight=-5.0, seed=3, max_steps=6, auto_reset=True, obs=False)
    actors = MultiAgentActors(sc.K, P, P, "mlp", device="cuda", seed=1)
    ro = Rollout(env, actors, replay_slots=SLOTS, training=True, seed=4, patch=P, desc_ring="only")
    rp = ro.replay
    assert ro.fused and ro.desc_only and rp.desc_only and rp.obs is None and rp.final_obs is None
    assert tuple(rp.desc.shape) == (SLOTS, E, 12) and not ro.patch_async
    obs_m = torch.zeros((SLOTS, sc.K, E, P, P), device="cuda")
    fin_m = torch.zeros_like(obs_m)
    ro.reset()
    assert rp.use_desc
    obs_m[0].copy_(env.obs_patch(P))
    cover = _Cover(sc.H, sc.W, sc.N, sc.K, P)
    for t in range(1, 21):
        cur, nxt = (t - 1) % SLOTS, t % SLOTS
        ro.step()
        w, f = env.obs_patch(P, final=True)
        obs_m[nxt].copy_(w)
        fin_m[cur].copy_(f)
        if t in COMPARE_AT:
            cover.add(rp, *_compare(rp, P, (obs_m, fin_m)))
    cover.check()
    env.close()


class _DirectRing:
    """The ring built directly (the level below Rollout): the device-random policy drives the env, every step
    writes its rewards / terminations / dones into the ring's slots and gw_obs_desc_copy its descriptors."""

    def __init__(self, sc, P, E, fear=True, max_steps=12, seed=7):
        from marlnav.rollout import ReplayRing
        self.sc, self.P = sc, P
        self.env = VecGridEnv(sc, num_envs=E, fear=fear, fear_weight=-5.0, seed=seed, max_steps=max_steps,
                              auto_reset=True)
        self.rp = ReplayRing(self.env, SLOTS, patch=P, desc="only")
        self.rp.probs.copy_(torch.rand(self.rp.probs.shape, generator=torch.Generator().manual_seed(1)))
        self.obs_m = torch.zeros((SLOTS, sc.K, E, P, P), device="cuda")
        self.fin_m = torch.zeros_like(self.obs_m)
        self.env.reset()
        self._desc(0)
        self.rp.desc_ok = True
        self.obs_m[0].copy_(self.env.obs_patch(P))
        self.t = 0

    def _desc(self, slot):
        _lib.check(self.env.lib.gw_obs_desc_copy(self.env.handle, self.rp.desc[slot].data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "gw_obs_desc_copy")

    def step(self):
        rp, cur, nxt = self.rp, self.t % SLOTS, (self.t + 1) % SLOTS
        self.env.step(None, into=dict(shaped=rp.reward[cur], term=rp.term[cur], done=rp.done[cur]))
        self._desc(nxt)
        w, f = self.env.obs_patch(self.P, final=True)
        self.obs_m[nxt].copy_(w)
        self.fin_m[cur].copy_(f)
        self.t += 1
        rp.t = self.t
        rp.t_dev.fill_(self.t)


DIRECT_CASES = [("7x9_n3_k3", 5, 35), ("2x2_n4_k2", 2, 33), ("1x8_n2_k1", 3, 33), ("13x3_n3_k1", 9, 33),
                ("64x64_n8_k8", DP.MAXP, 36)]


@pytest.mark.parametrize("sid,P,E", DIRECT_CASES, ids=[c[0] for c in DIRECT_CASES])
def test_rows_equal_obs_patch_windows_direct(sid, P, E):
    """The shapes the fused window actor does not cover, at the ring's own level: E % 4 != 0; even P with window
    == map and free cells == N; H = 1 (overhang above and below); a window wider than the map; and the largest
    P gw_obs_patch takes on 64 x 64 with K = 8, whose mirror comes from the per-element wide-window writer (B
    limited to 2 E rows: the newest and the oldest stored transition)."""
    sc = SH.scenario(sid)
    ring = _DirectRing(sc, P, E, max_steps=SH.SWEEP["max_steps"], seed=SH.SWEEP["seed"])
    cover = _Cover(sc.H, sc.W, sc.N, sc.K, P)
    for t in range(1, SH.SWEEP["steps"] + 1):  # compared after every step: the shapes are small
        ring.step()
        n = min(t, SLOTS - 1)
        steps = (0, n - 1) if P == DP.MAXP else None
        cover.add(ring.rp, *_compare(ring.rp, P, (ring.obs_m, ring.fin_m), steps=steps))
    cover.check()
    ring.env.close()


def test_in_kernel_draws_pick_the_same_rows():
    """u = env = NULL: with the same seed and counter the new gather's tr_out and rows equal gw_replay_gather's on
    the mirror (both document the same Philox rule), at two counters."""
    ring = _DirectRing(SH.scenario("7x9_n3_k3"), 5, 35)
    for _ in range(9):
        ring.step()
    ctr = torch.tensor([5], dtype=torch.int32, device="cuda")
    trs = []
    for c in (5, 6):
        ctr.fill_(c)
        a = _gather(ring.rp, 5, B=512, seed=0x1234_5678_9ABC, ctr=ctr)
        b = _gather(ring.rp, 5, mirror=(ring.obs_m, ring.fin_m), B=512, seed=0x1234_5678_9ABC, ctr=ctr)
        torch.cuda.synchronize()
        _assert_equal(a, b)
        trs.append(a["tr"].clone())
    assert len(torch.unique(trs[0])) == SLOTS - 1 and not torch.equal(trs[0], trs[1])
    ring.env.close()


def _window_spans(desc_ring, fear):
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    sc = S.builtin("grid32")
    env = VecGridEnv(sc, num_envs=256, fear=fear, fear_weight=-5.0, seed=3, max_steps=6, auto_reset=True, obs=False)
    actors = MultiAgentActors(sc.K, 11, 11, "mlp", device="cuda", seed=1)
    ro = Rollout(env, actors, replay_slots=SLOTS, training=True, seed=4, patch=11, desc_ring=desc_ring)
    ro.reset()
    ro.step()
    torch.cuda.synchronize()
    env.profile(True, reserve=256)
    for _ in range(8):
        ro.step()
    torch.cuda.synchronize()
    kinds = env.profile_spans()[:, 0].astype(int).tolist()
    env.profile(False)
    env.close()
    return kinds


def test_no_window_writer_runs():
    """With gw_profile on, 8 steps of the descriptor-only rollout record no GW_SPAN_WINDOW span, FeAR off and on;
    the same steps on a dense window ring record one per step with FeAR off (gw_obs_patch after the step).  With
    FeAR on the dense ring's row writer rides inside the FeAR launch (gw_step_patch_next) and has no span of its
    own, so that pair cannot tell the two rings apart by spans; the FeAR-on descriptor-only rollout is checked
    to record other spans and no window span."""
    for fear in (False, True):
        kinds = _window_spans("only", fear)
        assert kinds and GW_SPAN_WINDOW not in kinds, kinds
    assert _window_spans(False, False).count(GW_SPAN_WINDOW) == 8


def test_resume_keeps_descriptor_rows():
    """Rollout.resume() on the descriptor-only ring against the test's mirror treated as resume treats a dense
    ring: the carried-over obs becomes the terminal obs of the last stored transition and its done flag is
    set.  Where that transition had already ended, its terminal obs is kept (the descriptor slot's own
    terminal half; the carried-over obs there is the next episode's reset obs).  Two resumes: after 10 steps
    with max_steps = 10 (the envs that never ended early are truncated at that step: done[prev] set) and 3
    steps later (most envs in mid-episode: the promoted step-encoded obs)."""
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    sc, P, E = S.builtin("grid32"), 11, 256
    env = VecGridEnv(sc, num_envs=E, fear=True, fear_weight=-5.0, seed=5, max_steps=10, auto_reset=True, obs=False)
    actors = MultiAgentActors(sc.K, P, P, "mlp", device="cuda", seed=2)
    ro = Rollout(env, actors, replay_slots=SLOTS, training=True, seed=1, patch=P, desc_ring="only")
    rp = ro.replay
    obs_m = torch.zeros((SLOTS, sc.K, E, P, P), device="cuda")
    fin_m = torch.zeros_like(obs_m)
    ro.reset()
    obs_m[0].copy_(env.obs_patch(P))

    def steps(n):
        for _ in range(n):
            cur, nxt = ro.t % SLOTS, (ro.t + 1) % SLOTS
            ro.step()
            w, f = env.obs_patch(P, final=True)
            obs_m[nxt].copy_(w)
            fin_m[cur].copy_(f)

    steps(10)
    seen_done = seen_live = 0
    for _ in range(2):
        cur, prev = ro.t % SLOTS, (ro.t - 1) % SLOTS
        was_done = rp.done[prev].bool().clone()
        seen_done += int(was_done.sum())
        seen_live += int((~was_done).sum())
        ro.resume()
        assert rp.desc_ok and rp.use_desc and bool(rp.done[prev].all())
        fin_m[prev][:, ~was_done] = obs_m[cur][:, ~was_done]
        obs_m[cur].copy_(env.obs_patch(P))
        _compare(rp, P, (obs_m, fin_m))
        steps(3)
        _compare(rp, P, (obs_m, fin_m))
        assert rp.desc_ok
    assert seen_done > 0 and seen_live > 0
    env.close()


def test_checkpoint_round_trip():
    from marlnav.rollout import ReplayRing
    ring = _DirectRing(SH.scenario("7x9_n3_k3"), 5, 35)
    for _ in range(8):
        ring.step()
    rp = ring.rp
    sd = {k: v.detach().clone().cpu() for k, v in rp.state_dict().items()}
    assert "desc" in sd and "obs" not in sd and "final_obs" not in sd
    fresh = ReplayRing(ring.env, SLOTS, patch=5, desc="only")
    assert not fresh.use_desc
    fresh.load_state_dict({k: v.cuda() for k, v in sd.items()})
    assert fresh.use_desc and fresh.t == rp.t and int(fresh.t_dev) == int(rp.t_dev)
    _compare(rp, 5, (ring.obs_m, ring.fin_m), other=fresh)
    bad = dict(sd, desc=sd["desc"][:, :-1])
    with pytest.raises(ValueError, match="desc"):
        fresh.load_state_dict({k: v.cuda() for k, v in bad.items()})
    del bad["desc"]
    with pytest.raises(ValueError, match="desc"):
        fresh.load_state_dict({k: v.cuda() for k, v in bad.items()})
    ring.env.close()


def test_training_on_desc_windows_equals_dense_windows():
    """Two MADDPGTrainer(patch=11) from the same seeds on grid32, one on the descriptor-only ring (the default with
    the fused MLP window actor), one with its rollout forced to the dense window ring: after 24 env steps with
    updates every weight is equal.  The descriptor-only trainer never runs the full-grid descriptor learner."""
    from marlnav.maddpg import MADDPG
    from marlnav.rollout import Rollout
    from marlnav.train import MADDPGTrainer
    sc = S.builtin("grid32")
    states = []
    for only in (True, False):
        torch.manual_seed(5)  # the captured update draws from the default generators
        env = VecGridEnv(sc, num_envs=256, fear=True, fear_weight=-5.0, stats=True, seed=7, max_steps=10, obs=False)
        m = MADDPG(sc.K, 11, 11, device=env.device, seed=3, capturable=True)
        tr = MADDPGTrainer(env, m, memory_size=2048, updates_per_step=1, graph=True, seed=3, patch=11)
        assert tr.rollout.desc_only and tr.rollout.replay.obs is None
        if not only:
            tr.rollout = Rollout(env, m.actors, replay_slots=tr.rollout.replay.S, training=True, seed=3, patch=11)
            assert not tr.rollout.desc_only and tr.rollout.replay.desc is None
        tr.reset()
        assert tr.rollout.replay.use_desc == only
        assert not m.desc_capable(tr.rollout.replay)
        tr.train(24)
        torch.cuda.synchronize()
        assert tr.updates > 10
        assert not m._desc and not getattr(m, "_capture_is_desc", False)  # no full-grid descriptor update ran
        states.append({k: v.clone() for k, v in m.state_dict().items()})
        env.close()
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k


def test_trainer_patch_needs_matching_networks():
    from marlnav.maddpg import MADDPG
    from marlnav.train import MADDPGTrainer
    sc = S.builtin("grid32")
    env = VecGridEnv(sc, num_envs=64, fear=False, seed=7, obs=False)
    m = MADDPG(sc.K, 9, 9, device=env.device, seed=3)
    with pytest.raises(ValueError, match="patch=11"):
        MADDPGTrainer(env, m, memory_size=512, patch=11)
    env.close()


def test_argument_errors():
    from marlnav.actor import MultiAgentActors
    from marlnav.rollout import Rollout
    ring = _DirectRing(SH.scenario("7x9_n3_k3"), 5, 35)
    ring.step()
    rp, L = ring.rp, _lib.load()
    B, K = 8, rp.K
    u, env = _exhaustive_draws(rp)
    u, env = u[:B].contiguous(), env[:B].contiguous()
    st = torch.empty((K, B, 5, 5), device="cuda")
    pr = torch.empty((K, B, 9), device="cuda")
    rw = torch.empty((B, K), dtype=torch.float64, device="cuda")
    tm = torch.empty((B, K), dtype=torch.uint8, device="cuda")

    def call(src=rp._src, P=5, state=st.data_ptr(), probs_out=pr.data_ptr(), x=None):
        return L.gw_replay_gather_desc_patch(C.byref(src), rp.desc.data_ptr(), rp.probs.data_ptr(),
                                             rp.reward.data_ptr(), rp.term.data_ptr(), rp.done.data_ptr(),
                                             rp.t_dev.data_ptr(), u.data_ptr(), env.data_ptr(), rp.S, B, P, state,
                                             st.data_ptr(), probs_out, rw.data_ptr(), tm.data_ptr(), None, x, x, 0,
                                             None, torch.cuda.current_stream().cuda_stream)

    assert call() == 0
    for kw, msg in ((dict(P=0), "P <= 129"), (dict(P=130), "P <= 129"), (dict(state=None), "state"),
                    (dict(probs_out=None), "probs_out")):
        assert call(**kw) == GW_ERR_ARG, kw
        assert msg in L.gw_last_error().decode(), (kw, L.gw_last_error())
    big = _lib.GwObsSource.from_buffer_copy(rp._src)
    big.H, big.W = 65, 64  # H * W > 4096
    assert call(src=big) == GW_ERR_ARG and "4096" in L.gw_last_error().decode()
    torch.cuda.synchronize()
    ring.env.close()
    # Rollout(desc_ring="only"): the conditions, each with its own message
    sc = S.builtin("grid64_n8")
    env = VecGridEnv(sc, num_envs=64, fear=False, seed=3, obs=False)
    cnn = MultiAgentActors(sc.K, 16, 16, "cnn", device="cuda", seed=1)
    mlp = MultiAgentActors(sc.K, 16, 16, "mlp", device="cuda", seed=1)
    with pytest.raises(ValueError, match="CNN head"):
        Rollout(env, cnn, replay_slots=4, patch=16, desc_ring="only")
    with pytest.raises(ValueError, match="fused window actor"):
        Rollout(env, mlp, replay_slots=4, patch=16, desc_ring="only", fused=False)
    with pytest.raises(ValueError, match="replay ring"):
        Rollout(env, mlp, replay_slots=0, patch=16, desc_ring="only")
    full = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=1)
    with pytest.raises(ValueError, match="patch > 0"):
        Rollout(env, full, replay_slots=4, desc_ring="only")
    env.close()
