"""The delta obs writer (gw_set_obs_delta): a step into a buffer the env wrote last stores only the
changed cells, and every step's obs / final_obs stays bit-identical to the C oracle (native RNG, as
tests/test_gpu_parity.py) and to a second env with the delta table off.

Every case asserts with gw_obs_delta_counts which writer ran: the delta writer in the steady
cases, the full writer wherever the destination's bytes may be anything else (a buffer never
written, written through torch, forgotten, evicted, written in the other dtype, reset, captured).
Short episodes (max_steps 7) give many auto-resets and terminal obs within each run."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu

SCENES = {
    "level3": (lambda: S.builtin("level3"), 64, 0),
    "grid32": (lambda: S.builtin("grid32"), 256, 0),
    "grid64_n8": (lambda: S.builtin("grid64_n8"), 32, 0),
    "level3_single": (lambda: S.builtin("level3_single"), 64, 1),
    "k3n5": (lambda: S.compile_scenario(S.level3_like(10, 16, 5, 3)), 64, 0),  # as the parity suite's K > 2 case
}
STEPS = 32


@pytest.fixture(autouse=True)
def defer_path(monkeypatch):
    """The delta writer covers the defer kernel path (small batches would pick the merged one)."""
    monkeypatch.setenv("GW_KERNEL", "defer")
    monkeypatch.delenv("GW_OBS_DELTA", raising=False)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Trio:
    """An env with the delta table on, one with it off, and the oracle, stepped together."""

    def __init__(self, scene="grid32", E=None, mode="eager", seed=7, max_steps=7, final_obs=True):
        mk, e_def, variant = SCENES[scene]
        self.sc = sc = mk()
        self.E = E = E or e_def
        kw = dict(num_envs=E, fear=True, fear_weight=-5.0, max_steps=max_steps, auto_reset=True, seed=seed,
                  final_obs=final_obs, variant=variant)
        self.env, self.ref = VecGridEnv(sc, **kw), VecGridEnv(sc, **kw)
        assert self.env.kernel_path == "defer" and self.env.obs_delta
        self.ref.set_obs_delta(False)
        if mode != "sync":
            for e in (self.env, self.ref):
                e.set_obs_async("lazy" if mode == "lazy" else True)
        self.orc = O.OracleEnvs(sc, E, fear=True, fear_weight=-5.0, max_steps=max_steps, seed=seed, reset=False,
                                variant=variant)
        self.obs_o = np.zeros((sc.K, E, sc.HW), np.float32)
        self.fin_o = np.zeros((sc.K, E, sc.HW), np.float32)
        self.outs = (O.StepOut * E)()
        self.ended = 0
        self.oracle = True
        self.ringed = False
        self.reset()

    def reset(self):
        """The first reset is the oracle's too; a later one (the oracle's restarts its episode
        counters, gw_reset's does not) leaves the table-off env as the only reference."""
        if self.ended or self.counts()[0]:
            self.oracle = False
        else:
            self.orc.reset_all(obs=self.obs_o)
        obs = [e.reset()[0] for e in (self.env, self.ref)]
        torch.cuda.synchronize()
        assert torch.equal(_bits(obs[0]), _bits(obs[1]))
        if self.oracle:
            np.testing.assert_array_equal(obs[0].reshape(self.sc.K, self.E, -1).cpu().numpy(), self.obs_o)

    def counts(self):
        return self.env.obs_delta_counts()

    def step(self, dest=None, tag="", fdest=None):
        """One step of all three (the delta env's obs into ``dest``, its terminal obs into ``fdest``);
        -> (full, delta) writers it added.  The async pipeline alternates its two obs streams only when
        BOTH buffers differ from the last writer's, so a ring of obs needs a ring of final_obs (or an env
        without final_obs, as the benchmark's) for consecutive writers to run on different streams."""
        K, E = self.sc.K, self.E
        c0 = self.counts()
        self.ringed = self.ringed or fdest is not None  # from then on the own buffers hold different rows
        r = self.env.step(obs_out=dest, final_obs_out=fdest)
        q = self.ref.step()
        if self.oracle:
            self.orc.vec_step(None, obs=self.obs_o, outs=self.outs, final_obs=self.fin_o)
        self.env.obs_fence()
        self.ref.obs_fence()
        torch.cuda.synchronize()
        c1 = self.counts()
        assert self.ref.obs_delta_counts()[1] == 0
        assert torch.equal(_bits(r.obs), _bits(q.obs)), f"{tag} obs vs the table-off env"
        assert torch.equal(r.done, q.done), f"{tag} done"
        ended = np.flatnonzero(r.done.cpu().numpy())
        if r.final_obs is None:
            assert q.final_obs is None
        elif fdest is None and not self.ringed:  # both envs' own buffers: the same rows written since the start
            assert torch.equal(_bits(r.final_obs), _bits(q.final_obs)), f"{tag} final_obs vs the table-off env"
        else:  # the rows this step wrote
            assert torch.equal(_bits(r.final_obs[:, ended]), _bits(q.final_obs[:, ended])), f"{tag} final_obs rows"
        if self.oracle:
            np.testing.assert_array_equal(r.obs.reshape(K, E, -1).cpu().numpy(), self.obs_o, err_msg=f"{tag} obs")
            dn = np.array([self.outs[e].done for e in range(E)])
            np.testing.assert_array_equal(r.done.cpu().numpy(), dn, err_msg=f"{tag} done")
            if r.final_obs is not None:
                np.testing.assert_array_equal(r.final_obs.reshape(K, E, -1)[:, ended].cpu().numpy(),
                                              self.fin_o[:, ended], err_msg=f"{tag} final_obs")
        self.ended += len(ended)
        return c1[0] - c0[0], c1[1] - c0[1]

    def close(self):
        self.env.close()
        self.ref.close()


def _ring(env, n):
    base = torch.empty((n,) + tuple(env.out["obs"].shape), dtype=env.out["obs"].dtype, device=env.device)
    return base, [base[i] for i in range(n)]


def _fring(env, n):
    """n terminal-obs buffers (NaN where no env ended yet, as the env's own)."""
    return [torch.full_like(env.out["obs"], float("nan")) for _ in range(n)]


@pytest.mark.parametrize("slots", [1, 2, 5])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_steady_destinations_take_the_delta_writer(scene, slots):
    """One buffer every step, a 2-slot and a 5-slot ring (obs slots views of one tensor, the terminal
    obs ringed beside them, async obs): consecutive writers of the rings alternate between the two obs
    streams, so with 5 slots a delta writer follows the previous writer of its buffer from the OTHER
    stream (the entry's event orders them); with 2 slots a buffer stays on one stream.  The first step
    into each slot is a full write, every later one a delta."""
    t = Trio(scene)
    _, ring = _ring(t.env, slots)
    fring = _fring(t.env, slots)
    for i in range(STEPS):
        full, delta = t.step(ring[i % slots], f"{scene} t={i}", fring[i % slots])
        assert (full, delta) == ((1, 0) if i < slots else (0, 1)), (i, full, delta)
    assert t.ended > t.E  # many terminal obs and auto-resets went through the delta writer
    t.close()


@pytest.mark.parametrize("slots", [2, 5])
def test_obs_rings_without_final_obs(slots):
    """The benchmark's pattern: no final_obs, a ring of obs buffers, async obs on the two obs streams."""
    t = Trio("grid32", final_obs=False)
    _, ring = _ring(t.env, slots)
    for i in range(STEPS):
        assert t.step(ring[i % slots], f"nofinal t={i}") == ((1, 0) if i < slots else (0, 1))
    t.close()


@pytest.mark.parametrize("mode", ["sync", "eager", "lazy"])
def test_obs_modes(mode):
    t = Trio("grid32", mode=mode)
    _, ring = _ring(t.env, 2)
    fring = _fring(t.env, 3)
    tot = [0, 0]
    for i in range(STEPS):
        own = i % 8 >= 6  # the env's own buffers now and then
        d = t.step(None if own else ring[i % 2], f"{mode} t={i}", None if own else fring[i % 3])
        tot = [tot[0] + d[0], tot[1] + d[1]]
    assert tot == [3, STEPS - 3]
    t.close()


@pytest.mark.parametrize("E", [1, 77, 333])
def test_ragged_env_counts(E):
    """E not a multiple of the delta writer's envs per block (128 at K = 2), one and several blocks."""
    t = Trio("grid32", E=E)
    for i in range(16):
        assert t.step(None, f"E={E} t={i}") == ((1, 0) if i == 0 else (0, 1))
    t.close()


def test_chunked_writer(monkeypatch):
    monkeypatch.setenv("GW_OBS_CHUNKS", "2")
    t = Trio("grid32")
    _, ring = _ring(t.env, 5)
    fring = _fring(t.env, 5)
    for i in range(20):
        assert t.step(ring[i % 5], f"chunks t={i}", fring[i % 5]) == ((1, 0) if i < 5 else (0, 1))
    t.close()


def test_fresh_destination_every_step_is_always_full():
    t = Trio("level3")
    for i in range(20):
        assert t.step(torch.empty_like(t.env.out["obs"]), f"fresh t={i}") == (1, 0)  # the old ones are dropped
    t.close()


def test_torch_writes_force_a_full_rewrite():
    """A NaN fill of the destination, and a copy_ into ANOTHER slot of the same ring (views share
    the version counter: the whole ring is distrusted, once)."""
    t = Trio("grid32")
    buf = torch.empty_like(t.env.out["obs"])
    for i in range(12):
        if i in (5, 9):
            buf.fill_(float("nan"))
        assert t.step(buf, f"nan t={i}") == ((1, 0) if i in (0, 5, 9) else (0, 1))
    base, ring = _ring(t.env, 5)
    for i in range(25):
        if i == 12:
            ring[(i + 2) % 5].copy_(t.ref.out["obs"])
        full = i < 5 or 12 <= i < 17
        assert t.step(ring[i % 5], f"copy t={i}") == ((1, 0) if full else (0, 1))
    t.close()


def test_forget_called_directly():
    t = Trio("level3")
    buf = torch.empty_like(t.env.out["obs"])
    other = torch.empty_like(buf)
    for i in range(14):
        dest = other if i % 2 else buf
        if i == 6:  # what a raw-pointer writer must be followed by
            buf.data.view(torch.int32).bitwise_not_()  # .data: its own version counter, so the guard is blind
            _lib.check(t.env.lib.gw_obs_dest_forget(t.env.handle, buf.data_ptr()), "gw_obs_dest_forget")
        if i == 10:
            t.env.obs_dest_forget(None)  # every destination
        assert t.step(dest, f"forget t={i}") == ((1, 0) if i in (0, 1, 6, 10, 11) else (0, 1))
    t.close()


def test_more_destinations_than_entries():
    """GW_OBS_DESTS + 1 buffers in turn: each comes back after it was evicted, so each write is full;
    GW_OBS_DESTS buffers in turn all stay known."""
    t = Trio("level3")
    bufs = [torch.empty_like(t.env.out["obs"]) for _ in range(_lib.GW_OBS_DESTS + 1)]
    for i in range(2 * len(bufs)):
        assert t.step(bufs[i % len(bufs)], f"lru9 t={i}") == (1, 0)
    t.env.obs_dest_forget(None)
    n = _lib.GW_OBS_DESTS
    for i in range(3 * n):
        assert t.step(bufs[i % n], f"lru8 t={i}") == ((1, 0) if i < n else (0, 1))
    t.close()


def test_dtype_round_trip():
    """f32 -> bf16 -> f32 into the same bytes: the bf16 steps are full writes and leave no entry."""
    t = Trio("grid32")
    for i in range(4):
        t.step(None, f"f32a t={i}")
    raw = t.env.out["obs"]
    for e in (t.env, t.ref):
        _lib.check(e.lib.gw_set_obs_dtype(e.handle, 1), "gw_set_obs_dtype")
        e.obs_dtype = torch.bfloat16
        e._into_cache.clear()
    half = [x.out["obs"].view(torch.bfloat16).reshape(-1)[: raw.numel()].view(raw.shape) for x in (t.env, t.ref)]
    K, E = t.sc.K, t.E
    for i in range(4):
        c0 = t.counts()
        r, q = t.env.step(obs_out=half[0]), t.ref.step(obs_out=half[1])
        t.orc.vec_step(None, obs=t.obs_o, outs=t.outs, final_obs=t.fin_o)
        for e in (t.env, t.ref):
            e.obs_fence()
        torch.cuda.synchronize()
        c1 = t.counts()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 0)
        np.testing.assert_array_equal(r.obs.reshape(K, E, -1).float().cpu().numpy(), t.obs_o, err_msg=f"bf16 t={i}")
        assert torch.equal(_bits(r.obs), _bits(q.obs))
    for e in (t.env, t.ref):
        _lib.check(e.lib.gw_set_obs_dtype(e.handle, 0), "gw_set_obs_dtype")
        e.obs_dtype = torch.float32
        e._into_cache.clear()
    for i in range(6):
        assert t.step(None, f"f32b t={i}") == ((1, 0) if i == 0 else (0, 1))
    t.close()


def test_reset_into_a_known_destination():
    t = Trio("grid32")
    for i in range(5):
        t.step(None, f"a t={i}")
    t.reset()  # writes the env's own obs buffer, which the table knew
    for i in range(8):
        assert t.step(None, f"b t={i}") == ((1, 0) if i == 0 else (0, 1))
    t.close()


def test_captured_steps_are_full_writes_and_equal_eager():
    """A captured graph of steps records full writes (the host cannot vet a replay) and forgets every
    destination; the replays equal the eager run, and so do the eager steps after them."""
    n = 4
    t = Trio("grid32", mode="sync")
    for i in range(3):
        t.step(None, f"pre t={i}")
    c0 = t.counts()
    graph = t.env.capture_steps(n)
    c1 = t.counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (n, 0)
    K, E = t.sc.K, t.E
    for rep in range(3):
        graph.replay()
        for _ in range(n):
            q = t.ref.step()
            t.orc.vec_step(None, obs=t.obs_o, outs=t.outs, final_obs=t.fin_o)
        torch.cuda.synchronize()
        assert t.counts() == c1
        np.testing.assert_array_equal(t.env.out["obs"].reshape(K, E, -1).cpu().numpy(), t.obs_o, err_msg=f"rep {rep}")
        assert torch.equal(_bits(t.env.out["obs"]), _bits(q.obs))
        assert torch.equal(_bits(t.env.out["final_obs"]), _bits(q.final_obs))
    for i in range(6):
        assert t.step(None, f"post t={i}") == ((1, 0) if i == 0 else (0, 1))
    t.close()


def test_lazy_writer_vets_its_destination_when_it_is_launched():
    """Lazy async obs: the writer of step t is launched inside step t+1.  A torch write to its
    destination between the two steps (ordered before the writer on the stream) must make it a full
    writer, so the buffer ends up holding the complete obs of step t."""
    t = Trio("grid32", mode="lazy")
    a, b = torch.empty_like(t.env.out["obs"]), torch.empty_like(t.env.out["obs"])
    for i in range(4):
        t.step(b if i % 2 else a, f"warm t={i}")
    c0 = t.counts()
    t.env.step(obs_out=a)  # its (delta) writer stays queued
    q = t.ref.step()
    t.ref.obs_fence()
    want = q.obs.clone()
    a.fill_(float("nan"))
    t.env.step(obs_out=b)  # launches the queued writer of `a` first
    t.ref.step()
    t.env.obs_fence()
    t.ref.obs_fence()
    torch.cuda.synchronize()
    c1 = t.counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 1)  # `a` in full, `b` by delta
    assert torch.equal(_bits(a), _bits(want))
    assert torch.equal(_bits(b), _bits(t.ref.out["obs"]))
    t.close()
