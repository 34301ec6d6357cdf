"""The ride (fear_delta_kernel): on the defer path an eager async step whose obs writer is the delta
writer runs that writer as a block role of the FeAR launch on the step's own stream.  Where a step
rides is result-neutral, so every case steps an env with the ride on, a twin built with
GW_OBS_RIDE=0 (the obs streams' pipeline) and the C oracle together: every output of every step is
bit-identical between the two envs, and the obs equal the oracle's (as tests/test_gpu_obs_delta.py).

gw_obs_ride_count says which steps rode: every delta write of the steady eager cases (the first
write into a destination is a full one and does not ride), none with GW_OBS_CHUNKS=2, lazy or
synchronous obs, profiling, final_obs or captured steps.  The env counts are ragged on both sides of
FeAR's 64-env blocks and of the writer's blocks (128 envs at K = 2; 85 at K = 3, which does not
divide the 256 threads).  Short episodes (max_steps 5) put auto-resets into every few steps."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from marlnav import _lib
from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu

SCENES = {
    "grid32": lambda: S.builtin("grid32"),
    "grid64_n8": lambda: S.builtin("grid64_n8"),
    "k3n5": lambda: S.compile_scenario(S.level3_like(10, 16, 5, 3)),  # K = 3 (no built-in scenario has it)
}
STEPS = 40
STEP, OBS, FEAR = 0, 1, 2  # GW_SPAN_* (include/gridenv.h)
FIELDS = ("reward", "fear", "shaped", "term", "trunc", "done", "ep_return", "ep_fear", "stats")


@pytest.fixture(autouse=True)
def defer_path(monkeypatch):
    monkeypatch.setenv("GW_KERNEL", "defer")
    for name in ("GW_OBS_DELTA", "GW_OBS_RIDE", "GW_OBS_CHUNKS", "GW_OBS_STREAMS", "GW_FEAR_BE"):
        monkeypatch.delenv(name, raising=False)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Pair:
    """An env with the ride on, its twin with GW_OBS_RIDE=0 and the oracle, stepped together."""

    def __init__(self, monkeypatch, scene="grid32", E=128, mode="eager", seed=5, final_obs=False, environ=None):
        self.sc = sc = SCENES[scene]()
        self.E = E
        kw = dict(num_envs=E, fear=True, fear_weight=-5.0, max_steps=5, auto_reset=True, seed=seed, stats=True,
                  final_obs=final_obs)
        for name, value in (environ or {}).items():
            monkeypatch.setenv(name, value)
        self.env = VecGridEnv(sc, **kw)
        monkeypatch.setenv("GW_OBS_RIDE", "0")
        self.twin = VecGridEnv(sc, **kw)  # a fresh env: the switch is read when an env is built
        monkeypatch.delenv("GW_OBS_RIDE")
        assert self.env.kernel_path == "defer" and self.env.obs_delta and self.twin.obs_delta
        self.set_mode(mode)
        self.orc = O.OracleEnvs(sc, E, fear=True, fear_weight=-5.0, max_steps=5, seed=seed, reset=False)
        self.obs_o = np.zeros((sc.K, E, sc.HW), np.float32)
        self.outs = (O.StepOut * E)()
        self.oracle = True
        self.orc.reset_all(obs=self.obs_o)
        self.reset()
        self.ended = 0

    def set_mode(self, mode):
        for e in (self.env, self.twin):
            e.set_obs_async(False if mode == "sync" else ("lazy" if mode == "lazy" else True))

    def reset(self):
        obs = [e.reset()[0] for e in (self.env, self.twin)]
        torch.cuda.synchronize()
        assert torch.equal(_bits(obs[0]), _bits(obs[1]))
        if self.oracle:
            np.testing.assert_array_equal(obs[0].reshape(self.sc.K, self.E, -1).cpu().numpy(), self.obs_o)

    def launch(self, dest=None, tdest=None):
        """One step of all three, nothing fenced or compared."""
        r, q = self.env.step(obs_out=dest), self.twin.step(obs_out=tdest)
        if self.oracle:
            self.orc.vec_step(None, obs=self.obs_o, outs=self.outs)
        return r, q

    def check(self, r, q, tag):
        K, E = self.sc.K, self.E
        self.env.obs_fence()
        self.twin.obs_fence()
        torch.cuda.synchronize()
        assert self.twin.obs_ride_count() == 0
        assert torch.equal(_bits(r.obs), _bits(q.obs)), f"{tag} obs vs the twin"
        for name in FIELDS:
            a, b = getattr(r, name), getattr(q, name)
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{tag} {name} vs the twin"
        if self.oracle:
            np.testing.assert_array_equal(r.obs.reshape(K, E, -1).cpu().numpy(), self.obs_o, err_msg=f"{tag} obs")
            fear = np.array([list(self.outs[e].fear)[:K] for e in range(E)])
            np.testing.assert_array_equal(r.fear.cpu().numpy(), fear, err_msg=f"{tag} fear")
        self.ended += int(r.done.sum())

    def step(self, dest=None, tdest=None, tag=""):
        """One checked step; -> (full, delta, rode) writers it added to the env with the ride on."""
        c0 = self.env.obs_delta_counts() + (self.env.obs_ride_count(),)
        r, q = self.launch(dest, tdest)
        self.check(r, q, tag)
        c1 = self.env.obs_delta_counts() + (self.env.obs_ride_count(),)
        return tuple(b - a for a, b in zip(c0, c1))

    def close(self):
        self.env.close()
        self.twin.close()


def _ring(env, n):
    base = torch.empty((n,) + tuple(env.out["obs"].shape), dtype=torch.float32, device=env.device)
    return [base[i] for i in range(n)]


CASES = [("grid32", E) for E in (1, 63, 64, 65, 127, 128, 129, 200)] + [("k3n5", 100), ("grid64_n8", 33)]


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("scene,E", CASES)
def test_riding_steps_equal_the_twin_and_the_oracle(monkeypatch, scene, E, slots):
    """One obs buffer every step, and a 2-slot ring (the benchmark's pattern): the first write into
    each destination is full and does not ride, every later step's delta writer rides."""
    t = Pair(monkeypatch, scene, E)
    ring, tring = _ring(t.env, slots), _ring(t.twin, slots)
    for i in range(STEPS):
        got = t.step(ring[i % slots], tring[i % slots], f"{scene} E={E} t={i}")
        assert got == ((1, 0, 0) if i < slots else (0, 1, 1)), (i, got)
    assert t.env.obs_ride_count() == t.env.obs_delta_counts()[1] == STEPS - slots
    assert t.twin.obs_delta_counts() == (slots, STEPS - slots)
    assert t.ended > E  # many auto-resets went through the riding writer
    t.close()


def test_unfenced_steps_between_checks(monkeypatch):
    """Riding steps issued back to back (no fence, no host wait between them, two ring slots): the
    writer of step t and the world update of step t+1 are ordered by the stream alone."""
    t = Pair(monkeypatch, "grid32", 200)
    ring, tring = _ring(t.env, 2), _ring(t.twin, 2)
    for i in range(STEPS):
        r, q = t.launch(ring[i % 2], tring[i % 2])
        if i % 8 == 7:
            t.check(r, q, f"burst t={i}")
    assert t.env.obs_ride_count() == STEPS - 2
    assert torch.equal(_bits(ring[0]), _bits(tring[0])) and torch.equal(_bits(ring[1]), _bits(tring[1]))
    t.close()


@pytest.mark.parametrize("case", ["chunks2", "lazy", "sync", "final_obs"])
def test_steps_that_never_ride(monkeypatch, case):
    t = Pair(monkeypatch, "grid32", 129, mode=case if case in ("lazy", "sync") else "eager",
             final_obs=case == "final_obs", environ={"GW_OBS_CHUNKS": "2"} if case == "chunks2" else None)
    for i in range(12):
        got = t.step(None, None, f"{case} t={i}")
        assert got == ((1, 0, 0) if i == 0 else (0, 1, 0)), (i, got)
    assert t.env.obs_ride_count() == 0
    t.close()


def test_profiled_steps_keep_their_launches(monkeypatch):
    """Profiling on: no step rides, and the span kinds are those of the obs streams' pipeline."""
    t = Pair(monkeypatch, "grid32", 129)
    for e in (t.env, t.twin):
        e.profile(True)
    for i in range(6):
        assert t.step(None, None, f"prof t={i}")[2] == 0
    kinds = [[int(k) for k in e.profile_spans()[:, 0]] for e in (t.env, t.twin)]
    assert kinds[0] == kinds[1] == [STEP, FEAR, OBS] * 6
    assert t.env.obs_ride_count() == 0
    t.close()


def test_captured_steps_do_not_ride(monkeypatch):
    """A graph of captured steps (synchronous obs: the defer path's async pipeline is not capturable)
    records full writes; its replays equal the twin's eager steps, and no step rode."""
    n = 4
    t = Pair(monkeypatch, "grid32", 129, mode="sync")
    for i in range(3):
        t.step(None, None, f"pre t={i}")
    graph = t.env.capture_steps(n)
    for rep in range(2):
        graph.replay()
        for _ in range(n):
            q = t.twin.step()
            t.orc.vec_step(None, obs=t.obs_o, outs=t.outs)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(t.env.out["obs"].reshape(t.sc.K, t.E, -1).cpu().numpy(), t.obs_o)
        assert torch.equal(_bits(t.env.out["obs"]), _bits(q.obs))
    t.set_mode("eager")
    for i in range(4):
        assert t.step(None, None, f"post t={i}") == ((1, 0, 0) if i == 0 else (0, 1, 1))
    assert t.env.obs_ride_count() == 3
    t.close()


def test_torch_write_between_steps(monkeypatch):
    """A copy_ into the destination between two steps: forgotten, one full write on the obs stream
    (which follows the riding writers of the caller's stream), then riding again."""
    t = Pair(monkeypatch, "grid32", 129)
    buf, tbuf = torch.empty_like(t.env.out["obs"]), torch.empty_like(t.twin.out["obs"])
    for i in range(STEPS):
        if i in (9, 10, 25):
            buf.copy_(torch.full_like(buf, float("nan")))
        got = t.step(buf, tbuf, f"copy t={i}")
        assert got == ((1, 0, 0) if i in (0, 9, 10, 25) else (0, 1, 1)), (i, got)
    assert t.env.obs_ride_count() == STEPS - 4
    t.close()


def test_profiling_toggled_mid_run(monkeypatch):
    """Riding steps, profiled steps (the delta writer on the obs stream, behind the riding writers of
    its destination), riding steps again (behind that writer), over a 2-slot ring."""
    t = Pair(monkeypatch, "grid32", 200)
    ring, tring = _ring(t.env, 2), _ring(t.twin, 2)
    for i in range(STEPS):
        if i in (10, 15, 21, 22):
            for e in (t.env, t.twin):
                e.profile(i in (10, 21))
        prof = 10 <= i < 15 or i == 21
        got = t.step(ring[i % 2], tring[i % 2], f"toggle t={i}")
        assert got == ((1, 0, 0) if i < 2 else (0, 1, 0 if prof else 1)), (i, got)
    assert t.env.obs_ride_count() == STEPS - 2 - 6
    t.close()


def test_lazy_then_eager(monkeypatch):
    """Lazy steps leave their writer queued; the first eager step launches it on the obs stream and
    rides itself, ordered behind it by the destination's event (one buffer) and the descriptor
    buffer's (two steps later).  No fence between the last lazy and the first eager step."""
    t = Pair(monkeypatch, "grid32", 200, mode="lazy")
    ring, tring = _ring(t.env, 2), _ring(t.twin, 2)
    for i in range(9):
        assert t.step(ring[i % 2], tring[i % 2], f"lazy t={i}")[2] == 0
    t.launch(ring[1], tring[1])  # step 9: its writer stays queued
    want = t.obs_o.copy()
    t.set_mode("eager")
    for i in range(10, STEPS):
        got = t.step(ring[i % 2], tring[i % 2], f"eager t={i}")
        assert got[2] == 1 and got[0] == 0, (i, got)
        if i == 10:  # step 9's obs, written by the queued writer behind step 10's launch
            np.testing.assert_array_equal(ring[1].reshape(t.sc.K, t.E, -1).cpu().numpy(), want)
            assert torch.equal(_bits(ring[1]), _bits(tring[1]))
    assert t.env.obs_ride_count() == STEPS - 10
    t.close()


def test_reset_mid_run(monkeypatch):
    """gw_reset forgets every destination: a full write, then riding again.  The oracle checks the
    steps before the reset (its reset restarts the episode counters, gw_reset's does not); the twin
    checks all of them."""
    t = Pair(monkeypatch, "grid32", 129)
    for i in range(12):
        assert t.step(None, None, f"a t={i}") == ((1, 0, 0) if i == 0 else (0, 1, 1))
    t.oracle = False
    t.reset()
    for i in range(12):
        assert t.step(None, None, f"b t={i}") == ((1, 0, 0) if i == 0 else (0, 1, 1))
    assert t.env.obs_ride_count() == 22
    t.close()


def test_switch_values(monkeypatch):
    """GW_OBS_RIDE takes 0 or 1 only."""
    monkeypatch.setenv("GW_OBS_RIDE", "1")
    VecGridEnv("grid32", num_envs=4, fear=True).close()
    for bad in ("2", "", "on"):
        monkeypatch.setenv("GW_OBS_RIDE", bad)
        with pytest.raises(_lib.GwError):
            VecGridEnv("grid32", num_envs=4, fear=True)
