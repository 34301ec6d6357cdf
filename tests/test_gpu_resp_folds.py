"""Every responsibility fold armed at once (marlnav/resp_folds.py through Rollout and evaluate).

Each keyword alone is pinned to a host fold by its own test (test_gpu_fear_rows, _fear_alt, _feal, _fear_full,
_resp_map, _resp_footprint), so the single-keyword runs are the reference here: a run with all six armed must give
every one of their keys bit for bit, which pins the slices ``totals()`` cuts out of its one float64 vector with
every part present.  grid32 (N = 4, K = 2), E = 200 envs: no multiple of the 64-env wave or the 256-env block, so
the folds' tails are in play; 12 steps with max_steps = 8, so envs reset inside the run."""
import pytest
import torch

from marlnav import scenario as S
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu

E, STEPS, R = 200, 12, 5
ALL = dict(resp_matrix=True, fear_regret=True, feal=True, resp_full=True, resp_map=True, resp_footprint=R)
SHAPES = {"resp": (2, 4), "fear_regret": (2,), "fear_best": (2,), "feal_sum": (4,), "resp_full": (4, 4),
          "resp_map_counts": (2, 1024, 10, 10), "resp_map_visits": (1024,), "resp_map": (2, 32, 32),
          "resp_footprint_counts": (2, 9, 122, 10, 10), "resp_footprint_visits": (9,), "resp_footprint": (2, 9, 122)}
COUNTS = ("resp_steps", "fear_regret_steps", "feal_envs", "feal_steps", "resp_full_steps")


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return type(a) is type(b) and a == b


def _rollout(fear_async=False, **kw):
    from marlnav.rollout import Rollout
    env = VecGridEnv("grid32", num_envs=E, fear=True, fear_weight=-5.0, max_steps=8, seed=9, stats=True,
                     fear_rows=True, fear_alt=True, feal=True, fear_full=True, debug=True)
    try:
        ro = Rollout(env, None, obs_async=fear_async, fear_async=fear_async, **kw)
        ro.reset()
        for _ in range(STEPS):
            ro.step()
        ro.fence()
        tot = ro.totals()
        torch.cuda.synchronize()
        return tot
    finally:
        env.close()


@pytest.mark.parametrize("fear_async", [False, True], ids=["joined", "fear_async"])
def test_rollout_all_folds_equal_each_alone(monkeypatch, fear_async):
    monkeypatch.setenv("GW_KERNEL", "defer")  # (the path whose FeAR can stay unjoined)
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    every = _rollout(fear_async, **ALL)
    assert every["env_steps"] == E * STEPS and every["episodes"] > 0  # envs were reset inside the run
    seen = set()
    for kw, v in ALL.items():
        alone = _rollout(fear_async, **{kw: v})
        assert set(alone) <= set(every), kw
        for key, want in alone.items():
            assert _same(every[key], want), (kw, key)
        seen |= set(alone)
    assert seen == set(every) and set(SHAPES) | set(COUNTS) <= seen
    for key, shape in SHAPES.items():
        assert tuple(every[key].shape) == shape and bool(every[key].any()), key
    assert every["resp_steps"] == every["feal_steps"] == every["resp_full_steps"] == STEPS
    assert every["feal_envs"] == E * STEPS


def test_evaluate_all_folds_equal_each_alone():
    from marlnav.actor import MultiAgentActors
    from marlnav.evaluate import evaluate
    sc = S.builtin("grid32")
    actors = MultiAgentActors(sc.K, sc.H, sc.W, "mlp", device="cuda", seed=5)
    run = lambda **kw: evaluate(actors, sc, episodes=64, max_steps=40, fear=True, seed=11, **kw)  # noqa: E731
    every = run(**ALL)
    seen = set()
    for kw, v in ALL.items():
        alone = run(**{kw: v})
        assert set(alone) <= set(every), kw
        for key, want in alone.items():
            assert _same(every[key], want), (kw, key)
        seen |= set(alone)
    assert seen == set(every)
    assert {"resp", "fear_regret", "fear_best_frac", "feal", "resp_full", "resp_full_steps", "resp_map",
            "resp_map_counts", "resp_map_visits", "resp_footprint", "resp_footprint_counts",
            "resp_footprint_visits"} <= seen
    assert every["steps"] > 0 and int(every["resp_map_visits"].sum()) == every["steps"] * sc.N


def test_shield_with_all_folds(monkeypatch):
    monkeypatch.setenv("GW_KERNEL", "defer")
    monkeypatch.delenv("GW_FEAR_BE", raising=False)
    # the trajectory depends on the shield, so both runs carry it
    every, alone = _rollout(shield=0.0, **ALL), _rollout(shield=0.0)
    assert {"shield_replaced", "shield_stuck", "env_steps"} <= set(alone) and not set(alone) & set(SHAPES)
    for key, want in alone.items():  # the shield's counts and the statistics
        assert _same(every[key], want), key
    assert int(every["shield_replaced"].sum()) > 0
    for key, shape in SHAPES.items():
        assert tuple(every[key].shape) == shape and bool(every[key].any()), key
    for key in COUNTS:
        assert every[key] > 0, key
