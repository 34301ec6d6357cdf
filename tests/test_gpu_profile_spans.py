"""The profiling spans gw_step records on each of its host paths (gw_profile / gw_profile_spans).

Which launches a step makes, in which order and under which GW_SPAN_* kind is result-neutral, so the
parity tests cannot see it; this pins the sequence of span kinds per path.  Every case runs grid32
with 64 envs, the fear_alt table armed and profiling on, for three steps after a reset (and a
gw_obs_fence where the case pipelines the obs writer).  The spans of a step's streams are appended in
the order the host issues their launches, so the sequences are deterministic."""
import pytest
import torch

from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu

E, STEPS, WINDOW = 64, 3, 5
STEP, OBS, FEAR, FEAR_ALT = 0, 1, 2, 9  # GW_SPAN_* (include/gridenv.h)

# case -> (environment, FeAR on, obs outputs, obs pipelining: None / "eager" / "lazy", window request)
CASES = {
    "defer_sync": ({"GW_KERNEL": "defer"}, True, True, None, False),
    "defer_rows": ({"GW_KERNEL": "defer"}, True, False, None, True),  # P = 5: the FeAR + rows launch
    "defer_async_eager": ({"GW_KERNEL": "defer"}, True, True, "eager", False),
    "defer_async_lazy": ({"GW_KERNEL": "defer"}, True, True, "lazy", False),
    "merged_async": ({"GW_KERNEL": "merged"}, True, True, "eager", False),
    "defer_nofear": ({"GW_KERNEL": "defer"}, False, True, None, False),
    "merged_nofear": ({"GW_KERNEL": "merged"}, False, True, None, False),
    "defer_async_chunks2": ({"GW_KERNEL": "defer", "GW_OBS_CHUNKS": "2"}, True, True, "eager", False),
}

# Recorded with collect() below against the library of the commit BEFORE the host launch layer was
# collapsed (that commit's libgridenv.so, on an MI355X), never against the refactored code: the
# refactor has to reproduce them.  Repeated collections gave the same sequences.
EXPECTED = {
    "defer_sync": [STEP, FEAR, FEAR_ALT, OBS] * 3,
    "defer_rows": [STEP, FEAR, FEAR_ALT] * 3,
    "defer_async_eager": [STEP, FEAR, FEAR_ALT, OBS] * 3,
    "defer_async_lazy": [STEP, FEAR, FEAR_ALT] + [OBS, STEP, FEAR, FEAR_ALT] * 2 + [OBS],
    "merged_async": [STEP, FEAR_ALT] + [OBS, FEAR_ALT] * 2 + [OBS],
    "defer_nofear": [STEP, OBS] * 3,
    "merged_nofear": [STEP, OBS] * 3,
    "defer_async_chunks2": [STEP, FEAR, FEAR_ALT, OBS, OBS] * 3,
}


def collect(case, monkeypatch):
    """The span kinds of the case's three steps, in the order gw_profile_spans lists them."""
    environ, fear, obs, pipeline, window = CASES[case]
    for name in ("GW_KERNEL", "GW_OBS_CHUNKS", "GW_OBS_STREAMS", "GW_FEAR_BE", "GW_MERGE_BYTES"):
        monkeypatch.delenv(name, raising=False)
    for name, value in environ.items():
        monkeypatch.setenv(name, value)
    env = VecGridEnv("grid32", num_envs=E, fear=fear, seed=3, obs=obs, fear_alt=True)
    try:
        assert env.kernel_path == environ["GW_KERNEL"]
        if pipeline:
            env.set_obs_async("lazy" if pipeline == "lazy" else True)
        env.reset()
        env.profile(True)
        win = torch.empty((env.K, E, WINDOW, WINDOW), dtype=torch.float32, device=env.device) if window else None
        for _ in range(STEPS):
            if window:
                env.patch_next(WINDOW, win)
            env.step()
        env.obs_fence()
        torch.cuda.synchronize()
        return [int(k) for k in env.profile_spans()[:, 0]]
    finally:
        env.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_span_kinds_per_path(case, monkeypatch):
    kinds = collect(case, monkeypatch)
    print(case, kinds)
    assert kinds == EXPECTED[case]
