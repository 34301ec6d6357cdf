"""The profiling spans the fused actors record (gw_profile / gw_profile_spans): the counterpart of
test_gpu_profile_spans.py for the ops that take an env handle (csrc/actor_ops.hip).

Which launches an act makes, in which order and under which GW_SPAN_* kind is result-neutral, so the
actor parity tests cannot see it; this pins the sequence of span kinds per entry point.  Every case
runs 64 envs of grid32 (N = 4) or grid64_n8 (N = 8); profiling is switched on after a reset, one step
and the workspace's derivation (the prepare entries open no span), then one call of the entry point
is made through the wrappers of marlnav/actor.py.  GW_WCNN_LIST (the window CNN head's A/B listing
chain) is read once per process and is left alone: the default, fused listing is what is pinned."""
import pytest
import torch

from marlnav.actor import MultiAgentActors
from marlnav.vec_env import VecGridEnv

pytestmark = pytest.mark.gpu

E = 64
ACT, CNN_L1, CNN_LIST, CNN_RARE, WINDOW = 3, 4, 5, 6, 7  # GW_SPAN_* (include/gridenv.h)

# case -> (actor arch, window side P; 0 = the whole grid)
CASES = {
    "actor_act": ("mlp", 0),              # gw_actor_act
    "patch_actor_act": ("mlp", 5),        # gw_patch_actor_act
    "cnn_act": ("cnn", 0),                # gw_cnn_act
    "patch_cnn_act": ("cnn", 8),          # gw_patch_cnn_act
    "patch_cnn_act_listed": ("cnn", 8),   # gw_patch_cnn_write_list, then gw_patch_cnn_act_listed
}

# Recorded with collect() below against the library of the commit BEFORE actor_ops.hip's host launch
# layer was collapsed (that commit's libgridenv.so, on an MI355X), never against the refactored code:
# the refactor has to reproduce them.  Both scenarios gave the same sequences.  The listed case is
# (after gw_patch_cnn_write_list, after gw_patch_cnn_act_listed as well).
EXPECTED = {
    "actor_act": [ACT],
    "patch_actor_act": [ACT],
    "cnn_act": [CNN_L1, CNN_LIST, CNN_RARE, ACT],
    "patch_cnn_act": [CNN_L1, CNN_RARE, ACT],
    "patch_cnn_act_listed": ([WINDOW], [WINDOW, CNN_RARE, ACT]),
}


def collect(case, scenario):
    """The span kinds of the case's call(s), in the order gw_profile_spans lists them."""
    arch, P = CASES[case]
    env = VecGridEnv(scenario, num_envs=E, fear=False, seed=3, obs=False)
    try:
        actors = MultiAgentActors(env.K, P or env.H, P or env.W, arch, device=env.device, seed=1)
        assert actors.fusable(env, P)
        env.reset()
        env.step()
        actors.ensure_workspace(env, P)
        env.profile(True)

        def kinds():
            torch.cuda.synchronize()
            return [int(k) for k in env.profile_spans()[:, 0]]

        if case != "patch_cnn_act_listed":
            actors.act_env(env, env.out["mask"], True, seed=2, counter=0, patch=P)
            return kinds()
        win = torch.empty((env.K, E, P, P), dtype=torch.float32, device=env.device)
        assert actors.patch_cnn_write_list(env, P, win, None)
        listed = kinds()
        actors.act_env(env, env.out["mask"], True, seed=2, counter=0, patch=P, listed=True)
        return listed, kinds()
    finally:
        env.close()


@pytest.mark.parametrize("scenario", ["grid32", "grid64_n8"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_span_kinds_per_entry(case, scenario):
    got = collect(case, scenario)
    print(case, scenario, got)
    assert got == EXPECTED[case]
