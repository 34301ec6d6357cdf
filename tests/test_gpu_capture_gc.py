"""Graph captures keep Python's cyclic garbage collector out (marlnav/_lib.py graph_capture).

A dead Rollout <-> RolloutGraphs cycle owns HIP graphs, streams and tensors; when the collector finalises it
depends only on allocation counts, and inside a capture that is not a captured operation.  So every capture of
the package collects first and keeps the collector off until the capture ends."""
import gc
import inspect

import pytest
import torch

from marlnav import _lib, maddpg, rollout, vec_env
from marlnav.vec_env import VecGridEnv


def test_every_capture_of_the_package_goes_through_graph_capture():
    for mod in (maddpg, rollout, vec_env):
        src = inspect.getsource(mod)
        assert "torch.cuda.graph(" not in src, mod.__name__
        assert "_lib.graph_capture(" in src, mod.__name__


@pytest.mark.gpu
def test_dead_cycles_are_finalised_before_the_capture_and_none_inside():
    seen = []

    class Node:
        def __del__(self):
            seen.append(torch.cuda.is_current_stream_capturing())

    def cycle():
        a, b = Node(), Node()
        a.other, b.other = b, a

    env = VecGridEnv("grid32", num_envs=64, fear=True, seed=2)
    env.reset()
    env.step()
    torch.cuda.synchronize()
    assert gc.isenabled()
    cycle()  # dead before the capture: finalised by the collection that precedes it
    g = torch.cuda.CUDAGraph()
    with _lib.graph_capture(g):
        assert seen == [False, False]
        assert not gc.isenabled()
        cycle()  # dead inside the capture: left alone until it has ended
        junk = [[] for _ in range(5000)]  # far past the collector's threshold
        del junk
        env.step()
        assert seen == [False, False]
    assert gc.isenabled()
    gc.collect()
    assert seen == [False] * 4
    g.replay()
    torch.cuda.synchronize()
    # the collector's state is restored as found
    gc.disable()
    try:
        with _lib.graph_capture(torch.cuda.CUDAGraph()):
            env.step()
        assert not gc.isenabled()
    finally:
        gc.enable()
    env.close()
