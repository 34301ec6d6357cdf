"""Two-step crash lookahead (gw_step_lookahead): what can be checked without a GPU.

1. The reference alone (tests/_step_lookahead_ref.py: the C oracle stepped twice per (e, k, a, b)), so that the
   cases tests/test_gpu_step_lookahead.py compares are proven to reach every kind of entry before any GPU run.
   Each case's oracle tables must show a non-zero crash2 entry that is no trap and an ends bit for an action
   under which k itself does not crash; each case WITH scripted agents (N > K) a trap bit and an
   ahead_mask != safe_mask.  Over the whole run: an end by all-eaten, an end by the step cap with all nine bits
   set, an end by another RL agent's crash.
   Two conditions follow from the world update and are asserted as what they are:
   - Action 0 (stay) is in every cell's mask, so a trap needs `stay` to crash k in the second step, and with every
     other RL agent staying only a scripted agent can do that: a case with N == K has no trap and
     ahead_mask == safe_mask everywhere (asserted: trap9 == 0 there).
   - An agent changes another agent's final cell only through a collision, a collision marks both agents crashed,
     and an RL agent's crash ends the episode in both variants.  So among the first actions a of one (e, k) whose
     step goes on, the worlds differ in k's own cell only, and the scripted agents' second-step actions (drawn
     from their own cells) are the same for every such a.  The coverage condition "a (k, a) whose stage-2 scripted
     joint action differs from another a's" can therefore not hold in any case; the reference records those
     actions and the test asserts that they never differ.
2. The trap and mask rules (csrc/step_lookahead.h, the text the kernel runs) in the stand-alone host program
   tools/step_lookahead_check.cpp under AddressSanitizer + UBSan (its own main, no LD_PRELOAD).
3. Declaration and wiring: entry point, span kind 16, null env -> GW_ERR_ARG before any device use, the keywords
   exist and default off, ValueError with the joint modes before any device use."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _step_lookahead_ref as R
from marlnav import _lib


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_the_cases_reach_every_kind_of_entry(name):
    run = R.reference_run(name)
    sc = R.scenario_of(run["case"])
    cov = R.summed_coverage(name)
    print(f"{name}: oracle coverage {cov}")
    assert len(run["comps"]) == len(R.COMPARE_AT) + R.REPLAY_ROUNDS
    assert cov["crash2_no_trap"] > 0 and cov["ends_not_own"] > 0, cov
    assert cov["scripted2_differs"] == 0, cov  # (the docstring's second point)
    if sc.N > sc.K:
        assert cov["trap"] > 0 and cov["ahead_differs"] > 0, cov
    else:
        assert cov["trap"] == 0 and cov["ahead_differs"] == 0, cov
    for c in run["comps"]:  # the tables are consistent with their own rules
        tab = c["tab"]
        trap9, safe, ahead, sims = R.derived(tab, c["mask"])
        K = sc.K
        ends_bits = (tab["ends"][:, :, None] >> np.arange(9)) & 1
        assert not (tab["crash2"][ends_bits == 1] != 0).any()  # no second step where the first ends
        assert ((trap9 & tab["ends"]) == 0).all() and ((ahead & ~(c["mask"].astype(np.int64))) == 0).all()
        assert sims == 9 * K * run["case"].E + 9 * int((ends_bits == 0).sum())
        if run["case"].variant == 0:  # the own crash ends the episode: crash9 is a subset of ends
            assert ((tab["crash9"] & ~tab["ends"]) == 0).all()


def test_the_whole_run_ends_in_every_way():
    total = {}
    for name in R.CASE_IDS:
        for n, v in R.summed_coverage(name).items():
            total[n] = total.get(n, 0) + v
    print(f"all cases: {total}")
    assert total["end_eaten"] > 0 and total["end_cap"] > 0 and total["cap_all_nine"] > 0 and total["end_other"] > 0


def test_rules_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "step_lookahead_check")
    src = os.path.join(_lib.REPO_ROOT, "tools", "step_lookahead_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{_lib.CSRC}", src, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    m = re.match(r"(\d+) cases, (\d+) traps, (\d+) fall-backs, (\d+) masks shrunk", r.stdout)
    assert m and int(m.group(1)) == 9 * 2 * 512 * 512 + 11 * 512 * 512 and int(m.group(2)) > 0


def test_entry_point_is_declared_and_exported():
    lib = C.CDLL(_lib.build())
    grid = open(os.path.join(_lib.INCLUDE, "gridenv.h")).read()
    assert re.search(r"^gw_status gw_step_lookahead\(void \*env, const int32_t \*rl_actions, const int32_t \*scripted, "
                     r"const uint16_t \*mask,\s+uint16_t \*crash2, uint16_t \*ends, uint16_t \*crash9, "
                     r"uint16_t \*trap9, uint16_t \*ahead_mask,\s+int32_t \*actions, int32_t \*mdr, void \*stream\);",
                     grid, re.M)
    assert re.search(r"GW_SPAN_STEP_LOOKAHEAD = 16\b", grid) and re.search(r"GW_SPAN_CRASH_SHIELD = 15\b", grid)
    assert "gw_step_lookahead" in _lib.EXPORTS and hasattr(lib, "gw_step_lookahead")
    lib.gw_step_lookahead.argtypes = [C.c_void_p] * 12
    assert lib.gw_step_lookahead(*[None] * 12) == -1  # GW_ERR_ARG: null env, before any device use
    # a translation unit of its own; gridenv.hip only calls its launcher
    assert os.path.join(_lib.CSRC, "step_lookahead.hip") in _lib.HIP_SOURCES
    assert os.path.join(_lib.CSRC, "step_lookahead.h") in _lib.SOURCES
    src = open(os.path.join(_lib.CSRC, "gridenv.hip")).read()
    assert "launch_step_lookahead" in src and "step_lookahead_kernel" not in src
    kern = open(os.path.join(_lib.CSRC, "step_lookahead.hip")).read()
    assert '#include "step_lookahead.h"' in kern and "step_lookahead::rules(" in kern
    assert "asm" not in kern  # plain C++ stores, no inline assembly


def test_keywords_exist_default_off_and_refuse_the_joint_modes():
    from marlnav.evaluate import evaluate
    from marlnav.rollout import Rollout
    from marlnav.vec_env import VecGridEnv
    p = inspect.signature(VecGridEnv.step_lookahead).parameters
    assert list(p)[1:] == ["rl_actions", "scripted", "mask"] and all(p[n].default is None for n in list(p)[1:])
    assert inspect.signature(Rollout.__init__).parameters["shield_lookahead"].default is False
    assert inspect.signature(evaluate).parameters["shield_lookahead"].default is False
    src = open(os.path.join(_lib.REPO_ROOT, "marl-responsible-nav_amd", "customeval.py")).read()
    assert '"--shield-lookahead"' in src
    for mode in ("joint", "joint_crash"):
        with pytest.raises(ValueError, match="shield_lookahead"):
            evaluate(None, "level3", episodes=4, shield_mode=mode, shield_lookahead=True)
        with pytest.raises(ValueError, match="shield_lookahead"):
            Rollout.check_shield_args(mode, False, "Rollout", True)
    Rollout.check_shield_args("unilateral", False, "Rollout", True)
