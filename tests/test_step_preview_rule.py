"""Step outcome preview (gw_step_preview): what can be checked without a GPU.

1. The entry point is declared in include/gridenv.h and exported by the library; GW_SPAN_STEP_PREVIEW = 14; null
   env -> GW_ERR_ARG before any device use; the kernel is a translation unit of its own that gridenv.hip does
   not name; gw_step_out did not grow.
2. The safe-mask rule (csrc/step_preview.h, the text the kernel runs) and the pick the crash-aware shield makes
   from it (csrc/fear_shield.h on a zero table, tau = 0) in the stand-alone host program
   tools/step_preview_check.cpp, built with AddressSanitizer + UBSan, on crafted inputs: a safe proposal, an unsafe
   proposal with other safe actions, every masked action crashing (falls back to the mask), mask = 0, no mask;
   then every (mask, crash9) pair of a seeded sample against the rule restated here.
3. VecGridEnv.step_preview / Rollout(shield_crash=) / evaluate(shield_crash=) / customeval.py --shield-crash exist
   and default off; shield_crash with shield_mode="joint" raises ValueError before any device use; the wrapper's
   argument checks that need no device."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from marlnav import _lib

ALL = 0x1FF


def test_entry_point_is_declared_and_exported():
    lib = C.CDLL(_lib.build())
    grid = open(os.path.join(_lib.INCLUDE, "gridenv.h")).read()
    assert re.search(r"^gw_status gw_step_preview\(void \*env, const int32_t \*rl_actions, const int32_t \*scripted, "
                     r"const uint16_t \*mask,\s+uint16_t \*outcome, double \*reward_alt, uint16_t \*crash9, "
                     r"uint16_t \*safe_mask,\s+int32_t \*actions, void \*stream\);", grid, re.M)
    assert re.search(r"GW_SPAN_STEP_PREVIEW = 14\b", grid) and re.search(r"GW_SPAN_FEAR_SHIELD = 13\b", grid)
    assert "gw_step_preview" in _lib.EXPORTS and hasattr(lib, "gw_step_preview")
    lib.gw_step_preview.argtypes = [C.c_void_p] * 10
    assert lib.gw_step_preview(*[None] * 10) == -1  # GW_ERR_ARG: null env, before any device use
    # a translation unit of its own beside fear_preview.hip; gridenv.hip only calls its launcher
    assert os.path.join(_lib.CSRC, "step_preview.hip") in _lib.HIP_SOURCES
    assert os.path.join(_lib.CSRC, "step_preview.h") in _lib.SOURCES
    src = open(os.path.join(_lib.CSRC, "gridenv.hip")).read()
    assert "launch_step_preview" in src and "step_preview_kernel" not in src
    kern = open(os.path.join(_lib.CSRC, "step_preview.hip")).read()
    assert '#include "step_preview.h"' in kern and "step_preview::safe_mask(" in kern
    assert "asm" not in kern  # plain C++ stores, no inline assembly
    assert len(_lib.STEP_OUT_FIELDS) == 25 and _lib.STEP_OUT_FIELDS[-1] == "fear_row"


def _safe_ref(has_mask, mask, crash9):
    """include/gridenv.h: m & ~crash9 (no mask: all nine); empty -> m unchanged."""
    m = (mask & ALL) if has_mask else ALL
    safe = m & ~crash9
    return safe if safe else m


def _pick_ref(p, safe, pr):
    """fear_shield.h on a zero table with tau = 0: keep p if allowed, else the most probable allowed action
    (ties to the lowest); an empty mask keeps p."""
    if safe == 0 or (0 <= p < 9 and (safe >> p) & 1):
        return p, 0
    best = -1
    for a in range(9):
        if (safe >> a) & 1 and (best < 0 or pr[a] > pr[best]):
            best = a
    return best, 1


PR = np.array([0.05, 0.30, 0.10, 0.30, 0.05, 0.05, 0.05, 0.05, 0.05], np.float32)  # tied maxima at 1 and 3

# (has_mask, mask, crash9, p) -> (safe_mask, action, flags), worked out by hand from the stated rule
CRAFTED = [
    ((1, 0x1FF, 0x002, 3), (0x1FD, 3, 0)),   # the proposal is safe: kept
    ((1, 0x1FF, 0x008, 3), (0x1F7, 1, 1)),   # the proposal crashes, others are safe: the most probable safe one
    ((1, 0x00A, 0x002, 1), (0x008, 3, 1)),   # ... within the mask: 1 crashes, 3 is the only masked safe action
    ((1, 0x00A, 0x00A, 3), (0x00A, 3, 0)),   # every masked action crashes: the mask unchanged, the proposal kept
    ((1, 0x00A, 0x1FF, 1), (0x00A, 1, 0)),   # everything crashes
    ((1, 0x000, 0x004, 2), (0x000, 2, 0)),   # mask = 0 stays 0: the shield keeps the proposal
    ((0, 0x000, 0x008, 3), (0x1F7, 1, 1)),   # no mask: all nine, whatever the mask word holds
    ((0, 0x123, 0x000, 8), (0x1FF, 8, 0)),
    ((0, 0x000, 0x1FF, 0), (0x1FF, 0, 0)),   # no mask, everything crashes: all nine
    ((1, 0xFFFF, 0x001, 0), (0x1FE, 1, 1)),  # bits above the nine are ignored
]


def test_safe_mask_rule_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "step_preview_check")
    src = os.path.join(_lib.REPO_ROOT, "tools", "step_preview_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{_lib.CSRC}", src, "-o", exe], check=True, capture_output=True, text=True)
    rng = np.random.default_rng(20261)
    cases = [c for c, _ in CRAFTED]
    for _ in range(400):
        cases.append((int(rng.integers(0, 2)), int(rng.integers(0, 0x200)), int(rng.integers(0, 0x200)),
                      int(rng.integers(0, 9))))
    for m in (0, 1, 0x100, ALL):  # the edges of both words against each other
        for c9 in (0, 1, 0x100, ALL):
            cases.append((1, m, c9, 0))
    prs = " ".join(float(x).hex() for x in PR)
    text = "".join(f"{h} {hex(m)} {hex(c9)} {p} {prs}\n" for h, m, c9, p in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert len(got) == len(cases)
    for (case, want), g in zip(CRAFTED, got):
        assert g == want, (case, g, want)
    fell_back = shrunk = 0
    for (h, m, c9, p), g in zip(cases, got):
        safe = _safe_ref(h, m, c9)
        assert g == (safe,) + _pick_ref(p, safe, PR), (h, hex(m), hex(c9), p, g)
        mm = (m & ALL) if h else ALL
        assert safe & ~mm == 0 and (safe == mm or safe & c9 == 0)  # a subset of the mask; crash-free unless it fell back
        fell_back += int(mm != 0 and mm & ~c9 == 0)
        shrunk += int(safe != mm)
    assert fell_back > 0 and shrunk > 0


def test_keywords_exist_and_default_off():
    from marlnav.evaluate import evaluate
    from marlnav.rollout import Rollout
    from marlnav.vec_env import VecGridEnv
    p = inspect.signature(VecGridEnv.step_preview).parameters
    assert list(p)[1:] == ["rl_actions", "scripted", "mask", "reward"]
    assert p["rl_actions"].default is None and p["scripted"].default is None and p["mask"].default is None
    assert p["reward"].default is True
    assert inspect.signature(Rollout.__init__).parameters["shield_crash"].default is False
    assert inspect.signature(evaluate).parameters["shield_crash"].default is False
    src = open(os.path.join(_lib.REPO_ROOT, "marl-responsible-nav_amd", "customeval.py")).read()
    assert '"--shield-crash"' in src


def test_joint_mode_is_refused_before_any_device_use():
    from marlnav.evaluate import evaluate
    from marlnav.rollout import Rollout
    with pytest.raises(ValueError, match="shield_crash"):
        evaluate(None, "level3", episodes=4, shield=0.0, shield_mode="joint", shield_crash=True)
    with pytest.raises(ValueError, match="shield_crash"):
        evaluate(None, "level3", episodes=4, shield_mode="joint", shield_crash=True)
    # Rollout.__init__ needs an env (a device); its keyword check is the static method it calls
    with pytest.raises(ValueError, match="shield_crash"):
        Rollout.check_shield_args("joint", True)
    Rollout.check_shield_args("unilateral", True)
    Rollout.check_shield_args("joint", False)
    with pytest.raises(ValueError, match="shield_mode"):
        Rollout.check_shield_args("sideways", False)


def test_wrapper_argument_checks():
    from marlnav.vec_env import VecGridEnv
    chk = VecGridEnv._check_step_preview_args
    E, K, N = 5, 2, 4
    ok_mask = torch.zeros((E, K), dtype=torch.int16)
    chk(E, K, N, None, None, None)
    chk(E, K, N, np.zeros((E, K), np.int32), np.zeros((E, N - K), np.int32), ok_mask)
    with pytest.raises(ValueError, match="rl_actions"):
        chk(E, K, N, np.zeros((E, K + 1), np.int32), None, None)
    with pytest.raises(ValueError, match="scripted"):
        chk(E, K, N, None, np.zeros((E, N), np.int32), None)
    with pytest.raises(ValueError, match="mask"):
        chk(E, K, N, None, None, torch.zeros((E, K), dtype=torch.int32))       # wrong dtype
    with pytest.raises(ValueError, match="mask"):
        chk(E, K, N, None, None, torch.zeros((E, K + 1), dtype=torch.int16))   # wrong size
    with pytest.raises(ValueError, match="mask"):
        chk(E, K, N, None, None, torch.zeros((K, E), dtype=torch.int16).t())   # not contiguous
    with pytest.raises(ValueError, match="mask"):
        chk(E, K, N, None, None, np.zeros((E, K), np.int16))                   # not a tensor
