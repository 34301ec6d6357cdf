"""FeAR preview and the responsibility shield: what can be checked without a GPU.

1. gw_fear_preview / gw_fear_shield are declared in the headers and exported by the library;
   GW_SPAN_FEAR_PREVIEW = 12; gw_step_out did not grow (25 fields, fear_row last).
2. VecGridEnv.fear_preview / fear_shield exist; Rollout / evaluate accept shield=, default None (off);
   customeval.py has --shield.
3. The shield's selection rule (csrc/fear_shield.h, the text the kernel runs) in the stand-alone host program
   tools/fear_shield_check.cpp, built with AddressSanitizer + UBSan, against the numpy restatement of the rule
   (tests/_fear_shield_ref.py): every proposed action, masks 0 / full / MdR forbidden / partial, rows with exact
   ties, rows with an entry exactly equal to tau, tau in {-0.5, 0.0, 0.5, 8.0}, with and without probabilities
   (tied ones included), shielded or not."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np

from _fear_shield_ref import pick_one
from marlnav import _lib


def test_entry_points_are_declared_and_exported():
    lib = C.CDLL(_lib.build())
    grid = open(os.path.join(_lib.INCLUDE, "gridenv.h")).read()
    roll = open(os.path.join(_lib.INCLUDE, "rollout_ops.h")).read()
    assert re.search(r"^gw_status gw_fear_preview\(void \*env, const int32_t \*rl_actions, const int32_t \*scripted,"
                     r"\s+double \*fear_alt,\s+int32_t \*actions, int32_t \*mdr, void \*stream\);", grid, re.M)
    assert re.search(r"^gw_status gw_fear_shield\(const double \*fear_alt, const int32_t \*actions_in, "
                     r"const uint16_t \*mask,\s+const float \*probs, int64_t E, int32_t K, double tau, "
                     r"uint32_t agents,\s+int32_t \*actions_out, uint8_t \*flags, void \*stream\);", roll, re.M)
    assert re.search(r"GW_SPAN_FEAR_PREVIEW = 12\b", grid)
    for name in ("gw_fear_preview", "gw_fear_shield"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    # argument checks come before any device use
    lib.gw_fear_preview.argtypes = [C.c_void_p] * 7
    assert lib.gw_fear_preview(None, None, None, None, None, None, None) == -1  # GW_ERR_ARG: null env
    # the record builder is a translation unit of its own; draw_action lives in a header both units include
    assert os.path.join(_lib.CSRC, "fear_preview.hip") in _lib.HIP_SOURCES
    src = open(os.path.join(_lib.CSRC, "gridenv.hip")).read()
    assert '#include "draw_action.h"' in src and "preview_rec_kernel" not in src
    assert "int draw_action(" in open(os.path.join(_lib.CSRC, "draw_action.h")).read()


def test_step_out_did_not_grow():
    assert len(_lib.STEP_OUT_FIELDS) == 25 and _lib.STEP_OUT_FIELDS[-1] == "fear_row"
    assert C.sizeof(_lib.GwStepOut) == 25 * C.sizeof(C.c_void_p)


def test_keywords_exist_and_default_off():
    from marlnav.evaluate import evaluate
    from marlnav.rollout import Rollout
    from marlnav.vec_env import VecGridEnv
    p = inspect.signature(VecGridEnv.fear_preview).parameters
    assert p["rl_actions"].default is None and p["scripted"].default is None
    assert p["actions"].default is None and p["mdr"].default is None
    p = inspect.signature(VecGridEnv.fear_shield).parameters
    assert list(p)[1:3] == ["table", "actions"]
    assert p["mask"].default is None and p["probs"].default is None and p["agents"].default is None
    assert p["tau"].default == 0.0
    assert inspect.signature(Rollout.__init__).parameters["shield"].default is None
    assert inspect.signature(evaluate).parameters["shield"].default is None
    src = open(os.path.join(_lib.REPO_ROOT, "marl-responsible-nav_amd", "customeval.py")).read()
    assert '"--shield"' in src


VALUES = (-1.0, -0.5, 0.0, 0.5, 1.0, 2.0)
TAUS = (-0.5, 0.0, 0.5, 8.0)


def _cases():
    """(p, mask, shielded, tau, t [9] f64, pr [9] f32 or None)"""
    rng = np.random.default_rng(20260)
    rows = [np.zeros(9), np.full(9, 0.5), np.full(9, 2.0),              # every entry tied
            np.array([1.0, 0.5, 0.5, 2.0, 0.5, 1.0, 0.0, 0.0, 2.0]),   # ties at the minimum and at tau = 0.5
            np.array([2.0, 1.0, 1.0, 2.0, 1.0, 1.0, 2.0, 1.0, 2.0]),   # nothing <= 0.5: stuck unless tau = 8
            np.array([0.5, 1.0, -0.5, -1.0, -0.5, 2.0, 0.0, -1.0, 1.0])]
    rows += [rng.choice(VALUES, 9) for _ in range(6)]
    probs = [None, np.full(9, 1.0 / 9.0, np.float32),                    # all tied
             np.array([0.1, 0.2, 0.2, 0.05, 0.2, 0.05, 0.1, 0.05, 0.05], np.float32),  # tied maxima
             rng.random(9).astype(np.float32)]
    cases = []
    for ti, t in enumerate(rows):
        mdr = int(np.argmin(t))  # the row's least entry stands in for the MdR
        masks = [0, 0x1FF, 0x1FF & ~(1 << mdr), int(rng.integers(1, 0x200)), 1 << int(rng.integers(0, 9))]
        for m in masks:
            for tau in TAUS:
                for pr in probs:
                    for p in range(9):
                        cases.append((p, m, 1, tau, t, pr))
        cases.append((ti % 9, 0x1FF, 0, 0.0, t, None))  # not shielded: kept
    return cases


def test_selection_rule_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fear_shield_check")
    src = os.path.join(_lib.REPO_ROOT, "tools", "fear_shield_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{_lib.CSRC}", src, "-o", exe], check=True, capture_output=True, text=True)
    cases = _cases()
    lines = []
    for p, m, sh, tau, t, pr in cases:
        f = [str(p), hex(m), str(sh), float(tau).hex(), "1" if pr is not None else "0"]
        f += [float(x).hex() for x in t]
        if pr is not None:
            f += [float(x).hex() for x in pr]  # a float32 value is exact as a double's hex
        lines.append(" ".join(f))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert len(got) == len(cases)
    seen = set()
    for (p, m, sh, tau, t, pr), g in zip(cases, got):
        want = pick_one(t, p, m, pr, tau, sh)
        assert g == want, (p, hex(m), sh, tau, t.tolist(), None if pr is None else pr.tolist(), g, want)
        seen.add(want[1])
        if want[1] in (0, 1) and sh and m:  # an allowed pick is masked and within tau
            if want[1] == 1:
                assert (m >> want[0]) & 1 and t[want[0]] <= tau and want[0] != p
    assert seen == {0, 1, 2, 3}  # every outcome occurs in the case set
