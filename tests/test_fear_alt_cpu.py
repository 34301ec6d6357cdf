"""The per-action counterfactual FeAR table's ABI and keywords (no GPU needed): gw_set_fear_alt and
gw_fear_regret_accum are declared and exported, gw_step_out did NOT grow (the table's pointer lives in
the env; fear_row stays the struct's last field), and the opt-in keywords default to off."""
import ctypes as C
import dataclasses
import inspect

from marlnav import _lib


def test_entry_points_are_declared_and_exported():
    lib = C.CDLL(_lib.build())
    for name in ("gw_set_fear_alt", "gw_fear_regret_accum"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)


def test_step_out_did_not_grow():
    assert _lib.STEP_OUT_FIELDS[-1] == "fear_row"
    assert "fear_alt" not in _lib.STEP_OUT_FIELDS
    assert len(_lib.STEP_OUT_FIELDS) == 25
    assert C.sizeof(_lib.GwStepOut) == 25 * C.sizeof(C.c_void_p)


def test_keywords_exist_and_default_off():
    from marlnav.evaluate import evaluate
    from marlnav.rollout import Rollout
    from marlnav.vec_env import StepResult, VecGridEnv
    assert inspect.signature(VecGridEnv.__init__).parameters["fear_alt"].default is False
    assert inspect.signature(Rollout.__init__).parameters["fear_regret"].default is False
    assert inspect.signature(evaluate).parameters["fear_regret"].default is False
    f = {x.name: x for x in dataclasses.fields(StepResult)}
    assert f["fear_alt"].default is None


def test_task_arithmetic_under_sanitizers(tmp_path):
    """The kernel's pure index functions (csrc/fear_alt_tasks.h) in a stand-alone host program built
    with AddressSanitizer + UBSan (tools/fear_alt_tasks_check.cpp): every (N, K, close set, task)."""
    import os
    import shutil
    import subprocess
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fear_alt_tasks_check")
    src = os.path.join(_lib.REPO_ROOT, "tools", "fear_alt_tasks_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{_lib.CSRC}", src, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "task arithmetic ok" in r.stdout
