"""Per-agent FeAL from the step: what can be checked without a GPU.

1. The host table the kernel looks FeAL up in (csrc/resp_tables.h, uploaded by gw_create) equals
   numpy's np.clip(va / (vm + 1e-6), -1, 1) entry by entry, bit for bit (and the Resp half of the same
   table its own formula): a stand-alone host program prints it (tools/feal_table_check.cpp).
2. gw_set_feal and gw_feal_accum are declared in the headers and exported by the library.
3. VecGridEnv, Rollout, evaluate and the facade accept feal=, default off."""
import ctypes as C
import dataclasses
import inspect
import os
import re
import shutil
import subprocess

import numpy as np

from marlnav import _lib


def test_host_table_equals_numpy(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "feal_table_check")
    src = os.path.join(_lib.REPO_ROOT, "tools", "feal_table_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O2", f"-I{_lib.CSRC}", src, "-o", exe], check=True, capture_output=True,
                   text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {"resp": np.full((10, 10), np.nan), "feal": np.full((10, 10), np.nan)}
    for line in r.stdout.splitlines():
        name, vm, va, val = line.split()
        got[name][int(vm), int(va)] = float.fromhex(val)
    vm = np.arange(10, dtype=np.float64)[:, None]
    va = np.arange(10, dtype=np.float64)[None, :]
    want_feal = np.clip(va / (vm + 1e-6), -1, 1)
    want_resp = np.clip((vm - va) / (vm + 1e-6), -1, 1)
    for i in range(10):
        for j in range(10):
            assert got["feal"][i, j] == want_feal[i, j], (i, j, got["feal"][i, j], want_feal[i, j])
            assert got["resp"][i, j] == want_resp[i, j], (i, j)
    assert got["feal"][0, 0] == 0.0 and got["feal"][0, 1] == 1.0 and got["feal"][9, 9] < 1.0


def test_entry_points_are_declared_and_exported():
    lib = C.CDLL(_lib.build())
    text = {h: open(os.path.join(_lib.INCLUDE, h)).read() for h in ("gridenv.h", "rollout_ops.h")}
    assert re.search(r"^gw_status gw_set_feal\(void \*env, double \*feal, uint16_t \*feal_valid\);", text["gridenv.h"],
                     re.M)
    assert re.search(r"^gw_status gw_feal_accum\(", text["rollout_ops.h"], re.M)
    assert re.search(r"GW_SPAN_FEAL = 10\b", text["gridenv.h"])
    for name in ("gw_set_feal", "gw_feal_accum"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert "feal" not in _lib.STEP_OUT_FIELDS and "feal_valid" not in _lib.STEP_OUT_FIELDS  # kept in the env


def test_keywords_exist_and_default_off():
    from custom.ma_customenv import CustomMAEnv
    from marlnav.evaluate import evaluate
    from marlnav.rollout import Rollout
    from marlnav.vec_env import StepResult, VecGridEnv
    for f in (VecGridEnv.__init__, Rollout.__init__, evaluate, CustomMAEnv.__init__):
        assert inspect.signature(f).parameters["feal"].default is False, f
    fields = {x.name: x for x in dataclasses.fields(StepResult)}
    assert fields["feal"].default is None and fields["feal_valid"].default is None
