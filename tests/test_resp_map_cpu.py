"""Responsibility maps (gw_resp_map_accum, marlnav.resp_map_from_counts): what needs no GPU.

1. The op is wired through every layer: its own translation unit in the build, the export, the declared
   contract, VecGridEnv.resp_map_accum / copy_pos, Rollout(resp_map=), evaluate(resp_map=), customeval.py
   --resp-map; the order in which the op reads the two sets is the order fear_full_kernel stores them.
2. ``resp_map_from_counts`` against a plain Python triple loop (vm outer, va inner, from 0.0), counts up to
   about 2^40: exactly equal in f64.  The table equals csrc/resp_tables.h's rule.
3. The per-cell sums of a synthetic step equal the step's resp_full entries binned by cell within the derived
   bound n * 2^-53 * sum|x| (tests/_resp_map_ref.py: why that bound holds).
4. The bin rule (csrc/resp_map.h, the text the kernel runs) in the stand-alone host program
   tools/resp_map_check.cpp, built with AddressSanitizer + UBSan: every set_mdr in 0..0xFFFF against a sample
   of (set_act, cell_i, cell_j, HW) with out-of-range cells, against the numpy restatement."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import torch

import marlnav
from marlnav import _lib

import _resp_map_ref as R


def test_wired_through_every_layer():
    assert os.path.join(_lib.CSRC, "resp_map.hip") in _lib.HIP_SOURCES
    assert os.path.join(_lib.CSRC, "resp_map.h") in _lib.SOURCES
    assert "gw_resp_map_accum" in _lib.EXPORTS
    with open(os.path.join(_lib.INCLUDE, "rollout_ops.h")) as f:
        assert re.search(r"gw_status\s+gw_resp_map_accum\(const uint16_t \*resp_valid, const int32_t \*cells", f.read())
    from marlnav.evaluate import evaluate
    from marlnav.rollout import Rollout
    from marlnav.vec_env import VecGridEnv
    assert callable(VecGridEnv.resp_map_accum) and callable(VecGridEnv.copy_pos)
    assert inspect.signature(Rollout.__init__).parameters["resp_map"].default is False
    assert inspect.signature(evaluate).parameters["resp_map"].default is False
    with open(os.path.join(_lib.PKG_ROOT, "customeval.py")) as f:
        assert '"--resp-map"' in f.read()
    # fear_full_kernel stores [0] (actor on its MdR) in the low half and [1] (actual) in the high half of one
    # word; the bin rule reads vm from the low half and va from the high half
    with open(os.path.join(_lib.CSRC, "fear_full.hip")) as f:
        assert "vm_set | (va_set << 16)" in f.read()
    with open(os.path.join(_lib.CSRC, "resp_map.h")) as f:
        assert "vm = count9(word), va = count9(word >> 16)" in f.read()
    # the step kernels' translation unit sees neither the new header nor the one the op is declared in
    deps = [os.path.basename(d) for d in _lib._deps(os.path.join(_lib.CSRC, "gridenv.hip"))]
    assert "resp_map.h" not in deps and "rollout_ops.h" not in deps


def test_table_is_the_host_rule():
    T = marlnav.resp_table()
    assert T.shape == (10, 10) and T.dtype == np.float64
    for vm in range(10):
        for va in range(10):
            want = min(1.0, max(-1.0, (float(vm) - float(va)) / (float(vm) + 0.000001)))
            assert T[vm, va] == want, (vm, va)
        assert T[vm, vm] == 0.0 and not np.signbit(T[vm, vm])
    assert (T[0, 1:] == -1.0).all() and T[9, 0] < 1.0 and T[1, 9] == -1.0


def test_from_counts_equals_the_triple_loop():
    rng = np.random.default_rng(7)
    HW = 7
    counts = rng.integers(0, 50, size=(2, HW, 10, 10), dtype=np.int64)
    big = rng.random((2, HW, 10, 10)) < 0.3
    counts[big] = (1 << 40) - rng.integers(0, 1 << 20, size=int(big.sum()))
    counts[0, 0] = 0
    counts[1, 3] = (1 << 40) + rng.integers(0, 1 << 12, size=(10, 10))
    T = marlnav.resp_table()
    got, pairs = marlnav.resp_map_from_counts(torch.from_numpy(counts), T)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, HW)
    assert pairs.dtype == torch.int64 and tuple(pairs.shape) == (2, HW)
    for p in range(2):
        for c in range(HW):
            acc = 0.0
            for vm in range(10):
                for va in range(10):
                    acc = acc + float(int(counts[p, c, vm, va])) * float(T[vm, va])
            assert float(got[p, c]) == acc, (p, c, float(got[p, c]), acc)
            assert int(pairs[p, c]) == int(counts[p, c].sum())
    assert float(got[0, 0]) == 0.0 and (got != 0).sum() >= 2 * HW - 2
    # the default table, numpy input, unsigned counts
    again, _ = marlnav.resp_map_from_counts(counts.astype(np.uint64))
    assert torch.equal(again, got)


def test_cell_sums_of_a_synthetic_step():
    rng = np.random.default_rng(11)
    E, N, HW = 300, 4, 9  # ~ 400 terms per cell and plane
    T = marlnav.resp_table()
    sets = rng.integers(0, 512, size=(E, N, N, 2))
    sets[:, np.arange(N), np.arange(N)] = 0
    cells = rng.integers(0, HW - 1, size=(N, E)).astype(np.int32)  # the last cell stays empty
    resp = T[R.popcount9(sets[..., 0]), R.popcount9(sets[..., 1])]
    resp[:, np.arange(N), np.arange(N)] = 0.0
    counts, visits = R.fold(sets, cells, HW)
    assert counts.sum() == 2 * E * N * (N - 1) and visits.sum() == E * N
    got, pairs = marlnav.resp_map_from_counts(counts, T)
    exact, mag, n, _ = R.bin_resp([(resp, cells, None)], HW)
    np.testing.assert_array_equal(pairs.numpy(), n)
    err, bound = np.abs(got.numpy() - exact), n * R.U * mag
    print(f"synthetic step: terms per cell {n.min()}..{n.max()}, max |err| {err.max():.3e}, "
          f"bound min (non-empty) {bound[n > 0].min():.3e}")
    assert (err <= bound).all()
    assert (n[:, HW - 1] == 0).all() and (got.numpy()[:, HW - 1] == 0.0).all() and (mag[:, :HW - 1] > 0).all()


def test_bin_rule_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "resp_map_check")
    src = os.path.join(_lib.REPO_ROOT, "tools", "resp_map_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{_lib.CSRC}", src, "-o", exe], check=True, capture_output=True, text=True)
    rng = np.random.default_rng(3)
    imin, imax = -2 ** 31, 2 ** 31 - 1
    samples = [(0, 0, 0, 1), (0x1FF, -1, 1, 1), (0xFFFF, -1, 4, 4), (0xFE00, 4, -1, 4), (0x0155, 3, 0, 4),
               (0x01FF, 1024, -1, 1024), (0x8001, 1023, 1024, 1024), (0x0200, imin, imax, 1024),
               (0x00FF, imax, imin, 4096), (0x1FF, 4095, 4096, 4096), (0x0F0F, 4096, 4095, 4096),
               (0, -1, 63, 63), (0x1FE, 63, 62, 63)]
    for _ in range(11):
        HW = int(rng.choice([1, 4, 63, 1024, 4096]))
        samples.append((int(rng.integers(0, 1 << 16)), int(rng.integers(-3, HW + 3)), int(rng.integers(-3, HW + 3)), HW))
    r = subprocess.run([exe], input="".join(f"{a:#x} {ci} {cj} {hw}\n" for a, ci, cj, hw in samples).encode(),
                       capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    got = np.frombuffer(r.stdout, dtype=np.int64).reshape(len(samples), 65536, 2)
    set_mdr = np.arange(65536)
    for s, (a, ci, cj, hw) in enumerate(samples):
        ca, re_ = R.bins(set_mdr, np.full(65536, a), np.full(65536, ci), np.full(65536, cj), hw)
        np.testing.assert_array_equal(got[s, :, 0], ca, err_msg=str(samples[s]))
        np.testing.assert_array_equal(got[s, :, 1], re_, err_msg=str(samples[s]))
        assert got[s].min() >= 0 and got[s].max() < 2 * hw * 100
        assert (got[s, :, 0] < hw * 100).all() and (got[s, :, 1] >= hw * 100).all()  # each in its own plane
