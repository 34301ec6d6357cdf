"""Responsibility footprints (gw_resp_footprint_accum, marlnav.resp_footprint_from_counts): what needs no GPU.

1. The op is wired through every layer, and the step kernels' translation unit sees none of it.
2. The bin rule (csrc/resp_footprint.h, the text the kernel runs) in the stand-alone host program
   tools/resp_footprint_check.cpp, built with AddressSanitizer + UBSan: its own sweep (R in 1..15, cells of -1
   and HW, actions of -1, 9 and INT_MAX) against its plain restatement, and a sample of bins against the numpy
   restatement (tests/_resp_footprint_ref.py).
3. ``resp_footprint_from_counts`` on hand-made counts: equal to the plain triple loop, and within the derived
   bound n * 2^-53 * sum|x| of ``math.fsum`` over the terms the counts stand for.
4. Orientation, through the numpy restatement, on a non-square map: agent 1 two rows below and one column left
   of agent 0 lands at (+2, -1) under agent 0's action and agent 0 at (-2, +1) under agent 1's."""
import inspect
import math
import os
import shutil
import subprocess

import numpy as np
import torch

import marlnav
from marlnav import _lib

import _resp_footprint_ref as F


def test_wired_through_every_layer():
    assert os.path.join(_lib.CSRC, "resp_footprint.hip") in _lib.HIP_SOURCES
    assert os.path.join(_lib.CSRC, "resp_footprint.h") in _lib.SOURCES
    assert "gw_resp_footprint_accum" in _lib.EXPORTS
    with open(os.path.join(_lib.INCLUDE, "rollout_ops.h")) as f:
        assert "gw_status gw_resp_footprint_accum(const uint16_t *resp_valid, const int32_t *cells" in f.read()
    from marlnav.evaluate import evaluate
    from marlnav.rollout import Rollout
    from marlnav.vec_env import VecGridEnv
    assert inspect.signature(VecGridEnv.resp_footprint_accum).parameters["radius"].default == 5
    assert inspect.signature(Rollout.__init__).parameters["resp_footprint"].default is None
    assert inspect.signature(evaluate).parameters["resp_footprint"].default is None
    with open(os.path.join(_lib.PKG_ROOT, "customeval.py")) as f:
        text = f.read()
    assert '"--resp-footprint"' in text and '"--resp-footprint-file"' in text
    deps = [os.path.basename(d) for d in _lib._deps(os.path.join(_lib.CSRC, "gridenv.hip"))]
    assert "resp_footprint.h" not in deps and "rollout_ops.h" not in deps
    deps = [os.path.basename(d) for d in _lib._deps(os.path.join(_lib.CSRC, "resp_footprint.hip"))]
    assert "resp_footprint.h" in deps and "resp_map.h" in deps  # count9 is the maps'


def test_bin_rule_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "resp_footprint_check")
    src = os.path.join(_lib.REPO_ROOT, "tools", "resp_footprint_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{_lib.CSRC}", src, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(r.stdout.split()[0]) > 100000 and r.stdout.strip().endswith("bins checked")
    rng = np.random.default_rng(3)
    imax = 2 ** 31 - 1
    samples = [(0, 0, 0, 0, 1, 1, 1), (0x01FF01FF, -1, 39, -1, 3, 39, 2), (0xFFFFFFFF, 39, -1, 9, 3, 39, 15),
               (0x00550003, 0, 38, imax, 3, 39, 12), (0x01000001, 14, 19, 8, 3, 39, 2), (0x00010100, 19, 14, 4, 3, 39, 2),
               (0xFE00FE00, 1023, 0, 3, 32, 1024, 5), (0x00FF000F, 0, 1023, 5, 32, 1024, 15), (0x1, 4096, 4095, 7, 64, 4096, 15)]
    for _ in range(400):
        H, W = (int(x) for x in rng.choice([1, 2, 3, 8, 13, 32, 64], 2))
        HW = H * W
        samples.append((int(rng.integers(0, 1 << 32)), int(rng.integers(-2, HW + 2)), int(rng.integers(-2, HW + 2)),
                        int(rng.choice([-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, imax])), W, HW, int(rng.integers(1, 16))))
    r = subprocess.run([exe, "-"], input="".join(" ".join(str(v) for v in s) + "\n" for s in samples),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.array([int(x) for x in r.stdout.split()], np.int64)
    assert got.size == len(samples)
    for g, (w, ci, cj, a, W, HW, R) in zip(got, samples):
        want = int(F.bins(w & 0xFFFF, w >> 16, ci, cj, a, W, HW, R))
        assert g == want and 0 <= g < 9 * F.n_offsets(R) * 100, (w, ci, cj, a, W, HW, R, int(g), want)
    # the two orientation samples: (+1, +2) of cell 14 = (4, 2) -> 19 = (6, 1) is (dr, dc) = (+2, -1) at R = 2
    assert got[4] == ((8 * 26 + (4 * 5 + 1)) * 10 + 1) * 10 + 1 and got[5] == ((4 * 26 + (0 * 5 + 3)) * 10 + 1) * 10 + 1


def test_from_counts_against_fsum():
    rng = np.random.default_rng(7)
    R = 2
    O = F.n_offsets(R)
    counts = rng.integers(0, 6, size=(2, 9, O, 10, 10), dtype=np.int64)
    counts[rng.random(counts.shape) < 0.7] = 0
    counts[0, 0] = 0
    counts[1, 4, 3] = 0
    T = marlnav.resp_table()
    fp, pairs, (near, far) = marlnav.resp_footprint_from_counts(torch.from_numpy(counts), T)
    assert fp.dtype == torch.float64 and tuple(fp.shape) == (2, 9, O)
    assert pairs.dtype == torch.int64 and tuple(pairs.shape) == (2, 9, O)
    assert tuple(near.shape) == (2, 9, 5, 5) and tuple(far.shape) == (2, 9)
    assert torch.equal(near.reshape(2, 9, 25), fp[:, :, :25]) and torch.equal(far, fp[:, :, 25])
    worst = 0.0
    for p in range(2):
        for a in range(9):
            for o in range(O):
                acc, terms = 0.0, []
                for vm in range(10):
                    for va in range(10):
                        acc = acc + float(int(counts[p, a, o, vm, va])) * float(T[vm, va])
                        terms += [float(T[vm, va])] * int(counts[p, a, o, vm, va])
                assert float(fp[p, a, o]) == acc, (p, a, o)  # the fixed order: vm outer, va inner, from 0.0
                assert int(pairs[p, a, o]) == len(terms) == int(counts[p, a, o].sum())
                err = abs(float(fp[p, a, o]) - math.fsum(terms))
                assert err <= len(terms) * F.U * math.fsum(abs(t) for t in terms)
                worst = max(worst, err)
    print(f"from_counts vs fsum: max |err| {worst:.3e}")
    assert (fp[0, 0] == 0.0).all() and float(fp[1, 4, 3]) == 0.0 and (fp != 0).sum() > 200
    again = marlnav.resp_footprint_from_counts(counts.astype(np.uint64))[0]  # default table, numpy, unsigned
    assert torch.equal(again, fp)
    for bad in (np.zeros((2, 9, 27, 10, 10), np.int64), np.zeros((2, 9, 17, 10, 10), np.int64),
                np.zeros((2, 8, 26, 10, 10), np.int64), np.zeros((2, 9, 26, 10, 10), np.float64)):
        try:
            marlnav.resp_footprint_from_counts(bad)
        except ValueError:
            continue
        raise AssertionError(f"accepted counts of shape {bad.shape}, dtype {bad.dtype}")


def orientation_inputs(H, W, E):
    """Synthetic N = 2 inputs: agent 0 at (r, c), agent 1 at (r + 2, c - 1) (H == 1: (0, c + 2)), distinct
    actions and distinct vm / va per direction -> (sets [E, 2, 2, 2], cells [2, E], actions [E, 2], (dr, dc))."""
    dr, dc = (0, 2) if H == 1 else (2, -1)
    sets = np.zeros((E, 2, 2, 2), np.int64)
    sets[:, 0, 1] = (0x07F, 0x003)  # 0 -> 1: vm 7, va 2
    sets[:, 1, 0] = (0x1FF, 0x00F)  # 1 -> 0: vm 9, va 4
    cells = np.zeros((2, E), np.int32)
    for e in range(E):
        r, c = (0 if H == 1 else e % (H - 2)), (e % (W - 3) if H == 1 else 1 + e % (W - 1))
        cells[0, e], cells[1, e] = r * W + c, (r + dr) * W + (c + dc)
    actions = np.tile(np.array([[6, 3]], np.int32), (E, 1))
    return sets, cells, actions, (dr, dc)


def check_orientation(counts, visits, E, R, off):
    dr, dc = off
    S = 2 * R + 1
    want = np.zeros((9, F.n_offsets(R), 10, 10), np.int64)
    want[6, (dr + R) * S + (dc + R), 7, 2] = E   # pair 0 -> 1 under agent 0's action
    want[3, (-dr + R) * S + (-dc + R), 9, 4] = E  # pair 1 -> 0 under agent 1's action
    np.testing.assert_array_equal(counts[0], want)
    assert visits[6] == E and visits[3] == E and visits.sum() == 2 * E


def test_orientation_through_the_restatement():
    for H, W in ((13, 3), (1, 8)):
        E, R = 5, 2
        sets, cells, actions, off = orientation_inputs(H, W, E)
        counts, visits = F.fold(sets, cells, actions, W, H * W, R)
        check_orientation(counts, visits, E, R, off)
        assert counts[1].sum() == 0
        swapped = F.fold(sets, cells, actions, H, H * W, R)[0]  # W taken for H does not pass
        assert not np.array_equal(swapped, counts) or H == W
