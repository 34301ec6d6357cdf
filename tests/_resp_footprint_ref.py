"""numpy restatement of gw_resp_footprint_accum, written from the op's contract (include/rollout_ops.h), and of
the per-(action, offset) sums its counts stand for; shared by tests/test_resp_footprint_cpu.py and
tests/test_gpu_resp_footprint.py.  The bound on the derived sums is the one derived in tests/_resp_map_ref.py:
|footprint - fsum| <= n * 2^-53 * sum|x| per bin of n terms x."""
import math

import numpy as np

from _resp_map_ref import U, popcount9  # noqa: F401  (U: re-exported for the tests)

NV, NA = 10, 9


def n_offsets(R):
    return (2 * R + 1) ** 2 + 1


def offset_bins(cell_i, cell_j, W, HW, R):
    """The offset bin of the affected agent's cell as seen from the actor's: near bins row-major, far last."""
    ci = np.clip(np.asarray(cell_i, np.int64), 0, HW - 1)
    cj = np.clip(np.asarray(cell_j, np.int64), 0, HW - 1)
    dr, dc = cj // W - ci // W, cj % W - ci % W
    near = (np.abs(dr) <= R) & (np.abs(dc) <= R)
    return np.where(near, (dr + R) * (2 * R + 1) + (dc + R), (2 * R + 1) ** 2)


def act9(a):
    a = np.asarray(a, np.int64)
    return np.where((a < 0) | (a > 8), 0, a)


def bins(set_mdr, set_act, cell_i, cell_j, a_i, W, HW, R):
    """-> flat int64 indices into one plane [9][O][10][10]."""
    vm, va = popcount9(set_mdr), popcount9(set_act)
    return ((act9(a_i) * n_offsets(R) + offset_bins(cell_i, cell_j, W, HW, R)) * NV + vm) * NV + va


def fold(resp_valid, cells, actions, W, HW, R, crash_bits=None, active=None):
    """One step: resp_valid [E, N, N, 2] (non-negative ints), cells [N, E], actions [E, N], crash_bits [E] or
    None, active [E] bool or None -> (counts [2, 9, O, 10, 10] int64, visits [9] int64)."""
    E, N = resp_valid.shape[:2]
    O = n_offsets(R)
    plane = NA * O * NV * NV
    counts, visits = np.zeros(2 * plane, np.int64), np.zeros(NA, np.int64)
    on = np.ones(E, bool) if active is None else np.asarray(active, bool)
    for i in range(N):
        np.add.at(visits, act9(actions[on, i]), 1)
        for j in range(N):
            if i == j:
                continue
            b = bins(resp_valid[on, i, j, 0], resp_valid[on, i, j, 1], cells[i, on], cells[j, on], actions[on, i],
                     W, HW, R)
            np.add.at(counts, b, 1)
            if crash_bits is not None:
                hit = ((np.asarray(crash_bits)[on].astype(np.int64) >> j) & 1).astype(bool)
                np.add.at(counts, plane + b[hit], 1)
    return counts.reshape(2, NA, O, NV, NV), visits


def bin_resp(steps, W, HW, R):
    """steps: [(resp_full [E, N, N] f64, cells [N, E], actions [E, N])] -> per (action, offset), over all steps:
    (the correctly rounded sum [9, O], sum|x| [9, O], the number of terms [9, O])."""
    O = n_offsets(R)
    terms = [[] for _ in range(NA * O)]
    for resp, cells, actions in steps:
        N = resp.shape[1]
        for i in range(N):
            for j in range(N):
                if i == j:
                    continue
                b = act9(actions[:, i]) * O + offset_bins(cells[i], cells[j], W, HW, R)
                for bb, xx in zip(b.tolist(), resp[:, i, j].tolist()):
                    terms[bb].append(xx)
    exact = np.array([math.fsum(t) for t in terms]).reshape(NA, O)
    mag = np.array([math.fsum(abs(v) for v in t) for t in terms]).reshape(NA, O)
    n = np.array([len(t) for t in terms]).reshape(NA, O)
    return exact, mag, n
