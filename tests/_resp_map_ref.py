"""numpy restatement of gw_resp_map_accum (include/rollout_ops.h, csrc/resp_map.h) and of the per-cell sums
its counts stand for; shared by tests/test_resp_map_cpu.py and tests/test_gpu_resp_map.py.

The bound.  ``resp_map_from_counts`` forms, per cell, sum_b c_b * T_b over the m <= 100 non-empty (vm, va)
bins b of the cell (an empty bin adds an exact 0.0): one rounded product each (exact when c_b == 1) and m - 1
rounded additions, so it differs from the exact sum S = sum of the cell's n >= m terms x (each x is one T_b) by
at most about m * u * sum|x|, u = 2^-53.  The reference sum here is ``math.fsum``, the correctly rounded S
(within u / 2 * |S| of it), so |map - reference| <= n * u * sum|x| holds by derivation; the tests use exactly
that bound, computed from the data, per cell."""
import math

import numpy as np

U = 2.0 ** -53
NV = 10


def popcount9(x):
    x = np.asarray(x).astype(np.int64) & 0x1FF
    return sum((x >> b) & 1 for b in range(9))


def bins(set_mdr, set_act, cell_i, cell_j, HW):
    """-> (caused, received) int64 indices into counts[2][HW][10][10] (flat)."""
    vm, va = popcount9(set_mdr), popcount9(set_act)
    ci = np.clip(np.asarray(cell_i, np.int64), 0, HW - 1)
    cj = np.clip(np.asarray(cell_j, np.int64), 0, HW - 1)
    return (ci * NV + vm) * NV + va, ((HW + cj) * NV + vm) * NV + va


def fold(resp_valid, cells, HW, active=None):
    """One step: resp_valid [E, N, N, 2] (non-negative ints), cells [N, E], active [E] bool or None
    -> (counts [2, HW, 10, 10] int64, visits [HW] int64)."""
    E, N = resp_valid.shape[:2]
    counts, visits = np.zeros(2 * HW * NV * NV, np.int64), np.zeros(HW, np.int64)
    on = np.ones(E, bool) if active is None else np.asarray(active, bool)
    for i in range(N):
        np.add.at(visits, np.clip(cells[i, on].astype(np.int64), 0, HW - 1), 1)
        for j in range(N):
            if i == j:
                continue
            ca, re = bins(resp_valid[on, i, j, 0], resp_valid[on, i, j, 1], cells[i, on], cells[j, on], HW)
            np.add.at(counts, ca, 1)
            np.add.at(counts, re, 1)
    return counts.reshape(2, HW, NV, NV), visits


def bin_resp(steps, HW):
    """steps: [(resp_full [E, N, N] f64, cells [N, E], active [E] bool or None)] -> per plane and cell, over all
    steps: (the correctly rounded sum [2, HW], sum|x| [2, HW], the number of terms [2, HW], numpy's own
    sequential binning [2, HW])."""
    terms = [[[] for _ in range(HW)] for _ in range(2)]
    seq = np.zeros((2, HW))
    for resp, cells, active in steps:
        E, N = resp.shape[:2]
        on = np.ones(E, bool) if active is None else np.asarray(active, bool)
        for i in range(N):
            for j in range(N):
                if i == j:
                    continue
                x = resp[on, i, j]
                for p, c in ((0, cells[i, on]), (1, cells[j, on])):
                    c = np.clip(c.astype(np.int64), 0, HW - 1)
                    np.add.at(seq[p], c, x)
                    for cc, xx in zip(c.tolist(), x.tolist()):
                        terms[p][cc].append(xx)
    exact = np.array([[math.fsum(t) for t in plane] for plane in terms])
    mag = np.array([[math.fsum(abs(v) for v in t) for t in plane] for plane in terms])
    n = np.array([[len(t) for t in plane] for plane in terms])
    return exact, mag, n, seq
