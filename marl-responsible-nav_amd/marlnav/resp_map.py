"""Responsibility maps on the host: the counts of gw_resp_map_accum (include/rollout_ops.h) into sums of Resp.

The device counts, per plane (0: caused at the actor's cell, 1: received at the affected agent's cell), cell
and pair of valid-action counts (vm, va), how many (env, actor, affected) pair-steps fell there.  Since
``resp_full[e, i, j] == T[vm][va]`` the per-cell sum of Resp is a weighted sum of at most 100 integers, formed
here in one fixed order: the totals are the same bit for bit whatever order the device's increments arrived in.
Pure host code (numpy / CPU torch); no GPU needed."""
from __future__ import annotations

import numpy as np
import torch

NV = 10  # valid-action counts 0..9
EPS = 0.000001


def resp_table() -> np.ndarray:
    """The Resp half of the host table every env is created with (csrc/resp_tables.h):
    T[vm][va] = clip((vm - va) / (vm + 1e-6), -1, 1), one rounded IEEE f64 operation each -> [10, 10] f64."""
    vm = np.arange(NV, dtype=np.float64)[:, None]
    va = np.arange(NV, dtype=np.float64)[None, :]
    return np.clip((vm - va) / (vm + EPS), -1.0, 1.0)


def resp_map_from_counts(counts, table=None):
    """-> (map [2, HW] f64, pairs [2, HW] int64), CPU tensors.
    counts: [2, HW, 10, 10] integers (gw_resp_map_accum's buffer; a tensor or an array), table: T [10, 10]
    f64 (default ``resp_table()``).
    map[p][c] = sum_vm sum_va counts[p][c][vm][va] * T[vm][va], accumulated in f64 from 0.0 with vm outer and
    va inner, both ascending; pairs[p][c] = sum counts[p][c] (the pair-steps binned at the cell, exact), so
    map / pairs is the mean Resp per pair-step there."""
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    if c.ndim != 4 or c.shape[0] != 2 or c.shape[2:] != (NV, NV) or c.dtype.kind not in "iu":
        raise ValueError("resp_map_from_counts: counts must be integers of shape [2, HW, 10, 10]")
    T = resp_table() if table is None else np.asarray(
        table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else table, dtype=np.float64)
    if T.shape != (NV, NV):
        raise ValueError("resp_map_from_counts: table must be [10, 10]")
    cf = c.astype(np.float64)  # (exact below 2^53)
    out = np.zeros(c.shape[:2], np.float64)
    for vm in range(NV):  # the order is the contract: one rounded multiply and one rounded add per term
        for va in range(NV):
            out = out + cf[:, :, vm, va] * T[vm, va]
    pairs = c.astype(np.int64).reshape(2, c.shape[1], NV * NV).sum(-1)
    return torch.from_numpy(out), torch.from_numpy(pairs)
