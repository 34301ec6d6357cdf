"""Responsibility footprints on the host: the counts of gw_resp_footprint_accum (include/rollout_ops.h) into
sums of Resp.

The device counts, per plane (0: every affected agent, 1: the affected agents that crashed in the step), per
action of the actor (0..8), per offset (dr, dc) of the affected agent from the actor (the (2R + 1)^2 near bins
in row-major order, then one far bin for everything beyond radius R) and per pair of valid-action counts
(vm, va), how many (env, actor, affected) pair-steps fell there.  Since ``resp_full[e, i, j] == T[vm][va]`` the
sum of Resp per (action, offset) is a weighted sum of at most 100 integers, formed here in the fixed order of
``resp_map_from_counts``: the totals are the same bit for bit whatever order the device's increments arrived in.
Pure host code (numpy / CPU torch); no GPU needed."""
from __future__ import annotations

import math

import numpy as np
import torch

from .resp_map import NV, resp_table

NA = 9  # the actor's actions 0..8


def offsets(radius: int) -> int:
    """O = (2R + 1)^2 + 1: the near window's bins and the far bin."""
    return (2 * int(radius) + 1) ** 2 + 1


def radius_of(n_offsets: int) -> int:
    """The R whose ``offsets(R)`` is n_offsets (ValueError if there is none in 1..15)."""
    side = math.isqrt(max(int(n_offsets) - 1, 0))
    if side * side != n_offsets - 1 or side % 2 == 0 or not 1 <= side // 2 <= 15:
        raise ValueError(f"resp_footprint: {n_offsets} offset bins is (2R + 1)^2 + 1 for no R in 1..15")
    return side // 2


def resp_footprint_from_counts(counts, table=None):
    """-> (footprint [2, 9, O] f64, pairs [2, 9, O] int64, (near [2, 9, 2R+1, 2R+1], far [2, 9])), CPU tensors.
    counts: [2, 9, O, 10, 10] integers (gw_resp_footprint_accum's buffer; a tensor or an array), table: T
    [10, 10] f64 (default ``resp_table()``).
    footprint[p][a][o] = sum_vm sum_va counts[p][a][o][vm][va] * T[vm][va], accumulated in f64 from 0.0 with vm
    outer and va inner, both ascending; pairs[p][a][o] = sum counts[p][a][o] (the pair-steps binned there,
    exact).  near and far are views of footprint: near[p][a][dr + R][dc + R] is the Resp action a caused to an
    agent standing at offset (dr, dc) from the actor, far[p][a] what it caused beyond radius R."""
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    if c.ndim != 5 or c.shape[:2] != (2, NA) or c.shape[3:] != (NV, NV) or c.dtype.kind not in "iu":
        raise ValueError("resp_footprint_from_counts: counts must be integers of shape [2, 9, O, 10, 10]")
    O = c.shape[2]
    R = radius_of(O)
    T = resp_table() if table is None else np.asarray(
        table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else table, dtype=np.float64)
    if T.shape != (NV, NV):
        raise ValueError("resp_footprint_from_counts: table must be [10, 10]")
    cf = c.astype(np.float64)  # (exact below 2^53)
    out = np.zeros(c.shape[:3], np.float64)
    for vm in range(NV):  # the order is the contract: one rounded multiply and one rounded add per term
        for va in range(NV):
            out = out + cf[:, :, :, vm, va] * T[vm, va]
    pairs = c.astype(np.int64).reshape(2, NA, O, NV * NV).sum(-1)
    fp = torch.from_numpy(out)
    S = 2 * R + 1
    return fp, torch.from_numpy(pairs), (fp[:, :, :O - 1].unflatten(2, (S, S)), fp[:, :, O - 1])
