"""The descriptor-only window ring's rules restated in numpy (tests/test_replay_desc_patch_cpu.py pins them to
the oracle's full observations; tests/test_gpu_replay_desc_patch.py uses the descriptor decode for its
coverage conditions).  A descriptor is 12 u32 words: words 0-3 the agents' cells of the obs half (16 bits each),
word 4 the flags (bit 0 reset encoding, bits 8-15 the apples present in the obs, bits 16-23 in the terminal
obs), words 8-11 the agents' cells of the terminal half."""
import numpy as np

MAXP = 129  # gw_obs_patch's largest window


def magic(d):
    """min(2^32 - 1, ceil(2^32 / d)): the multiplier gw_replay_gather_desc_patch computes for i / P."""
    d = np.asarray(d, np.uint64)
    return np.minimum(np.uint64(0xFFFFFFFF), ((np.uint64(1) << np.uint64(32)) + d - np.uint64(1)) // d)


def half_cells(desc, which, N):
    """desc [..., 12] (any integer dtype holding the u32 words) -> the agents' cells [..., N] of the obs half
    (which = 0) or the terminal half (which = 1)."""
    d = np.asarray(desc).astype(np.int64) & 0xFFFFFFFF
    w = d[..., 8:12] if which else d[..., 0:4]
    return np.stack([(w[..., n >> 1] >> (16 * (n & 1))) & 0xFFFF for n in range(N)], -1)


def half_flags(desc, which):
    """-> (reset encoded?, apple bits) of that half; the terminal half is never reset-encoded."""
    f = np.asarray(desc).astype(np.int64)[..., 4] & 0xFFFFFFFF
    if which:
        return np.zeros(f.shape, bool), (f >> 16) & 0xFF
    return (f & 1).astype(bool), (f >> 8) & 0xFF


def agent_value(reset, n, k, on_apple, variant=0):
    """csrc/obs_value.h: the obs value of agent n's cell in RL agent k's observation."""
    if reset:
        return 9.5 if on_apple else 0.5
    if on_apple:
        return float(n + 1 + 9)
    if variant == 1:
        return float(n + 1)
    v = n + 1
    if 1 <= v <= 4 and v != k + 1:
        v = 5
    if v == k + 1:
        v = 1
    return float(v)


def window(cells, apple_bits, reset, k, P, base, apple_cells, variant=0):
    """The P x P window of RL agent k's obs from one descriptor half: rows / cols -P/2 .. P-1-P/2 around agent
    k's own cell in that half, -1 outside the grid, the map value else (base [H, W]: 0 road, -1 inactive), then
    the patched cells in slot order (the own apple first, then agents 0 .. N-1: a later one overrides)."""
    H, W = base.shape
    half = P // 2
    cr, cc = divmod(int(cells[k]), W)
    out = np.full((P, P), -1.0, np.float32)
    r0, c0 = cr - half, cc - half
    ra, rb = max(r0, 0), min(r0 + P, H)
    ca, cb = max(c0, 0), min(c0 + P, W)
    out[ra - r0:rb - r0, ca - c0:cb - c0] = base[ra:rb, ca:cb]
    patches = []
    ac = int(apple_cells[k]) if (int(apple_bits) >> k) & 1 else -1
    if ac >= 0:
        av = float(base.reshape(-1)[ac]) + 9.0
        if not reset and av == float(k + 1):
            av = 1.0
        patches.append((ac, av))
    for n, c in enumerate(cells):
        patches.append((int(c), agent_value(reset, n, k, int(c) == ac, variant)))
    for c, v in patches:
        wr, wc = c // W - r0, c % W - c0
        if 0 <= wr < P and 0 <= wc < P:
            out[wr, wc] = v
    return out


def crop(obs2d, cell, P):
    """The same window as a crop of the full obs [H, W] padded with -1."""
    H, W = obs2d.shape
    pad = np.full((H + 2 * P, W + 2 * P), -1.0, np.float32)
    pad[P:P + H, P:P + W] = obs2d
    cr, cc = divmod(int(cell), W)
    r0, c0 = cr - P // 2 + P, cc - P // 2 + P
    return pad[r0:r0 + P, c0:c0 + P]


def coverage(cells_k, cells_all, H, W, P):
    """Coverage of a set of windows, decided from cells alone.  cells_k [M]: the centres; cells_all [M, N]: every
    agent's cell of the same half; -> (overhang top, bottom, left, right: bool each; windows holding another
    agent's cell; windows with another agent's cell outside)."""
    half = P // 2
    cr, cc = cells_k // W, cells_k % W
    r0, c0 = cr - half, cc - half
    over = ((r0 < 0).any(), (r0 + P > H).any(), (c0 < 0).any(), (c0 + P > W).any())
    wr, wc = cells_all // W - r0[:, None], cells_all % W - c0[:, None]
    inside = (wr >= 0) & (wr < P) & (wc >= 0) & (wc < P)
    other = cells_all != cells_k[:, None]
    return over, int((inside & other).any(1).sum()), int((~inside & other).any(1).sum())
