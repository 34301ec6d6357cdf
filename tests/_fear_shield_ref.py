"""A numpy restatement of the responsibility shield's selection rule (include/rollout_ops.h gw_fear_shield),
written from the rule's wording, not from csrc/fear_shield.h: the reference of the CPU and GPU shield tests."""
import numpy as np


def pick_one(t, p, m, pr, tau, shielded):
    """One agent: table row t [9] f64, proposed action p, 9-bit mask m, probabilities pr [9] f32 or None."""
    m = int(m) & 0x1FF
    if not shielded or m == 0:
        return int(p), 0
    masked = [a for a in range(9) if (m >> a) & 1]
    allowed = [a for a in masked if np.float64(t[a]) <= np.float64(tau)]
    if int(p) in allowed:
        return int(p), 0
    if allowed:
        if pr is not None:
            best = max(np.float32(pr[a]) for a in allowed)
            a = min(a for a in allowed if np.float32(pr[a]) == best)
        else:
            best = min(np.float64(t[a]) for a in allowed)
            a = min(a for a in allowed if np.float64(t[a]) == best)
        return a, 1
    best = min(np.float64(t[a]) for a in masked)
    a = min(a for a in masked if np.float64(t[a]) == best)
    return a, 2 | int(a != int(p))


def shield_ref(table, actions, mask=None, probs=None, tau=0.0, agents=None):
    """table [E, K, 9] f64, actions [E, K], mask [E, K] or None, probs [K, E, 9] f32 or None, agents: bitmask
    or None (all) -> (actions [E, K] int32, flags [E, K] uint8)."""
    E, K = actions.shape
    out = np.zeros((E, K), np.int32)
    flags = np.zeros((E, K), np.uint8)
    bits = (1 << K) - 1 if agents is None else int(agents)
    for e in range(E):
        for k in range(K):
            m = 0x1FF if mask is None else int(mask[e, k]) & 0xFFFF
            out[e, k], flags[e, k] = pick_one(table[e, k], actions[e, k], m, None if probs is None else probs[k, e],
                                              tau, (bits >> k) & 1)
    return out, flags
