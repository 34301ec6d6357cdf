// fear_shield.h -- the selection rule of gw_fear_shield (csrc/rollout_ops.hip, include/rollout_ops.h).
//
// A pure function, host and device, so that the kernel and a stand-alone CPU program
// (tools/fear_shield_check.cpp) run the same text.  One RL agent of one env: its proposed action p, its row
// t[9] of gw_fear_preview's table (its FeAR under each of its nine actions while everybody else plays the
// action the step will apply), its 9-bit action mask m, optionally its actor's probabilities pr[9], the
// threshold tau.
//   not shielded, or m == 0:        keep p, flags 0.
//   A = { a : bit a of m, t[a] <= tau }   (an f64 compare: equality is allowed)
//   p in A:                         keep p, flags 0.
//   A non-empty:                    the a in A with the largest pr[a] (no pr: the smallest t[a]), ties to the
//                                   lowest a; flags 1 (replaced).
//   A empty:                        the masked a with the smallest t[a], ties to the lowest a; flags 2 (stuck),
//                                   3 if that differs from p.
// The shield is unilateral: the row assumes that the OTHER agents play their proposed actions.  When one
// agent alone is shielded the step's fear of that agent is exactly the chosen entry t[pick]; with several
// agents shielded at once that holds for an agent only if the others' actions were kept.
// gw_fear_shield_joint (csrc/fear_shield_joint.hip, include/gridenv.h) runs this same pick agent after agent,
// each on the row of the actions fixed so far, and hands back the table of the applied joint action.
#ifndef FEAR_SHIELD_H
#define FEAR_SHIELD_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FS_HD __host__ __device__ __forceinline__
#else
#define FS_HD inline
#endif

namespace fear_shield {

constexpr int NA = 9;  // GW_N_ACTIONS

struct Pick {
    int action;
    int flags;  // bit 0: the action differs from the proposed one; bit 1: no allowed action existed
};

FS_HD Pick pick(const double *t, int p, uint32_t m, const float *pr, double tau, bool shielded) {
    Pick r;
    r.action = p;
    r.flags = 0;
    m &= 0x1FFu;
    if (!shielded || m == 0u) return r;
    uint32_t A = 0u;
    for (int a = 0; a < NA; ++a)
        if (((m >> a) & 1u) && t[a] <= tau) A |= 1u << a;
    if (p >= 0 && p < NA && ((A >> p) & 1u)) return r;
    const uint32_t from = A ? A : m;  // no allowed action: the least-FeAR masked one
    const bool by_prob = A && pr;
    int best = -1;
    for (int a = 0; a < NA; ++a) {
        if (!((from >> a) & 1u)) continue;
        if (best < 0 || (by_prob ? pr[a] > pr[best] : t[a] < t[best])) best = a;  // strict: ties stay at the lowest a
    }
    r.action = best;  // from != 0: best >= 0
    r.flags = A ? 1 : (2 | (best != p ? 1 : 0));
    return r;
}

}  // namespace fear_shield
#endif  // FEAR_SHIELD_H
