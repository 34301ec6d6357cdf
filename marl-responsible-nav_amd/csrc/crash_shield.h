// crash_shield.h -- the visit rule of gw_crash_shield_joint (csrc/crash_shield_joint.hip, include/gridenv.h).
//
// A pure function, host and device, on top of fear_shield.h and step_preview.h, so that the kernel and a
// stand-alone CPU program (tools/crash_shield_check.cpp) run the same text.  One visit of one RL agent: its
// current action cur, its 9-bit action mask m (has_mask false: no mask was given, all nine), crash9 (bit a set
// when the agent itself crashes under action a while everybody else plays the actions fixed so far), its row
// t[9] of the FeAR table of those actions (read only with use_fear), optionally its actor's probabilities
// pr[9], the threshold tau.
//   m'          = step_preview::safe_mask(has_mask, m, crash9): the mask without the crashing actions, or the
//                 mask itself where nothing avoids the crash;
//   r           = fear_shield::pick(use_fear ? t : nine zeros, cur, m', pr, use_fear ? tau : 0.0, true);
//   unavoidable = the mask (all nine if none) is non-empty and every action of it crashes the agent.
// The answer: r.action, and flags = r.flags (bit 0 the action differs from cur, bit 1 no allowed action)
// | unavoidable << 5 (the bit's place in gw_crash_shield_joint's flags).
// Without FeAR the table is zero under tau = 0, so every action of m' is allowed: an agent that would crash
// is moved to the most probable action under which it does not (no pr: the lowest), and nothing else moves.
// A non-empty m' always holds the answer, so the agent crashes under it only where the visit was unavoidable.
#ifndef CRASH_SHIELD_H
#define CRASH_SHIELD_H
#include <stdint.h>

#include "fear_shield.h"
#include "step_preview.h"

namespace crash_shield {

constexpr int UNAVOIDABLE = 1 << 5;

struct Visit {
    int action;
    int flags;  // bits 0-1: fear_shield::Pick's; bit 5: unavoidable
};

FS_HD Visit visit(const double *t, int cur, bool has_mask, uint32_t m, uint32_t crash9, const float *pr,
                  bool use_fear, double tau) {
    static constexpr double zero[fear_shield::NA] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // (no stack copy)
    crash9 &= step_preview::ALL;
    const uint32_t safe = step_preview::safe_mask(has_mask, m, crash9);
    const fear_shield::Pick r = fear_shield::pick(use_fear ? t : zero, cur, safe, pr, use_fear ? tau : 0.0, true);
    const uint32_t mm = has_mask ? (m & step_preview::ALL) : step_preview::ALL;
    Visit v;
    v.action = r.action;
    v.flags = r.flags | ((mm != 0u && (mm & ~crash9) == 0u) ? UNAVOIDABLE : 0);
    return v;
}

}  // namespace crash_shield
#endif  // CRASH_SHIELD_H
