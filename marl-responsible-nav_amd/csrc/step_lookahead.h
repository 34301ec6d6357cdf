// step_lookahead.h -- the trap and mask rules of gw_step_lookahead (csrc/step_lookahead.hip, include/gridenv.h).
//
// A pure function, host and device, so that the kernel and a stand-alone CPU program
// (tools/step_lookahead_check.cpp) run the same text.  One RL agent k of one env:
//   m        its 9-bit action mask (has_mask false: no mask was given, all nine);
//   crash9   bit a: k itself crashes in the step about to run under first action a (gw_step_preview's);
//   ends     bit a: that step ends the episode under a, so no second step exists;
//   mask2[a] the action mask the step would return under a (the cell table's bits of k's cell after a);
//   crash2[a] bit b: k itself crashes in the step after, playing b from that cell (0 where the step ends).
// Trap: a is a trap action when the step goes on under a, the cell after it allows some action, and every
// action it allows crashes k:
//   trap9 bit a = !ends[a] && mask2[a] != 0 && (mask2[a] & ~crash2[a]) == 0
// The lookahead mask takes the crashing and the trap actions out of m; if nothing is left it is the preview's
// safe mask (step_preview.h: m & ~crash9, or m unchanged if that is empty too):
//   ahead = m & ~crash9 & ~trap9,  empty: step_preview::safe_mask(m, crash9)
#ifndef STEP_LOOKAHEAD_H
#define STEP_LOOKAHEAD_H
#include <stdint.h>

#include "step_preview.h"

namespace step_lookahead {

constexpr int NA = 9;
constexpr uint32_t ALL = step_preview::ALL;

struct Ahead {
    uint32_t trap9, ahead_mask;
};

// mask2 / crash2: nine entries each, read through operator[] (a pointer, or the kernel's LDS views)
template <class Mask2, class Crash2>
SP_HD Ahead rules(bool has_mask, uint32_t m, uint32_t crash9, uint32_t ends, const Mask2 &mask2,
                  const Crash2 &crash2) {
    uint32_t trap9 = 0u;
    for (int a = 0; a < NA; ++a) {
        const uint32_t m2 = (uint32_t)mask2[a] & ALL, c2 = (uint32_t)crash2[a] & ALL;
        const bool goes_on = !((ends >> a) & 1u);
        trap9 |= (uint32_t)(goes_on && m2 != 0u && (m2 & ~c2) == 0u) << a;
    }
    crash9 &= ALL;
    const uint32_t mm = has_mask ? (m & ALL) : ALL;
    const uint32_t ahead = mm & ~crash9 & ~trap9;
    return Ahead{trap9, ahead ? ahead : step_preview::safe_mask(has_mask, m, crash9)};
}

}  // namespace step_lookahead
#endif  // STEP_LOOKAHEAD_H
