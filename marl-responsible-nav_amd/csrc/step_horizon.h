// step_horizon.h -- the depth, viable-set and mask rules of gw_step_horizon (csrc/step_horizon.hip,
// include/gridenv.h).
//
// Pure functions, host and device, so that the kernel and a stand-alone CPU program
// (tools/step_horizon_check.cpp) run the same text.  One RL agent k of one env, horizon H (2..HORIZON_MAX).
// The forward pass leaves a transition table: level h (0..H-1) is the world after h steps that k survived, a
// node of level h a cell k can stand in there (level 0: one node, k's present cell), and every action b the
// node allows has one transition code for step h + 1 played from it:
//   CRASH        k itself crashes in that step;
//   END          k does not crash and the step ends the episode;
//   anything else: k does not crash, the episode goes on, and the code is k's node at level h + 1.
// Depth is the largest d such that some continuation keeps k from crashing in steps 1..d, counted as H when the
// horizon or an episode end is reached, or when k stands in a node that allows no action:
//   after(h, code)  = CRASH: h;  END: H;  node: h + 1 == H ? H : depth[h + 1][node]
//   depth[h][node]  = mask == 0 ? H : max over the allowed b of after(h, next[b])        (h >= 1)
//   depth9[a]       = after(0, first[a])                                                 (every first action a)
// The levels are folded from H - 1 down to 1, so depth[h + 1] is complete when level h reads it.
//   viable9 bit a = depth9[a] == H
//   horizon_mask  = the actions of m (has_mask false: all nine) whose depth is the maximum over m; m == 0: 0.
// At H = 2 depth 0 / 1 / 2 is "a crashes k" / "a is a trap action" / neither, and the mask rule is
// step_lookahead.h's chain: m without crashes and traps, else m without crashes, else m.
#ifndef STEP_HORIZON_H
#define STEP_HORIZON_H
#include <stdint.h>

#include "step_preview.h"

namespace step_horizon {

constexpr int NA = 9;
constexpr int HORIZON_MAX = 4;  // GW_HORIZON_MAX (include/gridenv.h)
constexpr uint32_t ALL = step_preview::ALL;
constexpr uint32_t CRASH = 0xFFu, END = 0xFEu;  // transition codes; a node index is below END

struct Horizon {
    uint32_t viable9, horizon_mask;
};

// k plays one action at level h (step h + 1) with transition `code`; deeper[node]: the depths of level h + 1
template <class Deeper>
SP_HD uint32_t after(int h, int H, uint32_t code, const Deeper &deeper) {
    if (code == CRASH) return (uint32_t)h;
    if (code == END || h + 1 >= H) return (uint32_t)H;
    const uint32_t d = (uint32_t)deeper[code];
    return d < (uint32_t)H ? d : (uint32_t)H;
}

// k stands in a node of level h >= 1 whose cell allows `mask`; next[b]: the transition code of action b (read for
// the allowed b only)
template <class Next, class Deeper>
SP_HD uint32_t node_depth(int h, int H, uint32_t mask, const Next &next, const Deeper &deeper) {
    mask &= ALL;
    if (mask == 0u) return (uint32_t)H;
    uint32_t best = (uint32_t)h;
    for (int b = 0; b < NA; ++b) {
        if (!((mask >> b) & 1u)) continue;
        const uint32_t d = after(h, H, (uint32_t)next[b], deeper);
        best = d > best ? d : best;
    }
    return best;
}

// depth9: nine entries in 0..H, read through operator[]
template <class Depth9>
SP_HD Horizon rules(bool has_mask, uint32_t m, int H, const Depth9 &depth9) {
    const uint32_t mm = has_mask ? (m & ALL) : ALL;
    uint32_t viable9 = 0u, top = 0u, pick = 0u;
    for (int a = 0; a < NA; ++a) {
        const uint32_t d = (uint32_t)depth9[a];
        viable9 |= (uint32_t)(d == (uint32_t)H) << a;
        if (!((mm >> a) & 1u)) continue;
        if (d > top || pick == 0u) {
            top = d;
            pick = 0u;
        }
        pick |= (uint32_t)(d == top) << a;
    }
    return Horizon{viable9, pick};
}

}  // namespace step_horizon
#endif  // STEP_HORIZON_H
