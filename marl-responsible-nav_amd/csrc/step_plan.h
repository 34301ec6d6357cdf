// step_plan.h -- the depth, return, path and mask rules of gw_step_plan (csrc/step_plan.hip, include/gridenv.h).
//
// Pure functions, host and device, so that the kernel and a stand-alone CPU program (tools/step_plan_check.cpp)
// run the same text.  One RL agent k of one env, horizon H (2..HORIZON_MAX), on step_horizon.h's levels and
// nodes: level h is the world after h steps that k survived, a node of level h a cell k can stand in there.
// Beside its cell, k's state is whether its own apple is still there; nothing else differs between k's choices.
// Every action b a node allows has one transition (Tr) for step h + 1 played from it:
//   code  step_horizon.h's transition code in the world WITHOUT k's apple: CRASH (k itself crashes), END (k does
//         not crash and the step cap or another RL agent's crash ends the episode), else k's node at level h + 1;
//   eat   with k's apple present, the step pops it;
//   last  ... and that was the env's last apple, which ends the episode (k not crashing);
//   rw    the step's env reward for k, in tenths, with k's apple present.
// Without its apple k earns nothing but its crash, so that world keeps step_horizon.h's recursion:
//   D0[h][node] = step_horizon::node_depth;  the return from there is 0 if D0 == H, else CRASH_TENTHS.
// With the apple present a node keeps the lexicographic maximum (depth first, return second) over its allowed b of
//   after1(h, t) = CRASH:                       (h, rw)
//                  END, last, or h + 1 == H:    (H, rw)
//                  eat:                         (D0[h + 1][code], rw + (that depth == H ? 0 : CRASH_TENTHS))
//                  otherwise:                   (D1[h + 1][code], rw + R1[h + 1][code])
// and a node that allows nothing is (H, 0) in both worlds.  Ties go to the lowest action.  The first step is
// after1(0, t) with t.eat = "k's apple is not there after step 1" (eaten by it, or before) and t.last = false (its
// END covers every episode end).  The levels are folded from H - 1 down to 1.
//   plan_mask = the actions of m (has_mask false: all nine) whose (depth, ret) is the lexicographic maximum over m;
//               m == 0: 0.
// A node also keeps, per world, the step its best continuation takes (link), from which path() reads the actions
// after the first: the crash step is the path's last entry, as is the step that ends the episode or reaches the
// horizon; a node that allows nothing ends the path before it.
#ifndef STEP_PLAN_H
#define STEP_PLAN_H
#include <stdint.h>

#include "step_horizon.h"

namespace step_plan {

constexpr int NA = step_horizon::NA;
constexpr int HORIZON_MAX = step_horizon::HORIZON_MAX;
constexpr uint32_t ALL = step_horizon::ALL, CRASH = step_horizon::CRASH, END = step_horizon::END;
constexpr int32_t CRASH_TENTHS = -100;   // the env's -10 for k's own crash
constexpr uint32_t NO_ACTION = 0xFu;     // a link's action where the node allows nothing
constexpr uint32_t NO_PATH = 0xFFFFFFu;  // HORIZON_MAX - 1 path entries of 0xFF
static_assert(HORIZON_MAX - 1 == 3, "path() packs HORIZON_MAX - 1 entries into three bytes");

struct Tr {
    uint32_t code;
    bool eat, last;
    int32_t rw;
};

// one 32-bit word per transition: code | eat << 8 | last << 9 | rw (i16) << 16
SP_HD uint32_t pack(const Tr &t) {
    return (t.code & 0xFFu) | ((uint32_t)t.eat << 8) | ((uint32_t)t.last << 9) | (((uint32_t)t.rw & 0xFFFFu) << 16);
}
SP_HD Tr unpack(uint32_t w) {
    return Tr{w & 0xFFu, ((w >> 8) & 1u) != 0u, ((w >> 9) & 1u) != 0u, (int32_t)(int16_t)(uint16_t)(w >> 16)};
}

struct Val {
    uint32_t depth;
    int32_t ret;
};
SP_HD bool better(const Val &a, const Val &b) { return a.depth > b.depth || (a.depth == b.depth && a.ret > b.ret); }

// the world without k's apple from a state of depth d on
SP_HD Val bare(uint32_t d, int H) { return Val{d, d == (uint32_t)H ? 0 : CRASH_TENTHS}; }

// Deeper: the values of level h + 1 by transition code: d0(code), d1(code), r1(code)
template <class Deeper>
struct D0Of {  // ... as step_horizon's functions read its D0
    const Deeper &dp;
    SP_HD uint32_t operator[](uint32_t code) const { return dp.d0(code); }
};

template <class Deeper>
SP_HD Val after0(int h, int H, const Tr &t, const Deeper &dp) {
    return bare(step_horizon::after(h, H, t.code, D0Of<Deeper>{dp}), H);
}

template <class Deeper>
SP_HD Val after1(int h, int H, const Tr &t, const Deeper &dp) {
    if (t.code == CRASH) return Val{(uint32_t)h, t.rw};
    if (t.code == END || t.last || h + 1 >= H) return Val{(uint32_t)H, t.rw};
    if (t.eat) {
        const Val v = after0(h, H, t, dp);
        return Val{v.depth, t.rw + v.ret};
    }
    const uint32_t d = dp.d1(t.code);
    return Val{d < (uint32_t)H ? d : (uint32_t)H, t.rw + dp.r1(t.code)};
}

// The step a continuation takes from a node of level h: b | it goes on to a node << 4 | k's apple is there
// afterwards << 5 | that node << 8; present: k's apple is there before the step
SP_HD uint32_t link(int h, int H, uint32_t b, const Tr &t, bool present) {
    const bool on = t.code < END && !(present && t.last) && h + 1 < H;
    return (b & 0xFu) | ((uint32_t)on << 4) | ((uint32_t)(present && !t.eat) << 5) | ((t.code & 0xFFu) << 8);
}

struct Node {
    uint32_t d0, l0;  // without k's apple: depth, link
    uint32_t d1, l1;  // with it: depth, link ...
    int32_t r1;       // ... and return
};

// k stands in a node of level h >= 1 whose cell allows `mask`; next[b]: the packed transition of action b (read for
// the allowed b only)
template <class Next, class Deeper>
SP_HD Node node(int h, int H, uint32_t mask, const Next &next, const Deeper &dp) {
    mask &= ALL;
    Node n{(uint32_t)H, NO_ACTION, (uint32_t)H, NO_ACTION, 0};
    bool any = false;
    for (int b = 0; b < NA; ++b) {
        if (!((mask >> b) & 1u)) continue;
        const Tr t = unpack((uint32_t)next[b]);
        const Val v0 = after0(h, H, t, dp), v1 = after1(h, H, t, dp);
        if (!any || v0.depth > n.d0) {
            n.d0 = v0.depth;
            n.l0 = link(h, H, (uint32_t)b, t, false);
        }
        if (!any || better(v1, Val{n.d1, n.r1})) {
            n.d1 = v1.depth;
            n.r1 = v1.ret;
            n.l1 = link(h, H, (uint32_t)b, t, true);
        }
        any = true;
    }
    return n;
}

// The actions after the first of the continuation that attains the first action's value: entry h - 1 in bits
// 8 (h - 1)..8 (h - 1) + 7, 0xFF past the end.  links(h, node, present): the node's link in that world.
template <class Links>
SP_HD uint32_t path(int H, const Tr &first, const Links &links) {
    uint32_t out = NO_PATH, code = first.code;
    bool present = !first.eat;
    for (int h = 1; h < H && h < HORIZON_MAX && code < END; ++h) {
        const uint32_t l = (uint32_t)links(h, code, present);
        if ((l & 0xFu) >= (uint32_t)NA) break;
        const int sh = 8 * (h - 1);
        out = (out & ~(0xFFu << sh)) | ((l & 0xFu) << sh);
        if (!((l >> 4) & 1u)) break;
        present = ((l >> 5) & 1u) != 0u;
        code = (l >> 8) & 0xFFu;
    }
    return out;
}

// depth9 / ret9: nine entries each, read through operator[]
template <class Depth9, class Ret9>
SP_HD uint32_t plan_mask(bool has_mask, uint32_t m, const Depth9 &depth9, const Ret9 &ret9) {
    const uint32_t mm = has_mask ? (m & ALL) : ALL;
    Val top{0u, 0};
    uint32_t pick = 0u;
    for (int a = 0; a < NA; ++a) {
        if (!((mm >> a) & 1u)) continue;
        const Val v{(uint32_t)depth9[a], (int32_t)ret9[a]};
        if (pick == 0u || better(v, top)) {
            top = v;
            pick = 0u;
        }
        pick |= (uint32_t)(v.depth == top.depth && v.ret == top.ret) << a;
    }
    return pick;
}

}  // namespace step_plan
#endif  // STEP_PLAN_H
