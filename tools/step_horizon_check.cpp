// step_horizon_check.cpp -- stand-alone host program around the depth, viable-set and mask rules of gw_step_horizon
// (csrc/step_horizon.h, the text the kernel runs), for tests/test_step_horizon_cpu.py, which builds it with
// AddressSanitizer + UBSan.  It compares the rules with a plain restatement of include/gridenv.h's wording:
//   depth: random transition tables (H = 2..4, up to 12 nodes per level, masks with and without holes, empty
//     masks, every transition code), folded level by level as the kernel folds them, against a depth-first search
//     over the same table with no memoisation;
//   mask:  every depth table of (H + 1)^9 for H = 2, 3 and 4 under no mask and under a set of small masks, against
//     "the actions of m whose depth is the maximum over m"; at H = 2 also against the chain of
//     csrc/step_lookahead.h (crash9 = depth 0, trap9 = depth 1): horizon_mask == ahead_mask.
// Prints the number of cases; exit status 1 on the first difference.
//
//     c++ -std=c++17 -fsanitize=address,undefined -I marl-responsible-nav_amd/csrc tools/step_horizon_check.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "step_horizon.h"
#include "step_lookahead.h"

namespace {

constexpr uint32_t ALL = 0x1FFu;
using step_horizon::CRASH;
using step_horizon::END;

struct Level {
    std::vector<uint32_t> mask;  // [node]
    std::vector<uint8_t> next;   // [node * 9 + b]
};

struct Table {
    int H;
    std::vector<uint8_t> first;  // [9]
    std::vector<Level> lv;       // lv[h], h = 1..H-1 (lv[0] unused)
};

uint32_t rng_state = 12345u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// include/gridenv.h, word for word: the largest d for which some continuation exists in which k does not crash in
// the steps 1..d; an episode end, the horizon, or a cell that allows nothing counts as H
int ref_after(const Table &t, int h, uint32_t code);
int ref_node(const Table &t, int h, uint32_t node) {
    const uint32_t m = t.lv[h].mask[node] & ALL;
    if (m == 0u) return t.H;
    int best = h;  // k has survived h steps
    for (int b = 0; b < 9; ++b)
        if ((m >> b) & 1u) {
            const int d = ref_after(t, h, t.lv[h].next[node * 9 + b]);
            if (d > best) best = d;
        }
    return best;
}
int ref_after(const Table &t, int h, uint32_t code) {
    if (code == CRASH) return h;      // k crashes in step h + 1
    if (code == END) return t.H;      // the episode ends without k's crash
    if (h + 1 == t.H) return t.H;     // the horizon is reached
    return ref_node(t, h + 1, code);
}

uint32_t mask_ref(bool has_mask, uint32_t m, const uint8_t *depth9) {
    const uint32_t mm = has_mask ? (m & ALL) : ALL;
    int top = -1;
    for (int a = 0; a < 9; ++a)
        if (((mm >> a) & 1u) && depth9[a] > top) top = depth9[a];
    uint32_t out = 0u;
    for (int a = 0; a < 9; ++a)
        if (((mm >> a) & 1u) && depth9[a] == top) out |= 1u << a;
    return out;
}

}  // namespace

int main() {
    long tables = 0, entries = 0, masks = 0, by_depth[5] = {0, 0, 0, 0, 0};
    for (int round = 0; round < 20000; ++round) {
        Table t;
        t.H = 2 + (int)(rnd() % 3u);
        t.lv.resize(t.H);
        std::vector<uint32_t> n(t.H + 1, 0u);
        for (int h = 1; h < t.H; ++h) n[h] = 1u + rnd() % 12u;
        auto code = [&](int h) -> uint8_t {  // a transition of step h + 1
            const uint32_t r = rnd() % 8u;
            if (r < 3u) return (uint8_t)CRASH;
            if (r == 3u) return (uint8_t)END;
            return (uint8_t)(h + 1 < t.H ? rnd() % n[h + 1] : rnd() % 200u);  // past the horizon: never looked up
        };
        t.first.resize(9);
        for (int a = 0; a < 9; ++a) t.first[a] = code(0);
        for (int h = 1; h < t.H; ++h) {
            t.lv[h].mask.resize(n[h]);
            t.lv[h].next.resize(n[h] * 9);
            for (uint32_t j = 0; j < n[h]; ++j) {
                const uint32_t r = rnd() % 6u;
                t.lv[h].mask[j] = (r == 0u ? 0u : r == 1u ? ALL : (rnd() & ALL)) | 0xFE00u;  // bits above the nine are ignored
                for (int b = 0; b < 9; ++b) t.lv[h].next[j * 9 + b] = code(h);
            }
        }
        // the kernel's fold: the deepest level first, exactly-sized rows on the heap
        std::vector<std::vector<uint8_t>> dep(t.H + 1);
        for (int h = t.H - 1; h >= 1; --h) {
            dep[h].resize(n[h]);
            for (uint32_t j = 0; j < n[h]; ++j)
                dep[h][j] = (uint8_t)step_horizon::node_depth(h, t.H, t.lv[h].mask[j], t.lv[h].next.data() + j * 9,
                                                              dep[h + 1].data());
        }
        std::vector<uint8_t> d9(9);
        for (int a = 0; a < 9; ++a) {
            d9[a] = (uint8_t)step_horizon::after(0, t.H, t.first[a], dep[1].data());
            const int want = ref_after(t, 0, t.first[a]);
            if ((int)d9[a] != want) {
                std::fprintf(stderr, "depth: round %d H %d a %d: got %d want %d\n", round, t.H, a, (int)d9[a], want);
                return 1;
            }
            ++by_depth[want];
            ++entries;
        }
        ++tables;
    }
    const uint32_t small[] = {0u, 1u, 0x100u, 0x00Au, 0x015u, 0x0F0u, 0x1FEu, ALL, 0xFFFFu};
    std::vector<uint8_t> d9(9);
    std::vector<uint16_t> mask2(9), crash2(9);
    for (int H = 2; H <= step_horizon::HORIZON_MAX; ++H) {
        long n = 1;
        for (int a = 0; a < 9; ++a) n *= H + 1;
        const int nm = H == 2 ? 9 : H == 3 ? 4 : 2;  // fewer masks where the tables are many
        for (long v = 0; v < n; ++v) {
            long q = v;
            uint32_t want_viable = 0u, crash9 = 0u, trap9 = 0u;
            for (int a = 0; a < 9; ++a) {
                d9[a] = (uint8_t)(q % (H + 1));
                q /= H + 1;
                want_viable |= (uint32_t)(d9[a] == H) << a;
                crash9 |= (uint32_t)(d9[a] == 0) << a;
                trap9 |= (uint32_t)(d9[a] == 1) << a;
            }
            for (int mi = -1; mi < nm; ++mi) {
                const bool has_mask = mi >= 0;
                const uint32_t m = has_mask ? small[(mi * 7 + H) % 9] : 0x123u;  // no mask: whatever the word holds
                const step_horizon::Horizon r = step_horizon::rules(has_mask, m, H, d9.data());
                const uint32_t want = mask_ref(has_mask, m, d9.data());
                if (r.viable9 != want_viable || r.horizon_mask != want) {
                    std::fprintf(stderr, "mask: H %d table %ld has_mask %d m %#x: got viable %#x mask %#x want %#x %#x\n", H,
                                 v, (int)has_mask, m, r.viable9, r.horizon_mask, want_viable, want);
                    return 1;
                }
                if (H == 2) {  // the lookahead's chain on rows that are traps where depth is 1
                    for (int a = 0; a < 9; ++a) {
                        const bool tr = (trap9 >> a) & 1u;
                        mask2[a] = (uint16_t)(tr ? 0x012u : ALL);
                        crash2[a] = (uint16_t)(tr ? 0x01Au : 0x010u);
                    }
                    const step_lookahead::Ahead la =
                        step_lookahead::rules(has_mask, m, crash9, crash9, mask2.data(), crash2.data());
                    if (la.trap9 != trap9 || la.ahead_mask != r.horizon_mask) {
                        std::fprintf(stderr, "H = 2: table %ld m %#x: ahead_mask %#x horizon_mask %#x\n", v, m, la.ahead_mask,
                                     r.horizon_mask);
                        return 1;
                    }
                }
                ++masks;
            }
        }
    }
    std::printf("%ld tables, %ld depth entries (%ld %ld %ld %ld %ld by depth), %ld mask cases\n", tables, entries,
                by_depth[0], by_depth[1], by_depth[2], by_depth[3], by_depth[4], masks);
    return (by_depth[0] > 0 && by_depth[1] > 0 && by_depth[2] > 0 && by_depth[3] > 0 && by_depth[4] > 0) ? 0 : 1;
}
