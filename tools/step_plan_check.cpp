// step_plan_check.cpp -- stand-alone host program around the depth, return, path and mask rules of gw_step_plan
// (csrc/step_plan.h, the text the kernel runs), for tests/test_step_plan_cpu.py, which builds it with
// AddressSanitizer + UBSan.  It compares the rules with a plain restatement of include/gridenv.h's wording:
//   recursion and ties: random transition tables (H = 2..4, up to 12 nodes per level, masks with and without holes,
//     empty masks, every transition code, eat and last bits, rewards in tenths), folded level by level as the
//     kernel folds them (two depths, one return and two links per node), against a depth-first search over the
//     same table whose state is (node, is the apple still there), with no memoisation: depth, return and the whole
//     path of every first action;
//   mask: random (depth, return) tables under no mask and under random masks against "the actions of m whose
//     (depth, ret) is the lexicographic maximum over m", and plan_mask within step_horizon::rules' horizon_mask.
// Prints the number of cases; exit status 1 on the first difference.
//
//     c++ -std=c++17 -fsanitize=address,undefined -I marl-responsible-nav_amd/csrc tools/step_plan_check.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "step_plan.h"

namespace {

constexpr uint32_t ALL = 0x1FFu;
using step_plan::CRASH;
using step_plan::END;
using step_plan::Tr;

struct Level {
    std::vector<uint32_t> mask;  // [node]
    std::vector<uint32_t> next;  // [node * 9 + b]: packed transitions
};

struct Table {
    int H;
    std::vector<uint32_t> first;  // [9]: packed; eat = the apple is not there after step 1
    std::vector<Level> lv;        // lv[h], h = 1..H-1 (lv[0] unused)
};

uint32_t rng_state = 2468u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

struct Res {
    int d, r;
    std::vector<int> path;
};

long eats = 0, lasts = 0;  // on the best continuations

// include/gridenv.h, word for word: continuations ordered by (depth, return); a continuation stops at k's crash
// (which it includes), at an episode end, at the horizon and in a cell that allows nothing; without its apple k
// earns nothing but its crash
Res ref_node(const Table &t, int h, uint32_t node, bool present, bool count);
Res ref_after(const Table &t, int h, const Tr &tr, bool present, bool count) {
    const int rw = present ? tr.rw : (tr.code == CRASH ? -100 : 0);
    if (tr.code == CRASH) return Res{h, rw, {}};
    if (present && tr.last) {
        lasts += count;
        eats += count && tr.eat;
        return Res{t.H, rw, {}};
    }
    eats += count && present && tr.eat;
    if (tr.code == END || h + 1 == t.H) return Res{t.H, rw, {}};
    Res n = ref_node(t, h + 1, tr.code, present && !tr.eat, count);
    n.r += rw;
    return n;
}
Res ref_node(const Table &t, int h, uint32_t node, bool present, bool count) {
    const uint32_t m = t.lv[h].mask[node] & ALL;
    if (m == 0u) return Res{t.H, 0, {}};
    Res best{-1, 0, {}};
    int best_b = -1;
    for (int b = 0; b < 9; ++b)
        if ((m >> b) & 1u) {
            const Res v = ref_after(t, h, step_plan::unpack(t.lv[h].next[node * 9 + b]), present, false);
            if (best_b < 0 || v.d > best.d || (v.d == best.d && v.r > best.r)) best = v, best_b = b;
        }
    if (count) best = ref_after(t, h, step_plan::unpack(t.lv[h].next[node * 9 + best_b]), present, true);
    best.path.insert(best.path.begin(), best_b);
    return best;
}

struct Deeper {
    const std::vector<uint8_t> &v0, &v1;
    const std::vector<int16_t> &vr;
    uint32_t d0(uint32_t c) const { return v0.at(c); }
    uint32_t d1(uint32_t c) const { return v1.at(c); }
    int32_t r1(uint32_t c) const { return vr.at(c); }
};

uint32_t mask_ref(bool has_mask, uint32_t m, const int *d9, const int *r9) {
    const uint32_t mm = has_mask ? (m & ALL) : ALL;
    int a0 = -1;
    for (int a = 0; a < 9; ++a)
        if (((mm >> a) & 1u) && (a0 < 0 || d9[a] > d9[a0] || (d9[a] == d9[a0] && r9[a] > r9[a0]))) a0 = a;
    uint32_t out = 0u;
    for (int a = 0; a < 9 && a0 >= 0; ++a)
        if (((mm >> a) & 1u) && d9[a] == d9[a0] && r9[a] == r9[a0]) out |= 1u << a;
    return out;
}

}  // namespace

int main() {
    long tables = 0, entries = 0, masks = 0, strict = 0, by_depth[5] = {0, 0, 0, 0, 0}, path_len[4] = {0, 0, 0, 0};
    const int rewards[] = {0, 0, 0, 10, 1, -100, 200, 210, 400, 410, 100, 201};
    for (int round = 0; round < 20000; ++round) {
        Table t;
        t.H = 2 + (int)(rnd() % 3u);
        t.lv.resize(t.H);
        std::vector<uint32_t> n(t.H + 1, 0u);
        for (int h = 1; h < t.H; ++h) n[h] = 1u + rnd() % 12u;
        auto trans = [&](int h) -> uint32_t {  // a transition of step h + 1
            Tr tr;
            const uint32_t r = rnd() % 8u;
            tr.code = r < 3u ? CRASH : r == 3u ? END : (h + 1 < t.H ? rnd() % n[h + 1] : rnd() % 200u);
            tr.eat = rnd() % 4u == 0u;
            tr.last = h > 0 && tr.eat && tr.code < END && rnd() % 2u == 0u;  // (the first step's END covers it)
            tr.rw = rewards[rnd() % 12u] + (tr.code == CRASH ? -100 : 0);
            return step_plan::pack(tr);
        };
        t.first.resize(9);
        for (int a = 0; a < 9; ++a) t.first[a] = trans(0);
        for (int h = 1; h < t.H; ++h) {
            t.lv[h].mask.resize(n[h]);
            t.lv[h].next.resize(n[h] * 9);
            for (uint32_t j = 0; j < n[h]; ++j) {
                const uint32_t r = rnd() % 6u;
                t.lv[h].mask[j] = (r == 0u ? 0u : r == 1u ? ALL : (rnd() & ALL)) | 0xFE00u;  // bits above the nine are ignored
                for (int b = 0; b < 9; ++b) t.lv[h].next[j * 9 + b] = trans(h);
            }
        }
        // the kernel's fold: the deepest level first, exactly-sized rows on the heap
        std::vector<std::vector<uint8_t>> d0(t.H + 1), d1(t.H + 1);
        std::vector<std::vector<int16_t>> r1(t.H + 1);
        std::vector<std::vector<uint16_t>> lk(t.H + 1);  // [h][node * 2 + world]
        for (int h = t.H - 1; h >= 1; --h) {
            d0[h].resize(n[h]), d1[h].resize(n[h]), r1[h].resize(n[h]), lk[h].resize(2 * n[h]);
            for (uint32_t j = 0; j < n[h]; ++j) {
                const step_plan::Node nd = step_plan::node(h, t.H, t.lv[h].mask[j], t.lv[h].next.data() + j * 9,
                                                           Deeper{d0[h + 1], d1[h + 1], r1[h + 1]});
                d0[h][j] = (uint8_t)nd.d0, d1[h][j] = (uint8_t)nd.d1, r1[h][j] = (int16_t)nd.r1;
                lk[h][2 * j] = (uint16_t)nd.l0, lk[h][2 * j + 1] = (uint16_t)nd.l1;
            }
        }
        auto links = [&](int h, uint32_t node, bool present) -> uint32_t { return lk.at(h).at(2 * node + (present ? 1 : 0)); };
        for (int a = 0; a < 9; ++a) {
            const Tr tr = step_plan::unpack(t.first[a]);
            const step_plan::Val v = step_plan::after1(0, t.H, tr, Deeper{d0[1], d1[1], r1[1]});
            const uint32_t pth = step_plan::path(t.H, tr, links);
            // the first step is priced with the apple's state before it: its reward is tr.rw as it stands
            Res want;
            if (tr.code == CRASH) want = Res{0, tr.rw, {}};
            else if (tr.code == END) want = Res{t.H, tr.rw, {}};
            else {
                want = ref_node(t, 1, tr.code, !tr.eat, true);
                want.r += tr.rw;
            }
            uint32_t want_pth = step_plan::NO_PATH;
            for (size_t i = 0; i < want.path.size(); ++i)
                want_pth = (want_pth & ~(0xFFu << (8 * i))) | ((uint32_t)want.path[i] << (8 * i));
            if ((int)v.depth != want.d || v.ret != want.r || pth != want_pth) {
                std::fprintf(stderr, "round %d H %d a %d: got (%u, %d, %#x) want (%d, %d, %#x)\n", round, t.H, a, v.depth,
                             v.ret, pth, want.d, want.r, want_pth);
                return 1;
            }
            if (want.d < t.H && want.path.size() != (size_t)want.d) {  // the crash step is the path's last entry
                std::fprintf(stderr, "round %d a %d: depth %d with a path of %zu\n", round, a, want.d, want.path.size());
                return 1;
            }
            ++by_depth[want.d];
            ++path_len[want.path.size()];
            ++entries;
        }
        ++tables;
    }
    for (int round = 0; round < 200000; ++round) {
        const int H = 2 + (int)(rnd() % 3u);
        int d9[9], r9[9];
        uint8_t du[9];
        for (int a = 0; a < 9; ++a) {
            d9[a] = (int)(rnd() % (uint32_t)(H + 1));
            du[a] = (uint8_t)d9[a];
            r9[a] = rewards[rnd() % 12u] - (d9[a] < H ? 100 : 0);
        }
        const bool has_mask = rnd() % 4u != 0u;
        const uint32_t m = (rnd() % 8u == 0u ? 0u : rnd() & 0xFFFFu);
        const uint32_t got = step_plan::plan_mask(has_mask, m, d9, r9), want = mask_ref(has_mask, m, d9, r9);
        const uint32_t hm = step_horizon::rules(has_mask, m, H, du).horizon_mask;
        if (got != want || (got & ~hm) != 0u || (got == 0u) != (hm == 0u)) {
            std::fprintf(stderr, "mask: round %d has_mask %d m %#x: got %#x want %#x horizon_mask %#x\n", round,
                         (int)has_mask, m, got, want, hm);
            return 1;
        }
        strict += got != hm;
        ++masks;
    }
    std::printf("%ld tables, %ld entries (%ld %ld %ld %ld %ld by depth, %ld %ld %ld %ld by path length), %ld eats, %ld last "
                "apples, %ld mask cases (%ld strict subsets)\n",
                tables, entries, by_depth[0], by_depth[1], by_depth[2], by_depth[3], by_depth[4], path_len[0], path_len[1],
                path_len[2], path_len[3], eats, lasts, masks, strict);
    bool ok = eats > 0 && lasts > 0 && strict > 0;
    for (int i = 0; i < 5; ++i) ok = ok && by_depth[i] > 0;
    for (int i = 0; i < 4; ++i) ok = ok && path_len[i] > 0;
    return ok ? 0 : 1;
}
