// step_lookahead_check.cpp -- stand-alone host program around the trap and mask rules of gw_step_lookahead
// (csrc/step_lookahead.h, the text the kernel runs), for tests/test_step_lookahead_cpu.py, which builds it with
// AddressSanitizer + UBSan.  It compares the rules with a plain restatement of include/gridenv.h's wording:
//   traps: one first action at a time, every (ends bit, mask2, crash2) of 2 x 2^9 x 2^9, at each of the nine
//     bit positions (the other eight entries hold a pattern that is no trap);
//   mask:  every (crash9, trap9) of 2^9 x 2^9 under no mask and under a set of small masks, the trap sets made
//     from rows that are traps or not.
// Prints the number of cases and of traps / fall-backs seen; exit status 1 on the first difference.
//
//     c++ -std=c++17 -fsanitize=address,undefined -I marl-responsible-nav_amd/csrc tools/step_lookahead_check.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "step_lookahead.h"

namespace {

constexpr uint32_t ALL = 0x1FFu;

// include/gridenv.h, word for word
bool trap_ref(bool ends, uint32_t mask2, uint32_t crash2) {
    if (ends) return false;          // the step does not end under a,
    if (mask2 == 0u) return false;   // mask2 != 0,
    for (int b = 0; b < 9; ++b)      // every action the cell allows crashes k
        if (((mask2 >> b) & 1u) && !((crash2 >> b) & 1u)) return false;
    return true;
}

uint32_t ahead_ref(bool has_mask, uint32_t m, uint32_t crash9, uint32_t trap9) {
    const uint32_t mm = has_mask ? (m & ALL) : ALL;
    uint32_t out = 0u;
    for (int a = 0; a < 9; ++a)
        if (((mm >> a) & 1u) && !((crash9 >> a) & 1u) && !((trap9 >> a) & 1u)) out |= 1u << a;
    if (out) return out;
    for (int a = 0; a < 9; ++a)  // the preview's safe mask
        if (((mm >> a) & 1u) && !((crash9 >> a) & 1u)) out |= 1u << a;
    return out ? out : mm;
}

}  // namespace

int main() {
    long cases = 0, traps = 0, fell_back = 0, shrunk = 0;
    // exactly nine entries each, on the heap: a read past a row is an AddressSanitizer error
    std::vector<uint16_t> mask2(9), crash2(9);
    for (int a = 0; a < 9; ++a)
        for (uint32_t ends_bit = 0; ends_bit < 2; ++ends_bit)
            for (uint32_t m2 = 0; m2 <= ALL; ++m2)
                for (uint32_t c2 = 0; c2 <= ALL; ++c2) {
                    for (int q = 0; q < 9; ++q) {
                        mask2[q] = (uint16_t)ALL;  // allowed and crash-free: no trap
                        crash2[q] = 0;
                    }
                    mask2[a] = (uint16_t)(m2 | 0xFE00u);  // bits above the nine are ignored
                    crash2[a] = (uint16_t)c2;
                    const step_lookahead::Ahead r = step_lookahead::rules(false, 0u, 0u, ends_bit << a, mask2.data(),
                                                                          crash2.data());
                    const uint32_t want = (uint32_t)trap_ref(ends_bit != 0, m2, c2) << a;
                    if (r.trap9 != want) {
                        std::fprintf(stderr, "trap: a %d ends %u mask2 %#x crash2 %#x: got %#x want %#x\n", a, ends_bit,
                                     m2, c2, r.trap9, want);
                        return 1;
                    }
                    traps += want != 0u;
                    ++cases;
                }
    const uint32_t masks[] = {0u, 1u, 2u, 0x100u, 0x00Au, 0x015u, 0x0F0u, 0x1FEu, ALL, 0xFFFFu};
    for (int mi = -1; mi < (int)(sizeof(masks) / sizeof(masks[0])); ++mi) {
        const bool has_mask = mi >= 0;
        const uint32_t m = has_mask ? masks[mi] : 0x123u;  // no mask: whatever the word holds
        for (uint32_t crash9 = 0; crash9 <= ALL; ++crash9)
            for (uint32_t trap9 = 0; trap9 <= ALL; ++trap9) {
                for (int q = 0; q < 9; ++q) {  // a row that is a trap where trap9 says so
                    const bool tr = (trap9 >> q) & 1u;
                    mask2[q] = (uint16_t)(tr ? 0x012u : ALL);
                    crash2[q] = (uint16_t)(tr ? 0x01Au : 0x010u);
                }
                const step_lookahead::Ahead r = step_lookahead::rules(has_mask, m, crash9, 0u, mask2.data(), crash2.data());
                const uint32_t want = ahead_ref(has_mask, m, crash9, trap9);
                if (r.trap9 != trap9 || r.ahead_mask != want) {
                    std::fprintf(stderr, "mask: has_mask %d m %#x crash9 %#x trap9 %#x: got trap9 %#x ahead %#x want %#x\n",
                                 (int)has_mask, m, crash9, trap9, r.trap9, r.ahead_mask, want);
                    return 1;
                }
                const uint32_t mm = has_mask ? (m & ALL) : ALL;
                fell_back += mm != 0u && (mm & ~crash9 & ~trap9) == 0u;
                shrunk += want != mm;
                ++cases;
            }
    }
    std::printf("%ld cases, %ld traps, %ld fall-backs, %ld masks shrunk\n", cases, traps, fell_back, shrunk);
    return (traps > 0 && fell_back > 0 && shrunk > 0) ? 0 : 1;
}
