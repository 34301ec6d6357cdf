// resp_footprint.h -- the bin rule of gw_resp_footprint_accum (csrc/resp_footprint.hip, include/rollout_ops.h).
//
// A pure function, host and device, so that the kernel and a stand-alone CPU program
// (tools/resp_footprint_check.cpp) run the same text.  One ordered pair (actor i, affected agent j != i) of one
// env: the pair's 4-byte resp_valid word (resp_map.h's meaning: vm's set in the low half, va's in the high
// half), the two agents' pre-move cells, the actor's action in the step, the map width W, the map size HW and
// the radius R of the near window.
//   vm = count9(low half), va = count9(high half)                   (each 0..9: Resp = T[vm][va])
//   a  = a_i if 0 <= a_i <= 8, else 0                               (as the step reads an action)
//   dr = cell_j / W - cell_i / W,  dc = cell_j % W - cell_i % W     (both cells clamped to [0, HW) first)
//   o  = (dr + R) * (2R + 1) + (dc + R)   if |dr| <= R and |dc| <= R,   else (2R + 1)^2, the far bin
//   O  = (2R + 1)^2 + 1
//   bin = ((a * O + o) * 10 + vm) * 10 + va
// which lies in [0, 9 * O * 100) whatever the word, the cells and the action hold (W >= 1, HW >= 1, R >= 0).
#ifndef RESP_FOOTPRINT_H
#define RESP_FOOTPRINT_H
#include <stdint.h>

#include "resp_map.h"

namespace resp_footprint {

constexpr int NV = resp_map::NV;
constexpr int NA = 9;  // actions 0..8 (GW_N_ACTIONS)

RM_HD int offsets(int32_t R) { return (2 * R + 1) * (2 * R + 1) + 1; }  // O: the near window and the far bin

RM_HD int action9(int32_t a) { return a < 0 || a > NA - 1 ? 0 : a; }

RM_HD int offset_bin(int32_t cell_i, int32_t cell_j, int32_t W, int32_t HW, int32_t R) {
    const int ci = resp_map::clamp_cell(cell_i, HW), cj = resp_map::clamp_cell(cell_j, HW);
    const int dr = cj / W - ci / W, dc = cj % W - ci % W;  // (non-negative operands: plain division)
    const int S = 2 * R + 1;
    if (dr < -R || dr > R || dc < -R || dc > R) return S * S;
    return (dr + R) * S + (dc + R);
}

RM_HD int64_t bin(uint32_t word, int32_t cell_i, int32_t cell_j, int32_t a_i, int32_t W, int32_t HW, int32_t R) {
    const int vm = resp_map::count9(word), va = resp_map::count9(word >> 16);
    const int64_t ao = (int64_t)action9(a_i) * offsets(R) + offset_bin(cell_i, cell_j, W, HW, R);
    return (ao * NV + vm) * NV + va;
}

}  // namespace resp_footprint
#endif  // RESP_FOOTPRINT_H
