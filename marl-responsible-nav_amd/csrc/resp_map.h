// resp_map.h -- the bin rule of gw_resp_map_accum (csrc/resp_map.hip, include/rollout_ops.h).
//
// A pure function, host and device, so that the kernel and a stand-alone CPU program
// (tools/resp_map_check.cpp) run the same text.  One ordered pair (actor i, affected agent j != i) of one
// env: the 4-byte word fear_full_kernel stored for it (csrc/fear_full.hip: vm_set | va_set << 16, i.e.
// resp_valid[e][i][j][0] = the 9-bit set with the actor on its MdR in the low half, [1] = the set under
// the actual actions in the high half), the two agents' pre-move cells and the map size HW.
//   vm = popc(low half & 0x1FF), va = popc(high half & 0x1FF)      (each 0..9: Resp = T[vm][va])
//   caused   = ((0 * HW + cell_i) * 10 + vm) * 10 + va              (plane 0: the actor's cell)
//   received = ((1 * HW + cell_j) * 10 + vm) * 10 + va              (plane 1: the affected agent's cell)
// Every cell is clamped to [0, HW) and every count to [0, 9] before it indexes anything, so both indices lie
// in [0, 2 * HW * 100) whatever the inputs hold (HW >= 1).
#ifndef RESP_MAP_H
#define RESP_MAP_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RM_HD __host__ __device__ __forceinline__
#else
#define RM_HD inline
#endif

namespace resp_map {

constexpr int NV = 10;  // valid-action counts 0..9 (GW_N_ACTIONS + 1)

struct Bins {
    int64_t caused;    // into counts[0][cell_i][vm][va]
    int64_t received;  // into counts[1][cell_j][vm][va]
};

RM_HD int clamp_cell(int32_t c, int32_t HW) { return c < 0 ? 0 : (c >= HW ? HW - 1 : c); }

RM_HD int count9(uint32_t set) {
    const int n = __builtin_popcount(set & 0x1FFu);
    return n > NV - 1 ? NV - 1 : n;  // (nine bits: never taken; the clamp the index relies on)
}

RM_HD Bins bins(uint32_t word, int32_t cell_i, int32_t cell_j, int32_t HW) {
    const int vm = count9(word), va = count9(word >> 16);
    const int64_t v = vm * NV + va;
    Bins b;
    b.caused = (int64_t)clamp_cell(cell_i, HW) * (NV * NV) + v;
    b.received = ((int64_t)HW + clamp_cell(cell_j, HW)) * (NV * NV) + v;
    return b;
}

}  // namespace resp_map
#endif  // RESP_MAP_H
