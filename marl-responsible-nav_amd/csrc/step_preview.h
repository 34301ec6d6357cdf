// step_preview.h -- the safe-mask rule of gw_step_preview (csrc/step_preview.hip, include/gridenv.h).
//
// A pure function, host and device, so that the kernel and a stand-alone CPU program
// (tools/step_preview_check.cpp) run the same text.  One RL agent of one env: its 9-bit action mask m (has_mask
// false: no mask was given, all nine) and crash9, bit a set when the agent itself crashes under action a while
// everybody else plays the action the step will apply.
//   safe = m & ~crash9
//   safe empty:   m unchanged (nothing avoids the crash, so nothing is taken away; m == 0 stays 0).
// The preview is unilateral, as gw_fear_shield's rows are: crash9 assumes that the OTHER agents play their
// proposed actions, so a pick from the safe mask is crash-free only where the others' actions were kept.
#ifndef STEP_PREVIEW_H
#define STEP_PREVIEW_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SP_HD __host__ __device__ __forceinline__
#else
#define SP_HD inline
#endif

namespace step_preview {

constexpr uint32_t ALL = 0x1FFu;  // GW_N_ACTIONS = 9 bits

SP_HD uint32_t safe_mask(bool has_mask, uint32_t m, uint32_t crash9) {
    m = has_mask ? (m & ALL) : ALL;
    const uint32_t safe = m & ~crash9;
    return safe ? safe : m;
}

}  // namespace step_preview
#endif  // STEP_PREVIEW_H
