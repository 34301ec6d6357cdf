// desc_rows.h -- internal: the one statement of how a 48-byte obs descriptor expands to the patched cells
// of an observation, shared by the replay ring's descriptor samplers: rollout_ops.hip (full-grid rows,
// replay_gather_desc_kernel) and replay_patch.hip (P x P window rows, replay_gather_desc_patch_kernel).
// The text stood in rollout_ops.hip; every includer gets its own internal copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gridenv.h"
#include "obs_value.h"

namespace {

// ---- replay-ring sample from the descriptor ring: the same rows, expanded from 48-byte obs
// descriptors instead of read from the dense obs slots (so the learner never waits for the obs
// writer of the step it follows).  The cell values restate the obs writer (gridenv.hip obs_block;
// ma_customenv.py:197-209 reset encoding, :303-322 step encoding): map 0 / -1, own apple
// +9 first, then agent n's cell (a later patch overrides an earlier one) ----
constexpr int DESC_WORDS = 12;  // gridenv.hip NDESC
constexpr uint32_t DF_RESET = 1u;

struct DescSrc {
    const float *base;
    int apples[GW_MAX_AGENTS];
    int N, K, HW, variant;
    int64_t E;
};

// patches of (descriptor words d[0..11], agent k): which 0 = the obs, 1 = the terminal obs (words
// 8-11); apple_map = the map value under agent k's apple cell
__device__ __forceinline__ int desc_patches(const DescSrc &q, const uint32_t (&d)[DESC_WORDS], int which, int k,
                                            float apple_map, int *pc, float *pv) {
    const uint32_t f = d[4];
    const bool reset = which == 0 && (f & DF_RESET);
    const uint32_t apples = which == 0 ? (f >> 8) & 0xFFu : (f >> 16) & 0xFFu;
    const int ac = ((apples >> k) & 1u) ? q.apples[k] : -1;
    int np = 0;
    if (ac >= 0) {
        float av = apple_map + 9.0f;
        if (!reset && av == (float)(k + 1)) av = 1.0f;
        pc[np] = ac;
        pv[np] = av;
        ++np;
    }
    for (int n = 0; n < q.N; ++n) {
        const uint32_t w = which == 0 ? d[n >> 1] : d[8 + (n >> 1)];
        const int c = (int)((w >> (16 * (n & 1))) & 0xFFFFu);
        pc[np] = c;
        pv[np] = gwobs::agent_value(reset, n, k, c == ac, q.variant);
        ++np;
    }
    return np;
}

}  // namespace
