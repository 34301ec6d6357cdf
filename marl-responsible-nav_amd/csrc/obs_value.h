// obs_value.h — internal: the observation encoding's one agent-cell rule, shared by the obs writer
// (gridenv.hip), the window writers (patch_ops.hip, window_rows.h), the fused actors (actor_ops.hip)
// and the descriptor learner's samplers (rollout_ops.hip, maddpg_desc.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace gwobs {

// obs value of agent n's cell in RL agent k's observation: ma_customenv.py:197-209 reset encoding
// (0.5 at agents, +9 on the own apple), :303-322 step encoding (agent n -> n + 1, +9 on its apple,
// then the relabel)
__device__ __forceinline__ float agent_value(bool reset, int n, int k, bool on_apple, int variant) {
    if (reset) return on_apple ? 9.5f : 0.5f;
    if (on_apple) return (float)(n + 1 + 9);
    if (variant == 1) return (float)(n + 1);  // customenv.py:163-166: raw WorldState ids
    int v = n + 1;
    if (v >= 1 && v <= 4 && v != k + 1) v = 5;   // other ids -> 5 (all_ids = [1,2,3,4], :314)
    if (v == k + 1) v = 1;                        // my id -> 1 (:321)
    return (float)v;
}

}  // namespace gwobs
