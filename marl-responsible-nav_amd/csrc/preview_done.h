// preview_done.h -- internal: what the kernels that look past the step about to run share (step_lookahead.hip,
// step_horizon.hip): the step's `done` rule for one world update and the wave-scope ordering of LDS.  Included
// inside namespace gw, after cf_env.h.
#pragma once

// Orders one wave's LDS accesses (shield_joint_core.h's rule restated: the LDS serves a wave's instructions in
// issue order, so it is enough to keep the compiler from moving an access across this point).
__device__ __forceinline__ void lookahead_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The step's `done` (finish_env, gridenv.hip; agent.py:241-243) restated for one world update, nothing stored:
// all terminated, or all truncated, or the step cap.  flags: the env's apples | term << 8 | trunc << 16 before
// the step; caught / crash: simulate's; t: the env's step count before the step.
__device__ __forceinline__ bool preview_done(const Params &p, int K, uint32_t flags, uint32_t caught, uint32_t crash,
                                             int t) {
    const bool single = p.variant == 1;
    uint32_t apples = flags & 0xFFu, term = (flags >> 8) & 0xFFu, trunc = (flags >> 16) & 0xFFu;
    const uint32_t allk = (1u << K) - 1u;
    const uint32_t popped = single ? (((caught >> 8) == 1u) ? (caught & apples & 1u) : 0u) : (caught & apples & 0xFFu);
    apples &= ~popped;
    if (popped && apples == 0u) trunc = single ? (trunc | 1u) : allk;  // all eaten
    const uint32_t own = crash & allk;                                  // the RL agents that crash
    if (own) {
        term |= own;
        if (!single) trunc = allk;  // any RL crash truncates every agent (ma_customenv.py:281-285)
    }
    return ((term & allk) == allk) || ((trunc & allk) == allk) || (p.max_steps > 0 && t + 1 >= p.max_steps);
}
