// preview_reward.h -- internal: the env reward of one world update for one RL agent, shared by the kernels that
// price a step without running it (step_preview.hip, step_plan.hip).  Included inside namespace gw, after cf_env.h.
#pragma once

// The env reward gw_step_out.reward[e][k] of one world update for the single RL agent k: finish_env's
// arithmetic (gridenv.hip; ma_customenv.py:258-302, customenv.py:127-160) restated for one agent, nothing stored.
// apples: the env's apples still present; caught: simulate's; apple_k: k's apple cell; prev: the env's
// prev_dist of k.
__device__ __forceinline__ double preview_reward(const Params &p, int k, uint32_t apples, uint32_t caught,
                                                 uint32_t crash, int fin_k, int apple_k, int prev) {
    const bool single = p.variant == 1;
    const uint32_t popped = single ? (((caught >> 8) == 1u) ? (caught & apples & 1u) : 0u) : (caught & apples & 0xFFu);
    apples &= ~popped;
    int rew = 0;
    if ((popped >> k) & 1u) rew += 20;                   // the own apple, once
    if (popped && apples == 0u && !single) rew += 20;    // all eaten
    if ((crash >> k) & 1u) rew -= 10;
    bool bonus = false;
    if (single) {  // distance to the apple cell, eaten or not
        bonus = manhattan(p, fin_k, apple_k) < prev;
    } else {
        const int d = ((apples >> k) & 1u) ? manhattan(p, fin_k, apple_k) : -1;
        if (prev >= 0 && d >= 0 && prev > d) rew += 1;
    }
    return bonus ? __dadd_rn((double)rew, 0.1) : (double)rew;
}

// The apples the step pops (finish_env's and preview_reward's rule): apples: the env's apples still present;
// caught: simulate's
__device__ __forceinline__ uint32_t preview_popped(const Params &p, uint32_t apples, uint32_t caught) {
    return p.variant == 1 ? (((caught >> 8) == 1u) ? (caught & apples & 1u) : 0u) : (caught & apples & 0xFFu);
}
