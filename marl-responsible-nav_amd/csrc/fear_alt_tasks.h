// fear_alt_tasks.h — task-list arithmetic of the per-action FeAR table (csrc/fear_alt_core.h: fear_alt_kernel in
// fear_cf.hip, fear_shield_joint_kernel in fear_shield_joint.hip).
//
// Pure integer functions, host and device, so that a stand-alone CPU program can check them
// (tools/fear_alt_tasks_check.cpp).  Per env and RL actor k with close count c (k included), the
// counterfactual world updates of the [9] table row are
//     t = a * S(c) + s,   a = k's action variant 0..8,   S(c) = 1 + 8 (c - 1),
//     s = 0            the base sim of variant a (nobody else changed),
//     s = 1 + 8 q + bi the bi-th alternative (the 8 actions b != act[j]) of the q-th close agent j != k.
// The tasks of an env's actors follow each other (actor 0's, then actor 1's, ...) and are dealt to
// the 64 lanes of the env's wave round-robin: lane = (a, j, b).
#ifndef FEAR_ALT_TASKS_H
#define FEAR_ALT_TASKS_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FA_HD __host__ __device__ __forceinline__
#else
#define FA_HD inline
#endif

namespace fear_alt {

constexpr int NA = 9;  // GW_N_ACTIONS

// sims of one actor variant / of one actor, close count c in 1..N (the actor itself included)
FA_HD constexpr int per_variant(int c) { return 1 + (NA - 1) * (c - 1); }
FA_HD constexpr int per_actor(int c) { return NA * per_variant(c); }
// the most sims an env can need: every actor close to everybody
FA_HD constexpr int max_per_env(int N, int K) { return K * per_actor(N); }
// u32 words of an env's valid-move bit sets: [K][9 variants][N affected], 9 bits used per word
FA_HD constexpr int bit_words(int N, int K) { return K * NA * N; }

struct Task {
    int a;     // the actor's action variant, 0..8
    int slot;  // -1: base sim; else index into the actor's close agents (itself excluded), 0..c-2
    int bi;    // alternative index 0..7 of that agent (valid with slot >= 0)
};

// task r in [0, per_actor(c)) of an actor with close count c (clamped to the last task)
FA_HD Task decode(int r, int c) {
    const int S = per_variant(c);
    const int last = NA * S - 1;
    r = r < 0 ? 0 : (r > last ? last : r);
    Task t;
    t.a = r / S;
    const int s = r - t.a * S;
    t.slot = s == 0 ? -1 : (s - 1) >> 3;
    t.bi = s == 0 ? 0 : (s - 1) & 7;
    return t;
}

FA_HD constexpr int encode(int a, int slot, int bi, int c) {
    return a * per_variant(c) + (slot < 0 ? 0 : 1 + 8 * slot + bi);
}

struct Actor {
    int k;  // the actor
    int r;  // its task, 0..tcount[k]-1
};

// task ti of a run over the actors in `sel`, whose tasks follow each other in ascending actor order (tcount[q]
// tasks of actor q): the actor and its task.  ti at or past the selected total: actor N - 1 with r past its last
// task (decode clamps it), so every index built from the result stays in range.  N - 1 steps, no bound read from data
template <int N>
FA_HD Actor actor_of(uint32_t sel, const int (&tcount)[N], int ti) {
    Actor t{0, ti};
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int q = 0; q < N - 1; ++q) {  // k moves on past q while the task lies behind q's (none if q is not selected)
        const int tc = ((sel >> q) & 1u) ? tcount[q] : 0;
        if (q == t.k && t.r >= tc) {
            t.r -= tc;
            ++t.k;
        }
    }
    return t;
}

// the bi-th action other than `own` (0..8): the 8 alternatives in ascending order
FA_HD constexpr int alternative(int bi, int own) { return bi + (bi >= own ? 1 : 0); }

// the slot-th (0-based) set bit of `others` (the close set without the actor), or -1 if there
// are fewer: at most 7 steps, no loop bound read from data
FA_HD int nth_agent(uint32_t others, int slot) {
    others &= 0xFFu;
    for (int i = 0; i < 7; ++i)
        if (i < slot) others &= others - 1u;
    if (!others) return -1;
    int j = 0;
    while (!((others >> j) & 1u)) ++j;  // others != 0, bits 0-7 only: j <= 7
    return j;
}

}  // namespace fear_alt
#endif  // FEAR_ALT_TASKS_H
