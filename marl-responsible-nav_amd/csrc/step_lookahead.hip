// step_lookahead.hip -- step_lookahead_kernel (gw_step_lookahead): the two-step crash lookahead.  For each RL agent k
// and first action a the real world update of the step about to run (gw_step_preview's task), whether that step
// ends the episode, and, where it does not, the nine real world updates of the step after it from the cells the
// first one left: k playing b, the other RL agents staying, the scripted agents' Philox draws of step t + 1
// recomputed from their new cells.  From these the trap actions and the lookahead mask (step_lookahead.h).
// A translation unit of its own on the shared headers (cf_env.h, draw_action.h), so that the code object of
// gridenv.hip's step kernels does not change with it; gridenv.hip runs this kernel right behind
// preview_rec_kernel (fear_preview.hip) on gw_step_preview's record buffer.
#include <hip/hip_runtime.h>

#include "cf_env.h"
#include "dispatch.h"
#include "philox.h"
#include "prof.h"
#include "step_lookahead.h"

namespace gw {

#include "draw_action.h"
#include "preview_done.h"

// gw_step_lookahead's action masks after the first step, as step_lookahead::rules reads them: entry a is the cell
// table's action-mask bits of agent k's cell in the world (k, a)
template <int N>
struct Mask2View {
    const uint16_t (*cells)[N];  // the wave's worlds of agent k: [9][N]
    const uint32_t *ctab;
    int k, HW;
    __device__ __forceinline__ uint32_t operator[](int a) const {
        const int cell = min((int)(cells[a][k] & 0xFFFu), HW - 1);
        return (ctab[cell] >> CT_AMASK) & step_lookahead::ALL;
    }
};

// ---------------------------------------------------------------------------------------
// step_lookahead_kernel (gw_step_lookahead) on the wave-per-env scaffold (CfEnv), from the record
// preview_rec_kernel built.  Per env (one wave), K <= N RL agents:
//   stage A: the K x 9 tasks (k, a) dealt round-robin (step_preview_kernel's task).  A task stores the final cells
//     of all N agents as u16 into cells[k * 9 + a][n] and ORs k's own crash bit into c9[k], the step's ends bit
//     into e9[k];
//   draws: one per (k, a, n >= K) whose step goes on: draw_action at step t + 1 from the agent's stage-A cell, the
//     Philox law always (a Params whose `scripted` is null), packed beside the cell: cell | action << 12 (a cell
//     needs 12 bits: H * W <= 4096; an action 4);
//   stage B: the K x 81 tasks (k, a, b) dealt round-robin; the tasks of an ending (k, a) are skipped.  A task reads
//     its world from LDS (cells and actions clamped), runs one world update (no apples: they cannot change who
//     crashes) with k playing b and the other RL agents 0 and ORs k's own crash bit into c2[k * 9 + a];
//   stores: lane (k, a) crash2; lane k crash9, ends, trap9 and ahead_mask (step_lookahead::rules).
// No wave-collective operation stands inside the task loops (their last turn and stage B's skipped tasks leave
// lanes idle; the wave reconverges before lookahead_lds_order() and end()); the four waves of a block are four envs with different numbers
// of skipped tasks: nothing between begin()'s barrier and end()'s is block-wide, a wave owns its rows of every
// array below and orders its own LDS accesses with lookahead_lds_order(); a wave past the env range has no task
// and goes straight to end().
// ---------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(CF_T) step_lookahead_kernel(Params p, StepLookaheadArgs a) {
    constexpr bool LIST = N >= GW_LIST_MIN_N;
    constexpr int NT = N * NA;                   // (k, a) pairs per env, sized for K = N
    __shared__ uint16_t cells[CF_WAVES][NT][N];  // [k * 9 + a][n]: n's cell after (k, a) | n >= K: its next action << 12
    __shared__ uint32_t c2[CF_WAVES][NT];        // [k * 9 + a]: bit b = k itself crashes in the second step under b
    __shared__ uint32_t c9[CF_WAVES][N];         // [k]: bit a = k itself crashes in the first step under a
    __shared__ uint32_t e9[CF_WAVES][N];         // [k]: bit a = the first step ends the episode under a
    __shared__ uint2 wl[LIST ? CF_T * N : 1];    // World<N, true> rows (one per thread)
    __shared__ unsigned int s_nsim;
    static_assert(sizeof(uint16_t) * CF_WAVES * NT * N + sizeof(uint32_t) * CF_WAVES * (NT + 2 * N) +
                          sizeof(uint2) * (LIST ? CF_T * N : 1) <= 23 * 1024,
                  "static LDS of step_lookahead_kernel");
    CfEnv<N> c;
    c.begin(p, 0, s_nsim, [&] {
        if (c.lane < N) c9[c.wave][c.lane] = e9[c.wave][c.lane] = 0u;
        for (int i = c.lane; i < NT; i += 64) c2[c.wave][i] = 0u;
    });
    const int tid = threadIdx.x, wave = c.wave, lane = c.lane, K = min(p.K, N);
    const CtabOk okv{c.ctab};
    const int ntask = c.live ? K * NA : 0;
    const uint32_t flags = c.live ? p.st.flags[c.e] : 0u;
    const int t = c.live ? p.st.t[c.e] : 0;
    const uint32_t episode = c.live ? p.st.episode[c.e] : 0u;
    uint2 *const wl_row = LIST ? &wl[tid * N] : nullptr;
    int apple[MAXN], no_apple[MAXN];
#pragma unroll
    for (int q = 0; q < MAXN; ++q) {
        apple[q] = (q < K && ((flags >> q) & 1u)) ? p.apples[q] : -1;
        no_apple[q] = -1;
    }

    // stage A: the step about to run under each (k, a)
    for (int ti = lane; ti < ntask; ti += 64) {
        const int k = ti / NA, b = ti - k * NA;  // k < K <= N
        int joint[N], fin[N];
#pragma unroll
        for (int n = 0; n < N; ++n) joint[n] = (n == k) ? b : c.act[n];
        World<N, LIST> w;
        w.init(c.pos, joint, p.W, p.w_magic);
        if constexpr (LIST) w.lw = wl_row;
        uint32_t caught;
        simulate<N, true>(w, okv, K, apple, caught, fin);
#pragma unroll
        for (int n = 0; n < N; ++n) cells[wave][ti][n] = (uint16_t)fin[n];
        if ((w.crash >> k) & 1u) atomicOr(&c9[wave][k], 1u << b);
        if (preview_done(p, K, flags, caught, w.crash, t)) atomicOr(&e9[wave][k], 1u << b);
    }
    lookahead_lds_order();
    int nlive = 0;  // the (k, a) whose step goes on (uniform: every lane reads the same words)
    for (int k = 0; k < K && ntask; ++k) nlive += __popc(~e9[wave][k] & step_lookahead::ALL);

    // the scripted agents' draws of step t + 1, once per (k, a, n)
    {
        Params p2 = p;
        p2.scripted = nullptr;  // a caller's override holds for the step about to run only
        const int nscr = N - K, ndraw = ntask * nscr;
        for (int i = lane; i < ndraw; i += 64) {
            const int ti = i / nscr, n = K + (i - ti * nscr);  // ndraw > 0: nscr >= 1; n in K..N-1
            const int k = ti / NA, a1 = ti - k * NA;
            if ((e9[wave][k] >> a1) & 1u) continue;
            const int cell = min((int)(cells[wave][ti][n] & 0xFFFu), p.HW - 1);
            const int act = draw_action(p2, c.e, n, episode, t + 1, cell, c.ctab, nullptr);  // in 0..8
            cells[wave][ti][n] = (uint16_t)((uint32_t)cell | ((uint32_t)act << 12));
        }
    }
    lookahead_lds_order();

    // stage B: the step after, under each (k, a, b)
    const int ntask2 = ntask * NA;
    for (int i = lane; i < ntask2; i += 64) {
        const int ti = i / NA, b = i - ti * NA;
        const int k = ti / NA, a1 = ti - k * NA;
        if ((e9[wave][k] >> a1) & 1u) continue;
        int pos[N], joint[N], fin[N];
#pragma unroll
        for (int n = 0; n < N; ++n) {
            const uint32_t v = cells[wave][ti][n];
            pos[n] = min((int)(v & 0xFFFu), p.HW - 1);
            const int drawn = min((int)(v >> 12), NA - 1);
            joint[n] = (n < K) ? ((n == k) ? b : 0) : drawn;
        }
        World<N, LIST> w;
        w.init(pos, joint, p.W, p.w_magic);
        if constexpr (LIST) w.lw = wl_row;
        uint32_t caught;
        simulate<N, false>(w, okv, 0, no_apple, caught, fin);
        if ((w.crash >> k) & 1u) atomicOr(&c2[wave][ti], 1u << b);
    }
    lookahead_lds_order();

    if (a.crash2)
        for (int ti = lane; ti < ntask; ti += 64)  // ti = k * 9 + a < 9 p.K
            a.crash2[c.e * p.K * NA + ti] = (uint16_t)(c2[wave][ti] & step_lookahead::ALL);
    if (c.live && lane < K) {
        const int64_t ek = c.e * p.K + lane;
        const uint32_t crash9 = c9[wave][lane] & step_lookahead::ALL, ends = e9[wave][lane] & step_lookahead::ALL;
        const Mask2View<N> mask2{&cells[wave][lane * NA], c.ctab, lane, p.HW};
        const step_lookahead::Ahead r =
            step_lookahead::rules(a.mask != nullptr, a.mask ? a.mask[ek] : 0u, crash9, ends, mask2, &c2[wave][lane * NA]);
        if (a.crash9) a.crash9[ek] = (uint16_t)crash9;
        if (a.ends) a.ends[ek] = (uint16_t)ends;
        if (a.trap9) a.trap9[ek] = (uint16_t)r.trap9;
        if (a.ahead_mask) a.ahead_mask[ek] = (uint16_t)r.ahead_mask;
    }
    c.end(p, s_nsim, ntask + NA * nlive);
}

hipError_t launch_step_lookahead(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                                 const StepLookaheadArgs &a) {
    return with_agents(N, hipErrorInvalidValue, [&](auto n) {
        gwprof::launch(step_lookahead_kernel<decltype(n)::value>, grid, block, dyn, s, p, a);
        return hipSuccess;  // a launch error stays in hipGetLastError for the caller (launch_cf)
    });
}

}  // namespace gw
