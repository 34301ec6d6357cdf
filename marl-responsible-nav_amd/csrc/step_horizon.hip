// step_horizon.hip -- step_horizon_kernel (gw_step_horizon): the crash horizon.  For each RL agent k and first
// action a, how many of the next H steps k can survive (depth), without moving the world.  As long as k has not
// crashed, the world differs between k's choices in k's own cell only (an agent changes another agent's cell only
// through a collision, a collision marks both crashed, and an RL crash ends the episode), so the steps after the
// first are a dynamic programme over k's cell: one world update per (level, distinct cell, allowed action)
// against that level's one background, then a backward pass over the stored transitions (step_horizon.h).
// A translation unit of its own on the shared headers (cf_env.h, draw_action.h), so that the code object of
// gridenv.hip's step kernels does not change with it; gridenv.hip runs this kernel right behind
// preview_rec_kernel (fear_preview.hip) on gw_step_preview's record buffer.
#include <hip/hip_runtime.h>

#include "cf_env.h"
#include "dispatch.h"
#include "philox.h"
#include "prof.h"
#include "step_horizon.h"

namespace gw {

#include "draw_action.h"
#include "preview_done.h"

#include "horizon_window.h"

// One wave's (one env's) LDS, reused by its RL agents in turn
struct HzWave {
    uint32_t occ[HZ_LEVELS][HZ_WORDS];  // [h - 1]: bit s = k can stand in slot s after h steps (and the episode goes on)
    uint32_t best;                      // the lowest task index of this level whose step goes on (HZ_NONE: none)
    uint32_t c9, e9;                    // bit a = k itself crashes / the episode ends in the first step under a
    uint32_t nrun;                      // world updates of the levels >= 1, all k
    uint32_t nn[HZ_LEVELS + 1];         // [h]: nodes of level h
    uint16_t bg[MAXN];                  // this level's background: n's cell | n >= K: its action << 12
    uint8_t nodes[HZ_NODES + 1];        // [hz_off(h) + j]: the slot of node j of level h, ascending
    uint8_t tr[HZ_NODES * NA];          // [node * 9 + b]: transition code (step_horizon.h) of an allowed b
    uint8_t first[12], d9[12];          // [a]: transition code of the first step / its depth
    uint8_t dep[2][HZ_SLOTS + 3];       // [h & 1][slot]: depth of the level-h node in that slot
};

// ---------------------------------------------------------------------------------------
// step_horizon_kernel (gw_step_horizon) on the wave-per-env scaffold (CfEnv), from the record preview_rec_kernel
// built.  Per env (one wave), for each RL agent k < K in turn:
//   level 0: the nine first actions (step_preview_kernel's task, lanes 0-8).  A task stores its transition code
//     (first[a]), ORs k's own crash bit into c9 and the step's ends bit into e9 and, where k is fine and the
//     episode goes on, sets k's slot in occ[0];
//   level h = 1..H - 1, while some task of the level before goes on: that level's lowest such task (atomicMin
//     on its index; its lane kept the final cells in registers) writes the background bg; lanes 0..N-K-1 draw
//     the scripted agents' actions of step t + h from their background cells (the Philox law always: a caller's
//     override holds for the first step only); the set bits of occ[h - 1] become the ascending node list (a lane
//     ranks its slots by population counts of the words: nothing wave-collective); the tasks (node, b) are dealt
//     round-robin, a b the node's cell does not allow is skipped, every other one is one world update (no apples)
//     of the background with k in the node's cell playing b and the other RL agents 0;
//   backward: depth per node from level H - 1 down to 1, one node per lane (step_horizon::node_depth), then per
//     first action (step_horizon::after), then lane 0 stores the sets and the mask (step_horizon::rules).
// A step that ends the episode ends it for every task of its level that k survives (the cap, or another RL
// agent's crash, which does not depend on k), so `best` stays HZ_NONE and the forward pass stops there.
// No wave-collective operation stands inside the task loops (their last turn and the skipped tasks leave lanes
// idle; the wave reconverges before lookahead_lds_order() and end()); every loop bound and break below is read
// from LDS words that all lanes read alike; the four waves of a block are four envs: nothing between begin()'s
// barrier and end()'s is block-wide, a wave owns its HzWave and orders its own LDS accesses with
// lookahead_lds_order(); a wave past the env range has no agent and goes straight to end().
// ---------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(CF_T) step_horizon_kernel(Params p, StepHorizonArgs a) {
    constexpr bool LIST = N >= GW_LIST_MIN_N;
    __shared__ HzWave hw[CF_WAVES];
    __shared__ uint2 wl[LIST ? CF_T * N : 1];  // World<N, true> rows (one per thread)
    __shared__ unsigned int s_nsim;
    static_assert(sizeof(HzWave) * CF_WAVES + sizeof(uint2) * (LIST ? CF_T * N : 1) <= 25 * 1024 &&
                      sizeof(HzWave) * CF_WAVES <= 9 * 1024,
                  "static LDS of step_horizon_kernel");
    CfEnv<N> c;
    c.begin(p, 0, s_nsim, [&] {
        if (c.lane == 0) hw[c.wave].nrun = 0u;
    });
    const int tid = threadIdx.x, lane = c.lane, K = min(p.K, N);
    HzWave &s = hw[c.wave];
    const CtabOk okv{c.ctab};
    const int H = min(max(a.horizon, 2), GW_HORIZON_MAX);
    const int nk = c.live ? K : 0;
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

    for (int k = 0; k < nk; ++k) {
        for (int i = lane; i < HZ_LEVELS * HZ_WORDS; i += 64) (&s.occ[0][0])[i] = 0u;
        if (lane == 0) {
            s.best = HZ_NONE;
            s.c9 = s.e9 = 0u;
        }
        lookahead_lds_order();
        HzWindow<N> win;
        int here = 0;  // k's present cell (a select over the unrolled n: no dynamically indexed register array)
#pragma unroll
        for (int n = 0; n < N; ++n) here = (n == k) ? c.pos[n] : here;
        win.r0 = div_w(p, here);
        win.c0 = here - win.r0 * p.W;
        win.H = p.H, win.W = p.W, win.w_magic = p.w_magic;
        uint32_t mine = HZ_NONE;  // this lane's lowest task of the level whose step goes on ...
        int keep[N];              // ... and the cells that task left
#pragma unroll
        for (int n = 0; n < N; ++n) keep[n] = 0;

        // level 0: the step about to run under each first action
        if (lane < NA) {
            int joint[N], fin[N];
#pragma unroll
            for (int n = 0; n < N; ++n) joint[n] = (n == k) ? lane : c.act[n];
            World<N, LIST> w;
            w.init(c.pos, joint, p.W, p.w_magic);
            if constexpr (LIST) w.lw = wl_row;
            uint32_t caught;
            simulate<N, true>(w, okv, K, apple, caught, fin);
            const bool crash = (w.crash >> k) & 1u, done = preview_done(p, K, flags, caught, w.crash, t);
            const uint32_t code = crash ? step_horizon::CRASH : done ? step_horizon::END : (uint32_t)win.slot_of(fin[k]);
            if (crash) atomicOr(&s.c9, 1u << lane);
            if (done) atomicOr(&s.e9, 1u << lane);
            if (code < step_horizon::END) {
                atomicOr(&s.occ[0][code >> 5], 1u << (code & 31u));
                atomicMin(&s.best, (uint32_t)lane);
                mine = (uint32_t)lane;
#pragma unroll
                for (int n = 0; n < N; ++n) keep[n] = fin[n];
            }
            s.first[lane] = (uint8_t)code;
        }
        lookahead_lds_order();

        int top = 0;  // the last level whose tasks ran
        for (int h = 1; h < H; ++h) {
            const uint32_t b0 = s.best;  // the same word for every lane
            if (b0 == HZ_NONE) break;    // k crashed in, or the episode ended with, every task of the level before
            if (mine == b0) {
#pragma unroll
                for (int n = 0; n < N; ++n) s.bg[n] = (uint16_t)keep[n];
            }
            lookahead_lds_order();
            mine = HZ_NONE;
            if (lane == 0) s.best = HZ_NONE;
            if (lane < N - K) {  // the scripted agents' draws of step t + h, once per level
                Params p2 = p;
                p2.scripted = nullptr;  // a caller's override holds for the step about to run only
                const int n = K + lane;
                const int cell = min((int)(s.bg[n] & 0xFFFu), p.HW - 1);
                const int act = draw_action(p2, c.e, n, episode, t + h, cell, c.ctab, nullptr);  // in 0..8
                s.bg[n] = (uint16_t)((uint32_t)cell | ((uint32_t)act << 12));
            }
            // the node list: the set slots of occ[h - 1], ascending
            const int off = hz_off(h), cap = hz_cap(h);
            uint32_t words[HZ_WORDS];
#pragma unroll
            for (int q = 0; q < HZ_WORDS; ++q) words[q] = s.occ[h - 1][q];
            const int nn = hz_list_nodes(words, lane, cap, &s.nodes[off]);
            if (lane == 0) s.nn[h] = (uint32_t)nn;
            lookahead_lds_order();

            // the level's tasks: step h + 1 from each node under each action its cell allows
            const int ntask = nn * NA;
            for (int i = lane; i < ntask; i += 64) {
                const int j = i / NA, b = i - j * NA;  // j < nn <= cap
                const int cell = win.cell_of(min((int)s.nodes[off + j], HZ_SLOTS - 1));
                const uint32_t m = (c.ctab[cell] >> CT_AMASK) & step_horizon::ALL;
                if (!((m >> b) & 1u)) continue;
                int pos[N], joint[N], fin[N];
#pragma unroll
                for (int n = 0; n < N; ++n) {
                    const uint32_t v = s.bg[n];
                    pos[n] = (n == k) ? cell : min((int)(v & 0xFFFu), p.HW - 1);
                    joint[n] = (n == k) ? b : (n < K) ? 0 : min((int)(v >> 12), NA - 1);
                }
                World<N, LIST> w;
                w.init(pos, joint, p.W, p.w_magic);
                if constexpr (LIST) w.lw = wl_row;
                uint32_t caught;
                simulate<N, false>(w, okv, 0, no_apple, caught, fin);
                atomicAdd(&s.nrun, 1u);
                const bool crash = (w.crash >> k) & 1u, done = preview_done(p, K, 0u, 0u, w.crash, t + h);
                const uint32_t code =
                    crash ? step_horizon::CRASH : done ? step_horizon::END : (uint32_t)win.slot_of(fin[k]);
                if (code < step_horizon::END && h + 1 < H) {
                    atomicOr(&s.occ[h][code >> 5], 1u << (code & 31u));
                    atomicMin(&s.best, (uint32_t)i);
                    if (mine == HZ_NONE) {
                        mine = (uint32_t)i;
#pragma unroll
                        for (int n = 0; n < N; ++n) keep[n] = fin[n];
                    }
                }
                s.tr[(off + j) * NA + b] = (uint8_t)code;
            }
            lookahead_lds_order();
            top = h;
        }

        // backward: depth per node, the deepest level first
        for (int h = top; h >= 1; --h) {
            const int off = hz_off(h), nn = min((int)s.nn[h], hz_cap(h));
            for (int j = lane; j < nn; j += 64) {
                const int slot = min((int)s.nodes[off + j], HZ_SLOTS - 1);
                const uint32_t m = (c.ctab[win.cell_of(slot)] >> CT_AMASK) & step_horizon::ALL;
                s.dep[h & 1][slot] = (uint8_t)step_horizon::node_depth(h, H, m, &s.tr[(off + j) * NA], HzDepths{s.dep[(h + 1) & 1]});
            }
            lookahead_lds_order();
        }
        if (lane < NA) {
            const uint32_t d = step_horizon::after(0, H, s.first[lane], HzDepths{s.dep[1]});
            s.d9[lane] = (uint8_t)d;
            if (a.depth) a.depth[(c.e * p.K + k) * NA + lane] = (uint8_t)d;
        }
        lookahead_lds_order();
        if (lane == 0) {
            const int64_t ek = c.e * p.K + k;
            const step_horizon::Horizon r = step_horizon::rules(a.mask != nullptr, a.mask ? a.mask[ek] : 0u, H, s.d9);
            if (a.crash9) a.crash9[ek] = (uint16_t)(s.c9 & step_horizon::ALL);
            if (a.ends) a.ends[ek] = (uint16_t)(s.e9 & step_horizon::ALL);
            if (a.viable9) a.viable9[ek] = (uint16_t)r.viable9;
            if (a.horizon_mask) a.horizon_mask[ek] = (uint16_t)r.horizon_mask;
        }
        lookahead_lds_order();
    }
    c.end(p, s_nsim, nk ? NA * nk + (int)s.nrun : 0);
}

hipError_t launch_step_horizon(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                               const StepHorizonArgs &a) {
    return with_agents(N, hipErrorInvalidValue, [&](auto n) {
        gwprof::launch(step_horizon_kernel<decltype(n)::value>, grid, block, dyn, s, p, a);
        return hipSuccess;  // a launch error stays in hipGetLastError for the caller (launch_cf)
    });
}

}  // namespace gw
