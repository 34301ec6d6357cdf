// step_plan.hip -- step_plan_kernel (gw_step_plan): the reward horizon.  For each RL agent k and first action a,
// how many of the next H steps k can survive (depth) and the largest env reward those steps can pay it (ret), with
// the actions that do so (path), without moving the world.  step_horizon.hip's dynamic programme over k's cell on
// the world with its real apples: while k has not crashed the world differs between k's choices in k's cell and in
// whether k's apple is still there, nothing else (motion and crashes do not depend on apples; the other agents'
// apples belong to the level's one background; k's prev_dist is a function of its cell and its apple bit), so a
// node is still a cell: one world update per (level, distinct cell, allowed action) with k's apple present, whose
// transition keeps what both worlds need (step_plan.h), then a backward pass with two values per node.
// A translation unit of its own on the shared headers, so that the code object of gridenv.hip's step kernels does
// not change with it; gridenv.hip runs this kernel right behind preview_rec_kernel (fear_preview.hip) on
// gw_step_preview's record buffer.
#include <hip/hip_runtime.h>

#include "cf_env.h"
#include "dispatch.h"
#include "philox.h"
#include "prof.h"
#include "step_plan.h"

namespace gw {

#include "draw_action.h"
#include "preview_done.h"
#include "preview_reward.h"
#include "horizon_window.h"

static_assert(GW_HORIZON_MAX == step_plan::HORIZON_MAX, "step_plan.h restates GW_HORIZON_MAX");

// One wave's (one env's) LDS, reused by its RL agents in turn
struct PlWave {
    uint32_t occ[2][HZ_LEVELS][HZ_WORDS];  // [w][h - 1]: bit s = k can stand in slot s after h steps, its apple there (w = 1) or not
    uint32_t best;                         // the lowest task index of this level whose step goes on (HZ_NONE: none)
    uint32_t c9, e9;                       // bit a = k itself crashes / the episode ends in the first step under a
    uint32_t nrun;                         // world updates of the levels >= 1, all k
    uint32_t bgflags;                      // this level's background: the OTHER agents' apples | term << 8 | trunc << 16
    uint32_t nn[HZ_LEVELS + 1];            // [h]: nodes of level h
    uint32_t tr[HZ_NODES * NA];            // [node * 9 + b]: packed transition (step_plan.h) of an allowed b
    uint32_t first[12];                    // [a]: packed transition of the first step
    int16_t r1[2][HZ_SLOTS + 3];           // [h & 1][slot]: return of the level-h node in that slot, k's apple present
    int16_t r9[12];                        // [a]: return of the first action
    uint16_t bg[MAXN];                     // this level's background: n's cell | n >= K: its action << 12
    uint16_t link[HZ_LEVELS][HZ_SLOTS][2]; // [h - 1][slot][w]: the step the node's best continuation takes in world w
    uint8_t nodes[HZ_NODES + 1];           // [hz_off(h) + j]: the slot of node j of level h, ascending
    uint8_t d0[2][HZ_SLOTS + 3];           // [h & 1][slot]: depth of the level-h node in that slot without k's apple ...
    uint8_t d1[2][HZ_SLOTS + 3];           // ... and with it
    uint8_t d9[12];                        // [a]: depth of the first action
};

// A level's values as step_plan's functions read them: by transition code, clamped to the window
struct PlDeeper {
    const uint8_t *p0, *p1;
    const int16_t *pr;
    __device__ __forceinline__ uint32_t d0(uint32_t slot) const { return p0[min(slot, (uint32_t)HZ_SLOTS - 1u)]; }
    __device__ __forceinline__ uint32_t d1(uint32_t slot) const { return p1[min(slot, (uint32_t)HZ_SLOTS - 1u)]; }
    __device__ __forceinline__ int32_t r1(uint32_t slot) const { return pr[min(slot, (uint32_t)HZ_SLOTS - 1u)]; }
};

// The links as step_plan::path reads them: level, node and world clamped
struct PlLinks {
    const uint16_t (*l)[HZ_SLOTS][2];
    __device__ __forceinline__ uint32_t operator()(int h, uint32_t slot, bool present) const {
        return l[min(max(h, 1), HZ_LEVELS) - 1][min(slot, (uint32_t)HZ_SLOTS - 1u)][present ? 1 : 0];
    }
};

// an env reward in tenths (the rewards are sums of 20, 20, -10, 1 and 0.1)
__device__ __forceinline__ int32_t reward_tenths(double r) { return __double2int_rn(__dmul_rn(r, 10.0)); }

// ---------------------------------------------------------------------------------------
// step_plan_kernel (gw_step_plan) on the wave-per-env scaffold (CfEnv), from the record preview_rec_kernel built.
// step_horizon_kernel's passes (step_horizon.hip), per env (one wave) and RL agent k < K in turn, with these
// differences:
//   level 0: a task also keeps the step's reward (step_preview_kernel's reward_alt entry, in tenths) and whether
//     k's apple is still there afterwards, and sets k's slot in the occupancy of that world;
//   level h >= 1: the background also carries the other agents' apples and the term / trunc flags (an episode that
//     goes on leaves them as they were); the node list is the union of the two worlds' occupancies; a task is one
//     REAL world update (eaters 0..K-1) with k's apple present if it was at the call, priced by preview_reward
//     from prev_dist = the distance of the node's cell to k's apple, and judged by preview_done twice: without
//     k's apple for the transition code, with it for the `last` bit.  (The two can differ in that bit only: in the
//     steps after the first the other RL agents stay, and an agent that stays on its apple's cell has eaten it
//     before, so only k pops an apple there.)  Its target joins the world the node's reachable worlds lead to;
//   backward: step_plan::node per node (two depths, one return, two links), step_plan::after1 and
//     step_plan::path per first action, then lane 0 stores the sets and step_plan::plan_mask.
// Values of a world in which a node cannot be reached are computed and never read by a reachable one: a reachable
// state's transitions lead to listed nodes only.
// The safety rules are step_horizon_kernel's: no wave-collective operation inside the task loops; every loop bound
// and break is read from LDS words that all lanes read alike; nothing between begin()'s barrier and end()'s is
// block-wide, a wave owns its PlWave and orders its own LDS accesses with lookahead_lds_order(); every decoded
// slot, cell, action and index is clamped before it indexes anything; a wave past the env range has no agent and
// goes straight to end().
// ---------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(CF_T) step_plan_kernel(Params p, StepPlanArgs a) {
    constexpr bool LIST = N >= GW_LIST_MIN_N;
    __shared__ PlWave pw[CF_WAVES];
    __shared__ uint2 wl[LIST ? CF_T * N : 1];  // World<N, true> rows (one per thread)
    __shared__ unsigned int s_nsim;
    static_assert(sizeof(PlWave) * CF_WAVES + sizeof(uint2) * (LIST ? CF_T * N : 1) <= 52 * 1024 &&
                      sizeof(PlWave) * CF_WAVES <= 36 * 1024,
                  "static LDS of step_plan_kernel");
    CfEnv<N> c;
    c.begin(p, 0, s_nsim, [&] {
        if (c.lane == 0) pw[c.wave].nrun = 0u;
    });
    const int tid = threadIdx.x, lane = c.lane, K = min(p.K, N);
    PlWave &s = pw[c.wave];
    const CtabOk okv{c.ctab};
    const int H = min(max(a.horizon, 2), GW_HORIZON_MAX);
    const int nk = c.live ? K : 0;
    const uint32_t flags = c.live ? p.st.flags[c.e] : 0u;
    const uint32_t apples0 = flags & 0xFFu, upper = flags & 0xFFFF00u;
    const int t = c.live ? p.st.t[c.e] : 0;
    const uint32_t episode = c.live ? p.st.episode[c.e] : 0u;
    uint2 *const wl_row = LIST ? &wl[tid * N] : nullptr;
    int apple[MAXN];
#pragma unroll
    for (int q = 0; q < MAXN; ++q) apple[q] = (q < K && ((apples0 >> q) & 1u)) ? p.apples[q] : -1;

    for (int k = 0; k < nk; ++k) {
        for (int i = lane; i < 2 * HZ_LEVELS * HZ_WORDS; i += 64) (&s.occ[0][0][0])[i] = 0u;
        if (lane == 0) {
            s.best = HZ_NONE;
            s.c9 = s.e9 = 0u;
        }
        lookahead_lds_order();
        HzWindow<N> win;
        int here = 0, apple_k = 0;  // k's present cell and its apple's (selects over the unrolled n)
#pragma unroll
        for (int n = 0; n < N; ++n) {
            here = (n == k) ? c.pos[n] : here;
            apple_k = (n == k) ? p.apples[n] : apple_k;
        }
        win.r0 = div_w(p, here);
        win.c0 = here - win.r0 * p.W;
        win.H = p.H, win.W = p.W, win.w_magic = p.w_magic;
        const uint32_t kbit = 1u << k, kap = apples0 & kbit;  // kap: k's apple is there at the call
        const int prev0 = p.st.prev[(int64_t)k * p.E + c.e];
        uint32_t mine = HZ_NONE;  // this lane's lowest task of the level whose step goes on ...
        int keep[N];              // ... the cells that task left ...
        uint32_t keep_flags = 0u; // ... and the background flags after it
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
            int fin_k = fin[0];
#pragma unroll
            for (int n = 1; n < N; ++n) fin_k = (n == k) ? fin[n] : fin_k;
            const bool crash = (w.crash >> k) & 1u, done = preview_done(p, K, flags, caught, w.crash, t);
            const uint32_t left = apples0 & ~preview_popped(p, apples0, caught);
            const bool present = (left & kbit) != 0u;
            step_plan::Tr tr;
            tr.code = crash ? step_plan::CRASH : done ? step_plan::END : (uint32_t)win.slot_of(fin_k);
            tr.eat = !present;
            tr.last = false;
            tr.rw = reward_tenths(preview_reward(p, k, apples0, caught, w.crash, fin_k, apple_k, prev0));
            if (crash) atomicOr(&s.c9, 1u << lane);
            if (done) atomicOr(&s.e9, 1u << lane);
            if (tr.code < step_plan::END) {
                atomicOr(&s.occ[present ? 1 : 0][0][tr.code >> 5], 1u << (tr.code & 31u));
                atomicMin(&s.best, (uint32_t)lane);
                mine = (uint32_t)lane;
                keep_flags = upper | (left & ~kbit);
#pragma unroll
                for (int n = 0; n < N; ++n) keep[n] = fin[n];
            }
            s.first[lane] = step_plan::pack(tr);
        }
        lookahead_lds_order();

        int top = 0;  // the last level whose tasks ran
        for (int h = 1; h < H; ++h) {
            const uint32_t b0 = s.best;  // the same word for every lane
            if (b0 == HZ_NONE) break;    // k crashed in, or the episode ended with, every task of the level before
            if (mine == b0) {
#pragma unroll
                for (int n = 0; n < N; ++n) s.bg[n] = (uint16_t)keep[n];
                s.bgflags = keep_flags;
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
            // the node list: the slots set in either world's occupancy, ascending
            const int off = hz_off(h), cap = hz_cap(h);
            uint32_t words[HZ_WORDS];
#pragma unroll
            for (int q = 0; q < HZ_WORDS; ++q) words[q] = s.occ[0][h - 1][q] | s.occ[1][h - 1][q];
            const int nn = hz_list_nodes(words, lane, cap, &s.nodes[off]);
            if (lane == 0) s.nn[h] = (uint32_t)nn;
            lookahead_lds_order();

            // the level's tasks: step h + 1 from each node under each action its cell allows
            const uint32_t lf = s.bgflags, up = lf & 0xFFFF00u;
            const uint32_t apples_bg = lf & 0xFFu & ~kbit, apples1 = apples_bg | kap;
            int lap[MAXN];  // the level's apples, k's present if it was at the call
#pragma unroll
            for (int q = 0; q < MAXN; ++q) lap[q] = (q < K && ((apples1 >> q) & 1u)) ? p.apples[q] : -1;
            const int ntask = nn * NA;
            for (int i = lane; i < ntask; i += 64) {
                const int j = i / NA, b = i - j * NA;  // j < nn <= cap
                const int slot = min((int)s.nodes[off + j], HZ_SLOTS - 1);
                const int cell = win.cell_of(slot);
                const uint32_t m = (c.ctab[cell] >> CT_AMASK) & step_plan::ALL;
                if (!((m >> b) & 1u)) continue;
                const bool r0 = (s.occ[0][h - 1][slot >> 5] >> (slot & 31)) & 1u;  // the worlds the node is reached in
                const bool r1 = (s.occ[1][h - 1][slot >> 5] >> (slot & 31)) & 1u;
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
                simulate<N, true>(w, okv, K, lap, caught, fin);
                atomicAdd(&s.nrun, 1u);
                int fin_k = fin[0];
#pragma unroll
                for (int n = 1; n < N; ++n) fin_k = (n == k) ? fin[n] : fin_k;
                const bool crash = (w.crash >> k) & 1u;
                const bool done0 = preview_done(p, K, up | apples_bg, caught, w.crash, t + h);
                const bool done1 = preview_done(p, K, up | apples1, caught, w.crash, t + h);
                const uint32_t popped = preview_popped(p, apples1, caught);
                step_plan::Tr tr;
                tr.code = crash ? step_plan::CRASH : done0 ? step_plan::END : (uint32_t)win.slot_of(fin_k);
                tr.eat = (popped & kbit) != 0u;
                tr.last = !crash && !done0 && done1;
                tr.rw = reward_tenths(preview_reward(p, k, apples1, caught, w.crash, fin_k, apple_k,
                                                     manhattan(p, cell, apple_k)));
                if (tr.code < step_plan::END && h + 1 < H) {
                    const bool on1 = r1 && !tr.last;  // with its apple k goes on, into the world the step leaves
                    const bool to0 = r0 || (on1 && tr.eat), to1 = on1 && !tr.eat;
                    if (to0) atomicOr(&s.occ[0][h][tr.code >> 5], 1u << (tr.code & 31u));
                    if (to1) atomicOr(&s.occ[1][h][tr.code >> 5], 1u << (tr.code & 31u));
                    if (to0 || to1) {
                        atomicMin(&s.best, (uint32_t)i);
                        if (mine == HZ_NONE) {
                            mine = (uint32_t)i;
                            keep_flags = up | (apples_bg & ~popped);
#pragma unroll
                            for (int n = 0; n < N; ++n) keep[n] = fin[n];
                        }
                    }
                }
                s.tr[(off + j) * NA + b] = step_plan::pack(tr);
            }
            lookahead_lds_order();
            top = h;
        }

        // backward: two depths, a return and two links per node, the deepest level first
        for (int h = top; h >= 1; --h) {
            const int off = hz_off(h), nn = min((int)s.nn[h], hz_cap(h));
            const int up1 = (h + 1) & 1;
            for (int j = lane; j < nn; j += 64) {
                const int slot = min((int)s.nodes[off + j], HZ_SLOTS - 1);
                const uint32_t m = (c.ctab[win.cell_of(slot)] >> CT_AMASK) & step_plan::ALL;
                const step_plan::Node nd =
                    step_plan::node(h, H, m, &s.tr[(off + j) * NA], PlDeeper{s.d0[up1], s.d1[up1], s.r1[up1]});
                s.d0[h & 1][slot] = (uint8_t)nd.d0;
                s.d1[h & 1][slot] = (uint8_t)nd.d1;
                s.r1[h & 1][slot] = (int16_t)nd.r1;
                s.link[h - 1][slot][0] = (uint16_t)nd.l0;
                s.link[h - 1][slot][1] = (uint16_t)nd.l1;
            }
            lookahead_lds_order();
        }
        if (lane < NA) {
            const step_plan::Tr tr = step_plan::unpack(s.first[lane]);
            const step_plan::Val v = step_plan::after1(0, H, tr, PlDeeper{s.d0[1], s.d1[1], s.r1[1]});
            s.d9[lane] = (uint8_t)v.depth;
            s.r9[lane] = (int16_t)v.ret;
            const int64_t o = (c.e * p.K + k) * NA + lane;
            if (a.depth) a.depth[o] = (uint8_t)v.depth;
            if (a.ret) a.ret[o] = (int16_t)v.ret;
            if (a.path) {
                const uint32_t pth = step_plan::path(H, tr, PlLinks{s.link});  // (a node it enters is one of a level that ran)
#pragma unroll
                for (int q = 0; q < GW_HORIZON_MAX - 1; ++q) a.path[o * (GW_HORIZON_MAX - 1) + q] = (uint8_t)(pth >> (8 * q));
            }
        }
        lookahead_lds_order();
        if (lane == 0) {
            const int64_t ek = c.e * p.K + k;
            if (a.crash9) a.crash9[ek] = (uint16_t)(s.c9 & step_plan::ALL);
            if (a.ends) a.ends[ek] = (uint16_t)(s.e9 & step_plan::ALL);
            if (a.plan_mask)
                a.plan_mask[ek] = (uint16_t)step_plan::plan_mask(a.mask != nullptr, a.mask ? a.mask[ek] : 0u, s.d9, s.r9);
        }
        lookahead_lds_order();
    }
    c.end(p, s_nsim, nk ? NA * nk + (int)s.nrun : 0);
}

hipError_t launch_step_plan(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                            const StepPlanArgs &a) {
    return with_agents(N, hipErrorInvalidValue, [&](auto n) {
        gwprof::launch(step_plan_kernel<decltype(n)::value>, grid, block, dyn, s, p, a);
        return hipSuccess;  // a launch error stays in hipGetLastError for the caller (launch_cf)
    });
}

}  // namespace gw
