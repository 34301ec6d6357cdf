// crash_shield_joint.hip -- crash_shield_joint_kernel (gw_crash_shield_joint): the coordinated crash-aware
// shield, the step outcome preview's safe masks inside the joint shield's sweeps.  A translation unit of its own
// on the shared headers (cf_env.h, fear_alt_core.h, crash_shield.h), so that the code objects of gridenv.hip's
// step kernels, of fear_shield_joint.hip and of step_preview.hip do not change with it; gridenv.hip owns the
// preview's record buffer, runs preview_rec_kernel on it and then this kernel (launch_cf: geometry, LDS, span).
#include <hip/hip_runtime.h>

#include "cf_env.h"
#include "crash_shield.h"
#include "dispatch.h"
#include "fear_alt_core.h"
#include "prof.h"

namespace gw {

namespace {

// Orders one wave's LDS accesses (as fear_shield_joint.hip's): the LDS serves a wave's instructions in issue
// order, so what is left to do is to keep the compiler from moving an access across this point.
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One REAL world update (step_preview_kernel's task: the full joint action, eaters 0..K-1, the apples still
// present) of cells `pos` under `joint`, in registers: crash bits | restricted bits << 8.
template <int N, bool LIST>
__device__ __forceinline__ uint32_t real_update(const Params &p, const CtabOk &okv, const int (&pos)[N],
                                                const int (&joint)[N], int K, const int (&apple)[MAXN],
                                                uint2 *wl_row) {
    int fin[N];
    World<N, LIST> w;
    w.init(pos, joint, p.W, p.w_magic);
    if constexpr (LIST) w.lw = wl_row;
    uint32_t caught;
    simulate<N, true>(w, okv, K, apple, caught, fin);
    return (w.crash & 0xFFu) | ((w.restr & 0xFFu) << 8);
}

// nine bits from bit `at` (< 119) of the 128-bit value hi:lo
__device__ __forceinline__ uint32_t bits9(uint64_t lo, uint64_t hi, int at) {
    uint64_t v;
    if (at >= 64)
        v = hi >> (at - 64);
    else
        v = (lo >> at) | (at > 55 ? hi << (64 - at) : 0ull);  // at > 55: 64 - at in 1..8
    return (uint32_t)v & step_preview::ALL;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// crash_shield_joint_kernel (gw_crash_shield_joint; the rule and the sim count: include/gridenv.h).  On the
// wave-per-env scaffold (CfEnv) from the preview's record, built like fear_shield_joint_kernel: every lane of the
// wave keeps the env's current joint action `act` in registers; every trip count and every branch around a
// wave-wide operation (ballot, shuffle, the LDS ordering) is the same in all 64 lanes.
//   A visit of shielded actor k:
//     the crash preview: lanes 0-8 run one real world update each, act with k playing the lane's action; k's own
//       crash bit reaches all lanes as a wave ballot (crash9), no LDS.  The first visit of the env still sees the
//       proposal, so its lane act[k] holds the proposal's outcome (O_prop), handed round by a shuffle;
//     the FeAR half (use_fear only): FearAltCore's clear / run / row as in the joint shield, lanes 0-8 store the
//       row into s_row;
//     every lane runs crash_shield::visit and updates its copy of act[k].
//   After the sweeps: the K x 9 crash tasks (k, a) of the FINAL joint action dealt round-robin (K = 8: 72 tasks,
//     lanes 0-7 take a second turn), their own-crash bits collected by one ballot per turn; the task (0, act[0])
//     IS the update of the final joint action, so its lane holds O.  Then the table as in the joint shield (only
//     with use_fear or a table to store), the rows of the shielded actors reused after an unchanged last sweep.
//     Lane i = (k, a) stores T[k][a]; the lane with a == act[k] stores actions_out[k] and flags[k]; lanes 0..K-1
//     store crash9; lanes 0..N-1 joint; lane 0 the two outcomes.
// Nothing between begin()'s barrier and end()'s is block-wide: the four waves are four envs that need different
// numbers of visits.  One wave owns vb[wave] and s_row[wave] (and a thread its wl row).  A wave past the env
// range goes straight to end().
// ---------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(CF_T) crash_shield_joint_kernel(Params p, CrashShieldArgs a) {
    using Core = FearAltCore<N>;
    constexpr bool LIST = Core::LIST;
    constexpr int VBW = Core::VBW;  // per env, sized for K = N
    __shared__ uint32_t vb[CF_WAVES][VBW];
    __shared__ uint2 wl[LIST ? CF_T * N : 1];  // World<N, true> rows (one per thread), both kinds of update
    __shared__ double s_row[CF_WAVES][NA];     // the visited actor's table row
    __shared__ unsigned int s_nsim;
    static_assert(sizeof(uint32_t) * CF_WAVES * VBW + sizeof(uint2) * (LIST ? CF_T * N : 1) +
                          sizeof(double) * CF_WAVES * NA <= 26 * 1024,
                  "static LDS: fear_shield_joint_kernel's budget");
    CfEnv<N> c;
    c.begin(p, 0, s_nsim, [&] { if (c.lane < NA) s_row[c.wave][c.lane] = 0.0; });
    const int tid = threadIdx.x, wave = c.wave, lane = c.lane, K = min(p.K, N);
    const CtabOk okv{c.ctab};
    uint32_t *const vbw = vb[wave];
    uint2 *const wl_row = LIST ? &wl[tid * N] : nullptr;
    const bool use_fear = a.use_fear != 0, want_table = use_fear || a.table != nullptr;
    const uint32_t apples = c.live ? (p.st.flags[c.e] & 0xFFu) : 0u;
    int apple[MAXN];
#pragma unroll
    for (int q = 0; q < MAXN; ++q) apple[q] = (q < K && ((apples >> q) & 1u)) ? p.apples[q] : -1;
    int act[N];  // the current joint action: act[0..K) is `cur` of the rule
#pragma unroll
    for (int n = 0; n < N; ++n) act[n] = c.act[n];
    Core core;
    core.plan(p, c.pos, K);
    int nsim = 0;  // world updates this wave ran

    // the real world update of `act` with actor k playing b
    auto crash_task = [&](int k, int b) {
        int joint[N];
#pragma unroll
        for (int n = 0; n < N; ++n) joint[n] = (n == k) ? b : act[n];
        return real_update<N, LIST>(p, okv, c.pos, joint, K, apple, wl_row);
    };
    // the FeAR world updates of the actors in sel (non-zero, bits below K) under `act` into their sets, cleared first
    auto run = [&](uint32_t sel) {
        Core::clear(sel, vbw, lane);
        wave_lds_order();
        nsim += core.run(sel, act, p, okv, c.pos, vbw, wl_row, lane);
        wave_lds_order();
    };
    auto row = [&](int k, int va) { return Core::row(k, va, c.mdr, vbw, c.tab); };

    const uint32_t all_k = (1u << K) - 1u, shielded = a.agents & all_k;
    uint32_t stuck = 0u, unavoidable = 0u;
    uint32_t o_prop = 0u;
    bool have_prop = false;  // a visit has run (uniform): o_prop is the proposal's outcome
    bool changed = false;    // the last sweep that ran changed an action
    if (c.live && shielded) {
        for (int s = 0; s < a.sweeps; ++s) {
            changed = false;
            for (int k = 0; k < K; ++k) {
                if (!((shielded >> k) & 1u)) continue;
                int cur = 0;
#pragma unroll
                for (int q = 0; q < N; ++q)
                    if (q == k) cur = act[q];
                uint32_t oc = 0u;
                if (lane < NA) oc = crash_task(k, lane);
                nsim += NA;
                const uint32_t crash9 = (uint32_t)__ballot((int)((oc >> k) & 1u)) & step_preview::ALL;
                if (!have_prop) {  // nothing has moved yet: lane cur ran the proposal itself
                    o_prop = (uint32_t)__shfl((int)oc, cur);
                    have_prop = true;
                }
                if (use_fear) {
                    run(1u << k);
                    if (lane < NA) s_row[wave][lane] = row(k, lane);
                    wave_lds_order();
                }
                const int64_t ek = c.e * p.K + k;
                const crash_shield::Visit r =
                    crash_shield::visit(s_row[wave], cur, a.mask != nullptr, a.mask ? a.mask[ek] : 0u, crash9,
                                        a.probs ? a.probs + ((int64_t)k * p.E + c.e) * NA : nullptr, use_fear, a.tau);
                wave_lds_order();  // s_row is read before the next visit rewrites it
                const int pick = min(max(r.action, 0), NA - 1);
                stuck = (stuck & ~(1u << k)) | ((uint32_t)((r.flags >> 1) & 1) << k);
                unavoidable = (unavoidable & ~(1u << k)) | ((uint32_t)((r.flags >> 5) & 1) << k);
                if (pick != cur) {
                    changed = true;
#pragma unroll
                    for (int q = 0; q < N; ++q)
                        if (q == k) act[q] = pick;
                }
            }
            if (!changed) break;
        }
    }
    if (c.live) {
        // the own-crash sets of the final joint action, and its outcome from the task (0, act[0])
        const int ntask = K * NA;  // <= 72
        uint64_t own_lo = 0ull, own_hi = 0ull;
        uint32_t o_fin = 0u;
        for (int base = 0; base < ntask; base += 64) {
            const int ti = base + lane;
            uint32_t oc = 0u;
            bool own = false;
            if (ti < ntask) {
                const int k = ti / NA;  // k < K <= N
                oc = crash_task(k, ti - k * NA);
                own = (oc >> k) & 1u;
            }
            const uint64_t bal = __ballot((int)own);
            if (base == 0) {
                own_lo = bal;
                o_fin = (uint32_t)__shfl((int)oc, act[0]);  // act[0] in 0..8: a lane of the first turn
            } else {
                own_hi = bal;
            }
        }
        nsim += ntask;
        if (!have_prop) o_prop = o_fin;  // no visit: the proposal is the final joint action
        if (want_table) {
            // an unchanged last sweep left the shielded actors' rows of the final joint action in vb
            const uint32_t have = (use_fear && shielded && !changed) ? shielded : 0u;
            if (all_k & ~have) run(all_k & ~have);
        }
        for (int i = lane; i < K * NA; i += 64) {
            const int k = i / NA, va = i - k * NA;
            const double t = want_table ? row(k, va) : 0.0;
            const int64_t ek = c.e * p.K + k;
            if (a.table) a.table[ek * NA + va] = t;
            int cur = 0, prop = 0;
#pragma unroll
            for (int q = 0; q < N; ++q)
                if (q == k) {
                    cur = act[q];
                    prop = c.act[q];
                }
            if (va != cur) continue;
            a.actions_out[ek] = cur;
            const bool sh = (shielded >> k) & 1u;
            const uint32_t f = (uint32_t)(cur != prop) | (((stuck >> k) & 1u) << 1) |
                               ((uint32_t)(use_fear && sh && t > a.tau) << 2) | ((uint32_t)changed << 3) |
                               (((o_fin >> k) & 1u) << 4) | (((unavoidable >> k) & 1u) << 5);
            if (a.flags) a.flags[ek] = (uint8_t)f;
        }
        if (a.crash9 && lane < K) a.crash9[c.e * p.K + lane] = (uint16_t)bits9(own_lo, own_hi, lane * NA);
        if (a.joint && lane < N) {
            int v = 0;
#pragma unroll
            for (int q = 0; q < N; ++q)
                if (q == lane) v = act[q];
            a.joint[c.e * N + lane] = v;
        }
        if (lane == 0) {
            if (a.outcome) a.outcome[c.e] = (uint16_t)o_fin;
            if (a.outcome_prop) a.outcome_prop[c.e] = (uint16_t)o_prop;
        }
    }
    c.end(p, s_nsim, nsim);
}

hipError_t launch_crash_shield_joint(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                                     const CrashShieldArgs &a) {
    return with_agents(N, hipErrorInvalidValue, [&](auto n) {
        gwprof::launch(crash_shield_joint_kernel<decltype(n)::value>, grid, block, dyn, s, p, a);
        return hipSuccess;  // a launch error stays in hipGetLastError for the caller (launch_cf)
    });
}

}  // namespace gw
