// fear_shield_joint.hip -- fear_shield_joint_kernel (gw_fear_shield_joint): the coordinated responsibility
// shield.  A translation unit of its own on the shared headers (cf_env.h, fear_alt_core.h, fear_shield.h),
// so that the code object of gridenv.hip's step kernels does not change with it; gridenv.hip owns the
// preview's record buffer, runs preview_rec_kernel on it and then this kernel (launch_cf: geometry, LDS, span).
#include <hip/hip_runtime.h>

#include "cf_env.h"
#include "dispatch.h"
#include "fear_alt_core.h"
#include "fear_shield.h"
#include "prof.h"

namespace gw {

// Orders one wave's LDS accesses: the LDS serves a wave's instructions in issue order, so what is left to do is
// to keep the compiler from moving an access across this point.  No instruction, no other wave involved.
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------------
// fear_shield_joint_kernel (gw_fear_shield_joint; the rule: include/gridenv.h).  On the wave-per-env scaffold
// (CfEnv) from the preview's record: the env's cells and the joint action (prop, scripted) the next step would
// apply, both clamped to their ranges by CfEnv::begin.  Every lane of the wave keeps the env's current joint
// action `act` in registers; everything a loop's trip count or a branch depends on is the same in all 64 lanes.
//   run(sel): FearAltCore's clear and run (csrc/fear_alt_core.h, shared with fear_alt_kernel): the world updates
//     of the actors in `sel` under `act` into their 9-bit valid sets; an actor's [9][N] words of vb are cleared first.
//   row(k, a): FearAltCore's row, the code that computes fear_alt_kernel's table entry.
//   A visit of shielded actor k: run(1 << k); lanes 0-8 store row(k, lane) into s_row; every lane runs
//     fear_shield::pick on s_row and updates its copy of act[k].
//   After the sweeps: the rows of the shielded actors are those of the final joint action if the last sweep
//     changed nothing (every one of its visits saw that joint action), so only the other actors' tasks run;
//     else all K actors' run.  Lane i = (k, a) stores T[k][a]; the lane with a == act[k] also stores
//     actions_out[k] and flags[k] (bit 2 from its own entry).  Lanes 0..N-1 store joint.
// The four waves of a block are four envs that need different numbers of visits: nothing between begin()'s
// barrier and end()'s is block-wide.  One wave owns vb[wave] and s_row[wave] (and a thread its wl row); a wave's
// LDS accesses are ordered by wave_lds_order().  A wave past the env range runs no visit and no task and goes
// straight to end().
// ---------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(CF_T) fear_shield_joint_kernel(Params p, ShieldJointArgs a) {
    using Core = FearAltCore<N>;
    constexpr bool LIST = Core::LIST;
    constexpr int VBW = Core::VBW;  // per env, sized for K = N
    __shared__ uint32_t vb[CF_WAVES][VBW];
    __shared__ uint2 wl[LIST ? CF_T * N : 1];  // World<N, true> rows (one per thread)
    __shared__ double s_row[CF_WAVES][NA];     // the visited actor's table row
    __shared__ unsigned int s_nsim;
    static_assert(sizeof(uint32_t) * CF_WAVES * VBW + sizeof(uint2) * (LIST ? CF_T * N : 1) +
                          sizeof(double) * CF_WAVES * NA <= 26 * 1024,
                  "static LDS: fear_alt_kernel's budget");
    CfEnv<N> c;
    c.begin(p, 0, s_nsim, [] {});  // run() clears the sets it fills
    const int tid = threadIdx.x, wave = c.wave, lane = c.lane, K = min(p.K, N);
    const CtabOk okv{c.ctab};
    uint32_t *const vbw = vb[wave];
    int act[N];  // the current joint action: act[0..K) is `cur` of the rule
#pragma unroll
    for (int n = 0; n < N; ++n) act[n] = c.act[n];
    Core core;
    core.plan(p, c.pos, K);
    int nsim = 0;  // world updates this wave ran

    // the world updates of the actors in sel (non-zero, bits below K) under `act` into their sets, cleared first
    auto run = [&](uint32_t sel) {
        Core::clear(sel, vbw, lane);
        wave_lds_order();
        nsim += core.run(sel, act, p, okv, c.pos, vbw, LIST ? &wl[tid * N] : nullptr, lane);
        wave_lds_order();
    };
    auto row = [&](int k, int va) { return Core::row(k, va, c.mdr, vbw, c.tab); };

    const uint32_t all_k = (1u << K) - 1u, shielded = a.agents & all_k;
    uint32_t stuck = 0u;
    bool changed = false;  // the last sweep that ran changed an action
    if (c.live && shielded) {
        for (int s = 0; s < a.sweeps; ++s) {
            changed = false;
            for (int k = 0; k < K; ++k) {
                if (!((shielded >> k) & 1u)) continue;
                run(1u << k);
                if (lane < NA) s_row[wave][lane] = row(k, lane);
                wave_lds_order();
                int cur = 0;
#pragma unroll
                for (int q = 0; q < N; ++q)
                    if (q == k) cur = act[q];
                const int64_t ek = c.e * p.K + k;
                const fear_shield::Pick r = fear_shield::pick(s_row[wave], cur, a.mask ? a.mask[ek] : 0x1FFu,
                                                              a.probs ? a.probs + ((int64_t)k * p.E + c.e) * NA : nullptr,
                                                              a.tau, true);
                wave_lds_order();  // s_row is read before the next visit rewrites it
                const int pick = min(max(r.action, 0), NA - 1);
                stuck = (stuck & ~(1u << k)) | ((uint32_t)((r.flags >> 1) & 1) << k);
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
        // an unchanged last sweep left the shielded actors' rows of the final joint action in vb
        const uint32_t have = (shielded && !changed) ? shielded : 0u;
        if (all_k & ~have) run(all_k & ~have);
        for (int i = lane; i < K * NA; i += 64) {
            const int k = i / NA, va = i - k * NA;
            const double t = row(k, va);
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
                               ((uint32_t)(sh && t > a.tau) << 2) | ((uint32_t)changed << 3);
            if (a.flags) a.flags[ek] = (uint8_t)f;
        }
        if (a.joint && lane < N) {
            int v = 0;
#pragma unroll
            for (int q = 0; q < N; ++q)
                if (q == lane) v = act[q];
            a.joint[c.e * N + lane] = v;
        }
    }
    c.end(p, s_nsim, nsim);
}

hipError_t launch_fear_shield_joint(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                                    const ShieldJointArgs &a) {
    return with_agents(N, hipErrorInvalidValue, [&](auto n) {
        gwprof::launch(fear_shield_joint_kernel<decltype(n)::value>, grid, block, dyn, s, p, a);
        return hipSuccess;  // a launch error stays in hipGetLastError for the caller (launch_cf)
    });
}

}  // namespace gw
