// fear_shield_joint.hip -- fear_shield_joint_kernel (gw_fear_shield_joint): the coordinated responsibility
// shield.  A translation unit of its own on the shared headers (cf_env.h, fear_alt_tasks.h, fear_shield.h,
// np_sum.h), so that the code object of gridenv.hip's step kernels does not change with it; gridenv.hip owns the
// preview's record buffer, runs preview_rec_kernel on it and then this kernel (launch_cf: geometry, LDS, span).
#include <hip/hip_runtime.h>

#include "cf_env.h"
#include "dispatch.h"
#include "fear_shield.h"
#include "np_sum.h"
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
//   run(sel): the world updates of the actors in `sel` under `act`, fear_alt_kernel's tasks (csrc/fear_alt_tasks.h)
//     and 9-bit valid sets, dealt to the lanes round-robin; an actor's [9][N] words of vb are cleared first.
//   row(k, a): V counts -> Resp table -> np_sum_row, fear_alt_kernel's arithmetic: bit-equal to its table entry.
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
    constexpr bool LIST = N >= GW_LIST_MIN_N;
    constexpr int VBW = fear_alt::bit_words(N, N);  // per env, sized for K = N
    static_assert(VBW == N * NA * N && VBW <= 576, "valid-bit sets: [K <= N][9][N] words per env");
    static_assert(fear_alt::max_per_env(N, N) <= 4104, "tasks per env and run fit an int with room");
    __shared__ uint32_t vb[CF_WAVES][VBW];
    __shared__ uint2 wl[LIST ? CF_T * N : 1];  // World<N, true> rows (one per thread)
    __shared__ double s_row[CF_WAVES][NA];     // the visited actor's table row
    __shared__ unsigned int s_nsim;
    static_assert(sizeof(uint32_t) * CF_WAVES * VBW + sizeof(uint2) * (LIST ? CF_T * N : 1) +
                          sizeof(double) * CF_WAVES * NA <= 26 * 1024,
                  "static LDS: fear_alt_kernel's budget");
    CfEnv<N> c;
    c.begin(p, 0, s_nsim, [] {});  // run() clears the sets it fills
    const int (&pos)[N] = c.pos, (&mdr)[N] = c.mdr;
    const int tid = threadIdx.x, wave = c.wave, lane = c.lane, K = min(p.K, N);
    const CtabOk okv{c.ctab};
    uint32_t *const vbw = vb[wave];
    int act[N];  // the current joint action: act[0..K) is `cur` of the rule
#pragma unroll
    for (int n = 0; n < N; ++n) act[n] = c.act[n];
    uint32_t close[N];
    int tcount[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        close[k] = 0u;
        tcount[k] = 0;
        if (k >= K) continue;
#pragma unroll
        for (int n = 0; n < N; ++n)
            if (n == k || manhattan(p, pos[k], pos[n]) <= 5) close[k] |= 1u << n;
        tcount[k] = fear_alt::per_actor(__popc(close[k]));
    }
    int nsim = 0;  // world updates this wave ran

    // the world updates of the actors in sel (non-zero, bits below K) under `act` into their sets
    auto run = [&](uint32_t sel) {
        const int lo = (int)__builtin_ctz(sel) * NA * N, hi = (32 - (int)__builtin_clz(sel)) * NA * N;
        for (int i = lo + lane; i < min(hi, VBW); i += 64)
            if ((sel >> (i / (NA * N))) & 1u) vbw[i] = 0u;
        wave_lds_order();
        int ntask = 0;
#pragma unroll
        for (int q = 0; q < N; ++q) ntask += ((sel >> q) & 1u) ? tcount[q] : 0;
        for (int ti = lane; ti < ntask; ti += 64) {
            // (actor k, task r of k): the selected actors' tasks follow each other
            int k = 0, r = ti;
            bool found = false;
            uint32_t cl = 1u;
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const int tc = ((sel >> q) & 1u) ? tcount[q] : 0;
                if (!found && r < tc) {
                    k = q;
                    cl = close[q];
                    found = true;
                } else if (!found) {
                    r -= tc;
                }
            }
            const fear_alt::Task tk = fear_alt::decode(r, __popc(cl));
            const int j = tk.slot < 0 ? -1 : fear_alt::nth_agent(cl & ~(1u << k), tk.slot);
            int joint[N], b = 0;
#pragma unroll
            for (int n = 0; n < N; ++n) {
                joint[n] = ((cl >> n) & 1u) ? act[n] : 0;
                if (n == k) joint[n] = tk.a;
                if (n == j) joint[n] = b = fear_alt::alternative(tk.bi, act[n]);
            }
            const uint32_t valid = cf_valid<N, LIST, true>(p.W, p.w_magic, okv, pos, joint, LIST ? &wl[tid * N] : nullptr);
            uint32_t *row = &vbw[(k * NA + tk.a) * N];  // k < K <= N, a <= 8: inside the wave's VBW words
            if (j >= 0) {
                if ((valid >> j) & 1u) atomicOr(&row[j], 1u << b);
            } else {
#pragma unroll
                for (int n = 0; n < N; ++n)
                    if (n != k && ((valid >> n) & 1u)) atomicOr(&row[n], ((cl >> n) & 1u) ? (1u << act[n]) : 0x1FFu);
            }
        }
        wave_lds_order();
        nsim += ntask;
    };
    // T[k][va] of the sets in vb: fear_alt_kernel's arithmetic
    auto row = [&](int k, int va) -> double {
        int mk = 0;
#pragma unroll
        for (int q = 0; q < N; ++q)
            if (q == k) mk = mdr[q];
        const uint32_t *rm = &vbw[(k * NA + mk) * N], *ra = &vbw[(k * NA + va) * N];
        double resp[N];
#pragma unroll
        for (int jj = 0; jj < N; ++jj) {
            const int vm = __popc(rm[jj] & 0x1FFu), vv = __popc(ra[jj] & 0x1FFu);
            resp[jj] = (jj == k) ? 0.0 : c.tab[vm * 10 + vv];
        }
        return np_sum_row<N>(resp, k);
    };

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
