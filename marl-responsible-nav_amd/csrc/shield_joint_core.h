// shield_joint_core.h -- internal: the one body of the two coordinated shields on the wave-per-env scaffold
// (cf_env.h), fear_shield_joint_kernel (fear_shield_joint.hip, gw_fear_shield_joint) and crash_shield_joint_kernel
// (crash_shield_joint.hip, gw_crash_shield_joint).  The two stay translation units of their own, a __global__
// wrapper and a launcher each, so that a change to one shield leaves the other code objects alone; the sweeps
// around FearAltCore, their LDS and the rules that keep them sound are stated here once.
#pragma once
#include "cf_env.h"
#include "crash_shield.h"
#include "fear_alt_core.h"
#include "fear_shield.h"

namespace gw {

// Orders one wave's LDS accesses: the LDS serves a wave's instructions in issue order, so what is left to do is
// to keep the compiler from moving an access across this point.  No instruction, no other wave involved.
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One REAL world update (step_preview_kernel's task: the full joint action, eaters 0..K-1, the apples still
// present) of cells `pos` under `act` with actor k playing b, in registers: crash bits | restricted bits << 8.
template <int N, bool LIST>
__device__ __forceinline__ uint32_t real_update(const Params &p, const CtabOk &okv, const int (&pos)[N],
                                                const int (&act)[N], int k, int b, int K, const int (&apple)[MAXN],
                                                uint2 *wl_row) {
    int fin[N], joint[N];
#pragma unroll
    for (int n = 0; n < N; ++n) joint[n] = (n == k) ? b : act[n];
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

// ---------------------------------------------------------------------------------------
// shield_joint_body<N, CRASH> (the rules and the sim counts: include/gridenv.h).  On the wave-per-env scaffold
// (CfEnv) from the preview's record: the env's cells and the joint action (prop, scripted) the next step would
// apply, both clamped to their ranges by CfEnv::begin.  Every lane of the wave keeps the env's current joint
// action `act` in registers.
//   run(sel): FearAltCore's clear and run (csrc/fear_alt_core.h, shared with fear_alt_kernel): the world updates
//     of the actors in `sel` under `act` into their 9-bit valid sets; an actor's [9][N] words of vb are cleared first.
//   row(k, a): FearAltCore's row, the code that computes fear_alt_kernel's table entry.
//   A visit of shielded actor k: run(1 << k); lanes 0-8 store row(k, lane) into s_row; every lane runs
//     fear_shield::pick on s_row and updates its copy of act[k].
//   After the sweeps: the rows of the shielded actors are those of the final joint action if the last sweep
//     changed nothing (every one of its visits saw that joint action), so only the other actors' tasks run;
//     else all K actors' run.  Lane i = (k, a) stores T[k][a]; the lane with a == act[k] also stores
//     actions_out[k] and flags[k] (bit 2 from its own entry).  Lanes 0..N-1 store joint.
// What CRASH adds (with CRASH false none of it is compiled: no real world update, no ballot, s_row not zeroed,
// use_fear and want_table constant true):
//   A visit first runs the crash preview: lanes 0-8 run one real world update each, act with k playing the
//     lane's action; k's own crash bit reaches all lanes as a wave ballot (crash9), no LDS.  The first visit of
//     the env still sees the proposal, so its lane act[k] holds the proposal's outcome (O_prop), handed round by
//     a shuffle.  The FeAR half of the visit runs only with use_fear, and the pick is crash_shield::visit.
//   After the sweeps: the K x 9 crash tasks (k, a) of the FINAL joint action dealt round-robin (K = 8: 72 tasks,
//     lanes 0-7 take a second turn), their own-crash bits collected by one ballot per turn; the task (0, act[0])
//     IS the update of the final joint action, so its lane holds O.  The table only with use_fear or a table to
//     store (want_table), the shielded actors' rows reused only if the visits ran FeAR.  Flags bits 4 and 5;
//     lanes 0..K-1 store crash9; lane 0 the two outcomes.
// What keeps this sound:
//   every trip count and every branch around a wave-wide operation (ballot, shuffle, the LDS ordering) is the
//     same in all 64 lanes;
//   the four waves of a block are four envs that need different numbers of visits: nothing between begin()'s
//     barrier and end()'s is block-wide;
//   one wave owns vb[wave] and s_row[wave] (and a thread its wl row); a wave's LDS accesses are ordered by
//     wave_lds_order();
//   a wave past the env range runs no visit and no task and goes straight to end().
// ---------------------------------------------------------------------------------------
template <int N, bool CRASH>
__device__ __forceinline__ void shield_joint_body(const Params &p, const JointShieldArgs &a) {
    using Core = FearAltCore<N>;
    constexpr bool LIST = Core::LIST;
    constexpr int VBW = Core::VBW;  // per env, sized for K = N
    __shared__ uint32_t vb[CF_WAVES][VBW];
    __shared__ uint2 wl[LIST ? CF_T * N : 1];  // World<N, true> rows (one per thread), both kinds of update
    __shared__ double s_row[CF_WAVES][NA];     // the visited actor's table row
    __shared__ unsigned int s_nsim;
    static_assert(sizeof(uint32_t) * CF_WAVES * VBW + sizeof(uint2) * (LIST ? CF_T * N : 1) +
                          sizeof(double) * CF_WAVES * NA <= 26 * 1024,
                  "static LDS of the joint shields: 26 KiB (fear_alt_kernel's sets and rows plus s_row)");
    CfEnv<N> c;
    // run() clears the sets it fills; a crash-only visit reads s_row without having written it
    c.begin(p, 0, s_nsim, [&] {
        if constexpr (CRASH)
            if (c.lane < NA) s_row[c.wave][c.lane] = 0.0;
    });
    const int tid = threadIdx.x, wave = c.wave, lane = c.lane, K = min(p.K, N);
    const CtabOk okv{c.ctab};
    uint32_t *const vbw = vb[wave];
    uint2 *const wl_row = LIST ? &wl[tid * N] : nullptr;
    const bool use_fear = !CRASH || a.use_fear != 0, want_table = use_fear || a.table != nullptr;
    [[maybe_unused]] int apple[MAXN];  // CRASH: the apples still present
    if constexpr (CRASH) {
        const uint32_t apples = c.live ? (p.st.flags[c.e] & 0xFFu) : 0u;
#pragma unroll
        for (int q = 0; q < MAXN; ++q) apple[q] = (q < K && ((apples >> q) & 1u)) ? p.apples[q] : -1;
    }
    int act[N];  // the current joint action: act[0..K) is `cur` of the rule
#pragma unroll
    for (int n = 0; n < N; ++n) act[n] = c.act[n];
    Core core;
    core.plan(p, c.pos, K);
    int nsim = 0;  // world updates this wave ran

    // the FeAR world updates of the actors in sel (non-zero, bits below K) under `act` into their sets, cleared first
    auto run = [&](uint32_t sel) {
        Core::clear(sel, vbw, lane);
        wave_lds_order();
        nsim += core.run(sel, act, p, okv, c.pos, vbw, wl_row, lane);
        wave_lds_order();
    };
    auto row = [&](int k, int va) { return Core::row(k, va, c.mdr, vbw, c.tab); };

    const uint32_t all_k = (1u << K) - 1u, shielded = a.agents & all_k;
    uint32_t stuck = 0u;
    bool changed = false;  // the last sweep that ran changed an action
    // CRASH only: unavoidable bits, the proposal's outcome, and whether a visit has run (uniform) so that it is known
    [[maybe_unused]] uint32_t unavoidable = 0u, o_prop = 0u;
    [[maybe_unused]] bool have_prop = false;
    if (c.live && shielded) {
        for (int s = 0; s < a.sweeps; ++s) {
            changed = false;
            for (int k = 0; k < K; ++k) {
                if (!((shielded >> k) & 1u)) continue;
                int cur = 0;
#pragma unroll
                for (int q = 0; q < N; ++q)
                    if (q == k) cur = act[q];
                [[maybe_unused]] uint32_t crash9 = 0u;
                if constexpr (CRASH) {
                    uint32_t oc = 0u;
                    if (lane < NA) oc = real_update<N, LIST>(p, okv, c.pos, act, k, lane, K, apple, wl_row);
                    nsim += NA;
                    crash9 = (uint32_t)__ballot((int)((oc >> k) & 1u)) & step_preview::ALL;
                    if (!have_prop) {  // nothing has moved yet: lane cur ran the proposal itself
                        o_prop = (uint32_t)__shfl((int)oc, cur);
                        have_prop = true;
                    }
                }
                if (use_fear) {
                    run(1u << k);
                    if (lane < NA) s_row[wave][lane] = row(k, lane);
                    wave_lds_order();
                }
                const int64_t ek = c.e * p.K + k;
                const float *const pr = a.probs ? a.probs + ((int64_t)k * p.E + c.e) * NA : nullptr;
                crash_shield::Visit r;
                if constexpr (CRASH) {
                    r = crash_shield::visit(s_row[wave], cur, a.mask != nullptr, a.mask ? a.mask[ek] : 0u, crash9, pr,
                                            use_fear, a.tau);
                } else {
                    const fear_shield::Pick q = fear_shield::pick(s_row[wave], cur, a.mask ? a.mask[ek] : 0x1FFu, pr,
                                                                  a.tau, true);
                    r.action = q.action;
                    r.flags = q.flags;
                }
                wave_lds_order();  // s_row is read before the next visit rewrites it
                const int pick = min(max(r.action, 0), NA - 1);
                stuck = (stuck & ~(1u << k)) | ((uint32_t)((r.flags >> 1) & 1) << k);
                if constexpr (CRASH) unavoidable = (unavoidable & ~(1u << k)) | ((uint32_t)((r.flags >> 5) & 1) << k);
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
        [[maybe_unused]] uint64_t own_lo = 0ull, own_hi = 0ull;  // CRASH: the own-crash bits of the tasks (k, a)
        [[maybe_unused]] uint32_t o_fin = 0u;                    // CRASH: the final joint action's outcome
        if constexpr (CRASH) {
            // the own-crash sets of the final joint action, and its outcome from the task (0, act[0])
            const int ntask = K * NA;  // <= 72
            for (int base = 0; base < ntask; base += 64) {
                const int ti = base + lane;
                uint32_t oc = 0u;
                bool own = false;
                if (ti < ntask) {
                    const int k = ti / NA;  // k < K <= N
                    oc = real_update<N, LIST>(p, okv, c.pos, act, k, ti - k * NA, K, apple, wl_row);
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
        }
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
            uint32_t f = (uint32_t)(cur != prop) | (((stuck >> k) & 1u) << 1) |
                         ((uint32_t)(use_fear && sh && t > a.tau) << 2) | ((uint32_t)changed << 3);
            if constexpr (CRASH) f |= (((o_fin >> k) & 1u) << 4) | (((unavoidable >> k) & 1u) << 5);
            if (a.flags) a.flags[ek] = (uint8_t)f;
        }
        if constexpr (CRASH)
            if (a.crash9 && lane < K) a.crash9[c.e * p.K + lane] = (uint16_t)bits9(own_lo, own_hi, lane * NA);
        if (a.joint && lane < N) {
            int v = 0;
#pragma unroll
            for (int q = 0; q < N; ++q)
                if (q == lane) v = act[q];
            a.joint[c.e * N + lane] = v;
        }
        if constexpr (CRASH)
            if (lane == 0) {
                if (a.outcome) a.outcome[c.e] = (uint16_t)o_fin;
                if (a.outcome_prop) a.outcome_prop[c.e] = (uint16_t)o_prop;
            }
    }
    c.end(p, s_nsim, nsim);
}

}  // namespace gw
