// fear_cf.hip -- fear_alt_kernel (gw_set_fear_alt, gw_fear_preview) and feal_kernel (gw_set_feal): the step's
// per-action FeAR table and per-agent FeAL on the wave-per-env scaffold.  A translation unit of its own on the
// shared headers (cf_env.h, fear_alt_core.h), so that the code object of gridenv.hip's step kernels
// does not change with it; gridenv.hip arms and orders the launches (launch_cf: geometry, LDS, span).
#include <hip/hip_runtime.h>

#include "cf_env.h"
#include "dispatch.h"
#include "fear_alt_core.h"
#include "prof.h"

namespace gw {

// ---------------------------------------------------------------------------------------
// fear_alt_kernel (gw_set_fear_alt): the per-action counterfactual FeAR table of a step,
//   fear_alt[e][k][a] = np.sum(Resp) of FeAR_4_one_actor(actor = k) with k playing a,
// from the step's FearRec, on the wave-per-env scaffold (CfEnv).  The env's tasks are those of
// csrc/fear_alt_tasks.h: per actor 9 variants x (1 base + 8 alternatives of each close agent).
// The plan, the tasks and the row arithmetic are FearAltCore's (csrc/fear_alt_core.h, shared with
// fear_shield_joint_kernel): one run over all K actors between begin()'s barrier, before which the
// sets are cleared, and end()'s, after which lane (k, a) reads them.
// ---------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(CF_T) fear_alt_kernel(Params p, double *__restrict__ table) {
    using Core = FearAltCore<N>;
    constexpr bool LIST = Core::LIST;
    constexpr int VBW = Core::VBW;  // per env, sized for K = N
    static_assert(fear_alt::max_per_env(4, 2) == 450 && fear_alt::max_per_env(8, 2) == 1026, "task maxima");
    __shared__ uint32_t vb[CF_WAVES][VBW];
    __shared__ uint2 wl[LIST ? CF_T * N : 1];  // World<N, true> rows (one per thread)
    __shared__ unsigned int s_nsim;
    static_assert(sizeof(uint32_t) * CF_WAVES * VBW + sizeof(uint2) * (LIST ? CF_T * N : 1) <= 26 * 1024,
                  "static LDS of fear_alt_kernel");
    CfEnv<N> c;
    c.begin(p, 0, s_nsim, [&] { for (int i = c.lane; i < VBW; i += 64) vb[c.wave][i] = 0u; });
    const int tid = threadIdx.x, wave = c.wave, lane = c.lane, K = min(p.K, N);
    const CtabOk okv{c.ctab};
    Core core;
    core.plan(p, c.pos, K);
    const int ntask = c.live ? core.run((1u << K) - 1u, c.act, p, okv, c.pos, vb[wave],
                                        LIST ? &wl[tid * N] : nullptr, lane)
                             : 0;
    c.end(p, s_nsim, ntask);
    if (!c.live) return;
    for (int i = lane; i < K * NA; i += 64) {
        const int k = i / NA, a = i - k * NA;
        table[(c.e * p.K + k) * NA + a] = Core::row(k, a, c.mdr, vb[wave], c.tab);
    }
}

// ---------------------------------------------------------------------------------------
// feal_kernel (gw_set_feal): Responsibility.FeAL (custom/Responsibility.py:213-303) of a step for
// every world agent i, from the step's FearRec (pre-step cells, joint action; every agent listed):
//   feal[e][i] = T[vm][va],  vm / va = agent i's valid moves (neither crashed nor restricted,
//   CountValidMovesOfAffected :16-54) over its nine actions b while every other agent plays its
//   MdR / its actual action; the two 9-bit sets go to valid[e][i][0 / 1].
// On the wave-per-env scaffold (CfEnv), with the FeAL table T in the Resp table's place.  Tasks
// [0, 9 N): (i, others actual, b); then 9 per agent whose two variants differ: (i, others MdR, b).
// The variants of i coincide when every other agent's action is its MdR (diff & ~(1 << i) == 0,
// the same in every lane of the wave): that agent's MdR set is a copy of its actual set.
// A task ORs bit b into the set (i, v) in LDS; after the barrier lane i counts and looks T up.
// ---------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(CF_T) feal_kernel(Params p, double *__restrict__ feal,
                                                    uint16_t *__restrict__ valid_out) {
    constexpr bool LIST = N >= GW_LIST_MIN_N;
    constexpr int MAXT = 2 * NA * N;  // tasks per env at most
    static_assert(MAXT <= 144, "18 N tasks per env: at most 3 turns of a wave");
    __shared__ uint32_t vb[CF_WAVES][2 * N];  // [i][v]: 9-bit valid sets, v = 0 others MdR, 1 others actual
    __shared__ uint2 wl[LIST ? CF_T * N : 1];  // World<N, true> rows (one per thread)
    __shared__ unsigned int s_nsim;
    static_assert(sizeof(uint32_t) * CF_WAVES * 2 * N + sizeof(uint2) * (LIST ? CF_T * N : 1) <= 17 * 1024,
                  "static LDS of feal_kernel");
    CfEnv<N> c;
    c.begin(p, 100, s_nsim, [&] { if (c.lane < 2 * N) vb[c.wave][c.lane] = 0u; });
    const int (&pos)[N] = c.pos, (&act)[N] = c.act, (&mdr)[N] = c.mdr;
    const int tid = threadIdx.x, wave = c.wave, lane = c.lane;
    const CtabOk okv{c.ctab};
    uint32_t diff = 0u;  // agents whose action is not their MdR
#pragma unroll
    for (int n = 0; n < N; ++n) diff |= (uint32_t)(act[n] != mdr[n]) << n;
    uint32_t need = 0u;  // agents whose others-MdR variant is a world of its own
#pragma unroll
    for (int i = 0; i < N; ++i) need |= (uint32_t)((diff & ~(1u << i)) != 0u) << i;
    const int ntask = c.live ? NA * (N + __popc(need)) : 0;  // <= MAXT, from registers

    for (int ti = lane; ti < min(ntask, MAXT); ti += 64) {
        const int g = ti / NA, b = ti - g * NA;
        const bool actual = g < N;
        int i = actual ? g : fear_alt::nth_agent(need, g - N);
        i = min(max(i, 0), N - 1);
        int joint[N];
#pragma unroll
        for (int n = 0; n < N; ++n) joint[n] = (n == i) ? b : (actual ? act[n] : mdr[n]);
        const uint32_t valid = cf_valid<N, LIST, false>(p.W, p.w_magic, okv, pos, joint, LIST ? &wl[tid * N] : nullptr);
        if ((valid >> i) & 1u) atomicOr(&vb[wave][2 * i + (actual ? 1 : 0)], 1u << b);
    }
    c.end(p, s_nsim, ntask);
    if (!c.live || lane >= N) return;
    const uint32_t va_set = vb[wave][2 * lane + 1] & 0x1FFu;
    const uint32_t vm_set = ((need >> lane) & 1u) ? (vb[wave][2 * lane] & 0x1FFu) : va_set;
    if (feal) feal[c.e * N + lane] = c.tab[__popc(vm_set) * 10 + __popc(va_set)];
    // the pair [0] others MdR, [1] others actual as one 4-byte store (gw_set_feal checks the alignment)
    if (valid_out) reinterpret_cast<uint32_t *>(valid_out)[c.e * N + lane] = vm_set | (va_set << 16);
}

hipError_t launch_fear_alt(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p, double *table) {
    return with_agents(N, hipErrorInvalidValue, [&](auto n) {
        gwprof::launch(fear_alt_kernel<decltype(n)::value>, grid, block, dyn, s, p, table);
        return hipSuccess;  // a launch error stays in hipGetLastError for the caller (launch_cf)
    });
}

hipError_t launch_feal(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p, double *feal,
                       uint16_t *feal_valid) {
    return with_agents(N, hipErrorInvalidValue, [&](auto n) {
        gwprof::launch(feal_kernel<decltype(n)::value>, grid, block, dyn, s, p, feal, feal_valid);
        return hipSuccess;  // a launch error stays in hipGetLastError for the caller (launch_cf)
    });
}

}  // namespace gw
