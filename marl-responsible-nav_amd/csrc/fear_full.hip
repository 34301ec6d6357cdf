// fear_full.hip -- fear_full_kernel (gw_set_fear_full): the step's N x N responsibility matrix with every
// world agent as actor.  A translation unit of its own on the shared scaffold (cf_env.h), so that the code
// object of gridenv.hip's step kernels does not change with it; gridenv.hip arms and orders the launch.
#include <hip/hip_runtime.h>

#include "cf_env.h"
#include "dispatch.h"
#include "prof.h"

namespace gw {

// ---------------------------------------------------------------------------------------
// fear_full_kernel (gw_set_fear_full): Responsibility.FeAR (custom/Responsibility.py:57-132) of a
// step with every world agent as actor and every agent listed, from the step's FearRec:
//   resp[e][i][j] = T[vm][va] (the Resp table), resp[e][i][i] = 0.0,
//   va = agent j's valid actions b (neither crashed nor restricted) with the action list unchanged
//   except that j plays b, vm = the same with actor i swapped to its MdR; the two 9-bit sets go to
//   valid[e][i][j][0 / 1] (zero on the diagonal).
// On the wave-per-env scaffold (CfEnv).  Tasks [0, 9 N): (j, b), everybody else actual -- the
// reference's "actor moves" list is the unchanged list for every actor, so these serve all N rows.
// Then 9 (N - 1) per actor i off its MdR (bit i of diff, the same in every lane of the wave):
// (i on its MdR, j != i, b).  An actor on its MdR has the unchanged list as its MdR list: its MdR
// sets are copies of the action sets and its row is T[v][v] == 0.0 (gw_create checks the diagonal).
// A task ORs bit b into its set in LDS: vb[j] action sets, vb[N + i N + j] MdR sets; after the
// barrier lane (i, j) counts and looks T up.
// ---------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(CF_T) fear_full_kernel(Params p, double *__restrict__ resp,
                                                         uint16_t *__restrict__ valid_out) {
    constexpr bool LIST = N >= GW_LIST_MIN_N;
    constexpr int NO = N > 1 ? N - 1 : 1;   // affected agents of an MdR group (no such group at N = 1)
    constexpr int MAXT = NA * N * N;        // tasks per env at most: 9 N + 9 (N - 1) N
    constexpr int VBW = N + N * N;          // sets per env: [N] action, [N][N] MdR
    static_assert(N * N <= 64, "one lane per matrix entry");
    static_assert(MAXT <= 576, "9 N^2 tasks per env: at most 9 turns of a wave");
    __shared__ uint32_t vb[CF_WAVES][VBW];
    __shared__ uint2 wl[LIST ? CF_T * N : 1];  // World<N, true> rows (one per thread)
    __shared__ unsigned int s_nsim;
    static_assert(sizeof(uint32_t) * CF_WAVES * VBW + sizeof(uint2) * (LIST ? CF_T * N : 1) <= 18 * 1024,
                  "static LDS of fear_full_kernel");
    CfEnv<N> c;
    c.begin(p, 0, s_nsim, [&] { for (int i = c.lane; i < VBW; i += 64) vb[c.wave][i] = 0u; });
    const int (&pos)[N] = c.pos, (&act)[N] = c.act, (&mdr)[N] = c.mdr;
    const int tid = threadIdx.x, wave = c.wave, lane = c.lane;
    const CtabOk okv{c.ctab};
    uint32_t diff = 0u;  // actors whose action is not their MdR
#pragma unroll
    for (int n = 0; n < N; ++n) diff |= (uint32_t)(act[n] != mdr[n]) << n;
    const int ntask = c.live ? NA * (N + (N - 1) * __popc(diff)) : 0;  // <= MAXT, from registers

    for (int ti = lane; ti < min(ntask, MAXT); ti += 64) {
        const int g = ti / NA, b = ti - g * NA;
        const bool actual = g < N;
        const int q = actual ? 0 : (g - N) / NO, r = actual ? 0 : (g - N) - q * NO;
        // i = -1 in an action group: no agent is swapped to its MdR below, and the set index does not use it
        int i = actual ? -1 : min(max(fear_alt::nth_agent(diff, q), 0), N - 1);
        int j = actual ? g : r + (r >= i ? 1 : 0);
        j = min(max(j, 0), N - 1);
        int joint[N];
#pragma unroll
        for (int n = 0; n < N; ++n) joint[n] = (n == j) ? b : (n == i ? mdr[n] : act[n]);
        const uint32_t valid = cf_valid<N, LIST, false>(p.W, p.w_magic, okv, pos, joint, LIST ? &wl[tid * N] : nullptr);
        if ((valid >> j) & 1u) atomicOr(&vb[wave][actual ? j : N + i * N + j], 1u << b);
    }
    c.end(p, s_nsim, ntask);
    if (!c.live || lane >= N * N) return;
    const int i = lane / N, j = lane - i * N;
    uint32_t va_set = 0u, vm_set = 0u;
    double r = 0.0;
    if (i != j) {
        va_set = vb[wave][j] & 0x1FFu;
        vm_set = ((diff >> i) & 1u) ? (vb[wave][N + lane] & 0x1FFu) : va_set;
        r = c.tab[__popc(vm_set) * 10 + __popc(va_set)];
    }
    if (resp) resp[c.e * (N * N) + lane] = r;
    // the pair [0] actor on its MdR, [1] actual as one 4-byte store (gw_set_fear_full checks the alignment)
    if (valid_out) reinterpret_cast<uint32_t *>(valid_out)[c.e * (N * N) + lane] = vm_set | (va_set << 16);
}

hipError_t launch_fear_full(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                            double *resp_full, uint16_t *resp_valid) {
    return with_agents(N, hipErrorInvalidValue, [&](auto n) {
        gwprof::launch(fear_full_kernel<decltype(n)::value>, grid, block, dyn, s, p, resp_full, resp_valid);
        return hipSuccess;  // a launch error stays in hipGetLastError for the caller (launch_cf)
    });
}

}  // namespace gw
