// step_preview.hip -- step_preview_kernel (gw_step_preview): crash bits, restricted bits and env reward of the
// step the next gw_step will run, under each of the nine actions of each RL agent, without moving the world.
// A translation unit of its own on the shared headers (cf_env.h, step_preview.h), so that the code object of
// gridenv.hip's step kernels does not change with it; gridenv.hip owns the preview's record buffer and runs this
// kernel right behind preview_rec_kernel (fear_preview.hip) on it.
#include <hip/hip_runtime.h>

#include "cf_env.h"
#include "dispatch.h"
#include "prof.h"
#include "step_preview.h"

namespace gw {

#include "preview_reward.h"

// ---------------------------------------------------------------------------------------
// step_preview_kernel (gw_step_preview) on the wave-per-env scaffold (CfEnv), from the record
// preview_rec_kernel built: the env's current cells and the joint action the next gw_step will apply.
// Tasks (k, a), k < K, a < 9, dealt to the wave's lanes round-robin (task k * 9 + a; K = N = 8: 72 tasks, a
// second turn for lanes 0-7).  A task runs the REAL world update (the full joint action with k playing a,
// eaters 0..K-1, the apples still present) in registers and stores its own outcome and reward entry; k's own
// crash bit is ORed into a 9-bit set in LDS, from which lane k forms crash9 and the safe mask after end()'s
// barrier.
// ---------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(CF_T) step_preview_kernel(Params p, StepPreviewArgs a) {
    constexpr bool LIST = N >= GW_LIST_MIN_N;
    __shared__ uint32_t c9[CF_WAVES][N];       // [k]: bit a = k itself crashes under a
    __shared__ uint2 wl[LIST ? CF_T * N : 1];  // World<N, true> rows (one per thread)
    __shared__ unsigned int s_nsim;
    static_assert(sizeof(uint32_t) * CF_WAVES * N + sizeof(uint2) * (LIST ? CF_T * N : 1) <= 17 * 1024,
                  "static LDS of step_preview_kernel");
    CfEnv<N> c;
    c.begin(p, 0, s_nsim, [&] { if (c.lane < N) c9[c.wave][c.lane] = 0u; });
    const int tid = threadIdx.x, wave = c.wave, lane = c.lane, K = min(p.K, N);
    const CtabOk okv{c.ctab};
    const int ntask = c.live ? K * NA : 0;
    const uint32_t apples = c.live ? (p.st.flags[c.e] & 0xFFu) : 0u;
    int apple[MAXN];
#pragma unroll
    for (int q = 0; q < MAXN; ++q) apple[q] = (q < K && ((apples >> q) & 1u)) ? p.apples[q] : -1;

    for (int ti = lane; ti < ntask; ti += 64) {
        const int k = ti / NA, b = ti - k * NA;  // k < K <= N
        int joint[N], fin[N];
#pragma unroll
        for (int n = 0; n < N; ++n) joint[n] = (n == k) ? b : c.act[n];
        World<N, LIST> w;
        w.init(c.pos, joint, p.W, p.w_magic);
        if constexpr (LIST) w.lw = &wl[tid * N];
        uint32_t caught;
        simulate<N, true>(w, okv, K, apple, caught, fin);
        const int64_t o = (c.e * p.K + k) * NA + b;
        a.outcome[o] = (uint16_t)((w.crash & 0xFFu) | ((w.restr & 0xFFu) << 8));
        if (a.reward_alt) {
            int fin_k = fin[0], apple_k = p.apples[0];  // selects, not a lane-indexed register array
#pragma unroll
            for (int n = 1; n < N; ++n) {
                fin_k = (n == k) ? fin[n] : fin_k;
                apple_k = (n == k) ? p.apples[n] : apple_k;
            }
            a.reward_alt[o] = preview_reward(p, k, apples, caught, w.crash, fin_k, apple_k,
                                             p.st.prev[(int64_t)k * p.E + c.e]);
        }
        if ((w.crash >> k) & 1u) atomicOr(&c9[wave][k], 1u << b);
    }
    c.end(p, s_nsim, ntask);
    if (!c.live || lane >= K) return;
    const int64_t ek = c.e * p.K + lane;
    const uint32_t crash9 = c9[wave][lane] & step_preview::ALL;
    if (a.crash9) a.crash9[ek] = (uint16_t)crash9;
    if (a.safe_mask)
        a.safe_mask[ek] = (uint16_t)step_preview::safe_mask(a.mask != nullptr, a.mask ? a.mask[ek] : 0u, crash9);
}

hipError_t launch_step_preview(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                               const StepPreviewArgs &a) {
    return with_agents(N, hipErrorInvalidValue, [&](auto n) {
        gwprof::launch(step_preview_kernel<decltype(n)::value>, grid, block, dyn, s, p, a);
        return hipSuccess;  // a launch error stays in hipGetLastError for the caller (launch_cf)
    });
}

}  // namespace gw
