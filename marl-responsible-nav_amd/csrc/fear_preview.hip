// fear_preview.hip -- preview_rec_kernel (gw_fear_preview): the FearRec of the step the next gw_step will run,
// built from the env's current state without moving the world.  A translation unit of its own on the shared
// headers (cf_env.h, draw_action.h), so that the code object of gridenv.hip's step kernels does not change with
// it; gridenv.hip owns the preview's record buffer and runs fear_alt_kernel (fear_cf.hip) on it right behind this
// kernel.
#include <hip/hip_runtime.h>

#include "cf_env.h"
#include "dispatch.h"
#include "philox.h"
#include "prof.h"

namespace gw {

#include "draw_action.h"

// ---------------------------------------------------------------------------------------
// preview_rec_kernel (gw_fear_preview): one thread per env.  Loads the env's cells (pos[n][e], structure of
// arrays: coalesced), step count and episode, draws the N actions exactly as the step kernels will (draw_action
// with p.rl / p.scripted or the Philox counters (seed; global env, episode, t, agent); the cell table and the
// CDFs read from global memory) and stores the record in store_fear_rec's layout into p.fwork, which here is
// the preview's own buffer.  The fields fear_alt_kernel does not read (done, env rewards, bonus) are zero.
// actions / mdr_out [E][N] or null: the joint action and the cells' MdR, as gw_step_out.actions / .mdr.
// ---------------------------------------------------------------------------------------
constexpr int PV_T = 256;

template <int N>
__global__ void __launch_bounds__(PV_T) preview_rec_kernel(Params p, int32_t *__restrict__ actions,
                                                           int32_t *__restrict__ mdr_out) {
    const int64_t e = p.e_begin + (int64_t)blockIdx.x * PV_T + threadIdx.x;
    if (e >= p.e_end) return;
    int pos[N], act[N];
#pragma unroll
    for (int n = 0; n < N; ++n) pos[n] = min(max(p.st.pos[(int64_t)n * p.E + e], 0), p.HW - 1);
    const int t = p.st.t[e];
    const uint32_t episode = p.st.episode[e];
#pragma unroll
    for (int n = 0; n < N; ++n) act[n] = draw_action(p, e, n, episode, t, pos[n], p.tb.celltab, nullptr);
    int rew[MAXN];
#pragma unroll
    for (int k = 0; k < MAXN; ++k) rew[k] = 0;
    store_fear_rec<N>(p, e, pos, act, rew, 0u, false);
#pragma unroll
    for (int n = 0; n < N; ++n) {
        if (actions) actions[e * N + n] = act[n];
        if (mdr_out) mdr_out[e * N + n] = min((int)((p.tb.celltab[pos[n]] >> CT_MDR) & 0xFu), NA - 1);
    }
}

hipError_t launch_preview_rec(int N, hipStream_t s, const Params &p, int32_t *actions, int32_t *mdr) {
    const int64_t count = p.e_end - p.e_begin;
    if (count <= 0) return hipSuccess;
    const dim3 grid((unsigned)((count + PV_T - 1) / PV_T)), block(PV_T);
    return with_agents(N, hipErrorInvalidValue, [&](auto n) {
        gwprof::launch(preview_rec_kernel<decltype(n)::value>, grid, block, 0, s, p, actions, mdr);
        return hipSuccess;  // a launch error stays in hipGetLastError for the caller (launch_cf)
    });
}

}  // namespace gw
