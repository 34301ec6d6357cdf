// fear_matrix.hip -- fear_matrix_kernel (gw_fear_matrix): FeAR and FeAL of world snapshots the caller supplies.
// A translation unit of its own on the shared header (cf_env.h), so that the code object of gridenv.hip's step
// kernels does not change with it; gridenv.hip checks the arguments, fills FmParams and launches.
#include <hip/hip_runtime.h>

#include "cf_env.h"
#include "dispatch.h"
#include "prof.h"

namespace gw {

// ---------------------------------------------------------------------------------------
// Responsibility.FeAR (custom/Responsibility.py:57-132, every agent as actor) and FeAL
// (:213-303) for n world snapshots, one 128-thread block per snapshot.  Every world update the
// two need is one task (9 per group):  "act" groups jj = 0..N-1 (the action list unchanged,
// agent jj's 9 actions: ValidMoves_action[.][jj] and FeAL's action count of jj), "MdR" groups
// (ii, jj != ii) (actor ii swapped to its MdR: ValidMoves_moveDeRigueur[ii][jj]) and "FeAL"
// groups ii (every other listed agent swapped to its MdR).  Agents outside the action list
// stay and ignore swaps (SwapActionIDs4Agents, grid_world.py:709-726).  Valid-move bits are
// OR-ed into LDS, counted, and mapped through exact host-computed f64 tables.
// ---------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(128) fear_matrix_kernel(FmParams q) {
    constexpr int T = 128, NG = N + N * (N - 1) + N;
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
    uint32_t *ctab = reinterpret_cast<uint32_t *>(dyn);
    __shared__ int s_loc[N], s_act[N], s_mdr[N];
    __shared__ uint32_t s_bits[NG];  // 9-bit valid masks per group
    __shared__ uint32_t s_in;
    const int tid = threadIdx.x;
    const int64_t e = blockIdx.x;
    lds_fill<T>(ctab, q.celltab, q.HW, tid);
    for (int g = tid; g < NG; g += T) s_bits[g] = 0;
    if (tid < N) {
        const int c = q.cells[e * N + tid];
        const int a = q.acts[e * N + tid];
        s_loc[tid] = ((unsigned)c < (unsigned)q.HW) ? c : 0;
        s_act[tid] = ((unsigned)a < (unsigned)NA) ? a : 0;
    }
    if (tid == 0) s_in = q.in_list ? (uint32_t)q.in_list[e] : 0xFFu;
    __syncthreads();
    if (tid < N) {
        const int m = q.mdr ? q.mdr[e * N + tid] : (int)((ctab[s_loc[tid]] >> CT_MDR) & 0xFu);
        s_mdr[tid] = ((unsigned)m < (unsigned)NA) ? m : 0;
    }
    __syncthreads();
    const uint32_t in = s_in;
    const CtabOk okv{ctab};
    for (int t = tid; t < 9 * NG; t += T) {
        const int g = t / 9, b = t - 9 * (t / 9);
        int joint[N], loc[N], fin[N];
#pragma unroll
        for (int n = 0; n < N; ++n) {
            loc[n] = s_loc[n];
            joint[n] = ((in >> n) & 1u) ? s_act[n] : 0;  // defaultAction 'stay' for the unlisted
        }
        int affected;
        if (g < N) {  // action list unchanged
            affected = g;
        } else if (g < N + N * (N - 1)) {  // actor ii -> MdR
            const int idx = g - N, ii = idx / (N - 1), r = idx - ii * (N - 1);
            affected = r + (r >= ii);
#pragma unroll
            for (int n = 0; n < N; ++n)
                if (n == ii && ((in >> n) & 1u)) joint[n] = s_mdr[n];
        } else {  // everybody but ii -> MdR (FeAL)
            affected = g - N - N * (N - 1);
#pragma unroll
            for (int n = 0; n < N; ++n)
                if (n != affected && ((in >> n) & 1u)) joint[n] = s_mdr[n];
        }
#pragma unroll
        for (int n = 0; n < N; ++n)
            if (n == affected && ((in >> n) & 1u)) joint[n] = b;
        // cf_valid's block in place (profiles/fear_scaffold/SUMMARY.md)
        int apple[MAXN];
#pragma unroll
        for (int k = 0; k < MAXN; ++k) apple[k] = -1;
        World<N> w;
        w.init(loc, joint, q.W, q.w_magic);
        uint32_t caught;
        simulate<N, false>(w, okv, 0, apple, caught, fin);
        if (!(((w.crash | w.restr) >> affected) & 1u)) atomicOr(&s_bits[g], 1u << b);
    }
    __syncthreads();
    if (tid < N * N) {
        const int ii = tid / N, jj = tid - ii * N;
        int m = 0, a = 0;
        double r = 0.0;
        if (ii != jj) {
            m = __popc(s_bits[N + ii * (N - 1) + (jj - (jj > ii))]);
            a = __popc(s_bits[jj]);
            r = q.tab[m * 10 + a];
        }
        q.resp[e * N * N + tid] = r;
        if (q.vm) q.vm[e * N * N + tid] = m;
        if (q.va) q.va[e * N * N + tid] = a;
    }
    if (tid < N) {
        const int m = __popc(s_bits[N + N * (N - 1) + tid]), a = __popc(s_bits[tid]);
        if (q.feal) q.feal[e * N + tid] = q.tab[100 + m * 10 + a];
        if (q.feal_vm) q.feal_vm[e * N + tid] = m;
        if (q.feal_va) q.feal_va[e * N + tid] = a;
    }
}

// N >= 2: gw_fear_matrix rejects N = 1, FeAR needs a second agent
hipError_t launch_fear_matrix(int N, int64_t n_blocks, size_t dyn, hipStream_t s, const FmParams &q) {
    return with_agents(N, hipErrorInvalidValue, [&](auto n) -> hipError_t {
        if constexpr (decltype(n)::value >= 2) {
            gwprof::launch(fear_matrix_kernel<decltype(n)::value>, dim3((unsigned)n_blocks), dim3(128), dyn, s, q);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    });
}

}  // namespace gw
