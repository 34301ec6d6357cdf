// fear_alt_core.h -- internal: the per-action FeAR table of one env on the wave-per-env scaffold (cf_env.h), the
// only copy of what fear_alt_kernel (fear_cf.hip) and fear_shield_joint_kernel (fear_shield_joint.hip) share, so
// that the shield's table stays the next step's fear_alt bit for bit:
//   plan: the actors' close sets and task counts;
//   run:  the tasks of csrc/fear_alt_tasks.h for a set of actors, ORed into the 9-bit valid sets;
//   row:  one table entry from the sets: V counts -> Resp table -> np_sum_row.
// No barrier and no fence in here: how the wave's LDS accesses are ordered around clear / run / row is the
// calling kernel's business (block barriers in fear_alt_kernel, wave scope in the shield).
#pragma once
#include "cf_env.h"
#include "np_sum.h"

namespace gw {

template <int N>
struct FearAltCore {
    static constexpr bool LIST = N >= GW_LIST_MIN_N;
    static constexpr int VBW = fear_alt::bit_words(N, N);  // u32 words of an env's sets [K <= N][9][N], for K = N
    static_assert(VBW == N * NA * N && VBW <= 576, "valid-bit sets: [K <= N][9][N] words per env");
    static_assert(fear_alt::max_per_env(N, N) <= 4104, "tasks per env and run fit an int with room");

    uint32_t close[N];  // actor k's close agents (k included); 0 for k >= K
    int tcount[N];      // actor k's tasks; 0 for k >= K

    // close sets and task counts of the actors k < K (K <= N), in registers
    __device__ __forceinline__ void plan(const Params &p, const int (&pos)[N], int K) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            close[k] = 0u;
            tcount[k] = 0;
            if (k >= K) continue;
#pragma unroll
            for (int n = 0; n < N; ++n)
                if (n == k || manhattan(p, pos[k], pos[n]) <= 5) close[k] |= 1u << n;
            tcount[k] = fear_alt::per_actor(__popc(close[k]));  // popc in 1..N: at most 9 (1 + 8 (N - 1))
        }
    }

    // clears the [9][N] words of the actors in sel (non-zero, bits below K) in the wave's sets vbw
    __device__ __forceinline__ static void clear(uint32_t sel, uint32_t *vbw, int lane) {
        const int lo = (int)__builtin_ctz(sel) * NA * N, hi = (32 - (int)__builtin_clz(sel)) * NA * N;
        for (int i = lo + lane; i < min(hi, VBW); i += 64)
            if ((sel >> (i / (NA * N))) & 1u) vbw[i] = 0u;
    }

    // The world updates of the actors in sel (bits below K) from cells `pos` under the joint action `act`, dealt
    // to the wave's lanes round-robin.  A sim ORs the affected agent's valid bit into the 9-bit set
    // vbw[k][a][j] (bit b = j valid under its action b; the base sim supplies bit act[j], and all nine bits of an
    // agent outside the close set, which stays: 9 * valid(base) as fear_record).  sel, act and the plan are the
    // same in all 64 lanes.  wl_row: the lane's World::lw row (LIST).  Returns the number of tasks.
    __device__ __forceinline__ int run(uint32_t sel, const int (&act)[N], const Params &p, const CtabOk &okv,
                                       const int (&pos)[N], uint32_t *vbw, uint2 *wl_row, int lane) const {
        int ntask = 0;
#pragma unroll
        for (int q = 0; q < N; ++q) ntask += ((sel >> q) & 1u) ? tcount[q] : 0;
        for (int ti = lane; ti < ntask; ti += 64) {
            const fear_alt::Actor at = fear_alt::actor_of<N>(sel, tcount, ti);
            const int k = at.k;
            uint32_t cl = 1u;
#pragma unroll
            for (int q = 0; q < N; ++q)
                if (q == k) cl = close[q];
            const fear_alt::Task tk = fear_alt::decode(at.r, __popc(cl));
            const int j = tk.slot < 0 ? -1 : fear_alt::nth_agent(cl & ~(1u << k), tk.slot);
            int joint[N], b = 0;
#pragma unroll
            for (int n = 0; n < N; ++n) {
                joint[n] = ((cl >> n) & 1u) ? act[n] : 0;
                if (n == k) joint[n] = tk.a;
                if (n == j) joint[n] = b = fear_alt::alternative(tk.bi, act[n]);
            }
            const uint32_t valid = cf_valid<N, LIST, true>(p.W, p.w_magic, okv, pos, joint, wl_row);
            uint32_t *row = &vbw[(k * NA + tk.a) * N];  // k < N, a <= 8: inside the wave's VBW words
            if (j >= 0) {
                if ((valid >> j) & 1u) atomicOr(&row[j], 1u << b);
            } else {
#pragma unroll
                for (int n = 0; n < N; ++n)
                    if (n != k && ((valid >> n) & 1u)) atomicOr(&row[n], ((cl >> n) & 1u) ? (1u << act[n]) : 0x1FFu);
            }
        }
        return ntask;
    }

    // T[k][a] of the sets in vbw: the MdR variant is one of the nine, so Resp[k][j](a) = tab[V(mdr[k], j)][V(a, j)],
    // the row summed as numpy sums the matrix.  tab: the Resp table's 100 f64
    __device__ __forceinline__ static double row(int k, int a, const int (&mdr)[N], const uint32_t *vbw,
                                                 const double *tab) {
        int mk = 0;
#pragma unroll
        for (int q = 0; q < N; ++q)
            if (q == k) mk = mdr[q];
        const uint32_t *rm = &vbw[(k * NA + mk) * N], *ra = &vbw[(k * NA + a) * N];
        double resp[N];
#pragma unroll
        for (int jj = 0; jj < N; ++jj) {
            const int vm = __popc(rm[jj] & 0x1FFu), va = __popc(ra[jj] & 0x1FFu);
            resp[jj] = (jj == k) ? 0.0 : tab[vm * 10 + va];
        }
        return np_sum_row<N>(resp, k);
    }
};

}  // namespace gw
