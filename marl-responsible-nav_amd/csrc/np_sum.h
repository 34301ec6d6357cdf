// np_sum.h -- internal: numpy's float64 sum of a Resp matrix with one non-zero row, shared by gridenv.hip's FeAR
// kernels and fear_shield_joint.hip.  gridenv.hip includes it where the function used to stand, so its own
// kernels compile as before.
#pragma once
#include <hip/hip_runtime.h>

namespace gw {

// numpy float64 sum (0.0 + pairwise_sum) of an N*N matrix whose only non-zero row is `row`
// (np.sum(FeAR_vals), custom/ma_customenv.py:252).  Zeros never change a partial sum here
// (no -0.0 can occur), so only the row's terms are accumulated, in numpy's order.
template <int N>
__device__ __forceinline__ double np_sum_row(const double (&v)[N], int row) {
    constexpr int n = N * N;
    if (n < 8) {
        double res = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) res = __dadd_rn(res, v[j]);
        return __dadd_rn(0.0, res);
    } else {
        static_assert(N * N <= 128, "N <= 11");
        double r[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) r[q] = 0.0;
        constexpr int main_end = n - (n % 8);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int idx = row * N + j;
            if (idx < main_end) {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if ((idx & 7) == q) r[q] = __dadd_rn(r[q], v[j]);
            }
        }
        double res = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), __dadd_rn(r[2], r[3])),
                               __dadd_rn(__dadd_rn(r[4], r[5]), __dadd_rn(r[6], r[7])));
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int idx = row * N + j;
            if (idx >= main_end) res = __dadd_rn(res, v[j]);
        }
        return __dadd_rn(0.0, res);
    }
}

}  // namespace gw
