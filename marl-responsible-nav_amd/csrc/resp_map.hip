// resp_map.hip -- gw_resp_map_accum (include/rollout_ops.h): where on the grid agents restrict each other.
// One step's N x N valid-action sets (gw_set_fear_full's resp_valid) binned by the agents' pre-move cells
// into integer counts per (plane, cell, vm, va); the host turns the counts into sums of Resp = T[vm][va] in
// a fixed order (marlnav/resp_map.py), so the totals do not depend on the order the increments arrive in.
// A translation unit of its own: no other kernel's code object changes with it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "resp_map.h"
#include "rollout_ops.h"

namespace {

constexpr int RM_T = 256;

// One thread per (pair = i N + j, env e), flat index t = pair * E + e: consecutive lanes are consecutive envs,
// so cells[i][e], cells[j][e] and active[e] are read coalesced and all but the waves that straddle a multiple
// of E share i and j (the diagonal test is uniform there).  The pair's two sets are one 4-byte load, 4 N^2 bytes apart between lanes: the N^2
// passes over an env's row re-read the lines from L2.  Increments are 64-bit global atomic adds whose result
// is not used (no-return global_atomic_add_x2); every index comes from resp_map::bins / clamp_cell.
__global__ void __launch_bounds__(RM_T) resp_map_kernel(const uint32_t *__restrict__ valid,
                                                        const int32_t *__restrict__ cells,
                                                        const uint8_t *__restrict__ active,
                                                        unsigned long long *__restrict__ counts,
                                                        unsigned long long *__restrict__ visits, int E, int N,
                                                        int HW) {
    const int64_t t = (int64_t)blockIdx.x * RM_T + threadIdx.x;
    if (t >= (int64_t)E * N * N) return;
    const int pair = (int)(t / E);
    const int e = (int)(t - (int64_t)pair * E);
    if (active && !active[e]) return;
    const int i = pair / N, j = pair - i * N;
    const int32_t cell_i = cells[(int64_t)i * E + e];
    if (i == j) {  // once per (e, i)
        if (visits) atomicAdd(&visits[resp_map::clamp_cell(cell_i, HW)], 1ull);
        return;
    }
    const int32_t cell_j = cells[(int64_t)j * E + e];
    const uint32_t word = valid[(int64_t)e * (N * N) + pair];
    const resp_map::Bins b = resp_map::bins(word, cell_i, cell_j, HW);
    atomicAdd(&counts[b.caused], 1ull);
    atomicAdd(&counts[b.received], 1ull);
}

}  // namespace

extern "C" gw_status gw_resp_map_accum(const uint16_t *resp_valid, const int32_t *cells, const uint8_t *active,
                                       uint64_t *counts, uint64_t *visits, int32_t E, int32_t N, int32_t HW,
                                       void *stream) {
    const char *bad = nullptr;
    if (!resp_valid || !cells || !counts) bad = "null resp_valid, cells or counts";
    else if (N < 2 || N > GW_MAX_AGENTS) bad = "N outside 2..8";
    else if (E <= 0 || HW <= 0) bad = "E <= 0 or HW <= 0";
    else if ((reinterpret_cast<uintptr_t>(resp_valid) & 3u) || (reinterpret_cast<uintptr_t>(counts) & 7u) ||
             (reinterpret_cast<uintptr_t>(visits) & 7u) || (reinterpret_cast<uintptr_t>(cells) & 3u))
        bad = "misaligned pointer (resp_valid and cells 4 bytes, counts and visits 8)";
    if (bad) {
        gw_set_last_error((std::string("gw_resp_map_accum: ") + bad).c_str());
        return GW_ERR_ARG;
    }
    const int64_t blocks = ((int64_t)E * N * N + RM_T - 1) / RM_T;  // <= 2^31 * 64 / 256: fits a grid
    hipLaunchKernelGGL(resp_map_kernel, dim3((unsigned)blocks), dim3(RM_T), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint32_t *>(resp_valid), cells, active,
                       reinterpret_cast<unsigned long long *>(counts), reinterpret_cast<unsigned long long *>(visits),
                       (int)E, (int)N, (int)HW);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        gw_set_last_error((std::string("gw_resp_map_accum: ") + hipGetErrorString(err)).c_str());
        return GW_ERR_HIP;
    }
    return GW_OK;
}
