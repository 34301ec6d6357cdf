// resp_footprint.hip -- gw_resp_footprint_accum (include/rollout_ops.h): how far, and in which direction, an
// action takes feasible actions away from others.  One step's N x N valid-action sets (gw_set_fear_full's
// resp_valid) binned by the actor's action and the affected agent's offset from the actor into integer counts
// per (plane, action, offset, vm, va); the host turns the counts into sums of Resp = T[vm][va] in a fixed order
// (marlnav/resp_footprint.py), so the totals do not depend on the order the increments arrive in.
// A translation unit of its own: no other kernel's code object changes with it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "resp_footprint.h"
#include "rollout_ops.h"

namespace {

constexpr int RF_T = 256;

// resp_map_kernel's form (csrc/resp_map.hip): one thread per (pair = i N + j, env e), flat index
// t = pair * E + e, so consecutive lanes are consecutive envs: cells[i][e], cells[j][e], active[e] and
// crash_bits[e] are read coalesced, actions[e][i] at a stride of N ints, the pair's two sets as one 4-byte load.
// The diagonal thread (i == j) counts the actor-step into visits[a_i].
// Equal bins are merged inside the wave before the atomics: the lanes that hold the same bin elect one lane,
// which adds the popcount of the match ballot (and, into the crash plane, the popcount of the matching lanes
// whose affected agent crashed) with one 64-bit global atomic add without return; the loop runs until no lane
// is left, its trip count wave-uniform.  A diagonal lane's key is 9 O 100 + a_i, so the visits (nine addresses)
// merge in the same loop.  At 65,536 envs of grid32 a launch's 1.05 M increments fall into about 9,300 bins:
// one atomic per increment took 1,983 us there, this form 385 us (profiles/resp_footprint).
// Every index comes from resp_footprint::bin / action9.
__global__ void __launch_bounds__(RF_T) resp_footprint_kernel(
    const uint32_t *__restrict__ valid, const int32_t *__restrict__ cells, const int32_t *__restrict__ actions,
    const uint8_t *__restrict__ crash_bits, const uint8_t *__restrict__ active,
    unsigned long long *__restrict__ counts, unsigned long long *__restrict__ visits, int E, int N, int W, int HW,
    int R) {
    const int64_t t = (int64_t)blockIdx.x * RF_T + threadIdx.x;
    const int plane = resp_footprint::NA * resp_footprint::offsets(R) * (resp_footprint::NV * resp_footprint::NV);
    int key = -1;  // the increment this lane holds: a bin of plane 0, plane + a_i for a visit, -1 for none
    bool crashed = false;
    if (t < (int64_t)E * N * N) {
        const int pair = (int)(t / E);
        const int e = (int)(t - (int64_t)pair * E);
        if (!active || active[e]) {
            const int i = pair / N, j = pair - i * N;
            const int32_t a_i = actions[(int64_t)e * N + i];
            if (i == j) {  // once per (e, i)
                if (visits) key = plane + resp_footprint::action9(a_i);
            } else {
                const int32_t cell_i = cells[(int64_t)i * E + e], cell_j = cells[(int64_t)j * E + e];
                const uint32_t word = valid[(int64_t)e * (N * N) + pair];
                key = (int)resp_footprint::bin(word, cell_i, cell_j, a_i, W, HW, R);
                crashed = crash_bits && ((crash_bits[e] >> j) & 1);
            }
        }
    }
    const int lane = (int)__lane_id();
    uint64_t left = __ballot(key >= 0);
    while (left) {  // (left is the same in every lane)
        const int lead = __ffsll((unsigned long long)left) - 1;
        const int k = __shfl(key, lead);
        const uint64_t same = __ballot(key == k);  // (k >= 0: only lanes that hold an increment match)
        const uint64_t hit = __ballot(key == k && crashed);
        if (lane == lead) {
            if (k >= plane) {
                atomicAdd(&visits[k - plane], (unsigned long long)__popcll(same));
            } else {
                atomicAdd(&counts[k], (unsigned long long)__popcll(same));
                if (hit) atomicAdd(&counts[plane + k], (unsigned long long)__popcll(hit));
            }
        }
        left &= ~same;
    }
}

}  // namespace

extern "C" gw_status gw_resp_footprint_accum(const uint16_t *resp_valid, const int32_t *cells, const int32_t *actions,
                                             const uint8_t *crash_bits, const uint8_t *active, uint64_t *counts,
                                             uint64_t *visits, int32_t E, int32_t N, int32_t H, int32_t W, int32_t R,
                                             void *stream) {
    const char *bad = nullptr;
    if (!resp_valid || !cells || !actions || !counts) bad = "null resp_valid, cells, actions or counts";
    else if (N < 2 || N > GW_MAX_AGENTS) bad = "N outside 2..8";
    else if (E <= 0 || H <= 0 || W <= 0) bad = "E <= 0, H <= 0 or W <= 0";
    else if ((int64_t)H * W > INT32_MAX) bad = "H * W does not fit the cells' int32";
    else if (R < 1 || R > 15) bad = "R outside 1..15";
    else if ((reinterpret_cast<uintptr_t>(resp_valid) & 3u) || (reinterpret_cast<uintptr_t>(counts) & 7u) ||
             (reinterpret_cast<uintptr_t>(visits) & 7u) || (reinterpret_cast<uintptr_t>(cells) & 3u) ||
             (reinterpret_cast<uintptr_t>(actions) & 3u))
        bad = "misaligned pointer (resp_valid, cells and actions 4 bytes, counts and visits 8)";
    if (bad) {
        gw_set_last_error((std::string("gw_resp_footprint_accum: ") + bad).c_str());
        return GW_ERR_ARG;
    }
    const int64_t blocks = ((int64_t)E * N * N + RF_T - 1) / RF_T;  // <= 2^31 * 64 / 256: fits a grid
    hipLaunchKernelGGL(resp_footprint_kernel, dim3((unsigned)blocks), dim3(RF_T), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<const uint32_t *>(resp_valid), cells, actions,
                       crash_bits, active, reinterpret_cast<unsigned long long *>(counts),
                       reinterpret_cast<unsigned long long *>(visits), (int)E, (int)N, (int)W, (int)(H * W), (int)R);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        gw_set_last_error((std::string("gw_resp_footprint_accum: ") + hipGetErrorString(err)).c_str());
        return GW_ERR_HIP;
    }
    return GW_OK;
}
