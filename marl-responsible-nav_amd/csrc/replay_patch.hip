// replay_patch.hip — gw_replay_gather_desc_patch (include/rollout_ops.h): the replay-ring sample of a
// local-window rollout whose ring holds obs descriptors only.  Each sampled (transition, env) row's P x P
// windows are expanded straight from the two 48-byte descriptors into the learner's rows, so the rollout
// step needs no window writer (gw_obs_patch / gw_step_patch_next) and the ring no K * P * P floats per
// env and slot.  The values restate gw_obs_patch's windows (patch_ops.hip: rows / cols -P/2 .. P-1-P/2
// around agent k's own cell in that half of that descriptor, -1 outside the grid, the map value else,
// then desc_patches' cells in slot order) bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "desc_rows.h"
#include "philox.h"
#include "rollout_ops.h"

namespace {

constexpr int GP_T = 256;                      // threads per block: one block per (row b, agent k)
constexpr int GP_SLOTS = GW_MAX_AGENTS + 1;    // patched cells of one obs: the apple, then N agents
constexpr int GP_MAXP = 129;                   // gw_obs_patch's largest window
constexpr int GP_MAXHW = 4096;                 // gw_replay_gather_desc's cell limit

struct WindowGeom {
    int H, W, P;
    uint32_t m_p;  // min(2^32 - 1, ceil(2^32 / P)): i / P == __umulhi(i, m_p) for every i < P * P, P <= 129
                   // (P == 1: i == 0 only); tests/test_replay_desc_patch_cpu.py checks every (P, i)
};

// Loads in three waves: (t_dev, u / env or the Philox draw, the apple's map value); (done, both descriptors
// whole, probs, reward, term); the map cells of both windows (one iteration of the cell loop up to P = 16;
// wider windows repeat it, every iteration independent of the one before).  Everything read from memory is
// clamped before it indexes anything: t through the modulo, e to [0, E), descriptor and apple cells to the
// map (a cell outside it patches nothing and centres on the last cell).
__global__ void __launch_bounds__(GP_T) replay_gather_desc_patch_kernel(
    DescSrc q, WindowGeom g, const uint32_t *__restrict__ desc, const float *__restrict__ probs,
    const double *__restrict__ reward, const uint8_t *__restrict__ term, const uint8_t *__restrict__ done,
    const int64_t *__restrict__ t_dev, const float *__restrict__ u, const int64_t *__restrict__ env, int64_t S,
    int64_t B, float *__restrict__ state, float *__restrict__ next_state, float *__restrict__ probs_out,
    double *__restrict__ reward_out, uint8_t *__restrict__ term_out, int64_t *__restrict__ tr_out,
    float *__restrict__ x_out, float *__restrict__ xn_out, uint64_t seed, const int32_t *__restrict__ ctr) {
    __shared__ int s_pc[2][GP_SLOTS];    // desc_patches' cells, then each cell's window offset (-1: outside)
    __shared__ float s_pv[2][GP_SLOTS];
    __shared__ int s_np[2], s_ctr[2];    // patch counts; window centres, row << 16 | col
    const int64_t b = blockIdx.x;
    const int k = blockIdx.y, K = q.K, tid = threadIdx.x;
    const int64_t E = q.E;
    const int H = g.H, W = g.W, P = g.P, PP = P * P, half = P / 2, HW = q.HW;
    // wave 1
    const int64_t t = t_dev[0];
    float ub;
    int64_t e;
    if (u) {
        ub = u[b];
        e = env[b];
    } else {  // in-kernel draws, as replay_gather_desc_kernel: Philox(seed; row, *ctr, tag)
        const uint4 r = gwrng::philox((uint32_t)b, (uint32_t)ctr[0], gwrng::TAG_SAMPLE, 0u, (uint32_t)seed,
                                      (uint32_t)(seed >> 32));
        ub = gwrng::unit(r.x);
        e = (int64_t)(((uint64_t)r.y * (uint64_t)E) >> 32);
    }
    e = e < 0 ? 0 : (e > E - 1 ? E - 1 : e);
    const int ack = q.apples[k];
    const float apple_map = (ack >= 0 && ack < HW) ? q.base[ack] : 0.0f;
    const int64_t n = t < 1 ? 1 : (t > S - 1 ? S - 1 : t);
    int64_t step = (int64_t)(ub * (float)n);  // as replay_gather_kernel (torch's draw)
    if (step > n - 1) step = n - 1;
    if (step < 0) step = 0;
    int64_t tr = (t - 1 - step) % S;
    if (tr < 0) tr += S;
    const int64_t nx = (tr + 1) % S;
    // wave 2: descriptor slot j holds the obs that a dense ring keeps in obs slot j; the terminal obs of
    // the transition in slot tr is the terminal half of descriptor slot tr + 1
    const bool dn = done[tr * E + e] != 0;
    if (tid < 2) {
        const uint4 *d4 = reinterpret_cast<const uint4 *>(desc + ((tid == 0 ? tr : nx) * E + e) * DESC_WORDS);
        const uint4 a = d4[0], bq = d4[1], c = d4[2];
        const uint32_t d[DESC_WORDS] = {a.x, a.y, a.z, a.w, bq.x, bq.y, bq.z, bq.w, c.x, c.y, c.z, c.w};
        const int np = desc_patches(q, d, tid == 0 ? 0 : (dn ? 1 : 0), k, apple_map, s_pc[tid], s_pv[tid]);
        s_np[tid] = np;
        // the window's centre: agent k's own cell in that half (the spawn cell of a reset-encoded obs, the
        // terminal cell of the terminal half); agents 0 .. N - 1 are the list's last N entries
        int cen = s_pc[tid][np - q.N + k];
        cen = cen > HW - 1 ? HW - 1 : cen;
        const int cr = cen / W, cc = cen - cr * W;
        s_ctr[tid] = (cr << 16) | cc;
        for (int j = 0; j < np; ++j) {  // each patched cell as a window offset, once
            const int pcell = s_pc[tid][j];
            const int rr = pcell / W;
            const int wr = rr - cr + half, wc = pcell - rr * W - cc + half;
            const bool in = pcell >= 0 && pcell < HW && (unsigned)wr < (unsigned)P && (unsigned)wc < (unsigned)P;
            s_pc[tid][j] = in ? wr * P + wc : -1;
        }
    }
    const int64_t ldx = (int64_t)K * PP + (int64_t)K * 9;
    if (tid < 9) {
        const float pv = probs[((tr * K + k) * E + e) * 9 + tid];
        probs_out[(k * B + b) * 9 + tid] = pv;
        if (x_out) x_out[b * ldx + (int64_t)K * PP + k * 9 + tid] = pv;
    }
    if (k == 0 && tid >= 64 && tid < 64 + K) {
        const int j = tid - 64;
        reward_out[b * K + j] = reward[(tr * E + e) * K + j];
        term_out[b * K + j] = term[(tr * E + e) * K + j];
    }
    if (k == 0 && tid == 128 && tr_out) tr_out[b] = tr;
    __syncthreads();
    const int np0 = s_np[0], np1 = s_np[1];
    const int r0 = (s_ctr[0] >> 16) - half, c0 = (s_ctr[0] & 0xFFFF) - half;
    const int r1 = (s_ctr[1] >> 16) - half, c1 = (s_ctr[1] & 0xFFFF) - half;
    // state / next_state may be NULL when the critic rows are all the caller needs
    float *so = state ? state + (k * B + b) * PP : nullptr;
    float *no = next_state ? next_state + (k * B + b) * PP : nullptr;
    float *xo = x_out ? x_out + b * ldx + (int64_t)k * PP : nullptr;
    float *xno = xn_out ? xn_out + b * ldx + (int64_t)k * PP : nullptr;
    // wave 3: the map cells of both windows, then the overrides (a later slot wins, as the obs writer's)
    for (int i = tid; i < PP; i += GP_T) {
        const int wr = (int)__umulhi((uint32_t)i, g.m_p), wc = i - wr * P;
        const int sr = r0 + wr, sc = c0 + wc, nr = r1 + wr, nc = c1 + wc;
        const bool sin = (unsigned)sr < (unsigned)H && (unsigned)sc < (unsigned)W;
        const bool nin = (unsigned)nr < (unsigned)H && (unsigned)nc < (unsigned)W;
        float sv = sin ? q.base[sr * W + sc] : -1.0f;
        float nv = nin ? q.base[nr * W + nc] : -1.0f;
        for (int j = 0; j < np0; ++j)
            if (s_pc[0][j] == i) sv = s_pv[0][j];
        for (int j = 0; j < np1; ++j)
            if (s_pc[1][j] == i) nv = s_pv[1][j];
        if (so) so[i] = sv;
        if (no) no[i] = nv;
        if (xo) xo[i] = sv;
        if (xno) xno[i] = nv;
    }
}

gw_status bad(const char *msg) {
    gw_set_last_error((std::string("gw_replay_gather_desc_patch: ") + msg).c_str());
    return GW_ERR_ARG;
}

}  // namespace

extern "C" gw_status gw_replay_gather_desc_patch(const gw_obs_source *src, const uint32_t *desc, const float *probs,
                                                 const double *reward, const uint8_t *term, const uint8_t *done,
                                                 const int64_t *t_dev, const float *u, const int64_t *env, int64_t S,
                                                 int64_t B, int32_t P, float *state, float *next_state,
                                                 float *probs_out, double *reward_out, uint8_t *term_out,
                                                 int64_t *tr_out, float *x_out, float *xn_out, uint64_t seed,
                                                 const int32_t *ctr, void *stream) {
    if (!src || !src->base || !desc || !probs || !reward || !term || !done || !t_dev)
        return bad("null source, descriptor ring or ring tensor");
    if ((!u != !env) || (!u && !ctr)) return bad("need u and env together, or ctr for the in-kernel draws");
    if ((!state || !next_state) && (!x_out || !xn_out))
        return bad("state / next_state may be NULL only when x_out and xn_out are given");
    if (!probs_out || !reward_out || !term_out) return bad("null probs_out, reward_out or term_out");
    if (P < 1 || P > GP_MAXP) return bad("need 1 <= P <= 129");
    if (src->H <= 0 || src->W <= 0 || (int64_t)src->H * src->W > GP_MAXHW) return bad("need 1 <= H * W <= 4096");
    if (S < 2 || src->K <= 0 || src->K > GW_MAX_AGENTS || src->N < src->K || src->N > GW_MAX_AGENTS ||
        src->E <= 0 || B < 0 || B > 0x7fffffff)
        return bad("bad S, K, N, E or B");
    if (reinterpret_cast<uintptr_t>(desc) & 15u) return bad("desc not 16-byte aligned");
    for (int k = 0; k < src->K; ++k)
        if (src->apples[k] >= src->H * src->W) return bad("apple cell outside the map");
    if (B == 0) return GW_OK;
    DescSrc q;
    q.base = src->base;
    for (int k = 0; k < GW_MAX_AGENTS; ++k) q.apples[k] = src->apples[k];
    q.N = src->N;
    q.K = src->K;
    q.HW = src->H * src->W;
    q.variant = src->variant;
    q.E = src->E;
    WindowGeom g;
    g.H = src->H;
    g.W = src->W;
    g.P = P;
    const uint64_t m = (0x100000000ull + (uint64_t)P - 1) / (uint64_t)P;
    g.m_p = m > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)m;
    hipLaunchKernelGGL(replay_gather_desc_patch_kernel, dim3((unsigned)B, (unsigned)q.K), dim3(GP_T), 0,
                       static_cast<hipStream_t>(stream), q, g, desc, probs, reward, term, done, t_dev, u, env, S, B,
                       state, next_state, probs_out, reward_out, term_out, tr_out, x_out, xn_out, seed, ctr);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        gw_set_last_error((std::string("gw_replay_gather_desc_patch: ") + hipGetErrorString(err)).c_str());
        return GW_ERR_HIP;
    }
    return GW_OK;
}
