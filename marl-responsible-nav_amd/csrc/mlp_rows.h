// mlp_rows.h — what the two MADDPG learners (maddpg_dense.hip, maddpg_desc.hip) share: the per-row
// layout of a 16-row block through a K-stacked MLP in marlnav/actor.py's StackedMLPActors layout
// (in -> 128 -> LayerNorm -> ReLU -> 128 -> LayerNorm -> ReLU -> out).  A row = 16 lanes, lane g holds
// features 8 g .. 8 g + 7; LayerNorm sums are 16-lane butterflies; the 128 x 128 layer runs on
// v_mfma_f32_16x16x4_f32 with W2 read from L2.  Everything is f32 with fixed summation orders.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "learner_ops.h"
#include "philox.h"

namespace {

constexpr int HID = 128, NA = 9, RB = 16, TILE_R = 128, MAXK = GW_MAX_AGENTS;
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr float LN_EPS = 1e-5f, G_EPS = 1e-20f;

// ---- host: argument checks both learners' entry points make -----------------------------------
inline gw_status fail(gw_status s, const std::string &msg) {
    gw_set_last_error(msg.c_str());
    return s;
}

inline gw_status check_net(const gw_mlp_actors &n, int K, int in_dim, int out, const std::string &w) {
    if (n.K != K || n.in_dim != in_dim || n.hidden != HID || n.n_actions != out || !n.layer_norm)
        return fail(GW_ERR_ARG, w + ": network shape (needs K, in_dim, hidden 128, LayerNorm, out)");
    if (!n.w1 || !n.b1 || !n.ln1_w || !n.ln1_b || !n.w2 || !n.b2 || !n.ln2_w || !n.ln2_b || !n.w3 || !n.b3)
        return fail(GW_ERR_ARG, w + ": null parameter");
    if ((reinterpret_cast<uintptr_t>(n.w1) | reinterpret_cast<uintptr_t>(n.w2)) & 15u)
        return fail(GW_ERR_ARG, w + ": w1 / w2 must be 16-byte aligned");
    return GW_OK;
}

// ---- per-row helpers (a row = 16 lanes, lane g holds features 8 g .. 8 g + 7) ---------------------
// v from the lane the DPP control names (within the lane's 16-lane row)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
// over the row's 16 lanes, a butterfly on DPP lane moves (VALU, no LDS round trip): pairs (xor 1),
// quads (xor 2), half rows (mirror within 8) and rows (mirror within 16); every lane ends with the
// same sum (each step adds two equal-valued partials in either order), the xor butterfly's values
__device__ __forceinline__ float row_sum(float v) {
    v += dpp_f<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v += dpp_f<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v += dpp_f<0x141>(v);  // row_half_mirror
    v += dpp_f<0x140>(v);  // row_mirror
    return v;
}

struct Mlp {  // one agent's parameters (pointers already offset to agent k)
    const float *w1, *b1, *lw1, *lb1, *w2, *b2, *lw2, *lb2, *w3, *b3;
};
__device__ __forceinline__ Mlp mlp_k(const gw_mlp_actors &n, int k, int in_dim, int out) {
    Mlp m;
    m.w1 = n.w1 + (int64_t)k * in_dim * HID;
    m.b1 = n.b1 + k * HID;
    m.lw1 = n.ln1_w + k * HID;
    m.lb1 = n.ln1_b + k * HID;
    m.w2 = n.w2 + (int64_t)k * HID * HID;
    m.b2 = n.b2 + k * HID;
    m.lw2 = n.ln2_w + k * HID;
    m.lb2 = n.ln2_b + k * HID;
    m.w3 = n.w3 + (int64_t)k * HID * out;
    m.b3 = n.b3 + k * out;
    return m;
}

// LayerNorm (biased variance, eps 1e-5) + affine + ReLU of the 8 features z; xhat / relu output
__device__ __forceinline__ void ln_relu(const float z[8], const float *lw, const float *lb, int g, float xh[8],
                                        float y[8], float &rstd_out) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += z[i];
    const float mean = row_sum(s) * (1.0f / HID);
    float v = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) v = fmaf(z[i] - mean, z[i] - mean, v);
    const float rstd = rsqrtf(row_sum(v) * (1.0f / HID) + LN_EPS);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        xh[i] = (z[i] - mean) * rstd;
        const float o = xh[i] * lw[8 * g + i] + lb[8 * g + i];
        y[i] = o > 0.0f ? o : 0.0f;
    }
    rstd_out = rstd;
}

// backward of ln_relu: gy = grad at the ReLU output; gv = gy * (y > 0) (the affine output's
// gradient, kept for the LayerNorm parameter gradients); dz = rstd (dxh - mean(dxh) - xh mean(dxh xh))
__device__ __forceinline__ void ln_relu_bwd(const float gy[8], const float y[8], const float xh[8], float rstd,
                                            const float *lw, int g, float gv[8], float dz[8]) {
    float dx[8], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        gv[i] = y[i] > 0.0f ? gy[i] : 0.0f;
        dx[i] = gv[i] * lw[8 * g + i];
        s1 += dx[i];
        s2 = fmaf(dx[i], xh[i], s2);
    }
    const float m1 = row_sum(s1) * (1.0f / HID), m2 = row_sum(s2) * (1.0f / HID);
#pragma unroll
    for (int i = 0; i < 8; ++i) dz[i] = rstd * (dx[i] - m1 - xh[i] * m2);
}

// The block's 16 rows through a 128 x 128 layer: z[r][n] = sum_c h[r][c] W[c][n] (transpose:
// W[n][c]) on v_mfma_f32_16x16x4_f32, W read straight from global memory (L2-resident: every
// block of the agent reads the same 64 KB), h from LDS.  WAVES = 4 (a 256-thread block, or one
// 4-wave group of a larger one): wave w computes the two column tiles 32 w .. 32 w + 31; WAVES = 8 (a
// 512-thread block): the one tile 16 w .. 16 w + 15.  Each output is the k-ordered f32 fma chain over
// c = 0 .. 127 from 0 (the per-row VALU GEMV it replaced, bit for bit), the same values for either
// WAVES.  All threads call it; s_z [16][HP] receives z (the caller syncs before reading it).
// gemv_t4: the transposed layer (W^T, the backward) feeds k-step 4 t + s with input
// c = 16 t + 4 lq + s, so a lane's four values of a step group are ONE float4 of its W row (and of
// its LDS row): 8 instead of 32 loads per column, each a contiguous 16 bytes (the strided c = 4 kk
// + lq order touched 16 rows' lines per load instruction: ~7 us per layer on freshly updated
// weights vs ~1.7 us forward).  The k order differs from the VALU loop's, so the backward layers
// are deterministic but no longer the loop's bits (the parity tests bound them against torch).
constexpr int HP = HID + 4;  // padded LDS row
template <int WAVES, int U = HID / 4>  // U: k-steps per unrolled batch (32: the whole layer's loads in flight)
__device__ __forceinline__ void gemv16(const float *s_h, const float *__restrict__ w, bool transpose, float *s_z) {
    constexpr int T = 8 / WAVES;  // column tiles per wave
    const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) & (WAVES - 1), lr = lane & 15, lq = lane >> 4;
    int n[T];
    f32x4 acc[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        n[j] = 16 * T * wave + lr + 16 * j;
        acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    if (transpose) {  // W^T: k-step 4 t + s takes c = 16 t + 4 lq + s (gemv_t4)
        float4 wv[HID / 16][T];
#pragma unroll
        for (int t = 0; t < HID / 16; ++t)
#pragma unroll
            for (int j = 0; j < T; ++j) wv[t][j] = *reinterpret_cast<const float4 *>(w + n[j] * HID + 16 * t + 4 * lq);
#pragma unroll
        for (int t = 0; t < HID / 16; ++t) {
            const float4 a = *reinterpret_cast<const float4 *>(s_h + lr * HP + 16 * t + 4 * lq);
#pragma unroll
            for (int j = 0; j < T; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wv[t][j].x, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < T; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wv[t][j].y, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < T; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wv[t][j].z, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < T; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wv[t][j].w, acc[j], 0, 0, 0);
        }
        // (this branch stores and returns by itself: sharing the stores below costs actor_tail 8 VGPRs)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j) s_z[(4 * lq + i) * HP + n[j]] = acc[j][i];
        return;
    }
    // fully unrolled (U = 32): the weight loads of a lane are all in flight before the first MFMA
    // needs one (one L2 round trip per layer instead of one per 8 k-steps)
#pragma unroll U
    for (int kk = 0; kk < HID / 4; ++kk) {
        const int c = 4 * kk + lq;
        const float a = s_h[lr * HP + c];
        float b[T];
#pragma unroll
        for (int j = 0; j < T; ++j) b[j] = w[c * HID + n[j]];
#pragma unroll
        for (int j = 0; j < T; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[j], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) s_z[(4 * lq + i) * HP + n[j]] = acc[j][i];
}

// the block's rows through a 128 x 128 layer in the per-row layout (thread (rl, g) holds row rl's
// features 8 g .. 8 g + 7): v -> LDS, gemv16, back to registers (two block barriers).  own: whether
// this thread is one of the row layout's owners (a 512-thread block's second group only joins the
// layer); the owners write v and read out
template <int WAVES, int U = HID / 4>
__device__ __forceinline__ void rows_gemv(const float v[8], int rl, int g, const float *w, bool transpose, float *s_in,
                                          float *s_out, float out[8], bool own = true) {
    if (own) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s_in[rl * HP + 8 * g + i] = v[i];
    }
    __syncthreads();
    gemv16<WAVES, U>(s_in, w, transpose, s_out);
    __syncthreads();
    if (own) {
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = s_out[rl * HP + 8 * g + i];
    }
}

// the 8 layer-1 pre-activations of (k, row r) lane g holds, from z [K][B][128]
__device__ __forceinline__ void z8(const float *zb, int B, int k, int r, int g, float z[8]) {
    const float *o = zb + ((int64_t)k * B + r) * HID + 8 * g;
    const float4 a = *reinterpret_cast<const float4 *>(o), b = *reinterpret_cast<const float4 *>(o + 4);
    z[0] = a.x; z[1] = a.y; z[2] = a.z; z[3] = a.w;
    z[4] = b.x; z[5] = b.y; z[6] = b.z; z[7] = b.w;
}

// save 8 features of row r to buf [K][B][128]
__device__ __forceinline__ void put8(float *buf, int B, int k, int r, int g, const float v[8]) {
    float *o = buf + ((int64_t)k * B + r) * HID + 8 * g;
    *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4 *>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// saved per-row quantities of one network's forward + backward (for the gradient kernels)
struct Saved {
    float *h1, *h2, *xh1, *xh2, *gv1, *gv2, *dz1, *dz2;  // [K][B][128]
    float *g3;                                           // [K][B][out] gradient at layer 3's output
    float *aux;                                          // [K][B]: the loss terms
};

// a row's forward through one network after layer 1
struct RowFwd {
    float xh1[8], y1[8], rs1, xh2[8], y2[8], rs2;
};

// row r's forward f and backward (gv1, dz1, gv2, dz2) into sv
__device__ __forceinline__ void save_rows(const Saved &sv, int k, int r, int g, int B, const RowFwd &f, const float gv1[8],
                                          const float dz1[8], const float gv2[8], const float dz2[8]) {
    put8(sv.h1, B, k, r, g, f.y1);
    put8(sv.h2, B, k, r, g, f.y2);
    put8(sv.xh1, B, k, r, g, f.xh1);
    put8(sv.xh2, B, k, r, g, f.xh2);
    put8(sv.gv1, B, k, r, g, gv1);
    put8(sv.gv2, B, k, r, g, gv2);
    put8(sv.dz1, B, k, r, g, dz1);
    put8(sv.dz2, B, k, r, g, dz2);
}

// after layer 1: LN -> ReLU -> the 128 x 128 layer (the caller's 4 waves) -> + b2 -> LN -> ReLU -> nout outputs
// (NOUT > 0: the head's loop unrolled over a compile-time nout)
template <int U = HID / 4, int NOUT = 0>
__device__ __forceinline__ void mlp_rest(float z[8], const Mlp &m, int nout, int rl, int g, float *s_in, float *s_out,
                                         RowFwd &f, float out[NA]) {
    ln_relu(z, m.lw1, m.lb1, g, f.xh1, f.y1, f.rs1);
    rows_gemv<4, U>(f.y1, rl, g, m.w2, false, s_in, s_out, z);
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] += m.b2[8 * g + i];
    ln_relu(z, m.lw2, m.lb2, g, f.xh2, f.y2, f.rs2);
    auto head = [&](int a, int no) {
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s = fmaf(f.y2[i], m.w3[(8 * g + i) * no + a], s);
        out[a] = row_sum(s) + m.b3[a];
    };
    if (NOUT > 0) {
#pragma unroll
        for (int a = 0; a < NOUT; ++a) head(a, NOUT);
    } else {
        for (int a = 0; a < nout; ++a) head(a, nout);
    }
}

// the 9 Gumbel uniforms of (agent kk, row r) in phase ph (0: the target actions, 1: the actor's
// sample): Philox(seed; r, c, 'GUM' + ph, 4 kk + j)
__device__ __forceinline__ void gumbel_u(uint64_t seed, uint32_t c, int ph, int kk, int r, float ur[NA]) {
#pragma unroll
    for (int j = 0; j < (NA + 3) / 4; ++j) {
        const uint4 d = gwrng::philox((uint32_t)r, c, gwrng::TAG_GUMBEL + (uint32_t)ph, (uint32_t)(4 * kk + j),
                                      (uint32_t)seed, (uint32_t)(seed >> 32));
        const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * j + i < NA) ur[4 * j + i] = gwrng::unit(w[i]);
    }
}

// GumbelSoftmax (tau 1) of logits lg with uniforms ur: torch's softmax((logits - log(-log(u + eps)
// + eps)) / 1), gw_gumbel_softmax's op order (pr may be lg)
__device__ __forceinline__ void gumbel_softmax(const float lg[NA], const float ur[NA], float pr[NA]) {
    float mx = -INFINITY;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        pr[a] = (lg[a] - logf(-logf(ur[a] + G_EPS) + G_EPS)) / 1.0f;
        mx = fmaxf(mx, pr[a]);
    }
    float sum = 0.0f;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        pr[a] = expf(pr[a] - mx);
        sum += pr[a];
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) pr[a] = pr[a] / sum;
}

}  // namespace
