// grad_core.h — the parameter-gradient accumulations both learners run over the rows a tail saved
// (Saved, mlp_rows.h), each a reduction over the B rows in a fixed order.  A 256-thread block calls
// one of them with the kernel's shared buffer (GRAD_SMEM floats, declared once in the kernel so the
// block types overlap in it) and then runs its own epilogue: grads_kernel (maddpg_dense.hip) stores
// the gradient, dgrads_adam (maddpg_desc.hip) steps Adam on it.
#pragma once
#include "mlp_rows.h"

namespace {

constexpr int GRG = 16;  // row groups of the vector / W3 blocks (rows rg, rg + 16, ...)
// W blocks: X^T [16][TILE_R + 4] + dz [TILE_R][128]; vector block: [16][6][128]; W3 block: [16][128][9] + [16][10]
constexpr int GRAD_SMEM = GRG * HID * NA + GRG * (NA + 1) > RB * (TILE_R + 4) + TILE_R * HID
                              ? GRG * HID * NA + GRG * (NA + 1)
                              : RB * (TILE_R + 4) + TILE_R * HID;

// A 16-input block of a weight gradient X^T dz [16][128] on v_mfma_f32_16x16x4_f32: over the rows in
// order (a k-ordered f32 fma chain from 0 across the 128-row tiles); wave w owns features 32 w ..
// 32 w + 31, acc0 / acc1 hold input 4 lq + i of columns n0 = 32 w + lr and n0 + 16.  X: row r's
// inputs xb[r * ldx + d], d < nd (<= 16; the others count as 0: W1's last block); dz: the agent's
// [B][128].  B: a multiple of 16.
__device__ __forceinline__ void xt_dz_tiles(const float *xb, int64_t ldx, int nd, const float *dz, int B, float *smem,
                                            f32x4 &acc0, f32x4 &acc1) {
    float (*s_x)[TILE_R + 4] = reinterpret_cast<float (*)[TILE_R + 4]>(smem);         // [input][row]
    float (*s_dz)[HID] = reinterpret_cast<float (*)[HID]>(smem + RB * (TILE_R + 4));  // [row][feature]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int n0 = 32 * wave + lr, n1 = n0 + 16;
    acc0 = acc1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int r0 = 0; r0 < B; r0 += TILE_R) {
        const int nr = min(TILE_R, B - r0);
        __syncthreads();
        // all of a thread's loads first, then the LDS stores (one memory round trip)
        constexpr int XN = RB * TILE_R / 256, ZN = TILE_R * HID / 4 / 256;
        float xv[XN];
        float4 zv[ZN];
#pragma unroll
        for (int t = 0; t < XN; ++t) {
            const int i = tid + 256 * t, r = i / RB, d = i % RB;
            xv[t] = (r < nr && d < nd) ? xb[(int64_t)(r0 + r) * ldx + d] : 0.0f;
        }
#pragma unroll
        for (int t = 0; t < ZN; ++t) {
            const int i = tid + 256 * t, r = i / (HID / 4), c = i % (HID / 4);
            zv[t] = r < nr ? reinterpret_cast<const float4 *>(dz + (int64_t)(r0 + r) * HID)[c]
                           : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int t = 0; t < XN; ++t) {
            const int i = tid + 256 * t;
            if (i / RB < nr) s_x[i % RB][i / RB] = xv[t];
        }
#pragma unroll
        for (int t = 0; t < ZN; ++t) {
            const int i = tid + 256 * t;
            if (i / (HID / 4) < nr) *reinterpret_cast<float4 *>(&s_dz[i / (HID / 4)][4 * (i % (HID / 4))]) = zv[t];
        }
        __syncthreads();
        for (int kk = 0; kk < nr / 4; ++kk) {  // nr: a multiple of 16 (B % 16 == 0)
            const int r = 4 * kk + lq;
            const float a = s_x[lr][r];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, s_dz[r][n0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, s_dz[r][n1], acc1, 0, 0, 0);
        }
    }
}

// The six vector gradients of agent k (b1, ln1 w, ln1 b, b2, ln2 w, ln2 b as sums of dz, gv xh, gv
// per layer): thread (row group rg, features 8 g .. 8 g + 7) sums rows rg, rg + 16, ...; leaves the
// 16 partials in vec6_part(smem)[rg][vector][feature] behind a barrier, for the caller to add in
// row-group order (a fixed order, independent of the launch)
__device__ __forceinline__ float (*vec6_part(float *smem))[6][HID] { return reinterpret_cast<float (*)[6][HID]>(smem); }
__device__ __forceinline__ void vec6_sums(const Saved &sv, int k, int B, float *smem) {
    const int rg = threadIdx.x >> 4, g = threadIdx.x & 15;
    const int64_t base = (int64_t)k * B * HID;
    float acc[6][8];
#pragma unroll
    for (int v = 0; v < 6; ++v)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[v][i] = 0.0f;
#pragma unroll 2
    for (int r = rg; r < B; r += GRG) {
        const int64_t o = base + (int64_t)r * HID + 8 * g;
        const float *src[6] = {sv.dz1 + o, sv.gv1 + o, sv.xh1 + o, sv.dz2 + o, sv.gv2 + o, sv.xh2 + o};
        float4 q[6][2];
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            q[v][0] = *reinterpret_cast<const float4 *>(src[v]);
            q[v][1] = *reinterpret_cast<const float4 *>(src[v] + 4);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int o2 = 3 * h;  // (dz, gv, xh) of layer h + 1
            const float dzv[8] = {q[o2][0].x, q[o2][0].y, q[o2][0].z, q[o2][0].w,
                                  q[o2][1].x, q[o2][1].y, q[o2][1].z, q[o2][1].w};
            const float gvv[8] = {q[o2 + 1][0].x, q[o2 + 1][0].y, q[o2 + 1][0].z, q[o2 + 1][0].w,
                                  q[o2 + 1][1].x, q[o2 + 1][1].y, q[o2 + 1][1].z, q[o2 + 1][1].w};
            const float xhv[8] = {q[o2 + 2][0].x, q[o2 + 2][0].y, q[o2 + 2][0].z, q[o2 + 2][0].w,
                                  q[o2 + 2][1].x, q[o2 + 2][1].y, q[o2 + 2][1].z, q[o2 + 2][1].w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                acc[o2][i] += dzv[i];                                  // db
                acc[o2 + 1][i] = fmaf(gvv[i], xhv[i], acc[o2 + 1][i]);  // d ln_w
                acc[o2 + 2][i] += gvv[i];                              // d ln_b
            }
        }
    }
    float (*part)[6][HID] = vec6_part(smem);
#pragma unroll
    for (int v = 0; v < 6; ++v)
#pragma unroll
        for (int i = 0; i < 8; ++i) part[rg][v][8 * g + i] = acc[v][i];
    __syncthreads();
}

// W3 = h2^T g3 [128][out], b3 = sum g3 and the loss terms' sum of agent k, in the same 16 row groups:
// leaves w3_part(smem)[rg][feature][a] and w3_pb(smem)[rg][a | loss at NA] behind a barrier
__device__ __forceinline__ float (*w3_part(float *smem))[HID][NA] { return reinterpret_cast<float (*)[HID][NA]>(smem); }
__device__ __forceinline__ float (*w3_pb(float *smem))[NA + 1] {
    return reinterpret_cast<float (*)[NA + 1]>(smem + GRG * HID * NA);
}
// CLAMP: g3's loads past `out` clamped to a valid address (they batch: dgrads_adam) instead of
// predicated (grads_kernel, whose register count the clamped form raises from 188 to 200); the same values
template <bool CLAMP>
__device__ __forceinline__ void w3_sums(const Saved &sv, int k, int B, int out, float *smem) {
    const int rg = threadIdx.x >> 4, g = threadIdx.x & 15;
    const int64_t base = (int64_t)k * B * HID;
    float acc[8][NA];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int a = 0; a < NA; ++a) acc[i][a] = 0.0f;
    float bacc[NA], lacc = 0.0f;
#pragma unroll
    for (int a = 0; a < NA; ++a) bacc[a] = 0.0f;
#pragma unroll 4
    for (int r = rg; r < B; r += GRG) {
        const float *hs = sv.h2 + base + (int64_t)r * HID + 8 * g;
        const float4 h0 = *reinterpret_cast<const float4 *>(hs), h1 = *reinterpret_cast<const float4 *>(hs + 4);
        const float hv[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
        const float *gs = sv.g3 + ((int64_t)k * B + r) * out;
        float gv[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const float x = (CLAMP || a < out) ? gs[a < out ? a : 0] : 0.0f;
            gv[a] = a < out ? x : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int a = 0; a < NA; ++a) acc[i][a] = fmaf(hv[i], gv[a], acc[i][a]);
#pragma unroll
        for (int a = 0; a < NA; ++a) bacc[a] += gv[a];
        lacc += sv.aux[(int64_t)k * B + r];
    }
    float (*part)[HID][NA] = w3_part(smem);
    float (*pb)[NA + 1] = w3_pb(smem);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int a = 0; a < NA; ++a) part[rg][8 * g + i][a] = acc[i][a];
    if (g == 0) {
#pragma unroll
        for (int a = 0; a < NA; ++a) pb[rg][a] = bacc[a];
        pb[rg][NA] = lacc;
    }
    __syncthreads();
}

}  // namespace
