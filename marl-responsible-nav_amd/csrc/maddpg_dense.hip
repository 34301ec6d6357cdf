// maddpg_dense.hip — one MADDPG update (agilerl 1.0.15 MADDPG.learn as called by
// maddpg/agent.py:199-224, restated in marlnav/maddpg.py) in a handful of MI355X launches
// (include/learner_ops.h: gw_maddpg_critic_grads, gw_maddpg_actor_grads; the Adam steps and the
// soft update are gw_adam_step / gw_soft_update2).
//
// The networks are K stacked MLPs in marlnav/actor.py's StackedMLPActors layout: in -> 128 ->
// LayerNorm -> ReLU -> 128 -> LayerNorm -> ReLU -> out (9 actor logits, 1 critic value).  A batch
// of B rows (B a multiple of 16) is processed as:
//   l1_kernel       layer 1 (the only wide GEMM: in = K*D + 9K for a critic) split over
//                   64-input chunks: one workgroup per (job, agent, chunk, 128-row tile) writes
//                   the chunk's partial [rows][128]; the consumer adds the chunks in order.
//   *_tail kernels  everything per row: the chunk sum, LayerNorms, ReLUs, layers 2-3 (the
//                   block's 16 rows x 128 on v_mfma_f32_16x16x4_f32, W2 read from L2), Gumbel
//                   softmax (the critic tail computes every agent's target action itself), TD
//                   target, the loss gradient and the backward through layers 3, 2 and the
//                   LayerNorms.  One workgroup per (agent, 16 rows); a row's 128 features live on
//                   16 lanes (8 each), LayerNorm sums are 16-lane butterflies.
//   grads_kernel    the parameter gradients, reductions over the rows in row order: W1 = X^T dz1,
//                   W2 = h1^T dz2, W3 = h2^T g3, biases, LayerNorm affines, the loss value; written
//                   (not accumulated) into the flat gradient buffer's per-layer views.
// Everything is f32 with fixed summation orders (deterministic).  It differs from the torch
// composition (tests/test_maddpg_fused.py) by f32 summation order, including inside LayerNorm's
// row statistics, so a ReLU whose input sits at the rounding edge can take the other side; the
// tests state the flip-tolerant bound.
// The per-row helpers are mlp_rows.h's and the gradient accumulations grad_core.h's, shared with the
// descriptor learner (maddpg_desc.hip).
#include <initializer_list>

#include "mlp_rows.h"
#include "grad_core.h"

namespace {

constexpr int DC = 64, MAXJOB = 4;

// ---- layer 1, split over input chunks ---------------------------------------------------------
// job: rows r of agent k read x[r * ldx + k * xk + col0 + d], weights w[k * wk + (wrow0 + d) * 128 + j]
// for d < D; part[((chunk * K + k) * B + r) * 128 + j] = sum over the chunk's inputs in order.
struct L1Job {
    const float *x;
    const float *w;
    float *part;
    int64_t ldx, xk, wk;
    int col0, wrow0, D, nchunk;
};
struct L1Params {
    L1Job job[MAXJOB];
    int njob, K, B, ntile;
    int start[MAXJOB + 1];  // first block of each job (blocks: job, k, chunk, row tile)
};

__global__ void __launch_bounds__(256) l1_kernel(L1Params p) {
    __shared__ __attribute__((aligned(16))) float s_x[DC][TILE_R + 4];  // [input][row]
    __shared__ __attribute__((aligned(16))) float s_w[DC][HID];         // [input][feature]
    int b = blockIdx.x, j = 0;
    while (j + 1 < p.njob && b >= p.start[j + 1]) ++j;
    const L1Job &jb = p.job[j];
    b -= p.start[j];
    const int tile = b % p.ntile;
    b /= p.ntile;
    const int chunk = b % jb.nchunk, k = b / jb.nchunk;
    const int tid = threadIdx.x;
    const int d0 = chunk * DC, r0 = tile * TILE_R;
    const int nd = min(DC, jb.D - d0);
    // stage x^T (rows of this tile, inputs of this chunk) and the chunk's weight rows
    // every load of a thread is issued before the first LDS store (one memory round trip: the
    // loop form waited for each of its 40 loads in turn, ~20 us per launch)
    const float *xb = jb.x + (int64_t)k * jb.xk + jb.col0 + d0;
    constexpr int XN = DC * TILE_R / 256, WN = DC * HID / 4 / 256;
    float xv[XN];
    float4 wv[WN];
#pragma unroll
    for (int t = 0; t < XN; ++t) {
        const int i = tid + 256 * t, r = i / DC, d = i % DC;  // consecutive threads: consecutive inputs of a row
        xv[t] = (d < nd && r0 + r < p.B) ? xb[(int64_t)(r0 + r) * jb.ldx + d] : 0.0f;
    }
    const float *wb = jb.w + (int64_t)k * jb.wk + (int64_t)(jb.wrow0 + d0) * HID;
#pragma unroll
    for (int t = 0; t < WN; ++t) {
        const int i = tid + 256 * t, d = i / (HID / 4), c = i % (HID / 4);
        wv[t] = d < nd ? reinterpret_cast<const float4 *>(wb + (int64_t)d * HID)[c] : make_float4(0, 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < XN; ++t) {
        const int i = tid + 256 * t;
        s_x[i % DC][i / DC] = xv[t];
    }
#pragma unroll
    for (int t = 0; t < WN; ++t) {
        const int i = tid + 256 * t;
        *reinterpret_cast<float4 *>(&s_w[i / (HID / 4)][4 * (i % (HID / 4))]) = wv[t];
    }
    __syncthreads();
    // v_mfma_f32_16x16x4_f32: wave w computes rows 32 w .. 32 w + 31 (two 16-row tiles) x all 128
    // features (eight 16-column tiles) over the chunk's inputs in order, four per instruction: a
    // k-ordered f32 fma chain from 0, bit for bit the VALU loop it replaced (inputs past the
    // chunk's end are staged as zeros: fma(0, 0, acc) = acc)
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    f32x4 acc[2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[a][c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int nk = (nd + 3) / 4;
    for (int kk = 0; kk < nk; ++kk) {
        const int d = 4 * kk + lq;
        const float a0 = s_x[d][32 * wave + lr], a1 = s_x[d][32 * wave + 16 + lr];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float bw = s_w[d][16 * c + lr];
            acc[0][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bw, acc[0][c], 0, 0, 0);
            acc[1][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bw, acc[1][c], 0, 0, 0);
        }
    }
    // D: row 4 lq + i of the tile, column lr
    float *ob = jb.part + ((int64_t)chunk * p.K + k) * p.B * HID;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + 32 * wave + 16 * a + 4 * lq + i;
            if (r < p.B) {
#pragma unroll
                for (int c = 0; c < 8; ++c) ob[(int64_t)r * HID + 16 * c + lr] = acc[a][c][i];
            }
        }
}

// ---- layer-1 pre-activations: the chunk partials summed in chunk order + the bias ------------------
// z[k][r][j] = (sum over chunks c in order of part[c][k][r][j]) + b1[k][j]: the sum the tails formed
// themselves until round 4, bit for bit, now with every (k, r, 4 features) of every job in
// parallel (a thread's chunk loads 16 at a time in flight) instead of a dependent chain of L2/HBM
// round trips inside each tail (the partials come from other XCDs' L2s: ~2 us per round trip).
struct ReduceJob {
    const float *part, *b1;  // [nch][K][B][HID], [K][HID]
    float *z;                // [K][B][HID]
    int nch;
};
struct ReduceParams {
    ReduceJob job[MAXJOB];
    int njob, K, B, per_job;  // per_job: float4 outputs of one job (K B HID / 4)
};
constexpr int RED_PRE = 16;
__global__ void __launch_bounds__(256) l1_reduce(ReduceParams p) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int j = (int)(t / p.per_job);
    if (j >= p.njob) return;
    const ReduceJob &jb = p.job[j];
    const int i = (int)(t - (int64_t)j * p.per_job);  // float4 index in [K][B][HID / 4]
    const int k = i / (p.B * (HID / 4));
    const int j4 = i % (HID / 4);
    const int64_t cstride = (int64_t)p.K * p.B * (HID / 4);
    const float4 *src = reinterpret_cast<const float4 *>(jb.part) + i;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int c0 = 0; c0 < jb.nch; c0 += RED_PRE) {
        float4 v[RED_PRE];
#pragma unroll
        for (int c = 0; c < RED_PRE; ++c)
            v[c] = c0 + c < jb.nch ? src[(c0 + c) * cstride] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int c = 0; c < RED_PRE; ++c) {
            if (c0 + c < jb.nch) {  // (past the end: nothing added, not even a zero)
                acc.x += v[c].x;
                acc.y += v[c].y;
                acc.z += v[c].z;
                acc.w += v[c].w;
            }
        }
    }
    const float4 b = reinterpret_cast<const float4 *>(jb.b1 + (int64_t)k * HID)[j4];
    reinterpret_cast<float4 *>(jb.z)[i] = make_float4(acc.x + b.x, acc.y + b.y, acc.z + b.z, acc.w + b.w);
}

struct TailParams {
    gw_mlp_actors actor_t, critic_t, critic, actor;  // parameter sets
    const float *x;        // [B][ldx] critic input rows (states, stored actions)
    float *x_next;         // [B][ldx] next states; target actions written into the action slots
    const double *reward;  // [B][K]
    const uint8_t *done;   // [B][K]
    const float *u;        // [K][B][9] Gumbel uniforms of this phase's sample, or null: Philox draws
    uint64_t seed;         // (u null) key of the in-kernel draws
    const int32_t *ctr;    // (u null) a device counter that changes per update
    const float *z_a, *z_ct, *z_c;  // layer-1 pre-activations (l1_reduce: actor-like, critic target, critic)
    Saved sv;
    float gamma;
    int64_t ldx;
    int K, B, D;
    float *probs_out;      // actor phase: [K][B][9] the fresh action probabilities (tests), may be null
};

// the 9 Gumbel uniforms of (agent kk, row r) in phase ph (0: the target actions, 1: the actor's
// sample): from p.u, or Philox(seed; r, *ctr, 'GUM' + ph, 4 kk + j) when p.u is null
__device__ __forceinline__ void gumbel_uniforms(const TailParams &p, int ph, int kk, int r, float ur[NA]) {
    if (p.u) {
        const float *src = p.u + ((int64_t)kk * p.B + r) * NA;
#pragma unroll
        for (int a = 0; a < NA; ++a) ur[a] = src[a];
        return;
    }
    gumbel_u(p.seed, (uint32_t)p.ctr[0], ph, kk, r, ur);
}

// ---- phase 1a: target actions a'_k = GumbelSoftmax(actor_target_k(s'_k)) -------------------
// agent kk's target action probabilities for row r (the per-row layout; all threads call it)
template <int U = HID / 4>
__device__ __forceinline__ void target_probs(const TailParams &p, int kk, int r, int rl, int g, float *s_in,
                                             float *s_out, float pr[NA]) {
    const Mlp m = mlp_k(p.actor_t, kk, p.D, NA);
    float z[8], ur[NA];
    RowFwd f;
    z8(p.z_a, p.B, kk, r, g, z);
    mlp_rest<U, NA>(z, m, NA, rl, g, s_in, s_out, f, pr);
    gumbel_uniforms(p, 0, kk, r, ur);
    gumbel_softmax(pr, ur, pr);
}

// forward of critic (m) on row r: z1 = partial sum + b1 + the action columns of `act` (9K values
// of this row, from LDS); saves into the given arrays; returns q
template <int U = HID / 4, int AU = 9>  // AU: action rows' loads in flight
__device__ __forceinline__ float critic_fwd(const Mlp &m, const float *zsrc, const TailParams &p, int k,
                                            int r, int rl, int g, const float *act, float *s_in, float *s_out,
                                            RowFwd &f) {
    float z[8];
    z8(zsrc, p.B, k, r, g, z);
    const int Ds = p.K * p.D;
#pragma unroll AU
    for (int a = 0; a < NA * p.K; ++a) {  // AU rows' loads in flight together, fmas in row order
        const float av = act[a];
        const float *wr = m.w1 + (int64_t)(Ds + a) * HID + 8 * g;
        const float4 w0 = *reinterpret_cast<const float4 *>(wr), w1 = *reinterpret_cast<const float4 *>(wr + 4);
        z[0] = fmaf(av, w0.x, z[0]); z[1] = fmaf(av, w0.y, z[1]); z[2] = fmaf(av, w0.z, z[2]); z[3] = fmaf(av, w0.w, z[3]);
        z[4] = fmaf(av, w1.x, z[4]); z[5] = fmaf(av, w1.y, z[5]); z[6] = fmaf(av, w1.z, z[6]); z[7] = fmaf(av, w1.w, z[7]);
    }
    float q[NA];
    mlp_rest<U, 1>(z, m, 1, rl, g, s_in, s_out, f, q);
    return q[0];
}

// backward through the critic from dq to dz1 (dh1 = dz2 W2^T on MFMA)
template <int U = HID / 4>
__device__ __forceinline__ void critic_bwd(const Mlp &m, float dq, int rl, int g, const RowFwd &f, float *s_in,
                                           float *s_out, float gv1[8], float dz1[8], float gv2[8], float dz2[8]) {
    float gy[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) gy[i] = dq * m.w3[8 * g + i];
    ln_relu_bwd(gy, f.y2, f.xh2, f.rs2, m.lw2, g, gv2, dz2);
    rows_gemv<4, U>(dz2, rl, g, m.w2, true, s_in, s_out, gy);
    ln_relu_bwd(gy, f.y1, f.xh1, f.rs1, m.lw1, g, gv1, dz1);
}

// ---- phase 1b: TD target from the critic target, the critic's forward, MSE gradient, backward ----
__global__ void __launch_bounds__(256) critic_tail(TailParams p) {
    __shared__ __attribute__((aligned(16))) float s_in[RB * HP];
    __shared__ __attribute__((aligned(16))) float s_out[RB * HP];
    __shared__ float s_act[RB][NA * MAXK];
    const int k = blockIdx.y, tid = threadIdx.x, rl = tid >> 4, g = tid & 15;
    const int r = blockIdx.x * RB + rl;
    const int na = NA * p.K;
    const int64_t Ds = (int64_t)p.K * p.D;
    // target critic on (s', a'): the target actions just computed
    const Mlp mt = mlp_k(p.critic_t, k, p.K * p.D + na, 1);
    const Mlp m = mlp_k(p.critic, k, p.K * p.D + na, 1);
    // every agent's target action on this block's rows (a block per agent recomputes the others':
    // K x a small MLP instead of a launch and a round trip through x_next); agent k's go to x_next
    // too (the caller's record of a')
    for (int kk = 0; kk < p.K; ++kk) {
        float pr[NA];
        target_probs(p, kk, r, rl, g, s_in, s_out, pr);
        if (g == 0) {
#pragma unroll
            for (int a = 0; a < NA; ++a) s_act[rl][NA * kk + a] = pr[a];
            if (kk == k) {
                float *o = p.x_next + (int64_t)r * p.ldx + Ds + NA * k;
#pragma unroll
                for (int a = 0; a < NA; ++a) o[a] = pr[a];
            }
        }
    }
    __syncthreads();
    RowFwd f;
    const float q_next = critic_fwd(mt, p.z_ct, p, k, r, rl, g, s_act[rl], s_in, s_out, f);
    // y = f32(r) + ((1 - d) * gamma) * q_next, gw_td_target's op order
    const float t1 = 1.0f - (float)p.done[(int64_t)r * p.K + k];
    const float y = (float)p.reward[(int64_t)r * p.K + k] + (t1 * p.gamma) * q_next;
    // online critic on (s, a): the stored actions are the x rows' action slots (in the partials)
    float z[8], q[NA];
    z8(p.z_c, p.B, k, r, g, z);
    RowFwd o;
    mlp_rest<HID / 4, 1>(z, m, 1, rl, g, s_in, s_out, o, q);
    const float diff = q[0] - y;
    const float dq = (1.0f / (float)p.B) * (2.0f * diff);  // MSELoss backward (gw_mean_loss_bwd's order)
    float gv1[8], dz1[8], gv2[8], dz2[8];
    critic_bwd(m, dq, rl, g, o, s_in, s_out, gv1, dz1, gv2, dz2);
    const Saved &sv = p.sv;
    save_rows(sv, k, r, g, p.B, o, gv1, dz1, gv2, dz2);
    if (g == 0) {
        sv.g3[(int64_t)k * p.B + r] = dq;
        sv.aux[(int64_t)k * p.B + r] = diff * diff;
    }
}

// ---- phase 2: the actor's forward, GumbelSoftmax, the (updated) critic on the mixed actions,
//      -mean Q gradient, backward through the critic (no parameter gradients) and the actor ----
__global__ void __launch_bounds__(256) actor_tail(TailParams p) {
    __shared__ __attribute__((aligned(16))) float s_in[RB * HP];
    __shared__ __attribute__((aligned(16))) float s_out[RB * HP];
    __shared__ float s_act[RB][NA * MAXK];
    const int k = blockIdx.y, tid = threadIdx.x, rl = tid >> 4, g = tid & 15;
    const int r = blockIdx.x * RB + rl;
    const int na = NA * p.K;
    const int64_t Ds = (int64_t)p.K * p.D;
    const Mlp ma = mlp_k(p.actor, k, p.D, NA);
    const Mlp mc = mlp_k(p.critic, k, p.K * p.D + na, 1);
    // actor forward
    for (int i = tid; i < RB * na; i += 256) s_act[i / na][i % na] = p.x[(int64_t)(blockIdx.x * RB + i / na) * p.ldx + Ds + i % na];
    __syncthreads();
    float z[8], lg[NA], ur[NA], pr[NA];
    RowFwd fa;
    z8(p.z_a, p.B, k, r, g, z);
    mlp_rest<HID / 4, NA>(z, ma, NA, rl, g, s_in, s_out, fa, lg);
    // GumbelSoftmax (tau 1); its gradient is the softmax backward below
    gumbel_uniforms(p, 1, k, r, ur);
    gumbel_softmax(lg, ur, pr);
    if (p.probs_out && g == 0)
        for (int a = 0; a < NA; ++a) p.probs_out[((int64_t)k * p.B + r) * NA + a] = pr[a];
    // the critic k on the mixed actions (own slot: the fresh probabilities; the row's 16 lanes are
    // one wave's, whose LDS operations complete in order)
    if (g == 0)
        for (int a = 0; a < NA; ++a) s_act[rl][NA * k + a] = pr[a];
    RowFwd fc;
    const float q = critic_fwd(mc, p.z_c, p, k, r, rl, g, s_act[rl], s_in, s_out, fc);
    const float dq = -(1.0f / (float)p.B);  // -mean Q backward (gw_mean_loss_bwd mode 1)
    float gv1[8], dz1[8], gv2[8], dz2[8];
    critic_bwd(mc, dq, rl, g, fc, s_in, s_out, gv1, dz1, gv2, dz2);
    // d probs_k = dz1 . W1[the agent's action rows]^T
    float dp[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const float *wr = mc.w1 + (Ds + NA * k + a) * HID + 8 * g;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s = fmaf(dz1[i], wr[i], s);
        dp[a] = row_sum(s);
    }
    // softmax backward: dlogits = p (dp - sum p dp)  (tau 1)
    float dot = 0.0f;
#pragma unroll
    for (int a = 0; a < NA; ++a) dot = fmaf(pr[a], dp[a], dot);
    float dl[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) dl[a] = pr[a] * (dp[a] - dot);
    // actor backward
    float gy[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float s = 0.0f;
#pragma unroll
        for (int a = 0; a < NA; ++a) s = fmaf(dl[a], ma.w3[(8 * g + i) * NA + a], s);
        gy[i] = s;
    }
    ln_relu_bwd(gy, fa.y2, fa.xh2, fa.rs2, ma.lw2, g, gv2, dz2);
    rows_gemv<4>(dz2, rl, g, ma.w2, true, s_in, s_out, gy);
    ln_relu_bwd(gy, fa.y1, fa.xh1, fa.rs1, ma.lw1, g, gv1, dz1);
    const Saved &sv = p.sv;
    save_rows(sv, k, r, g, p.B, fa, gv1, dz1, gv2, dz2);
    if (g == 0) {
        for (int a = 0; a < NA; ++a) sv.g3[((int64_t)k * p.B + r) * NA + a] = dl[a];
        sv.aux[(int64_t)k * p.B + r] = q;
    }
}

// ---- parameter gradients: reductions over the B rows, in row order ---------------------------
// blocks [0, nw1): W1 rows (16 inputs each); [nw1, nw1 + 8): W2 rows; then one block for W3, the
// vectors and the loss.  x: rows r of agent k's layer-1 input at x[r * ldx + k * xk + col0 + d].
struct GradParams {
    gw_mlp_actors grad;    // the gradient views (same layout as the parameters), written
    const float *x;
    int64_t ldx, xk;
    int col0, in_dim, out, K, B, nw1, mode;  // mode 0: critic (loss mean (q - y)^2), 1: actor (-mean q)
    Saved sv;
    float *loss;           // [K]
    int32_t *adam_step;    // the following Adam step's count, advanced here (may be null)
};

__global__ void __launch_bounds__(256) grads_kernel(GradParams p) {
    if (p.adam_step && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.adam_step[0] += 1;
    __shared__ __attribute__((aligned(16))) float smem[GRAD_SMEM];
    const int k = blockIdx.y, tid = threadIdx.x;
    const int b = blockIdx.x;
    if (b < p.nw1 + HID / RB) {  // W1 = X^T dz1 (the layer's inputs p.x) / W2 = h1^T dz2: 16 inputs per block
        const bool w1 = b < p.nw1;
        const int d0 = (w1 ? b : b - p.nw1) * RB;
        const int D = w1 ? p.in_dim : HID;
        const float *xb = w1 ? p.x + (int64_t)k * p.xk + p.col0 + d0 : p.sv.h1 + (int64_t)k * p.B * HID + d0;
        f32x4 acc0, acc1;
        xt_dz_tiles(xb, w1 ? p.ldx : HID, min(RB, D - d0), (w1 ? p.sv.dz1 : p.sv.dz2) + (int64_t)k * p.B * HID, p.B, smem,
                    acc0, acc1);
        const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
        const int n0 = 32 * wave + lr, n1 = n0 + 16;
        float *ob = const_cast<float *>(w1 ? p.grad.w1 + (int64_t)k * p.in_dim * HID : p.grad.w2 + (int64_t)k * HID * HID);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = d0 + 4 * lq + i;
            if (d < D) {
                ob[(int64_t)d * HID + n0] = acc0[i];
                ob[(int64_t)d * HID + n1] = acc1[i];
            }
        }
        return;
    }
    if (b == p.nw1 + HID / RB) {  // the vectors: b1, ln1 affine, b2, ln2 affine
        vec6_sums(p.sv, k, p.B, smem);
        float (*part)[6][HID] = vec6_part(smem);
        for (int t = tid; t < 6 * HID; t += 256) {
            const int v = t / HID, j = t % HID;
            float sum = 0.0f;
            for (int q = 0; q < GRG; ++q) sum += part[q][v][j];
            float *dst[6] = {const_cast<float *>(p.grad.b1), const_cast<float *>(p.grad.ln1_w),
                             const_cast<float *>(p.grad.ln1_b), const_cast<float *>(p.grad.b2),
                             const_cast<float *>(p.grad.ln2_w), const_cast<float *>(p.grad.ln2_b)};
            dst[v][k * HID + j] = sum;
        }
        return;
    }
    // W3 = h2^T g3 [128][out], b3 = sum g3, the loss
    const int out = p.out;
    w3_sums<false>(p.sv, k, p.B, out, smem);
    float (*part)[HID][NA] = w3_part(smem);
    float (*pb)[NA + 1] = w3_pb(smem);
    for (int t = tid; t < HID * out; t += 256) {
        const int j = t / out, a = t % out;
        float sum = 0.0f;
        for (int q = 0; q < GRG; ++q) sum += part[q][j][a];
        const_cast<float *>(p.grad.w3)[((int64_t)k * HID + j) * out + a] = sum;
    }
    if (tid < out) {
        float sum = 0.0f;
        for (int q = 0; q < GRG; ++q) sum += pb[q][tid];
        const_cast<float *>(p.grad.b3)[k * out + tid] = sum;
    } else if (tid == 64 && p.loss) {
        float sum = 0.0f;
        for (int q = 0; q < GRG; ++q) sum += pb[q][NA];
        p.loss[k] = p.mode == 0 ? sum / (float)p.B : -(sum / (float)p.B);
    }
}


// ---- workspace ---------------------------------------------------------------------------------
struct Ws {
    float *part_a, *part_ct, *part_c;
    float *z_a, *z_ct, *z_c;  // [K][B][HID] each
    Saved sv;
};
inline int nchunks(int64_t D) { return (int)((D + DC - 1) / DC); }
inline Ws ws_layout(float *w, int K, int B, int D) {
    const int64_t ldx = (int64_t)K * D + (int64_t)NA * K;
    Ws s;
    s.part_a = w;
    w += (int64_t)nchunks(D) * K * B * HID;
    s.part_ct = w;
    w += (int64_t)nchunks((int64_t)K * D) * K * B * HID;
    s.part_c = w;
    w += (int64_t)nchunks(ldx) * K * B * HID;
    s.z_a = w;
    s.z_ct = w + (int64_t)K * B * HID;
    s.z_c = w + 2LL * K * B * HID;
    w += 3LL * K * B * HID;
    float **f[8] = {&s.sv.h1, &s.sv.h2, &s.sv.xh1, &s.sv.xh2, &s.sv.gv1, &s.sv.gv2, &s.sv.dz1, &s.sv.dz2};
    for (float **q : f) {
        *q = w;
        w += (int64_t)K * B * HID;
    }
    s.sv.g3 = w;
    w += (int64_t)K * B * NA;
    s.sv.aux = w;
    return s;
}
int64_t ws_floats(int K, int B, int D) {
    const int64_t ldx = (int64_t)K * D + (int64_t)NA * K;
    return ((int64_t)nchunks(D) + nchunks((int64_t)K * D) + nchunks(ldx)) * K * B * HID + 11LL * K * B * HID +
           (int64_t)K * B * NA + (int64_t)K * B + 64;
}

void add_job(L1Params &lp, int &blocks, const float *x, int64_t ldx, int64_t xk, int col0, const float *w, int64_t wk,
             int wrow0, int D, float *part) {
    L1Job &j = lp.job[lp.njob];
    j.x = x;
    j.w = w;
    j.part = part;
    j.ldx = ldx;
    j.xk = xk;
    j.wk = wk;
    j.col0 = col0;
    j.wrow0 = wrow0;
    j.D = D;
    j.nchunk = nchunks(D);
    lp.start[lp.njob] = blocks;
    blocks += j.nchunk * lp.K * lp.ntile;
    lp.njob++;
    lp.start[lp.njob] = blocks;
}

void launch_reduce(int K, int B, std::initializer_list<ReduceJob> jobs, hipStream_t s) {
    ReduceParams rp{};
    for (const ReduceJob &j : jobs) rp.job[rp.njob++] = j;
    rp.K = K;
    rp.B = B;
    rp.per_job = K * B * (HID / 4);
    const int64_t threads = (int64_t)rp.njob * rp.per_job;
    hipLaunchKernelGGL(l1_reduce, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, rp);
}

gw_status check(const gw_maddpg_batch *b, const char *who) {
    const std::string w(who);
    if (!b || !b->x || !b->x_next || (!b->u && !b->ctr)) return fail(GW_ERR_ARG, w + ": null argument");
    if (b->K < 1 || b->K > MAXK) return fail(GW_ERR_ARG, w + ": K out of range");
    if (b->B < RB || b->B % RB) return fail(GW_ERR_ARG, w + ": B must be a positive multiple of 16");
    if (b->D < 1) return fail(GW_ERR_ARG, w + ": D must be >= 1");
    if ((reinterpret_cast<uintptr_t>(b->x) | reinterpret_cast<uintptr_t>(b->x_next)) & 3u)
        return fail(GW_ERR_ARG, w + ": misaligned rows");
    return GW_OK;
}

// what both entries fill the same way; each then sets only its networks and scalars
L1Params l1_params(int K, int B) {
    L1Params lp{};
    lp.K = K;
    lp.B = B;
    lp.ntile = (B + TILE_R - 1) / TILE_R;
    return lp;
}

TailParams tail_params(const gw_maddpg_batch &b, const Ws &w, int K, int B, int D) {
    TailParams tp{};
    tp.x = b.x;
    tp.x_next = b.x_next;
    tp.reward = b.reward;
    tp.done = b.done;
    tp.u = b.u;
    tp.seed = b.seed;
    tp.ctr = b.ctr;
    tp.z_a = w.z_a;
    tp.z_ct = w.z_ct;
    tp.z_c = w.z_c;
    tp.sv = w.sv;
    tp.ldx = (int64_t)K * D + (int64_t)NA * K;
    tp.K = K;
    tp.B = B;
    tp.D = D;
    return tp;
}

// xk: agent k's layer-1 input starts at column k * xk of a row of batch.x
GradParams grad_params(const gw_mlp_actors &grad, const gw_maddpg_batch &b, const Ws &w, int in_dim, int out, int64_t xk,
                       int mode, float *loss, int32_t *adam_step) {
    GradParams gp{};
    gp.grad = grad;
    gp.x = b.x;
    gp.ldx = (int64_t)b.K * b.D + (int64_t)NA * b.K;
    gp.xk = xk;
    gp.in_dim = in_dim;
    gp.out = out;
    gp.K = b.K;
    gp.B = b.B;
    gp.nw1 = (in_dim + RB - 1) / RB;
    gp.mode = mode;
    gp.sv = w.sv;
    gp.loss = loss;
    gp.adam_step = adam_step;
    return gp;
}

gw_status launch_grads(const GradParams &gp, hipStream_t s, const std::string &who) {
    hipLaunchKernelGGL(grads_kernel, dim3(gp.nw1 + HID / RB + 2, gp.K), dim3(256), 0, s, gp);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GW_ERR_HIP, who + ": " + hipGetErrorString(e));
    return GW_OK;
}

}  // namespace

extern "C" {

int64_t gw_maddpg_workspace_floats(int32_t K, int32_t B, int32_t D) { return ws_floats(K, B, D); }

gw_status gw_maddpg_critic_grads(const gw_mlp_actors *actor_target, const gw_mlp_actors *critic_target,
                                 const gw_mlp_actors *critic, const gw_mlp_actors *critic_grad,
                                 const gw_maddpg_batch *batch, float gamma, float *ws, float *loss,
                                 int32_t *adam_step, void *stream) {
    gw_status st = check(batch, "gw_maddpg_critic_grads");
    if (st != GW_OK) return st;
    if (!actor_target || !critic_target || !critic || !critic_grad || !ws || !batch->reward || !batch->done)
        return fail(GW_ERR_ARG, "gw_maddpg_critic_grads: null argument");
    const int K = batch->K, B = batch->B, D = batch->D;
    const int64_t ldx = (int64_t)K * D + (int64_t)NA * K;
    const std::string who("gw_maddpg_critic_grads");
    if ((st = check_net(*actor_target, K, D, NA, who)) != GW_OK) return st;
    if ((st = check_net(*critic_target, K, (int)ldx, 1, who)) != GW_OK) return st;
    if ((st = check_net(*critic, K, (int)ldx, 1, who)) != GW_OK) return st;
    const Ws w = ws_layout(ws, K, B, D);
    hipStream_t s = static_cast<hipStream_t>(stream);
    L1Params lp = l1_params(K, B);
    int blocks = 0;
    add_job(lp, blocks, batch->x_next, ldx, D, 0, actor_target->w1, (int64_t)D * HID, 0, D, w.part_a);
    add_job(lp, blocks, batch->x_next, ldx, 0, 0, critic_target->w1, ldx * HID, 0, K * D, w.part_ct);
    add_job(lp, blocks, batch->x, ldx, 0, 0, critic->w1, ldx * HID, 0, (int)ldx, w.part_c);
    hipLaunchKernelGGL(l1_kernel, dim3(blocks), dim3(256), 0, s, lp);
    launch_reduce(K, B, {{w.part_a, actor_target->b1, w.z_a, nchunks(D)},
                         {w.part_ct, critic_target->b1, w.z_ct, nchunks((int64_t)K * D)},
                         {w.part_c, critic->b1, w.z_c, nchunks(ldx)}}, s);
    TailParams tp = tail_params(*batch, w, K, B, D);
    tp.actor_t = *actor_target;
    tp.critic_t = *critic_target;
    tp.critic = *critic;
    tp.gamma = gamma;
    hipLaunchKernelGGL(critic_tail, dim3(B / RB, K), dim3(256), 0, s, tp);
    return launch_grads(grad_params(*critic_grad, *batch, w, (int)ldx, 1, 0, 0, loss, adam_step), s, who);
}

gw_status gw_maddpg_actor_grads(const gw_mlp_actors *actor, const gw_mlp_actors *critic,
                                const gw_mlp_actors *actor_grad, const gw_maddpg_batch *batch, float *ws, float *loss,
                                float *probs, int32_t *adam_step, void *stream) {
    gw_status st = check(batch, "gw_maddpg_actor_grads");
    if (st != GW_OK) return st;
    if (!actor || !critic || !actor_grad || !ws) return fail(GW_ERR_ARG, "gw_maddpg_actor_grads: null argument");
    const int K = batch->K, B = batch->B, D = batch->D;
    const int64_t ldx = (int64_t)K * D + (int64_t)NA * K;
    const std::string who("gw_maddpg_actor_grads");
    if ((st = check_net(*actor, K, D, NA, who)) != GW_OK) return st;
    if ((st = check_net(*critic, K, (int)ldx, 1, who)) != GW_OK) return st;
    const Ws w = ws_layout(ws, K, B, D);
    hipStream_t s = static_cast<hipStream_t>(stream);
    L1Params lp = l1_params(K, B);
    int blocks = 0;
    add_job(lp, blocks, batch->x, ldx, D, 0, actor->w1, (int64_t)D * HID, 0, D, w.part_a);
    add_job(lp, blocks, batch->x, ldx, 0, 0, critic->w1, ldx * HID, 0, K * D, w.part_c);  // state columns
    hipLaunchKernelGGL(l1_kernel, dim3(blocks), dim3(256), 0, s, lp);
    launch_reduce(K, B, {{w.part_a, actor->b1, w.z_a, nchunks(D)}, {w.part_c, critic->b1, w.z_c, nchunks((int64_t)K * D)}}, s);
    TailParams tp = tail_params(*batch, w, K, B, D);
    tp.actor = *actor;
    tp.critic = *critic;
    tp.probs_out = probs;
    hipLaunchKernelGGL(actor_tail, dim3(B / RB, K), dim3(256), 0, s, tp);
    return launch_grads(grad_params(*actor_grad, *batch, w, D, NA, D, 1, loss, adam_step), s, who);
}

}  // extern "C"
