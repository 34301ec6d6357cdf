// cf_env.h -- internal: the device code that gridenv.hip shares with the translation units of the
// counterfactual FeAR kernels (fear_cf.hip, fear_full.hip, fear_preview.hip, fear_shield_joint.hip,
// fear_matrix.hip) and of the step outcome preview (step_preview.hip): the launch parameters, one world update in registers (World, simulate, cf_valid), the
// step's FearRec, the cell table's bit layout, lds_fill, the CfEnv scaffold and those files' launchers, which
// gridenv.hip calls.  gridenv.hip includes it where this code used to stand, so its own kernels compile as before.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "gridenv.h"
#include "fear_alt_tasks.h"

namespace gw {

constexpr int NA = GW_N_ACTIONS;
typedef float f32x4 __attribute__((ext_vector_type(4)));

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_nt(float4 *dst, const float4 &v) {
    const f32x4 x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<f32x4 *>(dst));
}
constexpr int MAXN = GW_MAX_AGENTS;
constexpr int NDESC = 12;  // u32 words per obs descriptor

// desc[4] flag bits
constexpr uint32_t D_RESET = 1u;      // obs uses the reset encoding (0.5 agents, no relabel)
constexpr uint32_t D_WRITE = 2u;      // write obs for this env
constexpr uint32_t D_FINAL = 4u;      // write final_obs for this env (terminal encoding)

struct Tables {
    const uint8_t *okmask;    // [HW] bit d: unit move d (0 U,1 D,2 L,3 R) allowed
    const uint8_t *policy;    // [HW]
    const double *cdf;        // [P][2][9]
    const uint8_t *mdr;       // [HW]
    const uint16_t *amask;    // [HW]
    const int32_t *free_cells;// [F]
    const float *base;        // [HW] 0 road / -1 inactive
    const double *resp;       // [10][10] clip((vm-va)/(vm+EPS),-1,1)
    const uint32_t *celltab;  // [HW] policy | MdR<<8 | action mask<<12 | unit moves<<21 | road<<25
    const uint32_t *roadbits; // [ceil(HW/32)] bit c: cell c is road
};

struct State {
    int32_t *pos;
    uint32_t *flags;
    int32_t *t;
    uint32_t *episode;
    int32_t *prev;
    double *score;
    double *fscore;
};

struct Params {
    Tables tb;
    State st;
    gw_step_out out;
    uint32_t *desc;           // [E][NDESC]
    const int32_t *rl;        // [E][K] or null
    const int32_t *scripted;  // [E][N-K] or null
    const int32_t *spawn;     // [E][N] or null
    const uint8_t *rmask;     // reset mask or null
    int64_t E, env_offset;
    double fear_weight;
    int H, W, HW, N, K, F;
    int max_steps, auto_reset;
    uint32_t key0, key1;
    uint32_t w_magic;         // ceil(2^32 / W)  (exact /W for cells < 2^16)
    uint32_t hw4_magic;       // ceil(2^32 / (H*W/4))
    uint32_t hw8_magic;       // ceil(2^32 / (H*W/8))
    int lds_cdf, n_cdf, ctab_off, resp_off;  // step_v2 dynamic LDS: [cdf][cell table][Resp 100 f64]
    int obs_be;               // envs per obs_kernel block (<= OBS_BE)
    int obs_bf16;             // obs buffers hold bf16 (the merged step_obs kernel's writer role)
    int64_t e_begin, e_end;   // env range of this launch (step_v2 / obs_kernel chunks)
    uint4 *fwork;             // [E][FearRec<N>::R4] deferred-FeAR records (GW_KERNEL=defer; inline FeAR:
                              // only while gw_set_fear_alt, gw_set_feal or gw_set_fear_full is armed, else null)
    int64_t stats_row0;       // first gw_step_out.stats row this launch writes
    int variant;              // 0 CustomMAEnv, 1 single-agent CustomEnv (custom/customenv.py)
    int apples[MAXN];
    unsigned long long *sims;  // gw_count_sims: FeAR counterfactual world updates run (null: not counted)
};

__device__ __forceinline__ int div_w(const Params &p, int cell) {
    return (int)__umulhi((uint32_t)cell, p.w_magic);
}

__device__ __forceinline__ int manhattan(const Params &p, int a, int b) {
    const int ra = div_w(p, a), rb = div_w(p, b);
    const int ca = a - ra * p.W, cb = b - rb * p.W;
    return abs(ra - rb) + abs(ca - cb);
}

// ---------------------------------------------------------------------------------------
// One world update (GWorld.UpdateGWorld, custom/grid_world.py:424-563) in registers.
// Floor/ceil sub-path indices of (s+1)*len/4 and the overhang terms are compile-time per
// (len, s): len 1 -> f {0,0,0,1} c {1,1,1,1}; len 2 -> f {0,1,1,2} c {1,1,2,2}.
// ---------------------------------------------------------------------------------------
template <int S> struct SubStep;
template <> struct SubStep<0> { static constexpr int f1 = 0, c1 = 1, f2 = 0, c2 = 1, ohf1 = 3, ohc1 = 1, ohf2 = 2, ohc2 = 2; };
template <> struct SubStep<1> { static constexpr int f1 = 0, c1 = 1, f2 = 1, c2 = 1, ohf1 = 2, ohc1 = 2, ohf2 = 0, ohc2 = 0; };
template <> struct SubStep<2> { static constexpr int f1 = 0, c1 = 1, f2 = 1, c2 = 2, ohf1 = 1, ohc1 = 3, ohf2 = 2, ohc2 = 2; };
template <> struct SubStep<3> { static constexpr int f1 = 1, c1 = 1, f2 = 2, c2 = 2, ohf1 = 0, ohc1 = 0, ohf2 = 0, ohc2 = 0; };

// unit-move bits seen by the world update: the u32 cell table of step_v2 (bits CT_OK..CT_OK+3)
struct CtabOk {
    const uint32_t *t;
    __device__ __forceinline__ uint32_t operator()(int c) const { return t[c] >> 21; }
};

// LIST (N > 4, the 128-thread step_v2 chain): a collision pass walks this lane's own near pairs
// (a 64-bit mask, bit 8 ii + jj) and reads the two agents' floor / ceiling / start cells from a
// per-lane LDS row (`lw`, N uint2), instead of evaluating all N (N - 1) / 2 pairs under lane masks:
// with 64 envs per wave nearly every pair index has some lane near, so the unrolled form paid the
// whole pair list on every pass.
template <int N, bool LIST = false>
struct World {
    int nal[N][5];
    int loc[N];
    int delta[N];
    uint32_t two, mv, dir0, dir1;   // bit masks: 2-step action, moving action, direction bits
    uint32_t crash, restr;
    uint32_t near;                  // bit pair(ii, jj): start cells within Manhattan 4
    uint64_t near8 = 0;             // LIST: bit 8 ii + jj for the same pairs
    uint2 *lw = nullptr;            // LIST: this lane's LDS row [N] {floor | ceil << 16, start | two << 16}
    // A pair whose start cells are more than 4 apart can never trigger a rule of
    // collision_checks_and_resolution: every sub-path entry stays within 2 of its own start
    // (reverts go back to the start), so equal / crossing cells need distance <= 4.  Such
    // pairs are skipped; with no near pair at all the resolution loop is skipped.

    __device__ __forceinline__ static constexpr int pair_bit(int ii, int jj) {
        return ii * (2 * N - ii - 1) / 2 + (jj - ii - 1);
    }

    __device__ __forceinline__ void init(const int (&l)[N], const int (&a)[N], int W, uint32_t w_magic) {
        two = mv = dir0 = dir1 = crash = restr = near = 0;
        int rr[N], cc[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            rr[i] = (int)__umulhi((uint32_t)l[i], w_magic);
            cc[i] = l[i] - rr[i] * W;
        }
#pragma unroll
        for (int ii = 0; ii < N - 1; ++ii)
#pragma unroll
            for (int jj = ii + 1; jj < N; ++jj)
            {
                const bool nr = abs(rr[ii] - rr[jj]) + abs(cc[ii] - cc[jj]) <= 4;
                near |= (uint32_t)nr << pair_bit(ii, jj);
                if (LIST) near8 |= (uint64_t)nr << (8 * ii + jj);
            }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            loc[i] = l[i];
            nal[i][0] = l[i];
            const int act = a[i];
            const int d = (act - 1) & 3;  // 0 U, 1 D, 2 L, 3 R
            two |= (uint32_t)(act >= 5) << i;
            mv |= (uint32_t)(act != 0) << i;
            dir0 |= (uint32_t)(d & 1) << i;
            dir1 |= (uint32_t)(d >> 1) << i;
            delta[i] = (d == 0) ? -W : (d == 1) ? W : (d == 2) ? -1 : 1;
        }
    }

    __device__ __forceinline__ int dir_of(int i) const {
        return (int)(((dir0 >> i) & 1u) | (((dir1 >> i) & 1u) << 1));
    }

    // values, not a conditional lvalue: a select between two element addresses would keep
    // the sub-paths in scratch instead of registers
    template <int S>
    __device__ __forceinline__ int fl(int i) const {
        const int a2 = nal[i][SubStep<S>::f2], a1 = nal[i][SubStep<S>::f1];
        return ((two >> i) & 1u) ? a2 : a1;
    }
    template <int S>
    __device__ __forceinline__ int ce(int i) const {
        const int a2 = nal[i][SubStep<S>::c2], a1 = nal[i][SubStep<S>::c1];
        return ((two >> i) & 1u) ? a2 : a1;
    }

    template <int S, class OK>
    __device__ __forceinline__ void move(const OK &okm) {  // :462-518
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int old = nal[i][S];
            if (S >= 2) {  // every action has at most 2 sub-moves: (0, 0) from here on
                nal[i][S + 1] = old;
                continue;
            }
            const bool active_sub = (S == 0) || ((two >> i) & 1u);
            const bool moving = active_sub && ((mv >> i) & 1u) && !((crash >> i) & 1u);
            int nw = old;
            if (moving) {
                const bool ok = (okm(old) >> dir_of(i)) & 1u;  // clip + WorldState[new] >= 0
                nw = ok ? old + delta[i] : old;
                restr |= (uint32_t)(!ok) << i;
            }
            nal[i][S + 1] = nw;
        }
    }

    template <int S>
    __device__ __forceinline__ void resolve_list() {  // LIST form of resolve<S>
        if (near == 0) return;
#pragma unroll
        for (int i = 0; i < N; ++i) lw[i].y = (uint32_t)loc[i] | (((two >> i) & 1u) << 16);
        for (int pass = 0; pass < 2 * N; ++pass) {
#pragma unroll
            for (int i = 0; i < N; ++i) lw[i].x = (uint32_t)fl<S>(i) | ((uint32_t)ce<S>(i) << 16);
            uint32_t hit = 0;
            uint64_t m = near8;
            while (m) {  // this lane's near pairs, in ascending (ii, jj) order
                const int pb = (int)__builtin_ctzll(m);
                m &= m - 1;
                const int ii = pb >> 3, jj = pb & 7;
                const uint2 a = lw[ii], b = lw[jj];
                const int Af = (int)(a.x & 0xFFFFu), Ac = (int)(a.x >> 16), Li = (int)(a.y & 0xFFFFu);
                const int Bf = (int)(b.x & 0xFFFFu), Bc = (int)(b.x >> 16), Lj = (int)(b.y & 0xFFFFu);
                const bool t_i = (a.y >> 16) & 1u, t_j = (b.y >> 16) & 1u;
                const int ohf_i = t_i ? SubStep<S>::ohf2 : SubStep<S>::ohf1;
                const int ohc_i = t_i ? SubStep<S>::ohc2 : SubStep<S>::ohc1;
                const int ohf_j = t_j ? SubStep<S>::ohf2 : SubStep<S>::ohf1;
                const int ohc_j = t_j ? SubStep<S>::ohc2 : SubStep<S>::ohc1;
                const bool same_dir = (Ac - Af) == (Bc - Bf);
                // the elif chain of :276-378 as selects (the N <= 4 form of resolve)
                const bool x1 = Af == Bc, x2 = Ac == Bf;
                const bool cross = ((Af == Lj) | (Ac == Lj)) & ((Li == Bf) | (Li == Bc));
                const bool tail = x1 ? !((ohf_i + ohc_j) <= 4 && same_dir)
                                     : (x2 ? !((ohf_j + ohc_i) <= 4 && same_dir) : cross);
                const bool coll = (Af == Bf) | (Ac == Bc) | (x1 & x2) | tail;
                hit |= coll ? ((1u << ii) | (1u << jj)) : 0u;
            }
            crash |= hit;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                if ((crash >> i) & 1u) {
                    const int f = ((two >> i) & 1u) ? SubStep<S>::f2 : SubStep<S>::f1;
#pragma unroll
                    for (int k = 0; k <= S + 1; ++k)
                        if (k >= f) nal[i][k] = loc[i];
                }
            }
            if (hit == 0) break;
        }
    }

    template <int S>
    __device__ __forceinline__ void resolve() {  // collision_checks_and_resolution :233-405
        if constexpr (LIST) {
            resolve_list<S>();
            return;
        }
        if (near == 0) return;  // no pair can collide: every pass counts 0 (crash stays 0)
        for (int pass = 0; pass < 2 * N; ++pass) {
            uint32_t hit = 0;
#pragma unroll
            for (int ii = 0; ii < N - 1; ++ii) {
                const int Af = fl<S>(ii), Ac = ce<S>(ii);
                const bool t_i = (two >> ii) & 1u;
                const int ohf_i = t_i ? SubStep<S>::ohf2 : SubStep<S>::ohf1;
                const int ohc_i = t_i ? SubStep<S>::ohc2 : SubStep<S>::ohc1;
#pragma unroll
                for (int jj = ii + 1; jj < N; ++jj) {
                    if (!((near >> pair_bit(ii, jj)) & 1u)) continue;
                    const int Bf = fl<S>(jj), Bc = ce<S>(jj);
                    const bool t_j = (two >> jj) & 1u;
                    const int ohf_j = t_j ? SubStep<S>::ohf2 : SubStep<S>::ohf1;
                    const int ohc_j = t_j ? SubStep<S>::ohc2 : SubStep<S>::ohc1;
                    const bool same_dir = (Ac - Af) == (Bc - Bf);
                    bool coll;
                    if constexpr (N <= 4) {  // the same elif chain as selects (few pairs: no VGPR pressure)
                        const bool x1 = Af == Bc, x2 = Ac == Bf;
                        const bool cross = ((Af == loc[jj]) | (Ac == loc[jj])) & ((loc[ii] == Bf) | (loc[ii] == Bc));
                        const bool tail = x1 ? !((ohf_i + ohc_j) <= 4 && same_dir)
                                             : (x2 ? !((ohf_j + ohc_i) <= 4 && same_dir) : cross);
                        coll = (Af == Bf) | (Ac == Bc) | (x1 & x2) | tail;
                    } else if (Af == Bf || Ac == Bc) {
                        coll = true;                                    // :276-278
                    } else if (Af == Bc && Ac == Bf) {
                        coll = true;                                    // :291-294
                    } else if (Af == Bc) {
                        coll = !((ohf_i + ohc_j) <= 4 && same_dir);     // :307-337
                    } else if (Ac == Bf) {
                        coll = !((ohf_j + ohc_i) <= 4 && same_dir);     // :339-368
                    } else {
                        const int Li = loc[ii], Lj = loc[jj];           // :371-378
                        coll = (Af == Lj && Li == Bf) || (Ac == Lj && Li == Bc) ||
                               (Af == Lj && Li == Bc) || (Ac == Lj && Li == Bf);
                    }
                    if (coll) hit |= (1u << ii) | (1u << jj);
                }
            }
            crash |= hit;
            // revertStepsWithCollisions :190-209 (all crashed agents, every pass)
#pragma unroll
            for (int i = 0; i < N; ++i) {
                if ((crash >> i) & 1u) {
                    const int f = ((two >> i) & 1u) ? SubStep<S>::f2 : SubStep<S>::f1;
#pragma unroll
                    for (int k = 0; k <= S + 1; ++k)
                        if (k >= f) nal[i][k] = loc[i];
                }
            }
            if (hit == 0) break;  // this pass recorded no collision (CollisionCount == 0)
        }
    }

    template <int S>
    __device__ __forceinline__ int cf(int i) const {  // NewAgentLocations_CurrentFloor
        return (N == 1) ? loc[i] : fl<S>(i);
    }
};

// UpdateGWorld (grid_world.py:424-563).  caught: bits 0-7 = eaters k that stood on apple[k] at
// some sub-step (floor position, :530-545); bits 8+ = the number of (k, apple) entries the
// reference appends to apples_caught (the single-agent env rewards only len == 1).
template <int N, bool APPLES, class OK, bool LIST>
__device__ __forceinline__ void simulate(World<N, LIST> &w, const OK &okm, int K,
                                         const int (&apple)[MAXN], uint32_t &caught, int (&fin)[N]) {
    caught = 0;
    w.template move<0, OK>(okm);
    w.template resolve<0>();
    if (APPLES) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < K && w.template cf<0>(k) == apple[k]) caught = (caught | (1u << k)) + (1u << 8);
    }
    w.template move<1, OK>(okm);
    w.template resolve<1>();
    if (APPLES) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < K && w.template cf<1>(k) == apple[k]) caught = (caught | (1u << k)) + (1u << 8);
    }
    w.template move<2, OK>(okm);
    w.template resolve<2>();
    if (APPLES) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < K && w.template cf<2>(k) == apple[k]) caught = (caught | (1u << k)) + (1u << 8);
    }
    w.template move<3, OK>(okm);
    w.template resolve<3>();
#pragma unroll
    for (int i = 0; i < N; ++i) fin[i] = w.template cf<3>(i);
    if (APPLES) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < K && fin[k] == apple[k]) caught = (caught | (1u << k)) + (1u << 8);
    }
}

// One counterfactual world update of the wave-per-env kernels (fear_alt_core.h, feal_kernel, fear_full_kernel): `pos`
// under the joint action `joint`, no apples (APPLES is dead: K = 0).  Returns the N-bit set of agents
// that end valid (neither crashed nor restricted).  LIST: wl_row is the lane's World::lw row.  fear_task
// and fear_matrix_kernel keep this block in place (why: profiles/fear_scaffold/SUMMARY.md).
template <int N, bool LIST, bool APPLES, class OK>
__device__ __forceinline__ uint32_t cf_valid(int W, uint32_t w_magic, const OK &okv, const int (&pos)[N],
                                             const int (&joint)[N], uint2 *wl_row) {
    int fin[N];
    int apple[MAXN];
#pragma unroll
    for (int q = 0; q < MAXN; ++q) apple[q] = -1;
    World<N, LIST> w;
    w.init(pos, joint, W, w_magic);
    if constexpr (LIST) w.lw = wl_row;
    uint32_t caught;
    simulate<N, APPLES>(w, okv, 0, apple, caught, fin);
    return ~(w.crash | w.restr) & ((1u << N) - 1u);
}

// Deferred-FeAR record of one env step (GW_KERNEL=defer): what fear_v2 needs to finish the
// step after step_v2 has moved the world on.  R4 uint4 words per env, AoS for 16-byte
// coalesced access:  u16 pre-step cells [N] | u8 actions [N] (bit 7 of byte 0 = done, bit 6 of
// byte k = the single-agent env's +0.1 distance reward of agent k) | i8 integer env rewards [K].
// N <= 4: words 0-1 | 2 | 3;  N <= 8: words 0-3 | 4-5 | 6-7.
template <int N>
struct FearRec {
    static constexpr int R4 = N <= 4 ? 1 : 2, PW = 2 * R4, AW = PW, RW = PW + R4;
    uint32_t w[4 * R4];
};

template <int N>
__device__ __forceinline__ void store_fear_rec(const Params &p, int64_t e, const int (&pos)[N], const int (&act)[N],
                                               const int (&rew)[MAXN], uint32_t bonus, bool done) {
    using R = FearRec<N>;
    R r;
#pragma unroll
    for (int i = 0; i < 4 * R::R4; ++i) r.w[i] = 0u;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        r.w[n >> 1] |= ((uint32_t)pos[n] & 0xFFFFu) << (16 * (n & 1));
        r.w[R::AW + (n >> 2)] |= (((uint32_t)act[n] & 0x3Fu) | (((bonus >> n) & 1u) << 6)) << (8 * (n & 3));
        if (n < p.K) r.w[R::RW + (n >> 2)] |= ((uint32_t)rew[n] & 0xFFu) << (8 * (n & 3));
    }
    r.w[R::AW] |= (uint32_t)done << 7;
    uint4 *dst = p.fwork + e * R::R4;
#pragma unroll
    for (int q = 0; q < R::R4; ++q) dst[q] = make_uint4(r.w[4 * q], r.w[4 * q + 1], r.w[4 * q + 2], r.w[4 * q + 3]);
}

template <int N>
__device__ __forceinline__ void load_fear_rec(const Params &p, int64_t e, int (&pos)[N], int (&act)[N],
                                              int (&rew)[MAXN], uint32_t &bonus, bool &done) {
    using R = FearRec<N>;
    R r;
    const uint4 *src = p.fwork + e * R::R4;
#pragma unroll
    for (int q = 0; q < R::R4; ++q) {
        const uint4 v = src[q];
        r.w[4 * q] = v.x; r.w[4 * q + 1] = v.y; r.w[4 * q + 2] = v.z; r.w[4 * q + 3] = v.w;
    }
    bonus = 0;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        pos[n] = (int)((r.w[n >> 1] >> (16 * (n & 1))) & 0xFFFFu);
        const uint32_t byte = (r.w[R::AW + (n >> 2)] >> (8 * (n & 3))) & 0xFFu;
        act[n] = (int)(byte & 0x3Fu);
        bonus |= ((byte >> 6) & 1u) << n;
    }
#pragma unroll
    for (int k = 0; k < MAXN; ++k)
        rew[k] = (k < N) ? (int)(int8_t)((r.w[R::RW + (k >> 2)] >> (8 * (k & 3))) & 0xFFu) : 0;
    done = (r.w[R::AW] >> 7) & 1u;
}

// cell table bits
constexpr uint32_t CT_POL = 0, CT_MDR = 8, CT_AMASK = 12, CT_OK = 21, CT_ROAD = 25;

#ifndef GW_LIST_MIN_N  // the FeAR-off chain's world update walks per-lane near-pair lists from this N on
#define GW_LIST_MIN_N 5
#endif

// Copy n 32-bit words global -> LDS with 16-byte accesses, all loads of a lane issued before
// its stores (a plain element loop serialises one L2 round trip per iteration).
template <int T>
__device__ __forceinline__ void lds_fill(uint32_t *dst, const uint32_t *__restrict__ src, int n, int tid) {
    const int n4 = n >> 2;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    constexpr int U = 4;
    for (int base = 0; n4 > 0 && base < n4; base += U * T) {
        uint4 v0, v1, v2, v3;  // named registers: loads clamped in range, stores predicated
        const int i0 = base + tid, i1 = i0 + T, i2 = i1 + T, i3 = i2 + T;
        v0 = s4[min(i0, n4 - 1)];
        v1 = s4[min(i1, n4 - 1)];
        v2 = s4[min(i2, n4 - 1)];
        v3 = s4[min(i3, n4 - 1)];
        if (i0 < n4) d4[i0] = v0;
        if (i1 < n4) d4[i1] = v1;
        if (i2 < n4) d4[i2] = v2;
        if (i3 < n4) d4[i3] = v3;
    }
    for (int i = (n4 << 2) + tid; i < n; i += T) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------
// CfEnv: the wave-per-env scaffold of fear_alt_kernel, feal_kernel (fear_cf.hip), fear_full_kernel (fear_full.hip)
// and fear_shield_joint_kernel (fear_shield_joint.hip; the first and the last share fear_alt_core.h).  All run counterfactual
// world updates from the step's FearRec (pre-step cells, joint action): one wave per env, CF_WAVES
// envs per block, the env's tasks dealt to the wave's lanes round-robin, one register-resident world
// update (cf_valid) per lane and turn.  A task ORs valid bits into the kernel's 9-bit sets in LDS
// (`vb`), read after end()'s barrier.  Dynamic LDS (fear_lds): [cell table][100 f64 of p.tb.resp].
// ---------------------------------------------------------------------------------------
constexpr int CF_WAVES = 4, CF_T = 64 * CF_WAVES;

template <int N>
struct CfEnv {
    int pos[N], act[N], mdr[N];  // the record's cells and joint action, the cells' MdR
    int64_t e;
    bool live;                   // e < p.e_end: uniform per wave (a wave past the range runs no task)
    int wave, lane;
    uint32_t *ctab;              // LDS: the cell table
    double *tab;                 // LDS: the 100 f64 at p.tb.resp + tab_off

    // Loads the env's record and fills the tables; zero_vb() clears the kernel's own sets before
    // the block's first barrier.  s_nsim: the block's task count (a __shared__ word of the kernel).
    template <class ZeroVb>
    __device__ __forceinline__ void begin(const Params &p, int tab_off, unsigned int &s_nsim, ZeroVb zero_vb) {
        extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
        ctab = reinterpret_cast<uint32_t *>(dyn + p.ctab_off);
        tab = reinterpret_cast<double *>(dyn + p.resp_off);
        const int tid = threadIdx.x;
        wave = tid >> 6, lane = tid & 63;
        e = p.e_begin + (int64_t)blockIdx.x * CF_WAVES + wave;
        live = e < p.e_end;
        int rew[MAXN];
        uint32_t bonus = 0;
        bool done = false;
#pragma unroll
        for (int n = 0; n < N; ++n) pos[n] = act[n] = 0;
        if (live) load_fear_rec<N>(p, e, pos, act, rew, bonus, done);
        lds_fill<CF_T>(ctab, p.tb.celltab, p.HW, tid);
        lds_fill<CF_T>(reinterpret_cast<uint32_t *>(tab), reinterpret_cast<const uint32_t *>(p.tb.resp + tab_off), 200, tid);
        zero_vb();
        if (tid == 0) s_nsim = 0u;
        __syncthreads();
        // the record's fields are clamped to their ranges before they index anything
#pragma unroll
        for (int n = 0; n < N; ++n) {
            pos[n] = min(pos[n], p.HW - 1);
            act[n] = min(act[n], NA - 1);
            mdr[n] = min((int)((ctab[pos[n]] >> CT_MDR) & 0xFu), NA - 1);
        }
    }

    // The wave ran ntask world updates: the block's sum goes to p.sims (gw_count_sims) once.
    __device__ __forceinline__ void end(const Params &p, unsigned int &s_nsim, int ntask) const {
        if (lane == 0 && p.sims && ntask) atomicAdd(&s_nsim, (unsigned int)ntask);
        __syncthreads();
        if (threadIdx.x == 0 && p.sims && s_nsim) atomicAdd(p.sims, (unsigned long long)s_nsim);
    }
};

// fear_full_kernel<N> (fear_full.hip, gw_set_fear_full) over p's env range on s, through gwprof::launch
hipError_t launch_fear_full(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                            double *resp_full, uint16_t *resp_valid);

// preview_rec_kernel<N> (fear_preview.hip, gw_fear_preview) over p's env range on s, through gwprof::launch:
// the record of the step the next gw_step will run into p.fwork, its joint action and MdRs into actions / mdr
// ([E][N] or null)
hipError_t launch_preview_rec(int N, hipStream_t s, const Params &p, int32_t *actions, int32_t *mdr);

// gw_step_preview's outputs beside the env's (include/gridenv.h): mask [E][K] or null, outcome [E][K][9],
// reward_alt [E][K][9] / crash9 [E][K] / safe_mask [E][K] or null
struct StepPreviewArgs {
    const uint16_t *mask;
    uint16_t *outcome;
    double *reward_alt;
    uint16_t *crash9;
    uint16_t *safe_mask;
};

// step_preview_kernel<N> (step_preview.hip, gw_step_preview) over p's env range on s, through gwprof::launch,
// from the record in p.fwork
hipError_t launch_step_preview(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                               const StepPreviewArgs &a);

// gw_step_lookahead's outputs beside the env's (include/gridenv.h): mask [E][K] or null, crash2 [E][K][9] /
// ends [E][K] / crash9 [E][K] / trap9 [E][K] / ahead_mask [E][K] or null
struct StepLookaheadArgs {
    const uint16_t *mask;
    uint16_t *crash2;
    uint16_t *ends;
    uint16_t *crash9;
    uint16_t *trap9;
    uint16_t *ahead_mask;
};

// step_lookahead_kernel<N> (step_lookahead.hip, gw_step_lookahead) over p's env range on s, through gwprof::launch,
// from the record in p.fwork
hipError_t launch_step_lookahead(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                                 const StepLookaheadArgs &a);

// gw_step_horizon's arguments beside the env's (include/gridenv.h): mask [E][K] or null, horizon in
// 2..GW_HORIZON_MAX, depth [E][K][9] / ends [E][K] / crash9 [E][K] / viable9 [E][K] / horizon_mask [E][K] or null
struct StepHorizonArgs {
    const uint16_t *mask;
    int horizon;
    uint8_t *depth;
    uint16_t *ends;
    uint16_t *crash9;
    uint16_t *viable9;
    uint16_t *horizon_mask;
};

// step_horizon_kernel<N> (step_horizon.hip, gw_step_horizon) over p's env range on s, through gwprof::launch,
// from the record in p.fwork
hipError_t launch_step_horizon(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                               const StepHorizonArgs &a);

// gw_step_plan's arguments beside the env's (include/gridenv.h): mask [E][K] or null, horizon in 2..GW_HORIZON_MAX,
// depth [E][K][9] / ret [E][K][9] / path [E][K][9][GW_HORIZON_MAX - 1] / ends [E][K] / crash9 [E][K] /
// plan_mask [E][K] or null
struct StepPlanArgs {
    const uint16_t *mask;
    int horizon;
    uint8_t *depth;
    int16_t *ret;
    uint8_t *path;
    uint16_t *ends;
    uint16_t *crash9;
    uint16_t *plan_mask;
};

// step_plan_kernel<N> (step_plan.hip, gw_step_plan) over p's env range on s, through gwprof::launch, from the
// record in p.fwork
hipError_t launch_step_plan(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                            const StepPlanArgs &a);

// The arguments of the two joint shields beside the env's (include/gridenv.h; the kernels' one body:
// shield_joint_core.h): mask [E][K] or null, probs [K][E][9] or null, agents / sweeps already checked,
// actions_out [E][K], flags [E][K] / table [E][K][9] / joint [E][N] or null.  gw_crash_shield_joint alone reads
// use_fear and the outputs outcome [E] / outcome_prop [E] / crash9 [E][K] or null; gw_fear_shield_joint passes
// use_fear = 1 and null for the three
struct JointShieldArgs {
    const uint16_t *mask;
    const float *probs;
    int use_fear;
    double tau;
    uint32_t agents;
    int sweeps;
    int32_t *actions_out;
    uint8_t *flags;
    double *table;
    int32_t *joint;
    uint16_t *outcome;
    uint16_t *outcome_prop;
    uint16_t *crash9;
};

// fear_shield_joint_kernel<N> (fear_shield_joint.hip, gw_fear_shield_joint) and crash_shield_joint_kernel<N>
// (crash_shield_joint.hip, gw_crash_shield_joint) over p's env range on s, through gwprof::launch, from the
// record in p.fwork
hipError_t launch_fear_shield_joint(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                                    const JointShieldArgs &a);
hipError_t launch_crash_shield_joint(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                                     const JointShieldArgs &a);

// fear_alt_kernel<N> (fear_cf.hip; gw_set_fear_alt, and gw_fear_preview on the preview's record) over p's env
// range on s, through gwprof::launch: table [E][K][9]
hipError_t launch_fear_alt(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p, double *table);

// feal_kernel<N> (fear_cf.hip, gw_set_feal) over p's env range on s, through gwprof::launch
hipError_t launch_feal(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p, double *feal,
                       uint16_t *feal_valid);

// gw_fear_matrix's arguments: n world snapshots the caller supplies
struct FmParams {
    const uint32_t *celltab;
    const double *tab;        // [0, 100) Resp(vm, va), [100, 200) FeAL(vm, va)
    int HW, W;
    uint32_t w_magic;
    const int32_t *cells, *acts, *mdr;  // [n][N]; mdr may be null (the cells' MdR)
    const uint8_t *in_list;             // [n] bit a: agent a in ActionID4Agents; null = all
    double *resp;                       // [n][N][N]
    int32_t *vm, *va;                   // [n][N][N] or null
    double *feal;                       // [n][N] or null
    int32_t *feal_vm, *feal_va;         // [n][N] or null
};

// fear_matrix_kernel<N> (fear_matrix.hip, gw_fear_matrix): one block per snapshot on s, through gwprof::launch;
// dyn: the cell table's bytes.  N = 1 is an error
hipError_t launch_fear_matrix(int N, int64_t n_blocks, size_t dyn, hipStream_t s, const FmParams &q);

}  // namespace gw
