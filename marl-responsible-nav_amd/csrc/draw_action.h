// draw_action.h -- internal: one agent's action of the step about to run, shared by gridenv.hip's step
// kernels and the record builder of gw_fear_preview (fear_preview.hip), which recomputes the draws the next
// gw_step will make.  gridenv.hip includes it where the function used to stand (inside namespace gw), so its
// own kernels compile as before.  Needs cf_env.h (Params, the cell table's bits) and philox.h before it.
#pragma once

// setup_step (ma_customenv.py:432-452) + RL override (:239-242) from the LDS tables: agent n
__device__ __forceinline__ int draw_action(const Params &p, int64_t e, int n, uint32_t episode, int t, int pos,
                                           const uint32_t *ctab, const double *cdf_s) {
    const uint32_t gid = (uint32_t)(p.env_offset + e);
    int a;
    if (n < p.K) {
        if (p.rl) {
            a = p.rl[e * p.K + n];
        } else {
            const uint4 r = gwrng::philox(gid, episode, (uint32_t)t, (2u << 24) | (uint32_t)n, p.key0, p.key1);
            a = (int)(((uint64_t)r.x * 9u) >> 32);
        }
    } else if (p.scripted) {
        a = p.scripted[e * (p.N - p.K) + (n - p.K)];
    } else {
        const uint4 r = gwrng::philox(gid, episode, (uint32_t)t, (1u << 24) | (uint32_t)n, p.key0, p.key1);
        const int uni = r.x < 0x40000000u;  // random.random() < 0.25 (:441)
        const double u = ((double)(r.y >> 5) * 67108864.0 + (double)(r.z >> 6)) * (1.0 / 9007199254740992.0);
        const int pid = (int)((ctab[pos] >> CT_POL) & 0xFFu);
        const double *cdf = (cdf_s ? cdf_s : p.tb.cdf) + (pid * 2 + uni) * NA;
        a = NA - 1;
#pragma unroll
        for (int q = NA - 2; q >= 0; --q)
            if (u < cdf[q]) a = q;  // searchsorted(cdf, u, 'right')
    }
    return ((unsigned)a < (unsigned)NA) ? a : 0;
}
