/* Rollout bookkeeping ops of libgridenv.so (marlnav/rollout.py, marlnav/parallel.py).
 *
 * Per step the batched rollout (maddpg/agent.py:124-173 over E envs) folds the step kernels'
 * per-block partial sums (gw_step_out.stats: completed-episode returns, episodes, FeAR, crashes,
 * apples, shaped rewards, lengths, env-steps) into running totals and advances the replay
 * ring's device-side step count.  As PyTorch ops that is a generic reduction, an add and an
 * increment (three launches, ~20 us at 65,536 envs); here it is one single-block launch.
 * Plain device pointers; enqueued on `stream`; statuses as in gridenv.h. */
#ifndef ROLLOUT_OPS_H
#define ROLLOUT_OPS_H

#include <stdint.h>

#include "gridenv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* s[f] = sum over r of partials[r][f] (r ascending per lane stride, then a fixed tree: the
 * result is deterministic); row_sum[f] = s[f] if row_sum != NULL; totals[f] += s[f] if
 * totals != NULL; *counter += 1 if counter != NULL.  n_fields <= 64. */
gw_status gw_rollout_tick(const double *partials, int64_t rows, int32_t n_fields, double *row_sum,
                          double *totals, int64_t *counter, void *stream);

/* Completed-episode return compaction of a window of gathered steps (marlnav/parallel.py
 * ReturnGather.compact; the reference appends scores[i] to completed_episode_scores for every
 * env done this step, maddpg/agent.py:229-247).  recv holds `steps` x `world` slots of
 * slot_bytes bytes: [emax] f64 returns, then [emax] u8 done flags (slot_bytes % 8 == 0,
 * slot_bytes >= 9 * emax).  Every done element, in (step, rank, env) order, is appended to the
 * ring scores[capacity] at (*n_completed + its rank) % capacity (only the last `capacity` of
 * the window are written), and *n_completed grows by the window's count.  scratch:
 * gw_return_compact_scratch(steps, world, emax) int32 words of device memory.  Two launches,
 * deterministic, no host synchronisation (graph-capturable). */
gw_status gw_return_compact(const uint8_t *recv, int64_t steps, int32_t world, int64_t emax,
                            int64_t slot_bytes, double *scores, int64_t capacity,
                            int64_t *n_completed, int32_t *scratch, void *stream);
int64_t gw_return_compact_scratch(int64_t steps, int32_t world, int64_t emax);

/* The packed per-step return gather of several ranks (marlnav/parallel.py ReturnGather, world > 1;
 * the reference's completed_episode_scores, maddpg/agent.py:229-247).  Instead of every env's
 * return + done flag (9 B per env per step), a rank sends only its completed episodes' returns:
 *
 * gw_gather_pack (sender, per step): this step's done envs' ep_return (env order) are appended to
 * the rank's FIFO fifo[fifo_cap] (ring, state ctl[4] = {head, tail, overflow, 0} int64, zeroed at
 * start); the send slot (32 + 8 cap bytes) gets the header {count, sent, backlog after, overflow}
 * (int64) and the FIFO's first sent = min(backlog, cap) entries.  scratch:
 * gw_gather_pack_scratch(E) int32 words.  Two launches, no host synchronisation.
 *
 * gw_gather_unpack (receiver, per window of `steps` gathered slots [steps][world][slot_bytes]):
 * appends every rank's payload to its mirror FIFO (mirror[world][mirror_cap]), queues the per-step
 * counts in pend[pend_cap][world], and appends to the score ring scores[capacity] (the last
 * `capacity` kept; *n_completed = completions ever) every pending step whose entries have all
 * arrived, in (step, rank, env) order: the reference's order with rank-major contiguous shards.
 * rstate: int64 [2 world + 4] = {received per rank, emitted per rank, pending head, pending tail,
 * overflow (sticky: a FIFO, mirror or pending ring ran out), max sender backlog of the window},
 * zeroed at start.  plan: gw_gather_unpack_plan_cap(steps, world, pend_cap) segments of 40 bytes
 * + 32 bytes.  Three launches, no host synchronisation. */
int64_t gw_gather_pack_scratch(int64_t E);
gw_status gw_gather_pack(const double *ep_return, const uint8_t *done, int64_t E, int64_t cap, double *fifo,
                         int64_t fifo_cap, int64_t *ctl, int32_t *scratch, uint8_t *slot, void *stream);
int64_t gw_gather_unpack_plan_cap(int64_t steps, int32_t world, int64_t pend_cap);
gw_status gw_gather_unpack(const uint8_t *recv, int64_t steps, int32_t world, int64_t slot_bytes, double *mirror,
                           int64_t mirror_cap, int64_t *rstate, int32_t *pend, int64_t pend_cap, void *plan,
                           int64_t plan_cap, double *scores, int64_t capacity, int64_t *n_completed, void *stream);

/* Replay-ring sample (agilerl MultiAgentReplayBuffer.sample, uniform; called at
 * maddpg/agent.py:209-211; marlnav/rollout.py ReplayRing.sample) as ONE gather launch.  Ring
 * layout: obs / final_obs [S, K, E, HW] (f32, or bf16 if obs_bf16), probs [S, K, E, 9] f32,
 * reward [S, E, K] f64, term [S, E, K] u8, done [S, E] u8; *t_dev = transitions stored.  For each
 * b < B:  n = clamp(*t_dev, 1, S - 1);  step = min((int64)(u[b] * (float)n), n - 1);
 * tr = (*t_dev - 1 - step) mod S;  nx = (tr + 1) mod S;  e = env[b];  then
 *   state[k, b] = obs[tr, k, e];  next[k, b] = done[tr, e] ? final_obs[tr, k, e] : obs[nx, k, e]
 *   probs_out[k, b] = probs[tr, k, e];  reward_out[b] = reward[tr, e];  term_out[b] = term[tr, e]
 * (outputs f32 [K, B, HW], [K, B, 9], f64 [B, K], u8 [B, K]); tr_out[b] = tr if tr_out != NULL.
 * x_out / xn_out (may be NULL): the critic's input rows [B, K*HW + K*9] of MADDPG.learn, agent-major
 * states then the K action slots (agilerl's torch.cat of states and actions):
 *   x_out[b] = [state[0, b] .. state[K-1, b], probs_out[0, b] .. probs_out[K-1, b]];
 *   xn_out[b][0, K*HW) = next_state[., b] (its action slots are left to the caller).
 * u = env = NULL: u[b] and e drawn in the kernel from Philox4x32-10(key seed; counter (b, *ctr,
 * 'SAMP', 0)) (the uniform from the first word, e = (second word * E) >> 32), as
 * gw_replay_gather_desc does, so both samplers pick the same rows. */
gw_status gw_replay_gather(const void *obs, const void *final_obs, int32_t obs_bf16, const float *probs,
                           const double *reward, const uint8_t *term, const uint8_t *done, const int64_t *t_dev,
                           const float *u, const int64_t *env, int64_t S, int32_t K, int64_t E, int64_t HW,
                           int64_t B, float *state, float *next_state, float *probs_out, double *reward_out,
                           uint8_t *term_out, int64_t *tr_out, float *x_out, float *xn_out, uint64_t seed,
                           const int32_t *ctr, void *stream);

/* gw_replay_gather with the obs rows expanded from a ring of obs descriptors instead of read
 * from the dense obs / final_obs slots (the learner then never waits for the obs writer of the
 * step it follows; the rows are bit for bit the ones the obs writer put in the ring).
 * desc [S][E][12] u32: slot j holds the descriptors of the step whose obs went to obs slot j
 * (gw_obs_desc_copy after that step, into slot j); the terminal obs of transition slot tr
 * comes from the terminal half of descriptor slot tr + 1.  src: gw_obs_view of the env
 * (base map, apple cells, N, K, H, W, variant, E; its desc pointer is not used).  Every other
 * argument and output as gw_replay_gather (f32 rows; K = src->K, HW = src->H * src->W <= 4096).
 * u = env = NULL: the (transition, env) draws are made in the kernel instead of read: row b's
 * uniform and env index from Philox4x32-10(key seed; counter (b, *ctr, 'SAMP', 0)), the env as
 * the multiply-high of a 32-bit draw and E (ctr: a device int32 that changes per sample, e.g.
 * the critic optimizer's step count before the update advances it).  state / next_state may be
 * NULL when x_out and xn_out are given (the fused learner reads only the critic rows). */
gw_status gw_replay_gather_desc(const gw_obs_source *src, const uint32_t *desc, const float *probs,
                                const double *reward, const uint8_t *term, const uint8_t *done, const int64_t *t_dev,
                                const float *u, const int64_t *env, int64_t S, int64_t B, float *state,
                                float *next_state, float *probs_out, double *reward_out, uint8_t *term_out,
                                int64_t *tr_out, float *x_out, float *xn_out, uint64_t seed, const int32_t *ctr,
                                void *stream);

/* gw_replay_gather_desc for a local-window rollout whose ring holds descriptors ONLY
 * (marlnav/rollout.py ReplayRing(patch=P, desc="only")): the obs rows are each agent's P x P window
 * (gw_obs_patch, include/gridenv.h) expanded straight from the descriptors, so the rollout step runs no
 * window writer and the ring keeps 48 bytes per env and slot instead of 2 * K * P * P * 4.  The argument
 * list and the sampling rule (n, step, tr, nx, explicit u / env or the in-kernel Philox draws with the
 * 'SAMP' tag) and probs_out, reward_out, term_out, tr_out are gw_replay_gather_desc's; with HW := P * P
 *   state[k, b]      = agent k's window of the obs of descriptor slot tr;
 *   next_state[k, b] = the window of descriptor slot nx, from its terminal half (words 8-11, apple bits
 *                      16-23) when done[tr, e] is set, as gw_replay_gather_desc chooses;
 *   x_out[b] = [state[0, b] .. state[K-1, b], probs_out[0, b] .. probs_out[K-1, b]] (K * P * P + 9 K floats);
 *   xn_out[b][0, K * P * P) = the next windows (its action slots are left to the caller);
 * state / next_state may be NULL when x_out and xn_out are given.
 * The window: rows and columns -P/2 .. P-1-P/2 around agent k's own cell IN THAT HALF OF THAT DESCRIPTOR
 * (the spawn cell of a reset-encoded obs, the terminal cell of the terminal half), cells outside the grid
 * -1, the map value else, then the descriptor's patched cells (the apple first, then agents 0 .. N-1, a
 * later one overrides): bit for bit gw_obs_patch(env, P, patch, final_patch) of the step that filled the
 * slot.  1 <= P <= 129 (gw_obs_patch's range), src->H * src->W <= 4096, desc 16-byte aligned; anything
 * else returns GW_ERR_ARG with a gw_last_error message.  One launch, one 256-thread block per (b, k); no
 * atomics; e, the descriptor cells and the apple cells are clamped before they index anything. */
gw_status gw_replay_gather_desc_patch(const gw_obs_source *src, const uint32_t *desc, const float *probs,
                                      const double *reward, const uint8_t *term, const uint8_t *done,
                                      const int64_t *t_dev, const float *u, const int64_t *env, int64_t S,
                                      int64_t B, int32_t P, float *state, float *next_state, float *probs_out,
                                      double *reward_out, uint8_t *term_out, int64_t *tr_out, float *x_out,
                                      float *xn_out, uint64_t seed, const int32_t *ctr, void *stream);

/* One evaluation step's totals (customeval.py:70-133 over E episodes at once; marlnav/evaluate.py):
 * for every env e with active[e]:  counts[0] += crashes[e];  counts[1] += apples[e];
 * counts[2] += 1;  *fear_total += sum_k fear[e, k];  then active[e] = 0 if done[e].
 * crashes / apples [E] i32, fear [E, K] f64, done / active [E] u8.  One block, fixed order. */
gw_status gw_eval_accum(const int32_t *crashes, const int32_t *apples, const double *fear, const uint8_t *done,
                        uint8_t *active, int64_t *counts, double *fear_total, int64_t E, int32_t K, void *stream);

/* Per-pair responsibility totals of one step (gw_step_out.fear_row, [E][K][N] f64):
 * totals[k][j] += sum over e (active[e] != 0, or all if active == NULL) of fear_row[e][k][j];
 * *steps += 1.  Fixed summation order (e ascending per lane stride, then a fixed tree):
 * deterministic.  One block, graph-capturable, no host sync.  Call it before gw_eval_accum in an
 * evaluation step (that op retires the done envs from `active`). */
gw_status gw_fear_row_accum(const double *fear_row, const uint8_t *active, int64_t E, int32_t K, int32_t N,
                            double *totals, int64_t *steps, void *stream);

/* Hindsight FeAR regret of one step (gw_set_fear_alt's table [E][K][9] f64 against the step's fear
 * [E][K] f64):  totals [K][2] f64:  [k][0] += sum_e (fear[e][k] - min_a fear_alt[e][k][a]);
 * [k][1] += #e with fear[e][k] == that minimum;  over envs with active[e] != 0 (NULL: all);
 * *steps += 1.  The minimum runs over all nine actions (masking is the caller's business).  The same
 * fixed summation order as gw_fear_row_accum: deterministic.  One block, graph-capturable, no host
 * sync.  Call it before gw_eval_accum in an evaluation step. */
gw_status gw_fear_regret_accum(const double *fear_alt, const double *fear, const uint8_t *active, int64_t E,
                               int32_t K, double *totals, int64_t *steps, void *stream);

/* Per-agent FeAL totals of one step (gw_set_feal's feal, [E][N] f64):
 * totals[i] += sum over e (active[e] != 0, or all if active == NULL) of feal[e][i];  *steps += 1;
 * *envs += the number of those envs.  The lane groups, env order and fixed tree of
 * gw_fear_row_accum: deterministic.  One block, graph-capturable, no host sync.  Call it before
 * gw_eval_accum in an evaluation step. */
gw_status gw_feal_accum(const double *feal, const uint8_t *active, int64_t E, int32_t N, double *totals,
                        int64_t *steps, int64_t *envs, void *stream);

/* Responsibility maps: one step's N x N valid-action sets binned by the cells the agents stood on.
 * resp_valid [E][N][N][2] u16 as gw_set_fear_full stores it ([0]: the affected agent's 9-bit valid set with
 * the actor on its MdR, [1]: under the actual actions; 4-byte aligned), cells [N][E] i32 the step's PRE-move
 * cells (the env's pos layout: gw_copy_state with only pos set, before the gw_step), active [E] u8 or NULL
 * (only the envs with active[e] != 0), counts [2][HW][10][10] u64 and visits [HW] u64 (may be NULL), both
 * ADDED to (8-byte aligned; the caller zeroes them once).  For every such env e and ordered pair i != j, with
 * vm = popc(resp_valid[e][i][j][0] & 0x1FF), va = popc(resp_valid[e][i][j][1] & 0x1FF):
 *   counts[0][cells[i][e]][vm][va] += 1    "caused here": the actor's cell;
 *   counts[1][cells[j][e]][vm][va] += 1    "received here": the affected agent's cell;
 *   visits[cells[i][e]] += 1               once per (e, i).
 * resp_full[e][i][j] == T[vm][va] (the Resp table, csrc/resp_tables.h), so the sum of Resp caused at cell c is
 * sum_vm sum_va counts[0][c][vm][va] * T[vm][va], formed on the host in that fixed order
 * (marlnav.resp_map_from_counts).  The device only counts: integer addition is exact, so the result is the
 * same bit for bit whatever order the increments arrive in, a graph replay equals the eager run, and several
 * ranks all-reduce the integers.  (A per-cell sum of doubles by atomics would depend on arrival order.)
 * Every cell is clamped to [0, HW) and every popcount to [0, 9] before it indexes anything (csrc/resp_map.h,
 * the same text the CPU check runs).  One launch of 256-thread blocks, one thread per (i, j, e) with e
 * fastest, one 4-byte load of the pair of sets per thread, 64-bit global atomic adds without return; no LDS,
 * no allocation, no host sync: graph-capturable.  Call it after the FeAR fence, and before gw_eval_accum in
 * an evaluation step.  It has no env handle and so no gw_profile_spans kind.
 * GW_ERR_ARG (with a gw_last_error message): NULL resp_valid, cells or counts; N outside 2..8; E <= 0 or
 * HW <= 0; a misaligned pointer. */
gw_status gw_resp_map_accum(const uint16_t *resp_valid, const int32_t *cells, const uint8_t *active,
                            uint64_t *counts, uint64_t *visits, int32_t E, int32_t N, int32_t HW, void *stream);

/* Responsibility footprints: the same sets binned by the ACTOR'S ACTION and the affected agent's OFFSET from
 * the actor, an egocentric map of how far and in which direction an action restricts others.
 * resp_valid, cells, active: as gw_resp_map_accum takes them; actions [E][N] i32 the step's joint action (the
 * step's `actions` output; 4-byte aligned); crash_bits [E] u8 or NULL (the step's `crash_bits` output: bit j =
 * agent j crashed in the step); R in 1..15 the radius of the near window; O = (2R + 1)^2 + 1;
 * counts [2][9][O][10][10] u64 and visits [9] u64 (may be NULL), both ADDED to (8-byte aligned; the caller
 * zeroes them once).  For every env e (active[e] != 0, or all if active == NULL) and ordered pair i != j, with
 * vm, va the popcounts as above, a = actions[e][i] (outside 0..8: 0, as the step reads it),
 * dr = cells[j][e] / W - cells[i][e] / W, dc = cells[j][e] % W - cells[i][e] % W and
 * o = (dr + R) (2R + 1) + (dc + R) if |dr| <= R and |dc| <= R, else the far bin (2R + 1)^2:
 *   counts[0][a][o][vm][va] += 1;
 *   counts[1][a][o][vm][va] += 1    if crash_bits != NULL and bit j of crash_bits[e] is set
 *                                   (crash_bits == NULL: plane 1 is not touched);
 *   visits[a] += 1                  once per (e, i).
 * The sum of the Resp that action a caused at offset o is sum_vm sum_va counts[0][a][o][vm][va] * T[vm][va],
 * formed on the host in that fixed order (marlnav.resp_footprint_from_counts).  The device only counts, so the
 * result is the same bit for bit eager, replayed and all-reduced, as the maps' is.  Every cell is clamped to
 * [0, H W) and every popcount to [0, 9] before it indexes anything (csrc/resp_footprint.h, the same text the
 * CPU check runs).  One launch of 256-thread blocks, one thread per (i, j, e) with e fastest; the lanes of a
 * wave that hold the same bin are merged into one 64-bit global atomic add without return of their number; no
 * LDS, no allocation, no host sync: graph-capturable.  Call it after the FeAR fence, and before gw_eval_accum
 * in an evaluation step.  It has no env handle and so no gw_profile_spans kind.
 * GW_ERR_ARG (with a gw_last_error message): NULL resp_valid, cells, actions or counts; N outside 2..8;
 * E <= 0, H <= 0 or W <= 0 (or H W beyond int32); R outside 1..15; a misaligned pointer. */
gw_status gw_resp_footprint_accum(const uint16_t *resp_valid, const int32_t *cells, const int32_t *actions,
                                  const uint8_t *crash_bits, const uint8_t *active, uint64_t *counts,
                                  uint64_t *visits, int32_t E, int32_t N, int32_t H, int32_t W, int32_t R,
                                  void *stream);

/* The responsibility shield: replace an RL action whose previewed FeAR exceeds tau, before the world moves.
 * fear_alt [E][K][9] f64 (gw_fear_preview's table for the proposed joint action), actions_in / actions_out
 * [E][K] i32 (may be the same buffer), mask [E][K] u16 9-bit action masks (NULL: all nine), probs
 * [K][E][9] f32 the actor's probabilities in the replay ring's layout (NULL: none), flags [E][K] u8 or
 * NULL, agents: bit k set = agent k is shielded.  Per (e, k), proposed action p, row t, mask m
 * (csrc/fear_shield.h, the same text the CPU check runs):
 *   bit k of agents clear, or m == 0: keep p, flags 0;
 *   A = { a : bit a of m set and t[a] <= tau } (f64 compare);  p in A: keep p, flags 0;
 *   A non-empty: the a in A with the largest probs[k][e][a] (no probs: the smallest t[a]), ties to the
 *     lowest a, flags 1 (replaced);
 *   A empty: the masked a with the smallest t[a], ties to the lowest a, flags 2 (stuck), 3 if it is not p.
 * t[mdr] == 0.0 always, so with tau >= 0 A is empty only when the mask forbids the MdR.
 * The shield is UNILATERAL: every row assumes that the other agents play their proposed actions.  When
 * one agent alone is shielded (agents = 1 << k), the following step's fear[e][k] is exactly the chosen
 * entry t[actions_out[e][k]], hence <= tau wherever flag bit 1 is clear.  With several agents shielded
 * at once that holds for an agent only in the envs where every other agent's action was kept.
 * gw_fear_shield_joint (include/gridenv.h) is the coordinated form: it visits the agents one after the other
 * and returns the table of the joint action that is applied.
 * One launch, one thread per (env, agent), deterministic, graph-capturable, no host sync. */
gw_status gw_fear_shield(const double *fear_alt, const int32_t *actions_in, const uint16_t *mask,
                         const float *probs, int64_t E, int32_t K, double tau, uint32_t agents,
                         int32_t *actions_out, uint8_t *flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif
