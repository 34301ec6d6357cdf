/*
 * gridenv.h — C ABI of the MI355X-native vectorised grid world (libgridenv.so).
 *
 * Drop-in boundary for the reference's hot path (Henweiz/MARL-Responsible-Nav):
 *   CustomMAEnv.__init__/reset/step   custom/ma_customenv.py:74-108, 169-215, 217-334
 *   GWorld.UpdateGWorld               custom/grid_world.py:424-563
 *   Responsibility.FeAR_4_one_actor   custom/Responsibility.py:135-210
 *   MADDPGAgent.train per-step reward/score arithmetic   maddpg/agent.py:120-173, 226-243
 * The reference has no FFI of its own (pure Python); these entry points are what its
 * PettingZoo surface binds to through the ctypes layer in marlnav/_lib.py.
 *
 * One handle = E independent envs resident in HBM (structure of arrays).  All device
 * pointers are plain HIP device addresses (e.g. torch.Tensor.data_ptr()); `stream` is a
 * hipStream_t passed as void*.  Calls only enqueue work on `stream`; there is no implicit
 * host synchronisation.  Statuses are negative on error; gw_last_error() explains.
 * Layout: obs are agent-major [K][E][H*W] float32 (each RL agent's actor reads one
 * contiguous [E, H*W] matrix); per-env per-agent outputs are [E][K].
 */
#ifndef GRIDENV_H
#define GRIDENV_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GW_MAX_AGENTS 8
#define GW_N_ACTIONS 9

typedef enum gw_status {
    GW_OK = 0,
    GW_ERR_ARG = -1,    /* invalid argument / scenario                        */
    GW_ERR_HIP = -2,    /* HIP runtime error                                  */
    GW_ERR_ALLOC = -3,  /* device allocation failed                           */
    GW_ERR_STATE = -4   /* call order (e.g. gw_step before the first reset)   */
} gw_status;

/* Static scenario tables (host pointers, copied by gw_create).
 * Replaces LoadJsonScenario + CustomMAEnv.setup_env's map build
 * (custom/grid_world.py:621-674, custom/ma_customenv.py:338-365, 422). */
typedef struct gw_scenario {
    int32_t H, W;               /* grid rows, columns (H*W <= 4096, W >= 2)             */
    const uint8_t *region;      /* [H*W] 1 active road, 0 inactive                      */
    const uint8_t *policy_id;   /* [H*W] policy index                                   */
    int32_t n_policies;
    const double *policy_cdf;   /* [n_policies][2][9] choice CDFs; [.][1] = the 25 %
                                   uniform-direction branch (ma_customenv.py:441-443)   */
    const uint8_t *mdr;         /* [H*W] MdR action per cell                            */
    const int32_t *apples;      /* [K] apple cell of RL agent k                         */
} gw_scenario;

typedef struct gw_config {
    int32_t N;                  /* world agents  (Scenario N_Agents)          1..8      */
    int32_t K;                  /* RL agents     (N_INTELLIGENT_AGENTS)       1..N      */
    int64_t num_envs;           /* E, envs owned by this handle                          */
    int64_t env_offset;         /* global id of local env 0 (RNG counter; sharding)      */
    int32_t fear;               /* CustomMAEnv(fear=...)                                 */
    double fear_weight;         /* INIT_HP["FeAR_weight"] (maddpg/agent.py:125)          */
    int32_t max_steps;          /* TRAIN_STEPS episode cap; 0 = none                     */
    int32_t auto_reset;         /* reset done envs inside gw_step                        */
    uint64_t seed;              /* Philox key (spawns, scripted policy, random RL policy)*/
    int32_t variant;            /* 0: CustomMAEnv (custom/ma_customenv.py); 1: the single-
                                   agent CustomEnv (custom/customenv.py:78-183): K must be 1,
                                   rewards -10 crash (terminated only) / +20 apple (exactly one
                                   apples_caught entry; truncated) / +0.1 closer to the apple,
                                   step obs = raw WorldState ids (no relabel), prev distance set
                                   at reset.  Everything else is shared.                    */
} gw_config;

/* Per-step outputs: device pointers, any may be NULL (not written).  New outputs are appended
 * at the end: every existing field keeps its offset (fear_row is the latest, after desc_copy). */
typedef struct gw_step_out {
    float *obs;          /* [K][E][H*W] obs after the step (reset obs if auto-reset)  */
    float *final_obs;    /* [K][E][H*W] terminal obs; rows written only for done envs */
    double *reward;      /* [E][K] env reward                (ma_customenv.py:258-302) */
    double *fear;        /* [E][K] info["fear"]              (ma_customenv.py:245-252) */
    double *shaped;      /* [E][K] FeAR_weight*FeAR + reward (maddpg/agent.py:130)     */
    uint8_t *term;       /* [E][K] terminations                                         */
    uint8_t *trunc;      /* [E][K] truncations                                          */
    uint8_t *done;       /* [E]   all(term) | all(trunc) | t >= max_steps               */
    uint16_t *mask;      /* [E][K] 9-bit action mask of the returned obs                */
    int32_t *crashes;    /* [E]   info["agent_crashes"]                                 */
    int32_t *apples;     /* [E]   info["apples_caught"]                                 */
    double *ep_return;   /* [E]   episode score incl. this step (maddpg/agent.py:173)   */
    double *ep_fear;     /* [E]   episode fear_score (maddpg/agent.py:141)              */
    int32_t *ep_len;     /* [E]   steps in the episode incl. this one                   */
    int32_t *actions;    /* [E][N] joint action applied (env.Action4Agents)             */
    int32_t *mdr;        /* [E][N] MdR4Agents                                           */
    int32_t *final_pos;  /* [E][N] positions after the move, before any auto-reset      */
    uint8_t *crash_bits; /* [E]   bit n: agent n crashed (UpdateGWorld agent_crashes)   */
    uint8_t *restr_bits; /* [E]   bit n: restricted move                                */
    double *stats;       /* [gw_stats_rows()][GW_STATS] per-block partial sums of this step:
                            completed-episode returns, episodes completed, FeAR, crashes,
                            apples caught, shaped rewards, completed-episode lengths, envs.
                            Deterministic (fixed reduction tree); fed to the RCCL
                            reduction of the multi-GPU rollout.                          */
    uint8_t *done_copy;  /* [E]   a second destination of `done` (e.g. the per-step return
                            gather's send buffer beside the replay ring's done slot)     */
    double *stats_acc;   /* [gw_stats_rows()][GW_STATS]: every step ADDS its per-block rows
                            (a running total without a per-step reduction launch; one
                            block owns each row, so the sums are deterministic)          */
    int64_t *tick;       /* [1]   += 1 per gw_step (e.g. the replay ring's step count)   */
    uint32_t *desc_copy; /* [E][12] a second destination of the step's obs descriptors
                            (gw_obs_view's layout; e.g. a descriptor replay ring's slot,
                            include/rollout_ops.h gw_replay_gather_desc); the terminal half
                            (words 8-11) only for envs that ended                         */
    double *fear_row;    /* [E][K][N]  Resp[k][j] of FeAR_4_one_actor(actor = k)
                            (custom/Responsibility.py:135-210): the row whose np.sum is
                            `fear`[e][k]; 0.0 at j == k, for an actor that plays its MdR, and
                            everywhere with FeAR off.  The step's pre-reset joint action, as
                            `fear`; a FeAR-owned output (gw_set_obs_async | 4: gw_fear_fence)  */
} gw_step_out;

#define GW_STATS 8

/* Env state (device arrays owned by the handle), structure of arrays. */
typedef struct gw_state {
    int32_t *pos;        /* [N][E] cell r*W+c of agent n            (World.AgentLocations) */
    uint32_t *flags;     /* [E] bits 0-7 apples present, 8-15 terminations, 16-23 truncations */
    int32_t *t;          /* [E] moves in the episode                 (num_moves)          */
    uint32_t *episode;   /* [E] episode counter (RNG)                                     */
    int32_t *prev_dist;  /* [K][E] previous distance to own apple, -1 = None              */
    double *score;       /* [E] running episode score                                     */
    double *fear_score;  /* [E] running episode fear score                                */
} gw_state;

/* CustomMAEnv(render=False, fear=cfg->fear, seed=cfg->seed) x E  (ma_customenv.py:74-108).
 * Allocates the state on `device`.  The envs are unusable until gw_reset. */
gw_status gw_create(const gw_scenario *sc, const gw_config *cfg, int device, void **out_env);

/* CustomMAEnv.reset (ma_customenv.py:169-215) for every env with env_mask[e] != 0
 * (env_mask NULL = all).  spawn_cells: [E][N] sorted road cells (replay) or NULL (Philox
 * spawn).  obs [K][E][H*W] and mask [E][K] are written for the reset envs (either may be
 * NULL). */
gw_status gw_reset(void *env, const uint8_t *env_mask, const int32_t *spawn_cells, float *obs,
                   uint16_t *mask, void *stream);

/* CustomMAEnv.step (ma_customenv.py:217-334) on all E envs at once.
 *   rl_actions [E][K] int32 in 0..8, or NULL = uniform random RL policy (Philox)
 *   scripted   [E][N-K] int32 actions of the scripted agents (replay), or NULL = the
 *              scenario policy sampled on device (ma_customenv.py:432-452)
 *   spawn      [E][N] spawn cells for envs that auto-reset (replay), or NULL = Philox */
gw_status gw_step(void *env, const int32_t *rl_actions, const int32_t *scripted,
                  const int32_t *spawn, const gw_step_out *out, void *stream);

/* Device pointers of the state arrays (valid until gw_destroy). */
gw_status gw_state_view(void *env, gw_state *out);

/* Copy the whole state to (to_env = 0) or from (to_env = 1) caller buffers with the
 * gw_state layout (device or pinned host memory), enqueued on stream. */
gw_status gw_copy_state(void *env, const gw_state *buf, int to_env, void *stream);

/* Per-launch timing: while enabled, the env's kernels carry HIP timing events in their dispatch
 * (start / stop of the launch itself, on the stream each is launched on), one span per launch
 * group of a kind: GW_SPAN_STEP the world-update kernel (step_v2), GW_SPAN_OBS the obs writer
 * (obs_kernel; the merged path's step_obs), GW_SPAN_FEAR the deferred FeAR kernel (fear_v2,
 * GW_KERNEL=defer only; it runs concurrently with the writer), and the ops that take this env's
 * handle: GW_SPAN_ACT the fused actors' MLP kernel (act_kernel of gw_actor_act,
 * gw_patch_actor_act, gw_cnn_act, gw_patch_cnn_act), GW_SPAN_CNN_L1 the CNN heads' layer-1
 * listing kernel, GW_SPAN_CNN_LIST their bucket scan + unit plan and scatter (two launches), GW_SPAN_CNN_RARE
 * their recompute of the listed conv positions, GW_SPAN_WINDOW the window writer (gw_obs_patch),
 * GW_SPAN_LEARN one whole descriptor-learner update (gw_maddpg_desc_update's four launches),
 * GW_SPAN_FEAR_ALT the per-action FeAR table's kernel (fear_alt_kernel, gw_set_fear_alt),
 * GW_SPAN_FEAL the per-agent FeAL kernel (feal_kernel, gw_set_feal),
 * GW_SPAN_FEAR_FULL the N x N responsibility matrix's kernel (fear_full_kernel, gw_set_fear_full),
 * GW_SPAN_FEAR_PREVIEW the two launches of gw_fear_preview (preview_rec_kernel, fear_alt_kernel),
 * GW_SPAN_FEAR_SHIELD the two launches of gw_fear_shield_joint (preview_rec_kernel, fear_shield_joint_kernel),
 * GW_SPAN_STEP_PREVIEW the two launches of gw_step_preview (preview_rec_kernel, step_preview_kernel),
 * GW_SPAN_CRASH_SHIELD the two launches of gw_crash_shield_joint (preview_rec_kernel, crash_shield_joint_kernel),
 * GW_SPAN_STEP_LOOKAHEAD the two launches of gw_step_lookahead (preview_rec_kernel, step_lookahead_kernel),
 * GW_SPAN_STEP_HORIZON the two launches of gw_step_horizon (preview_rec_kernel, step_horizon_kernel),
 * GW_SPAN_STEP_PLAN the two launches of gw_step_plan (preview_rec_kernel, step_plan_kernel).
 * enable > 1 also makes sure `enable` timing events exist now (creating them inside a profiled
 * step would put their host cost between its launches).  gw_profile_read synchronises on those
 * events, returns the summed elapsed milliseconds of the first three kinds and the number of
 * gw_step calls timed, and clears every span.  Used by bench.py for the live roofline. */
enum {
    GW_SPAN_STEP = 0, GW_SPAN_OBS = 1, GW_SPAN_FEAR = 2, GW_SPAN_ACT = 3, GW_SPAN_CNN_L1 = 4,
    GW_SPAN_CNN_LIST = 5, GW_SPAN_CNN_RARE = 6, GW_SPAN_WINDOW = 7, GW_SPAN_LEARN = 8,
    GW_SPAN_FEAR_ALT = 9, GW_SPAN_FEAL = 10, GW_SPAN_FEAR_FULL = 11, GW_SPAN_FEAR_PREVIEW = 12,
    GW_SPAN_FEAR_SHIELD = 13 /* the two launches of one gw_fear_shield_joint (preview_rec_kernel, fear_shield_joint_kernel) */,
    GW_SPAN_STEP_PREVIEW = 14 /* the two launches of one gw_step_preview (preview_rec_kernel, step_preview_kernel) */,
    GW_SPAN_CRASH_SHIELD = 15 /* the two launches of one gw_crash_shield_joint (preview_rec_kernel, crash_shield_joint_kernel) */,
    GW_SPAN_STEP_LOOKAHEAD = 16 /* the two launches of one gw_step_lookahead (preview_rec_kernel, step_lookahead_kernel) */,
    GW_SPAN_STEP_HORIZON = 17 /* the two launches of one gw_step_horizon (preview_rec_kernel, step_horizon_kernel) */,
    GW_SPAN_STEP_PLAN = 18 /* the two launches of one gw_step_plan (preview_rec_kernel, step_plan_kernel) */
};
gw_status gw_profile(void *env, int enable);
gw_status gw_profile_read(void *env, double out_ms[3], int64_t *n_steps);
/* The spans gw_profile_read would sum, one by one (call it first: gw_profile_read clears them):
 * out[3 i + 0] = kind (GW_SPAN_*), out[3 i + 1] / [3 i + 2] = the
 * launch's start / end in milliseconds after the first span's start; at most cap spans are
 * written, *n_spans = how many exist.  Synchronises on their events.  bench.py merges the obs
 * writers' intervals (writers of consecutive steps overlap on two streams) into the writer's
 * busy time per launch. */
gw_status gw_profile_spans(void *env, double *out, int64_t cap, int64_t *n_spans);

/* Responsibility.FeAR (custom/Responsibility.py:57-132: the N x N Resp matrix, every agent as
 * actor) and FeAL (:213-303) for n world snapshots of this env's map and N, on the device:
 *   cells [n][N] agent cells, actions [n][N] the joint action, mdr [n][N] moves de rigueur
 *   (NULL = the scenario's per-cell MdR), in_list [n] bit a = agent a is in ActionID4Agents
 *   (unlisted agents stay and ignore swaps, as CustomMAEnv's close_agents lists; NULL = all);
 *   resp [n][N][N] f64, vm / va [n][N][N] ValidMoves_moveDeRigueur / _action, feal [n][N] f64,
 *   feal_vm / feal_va [n][N] (each output but resp may be NULL).  Enqueued on stream. */
gw_status gw_fear_matrix(void *env, int64_t n, const int32_t *cells, const int32_t *actions,
                         const int32_t *mdr, const uint8_t *in_list, double *resp, int32_t *vm,
                         int32_t *va, double *feal, int32_t *feal_vm, int32_t *feal_va, void *stream);

/* Rows of the gw_step_out.stats buffer (one per kernel block; GW_KERNEL=defer: the world-update
 * kernel's rows then fear_v2's rows, each kernel filling the fields it owns, zeros elsewhere). */
int64_t gw_stats_rows(void *env);

/* The kernel path gw_create chose: 3 "defer", 4 "merged" (values 0-2 named the round-1..5 A/B
 * paths "v1", "split", "fused", removed in round 6).  "merged" when a step's obs is at most
 * GW_MERGE_BYTES (default 160 MiB: small batches, bound by the step's latency chain, gain from
 * one step_obs launch per pipelined step), else "defer"; GW_KERNEL=defer|merged forces one (both
 * produce the same results).  -1 on a null handle. */
int64_t gw_kernel_path(void *env);

/* After replaying (on `stream`) a HIP graph of captured gw_step calls: the env's host-side
 * pipeline state is again the one the capture ended in (merged path with async obs: the
 * writer of the last captured step is queued, for the next gw_step or fence).  The capture
 * itself leaves that state; a fence between replays clears it, this re-arms it. */
gw_status gw_graph_replayed(void *env, void *stream);

/* The host-side pipeline state of the merged path's async obs (the queued writer's parameters,
 * the descriptor buffer in use) as an opaque blob of gw_pipeline_state_bytes() bytes.  For callers
 * that capture several HIP graphs of steps writing DIFFERENT buffers (a replay ring's slots, one
 * graph per ring phase): save the state after capturing each graph and load it after replaying
 * that graph, so the next eager step, graph or fence launches the right queued writer (on
 * `stream`).  Synchronous obs leaves nothing queued; the defer path's pipeline is not capturable. */
int64_t gw_pipeline_state_bytes(void);
gw_status gw_pipeline_save(void *env, void *buf);
gw_status gw_pipeline_load(void *env, const void *buf, void *stream);

/* What the observation an env last wrote (gw_reset / gw_step) is made of, for ops that work
 * on it without reading it back (actor_ops.h): the static step-encoding map plus, per env, a
 * 48-byte descriptor (agent cells, reset / apple flags; ma_customenv.py:197-209, 303-322).
 * Device pointers owned by the handle, valid until gw_destroy; contents change with every
 * gw_reset / gw_step (stream-ordered; with async obs the desc pointer alternates per step). */
typedef struct gw_obs_source {
    const uint32_t *desc;      /* [E][12] u32: words 0-3 agent cells (16 bits each), word 4
                                  flags (bit 0 reset encoding, bits 8-15 apples present)      */
    const float *base;         /* [H*W] 0 road, -1 inactive                                   */
    int32_t apples[GW_MAX_AGENTS];  /* apple cell of RL agent k                               */
    int32_t N, K, H, W, variant;
    int64_t E, env_offset;
} gw_obs_source;
gw_status gw_obs_view(void *env, gw_obs_source *out);

/* Copy the descriptors of the last gw_reset / gw_step ([E][12] u32, as gw_obs_view's desc) to
 * dst, enqueued on stream after that step (a replay ring of descriptors: gw_replay_gather_desc,
 * include/rollout_ops.h). */
gw_status gw_obs_desc_copy(void *env, uint32_t *dst, void *stream);

/* Count the FeAR counterfactual world updates (custom/Responsibility.py:16-54's sims, after the
 * exact de-duplication of DESIGN §5.2: one base sim per (actor, variant) and the 8 other actions of
 * each close affected agent per variant) the env's FeAR kernels run from now on: every block adds
 * its task count to *counter (device uint64, one atomic per block per step).  counter NULL: stop
 * counting (the default).  bench.py reports sims/s from it beside the VALU roofline. */
gw_status gw_count_sims(void *env, uint64_t *counter);

/* Every following gw_step also writes fear_alt [E][K][9] f64 (NULL: off, the default):
 * fear_alt[e][k][a] = np.sum(Resp) of FeAR_4_one_actor(actor = k) on the step's pre-move world with
 * the step's joint action, except that agent k plays a; k's close set and MdR as in the step.
 * So fear_alt[e][k][actions[e][k]] == fear[e][k] and fear_alt[e][k][mdr[e][k]] == 0.0, bit for bit
 * (the same Resp table and numpy-ordered sum); with FeAR off (cfg.fear == 0) the step stores zeros.
 * It describes the pre-reset world of the step, as `fear`.  A FeAR-owned output: ordered on the
 * caller's stream like `fear`, with gw_set_obs_async(| 4) ready after gw_fear_fence.  One more kernel
 * per step (fear_alt_kernel: one wave per env, 9 (1 + 8 (c - 1)) world updates per actor with close
 * count c), launched after the world update beside the obs writer; gw_count_sims counts its sims
 * too.  The pointer is kept in the env (not in gw_step_out), so captured steps replay it.  May be
 * called any time after gw_create; GW_ERR_ARG on a null env. */
gw_status gw_set_fear_alt(void *env, double *fear_alt);

/* Every following gw_step also writes, for every world agent i (all N, not only the K RL agents),
 * Responsibility.FeAL (custom/Responsibility.py:213-303) of the step's pre-move world with the step's
 * full joint action list and MdR4Agents (every agent listed) -- what gw_fear_matrix(in_list = NULL)
 * gives for that snapshot:
 *   feal [E][N] f64: clip(va / (vm + 1e-6), -1, 1), from a 10 x 10 table computed on the host at
 *     gw_create (no division on the device);
 *   feal_valid [E][N][2] u16: bit b of [..][0] / [..][1] = action b of agent i is valid (neither
 *     crashed nor restricted) while every other agent plays its MdR / its actual action: the
 *     reference's Validity_of_Moves_MdR_FeAL / _action_FeAL as bit sets; vm / va are their popcounts.
 * Both NULL: off (the default); either alone may be NULL; feal_valid must be 4-byte aligned.  Both
 * describe the pre-reset world of the step, as `fear`.  FeAR-owned outputs: ordered on the caller's
 * stream like `fear`, with gw_set_obs_async(| 4) ready after gw_fear_fence.  One more kernel per step
 * (feal_kernel: one wave per env, at most 18 N world updates), launched where fear_alt_kernel is;
 * gw_count_sims counts its sims too.  The pointers are kept in the env, so captured steps replay them.
 * FeAL is computed from the record the FeAR-on step kernels keep: on an env created with
 * cfg.fear == 0 arming fails with GW_ERR_STATE (create the env with FeAR on, and fear_weight = 0 if
 * the shaped reward must equal the env reward).  GW_ERR_ARG on a null env. */
gw_status gw_set_feal(void *env, double *feal, uint16_t *feal_valid);

/* Every following gw_step also writes Responsibility.FeAR (custom/Responsibility.py:57-132) of the
 * step's pre-move world with every world agent as actor (the scripted ones included) and every agent
 * listed -- what gw_fear_matrix(in_list = NULL) gives for that snapshot, bit for bit:
 *   resp_full [E][N][N] f64: resp_full[e][i][j] = clip((vm - va) / (vm + 1e-6), -1, 1), how much actor i
 *     restricted agent j, from the 10 x 10 table computed on the host at gw_create; the diagonal is 0.0;
 *   resp_valid [E][N][N][2] u16: bit b of [..][i][j][1] = action b of agent j is valid (neither crashed
 *     nor restricted) with the step's action list unchanged except that j plays b, of [..][i][j][0] the
 *     same with actor i swapped to its MdR: ValidMoves_action / _moveDeRigueur as bit sets, va / vm
 *     their popcounts; the diagonal is zero.  [..][i][j][1] does not depend on i.
 * Both NULL: off (the default); either alone may be NULL; resp_valid must be 4-byte aligned.  Rows of
 * this matrix list every agent; gw_step_out.fear_row lists the step's close agents only, so the two
 * agree where the close set is full.  Conventions of gw_set_feal: pre-reset world; FeAR-owned outputs
 * ordered by gw_fear_fence; the pointers are kept in the env, so captured steps replay the writes;
 * GW_ERR_STATE on an env created with cfg.fear == 0; GW_ERR_ARG on a null env.  One more kernel per step
 * (fear_full_kernel: one wave per env, 9 N + 9 (N - 1) d <= 9 N^2 world updates with d the agents
 * off their MdR), launched behind feal_kernel's place; gw_count_sims counts its sims too. */
gw_status gw_set_fear_full(void *env, double *resp_full, uint16_t *resp_valid);

/* The forward-looking twin of gw_set_fear_alt: the per-action FeAR table of the step that
 * gw_step(env, rl_actions, scripted, ...) WOULD run next, without moving the world.
 *   fear_alt [E][K][9] f64: what gw_set_fear_alt's table would hold after that gw_step, provided nothing
 *     else touches the env in between, bit for bit (the same fear_alt_kernel, Resp table and numpy-ordered
 *     sum): agent k's FeAR had it played action a on the current world while everybody else plays the
 *     action the step will apply.  fear_alt[e][k][mdr[e][k]] == 0.0.
 *   actions [E][N] i32 or NULL: the joint action that step will apply (gw_step_out.actions);
 *   mdr [E][N] i32 or NULL: the current cells' MdR (gw_step_out.mdr).
 * rl_actions [E][K] / scripted [E][N-K] as gw_step's; NULL: the device-random RL policy / the scenario
 * policy, drawn with the Philox counters (seed; global env, episode, step, agent) the step itself uses,
 * so the draws are the step's.  Works on an env created with cfg.fear == 0 too (it needs no record from a
 * step kernel) and then gives the table of a FeAR-on twin with the same seed.
 * It changes no env state, no step output, no pipeline state and no obs-destination table, and it does
 * not touch the steps' record buffer: it keeps one of its own, [E] records, allocated by the first call
 * (a first call while `stream` is capturing returns GW_ERR_STATE; later calls can be captured).  No host
 * synchronisation: two launches enqueued on `stream` (preview_rec_kernel, one thread per env, then
 * fear_alt_kernel), one GW_SPAN_FEAR_PREVIEW span while profiling; gw_count_sims counts the world updates.
 * Every path of gw_step orders its world update before the caller's later work on the step's stream, so
 * a preview enqueued there after a step sees that step's state (with gw_set_obs_async(| 4) as well).
 * GW_ERR_STATE before the first gw_reset; GW_ERR_ARG on a null env or a null table. */
gw_status gw_fear_preview(void *env, const int32_t *rl_actions, const int32_t *scripted, double *fear_alt,
                          int32_t *actions, int32_t *mdr, void *stream);

/* Egocentric local patches of the env's last observation (an opt-in input format; the
 * reference observes the whole grid, ma_customenv.py:303-322): for every env and RL agent k the
 * P x P window of that agent's obs centred on its own cell (rows / cols -P/2 .. P-1-P/2), cells
 * outside the grid -1.  patch [K][E][P][P] f32 (envs whose obs the last gw_step / gw_reset
 * wrote), final_patch [K][E][P][P] (the terminal obs of envs done at the last step, centred on
 * the terminal cell); either may be NULL.  Works from the descriptors, so it needs no full obs
 * (gw_step_out.obs may be NULL).  Enqueued on stream, after the step on the same stream. */
gw_status gw_obs_patch(void *env, int32_t P, float *patch, float *final_patch, void *stream);
/* Arm the NEXT gw_step to also write its P x P windows exactly as gw_obs_patch(env, P, patch,
 * final_patch) right after it would: with FeAR on (joined) and the row writer's conditions
 * (2 <= P <= 16, E % 4 == 0) inside the FeAR launch (both read only the world update's outputs),
 * else as that gw_obs_patch on the step's stream.  One request per step (cleared by gw_step). */
gw_status gw_step_patch_next(void *env, int32_t P, float *patch, float *final_patch);

/* Async observation writes (a software pipeline across steps; default off).  While enabled,
 * gw_step enqueues the world update (+ FeAR) on an internal stream that waits for the caller's
 * prior work on `stream`, and `stream` joins it: rewards, dones, masks, state and stats are
 * stream-ordered as in the synchronous mode.  The observation writer of the step runs on a
 * second internal stream and overlaps the NEXT step's world update (which reads only the
 * state).  The obs / final_obs buffers of a step are therefore ready on `stream` only after
 * gw_obs_fence(env, stream) (or gw_reset, which fences itself).  The obs descriptor alternates
 * between two buffers: re-read gw_obs_view after every gw_step.  Disabling drains the writer.
 * enable = 1: the writer starts right after the step's world update; enable = 2 (lazy): it is
 * launched at the start of the next gw_step (behind the caller's work between the steps, e.g.
 * an actor kernel that should not share the CUs with it) or at a fence.
 * enable | 4 (defer path, FeAR on): `stream` joins only the world update; fear_v2 (fear,
 * shaped, ep_return, ep_fear, the FeAR stats rows, score / fear_score) finishes on the internal
 * stream and overlaps the caller's next work (an actor that needs only the descriptors and
 * masks); those outputs, and fear_row, are ready on `stream` after gw_fear_fence (gw_reset, gw_copy_state
 * and the next gw_step order themselves).
 * Both kernel paths pipeline (defer: the writer on its own streams; merged: one step_obs launch). */
gw_status gw_set_obs_async(void *env, int enable);

/* Observation element type of every obs / final_obs buffer the env writes (gw_reset, gw_step):
 * GW_OBS_F32 (default; the reference's values as float32) or GW_OBS_BF16 (the same values as
 * bfloat16 bits, [K][E][H*W] uint16: every value the env produces is exact in bf16, so this is
 * lossless and halves the obs bytes; needs H*W % 8 == 0).
 * The float* obs pointers then address bf16 buffers.  Called before the first gw_reset it may
 * also change gw_stats_rows (the FeAR kernel's envs per block follow the format's best choice):
 * size the stats buffer after it. */
enum { GW_OBS_F32 = 0, GW_OBS_BF16 = 1 };
gw_status gw_set_obs_dtype(void *env, int dtype);

/* The delta obs writer (default off).  An observation is the static map plus at most N + 1 patched
 * cells per (env, RL agent), so a buffer that already holds an obs this env wrote differs from the
 * next obs written there in at most 2 K (N + 1) cells per env.  While on, the env keeps a table of
 * GW_OBS_DESTS obs destinations it wrote last (least recently used evicted): the pointer, the dtype,
 * a device copy of the descriptors written there and the last writer's event.  A gw_step whose
 * gw_step_out.obs has a valid entry stores only the changed cells (obs_delta_kernel, ordered after
 * the previous writer of that buffer); any other step runs the full writer, which fills the entry.
 * The results are the same bit for bit.  final_obs always takes the full writer's path.
 * THE CALLER'S PROMISE while on: between two gw_steps that write the same obs pointer nothing else
 * writes those bytes (a fill, a copy into the buffer, another env, freeing the buffer and getting
 * the address back for another one), or the caller calls gw_obs_dest_forget(env, ptr) before the
 * second step (ptr NULL: every entry).  The library cannot see such writes: a pointer says nothing
 * about the bytes behind it.  marlnav.VecGridEnv keeps that promise for writes torch can see (it
 * holds the tensor and compares its version counter); writes through raw pointers need the call.
 * Always the full writer, and no entry survives: the merged kernel path, bf16 obs, gw_set_obs_dtype,
 * gw_reset, gw_pipeline_load, gw_graph_replayed (call one of the two after replaying a graph of
 * captured steps, or forget), and steps recorded while the stream is capturing.
 * gw_obs_delta_counts: out[0] / out[1] = gw_steps whose obs the full / the delta writer wrote.
 *
 * The ride.  On the defer path with FeAR on (joined, wide blocks), an eager async step
 * (gw_set_obs_async(env, 1)) whose delta writer covers the whole env range in one launch
 * (GW_OBS_CHUNKS unset or 1, no final_obs, profiling off, `stream` not capturing) runs that writer
 * as a block role of the FeAR launch on `stream` itself (fear_delta_kernel): the step is two
 * launches on the caller's stream and uses no internal stream, event or cross-queue wait.  After
 * such a step the obs are ordered on `stream` like every other output of the step, and gw_obs_fence
 * has nothing to wait for (calling it stays correct and cheap; a caller that reads the obs on
 * another stream orders that stream after `stream`, as for rewards and dones).  Every other step
 * takes the pipeline above unchanged, and the two forms may alternate from step to step.
 * gw_set_obs_ride(env, 0) turns the ride off and (env, 1) on again, between any two steps (only 0
 * or 1, else GW_ERR_ARG; A/B: the results are the same bit for bit); marlnav.VecGridEnv calls it
 * with GW_OBS_RIDE from the environment when it creates an env.  gw_obs_ride_count: the gw_steps
 * whose writer rode (each of them counts as a delta write in gw_obs_delta_counts too). */
#define GW_OBS_DESTS 8
gw_status gw_set_obs_delta(void *env, int on);
gw_status gw_obs_dest_forget(void *env, const void *ptr);
gw_status gw_obs_delta_counts(void *env, int64_t out[2]);
gw_status gw_set_obs_ride(void *env, int on);
gw_status gw_obs_ride_count(void *env, int64_t *out);

/* The FeAR kernel's envs per block, before the first gw_reset (it fixes gw_stats_rows: size the
 * stats buffer after it): wide = 1, 0 = narrow (half the envs per block).  The rule for the default:
 * wide for f32 obs (gw_create), narrow once gw_set_obs_dtype selects bf16 obs before the first
 * gw_reset; a caller whose env writes no full obs (the local-window rollouts) asks for narrow here
 * (c5patch 115 -> 111-112 us per step).  fear_v2's wide blocks are 64 envs on 256 threads (one lane
 * per (env, actor) in its per-env phases, four waves for the counterfactual sims), its narrow blocks
 * and fear_rows_kernel's blocks 128 threads; the statistics rows depend on the envs per block only.
 * GW_FEAR_BE=wide|narrow in the environment overrides it.  GW_ERR_STATE after gw_reset. */
gw_status gw_set_fear_blocks(void *env, int wide);
gw_status gw_obs_fence(void *env, void *stream);
gw_status gw_fear_fence(void *env, void *stream);
/* Set the thread-local error text returned by gw_last_error (for the library's other
 * translation units: learner_ops, actor_ops). */
void gw_set_last_error(const char *msg);
/* Sizes: H, W, N, K, E (out[0..4]). */
gw_status gw_dims(void *env, int64_t out[5]);

/* Thread-local description of the last error. */
const char *gw_last_error(void);

void gw_destroy(void *env);

/* The coordinated responsibility shield: gw_fear_preview and gw_fear_shield (include/rollout_ops.h) composed
 * over the RL agents one after the other, in one call, and the table of the joint action that will actually be
 * applied.  gw_fear_shield is unilateral: each agent's row assumes that the others keep their proposed actions,
 * so with several agents shielded at once its promise fails exactly in the envs where somebody else was
 * replaced.  Here every visit sees the actions the agents before it have fixed.  Per env, with `scripted` the
 * scripted agents' actions and prop[k] the proposed RL actions (given, or NULL = drawn with the step's own
 * Philox counters, exactly as gw_fear_preview does):
 *   cur = prop
 *   for s in 1..sweeps:
 *     changed = false
 *     for k in 0..K-1 ascending, where bit k of `agents` is set:
 *       t = row k of gw_fear_preview's table for the joint action (cur, scripted)
 *       r = the pick of csrc/fear_shield.h (gw_fear_shield's rule) on (t, cur[k], mask[k], probs of k, tau)
 *       stuck[k] = bit 1 of r's flags            (the last visit's answer)
 *       if r.action != cur[k]: cur[k] = r.action, changed = true
 *     if not changed: break
 *   T = gw_fear_preview's table for (cur, scripted)
 * Outputs: actions_out [E][K] = cur (required; may alias rl_actions); fear_alt [E][K][9] f64 = T, bit for bit
 * gw_fear_preview's; joint [E][N] = the joint action the step will apply; flags [E][K] u8 (each of the three
 * may be NULL):
 *   bit 0  cur[k] != prop[k];
 *   bit 1  stuck[k]: the agent's last visit found no allowed action;
 *   bit 2  "over": agent k is shielded and T[k][cur[k]] > tau (f64 compare): the promise does not hold here;
 *   bit 3  "unconverged": the last sweep that ran changed something; set on all K entries of the env.
 * An agent whose current action is still allowed keeps it; an unshielded agent is never visited and its flags are
 * 0 apart from bit 3; agents == 0 sets nothing.  A proposed action outside 0..8 is read as 0 (stay), which is
 * what gw_step and gw_fear_preview apply for it: prop, actions_out and bit 0 all speak of that 0.
 * It follows that
 *   - T[e][k][actions_out[e][k]] is bit for bit the fear[e][k] of the gw_step that applies actions_out (and the
 *     same scripted actions), for every k, shielded or not;
 *   - where bit 2 is clear, that step's fear[e][k] <= tau;
 *   - in an env with bit 3 clear every shielded agent with bit 1 clear and a non-zero mask has bit 2 clear (the
 *     unchanged sweep saw the final joint action; an agent whose mask is 0 is kept whatever its FeAR, flags 0);
 *   - sweeps = 1, agents = 1 << k gives gw_fear_shield's actions_out and flag bits 0-1 for that k.
 * mask [E][K] u16 9-bit action masks (NULL: all nine), probs [K][E][9] f32 in the replay ring's layout (NULL:
 * none), agents: bit k = RL agent k is shielded, sweeps in 1..GW_SHIELD_MAX_SWEEPS.
 * Conventions of gw_fear_preview: works on cfg.fear == 0 envs; changes no env state, step output, pipeline state
 * or obs-destination table; shares the preview's record buffer (a first call of either while `stream` captures
 * returns GW_ERR_STATE, later calls can be captured); no host synchronisation; GW_ERR_STATE before the first
 * gw_reset; GW_ERR_ARG on a null env, null actions_out or sweeps out of range.
 * Cost: two launches on `stream` (preview_rec_kernel, then fear_shield_joint_kernel: one wave per env, every
 * visit and the final table in it), one GW_SPAN_FEAR_SHIELD span while profiling.  A visit of agent k runs its
 * 9 (1 + 8 (c_k - 1)) world updates (close count c_k); the final table runs those of all K agents, or, when
 * the last sweep changed nothing, only those of the unshielded ones (the shielded agents' rows are then the
 * visits').  gw_count_sims counts them all.  The composed form costs sweeps x K previews (K rows each) and
 * sweeps x K shield launches plus one preview. */
#define GW_SHIELD_MAX_SWEEPS 8
gw_status gw_fear_shield_joint(void *env, const int32_t *rl_actions, const int32_t *scripted,
                               const uint16_t *mask, const float *probs, double tau, uint32_t agents,
                               int32_t sweeps, int32_t *actions_out, uint8_t *flags, double *fear_alt,
                               int32_t *joint, void *stream);

/* The step outcome preview: crash bits, restricted bits and env reward of the step that
 * gw_step(env, rl_actions, scripted, ...) WOULD run next, under each of the nine actions of each RL agent,
 * without moving the world.  For every env e, RL agent k < K and action a in 0..8 one real UpdateGWorld
 * (custom/grid_world.py:424-563) of the current world: the FULL joint action that gw_step will apply (far agents
 * move too: not FeAR's close-list variant) with agent k playing a instead, eaters 0..K-1, the apples still present.
 *   outcome [E][K][9] u16 (required): bits 0-7 that update's crash bits of all N agents (gw_step_out.crash_bits),
 *     bits 8-15 its restricted bits (restr_bits);
 *   reward_alt [E][K][9] f64 or NULL: the env reward gw_step_out.reward[e][k] the step would pay agent k
 *     (ma_customenv.py:258-302; variant 1: customenv.py:127-160): the own apple once, the all-eaten +20, -10 on
 *     a crash, +1 / +0.1 for moving closer, from the env's present apples and prev_dist, bit for bit.  It does
 *     not depend on FeAR;
 *   crash9 [E][K] u16 or NULL: bit a set when agent k ITSELF crashes under a (bit k of outcome[e][k][a]);
 *   safe_mask [E][K] u16 or NULL: m & ~crash9 with m = mask[e][k] (mask [E][K] 9-bit action masks; NULL: 0x1FF);
 *     if that is empty, m unchanged (nothing avoids the crash).  The rule is csrc/step_preview.h's.  Passed to
 *     gw_fear_shield (include/rollout_ops.h) in the action mask's place it makes the shield crash-aware; with
 *     a zero table and tau = 0 only crashing proposals are replaced, by the most probable safe action;
 *   actions [E][N] i32 or NULL: the joint action that step will apply (gw_step_out.actions).
 * rl_actions / scripted as gw_fear_preview's: NULL draws with the step's own Philox counters.  So
 * outcome[e][k][actions[e][k]] == crash_bits[e] | restr_bits[e] << 8 and reward_alt[e][k][actions[e][k]] ==
 * reward[e][k] of that gw_step, for every k.
 * The preview is UNILATERAL, as gw_fear_shield's rows are: each entry assumes that the other agents play their
 * proposed actions.  An agent moved to a safe action does not crash in the step only in envs where every other
 * agent's action was kept.
 * Conventions of gw_fear_preview: works on cfg.fear == 0 envs; changes no env state, step output, pipeline state
 * or obs-destination table; keeps a record buffer of its own, allocated by the first call (a first call while
 * `stream` captures returns GW_ERR_STATE, later calls can be captured); no host synchronisation; GW_ERR_STATE
 * before the first gw_reset; GW_ERR_ARG on a null env or a null outcome.
 * Cost: two launches on `stream` (preview_rec_kernel, then step_preview_kernel: one wave per env, the K x 9
 * tasks (k, a) dealt to its lanes, one register-resident world update per lane and turn; K = 8: 72 tasks, two
 * turns), one GW_SPAN_STEP_PREVIEW span while profiling; gw_count_sims counts the 9 K world updates per env. */
gw_status gw_step_preview(void *env, const int32_t *rl_actions, const int32_t *scripted, const uint16_t *mask,
                          uint16_t *outcome, double *reward_alt, uint16_t *crash9, uint16_t *safe_mask,
                          int32_t *actions, void *stream);

/* The two-step crash lookahead: gw_step_preview's own-crash sets for the step that gw_step(env, rl_actions,
 * scripted, ...) WOULD run next, and for the step after it, without moving the world.  The crash-aware shields
 * look one step ahead, and a crash they flag unavoidable was usually avoidable one step earlier: the agent had
 * stepped into a cell from which every action crashes.  Arguments and preconditions are gw_step_preview's.
 * Stage 1, for every env e, RL agent k < K and first action a in 0..8, is exactly gw_step_preview's task: the real
 *   world update of the step about to run under the joint action that step would apply (the proposals or the
 *   step's own device-random draws, `scripted` or the step's Philox draws) with agent k playing a, eaters 0..K-1,
 *   the env's apples still present.
 * ends [E][K] u16: bit a set when that step ends the episode, by the step's own `done` rule: all terminated, or
 *   all truncated, or t + 1 >= max_steps.  In the multi-agent variant any RL crash truncates every agent, so bit a
 *   is also set where ANOTHER RL agent's crash ends the episode while k itself is fine; the all-eaten truncation
 *   counts; variant 1 ends on the own crash or on the apple.
 * Stage 2 runs only where bit a of ends is clear: the world is stage 1's final cells at time t + 1 of the same
 *   episode.  Scripted agents n >= K play their Philox draw of step t + 1 from their stage-1 final cell (always the
 *   Philox law: a caller's `scripted` override applies to stage 1 only); RL agent k plays b in 0..8; EVERY OTHER RL
 *   AGENT PLAYS ACTION 0 (stay).  That is the one assumption: stage 2 is exact for K = 1, and wherever the others do
 *   stay.  One real world update per (k, a, b).
 * crash2 [E][K][9] u16: bit b of crash2[e][k][a] set when k itself crashes in stage 2; 0 where the step ends under a.
 * crash9 [E][K] u16: gw_step_preview's, bit for bit.
 * trap9 [E][K] u16: with mask2 the cell table's action-mask bits of k's stage-1 final cell under a (the mask the
 *   step would return), bit a is set when the step does not end under a, mask2 != 0 and
 *   (mask2 & ~crash2[e][k][a]) == 0: after a, every action that cell allows crashes k.
 * ahead_mask [E][K] u16: m & ~crash9 & ~trap9 with m = mask[e][k] (mask [E][K] 9-bit action masks; NULL: 0x1FF);
 *   where that is empty, gw_step_preview's safe_mask(m, crash9).  The rules are csrc/step_lookahead.h's.  Passed to
 *   gw_fear_shield in the action mask's place it makes the shield avoid trap actions as well as crashes.
 * Each of crash2, ends, crash9, trap9 and ahead_mask may be NULL; actions / mdr [E][N] i32 or NULL: the joint
 * action that step will apply and the cells' MdR (gw_step_out.actions / .mdr).
 * The promise: suppose the step applies the previewed joint action with k playing a, and the episode does not
 * end.  Then crash2[e][k][a] is, bit for bit, the crash9[e][k] that gw_step_preview returns before the following
 * step when every RL agent proposes 0.
 * Conventions of gw_step_preview: works on cfg.fear == 0 envs; changes no env state, step output, pipeline state or
 * obs-destination table; uses gw_step_preview's record buffer, allocated by the first call of either (a first call
 * while `stream` captures returns GW_ERR_STATE, later calls can be captured); no host synchronisation;
 * GW_ERR_STATE before the first gw_reset; GW_ERR_ARG on a null env or a u16 array that is not 2-byte aligned.
 * Cost: two launches on `stream` (preview_rec_kernel, then step_lookahead_kernel: one wave per env; the K x 9
 * stage-1 tasks dealt to its lanes, their final cells and the (N - K) x 9 K scripted draws of step t + 1 kept in
 * LDS, then up to K x 81 stage-2 tasks, one register-resident world update per lane and turn), one
 * GW_SPAN_STEP_LOOKAHEAD span while profiling; gw_count_sims counts 9 K + 9 x (the number of (k, a) whose step
 * does not end) world updates per env. */
gw_status gw_step_lookahead(void *env, const int32_t *rl_actions, const int32_t *scripted, const uint16_t *mask,
                            uint16_t *crash2, uint16_t *ends, uint16_t *crash9, uint16_t *trap9, uint16_t *ahead_mask,
                            int32_t *actions, int32_t *mdr, void *stream);

/* The crash horizon: for each RL agent k and first action a, how many of the next H steps k can survive, without
 * moving the world.  gw_step_lookahead looks two steps ahead; most agent-steps it leaves without a crash-free,
 * trap-free action need a longer horizon.  `horizon` is H, 2 <= H <= GW_HORIZON_MAX.  Arguments and preconditions
 * are gw_step_lookahead's.
 * Step 1, for every env e, RL agent k < K and first action a in 0..8, is exactly gw_step_preview's task: the real
 *   world update of the step about to run under the joint action that step would apply (`scripted` or the step's
 *   Philox draws) with agent k playing a, eaters 0..K-1, the env's apples still present.  crash9 [E][K] u16 and
 *   ends [E][K] u16 are gw_step_lookahead's, bit for bit.
 * Steps 2..H exist only while the episode goes on.  In step i the scripted agents n >= K play their Philox draw of
 *   step t + i - 1 from their own cells (always the Philox law: a caller's `scripted` override applies to step 1
 *   only), agent k plays an action b that the cell table's action-mask bits of the cell it stands in allow (the
 *   mask2 rule of trap9), and EVERY OTHER RL AGENT PLAYS ACTION 0 (stay).  That is the one assumption: the steps are
 *   exact for K = 1, and wherever the others do stay.  There are no apples after step 1: a later step ends the
 *   episode only by an RL agent's crash or by the step cap (t + i >= max_steps, max_steps > 0).  This is
 *   conservative: an all-eaten end after step 1, which would count as survival, is ignored.
 * depth [E][K][9] u8 in 0..H: the largest d for which some continuation exists in which k itself does not crash in
 *   the steps 1..d.  A continuation that reaches an episode end without k's own crash (another RL agent's crash,
 *   the cap, an apple or all-eaten end of step 1) counts as H; so does one that leaves k in a cell whose action
 *   mask is empty (trap9 reads an empty mask2 the same way).  At H = 2: depth 0 = a crashes k (crash9), depth 1 =
 *   a is a trap action (gw_step_lookahead's trap9), depth 2 = neither.
 * viable9 [E][K] u16: bit a set iff depth[e][k][a] == H.
 * horizon_mask [E][K] u16: with m = mask[e][k] (mask [E][K] 9-bit action masks; NULL: 0x1FF), the actions of m whose
 *   depth is the maximum over m; m == 0 gives 0.  At H = 2 it equals gw_step_lookahead's ahead_mask bit for bit.
 *   The rules are csrc/step_horizon.h's.  Passed to gw_fear_shield in the action mask's place it makes the shield
 *   pick among the actions that keep the agent alive longest.
 * Each of depth, ends, crash9, viable9 and horizon_mask may be NULL; actions / mdr [E][N] i32 or NULL: the joint
 * action that step will apply and the cells' MdR (gw_step_out.actions / .mdr).
 * How it is computed: while k has not crashed the world differs between k's choices in k's own cell only (an agent
 * changes another agent's cell only through a collision, a collision marks both agents crashed, and an RL crash
 * ends the episode), so level h (the world after h survived steps) is one background, the other agents' cells and
 * actions, and a set of distinct cells of k within Manhattan distance 2 h.
 * Conventions of gw_step_lookahead: works on cfg.fear == 0 envs; changes no env state, step output, pipeline state
 * or obs-destination table; uses gw_step_preview's record buffer, allocated by the first call of any of the three
 * (a first call while `stream` captures returns GW_ERR_STATE, later calls can be captured); no host
 * synchronisation; GW_ERR_STATE before the first gw_reset; GW_ERR_ARG on a null env (before any device use), a
 * horizon outside 2..GW_HORIZON_MAX or a u16 array that is not 2-byte aligned.
 * Cost: two launches on `stream` (preview_rec_kernel, then step_horizon_kernel: one wave per env, the RL agents in
 * turn), one GW_SPAN_STEP_HORIZON span while profiling.  gw_count_sims counts, per env, 9 K for step 1 plus, for
 * each k and each level h = 1..H - 1 that is reached (some first action, or some update of level h - 1, left k
 * uncrashed with the episode going on), one world update per distinct cell k can stand in at that level and per
 * action that cell's mask allows.  Every update is counted once; a level's background needs no update of its own
 * (it is read from the lowest-numbered update of the level before that goes on). */
#define GW_HORIZON_MAX 4
gw_status gw_step_horizon(void *env, const int32_t *rl_actions, const int32_t *scripted, const uint16_t *mask, int horizon,
                          uint8_t *depth, uint16_t *ends, uint16_t *crash9, uint16_t *viable9, uint16_t *horizon_mask,
                          int32_t *actions, int32_t *mdr, void *stream);

/* The reward horizon: for each RL agent k and first action a, how many of the next H steps k can survive AND the
 * largest env reward those steps can pay it, without moving the world.  gw_step_horizon tells which first actions
 * keep k alive; it removes the apples after step 1, so it cannot tell which of them is worth taking.  Arguments,
 * preconditions, status codes and capture rules are gw_step_horizon's; `horizon` is H, 2 <= H <= GW_HORIZON_MAX.
 * Step 1 is exactly gw_step_preview's task, and its reward is reward_alt[e][k][a], bit for bit, times 10.
 * Steps 2..H run the real world update WITH apples (eaters 0..K-1) while the episode goes on: every other RL agent
 *   plays 0 (stay; the one assumption, exact for K = 1), the scripted agents play their recomputed Philox draws (a
 *   caller's `scripted` override holds for step 1 only), and agent k plays an action the action mask of the cell it
 *   stands in allows.  Each step carries the apples, the term / trunc flags and k's prev_dist that the steps before
 *   it left; its `done` and its reward for k are the step's own rules on that state, so eating the env's last apple
 *   ends the episode, and so do the step cap and another RL agent's crash.
 * depth [E][K][9] u8 in 0..H: gw_step_horizon's definition on this world: the largest d for which some continuation
 *   keeps k from crashing in the steps 1..d; an episode end without k's own crash, the horizon, or a cell whose
 *   action mask is empty counts as H.  (It is never below gw_step_horizon's depth: the apples add episode ends.)
 * ret [E][K][9] i16, in tenths of a reward unit: the largest sum of env rewards the steps of a continuation pay
 *   agent k, over the continuations that reach depth[e][k][a].  Continuations are ordered lexicographically by
 *   (depth, return): survival first, return second.  A continuation that ends below H includes its one crash (-100);
 *   a continuation stops at an episode end, at the horizon, and in a cell that allows nothing.
 * path [E][K][9][GW_HORIZON_MAX - 1] u8: the actions after a of the continuation that attains (depth, ret); ties go
 *   to the lowest action at every level.  The crash step, the step that ends the episode and step H are the path's
 *   last entry; entries past the end are 0xFF (all of them where a itself crashes k or ends the episode).
 * ends, crash9 [E][K] u16: gw_step_horizon's, bit for bit.
 * plan_mask [E][K] u16: with m = mask[e][k] (mask [E][K] 9-bit action masks; NULL: 0x1FF), the actions of m whose
 *   (depth, ret) is the lexicographic maximum over m; m == 0 gives 0.  Its actions all have the maximal depth over
 *   m, so it is a subset of what gw_step_horizon's rule gives on this depth table.  Passed to gw_fear_shield in the
 *   action mask's place it makes the shield pick among the actions that keep the agent alive longest and, of
 *   those, collect the most reward.  The rules are csrc/step_plan.h's.
 * Each of depth, ret, path, ends, crash9 and plan_mask may be NULL; actions / mdr as in gw_step_horizon.
 * How it is computed: while k has not crashed the world differs between k's choices in two things only, k's cell
 * and whether k's apple is still there (motion and crashes do not depend on apples; the other agents' apples
 * belong to the level's one background; k's prev_dist is a function of its cell and its apple bit), so a node is
 * still a cell.  Every (node, allowed action) is one world update with k's apple present; the backward pass keeps
 * two values per node: the depth without k's apple (gw_step_horizon's recursion; the return from there is 0 if it
 * reaches H, else -100) and the best (depth, return) with it.
 * GW_ERR_ARG also on a ret array that is not 2-byte aligned.
 * Cost: two launches on `stream` (preview_rec_kernel, then step_plan_kernel: one wave per env, the RL agents in
 * turn), one GW_SPAN_STEP_PLAN span while profiling.  gw_count_sims counts as gw_step_horizon does: per env 9 K for
 * step 1 plus one world update per reached level, distinct cell k can stand in there (with or without its apple)
 * and action that cell's mask allows. */
gw_status gw_step_plan(void *env, const int32_t *rl_actions, const int32_t *scripted, const uint16_t *mask, int horizon,
                       uint8_t *depth, int16_t *ret, uint8_t *path, uint16_t *ends, uint16_t *crash9, uint16_t *plan_mask,
                       int32_t *actions, int32_t *mdr, void *stream);

/* The coordinated crash-aware shield: gw_step_preview's safe masks inside gw_fear_shield_joint's sweeps, in one call.
 * The crash-aware shield built from gw_step_preview and gw_fear_shield is unilateral: an agent moved to a safe action
 * is crash-free only where every other agent's action was kept, so two agents that were both moved can still meet.
 * Here every visit previews the agent's nine actions against the actions the agents before it have fixed.  Per env,
 * with `scripted` the scripted agents' actions and prop[k] the proposed RL actions (given, or NULL = drawn with the
 * step's own Philox counters; a proposal outside 0..8 is read as 0, as gw_step applies it):
 *   cur = prop
 *   O_prop = crash | restr << 8 of the real UpdateGWorld of the current world under (prop, scripted)
 *   for s in 1..sweeps:
 *     changed = false
 *     for k in 0..K-1 ascending, where bit k of `agents` is set:
 *       crash9 = { a : agent k ITSELF crashes in the real UpdateGWorld under (cur, scripted) with k playing a }
 *                (gw_step_preview's task: the full joint action, eaters 0..K-1, the apples still present)
 *       m'  = the safe mask of csrc/step_preview.h on (mask given, mask[k], crash9)
 *       t   = use_fear ? row k of gw_fear_preview's table for (cur, scripted) : nine zeros
 *       r   = the pick of csrc/fear_shield.h on (t, cur[k], m', probs of k, use_fear ? tau : 0.0)
 *       stuck[k]       = bit 1 of r's flags
 *       unavoidable[k] = the mask word of k (all nine if none) != 0 and (it & ~crash9) == 0
 *       if r.action != cur[k]: cur[k] = r.action, changed = true
 *     if not changed: break
 *   O = crash | restr << 8 of the real UpdateGWorld under (cur, scripted)
 *   T = gw_fear_preview's table for (cur, scripted)     (only if use_fear or fear_alt != NULL)
 * The visit (m', r, unavoidable) is csrc/crash_shield.h's.  use_fear == 0 is the crash shield alone: tau is ignored,
 * an agent that would crash is moved to its most probable action (no probs: the lowest) under which it does not,
 * and nothing else moves.
 * Outputs (any may be NULL except actions_out):
 *   actions_out [E][K] = cur (may alias rl_actions);  fear_alt [E][K][9] f64 = T;  joint [E][N] = the joint action
 *   the step will apply;  outcome [E] u16 = O;  outcome_prop [E] u16 = O_prop;  crash9 [E][K] u16 = the own-crash
 *   sets under the FINAL joint action, gw_step_preview's crash9 for (cur, scripted);  flags [E][K] u8:
 *     bits 0-3 as gw_fear_shield_joint's (replaced, stuck, over tau, unconverged); bit 2 is set only when use_fear;
 *     bit 4  bit k of O: agent k crashes in the step that applies actions_out;
 *     bit 5  unavoidable[k] of k's last visit (0 for an agent never visited).
 * It follows that
 *   - O[e] == crash_bits[e] | restr_bits[e] << 8 of the gw_step that applies actions_out with the same scripted
 *     actions;
 *   - with use_fear, T[e][k][actions_out[e][k]] is bit for bit that step's fear[e][k];
 *   - in an env with bit 3 clear every shielded agent with a non-zero mask and bit 5 clear has bit 4 clear (the
 *     unchanged sweep saw the final joint action, and every visit leaves the agent inside m');
 *   - where bit 2 is clear and use_fear, that step's fear[e][k] <= tau;
 *   - sweeps = 1, agents = 1 << k gives, for that k, the actions and flag bits 0-1 of the unilateral pipeline:
 *     gw_fear_preview, gw_step_preview's safe_mask, gw_fear_shield(agents = 1 << k) (use_fear == 0: on a zero table
 *     with tau = 0);
 *   - use_fear == 0 runs no FeAR world update at all unless fear_alt is given.
 * mask, probs, agents, sweeps as gw_fear_shield_joint's.  Its conventions too: works on cfg.fear == 0 envs; changes no
 * env state, step output, pipeline state or obs-destination table; shares the preview's record buffer (a first call
 * while `stream` captures returns GW_ERR_STATE, later calls can be captured); no host synchronisation; GW_ERR_STATE
 * before the first gw_reset; GW_ERR_ARG on a null env, null actions_out or sweeps out of range.
 * Cost: two launches on `stream` (preview_rec_kernel, then crash_shield_joint_kernel: one wave per env, every visit,
 * the final outcome and the table in it), one GW_SPAN_CRASH_SHIELD span while profiling.  The world updates the
 * kernel's schedule runs per env, all counted by gw_count_sims:
 *   - a visit of agent k: 9 real updates (one per action of k), and with use_fear the 9 (1 + 8 (c_k - 1)) FeAR
 *     updates of gw_fear_shield_joint's visit (close count c_k);
 *   - the proposal outcome: none of its own (with no visit it is the final outcome; else nothing has moved at the
 *     env's first visit, whose update under the agent's kept action is the proposal's);
 *   - the final outcome and crash9: 9 K real updates, always (the update of agent 0 under cur[0] is the final
 *     joint action's: O costs none of its own);
 *   - the final table, only if use_fear or fear_alt != NULL: the FeAR updates of all K agents; or, when use_fear
 *     and a sweep ran and the last one changed nothing, only those of the unshielded agents (the shielded agents'
 *     rows are then the visits').
 * Composed from gw_fear_preview, gw_step_preview and gw_fear_shield a visit costs three calls (six launches). */
gw_status gw_crash_shield_joint(void *env, const int32_t *rl_actions, const int32_t *scripted, const uint16_t *mask,
                                const float *probs, int32_t use_fear, double tau, uint32_t agents, int32_t sweeps,
                                int32_t *actions_out, uint8_t *flags, double *fear_alt, int32_t *joint,
                                uint16_t *outcome, uint16_t *outcome_prop, uint16_t *crash9, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GRIDENV_H */
