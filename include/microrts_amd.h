/*
 * microrts_amd.h -- C ABI of the MI355X-native vectorised MicroRTS engine
 * (libmicrorts_amd.so).
 *
 * This is the drop-in replacement for the FFI boundary the reference crosses
 * on every reset / step / get_action_mask: JPype -> Java
 * tests.JNIGridnetVecClient (constructed at
 * /root/reference/gym_microrts/envs/vec_env.py:259-271).  Plain pointers and
 * sizes only; no torch types.  Device buffers are allocated by the caller
 * (hipMalloc, or a torch tensor's data_ptr) and all work is enqueued on the
 * caller's hipStream_t, passed as `void *stream` (NULL = default stream).
 *
 * Ownership (reference: JNI path copies, shared-mem path aliases,
 * vec_env.py:1276-1283, 1331-1333): output buffers are written in place and
 * stay valid until the next call that writes them.
 *
 * Errors: every call returns MRTS_OK (0) or a negative MRTS_E* code, and
 * mrts_last_error() holds a message (the reference surfaces Java exceptions
 * through JPype; callers invoke e.printStackTrace(), ppo_gridnet.py:477-479).
 *
 * Threading: a handle is not thread-safe; one handle per device per process
 * (the reference runs one in-process JVM per process, vec_env.py:153-169).
 */
#ifndef MICRORTS_AMD_H
#define MICRORTS_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRTS_OK 0
#define MRTS_EINVAL (-1)
#define MRTS_EIO (-2)
#define MRTS_EHIP (-3)
#define MRTS_ENOTIMPL (-4)
#define MRTS_ESTATE (-5)

/* Opponent ids for bot envs; names as in gym_microrts/microrts_ai.py:13-61. */
#define MRTS_AI_PASSIVE 0
#define MRTS_AI_WORKER_RUSH 1
#define MRTS_AI_LIGHT_RUSH 2
#define MRTS_AI_RANDOM_BIASED 3
#define MRTS_AI_COAC 4
#define MRTS_AI_PO_WORKER_RUSH 5
#define MRTS_AI_PO_LIGHT_RUSH 6
#define MRTS_AI_PO_HEAVY_RUSH 7
#define MRTS_AI_PO_RANGED_RUSH 8
#define MRTS_AI_RANDOM 9 /* randomAI = ai.RandomBiasedSingleUnitAI (microrts_ai.py:7-10) */
#define MRTS_AI_COUNT 10

#define MRTS_OBS_INT32 0
#define MRTS_OBS_FLOAT32 1
#define MRTS_OBS_PACKED 2 /* one 32-bit one-hot word per cell: "Packed observations" below */

typedef struct mrts_vec mrts_vec;

/* Arguments of JNIGridnetVecClient(num_selfplay, num_bot, max_steps, rfs,
 * micrortsPath, mapPaths, ai2s, utt, partialObs) (vec_env.py:261-271).  The six
 * reward functions and the default UnitTypeTable are fixed (vec_env.py:172-195). */
typedef struct {
    int32_t num_selfplay_envs;   /* even; envs 2k/2k+1 are players 0/1 of game k */
    int32_t num_bot_envs;        /* envs num_selfplay + j play player 0 vs bot_ai[j] */
    int32_t max_steps;           /* JNIGridnetVecClient.maxSteps                     */
    int32_t partial_obs;         /* PartiallyObservableGameState (31 planes)         */
    int32_t num_maps;            /* map table: all maps share one height x width     */
    const char *const *map_paths;/* PhysicalGameState XML files (absolute paths)     */
    const int32_t *game_map;     /* [num_games] index into map_paths, NULL -> 0      */
    const int32_t *bot_ai;       /* [num_bot_envs] MRTS_AI_*, NULL -> passive        */
    int32_t obs_dtype;           /* MRTS_OBS_INT32 (reference dtype), FLOAT32 or
                                    PACKED (obs buffers are then [N][H][W] int32)    */
    const int32_t *bot_ai0;      /* [num_bot_envs] MRTS_AI_* of player 0 (bot vs bot,
                                    MicroRTSBotVecEnv / JNIBotClient, vec_env.py:1104-1236),
                                    -1 = the agent plays player 0; NULL = all agent */
    int32_t game_offset;         /* global index of game 0 when this handle is one shard
                                    of a larger batch (one process per GPU): keys the
                                    random bots' streams so shard r's games play exactly
                                    as games [game_offset, game_offset + num_games) of
                                    one unsharded run; 0 otherwise                    */
    int32_t map_capacity;        /* map template slots (>= num_maps; 0 -> num_maps):
                                    room for maps added later with mrts_add_map      */
} mrts_config;

typedef struct {
    int32_t height, width;
    int32_t num_envs, num_games;
    int32_t obs_planes;          /* 29, or 31 with partial obs                       */
    int32_t mask_channels;       /* 78 (getMasks' 79 minus the source channel)       */
    int32_t action_components;   /* 7                                                */
    size_t workspace_bytes;      /* device bytes mrts_bind_workspace needs           */
} mrts_info_t;

/* new JNIGridnetVecClient(...): parses the map XMLs, validates the config. */
int mrts_create(const mrts_config *cfg, mrts_vec **out);
int mrts_info(const mrts_vec *h, mrts_info_t *info);
/* Attach caller-owned device memory of mrts_info().workspace_bytes (game state
 * + map templates) and upload the maps on `stream`. */
int mrts_bind_workspace(mrts_vec *h, void *dev_workspace, void *stream);

/* JNIGridnetVecClient.reset(players) (vec_env.py:279): every game back to its
 * map; obs [N][H][W][planes] (int32 or float32 per obs_dtype). */
int mrts_reset(mrts_vec *h, void *stream, void *obs);

/* JNIGridnetVecClient.getMasks(0) (vec_env.py:1097): mask [N][H*W][78] int32
 * (channels 1..78) and source [N][H*W] int32 (channel 0). */
int mrts_get_masks(mrts_vec *h, void *stream, int32_t *mask, int32_t *source);

/* Bind device mask outputs (the zero-copy form of the reference's shared-memory
 * client, Client(..., obsBuf, maskBuf, actionBuf, 0), vec_env.py:1276-1283,
 * 1310-1324): from now on mrts_reset, mrts_step, mrts_step_weighted and
 * mrts_reset_games also write getMasks(0) of the state they leave behind --
 * the bytes a following mrts_get_masks would write -- into mask [N][H*W][78]
 * int32 and source [N][H*W] int32, in the same kernel pass.  `source` may be
 * the buffer mrts_step reads its rows from (each game reads its own rows
 * before it rewrites them).  NULL, NULL unbinds.  While bound, the mask buffer
 * is the engine's between steps; binding again (also the same pointers) tells
 * it that the buffer's contents are no longer its own (mrts_set_mask_delta). */
int mrts_bind_mask_outputs(mrts_vec *h, int32_t *mask, int32_t *source);

/* Bot fusion (default on).  A bot's getAction(1, gs) reads only the state
 * before the tick (JNIGridnetClient.gameStep: bot decisions, then issueSafe(p0),
 * issueSafe(p1), cycle).  With fusion, mrts_step's kernel decides the NEXT
 * tick's bot actions for every bot game in the same pass -- one wavefront of the
 * game's workgroup runs the bot on the state it has just stored while the other
 * wavefronts stream the observations and masks -- instead of a separate bot
 * kernel at the start of the next step; mrts_reset / mrts_reset_games decide
 * them for the games they reset.  Outputs are identical either way.  Applies
 * when no env has a bot as player 0 (MicroRTSBotVecEnv), the map has more than
 * 64 cells and its two LDS regions fit one workgroup (160 KB); on = 0 launches the bot kernel at every step. */
int mrts_set_bot_fusion(mrts_vec *h, int32_t on);

/* Delta masks (default on).  getMasks(0) sets no channel of a cell that holds no
 * idle unit of the player, so all but about 1 % of the bound mask rows are zero
 * and stay zero from tick to tick.  With delta masks, a step that follows a
 * launch which wrote every row of the bound buffers (mrts_reset, mrts_load_state,
 * a step, or mrts_get_masks into exactly the bound pointers) stores only the mask
 * rows that can differ from what the buffer holds: the source rows of the state
 * it loads (zeroed unless still source rows) and the source rows of the state it
 * leaves.  `source` is still written in full.  The bytes in the buffers are the
 * same either way, PROVIDED nobody else writes the mask buffer: while masks are
 * bound the engine owns that buffer between steps (callers read or copy it, as
 * the reference's rollout loop does).  A caller that wrote into it calls
 * mrts_bind_mask_outputs again (the same pointers will do) -- the next step then
 * writes every row -- or turns delta masks off.  on = 0: every step writes every
 * row. */
int mrts_set_mask_delta(mrts_vec *h, int32_t on);

/* Delta observations (default on; dense obs, int32 or float32).  A cell's obs row --
 * its P planes -- is a function of the cell's unit, its action and the terrain,
 * and all but about 2 % of the rows stay the same from tick to tick.  With delta observations, a step
 * whose `obs` is the buffer that the last launch which wrote every obs row wrote to
 * (mrts_reset, mrts_load_state, a step) stores only the rows whose content differs
 * from the one of the state it loads.  mrts_reset_games and mrts_park_games into
 * that buffer keep it current (they write their games' rows in full); given another
 * buffer they end it.  A step given any other pointer writes every row, and that
 * pointer is the current buffer from then on.  The bytes in the buffer are the same
 * either way, PROVIDED nobody else writes it: the engine owns the obs buffer between
 * steps (callers read or copy it, as the reference's rollout loop does).  A caller
 * that wrote into it calls mrts_invalidate_obs -- the next step then writes every
 * row -- or turns delta observations off.  on = 0: every step writes every row.
 * Packed obs (MRTS_OBS_PACKED) are always written in full, and so are the obs of
 * engines with partial observability (their rows also depend on the sight disks;
 * measured slower) and of maps of more than four cells per lane of the step
 * workgroup (more than 1024 cells). */
int mrts_set_obs_delta(mrts_vec *h, int32_t on);
/* The caller wrote into an obs buffer it gave to the engine: the next step writes
 * every row of its `obs`, whichever buffer that is. */
int mrts_invalidate_obs(mrts_vec *h);

/* step_async + JNIGridnetVecClient.gameStep (vec_env.py:968-984, 1002):
 * actions [N][H*W][7] int64 (device), source [N][H*W] int32 = the source
 * channel of the last mrts_get_masks (selects the rows, vec_env.py:974).
 * After mrts_set_action_format(h, MRTS_ACT_PACKED), `actions` is read as the packed
 * words [N][H*W] int32 instead ("Packed actions" below), here and in
 * mrts_step_weighted and mrts_step_group.
 * Outputs: obs, raw_reward [N][6] float64 (the six reward functions), done
 * [N][6] uint8.  Finished games auto-reset (terminal reward/done reported). */
int mrts_step(mrts_vec *h, void *stream, const int64_t *actions, const int32_t *source,
              void *obs, double *raw_reward, uint8_t *done);

/* Response.observation of the JNI client (vec_env.py:279-280, 1002-1003, 1035):
 * GameState.getVectorObservation per env, int32 [N][P_raw][H][W], P_raw = 6
 * (hp, resources, owner 1 = self / 2 = opponent, type id + 1, action type,
 * terrain) + 1 visibility plane with partial obs.  The unencoded form of the
 * obs mrts_reset / mrts_step write; for callers that keep the reference's own
 * python _encode_obs. */
int mrts_get_raw_obs(mrts_vec *h, void *stream, int32_t *raw);

/* reward_weight and reward_shaping of MicroRTSGridModeVecEnv (vec_env.py:102-103,
 * 1003-1004, 1057), used by mrts_step_weighted.  Host array of 6 doubles. */
int mrts_set_reward_weight(mrts_vec *h, const double *weight6, int32_t reward_shaping);

/* mrts_step + the step_wait reduction fused into the same kernel
 * (vec_env.py:1003-1004, 1057): reward [N] float64 = raw_reward @ weight
 * (k = 0..5 in order, round-to-nearest, no FMA; channels 1..5 taken as 0 when
 * reward_shaping is off) and done0 [N] uint8 = done[:, 0]. */
int mrts_step_weighted(mrts_vec *h, void *stream, const int64_t *actions, const int32_t *source, void *obs,
                       double *raw_reward, uint8_t *done, double *reward, uint8_t *done0);

/* One step of several engines -- the map-size buckets of one mixed batch --
 * equivalent to mrts_step (io[i].reward == NULL) or mrts_step_weighted on each
 * hs[i] in order on `stream`: mrts_step and mrts_step_weighted are this call
 * with n = 1 and MRTS_GROUP_BOTS_FIRST.  Replaces the sequence of
 * JNIGridnetVecClient.gameStep calls that one reference vec env per map size
 * makes (vec_env.py:148-150: one size per env; vec_env.py:986-1003: gameStep),
 * so that engines whose kernels share planes, obs dtype and bot fusion run in
 * one kernel launch instead of one each.  policy: MRTS_GROUP_SEPARATE (one
 * launch per engine), MRTS_GROUP_MERGE_FIT (merge members that still fit
 * >= 4 workgroups per CU at the launch's LDS size; larger maps keep their own
 * launch), MRTS_GROUP_MERGE_ALL (every compatible member), | MRTS_GROUP_BOTS_FIRST
 * (bot games start before selfplay games in the merged grid).  Outputs are the
 * same bytes whatever the policy.  1 <= n <= MRTS_STEP_GROUP_MAX, each handle once,
 * all on the device that runs `stream`.  Errors: the message is on the failing
 * member's handle and on hs[0].  Not atomic: when launch l fails with MRTS_EHIP the
 * members of earlier launches have stepped and the others have not. */
#define MRTS_STEP_GROUP_MAX 4
#define MRTS_GROUP_SEPARATE 0
#define MRTS_GROUP_MERGE_FIT 1
#define MRTS_GROUP_MERGE_ALL 2
#define MRTS_GROUP_BOTS_FIRST 4
typedef struct mrts_step_io {
    const int64_t *actions;
    const int32_t *source;
    void *obs;
    double *raw_reward;
    uint8_t *done;
    double *reward;   /* NULL: mrts_step's outputs only */
    uint8_t *done0;
} mrts_step_io;
int mrts_step_group(mrts_vec *const *hs, int32_t n, void *stream, const mrts_step_io *io, int32_t policy);

/* The launches mrts_step_group(hs, n, ..., policy) would make now: launch_of[i] =
 * the launch (0 ..) engine i runs in, *launches = their number.  No reference
 * counterpart (an engine-internal schedule, for profiling and tests). */
int mrts_step_group_plan(mrts_vec *const *hs, int32_t n, int32_t policy, int32_t *launch_of, int32_t *launches);

/* Map cycling (vec_env.py:1038-1056): reset `count` games (host arrays) onto
 * the given map indices and rewrite their envs' obs; parked games play again. */
int mrts_reset_games(mrts_vec *h, void *stream, const int32_t *games, const int32_t *maps, int32_t count, void *obs);

/* Park `count` games (host array): they stop ticking -- mrts_step, mrts_get_masks
 * and the bots skip them -- and their envs' obs (and bound mask / source) rows
 * are written as zeros now; reward / done rows are left to the caller.
 * mrts_reset_games restarts a parked game on a map (mrts_reset keeps it parked
 * and writes its zeros again).  Map cycling across map sizes
 * (MicroRTSSizeCyclingVecEnv): a game lives in one engine per size and plays in
 * one of them. */
int mrts_park_games(mrts_vec *h, void *stream, const int32_t *games, int32_t count, void *obs);

/* JNIGridnetVecClient.clients[i].mapPath = path / .selfPlayClients[j].mapPath =
 * path (vec_env.py:1044, 1051): the Java client re-reads the map file at its next
 * reset.  Here the map is loaded into a free template slot (config map_capacity)
 * and its index returned, for mrts_reset_games; a path already in the table
 * returns its existing index.  Same height x width as the handle's maps. */
int mrts_add_map(mrts_vec *h, void *stream, const char *path, int32_t *index);

/* Random masked action sampler of hello_world.py:27-64 on the device
 * (Philox4x32-10 keyed by seed, counter = (cell, env0 + env, step)): env0 is the
 * global index of row 0's env, so a shard draws the actions of its slice of
 * one larger batch.  Not a reference entry point: the bench's stand-in policy.
 * MRTS_EINVAL before any launch: a null pointer, hw < 1, num_envs < 0, env0 < 0,
 * num_envs * hw beyond 2^31 - 256, actions not 16-byte aligned (the rows are
 * written with 16-byte stores). */
int mrts_sample_actions(void *stream, const int32_t *mask, int32_t num_envs, int32_t hw, int32_t env0, uint64_t seed,
                        uint32_t step, int64_t *actions);

/* Same stream and output as mrts_sample_actions, given the source channel too:
 * mask rows of cells whose source is 0 are all zero (getMasks), so only the
 * rows of source cells are read.  Every row's 7 components are still written.
 * The same checks as mrts_sample_actions (num_envs * hw at most 2^31 - 257,
 * actions 16-byte aligned: MRTS_EINVAL otherwise). */
int mrts_sample_actions_src(void *stream, const int32_t *mask, const int32_t *source, int32_t num_envs, int32_t hw,
                            int32_t env0, uint64_t seed, uint32_t step, int64_t *actions);

/* mrts_sample_actions_src over up to MRTS_SAMPLE_GROUP_MAX batches at once (the map-size
 * buckets of one mixed batch) in ONE launch: segment k's actions are exactly those
 * mrts_sample_actions_src(stream, seg.mask, seg.source, seg.num_envs, seg.hw, seg.env0,
 * seed, step, seg.actions) writes.  Each segment: num_envs * hw below 2^31 - 256,
 * actions 16-byte aligned; MRTS_EINVAL otherwise.  The bench's stand-in policy. */
#define MRTS_SAMPLE_GROUP_MAX 4
typedef struct mrts_sample_seg {
    const int32_t *mask;     /* [num_envs][hw][78] */
    const int32_t *source;   /* [num_envs][hw] */
    int32_t num_envs, hw, env0;
    int64_t *actions;        /* [num_envs][hw][7] */
} mrts_sample_seg;
int mrts_sample_actions_src_group(void *stream, const mrts_sample_seg *segs, int32_t nseg, uint64_t seed, uint32_t step);

/* The masked action head of a GridNet policy on the device: CategoricalMasked per
 * action component and Agent.get_action_and_value's action is None branch
 * (/root/reference/experiments/ppo_gridnet.py:164-167, 225-232, 241-247).
 * logits [num_envs][hw][78] float32; mask / source as mrts_get_masks writes them
 * (only the mask and logit rows of source cells are read).  Writes actions
 * [num_envs][hw][7] int64 (what mrts_step takes; a non-source row gets the
 * no-valid-entry draw of mrts_sample_actions_src), and per env the summed log-prob
 * and entropy, logprob / entropy [num_envs] float32.  Per component with valid
 * entries: the float32 softmax over them, sampled by inverse CDF from the Philox
 * words of mrts_sample_actions_src (seed, counter = (cell, env0 + env, step):
 * exact under sharding); a component without valid entries contributes 0 to both
 * sums (the reference's float32 result for its -1e8 mask value).  Runs on `stream`,
 * allocates and synchronises nothing.  MRTS_EINVAL before any launch: a null
 * pointer, hw < 1, num_envs < 0, env0 < 0, num_envs * hw beyond 2^31 - 256. */
int mrts_policy_sample(void *stream, const float *logits, const int32_t *mask, const int32_t *source, int32_t num_envs,
                       int32_t hw, int32_t env0, uint64_t seed, uint32_t step, int64_t *actions, float *logprob, float *entropy);

/* Agent.get_action_and_value with given actions (ppo_gridnet.py:233-247, the PPO
 * update's call): logprob / entropy [num_envs] float32 of `actions` under the same
 * masked softmax.  An action the mask forbids, or one outside its component's range,
 * contributes exactly -1e8 (the reference's float32 value) and is never used as an
 * index.  The same checks and stream rules as mrts_policy_sample. */
int mrts_policy_evaluate(void *stream, const float *logits, const int32_t *mask, const int32_t *source, int32_t num_envs,
                         int32_t hw, const int64_t *actions, float *logprob, float *entropy);

/* What autograd derives for ppo_gridnet.py:241-247 (loss.backward() at :566): given
 * grad_logprob / grad_entropy [num_envs] float32, writes ALL of grad_logits
 * [num_envs][hw][78] float32 (no pre-zeroing): the softmax gradient on valid entries,
 * +0.0f on masked entries, components without valid entries and non-source rows. */
int mrts_policy_evaluate_backward(void *stream, const float *logits, const int32_t *mask, const int32_t *source, int32_t num_envs,
                                  int32_t hw, const int64_t *actions, const float *grad_logprob, const float *grad_entropy,
                                  float *grad_logits);

/* Packed masks: getMasks' 79-bit word per cell as it is, the form a rollout buffer
 * can afford to keep (12 bytes a row against the dense form's 316).
 *   packed [N][H*W][3] int32, holding uint32 bit patterns;
 *   word j, bit b of row (env, cell) is bit 32 j + b of the 79-bit word;
 *   bit 0 is the source channel, bit ch + 1 is mask channel ch;
 *   bits 79..95 are zero in everything this library writes, and every reader
 *   ignores them;
 *   a row is 12 bytes, so packed buffers need 4-byte alignment only.
 * The handle-free calls below take num_envs * hw up to 2^31 - 257 rows, as the
 * samplers do, and return MRTS_EINVAL before any launch for a null pointer, hw < 1,
 * num_envs < 0 or more rows; they run on `stream`, allocate and synchronise nothing.
 *
 * mrts_get_masks_packed: getMasks(0) of the current state as packed words -- the
 * bits mrts_get_masks writes, the source channel included; parked games' rows are
 * zero.  A launch of its own that reads the games only: the bound dense mask
 * outputs, and what delta masks know about them, stay as they are.  MRTS_EINVAL for
 * a null handle or output, MRTS_ESTATE while no workspace is bound. */
int mrts_get_masks_packed(mrts_vec *h, void *stream, int32_t *packed);

/* Dense -> packed: channel bit = (mask != 0), source bit = (source != 0).  Every row is
 * read and kept, a non-source row's stray bits too: the conversion is lossless. */
int mrts_pack_masks(void *stream, const int32_t *mask, const int32_t *source, int32_t num_envs, int32_t hw, int32_t *packed);

/* Packed -> dense: writes every element of mask [num_envs][hw][78] and source
 * [num_envs][hw] as 0 or 1 (16-byte stores when `mask` is 16-byte aligned). */
int mrts_unpack_masks(void *stream, const int32_t *packed, int32_t num_envs, int32_t hw, int32_t *mask, int32_t *source);

/* mrts_policy_sample, mrts_policy_evaluate and mrts_policy_evaluate_backward over
 * packed masks: `packed` [num_envs][hw][3] stands for `mask, source`, and everything
 * else -- contract, checks, stream rules -- is the dense call's, word for word.  The
 * outputs are the dense calls' bit for bit: the arithmetic is the same code, only the
 * way a row's 78 bits reach it differs. */
int mrts_policy_sample_packed(void *stream, const float *logits, const int32_t *packed, int32_t num_envs, int32_t hw, int32_t env0,
                              uint64_t seed, uint32_t step, int64_t *actions, float *logprob, float *entropy);
int mrts_policy_evaluate_packed(void *stream, const float *logits, const int32_t *packed, int32_t num_envs, int32_t hw,
                                const int64_t *actions, float *logprob, float *entropy);
int mrts_policy_evaluate_backward_packed(void *stream, const float *logits, const int32_t *packed, int32_t num_envs, int32_t hw,
                                         const int64_t *actions, const float *grad_logprob, const float *grad_entropy,
                                         float *grad_logits);

/* Packed actions: an action row's seven components in one 32-bit word per cell, the form a
 * rollout buffer can afford to keep (4 bytes a cell against the int64 row's 56).
 *   action_words [N][H*W] int32, holding uint32 bit patterns;
 *   bits 0..2 action type, 3..4 move direction, 5..6 harvest direction, 7..8 return direction,
 *   9..10 produce direction, 11..13 produce type, 14..19 attack cell: component k in the
 *   fewest bits that hold its entries, laid end to end;
 *   bit 20 + k, k = 0..6, is the INVALID flag of component k;
 *   bits 27..31 are zero in everything this library writes, and every reader ignores them.
 * Meaning: a word stands for the dense row whose component k is -1 when flag k is set and
 * the field's value otherwise (so a type field of 6 or 7, a produce type of 7 and an attack
 * cell of 49..63 are out of range exactly as the same int64 values are), and every reader
 * -- the step's decode, the action head's evaluate -- treats a word exactly as the dense
 * reader treats that row.  Packing an int64 row puts component k into its field when it lies
 * in [0, 2^bits_k); otherwise the field is 0 and flag k is set.  Hence unpack(pack(a)) == a
 * for every row whose components fit their fields (all that the samplers and the action
 * head ever write), and step / evaluate of pack(a) equal those of a for ANY int64 row: a
 * component that does not fit its field is out of range in the dense form as well.
 *
 * mrts_set_action_format: what the `actions` pointer of mrts_step, mrts_step_weighted and
 * this engine's member of mrts_step_group holds from now on -- MRTS_ACT_DENSE (default):
 * [N][H*W][7] int64; MRTS_ACT_PACKED: the words, [N][H*W] int32 behind the same pointer
 * type, 4-byte aligned (MRTS_EINVAL otherwise).  A per-engine setting like
 * mrts_set_mask_delta: one grouped launch may hold engines of either kind.  It changes no
 * game state and is not part of a snapshot's fingerprint: a state saved by an engine of
 * one format loads into an engine of the other.  MRTS_EINVAL for a null handle or any
 * other format value. */
#define MRTS_ACT_DENSE 0
#define MRTS_ACT_PACKED 1
int mrts_set_action_format(mrts_vec *h, int32_t format);

/* mrts_sample_actions_src's stream and picks, stored as packed action words [num_envs][hw]
 * int32: exactly pack of the rows mrts_sample_actions_src writes.  The same checks, `words`
 * 4-byte aligned.  (The dense mrts_sample_actions and the grouped sampler have no packed twin.) */
int mrts_sample_actions_src_packed(void *stream, const int32_t *mask, const int32_t *source, int32_t num_envs, int32_t hw,
                                   int32_t env0, uint64_t seed, uint32_t step, int32_t *words);

/* The converters between int64 rows [rows][7] and words [rows], by the rules above (unpack
 * writes every element).  rows up to 2^31 - 257; MRTS_EINVAL before any launch for a null
 * pointer, rows out of range, `actions` not 8-byte or `words` not 4-byte aligned; rows == 0
 * is MRTS_OK and launches nothing.  16-byte accesses on the int64 side when it is 16-byte
 * aligned.  They run on `stream`, allocate and synchronise nothing. */
int mrts_pack_actions(void *stream, const int64_t *actions, int64_t rows, int32_t *words);
int mrts_unpack_actions(void *stream, const int32_t *words, int64_t rows, int64_t *actions);

/* The action head with both formats as arguments: mask_format MRTS_MASK_DENSE (`mask`
 * [num_envs][hw][78] with `source`) or MRTS_MASK_PACKED (`mask` is the packed words
 * [num_envs][hw][3], `source` is not read and may be NULL); action_format MRTS_ACT_DENSE
 * (`actions` [num_envs][hw][7] int64, 8-byte aligned) or MRTS_ACT_PACKED (the words
 * [num_envs][hw] int32, 4-byte aligned).  Everything else is mrts_policy_sample's,
 * mrts_policy_evaluate's and mrts_policy_evaluate_backward's contract word for word, and the
 * results are theirs bit for bit: sample's words are pack of the dense call's actions, and
 * evaluate reads a word as the row it stands for (a flagged component is an action outside
 * its range: exactly -1e8).  MRTS_EINVAL also for any other format value. */
#define MRTS_MASK_DENSE 0
#define MRTS_MASK_PACKED 1
int mrts_policy_sample_fmt(void *stream, const float *logits, int32_t mask_format, const int32_t *mask, const int32_t *source,
                           int32_t num_envs, int32_t hw, int32_t env0, uint64_t seed, uint32_t step, int32_t action_format,
                           void *actions, float *logprob, float *entropy);
int mrts_policy_evaluate_fmt(void *stream, const float *logits, int32_t mask_format, const int32_t *mask, const int32_t *source,
                             int32_t num_envs, int32_t hw, int32_t action_format, const void *actions, float *logprob, float *entropy);
int mrts_policy_evaluate_backward_fmt(void *stream, const float *logits, int32_t mask_format, const int32_t *mask, const int32_t *source,
                                      int32_t num_envs, int32_t hw, int32_t action_format, const void *actions,
                                      const float *grad_logprob, const float *grad_entropy, float *grad_logits);

/* Packed observations: the one-hot obs as the 32-bit word per cell the engine builds
 * it from, the form a rollout buffer can afford to keep (4 bytes a cell against the
 * dense form's 116 or 124).
 *   packed_obs [N][H][W] int32, holding uint32 bit patterns;
 *   bit i of a cell's word is plane i of the dense obs of that env and cell, i < P
 *   (P = mrts_info().obs_planes: 29, or 31 with partial obs);
 *   bits P..31 are zero in everything this library writes, and every reader ignores
 *   them;
 *   a parked game's envs read the zero word, which unpacks to their all-zero dense obs.
 * An engine created with obs_dtype = MRTS_OBS_PACKED writes these words wherever a
 * dense engine writes obs -- mrts_reset, mrts_step, mrts_step_weighted, mrts_step_group,
 * mrts_reset_games, mrts_park_games, mrts_load_state -- into `obs` [N][H][W] int32
 * (16-byte stores when H * W is a multiple of 4 and `obs` is 16-byte aligned).
 * mrts_step_group and mrts_step_group_plan refuse a group of packed and dense engines
 * (MRTS_EINVAL, nothing stepped), and a state saved by a packed engine loads only into a
 * packed one (the configuration fingerprint).
 *
 * The handle-free converters below take rows = N * H * W of any batch (up to 2^31 - 257, as the
 * samplers do) and
 * planes 29 or 31; the dense elements are one of MRTS_ELEM_*.  MRTS_EINVAL before any
 * launch for a null pointer, rows out of range, any other planes or elem, or an `obs`
 * pointer not aligned to its element size; rows == 0 is MRTS_OK and launches nothing.
 * They run on `stream`, allocate and synchronise nothing. */
#define MRTS_ELEM_INT32 0
#define MRTS_ELEM_FLOAT32 1
#define MRTS_ELEM_FLOAT16 2
#define MRTS_ELEM_BFLOAT16 3
/* packed [rows] -> dense [rows][planes] of 0 / 1 in `elem`; bits >= planes ignored.  Every
 * element is written: a one as 1, 0x3f800000, 0x3c00 or 0x3f80, a zero as all-zero bits, so
 * int32 and float32 results are an int32 / float32 engine's own obs bit for bit.  16-byte
 * stores when `obs` is 16-byte aligned. */
int mrts_unpack_obs(void *stream, const int32_t *packed, int64_t rows, int32_t planes, int32_t elem, void *obs);
/* dense [rows][planes] -> packed [rows]: a bit is set where the element is non-zero (-0.0 is zero) */
int mrts_pack_obs(void *stream, const void *obs, int64_t rows, int32_t planes, int32_t elem, int32_t *packed);

/* The first encoder stage of a GridNet policy on the packed words, with no dense obs in between:
 * Conv2d(planes, channels, 3, padding = 1) -> MaxPool2d(3, 2, 1) -> ReLU.
 *   packed [n][height][width] int32 (bits >= planes ignored), weight [channels][planes][3][3]
 *   float32 (nn.Conv2d.weight's layout), bias [channels] float32;
 *   out [n][channels][Ho][Wo] float32, Ho = (height - 1) / 2 + 1, Wo = (width - 1) / 2 + 1.
 * Defined for arbitrary words.  conv(n, c, y, x) starts from bias[c] and visits the taps (ky, kx),
 * 0..2 each in row-major order, neighbour (y + ky - 1, x + kx - 1): a neighbour outside the map or
 * with a zero word (a parked game's) is skipped; otherwise t = the sum of weight[c][p][ky][kx]
 * over the word's set bits p in ascending order, starting from the first one's weight, and then
 * acc = acc + t.  Every + is one float32 round-to-nearest add, none reassociated.  A pooled
 * output is the first maximum (strict >) of conv over rows 2 i - 1 .. 2 i + 1 and columns
 * 2 j - 1 .. 2 j + 1 in row-major order, positions outside the map left out; out is that
 * maximum m when m > 0, else +0.0.  NaN or infinite weights are outside the contract.
 * The backward overwrites grad_weight [channels][planes][3][3] and grad_bias [channels]
 * from grad_out [n][channels][Ho][Wo]: for every output with m > 0, whose first maximum is at
 * (y, x), g = grad_out's element is added to grad_bias[c] and to grad_weight[c][p][ky][kx] for
 * every tap whose neighbour is inside the map and has bit p set.  It recomputes the forward from
 * the words, sums in a fixed order (no float atomics: the same inputs give the same bits), and
 * needs a `workspace` of at least the queried size, 16-byte aligned, whose contents it
 * overwrites.  The query returns that size in bytes (0 for n == 0), or MRTS_EINVAL.
 * MRTS_EINVAL before any launch for a null pointer, planes other than 29 or 31, channels outside
 * 1..64, height or width below 1, a map of more than 4096 cells, n < 0 or n * height * width
 * above 2^31 - 257, or a workspace smaller than the query's; n == 0 is MRTS_OK and launches
 * nothing (the gradients are then left as they are).  They run on `stream`, allocate and synchronise nothing. */
int64_t mrts_obs_conv_workspace_bytes(int32_t n, int32_t height, int32_t width, int32_t planes, int32_t channels);
int mrts_obs_conv_forward(void *stream, const int32_t *packed, int32_t n, int32_t height, int32_t width, int32_t planes,
                          const float *weight, const float *bias, int32_t channels, float *out);
int mrts_obs_conv_backward(void *stream, const int32_t *packed, int32_t n, int32_t height, int32_t width, int32_t planes,
                           const float *weight, const float *bias, int32_t channels, const float *grad_out,
                           void *workspace, int64_t workspace_bytes, float *grad_weight, float *grad_bias);

/* Episode statistics on the device, for callers of mrts_step_weighted who keep every buffer in
 * HBM: what the reference gets from VecMonitor (ppo_gridnet.py:384-385, read at :487-488: the
 * episode return and length) and MicroRTSStatsRecorder (ppo_gridnet.py:126-160, read at :489-490,
 * ppo_gridnet_eval.py:200-203, league.py:278: the per-reward-function episode sums).  Stateless
 * like the converters: the running state and the finished episodes' records live in one
 * caller-owned device buffer `state` of the queried size, 16-byte aligned:
 *   bytes 0..15   int64 cnt[2]: records written since init, double-buffered by the call's serial
 *                 number -- after the calls step = s0 .. s the count is cnt[(s + 1) & 1]; 16..31 zero
 *   then, N = num_envs elements each: ret float32[N], len int32[N], factor float64[N],
 *   rawsum float64[6][N], disc float64[7][N]   (component-major)
 *   then, from the next multiple of 16: the ring, float64 [capacity][MRTS_EPISODE_RECORD_DOUBLES]:
 *   env, step, ret, len, rawsum[0..5], disc[0..6], 0.
 * init: cnt = 0, every ret / len / rawsum / disc = 0, every factor = 1, the ring zero.
 * update, once per env-step with that step's outputs reward [N] float64, done0 [N] bytes
 * (non-zero = the episode ended), raw [N][6] float64, and `step`, the call's serial number
 * (>= 0, one more than the call before; the first call's is the caller's choice).  Every operation
 * is one IEEE round-to-nearest operation of the stated type, none fused; per env, in this order:
 *   ret = (float)((double)ret + reward)                    numpy's float32 += float64
 *   len = len + 1
 *   rawsum[k] = rawsum[k] + raw[k], k = 0..5
 *   tot = ((((raw[0] + raw[1]) + raw[2]) + raw[3]) + raw[4]) + raw[5]
 *   disc[k] = disc[k] + factor * raw[k], k = 0..5;  disc[6] = disc[6] + factor * tot
 *   factor = factor * gamma
 *   if done0: append the record (env, step, (double)ret, len, rawsum, disc), then ret = len = 0,
 *   rawsum = disc = 0, factor = 1.
 * Record k since init goes to ring row k % capacity, and k follows the reference's scan of its
 * infos: ascending env within a call, call order across calls -- decided by counting, not by
 * atomics, so equal inputs give equal bytes.  A call that ends more than `capacity` episodes
 * writes the last `capacity` of them.  Nothing runs on the host and nothing is copied.
 * MRTS_EINVAL before any launch (the query returns it too): num_envs < 1, capacity < 1, step < 0,
 * a null pointer, `state` not 16-byte aligned, reward / raw not 8-byte aligned.  They run on
 * `stream`, allocate and synchronise nothing. */
#define MRTS_EPISODE_RECORD_DOUBLES 18
int64_t mrts_episode_stats_bytes(int32_t num_envs, int32_t capacity);
int mrts_episode_stats_init(void *stream, void *state, int32_t num_envs, int32_t capacity);
int mrts_episode_stats_update(void *stream, void *state, int32_t num_envs, int32_t capacity, double gamma, int64_t step,
                              const double *reward, const uint8_t *done0, const double *raw);

/* Advantages and returns of a rollout buffer in one launch (ppo_gridnet.py:496-519's loop over
 * num_steps): rewards, values [T][N] float32, dones [T][N] and last_done [N] of done_elem
 * (MRTS_DONE_FLOAT32: float32, what the reference stores; MRTS_DONE_UINT8: bytes, read as
 * (float)byte), last_value [N] float32 -> advantages, returns [T][N] float32.  With
 * g = (float)gamma, gl = (float)(gamma * lambda) (the product in double), every operation one
 * float32 round-to-nearest operation, none fused, t = T - 1 .. 0, d_next / v_next = dones[t + 1] /
 * values[t + 1], or last_done / last_value at t = T - 1, nnt = 1 - d_next:
 *   MRTS_GAE_ADVANTAGES (:497-508):  delta = (r + (g * v_next) * nnt) - v,
 *                                    A_t = delta + (gl * nnt) * A_{t+1}, A_T = 0;  returns_t = A_t + v
 *   MRTS_GAE_RETURNS (:510-519):     R_t = r + (g * nnt) * R_{t+1}, R_T = last_value;  A_t = R_t - v.
 * MRTS_EINVAL before any launch: T < 1, N < 1, a null pointer, another done_elem or mode, a pointer
 * not aligned to its element.  Runs on `stream`, allocates and synchronises nothing. */
#define MRTS_DONE_FLOAT32 0
#define MRTS_DONE_UINT8 1
#define MRTS_GAE_ADVANTAGES 0
#define MRTS_GAE_RETURNS 1
int mrts_gae(void *stream, int32_t T, int32_t N, const float *rewards, const float *values, const void *dones, int32_t done_elem,
             const float *last_value, const void *last_done, double gamma, double lambda, int32_t mode, float *advantages,
             float *returns);

/* Per-game rollout statistics, host int32 out[num_games][MRTS_GAME_STATS]:
 * game time (ticks since the game's last reset; the reference's gs.getTime()),
 * env steps of the episode, steps since creation, and three never-reset
 * counters -- ticks whose ready actions executed in order on one lane (attacks
 * or a shared resource pile), action rows issued on the ordered one-lane path,
 * auto-resets.  Synchronises the stream.  Introspection only (bench.py reports
 * the episode phases and serial work its timed window covered). */
#define MRTS_GAME_STATS 6
int mrts_game_stats(mrts_vec *h, void *stream, int32_t *out);

/* render("rgb_array") (vec_env.py:1075-1084): the game of `env` drawn into a
 * device frame rgb [size][size][3] uint8 (RGB; the reference returns 640 x 640).
 * Drawing rules: DESIGN.md §4c (the Java panel is absent; parity unpinned). */
int mrts_render(mrts_vec *h, void *stream, int32_t env, uint8_t *rgb, int32_t size);

/* Env-state checkpoint (no reference counterpart; SURVEY.md §5 "env-state
 * checkpoint"): the games' whole state -- cells, scalars, map templates, the
 * device bots' abstract actions and PlayerActions, parked flags, and the host-side
 * mirrors -- copied into / out of a caller device buffer of mrts_state_bytes(h)
 * bytes (256-byte aligned).  mrts_save_state synchronises the stream.
 * mrts_load_state restores a snapshot of the same configuration and map table
 * into this handle -- same env split, obs layout, game offset, max_steps, bots (both
 * players) and map templates, checked by a fingerprint in the snapshot's header; MRTS_EINVAL
 * otherwise, before anything but the fixed header is read -- and writes the restored state's obs
 * into `obs` (and its next-tick masks into the bound mask outputs), as mrts_reset
 * does for a fresh state; stepping on from it repeats the saved run bit for bit.
 * The reward weights and shaping flag (mrts_set_reward_weight) are host settings the
 * caller may change between steps: they are not in the snapshot and not checked. */
size_t mrts_state_bytes(const mrts_vec *h);
int mrts_save_state(mrts_vec *h, void *stream, void *dst);
int mrts_load_state(mrts_vec *h, void *stream, const void *src, void *obs);

/* Engine invariant violations recorded on the device (OR over games). */
int mrts_error_flags(mrts_vec *h, void *stream, int32_t *flags_out);

/* Diagnostics of the bot-fused step kernel for a map size (no device work, no
 * handle): 1 = the bot may start beside the output words' build (its LDS writes
 * and that phase's reads / writes are disjoint, checked from both carves),
 * 0 = fusable but the bot waits for that phase, -1 = no bot fusion for this
 * size (fused LDS over 160 KB, or a bot LDS over the 64 KB mrts_create allows).  No reference counterpart (an engine-internal schedule). */
int mrts_fused_layout_ok(int32_t width, int32_t height);

/* UnitTypeTable JSON as rts.units.UnitTypeTable.toJSON / sendUTT()
 * (vec_env.py:276).  Valid for the lifetime of the handle. */
const char *mrts_utt_json(const mrts_vec *h);

const char *mrts_last_error(const mrts_vec *h);
void mrts_destroy(mrts_vec *h);
const char *mrts_version(void);

#ifdef __cplusplus
}
#endif
#endif
