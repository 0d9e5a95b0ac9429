// mrts_engine.h -- internal launch interface between the C ABI (mrts_capi.cpp)
// and the kernels: the game step, output streams and renderer (mrts_engine.hip),
// the scripted opponents (mrts_bots.hip), the stand-in samplers (mrts_sampler.hip),
// the masked action head (mrts_policy.hip), the obs converters (mrts_obs.hip) and
// the first encoder stage on the packed obs (mrts_conv.hip).
#ifndef MRTS_ENGINE_H
#define MRTS_ENGINE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "microrts_amd.h"   // mrts_sample_seg, MRTS_* limits

// four int32 as one 16-byte value: the operand of the kernels' 16-byte and non-temporal loads / stores
namespace mrts { typedef int v4i __attribute__((ext_vector_type(4))); }

// Phase stamps (tracing, experiment builds only: `make STAMPS=1`): each step
// workgroup takes a row of g_stamp and writes wall_clock64() (100 MHz) at its
// phase boundaries; mrts_debug_stamps (mrts_engine.hip) reads the rows back.
// Compiled out of the product library.
#ifdef MRTS_STAMPS
#define MRTS_STAMP_ROWS 65536
#define MRTS_STAMP_COLS 20   // 2..15 phase stamps, 16..19 bot counters (MRTS_STAMP_ADD)
static __device__ unsigned long long g_stamp[MRTS_STAMP_ROWS][MRTS_STAMP_COLS];
__shared__ int mrts_stamp_row;
// mrts_stamp_row: set by k_step's thread 0 before a barrier; every other kernel
// that reaches a stamp site (k_reset / k_masks through emit_outputs) sets it to -1
// first (MRTS_STAMP_NONE), and the unsigned bound check skips it
#define MRTS_STAMP(k, cond) \
    do { if ((cond) && (unsigned)mrts_stamp_row < (unsigned)MRTS_STAMP_ROWS) g_stamp[mrts_stamp_row][k] = wall_clock64(); } while (0)
#define MRTS_STAMP_MAX(k, cond) \
    do { if ((cond) && (unsigned)mrts_stamp_row < (unsigned)MRTS_STAMP_ROWS) \
             atomicMax(&g_stamp[mrts_stamp_row][k], (unsigned long long)wall_clock64()); } while (0)
#define MRTS_STAMP_NONE() do { if (threadIdx.x == 0) mrts_stamp_row = -1; __syncthreads(); } while (0)
// a counter of the row (one writer: the bot wave's lane 0)
#define MRTS_STAMP_ADD(k, v, cond) \
    do { if ((cond) && (unsigned)mrts_stamp_row < (unsigned)MRTS_STAMP_ROWS) g_stamp[mrts_stamp_row][k] += (v); } while (0)
#else
#define MRTS_STAMP(k, cond) do { } while (0)
#define MRTS_STAMP_MAX(k, cond) do { } while (0)
#define MRTS_STAMP_NONE() do { } while (0)
#define MRTS_STAMP_ADD(k, v, cond) do { } while (0)
#endif

// One workgroup's LDS: an unfused step or a k_bot workgroup stays within the 64 KB a HIP kernel gets
// without asking; the bot-fused step may take a CU's whole 160 KB.
#define MRTS_LDS_CAP 65536
#define MRTS_LDS_CAP_FUSED 163840

namespace mrts {
// LDS carving (all dynamic, 16-byte aligned pieces: cdna_hip_programming §6 G17).  A layout is ONE carve
// function that takes its arrays from a Carver in order: the pointers are the kernels', the end offset is
// the layout's size, and a SpanLog (host-side checks) receives each array's extent as it is taken.
__host__ __device__ inline size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }
// a wave-uniform offset as one scalar the compiler keeps rather than recomputes (the host: the value itself)
__host__ __device__ inline size_t lds_uniform(size_t o) {
#ifdef __HIP_DEVICE_COMPILE__
    return (size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)o);
#else
    return o;
#endif
}
struct Span {
    const unsigned char* p;
    size_t n;   // the bytes asked for (the slot is a16(n))
};
struct SpanLog {
    enum { MAX = 48 };
    Span s[MAX];
    int n = 0;
    __host__ __device__ Span of(const void* p) const {   // the array that starts at p; {null, 0}: not logged
        for (int i = 0; i < n; i++) if (s[i].p == p) return s[i];
        return Span{nullptr, 0};
    }
};
struct Carver {
    unsigned char* base;
    size_t o = 0;
    SpanLog* log = nullptr;
    template <typename T>
    __host__ __device__ T* take(size_t count) {
        unsigned char* p = base + o;
        if (log && log->n < SpanLog::MAX) log->s[log->n++] = Span{p, count * sizeof(T)};
        o += a16(count * (size_t)sizeof(T));
        return reinterpret_cast<T*>(p);
    }
};
// sizes are offsets: a carve runs on any base
__host__ __device__ inline unsigned char* lds_any_base() { return reinterpret_cast<unsigned char*>((size_t)1 << 20); }

// A move / produce targets position x + y * W + W, unchecked: 0 .. HW + 2 W - 1, one bit each.
// The three word counts differ by up to one word:
__host__ __device__ inline int pos_words_live(int HW, int W) { return (HW + 2 * W + 31) / 32; }   // words that hold a position
__host__ __device__ inline int pos_words(int HW, int W) { return (HW + 2 * W) / 32 + 1; }   // claim, bot pend / pab: + 1 when whole
__host__ __device__ inline int posbits_words(int HW, int W) { return pos_words_live(HW, W) + 1; }   // Lds::posbits: a spare word
__host__ __device__ inline int vis_words(int HW) { return HW / 32 + 1; }   // one player's visibility bits
}  // namespace mrts

// delta obs (EngineParams::obs_delta): a lane keeps a key of each of its cells in the loaded state in
// registers through the tick (mrts_engine.hip obs_key), for at most this many cells per lane: every
// prefetched size
#define MRTS_OBS_DELTA_CELLS 4
// delta masks (EngineParams::mask_delta): a lane keeps two bits per cell (which views held a source row there in
// the loaded state) in one register through the tick (mrts_engine.hip LaneRec::was_src), for at most this many
// cells per lane
#define MRTS_MASK_DELTA_CELLS 16
struct EngineParams {
    int4 *cells;            // [G][cstride] (the first HW records of each game's row)
    int cstride;            // int4 records between consecutive games' cells (>= HW)
    int32_t *genv;          // [G][MRTS_GENV_WORDS]
    const int4 *map_cells;  // [maps][HW]
    const uint8_t *map_wall;// [maps][HW]
    const int32_t *map_scal;// [maps][MRTS_MAP_SCALARS]
    int G, HW, W, H;
    int nmaps;              // map templates (1: every game's terrain is map 0's)
    int nsp, nsp_games, max_steps;
    int obs_kind;           // MRTS_OBS_*: what `obs` holds (the kernels' OT: int32_t, float, or mrts::PackedObs)
    int partial_obs;
    const int64_t *actions; // [N][HW][7], or the packed words [N][HW] int32 (act_packed)
    int act_packed;         // MRTS_ACT_PACKED: `actions` holds one 32-bit word per row (mrts_actions.h); a
                            // per-engine setting (mrts_set_action_format), so one grouped launch may hold both
    const int32_t *src;     // [N][HW]
    void *obs;              // [N][HW][P], or the packed words [N][HW] (MRTS_OBS_PACKED)
    double *raw_reward;     // [N][6]
    uint8_t *done;          // [N][6]
    int32_t *mask;          // [N][HW][78]: k_masks output; k_step / k_reset write the
    int32_t *src_out;       // [N][HW]      next tick's masks here when non-null
    int mask_delta;         // k_step: `mask` holds getMasks(0) of the state the step loads (mrts_capi.cpp keeps
                            // track), so only the rows that can differ are stored: the source rows of the loaded
                            // and of the final state (mrts_set_mask_delta); src_out is written in full either way
    int obs_delta;          // k_step, dense obs: `obs` holds the one-hot rows of the state the step loads (mrts_capi.cpp
                            // keeps track: obs_synced_ptr), so only the rows of cells whose content changed are stored
                            // (mrts_set_obs_delta); at most MRTS_OBS_DELTA_CELLS cells per lane
    // optional fused step_wait outputs (vec_env.py:1057): reward = raw @ rw
    // (float64, k = 0..5 in order; channels 1..5 zeroed when !shaping) and done[:,0]
    double *reward;         // [N] or null
    uint8_t *done0;         // [N] or null (torch.bool storage)
    double rw[6];
    int shaping;
    // device bots (mrts_bots.hip): bot game b = game nsp_games + b
    const int32_t *bot_ai;  // [Gb] MRTS_AI_* of player 1
    const int32_t *bot_ai0; // [Gb] MRTS_AI_* of player 0 in bot-vs-bot games, -1 = the agent
    int4 *aa;               // [Gb][2][HW][2] AbstractionLayerAI.actions per bot player
    int32_t *botpa;         // [Gb][2][HW] bot PlayerActions, cell | code << 16; null = none
    int nbot_active;        // bot players (either side) whose AI is not passiveAI
    const int32_t *bot_games; // k_bot: decide only for these games (device list), null = every bot game
    int bot_ngames;
    int fuse_bots;          // k_step: wave 0 of each bot game's workgroup decides the next tick's bot actions
    int game_offset;        // global index of game 0 (a shard of a larger batch): keys the bots' RNG
    int early_bot;          // fused k_step: the bot may start beside phase A; set by the step launch for its
                            // workgroup size (mrts_engine_step_layout's `early`), not by the engine's owner
    const uint8_t *parked;  // [G] 1 = parked (mrts_park_games): no tick, no masks / bots, zero outputs at
                            // reset; null while no game was ever parked
};
__device__ __forceinline__ bool game_parked(const EngineParams &p, int g) { return p.parked && p.parked[g]; }

// The step kernel's argument: the engines of one launch and the grid's segments
// (workgroups seg_block[k] .. seg_block[k + 1] - 1 run games seg_game[k].. of
// engine e[seg_member[k]]).
#define MRTS_STEP_GROUP_MAX 4
struct StepGroup {
    EngineParams e[MRTS_STEP_GROUP_MAX];
    int seg_block[2 * MRTS_STEP_GROUP_MAX + 1];
    int seg_member[2 * MRTS_STEP_GROUP_MAX];
    int seg_game[2 * MRTS_STEP_GROUP_MAX];
    int nseg;
};

extern "C" {
hipError_t mrts_engine_reset(const EngineParams *p, hipStream_t s, const int32_t *games, const int32_t *maps, int count);
hipError_t mrts_engine_masks(const EngineParams *p, hipStream_t s);
hipError_t mrts_engine_outputs(const EngineParams *p, hipStream_t s);
hipError_t mrts_engine_step_group(const EngineParams *ps, int n, hipStream_t s, int bots_first);
// The step workgroup of a map size: NT lanes (NT = 0 in: the size's own, else a launch's), its dynamic LDS
// (the end of the step carve, or of the fused carve) and whether the fused bot starts beside phase A.
struct mrts_step_layout_t {
    int NT, early;
    size_t lds_bytes;
};
mrts_step_layout_t mrts_engine_step_layout(int HW, int W, int fused, int partial, int NT);
hipError_t mrts_engine_bots(const EngineParams *p, hipStream_t s);
hipError_t mrts_engine_raw_obs(const EngineParams *p, hipStream_t s, int32_t *raw);
// mrts_sampler.hip: the stand-in samplers (n * hw within 32 bits, actions 16-byte aligned: mrts_capi.cpp checks)
hipError_t mrts_engine_sample(const int32_t *mask, int n, int hw, int env0, uint64_t seed, uint32_t step, int64_t *act, hipStream_t s);
hipError_t mrts_engine_sample_src(const int32_t *mask, const int32_t *src, int n, int hw, int env0, uint64_t seed, uint32_t step,
                                  int64_t *act, hipStream_t s);
hipError_t mrts_engine_sample_src_group(const mrts_sample_seg *segs, int nseg, uint64_t seed, uint32_t step, hipStream_t s);
// k_sample_src's picks as packed action words [n][hw] (mrts_actions.h), and the converters between the
// words and the int64 rows (rows = n * hw; 16-byte accesses on the int64 side when it is 16-byte aligned)
hipError_t mrts_engine_sample_src_packed(const int32_t *mask, const int32_t *src, int n, int hw, int env0, uint64_t seed, uint32_t step,
                                         int32_t *words, hipStream_t s);
hipError_t mrts_engine_pack_actions(const int64_t *act, long long rows, int32_t *words, hipStream_t s);
hipError_t mrts_engine_unpack_actions(const int32_t *words, long long rows, int64_t *act, hipStream_t s);
// mrts_policy.hip: the masked action head (sample / evaluate / evaluate's backward).  packed == 0: `mask` is
// the dense [n][hw][78] with its `src` [n][hw]; packed != 0: `mask` is the packed words [n][hw][3]
// (mrts_actions.h) and `src` is not read.  act_packed == 0: `act` is the int64 rows [n][hw][7]; != 0: it is
// the packed action words [n][hw] int32.  Then the mask converters (rows = n * hw).
hipError_t mrts_engine_policy_sample(int packed, int act_packed, const float *logits, const int32_t *mask, const int32_t *src, int n,
                                     int hw, int env0, uint64_t seed, uint32_t step, void *act, float *logprob, float *entropy,
                                     hipStream_t s);
hipError_t mrts_engine_policy_eval(int packed, int act_packed, const float *logits, const int32_t *mask, const int32_t *src, int n,
                                   int hw, const void *act, float *logprob, float *entropy, hipStream_t s);
hipError_t mrts_engine_policy_eval_bwd(int packed, int act_packed, const float *logits, const int32_t *mask, const int32_t *src, int n,
                                       int hw, const void *act, const float *g_lp, const float *g_ent, float *grad, hipStream_t s);
hipError_t mrts_engine_pack_masks(const int32_t *mask, const int32_t *src, long long rows, int32_t *packed, hipStream_t s);
hipError_t mrts_engine_unpack_masks(const int32_t *packed, long long rows, int32_t *mask, int32_t *src, hipStream_t s);
// mrts_obs.hip: the converters between the packed obs words (mrts_rules.h cell_onehot) and the dense planes.
// elem_bytes 2 or 4; `one`: a stored one's bits (unpack); `nonzero`: the bits that make an element non-zero (pack)
hipError_t mrts_engine_unpack_obs(const int32_t *packed, long long rows, int planes, int elem_bytes, uint32_t one, void *obs, hipStream_t s);
hipError_t mrts_engine_pack_obs(const void *obs, long long rows, int planes, int elem_bytes, uint32_t nonzero, int32_t *packed, hipStream_t s);
// mrts_conv.hip: the first encoder stage on the packed words (conv3x3 + max-pool + ReLU), its backward to the
// parameters (k_obs_conv_bwd into `ws`, then the reduction) and the bytes `ws` needs (-1: no tile of the shape fits)
long long mrts_engine_obs_conv_workspace(int n, int h, int w, int planes, int channels);
hipError_t mrts_engine_obs_conv_fwd(const int32_t *packed, int n, int h, int w, int planes, const float *weight, const float *bias,
                                    int channels, float *out, hipStream_t s);
hipError_t mrts_engine_obs_conv_bwd(const int32_t *packed, int n, int h, int w, int planes, const float *weight, const float *bias,
                                    int channels, const float *grad_out, float *ws, float *grad_weight, float *grad_bias, hipStream_t s);
// mrts_engine.hip again (mrts_engine_bot_lds_bytes: mrts_bots.hip)
hipError_t mrts_engine_masks_packed(const EngineParams *p, hipStream_t s, int32_t *packed);
hipError_t mrts_engine_render(const EngineParams *p, hipStream_t s, int game, int map, int size, uint8_t *rgb);
size_t mrts_engine_bot_lds_bytes(int HW, int W);
}
#endif
