// mrts_engine.hip -- gfx950 kernels of the vectorised MicroRTS engine.
//
// Restates, on the device, the Java path behind MicroRTSGridModeVecEnv
// (/root/reference/gym_microrts/envs/vec_env.py): JNIGridnetVecClient.reset
// (vec_env.py:279), .gameStep (vec_env.py:1002: JNIAI action decode, issueSafe
// p0/p1, GameState.cycle, the six ai.reward functions, auto-reset) and
// .getMasks (vec_env.py:1097), plus the python-side one-hot encoder
// _encode_obs (vec_env.py:311-321).  Rules: SURVEY.md Appendix A, DESIGN.md §4.
//
// Mapping: one workgroup per GAME, one lane per grid cell (16x16 -> 256 lanes),
// the game's cell records staged in LDS.  Everything that is per-cell runs
// lane-parallel (decode, legality, masks, readiness, one-hot); the parts of the
// Java that are inherently ordered (PlayerAction consistency filter, issue()
// conflict resolution, execution of ready actions in LinkedHashMap order) run
// on lane 0 over compact ballot-built lists, which hold only the few units
// that act this tick.  Outputs are written with 16-byte stores from compact
// per-cell bit words in LDS (one-hot obs: 1 word/cell, mask: 3 words/cell); of the
// bound mask rows the step stores only those that can differ from the last tick's
// (delta masks, stream_masks_delta).
// A step launch takes a StepGroup: one or more engines (map-size buckets) cut
// into grid segments, bot games first (mrts_step_group).
// In this unit: the game step, the output streams (reset / masks / packed masks / outputs / raw obs),
// the renderer, their launchers.  Elsewhere: the scripted opponents (mrts_bots.hip), the
// stand-in samplers (mrts_sampler.hip), the masked action head (mrts_policy.hip).
//
// Integer work only: no MFMA, the kernels are HBM-bound on the obs/mask writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "mrts_actions.h"
#include "mrts_engine.h"
#include "mrts_layout.h"

#include "mrts_rules.h"
#include "mrts_bots.h"

namespace mrts {

// ---------------------------------------------------------------------------
// The step workgroup's LDS (Carver: mrts_engine.h)
struct Lds {
    uint32_t* unit;
    int32_t* uid;
    uint32_t* act;
    uint32_t* seq;
    uint32_t* aux;   // decoded rows, then one-hot / mask bit words
    int32_t* resv;   // reservation holder per cell
    int32_t* list;   // compact cell lists
    int32_t* prod;   // pending produce cells
    int32_t* blist;  // the bot's PlayerAction order (bot games)
    int32_t* blist0; // player 0's bot PlayerAction (bot-vs-bot games)
    int4* snap;      // ready-action snapshots
    uint32_t* outw;  // emit_outputs one-hot words [NV][HW]: aliases resv .. snap (32 B per cell with outm)
    uint32_t* outm;  // emit_outputs mask words [NV][HW][3] (outw + 2 HW, unless the fused step places them)
    uint8_t* wall;
    unsigned long long* ballot;
    uint32_t* posbits;
    uint32_t* claim;   // [2][pos_words] target positions claimed by >= 1 / >= 2 rows this tick
    uint32_t* vis;   // [2][vis_words] cells observable by player 0 / 1 (partial obs)
    int* sc;         // scalars
};
// L.sc[0 .. MRTS_GENV_WORDS) mirrors genv (load_game / store_game)
enum { SC_TIME = MRTS_G_TIME, SC_RES0 = MRTS_G_RES0, SC_RES1 = MRTS_G_RES1, SC_UID = MRTS_G_NEXT_UID,
       SC_STEPS = MRTS_G_STEPS, SC_MAP = MRTS_G_MAP, SC_ERR = MRTS_G_ERR, SC_AA_N = MRTS_G_AA_N, SC_TICKS = MRTS_G_TICKS,
       SC_NPA = MRTS_G_NPA, SC_R0 = 16, /* rewards: [player][6] as ints */ SC_NPROD = 28, SC_RPROD = 29 /* ready produces */,
       SC_OVER = 30 /* a pending produce is over its owner's budget */,
       SC_HAS = 31 /* units of player 0 (bits 0..15) and player 1 (16..31) */,
       SC_PSUM = 32 /* [2] cost of the player's produce rows this tick */,
       SC_PMAX = 34 /* [2] largest cost among the player's pending produces */,
       SC_SERIAL = 36 /* the ready set executes in order */, SC_NPEND = 37 /* pending produces listed in L.prod */,
       SC_NREADY = 38 /* ready assignments listed in L.list */, SC_NLEFT = 39 /* rows (2a) left to the ordered path */,
       SC_WORDS = 40 };
static_assert(MRTS_GENV_WORDS <= SC_R0, "genv words overlap the LDS scalars");

// 16-byte store of an output row segment (obs / masks: written once, read by
// the consumer after the kernel; plain stores measured 5 % faster than
// non-temporal ones)
__device__ __forceinline__ void st16(void* dst, int a, int b, int c, int d) {
    v4i v = {a, b, c, d};
    *reinterpret_cast<v4i*>(dst) = v;
}

// The step layout.  b0: the blist0 array (player 0's bot PlayerAction: bot-vs-bot games,
// which are never bot-fused); own_wall: the terrain array (the fused step keeps it apart,
// fused_carve sets L.wall).  The layout's size is c.o afterwards.
__host__ __device__ inline Lds carve(Carver& c, int HW, int W, int NT, bool b0 = true, bool own_wall = true) {
    Lds L;
    L.unit = c.take<uint32_t>(HW);
    L.uid = c.take<int32_t>(HW);
    L.act = c.take<uint32_t>(HW);
    L.seq = c.take<uint32_t>(HW);
    L.aux = c.take<uint32_t>(HW);
    L.resv = c.take<int32_t>(HW);
    L.list = c.take<int32_t>(HW);
    L.prod = c.take<int32_t>(HW);
    L.blist = c.take<int32_t>(HW);
    // (!b0: unreachable by construction -- fused engines have no player-0 bots, mrts_capi fused())
    L.blist0 = b0 ? c.take<int32_t>(HW) : L.blist;
    L.snap = c.take<int4>(HW);
    L.outw = (uint32_t*)L.resv;   // resv, list, prod, blist, [blist0,] snap: >= 32 B per cell, contiguous
    L.outm = L.outw + 2 * HW;
    L.wall = own_wall ? c.take<uint8_t>(HW) : nullptr;
    const size_t ballots = (size_t)((HW + NT - 1) / NT) * (NT / 64);   // one 8-B word per wave and NT cells
    L.ballot = c.take<unsigned long long>(ballots + 1);
    L.posbits = c.take<uint32_t>(posbits_words(HW, W));
    L.sc = c.take<int>(SC_WORDS);
    // both players' visibility words (phase A), and before that the ballot words of the step's first compaction
    const size_t visw = vis_words(HW);
    L.vis = c.take<uint32_t>(2 * (visw > ballots ? visw : ballots));
    L.claim = c.take<uint32_t>(2 * (size_t)pos_words(HW, W));
    return L;
}
__host__ __device__ inline Lds carve(unsigned char* base, int HW, int W, int NT) {
    Carver c{base};
    return carve(c, HW, W, NT);
}

// Bot-fused k_step layout (24x24 52.3 KB -> 40.1 KB, 3 -> 4
// workgroups per CU), everything a fused workgroup needs, carved once:
//   [0, core)   the step's arrays (no blist0, no terrain) until phase A, the
//               bot's (unit uid act ucell uuid pa, abstract actions) afterwards
//   words       a bot game's output words: it streams them while wave 0 runs the
//               bot, so they lie outside the bot's region -- its mask words (one
//               view, 12 B per cell) here, its one-hot words (4 B per cell) in the
//               step's uid array on the early path (the bot reads uids only in its
//               setup, which the workgroup builds before the waves split), else
//               here behind the mask words
//   tail        the bot's small arrays (pend pab vis sc fw)
//   early_cnt   the streaming waves' phase-A meeting point (early path)
//   wall        the terrain, read in place by the step, phase A and the bot
// bot_game = false: a selfplay game of a fused launch, which runs no bot and aliases
// its output words onto the step's dead arrays, as the unfused kernel does.  `early`:
// the engine takes the early path (full observability and early_bot_disjoint).
struct FusedLds {
    Lds L;
    uint32_t* words;       // the output words' region (a bot game's L.outm / L.outw)
    uint32_t* tail;        // the bot's small arrays, tail_words of them: zeroed for the early bot
    int tail_words;
    int* early_cnt;
    size_t bytes;
    bots::BL B;            // the bot's arrays: its core over the step's, its small arrays in the tail, the step's terrain
};
// step_log: the extents of F.L's arrays, the words, the counter and the terrain; bot_log: of F.B's own arrays
// (two logs: the step's and the bot's arrays start at the same addresses)
__host__ __device__ inline FusedLds fused_carve(unsigned char* base, int HW, int W, int NT, bool early, bool bot_game,
                                                SpanLog* step_log = nullptr, SpanLog* bot_log = nullptr) {
    FusedLds F;
    Carver c{base, 0, step_log}, cb{base, 0, bot_log};
    F.L = carve(c, HW, W, NT, false, false);
    bots::bot_carve_core(cb, F.B, HW);
    c.o = cb.o = c.o > cb.o ? c.o : cb.o;
    F.words = c.take<uint32_t>((early ? 3 : 4) * (size_t)HW);
    if (bot_game) {
        F.L.outw = early ? reinterpret_cast<uint32_t*>(F.L.uid) : F.words;
        F.L.outm = early ? F.words : F.words + HW;
    }
    // the tail's offset as one scalar: left as a sum, the compiler rebuilds the whole chain (64-bit adds of
    // spilled terms and the max above) in front of every bot loop that walks a small array
    cb.o = c.o = lds_uniform(c.o);
    F.tail = reinterpret_cast<uint32_t*>(base + cb.o);
    bots::bot_carve_tail(cb, F.B, HW, W);
    F.tail_words = (int)((cb.o - c.o) / 4);
    c.o = cb.o;
    F.early_cnt = c.take<int>(1);
    F.L.wall = F.B.wall = c.take<uint8_t>(HW);
    F.bytes = c.o;
    return F;
}

// The early-bot k_step (FB, P == 29): while wave 0 runs bots::bot_game (its
// small arrays in the tail region, the step's terrain read in place, setup
// preset), waves 1.. run emit_outputs' phase A, which reads the step's unit / act
// / wall / scalars and writes the output words (one-hot into the uid array, mask
// words behind the bot's region) and the meeting counter.  True when, for this
// map size, the bot writes none of those bytes and phase A writes none the bot
// reads -- every extent is the one the fused carve took -- and the bot's unit / uid /
// act arrays are the step's (it reads the state just stored in place).  The step
// launch takes the early path only then (EngineParams::early_bot; mrts_fused_layout_ok).
__host__ __device__ inline bool early_bot_disjoint(int HW, int W, int NT) {
    SpanLog step, bot;
    const FusedLds F = fused_carve(lds_any_base(), HW, W, NT, true, true, &step, &bot);
    const Lds& S = F.L;
    const bots::BL& B = F.B;
    auto overlap = [](const Span& a, const Span& b) { return a.p < b.p + b.n && b.p < a.p + a.n; };
    if (B.unit != S.unit || B.uid != S.uid || B.act != S.act) return false;
    const Span bot_w[9] = {bot.of(B.ucell), bot.of(B.uuid), bot.of(B.pa), bot.of(B.aa), bot.of(B.pend),
                           bot.of(B.pab), bot.of(B.vis), bot.of(B.sc), bot.of(B.fw)};
    const Span bot_r[3] = {bot.of(B.unit), bot.of(B.act), step.of(B.wall)};   // (uids: read by the setup only)
    const Span a_r[3] = {step.of(S.unit), step.of(S.act), step.of(S.wall)};   // (resources: in registers)
    const Span a_w[3] = {step.of(S.uid), step.of(F.words), step.of(F.early_cnt)};
    auto missing = [](const Span* t, int n) {
        for (int i = 0; i < n; i++) if (!t[i].p) return true;
        return false;
    };   // an array the logs do not hold would go unchecked: fail closed
    if (missing(bot_w, 9) || missing(bot_r, 3) || missing(a_r, 3) || missing(a_w, 3)) return false;
    for (const Span& b : bot_w) {
        if (b.p + b.n > lds_any_base() + F.bytes) return false;
        for (const Span& a : a_r) if (overlap(a, b)) return false;
        for (const Span& a : a_w) if (overlap(a, b)) return false;
    }
    for (const Span& a : a_w)
        for (const Span& b : bot_r) if (overlap(a, b)) return false;
    return true;
}

// Ordered block-wide compaction: list <- cells c (ascending) with pred(c);
// put(position, c) is called for every entry as it is written.  TAIL = false
// drops the trailing barrier: the caller orders the list before its readers, and
// the next compaction must use another s_mask.
struct NoPut {
    __device__ void operator()(int, int) const {}
};
template <int NT, bool TAIL = true, typename F, typename G = NoPut>
__device__ __forceinline__ int compact_cells(int HW, F pred, int32_t* list, unsigned long long* s_mask, G put = G()) {
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int J = (HW + NT - 1) / NT;
    for (int j = 0; j < J; j++) {
        int c = j * NT + threadIdx.x;
        bool f = c < HW && pred(c);
        unsigned long long m = __ballot(f);
        if (lane == 0) s_mask[j * NW + w] = m;
    }
    __syncthreads();
    int total = 0;
    for (int j = 0; j < J; j++) {
        int mi = j * NW + w;
        int before = 0;
        for (int k = 0; k < J * NW; k++) {
            int pc = __popcll(s_mask[k]);
            if (k < mi) before += pc;
            if (j == 0) total += pc;
        }
        unsigned long long m = s_mask[mi];
        if ((m >> lane) & 1ull) {
            const int pos = before + __popcll(m & ((1ull << lane) - 1ull)), c = j * NT + threadIdx.x;
            list[pos] = c;
            put(pos, c);
        }
    }
    if (TAIL) __syncthreads();
    return total;
}

// The early bot's setup, by the whole workgroup (all NT lanes, the state final
// in LDS, before the waves split): the parts of bots::bot_game's setup that are
// per cell -- the pending assignments' reservations and produce costs
// (isUnitActionAllowed's ResourceUsage), the free-cell words of path finding, and
// the unit list in pgs.units order (appended in any order, then ranked by uid)
// -- into the bot's LDS arrays (its tail zeroed at the kernel's start); the bot
// wave then starts at the abstract actions (bot_game, preset).  Full observability
// only (the early path's condition), so the bot's view is the state itself.
template <int NT>
__device__ __forceinline__ void bot_setup_workgroup(const EngineParams& p, const bots::BL& B) {
    const int HW = p.HW, W = p.W, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // unit list by cell (B.pa), its uids alongside (the first words of B.aa, rewritten
    // by the bot later); B.sc[3] (zeroed with the tail) counts them
    int32_t* const ucells = B.pa;
    int32_t* const uids = reinterpret_cast<int32_t*>(B.aa);
    for (int base = 0; base < HW; base += NT) {
        const int c = base + (int)threadIdx.x;
        bool fr = false;
        if (c < HW) {
            const uint32_t u = B.unit[c], a = B.act[c];
            fr = !B.wall[c] && u == 0;
            if (u != 0) {
                const int pos = atomicAdd(&B.sc[3], 1);
                ucells[pos] = c;
                uids[pos] = B.uid[c];
            }
            if (a) {
                const int code = act_code(a), t = code_type(code);
                if (t == A_MOVE || t == A_PRODUCE) {
                    const int d = code_param(code), pos = c + (d == 0 ? -W : d == 1 ? 1 : d == 2 ? W : -1) + W;
                    atomicOr(&B.pend[pos >> 5], 1u << (pos & 31));
                    if (t == A_PRODUCE && u_owner(u) >= 0) atomicAdd(&B.sc[u_owner(u)], ut_cost(code_utype(code)));
                }
            }
        }
        const unsigned long long m = __ballot(fr);   // cells base + 64 wv .. + 63
        if (lane == 0 && base + 64 * wv < HW) {
            B.fw[(base + 64 * wv) / 32] = (uint32_t)m;
            B.fw[(base + 64 * wv) / 32 + 1] = (uint32_t)(m >> 32);
        }
    }
    __syncthreads();
    const int n = B.sc[3];
    for (int i = threadIdx.x; i < n; i += NT) {   // rank by uid (uids are unique)
        const int u = uids[i];
        int r = 0, j = 0;
        for (; j + 4 <= n; j += 4) {
            const int4 v = *reinterpret_cast<const int4*>(uids + j);
            r += (v.x < u) + (v.y < u) + (v.z < u) + (v.w < u);
        }
        for (; j < n; j++) r += uids[j] < u;
        B.ucell[r] = ucells[i];
        B.uuid[r] = u;
    }
}

// A wave-uniform flag as one scalar word, tested where it is used.  (A bool that lives across phases is kept as
// a 64-bit lane mask, two scalar registers, and the step kernel sits at its scalar-register limit; the empty
// asm keeps the compiler from merging the tests of one word into such a mask again.)
__device__ __forceinline__ int flag_word(int b) {
    b = __builtin_amdgcn_readfirstlane(b);
    asm volatile("" : "+s"(b));
    return b;
}
// The full-workgroup step (k_step's FULL: every engine of the launch has HW == NT, one cell per lane and no lane
// idle -- 16x16 on 256 lanes): HW is a compile-time constant from here to the next barrier.  The cell loops run
// once without a bound check, the wider paths drop out, and the LDS arrays' offsets fold into the instructions.
// Loads of p.HW behind a barrier are new loads: say it again there.
template <bool FULL, int NT>
__device__ __forceinline__ void full_hw(const EngineParams& p) {
    if (FULL) __builtin_assume(p.HW == NT);
}

struct Game {
    int g, env0, nviews, selfplay;
};
__device__ __forceinline__ Game game_of(const EngineParams& p, int g) {
    Game G;
    G.g = g;
    G.selfplay = flag_word(g < p.nsp_games);
    G.env0 = G.selfplay ? 2 * g : p.nsp + (g - p.nsp_games);
    G.nviews = G.selfplay ? 2 : 1;
    return G;
}

// PhysicalGameState.load + new GameState into LDS
template <int NT>
__device__ __forceinline__ void reset_into_lds(const EngineParams& p, const Lds& L, int map) {
    const int HW = p.HW;
    for (int c = threadIdx.x; c < HW; c += NT) {
        int4 v = p.map_cells[(size_t)map * HW + c];
        L.unit[c] = (uint32_t)v.x;
        L.uid[c] = v.y;
        L.act[c] = 0;
        L.seq[c] = 0;
        L.wall[c] = p.map_wall[(size_t)map * HW + c];
    }
    if (threadIdx.x == 0) {
        const int* ms = p.map_scal + (size_t)map * MRTS_MAP_SCALARS;
        L.sc[SC_TIME] = 0;
        L.sc[SC_RES0] = ms[MRTS_M_RES0];
        L.sc[SC_RES1] = ms[MRTS_M_RES1];
        L.sc[SC_UID] = ms[MRTS_M_NUNITS];
        L.sc[SC_STEPS] = 0;
        L.sc[SC_MAP] = map;
    }
}

template <int NT>
__device__ __forceinline__ void load_game(const EngineParams& p, const Lds& L, int g) {
    if (threadIdx.x < MRTS_GENV_WORDS) L.sc[threadIdx.x] = p.genv[(size_t)g * MRTS_GENV_WORDS + threadIdx.x];
    __syncthreads();
    const int HW = p.HW, map = L.sc[SC_MAP];
    const int4* src = p.cells + (size_t)g * p.cstride;
    for (int c = threadIdx.x; c < HW; c += NT) {
        int4 v = src[c];
        L.unit[c] = (uint32_t)v.x;
        L.uid[c] = v.y;
        L.act[c] = (uint32_t)v.z;
        L.seq[c] = (uint32_t)v.w;
        L.wall[c] = p.map_wall[(size_t)map * HW + c];
    }
    __syncthreads();
}

template <int NT>
__device__ __forceinline__ void store_game(const EngineParams& p, const Lds& L, int g) {
    const int HW = p.HW;
    int4* dst = p.cells + (size_t)g * p.cstride;
    for (int c = threadIdx.x; c < HW; c += NT) dst[c] = make_int4((int)L.unit[c], L.uid[c], (int)L.act[c], (int)L.seq[c]);
    if (threadIdx.x < MRTS_GENV_WORDS) p.genv[(size_t)g * MRTS_GENV_WORDS + threadIdx.x] = L.sc[threadIdx.x];
}

// PartiallyObservableGameState.observable for both players: a cell is seen by
// player q when some unit of q is within its sight radius (d^2 <= r^2).  Each
// unit lane ORs its sight disk into the player's LDS bitmap, one row span per
// atomic (or_sight_disk).
template <int NT>
__device__ __forceinline__ void compute_vis(const EngineParams& p, const Lds& L) {
    const int HW = p.HW, nw = vis_words(HW);
    for (int i = threadIdx.x; i < 2 * nw; i += NT) L.vis[i] = 0;
    __syncthreads();
    for (int c = threadIdx.x; c < HW; c += NT) {
        uint32_t u = L.unit[c];
        int q = u_owner(u);
        if (u == 0 || q < 0) continue;
        or_sight_disk(L.vis + q * nw, c % p.W, c / p.W, ut_sight(u_type(u)), p.W, p.H);
    }
    __syncthreads();
}

// view v's one-hot word of cell c (unit u, action a, terrain wl; with fog, the sight disks in L.vis)
template <int P>
__device__ __forceinline__ uint32_t onehot_word(const EngineParams& p, const Lds& L, int c, int v, uint32_t u, uint32_t a, uint8_t wl) {
    if (P == 31) {
        const int nw = vis_words(p.HW);
        const bool shown = u == 0 || u_owner(u) == v || ((L.vis[v * nw + (c >> 5)] >> (c & 31)) & 1u);
        const bool opp = (L.vis[(1 - v) * nw + (c >> 5)] >> (c & 31)) & 1u;
        return cell_onehot(u, a, wl, v, P, shown, opp);
    }
    return cell_onehot(u, a, wl, v);
}
// Delta obs (EngineParams::obs_delta): a one-hot word uses bits 0 .. P-1 (P <= 31); bit 31 carries
// whether the cell's row is stored at all.  step_game keeps a key of every cell of the loaded state
// and leaves it in L.outw, onehot_words marks the words of the cells whose key differs by now,
// stream_obs_delta stores the marked rows.  The dense streams mask the bit off.
constexpr uint32_t OBS_ROW_STORE = 1u << 31;
// The key: everything cell_onehot reads of the cell, for every view at once, in 16 bits, so that a lane
// holds two cells' keys per register (the views' full words would take four): the terrain bit, and for
// a unit a mixed-radix number of its clamped hit points (5) and resources (5), owner (3), action type (6)
// and type (7), 3150 values.  0 / 1: an empty cell.  Every view's word is a function of the key (the
// views differ in how they read the owner), so an equal key means equal rows, and a changed key a
// changed row in every view.  Full observability only: with fog the words also depend on the sight
// disks, and the pass that builds the loaded state's disks cost more than the stores it saved
// (profiles/obs_delta/README.md), so a fog engine steps dense (mrts_capi.cpp obs_delta_ok).
constexpr int OBS_KEY_BITS = 16;
template <int P>
constexpr bool obs_delta_built = P == 29;
__device__ __forceinline__ uint32_t obs_key(uint32_t u, uint32_t a, uint8_t wl) {
    const uint32_t empty = wl ? 1u : 0u;
    if (u == 0) return empty;
    const int hp = min(max(u_hp(u), 0), 4), res = min(u_res(u), 4), ow = u_owner(u);
    const int at = a ? min(code_type(act_code(a)), 5) : 0;
    const uint32_t idx = ((((uint32_t)hp * 5u + (uint32_t)res) * 3u + (uint32_t)(ow < 0 ? 0 : min(ow, 1) + 1)) * 6u + (uint32_t)at) * 7u +
                         (uint32_t)min(u_type(u), 6);   // < 3150
    return ((idx + 1u) << 1) | empty;   // 2 .. 6301
}
// phase A's one-hot word of cell c for every view of the game (into L.outw); `delta`: L.outw[c] holds
// the cell's key in the loaded state, and the words of a cell whose key differs are marked OBS_ROW_STORE
template <int P>
__device__ __forceinline__ void onehot_words(const EngineParams& p, const Lds& L, const Game& G, int c, bool delta = false) {
    const int HW = p.HW;
    const uint32_t u = L.unit[c], a = L.act[c];
    const uint8_t wl = L.wall[c];
    const uint32_t mark = obs_delta_built<P> && delta && obs_key(u, a, wl) != L.outw[c] ? OBS_ROW_STORE : 0u;
    for (int v = 0; v < G.nviews; v++) L.outw[v * HW + c] = onehot_word<P>(p, L, c, v, u, a, wl) | mark;
}
// Delta masks (EngineParams::mask_delta): a row's third word carries, above its 15
// mask bits (a row is 79 of the words' 96 bits), whether the row is stored at all.
// step_game presets the bit for the source rows of the state it loaded, mask_words
// adds the source rows of the final state, stream_masks_delta stores the marked rows.
// The dense stream never reads the bit.
constexpr uint32_t MASK_ROW_STORE = 1u << 31;
__device__ __forceinline__ void mask_words(const EngineParams& p, const Lds& L, const Game& G, int c, int res0, int res1,
                                           bool delta = false) {
    const int HW = p.HW;
    const Grid gd{p.W, p.H, HW};
    for (int v = 0; v < G.nviews; v++) {
        uint32_t m[3];
        cell_mask(gd, c, v, L.unit, L.act, L.wall, v == 0 ? res0 : res1, m);
        if (delta) m[2] |= (L.outm[3 * (v * HW + c) + 2] & MASK_ROW_STORE) | ((m[0] & 1u) ? MASK_ROW_STORE : 0u);
        L.outm[3 * (v * HW + c)] = m[0];
        L.outm[3 * (v * HW + c) + 1] = m[1];
        L.outm[3 * (v * HW + c) + 2] = m[2];
        p.src_out[(size_t)(G.env0 + v) * HW + c] = (int32_t)(m[0] & 1u);
    }
}
// phase B's obs rows of every view, lanes t0 .. t0 + nt
template <int P, typename OT>
__device__ __forceinline__ void stream_obs(const EngineParams& p, const Lds& L, const Game& G, int t0, int nt) {
    const int HW = p.HW, NV = G.nviews;
    const uint32_t* ow = L.outw;
    auto word = [&](int i) { return ow[i] & ~OBS_ROW_STORE; };   // (a word's store mark is the delta stream's)
    OT* out = reinterpret_cast<OT*>(p.obs) + (size_t)G.env0 * HW * P;
    const int total = NV * HW * P;
    if (((HW * P) & 3) == 0) {   // every env's rows start 16-B aligned
        constexpr int ONE = std::is_same<OT, float>::value ? 0x3f800000 : 1;   // 1.0f or 1 as stored bits
        // elements e .. e+3 are planes pl .. pl+3 of cell c, running on into cell
        // c+1 past plane P-1: one paired LDS read (cells c, c+1) per 16-B store.
        // (c+1 past the last cell reads the words behind: never used, as the last
        // store of the run ends at plane P-1.)  A one-hot word has no bit at or
        // above P, so (w0 >> pl) | (w1 << (P - pl)) are the window's bits.  (c, pl)
        // advance by a constant per trip: no division in the loop.
        // Software-pipelined: the next trip's word pair is read before this trip's
        // store, so the LDS round trip overlaps the bit work instead of stalling every
        // trip (a lone workgroup's stream -- the kernel's last round -- is bound by this
        // loop, not by the store path: scripts/store_rate.hip).  The read-ahead index is
        // clamped into the word region (its last trip's values are never used).
        const int dq = 4 * nt / P, dr = 4 * nt - dq * P, cmax = NV * HW - 1;
        int c = 4 * t0 / P, pl = 4 * t0 - c * P;
        uint32_t w0 = word(min(c, cmax)), w1 = word(min(c, cmax) + 1);
        for (int k = t0; k < total / 4; k += nt) {
            int cn = c + dq, pn = pl + dr;
            if (pn >= P) { pn -= P; cn++; }
            const int cr = min(cn, cmax);
            const uint32_t n0 = word(cr), n1 = word(cr + 1);
            const uint32_t bits = (w0 >> pl) | (w1 << (P - pl));
            st16(out + 4 * k, (bits & 1u) ? ONE : 0, (bits & 2u) ? ONE : 0, (bits & 4u) ? ONE : 0, (bits & 8u) ? ONE : 0);
            w0 = n0;
            w1 = n1;
            c = cn;
            pl = pn;
        }
    } else {
        for (int e = t0; e < total; e += nt) out[e] = (OT)((ow[e / P] >> (e % P)) & 1u);
    }
}
// Packed obs (MRTS_OBS_PACKED, OT = PackedObs; the format: mrts_rules.h cell_onehot): phase B's
// obs are the views' NV * HW one-hot words as phase A left them, copied out to p.obs [N][HW].
// HW % 4 == 0: every game's run starts 16-B aligned in a 16-B aligned buffer, in LDS too (outw
// is a carved array), so 16-byte copies; otherwise (9x13, or a buffer off 16 B) per word.
// Reads nothing but outw and kernel parameters, as phase B must.
struct PackedObs {};
template <typename OT>
constexpr bool obs_packed = std::is_same<OT, PackedObs>::value;
__device__ __forceinline__ void stream_obs_words(const EngineParams& p, const Lds& L, const Game& G, int t0, int nt) {
    const int HW = p.HW, n = G.nviews * HW;
    const uint32_t* ow = L.outw;
    int32_t* out = reinterpret_cast<int32_t*>(p.obs) + (size_t)G.env0 * HW;
    if ((HW & 3) == 0 && ((uintptr_t)p.obs & 15u) == 0) {
        const v4i* w4 = reinterpret_cast<const v4i*>(ow);
        for (int k = t0; k < n / 4; k += nt) *reinterpret_cast<v4i*>(out + 4 * k) = w4[k];
    } else {
        for (int i = t0; i < n; i += nt) out[i] = (int32_t)ow[i];
    }
}
// phase B's obs rows with delta obs: only the rows whose word is marked OBS_ROW_STORE (a few of a
// game's NV HW; the others hold these bytes already).  Each wave scans 64 words per trip, one per lane,
// and stores the marked rows two per instruction: lanes 0..P-1 one row, lanes 32..32+P-1 the next, a
// plane (4 bytes: a row is only 4-byte aligned) per lane.  Reads nothing but the words and kernel
// parameters, as phase B must.  Lanes t0 .. t0 + nt as the other streams; nt is a multiple of 64.
template <int P, typename OT>
__device__ __forceinline__ void stream_obs_delta(const EngineParams& p, const Lds& L, const Game& G, int t0, int nt) {
    static_assert(sizeof(OT) == 4 && P <= 31, "a plane per lane, half a wave per row; bit 31 is the mark");
    constexpr uint32_t ONE = std::is_same<OT, float>::value ? 0x3f800000u : 1u;   // 1.0f or 1 as stored bits
    const int rows = G.nviews * p.HW, lane = t0 & 63, pl = lane & 31;
    const uint32_t* ow = L.outw;
    uint32_t* out = reinterpret_cast<uint32_t*>(p.obs) + (size_t)G.env0 * p.HW * P;
    for (int base = t0 - lane; base < rows; base += nt) {   // wave-uniform
        const int r = base + lane;
        unsigned long long m = __ballot(r < rows && (ow[r] & OBS_ROW_STORE) != 0);
        while (m) {
            int b = __builtin_ctzll(m);   // the low half's row
            m &= m - 1;
            if (lane >= 32) b = m ? __builtin_ctzll(m) : -1;   // the high half's: the next marked one, if any
            m &= m - 1;   // (0 stays 0)
            if (b >= 0 && pl < P) out[(size_t)(base + b) * P + pl] = ((ow[base + b] >> pl) & 1u) ? ONE : 0u;
        }
    }
}
// phase B's obs of every view in the engine's obs kind; `delta`: only the marked rows (dense kinds)
template <int P, typename OT>
__device__ __forceinline__ void stream_obs_kind(const EngineParams& p, const Lds& L, const Game& G, int t0, int nt, bool delta = false) {
    if constexpr (obs_packed<OT>) {
        stream_obs_words(p, L, G, t0, nt);
    } else {
        if (delta) stream_obs_delta<P, OT>(p, L, G, t0, nt);
        else stream_obs<P, OT>(p, L, G, t0, nt);
    }
}
// phase B's mask rows of every view, lanes t0 .. t0 + nt
__device__ __forceinline__ void stream_masks(const EngineParams& p, const Lds& L, const Game& G, int t0, int nt) {
    const int HW = p.HW, NV = G.nviews;
    const uint32_t* mw = L.outm;
    int32_t* out = p.mask + (size_t)G.env0 * HW * MRTS_MASK_CH;
    const int total = NV * HW * MRTS_MASK_CH;
    if ((HW & 1) == 0) {   // HW * 78 % 4 == 0: every env's rows start 16-B aligned
        // elements e .. e+3 are channels ch .. ch+3 of row r = bits ch+1 .. ch+4 of
        // its 79-bit word (bit 0 = source); e is a multiple of 4 and a row pair
        // is 156 elements, so ch is even and only ch = 76 runs into row r+1
        // (channels 76, 77 = bits 77, 78, then bits 1, 2 of the next row, whose
        // first word is the word after bit 78's).  One paired LDS read per store.
        // (r, ch) advance by a constant per trip; the ch == 76 fix-up is a select,
        // not a branch.
        static_assert(MRTS_MASK_CH == 78, "mask row layout");
        // (software-pipelined as the obs loop: the next trip's word pair read ahead)
        const int dq = 4 * nt / MRTS_MASK_CH, dr = 4 * nt - dq * MRTS_MASK_CH, wmax = 3 * NV * HW - 1;
        int r = 4 * t0 / MRTS_MASK_CH, ch = 4 * t0 - r * MRTS_MASK_CH;
        int r3 = 3 * r;   // the row's first word
        int wr = min(r3 + ((ch + 1) >> 5), wmax);
        uint32_t lo = mw[wr], hi = mw[wr + 1];
        for (int k = t0; k < total / 4; k += nt) {
            int r3n = r3 + 3 * dq, chn = ch + dr;
            if (chn >= MRTS_MASK_CH) { chn -= MRTS_MASK_CH; r3n += 3; }
            wr = min(r3n + ((chn + 1) >> 5), wmax);
            const uint32_t nlo = mw[wr], nhi = mw[wr + 1];
            const int b0 = ch + 1;
            const uint32_t fun = (uint32_t)((((uint64_t)hi << 32) | lo) >> (b0 & 31));
            const uint32_t bits = ch == 76 ? ((fun & 3u) | ((hi << 1) & 0xCu)) : fun;
            st16(out + 4 * k, (int)(bits & 1u), (int)((bits >> 1) & 1u), (int)((bits >> 2) & 1u), (int)((bits >> 3) & 1u));
            lo = nlo;
            hi = nhi;
            r3 = r3n;
            ch = chn;
        }
    } else {
        for (int e = t0; e < total; e += nt) {
            const int r = e / MRTS_MASK_CH, b = e % MRTS_MASK_CH + 1;
            out[e] = (int)((mw[3 * r + (b >> 5)] >> (b & 31)) & 1u);
        }
    }
}

// phase B's mask rows with delta masks: only the rows marked MASK_ROW_STORE (some tens
// of a game's 2 HW; the others hold zeros already).  Each wave scans 64 rows per trip,
// one per lane, and stores the marked ones together: lanes 0..38 two channels each, one
// 8-byte store per row (a row starts at a multiple of 312 bytes: 8-byte aligned for
// every map size).  Lanes t0 .. t0 + nt as the other streams; nt is a multiple of 64.
__device__ __forceinline__ void stream_masks_delta(const EngineParams& p, const Lds& L, const Game& G, int t0, int nt) {
    static_assert(MRTS_MASK_CH == 78, "mask row layout");
    typedef int v2i __attribute__((ext_vector_type(2)));
    const int rows = G.nviews * p.HW, lane = t0 & 63;
    const uint32_t* mw = L.outm;
    int32_t* out = p.mask + (size_t)G.env0 * p.HW * MRTS_MASK_CH;
    for (int base = t0 - lane; base < rows; base += nt) {   // wave-uniform
        const int r = base + lane;
        unsigned long long m = __ballot(r < rows && (mw[3 * r + 2] & MASK_ROW_STORE) != 0);
        while (m) {
            const int rr = base + __builtin_ctzll(m);
            m &= m - 1;
            if (lane < MRTS_MASK_CH / 2) {
                // channels 2 lane, 2 lane + 1 = bits b, b + 1 of the row's words (bit 0 = source), b odd
                const int b = 2 * lane + 1;
                const uint32_t w0 = mw[3 * rr], w1 = mw[3 * rr + 1], w2 = mw[3 * rr + 2] & ~MASK_ROW_STORE;
                const uint32_t lo = b < 32 ? w0 : b < 64 ? w1 : w2, hi = b < 32 ? w1 : b < 64 ? w2 : 0u;
                const uint32_t bits = (uint32_t)((((uint64_t)hi << 32) | lo) >> (b & 31));
                const v2i v = {(int)(bits & 1u), (int)((bits >> 1) & 1u)};
                *reinterpret_cast<v2i*>(out + (size_t)rr * MRTS_MASK_CH + 2 * lane) = v;
            }
        }
    }
}

// All outputs of one game once its state is final.  Phase A (lane per cell):
// every view's one-hot word and, with `masks`, its getMasks(0) 79-bit word
// (+ the source channel, written straight out) into LDS; one barrier; phase B:
// the views' obs rows, then their mask rows, streamed with 16-byte stores and no
// further barrier (the envs of a game are adjacent: a selfplay pair 2k, 2k+1
// writes one contiguous run).  The words live in the region of the step's
// scratch lists (resv .. snap), dead by now.
// `skip`: lanes [0, skip) leave after phase A (the bot-fused k_step's wave 0) and
// the others stream phase B alone.
// `early_cnt` (the early-bot k_step): wave 0 is running the bot already, so
// phase A too runs on lanes [skip, NT) only and its end is a counter the
// streaming waves meet at in LDS instead of a workgroup barrier.
// res0 / res1: the players' resources (the masks' produce checks), read by the
// caller from L.sc before the early bot may overwrite the step's scalars.
// Masks first (no bot in the workgroup, skip == 0): the mask words (no fog
// dependency) are built and their 2.5x larger stream issued before the one-hot
// words (and, under partial observability, the sight disks) are computed, so a
// game's first bytes leave one phase earlier and the obs words are built while the
// mask stores drain; one more barrier before the obs stream.
// `delta` (k_step with EngineParams::mask_delta): the mask rows' third words arrive
// preset with MASK_ROW_STORE and only the marked rows are stored (stream_masks_delta).
// `odelta` (k_step with EngineParams::obs_delta): L.outw[0, HW) arrives holding the cells' keys
// (obs_key) in the loaded state, written by the lanes that own the cells in phase A or, on the
// early path, ahead of a barrier; only the rows of cells whose key changed are stored (stream_obs_delta).
// `deltas`: bit 0 `delta`, bit 1 `odelta`, as one flag word (flag_word) that each phase tests for itself.
template <int NT, int P, typename OT, bool FULL = false>
__device__ __forceinline__ void emit_outputs(const EngineParams& p, const Lds& L, const Game& G, bool obs, bool masks, int res0,
                                             int res1, int skip = 0, int* early_cnt = nullptr, int deltas = 0) {
    full_hw<FULL, NT>(p);
    const int HW = p.HW;
    const bool delta = (deltas & 1) != 0;
    if (skip == 0 && obs && masks) {
        const int nw = vis_words(HW);
        for (int c = threadIdx.x; c < HW; c += NT) mask_words(p, L, G, c, res0, res1, delta);
        if (P == 31)
            for (int i = threadIdx.x; i < 2 * nw; i += NT) L.vis[i] = 0;
        __syncthreads();
        MRTS_STAMP(8, threadIdx.x == 0);
        __builtin_amdgcn_s_setprio(0);
        full_hw<FULL, NT>(p);
        if (flag_word(deltas) & 1) stream_masks_delta(p, L, G, threadIdx.x, NT);
        else stream_masks(p, L, G, threadIdx.x, NT);
        const bool odelta = (flag_word(deltas) & 2) != 0;
        if (P == 31) {   // compute_vis's sight disks (cleared above)
            for (int c = threadIdx.x; c < HW; c += NT) {
                const uint32_t u = L.unit[c];
                const int q = u_owner(u);
                if (u != 0 && q >= 0) or_sight_disk(L.vis + q * nw, c % p.W, c / p.W, ut_sight(u_type(u)), p.W, p.H);
            }
            __syncthreads();
        }
        for (int c = threadIdx.x; c < HW; c += NT) onehot_words<P>(p, L, G, c, odelta);
        __syncthreads();
        full_hw<FULL, NT>(p);
        stream_obs_kind<P, OT>(p, L, G, threadIdx.x, NT, odelta);
        MRTS_STAMP_MAX(9, (threadIdx.x & 63) == 0);
        return;
    }
    if (obs && P == 31) compute_vis<NT>(p, L);
    full_hw<FULL, NT>(p);
    const bool odelta = (flag_word(deltas) & 2) != 0;
    const int a0 = early_cnt ? skip : 0;   // phase A's first lane
    for (int c = (int)threadIdx.x - a0; c < HW; c += NT - a0) {
        if (obs) onehot_words<P>(p, L, G, c, odelta);
        if (masks) mask_words(p, L, G, c, res0, res1, delta);
    }
    if (early_cnt) {   // the streaming waves' own meeting point (wave 0 never arrives)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if ((threadIdx.x & 63u) == 0) __hip_atomic_fetch_add(early_cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        while (__hip_atomic_load(early_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < (NT - skip) / 64)
            __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
    // ---- phase B -----------------------------------------------------------
    // Bot-fused k_step (skip = 64): from here on wave 0 runs bots::bot_game, whose
    // LDS region starts at smem offset 0 and overwrites the step's arrays but the
    // unit / act / wall it reads and, on the early path, the uid array.  Phase B
    // must read nothing but the output words `ow` / `mw` (FusedLds::words) and
    // kernel parameters.
    if ((int)threadIdx.x < skip) return;
    MRTS_STAMP(8, (int)threadIdx.x == skip);
    __builtin_amdgcn_s_setprio(0);
    const int t0 = (int)threadIdx.x - skip, nt = NT - skip;
    full_hw<FULL, NT>(p);
    if (obs) stream_obs_kind<P, OT>(p, L, G, t0, nt, (flag_word(deltas) & 2) != 0);
    if (masks && (flag_word(deltas) & 1)) stream_masks_delta(p, L, G, t0, nt);
    else if (masks) stream_masks(p, L, G, t0, nt);
    MRTS_STAMP_MAX(9, (threadIdx.x & 63) == 0);
}

// A parked game's envs read zero: mask / source rows (when p.mask is set), and
// obs rows (zero_outputs).
template <int NT>
__device__ __forceinline__ void zero_mask_rows(const EngineParams& p, const Game& G) {
    if (!p.mask) return;
    const size_t n = (size_t)G.nviews * p.HW;
    int32_t* m = p.mask + (size_t)G.env0 * p.HW * MRTS_MASK_CH;
    for (size_t i = threadIdx.x; i < n * MRTS_MASK_CH; i += NT) m[i] = 0;
    for (size_t i = threadIdx.x; i < n; i += NT) p.src_out[(size_t)G.env0 * p.HW + i] = 0;
}
template <int NT, int P, typename OT>
__device__ __forceinline__ void zero_outputs(const EngineParams& p, const Game& G) {
    const size_t n = (size_t)G.nviews * p.HW;
    if constexpr (obs_packed<OT>) {   // the zero word: what unpacks to the dense zeros
        int32_t* obs = reinterpret_cast<int32_t*>(p.obs) + (size_t)G.env0 * p.HW;
        for (size_t i = threadIdx.x; i < n; i += NT) obs[i] = 0;
    } else {
        OT* obs = reinterpret_cast<OT*>(p.obs) + (size_t)G.env0 * p.HW * P;
        for (size_t i = threadIdx.x; i < n * P; i += NT) obs[i] = (OT)0;
    }
    zero_mask_rows<NT>(p, G);
}

// ---------------------------------------------------------------------------
// Reset kernel: every game (or the listed ones) back to its map; obs out.
// Parked games (mrts_park_games) keep their state and write zero outputs.
template <int NT, int P, typename OT>
__global__ __launch_bounds__(NT) void k_reset(EngineParams p, const int32_t* games, const int32_t* maps, int count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MRTS_STAMP_NONE();
    Lds L = carve(smem, p.HW, p.W, NT);
    int g = games ? games[blockIdx.x] : blockIdx.x;
    if (game_parked(p, g)) {
        zero_outputs<NT, P, OT>(p, game_of(p, g));
        return;
    }
    int map = maps ? maps[blockIdx.x] : p.genv[(size_t)g * MRTS_GENV_WORDS + MRTS_G_MAP];
    // a reset keeps the never-reset counters (bot RNG ticks, rollout statistics)
    if (threadIdx.x < SC_WORDS) {
        const int w = threadIdx.x;
        const bool keep = w == SC_TICKS || w == MRTS_G_SERIAL || w == MRTS_G_ORDERED || w == MRTS_G_EPISODES;
        L.sc[w] = keep ? p.genv[(size_t)g * MRTS_GENV_WORDS + w] : 0;
    }
    __syncthreads();
    reset_into_lds<NT>(p, L, map);
    __syncthreads();
    store_game<NT>(p, L, g);
    Game G = game_of(p, g);
    emit_outputs<NT, P, OT>(p, L, G, true, p.mask != nullptr, L.sc[SC_RES0], L.sc[SC_RES1]);
}

// ---------------------------------------------------------------------------
// Raw observation kernel: Response.observation = GameState.getVectorObservation
// (player) as the JNI client returns it, int32 [N][P_raw][H][W] (P_raw = 6, or 7
// with partial obs) -- the input of the reference's python _encode_obs
// (vec_env.py:280, 1035).  Same per-cell rules as cell_onehot, unencoded.
template <int NT>
__global__ __launch_bounds__(NT) void k_raw(EngineParams p, int32_t* raw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Lds L = carve(smem, p.HW, p.W, NT);
    const int g = blockIdx.x, HW = p.HW;
    const Game G = game_of(p, g);
    const int PR = p.partial_obs ? 7 : 6, nw = vis_words(HW);
    if (game_parked(p, g)) {   // a parked game's envs read zero (mrts_park_games)
        int32_t* out = raw + (size_t)G.env0 * PR * HW;
        for (int i = threadIdx.x; i < G.nviews * PR * HW; i += NT) out[i] = 0;
        return;
    }
    load_game<NT>(p, L, g);
    if (p.partial_obs) compute_vis<NT>(p, L);
    for (int v = 0; v < G.nviews; v++) {
        int32_t* out = raw + (size_t)(G.env0 + v) * PR * HW;
        for (int c = threadIdx.x; c < HW; c += NT) {
            uint32_t u = L.unit[c], a = L.act[c];
            if (p.partial_obs && u != 0 && u_owner(u) != v && !((L.vis[v * nw + (c >> 5)] >> (c & 31)) & 1u)) u = 0;
            const int ow = u_owner(u);
            out[0 * HW + c] = u ? u_hp(u) : 0;
            out[1 * HW + c] = u ? u_res(u) : 0;
            out[2 * HW + c] = (u && ow >= 0) ? (ow == v ? 1 : 2) : 0;
            out[3 * HW + c] = u ? u_type(u) + 1 : 0;
            out[4 * HW + c] = (u && a) ? code_type(act_code(a)) : 0;
            out[5 * HW + c] = L.wall[c];
            if (p.partial_obs) out[6 * HW + c] = (u && ((L.vis[(1 - v) * nw + (c >> 5)] >> (c & 31)) & 1u)) ? 1 : 0;
        }
    }
}

// ---------------------------------------------------------------------------
// Mask kernel: JNIGridnetVecClient.getMasks(0) -> [N][HW][78] + source [N][HW]
template <int NT>
__global__ __launch_bounds__(NT) void k_masks(EngineParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MRTS_STAMP_NONE();
    Lds L = carve(smem, p.HW, p.W, NT);
    const int g = blockIdx.x;
    if (game_parked(p, g)) {   // the caller's buffers need not be the ones zeroed at park time
        zero_mask_rows<NT>(p, game_of(p, g));
        return;
    }
    load_game<NT>(p, L, g);
    emit_outputs<NT, 29, int32_t>(p, L, game_of(p, g), false, true, L.sc[SC_RES0], L.sc[SC_RES1]);
}

// ---------------------------------------------------------------------------
// Packed mask kernel: getMasks(0)'s 79-bit words as they are -> packed [N][HW][3]
// (mrts_actions.h), the dense buffers and EngineParams::mask / src_out untouched.
// cell_mask's words go to LDS in output order (a game's views are adjacent envs: one
// contiguous run of nviews * HW * 3 words, staged at L.outw -- 16-byte aligned, 24 of
// the region's 32 bytes per cell) and leave with 16-byte stores when the game's first
// row is 16-byte aligned (12-byte rows: an odd HW leaves some envs unaligned), per word
// otherwise.  A parked game's rows are zero.
template <int NT>
__global__ __launch_bounds__(NT) void k_masks_packed(EngineParams p, int32_t* __restrict__ packed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Lds L = carve(smem, p.HW, p.W, NT);
    const int g = blockIdx.x, HW = p.HW;
    const Game G = game_of(p, g);
    int32_t* out = packed + (size_t)G.env0 * HW * MASK_PACKED_WORDS;
    const int nw = G.nviews * HW * MASK_PACKED_WORDS;
    const bool al16 = ((uintptr_t)out & 15u) == 0;
    if (game_parked(p, g)) {
        if (al16) {
            for (int k = threadIdx.x; k < nw / 4; k += NT) st16(out + 4 * k, 0, 0, 0, 0);
            for (int i = 4 * (nw / 4) + threadIdx.x; i < nw; i += NT) out[i] = 0;
        } else {
            for (int i = threadIdx.x; i < nw; i += NT) out[i] = 0;
        }
        return;
    }
    load_game<NT>(p, L, g);
    const Grid gd{p.W, p.H, HW};
    const int res0 = L.sc[SC_RES0], res1 = L.sc[SC_RES1];
    uint32_t* mw = L.outw;
    for (int c = threadIdx.x; c < HW; c += NT) {
        for (int v = 0; v < G.nviews; v++) {
            uint32_t m[3];
            cell_mask(gd, c, v, L.unit, L.act, L.wall, v == 0 ? res0 : res1, m);
            mw[MASK_PACKED_WORDS * (v * HW + c)] = m[0];
            mw[MASK_PACKED_WORDS * (v * HW + c) + 1] = m[1];
            mw[MASK_PACKED_WORDS * (v * HW + c) + 2] = m[2] & MASK_PACKED_W2;
        }
    }
    __syncthreads();
    if (al16) {
        const v4i* m4 = reinterpret_cast<const v4i*>(mw);
        for (int k = threadIdx.x; k < nw / 4; k += NT) *reinterpret_cast<v4i*>(out + 4 * k) = m4[k];
        for (int i = 4 * (nw / 4) + threadIdx.x; i < nw; i += NT) out[i] = (int32_t)mw[i];
    } else {
        for (int i = threadIdx.x; i < nw; i += NT) out[i] = (int32_t)mw[i];
    }
}

// ---------------------------------------------------------------------------
// Outputs kernel: the obs (and, when bound, the next-tick masks) of every game's
// stored state, unchanged -- after an env-state checkpoint is restored
// (mrts_load_state).  Parked games read zero.
template <int NT, int P, typename OT>
__global__ __launch_bounds__(NT) void k_outputs(EngineParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MRTS_STAMP_NONE();
    Lds L = carve(smem, p.HW, p.W, NT);
    const int g = blockIdx.x;
    if (game_parked(p, g)) {
        zero_outputs<NT, P, OT>(p, game_of(p, g));
        return;
    }
    load_game<NT>(p, L, g);
    emit_outputs<NT, P, OT>(p, L, game_of(p, g), true, p.mask != nullptr, L.sc[SC_RES0], L.sc[SC_RES1]);
}

// ---------------------------------------------------------------------------
// Step kernel: JNIGridnetVecClient.gameStep for one game per workgroup.
enum : uint32_t { CAND = 1u << 31, LEGAL = 1u << 30 };
__device__ __forceinline__ int unchecked_pos(const Grid& gd, int c, int dir) {   // UnitAction.resourceUsage position
    const int off[4] = {-gd.W, 1, gd.W, -1};
    return c + off[dir];
}

__device__ __forceinline__ int res_of(const Lds& L, int player) { return L.sc[SC_RES0 + player]; }

// Step (2a)'s target-position claims of a move / produce row: bit b of claim[0..posw)
// when >= 1 row targets position b (x + y * W + W, unchecked), of claim[posw..) when >= 2.
__device__ __forceinline__ void claim_target(const Lds& L, const Grid& gd, int c, int code, int posw) {
    const int ty = code_type(code);
    if (ty != A_MOVE && ty != A_PRODUCE) return;
    const int b = unchecked_pos(gd, c, code_param(code)) + gd.W;
    const uint32_t bit = 1u << (b & 31);
    if (atomicOr(&L.claim[b >> 5], bit) & bit) atomicOr(&L.claim[posw + (b >> 5)], bit);
}

// PlayerAction.fromVectorAction consistency filter + GameState.issueSafe/issue
// for one player's PlayerAction (lane 0 only).  Entries are list[0..n) in
// PlayerAction order with their codes in L.aux: the agent's rows (ascending
// cells, `vector` = true: the fromVectorAction consistency filter applies and
// the LinkedHashMap rank is the cell) or a device bot's PlayerAction (already
// consistent, rank = position in the list).
__device__ __forceinline__ void issue_player(const EngineParams& p, const Lds& L, const Grid& gd, int q, const int32_t* list, int n,
                             bool vector) {
    const int time = L.sc[SC_TIME];
    // --- fromVectorAction: ResourceUsage.consistentWith(pa.ru) ----------------
    const int nposw = pos_words_live(gd.HW, gd.W);
    for (int i = 0; i < nposw; i++) L.posbits[i] = 0;
    int pa_cost = 0;
    for (int i = 0; vector && i < n; i++) {
        int c = list[i];
        uint32_t nw = L.aux[c];
        if (u_owner(L.unit[c]) != q) continue;
        int code = (int)(nw & 0xFFFu), type = code_type(code);
        if (type != A_MOVE && type != A_PRODUCE) continue;
        const int off[4] = {-gd.W, 1, gd.W, -1};
        int pos = c + off[code_param(code)];   // unchecked, as x + y*W + offset
        int cost = type == A_PRODUCE ? ut_cost(code_utype(code)) : 0;
        int bi = pos + gd.W;
        bool taken = (L.posbits[bi >> 5] >> (bi & 31)) & 1u;
        int s = cost + pa_cost;
        if (taken || (s > 0 && s > res_of(L, q))) {
            L.aux[c] = nw & ~CAND;   // dropped: gets fillWithNones
            continue;
        }
        L.posbits[bi >> 5] |= 1u << (bi & 31);
        pa_cost += cost;
    }
    // --- issueSafe + issue -----------------------------------------------------
    int* rw = L.sc + SC_R0 + 6 * q;
    for (int i = 0; i < n; i++) {
        int c = list[i];
        uint32_t nw = L.aux[c];
        if (u_owner(L.unit[c]) != q || !(nw & CAND)) continue;
        const int ut = u_type(L.unit[c]);
        int code = (int)(nw & 0xFFFu);
        // issueSafe: illegal -> NONE with the same ETA
        int cur = code, cur_dur = 1;   // cur_dur: duration when cur is NONE (a NONE code's param)
        if (code_type(code) == A_NONE) cur_dur = code_param(code);
        else if (!(nw & LEGAL)) { cur_dur = eta_code(code, ut); cur = A_NONE; }
        int te = cur;                  // the action the TraceEntry records
        const int ctype = code_type(cur);
        int pos = -1, cost_new = 0;
        if (ctype == A_MOVE || ctype == A_PRODUCE) pos = nb_cell(gd, c, code_param(cur));
        if (ctype == A_PRODUCE) cost_new = ut_cost(code_utype(cur));
        // uaa's inconsistent with the new ResourceUsage (the holder of the target
        // position, pending produces over a player's budget), visited in
        // LinkedHashMap order: each pass takes the candidate of least issue
        // sequence above the last one visited -- any number of candidates, no
        // buffer.  Visiting a candidate rewrites only its own action, and every
        // candidate is tested against its action before the visit, as in issue().
        const int nprod = L.sc[SC_NPROD];
        const int rc = (pos >= 0) ? L.resv[pos] : -1;
        bool original = true;
        uint32_t last = 0;
        for (bool first = true;; first = false) {
            int cc = -1;
            uint32_t best = 0xFFFFFFFFu;
            if (rc >= 0 && (first || L.seq[rc] > last) && L.seq[rc] < best) { cc = rc; best = L.seq[rc]; }
            for (int k = 0; k < nprod; k++) {
                const int pc = L.prod[k];
                const uint32_t sq = L.seq[pc];
                if (pc == rc || (!first && sq <= last) || sq >= best) continue;
                const uint32_t pa = L.act[pc];
                if (pa == 0 || code_type(act_code(pa)) != A_PRODUCE) continue;
                const int pp = u_owner(L.unit[pc]), cp = ut_cost(code_utype(act_code(pa)));
                bool bad = false;
                for (int pl = 0; pl < 2; pl++) {
                    const int s = (pp == pl ? cp : 0) + (q == pl ? cost_new : 0);
                    if (s > 0 && s > res_of(L, pl)) bad = true;
                }
                if (bad) { cc = pc; best = sq; }
            }
            if (cc < 0) break;
            last = best;
            uint32_t ua = L.act[cc];
            if (seq_time(L.seq[cc]) == time) {    // CANCEL_BOTH
                int ucode = act_code(ua);
                int d1 = eta_code(ucode, u_type(L.unit[cc]));
                int d2 = code_type(cur) == A_NONE ? cur_dur : eta_code(cur, ut);
                int d = min(d1, d2);
                int utp = code_type(ucode);
                if (utp == A_MOVE || utp == A_PRODUCE) {
                    int rp = nb_cell(gd, cc, code_param(ucode));
                    if (rp >= 0 && L.resv[rp] == cc) L.resv[rp] = -1;
                }
                L.act[cc] = act_make(A_NONE, time + d);
                cur = A_NONE;
                cur_dur = d;
                original = false;
            } else {                               // "Inconsistent actions were executed!"
                cur = A_NONE;
                cur_dur = -1;
                if (original) te = A_NONE;
            }
        }
        const int ft = code_type(cur);
        const int done = ft == A_NONE ? time + cur_dur : time + eta_code(cur, ut);
        L.act[c] = act_make(cur, done);
        L.seq[c] = seq_make(time, q, vector ? c : i);
        if (ft == A_MOVE || ft == A_PRODUCE) {
            L.resv[nb_cell(gd, c, code_param(cur))] = c;
            if (ft == A_PRODUCE) L.prod[L.sc[SC_NPROD]++] = c;
        }
        // ai.reward.* on the TraceEntry actions
        const int tt = code_type(te);
        if (tt == A_HARVEST || tt == A_RETURN) rw[1]++;
        if (tt == A_PRODUCE) {
            int pu = code_utype(te);
            if (pu == WORKER) rw[2]++;
            else if (pu == BASE || pu == BARRACKS) rw[3]++;
            else if (pu >= LIGHT) rw[5]++;
        }
        if (tt == A_ATTACK) rw[4]++;
    }
}

// UnitAction.execute for one ready assignment, from its snapshot.  Serial
// (lane 0, issue order) or, for an independent ready set, one lane per action
// (PAR: resource / error updates are atomic, the produced unit's id is given).
template <bool PAR = false>
__device__ __forceinline__ void execute_one(const Lds& L, const Grid& gd, int4 s, int produced_uid = -1) {
    const int c = s.x;
    const uint32_t u = (uint32_t)s.y;
    const int code = (int)(s.z);
    const int uid = s.w;
    const int t = u_type(u), owner = u_owner(u);
    const bool here = L.unit[c] != 0 && L.uid[c] == uid;   // not killed earlier this cycle
    const int type = code_type(code), param = code_param(code);
    switch (type) {
    case A_MOVE: {
        if (!here) break;
        int n = nb_cell(gd, c, param);
        if (n < 0 || L.unit[n] != 0) {
            if (PAR) atomicOr(&L.sc[SC_ERR], MRTS_ERR_MOVE_OCCUPIED);
            else L.sc[SC_ERR] |= MRTS_ERR_MOVE_OCCUPIED;
            break;
        }
        L.unit[n] = L.unit[c];
        L.uid[n] = uid;
        L.act[n] = 0;
        L.seq[n] = 0;
        L.unit[c] = 0;
        L.uid[c] = 0;
        L.act[c] = 0;
        L.seq[c] = 0;
        break;
    }
    case A_ATTACK: {
        int dx = param % MRTS_ATTACK_GRID - MRTS_ATTACK_GRID / 2, dy = param / MRTS_ATTACK_GRID - MRTS_ATTACK_GRID / 2;
        int x = c % gd.W + dx, y = c / gd.W + dy;
        if (x < 0 || y < 0 || x >= gd.W || y >= gd.H) break;
        int n = y * gd.W + x;
        uint32_t o = L.unit[n];
        if (o == 0) break;
        int hp = u_hp(o) - ut_damage(t);   // VERSION_ORIGINAL: min == max damage
        if (hp <= 0) {                     // GameState.removeUnit (+ its assignment)
            const int vo = u_owner(o);
            if (vo == 0 || vo == 1) {      // the players' unit counts (k_step's SC_HAS)
                if (PAR) atomicSub(&L.sc[SC_HAS], vo ? 1 << 16 : 1);
                else L.sc[SC_HAS] -= vo ? 1 << 16 : 1;
            }
            L.unit[n] = 0;
            L.uid[n] = 0;
            L.act[n] = 0;
            L.seq[n] = 0;
        } else {
            L.unit[n] = u_with_hp(o, hp);
        }
        break;
    }
    case A_HARVEST: {
        int n = nb_cell(gd, c, param);
        if (n < 0) break;
        uint32_t o = L.unit[n];
        if (o == 0 || u_type(o) != RESOURCE || !ut_can_harvest(t) || u_res(u) != 0) break;
        int left = u_res(o) - ut_harvest_amount(t);
        if (left <= 0) {
            L.unit[n] = 0;
            L.uid[n] = 0;
            L.act[n] = 0;
            L.seq[n] = 0;
        } else {
            L.unit[n] = u_with_res(o, left);
        }
        if (here) L.unit[c] = u_with_res(L.unit[c], ut_harvest_amount(t));
        break;
    }
    case A_RETURN: {
        int n = nb_cell(gd, c, param);
        if (n < 0) break;
        uint32_t o = L.unit[n];
        if (o == 0 || !ut_is_stockpile(u_type(o)) || u_res(u) <= 0) break;
        if (PAR) atomicAdd(&L.sc[SC_RES0 + owner], u_res(u));
        else L.sc[SC_RES0 + owner] += u_res(u);
        if (here) L.unit[c] = u_with_res(L.unit[c], 0);
        break;
    }
    case A_PRODUCE: {
        int n = nb_cell(gd, c, param);
        int put = code_utype(code);
        if (n < 0 || L.unit[n] != 0) {
            if (PAR) atomicOr(&L.sc[SC_ERR], MRTS_ERR_PRODUCE_OCCUPIED);
            else L.sc[SC_ERR] |= MRTS_ERR_PRODUCE_OCCUPIED;
            break;
        }
        L.unit[n] = u_make(put, owner, ut_hp(put), 0);
        L.uid[n] = PAR ? produced_uid : L.sc[SC_UID]++;
        if (owner == 0 || owner == 1) {
            if (PAR) atomicAdd(&L.sc[SC_HAS], owner ? 1 << 16 : 1);
            else L.sc[SC_HAS] += owner ? 1 << 16 : 1;
        }
        L.act[n] = 0;
        L.seq[n] = 0;
        if (PAR) atomicSub(&L.sc[SC_RES0 + owner], ut_cost(put));
        else L.sc[SC_RES0 + owner] -= ut_cost(put);
        break;
    }
    default: break;
    }
}

// Wider maps (NT < HW <= 4 NT, e.g. 24x24 and 32x32 on 256 lanes): the lane's
// cells, their source-unit words and the terrain in registers, all issued in one
// round trip with genv (the unprefetched path takes four: genv, cells, then the
// sources and the actions inside the decode); the source words reach the decode
// through L.aux.
struct WidePf {
    int4 cell[4];
    int src[4];   // bit v: the source-unit word of view v
    int wall[4];
    int genv, map;
    int bpa0, bpa1;   // bot games: entry `lane` of the bot PlayerActions (player 0 / 1)
};
template <int NT>
__device__ __forceinline__ void prefetch_wide(const EngineParams& p, const Game& G, int g, WidePf& pf) {
    const int HW = p.HW;
    pf.genv = p.genv[(size_t)g * MRTS_GENV_WORDS + min((int)threadIdx.x, MRTS_GENV_WORDS - 1)];
    pf.map = p.nmaps == 1 ? 0 : p.genv[(size_t)g * MRTS_GENV_WORDS + MRTS_G_MAP];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = min((int)threadIdx.x + k * NT, HW - 1);   // unconditional: counted waits
        pf.cell[k] = p.cells[(size_t)g * p.cstride + c];
        const int s0 = p.src[(size_t)G.env0 * HW + c], s1 = p.src[(size_t)(G.env0 + G.nviews - 1) * HW + c];
        pf.src[k] = (s0 ? 1 : 0) | (s1 ? 2 : 0);
        if (p.nmaps == 1) pf.wall[k] = p.map_wall[c];
    }
    if (!G.selfplay && p.botpa) {   // speculative: the counts arrive with genv
        const int32_t* bp = p.botpa + (size_t)(g - p.nsp_games) * 2 * HW;
        pf.bpa0 = p.bot_ai0 ? bp[threadIdx.x] : 0;
        pf.bpa1 = bp[HW + threadIdx.x];
    }
}
template <int NT>
__device__ __forceinline__ void commit_wide(const EngineParams& p, const Lds& L, const WidePf& pf) {
    if (threadIdx.x < MRTS_GENV_WORDS) L.sc[threadIdx.x] = pf.genv;
    const int HW = p.HW;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = (int)threadIdx.x + k * NT;
        if (c >= HW) break;
        L.unit[c] = (uint32_t)pf.cell[k].x;
        L.uid[c] = pf.cell[k].y;
        L.act[c] = (uint32_t)pf.cell[k].z;
        L.seq[c] = (uint32_t)pf.cell[k].w;
        L.wall[c] = p.nmaps == 1 ? (uint8_t)pf.wall[k] : p.map_wall[(size_t)pf.map * HW + c];
        L.resv[c] = -1;
        L.aux[c] = (uint32_t)pf.src[k];   // read back by the decode on this lane
    }
    __syncthreads();
}

// Register prefetch of a game's state (maps with HW <= NT: one cell per lane):
// issued before the current game's output stream, so the next game's state
// round trip overlaps those stores instead of stalling the block.
struct StatePf {
    int4 cell;
    int genv, src0, src1;
    int bpa0, bpa1;   // bot games: entry `lane` of the bot PlayerActions (player 0 / 1)
    int4 aa, aa2;     // bot-fused games, lanes < 64: words lane, lane + 64 of the bot's abstract actions
    int wall;         // single-map batches: this cell's terrain
    int map;          // the game's map (genv[MRTS_G_MAP], every lane: no barrier before the terrain load)
};
// the bot wave's first abstract-action words: lane, lane + 64 of the game's 2 * HW (clamped: small maps)
__device__ __forceinline__ void prefetch_aa(const EngineParams& p, int g, StatePf& pf) {
    const int4* aa = p.aa + ((size_t)(g - p.nsp_games) * 2 + 1) * p.HW * 2;
    pf.aa = aa[min((int)threadIdx.x, 2 * p.HW - 1)];
    pf.aa2 = aa[min(64 + (int)threadIdx.x, 2 * p.HW - 1)];
}
template <int NT, bool FB>
__device__ __forceinline__ void prefetch_game(const EngineParams& p, int g, StatePf& pf) {
    const Game G = game_of(p, g);
    const int HW = p.HW, c = min((int)threadIdx.x, HW - 1);   // unconditional: counted waits
    pf.cell = p.cells[(size_t)g * p.cstride + c];
    pf.src0 = p.src[(size_t)G.env0 * HW + c];
    pf.src1 = p.src[(size_t)(G.env0 + G.nviews - 1) * HW + c];
    pf.genv = p.genv[(size_t)g * MRTS_GENV_WORDS + min((int)threadIdx.x, MRTS_GENV_WORDS - 1)];
    if (!G.selfplay && p.botpa) {   // speculative: the counts arrive with genv
        const int32_t* bp = p.botpa + (size_t)(g - p.nsp_games) * 2 * HW;
        pf.bpa0 = p.bot_ai0 ? bp[c] : 0;   // player 0 bots: MicroRTSBotVecEnv only
        pf.bpa1 = bp[HW + c];
        if (FB && threadIdx.x < 64) prefetch_aa(p, g, pf);
    }
    if (p.nmaps == 1) pf.wall = p.map_wall[c];   // else the game's map is known only with genv
    else pf.map = p.genv[(size_t)g * MRTS_GENV_WORDS + MRTS_G_MAP];
}
template <int NT>
__device__ __forceinline__ void commit_game(const EngineParams& p, const Lds& L, const StatePf& pf) {
    if (threadIdx.x < MRTS_GENV_WORDS) L.sc[threadIdx.x] = pf.genv;
    const int HW = p.HW;
    if ((int)threadIdx.x < HW) {
        const int c = threadIdx.x;
        L.unit[c] = (uint32_t)pf.cell.x;
        L.uid[c] = pf.cell.y;
        L.act[c] = (uint32_t)pf.cell.z;
        L.seq[c] = (uint32_t)pf.cell.w;
        L.wall[c] = p.nmaps == 1 ? (uint8_t)pf.wall : p.map_wall[(size_t)pf.map * HW + c];
        L.resv[c] = -1;   // reservation holders (step 1)
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------
// The tick behind the decode, phase by phase (step_game below holds the load and the decode, then the list).
// Barriers: each phase is ordered after the last one that wrote what it reads from OTHER lanes; a phase that
// reads only its own lane's cells (the same c = threadIdx.x + k * NT walk) follows its predecessor without
// one.  Each phase's header says what it reads from other lanes, what it writes, which barrier it relies on
// and whether it ends with one.

// What the phases share.  Passed by reference; it dissolves when the phases are inlined.
struct Tick {
    const EngineParams& p;
    const Lds& L;
    const Grid gd;   // (gd.HW is the HW that full_hw made a constant at the kernel's start)
    const int g;
    Game G;
    int posw;        // words of one half of L.claim (pos_words)
    int time;        // of the loaded state
    bool bot0;       // bot-vs-bot game (MicroRTSBotVecEnv): player 0's PlayerAction comes from k_bot too
    int npa, npa0;   // entries of the device bots' PlayerActions (player 1 / player 0)
};
// What a lane keeps of its own cells from one phase to a later one.
constexpr int OKEY_PER_REG = 32 / OBS_KEY_BITS;
struct LaneRec {
    int4 aa, aa2;     // carried for write_back only: the bot wave's prefetched abstract-action words (StatePf::aa)
    // delta masks: bit 2 k + v = this lane's k-th cell was a source row of view v in the loaded state
    // (cell_mask's first test), i.e. the bound mask buffer holds a row there (mrts_capi.cpp delta_ok)
    uint32_t was_src;
    // delta obs: the keys (obs_key) of this lane's cells in the loaded state -- of what the obs buffer holds
    // (at most MRTS_OBS_DELTA_CELLS cells per lane: mrts_capi.cpp obs_delta_ok)
    uint32_t okey[MRTS_OBS_DELTA_CELLS / OKEY_PER_REG];
};

// delta obs: each lane leaves its cells' old keys where phase A writes the new one-hot words (L.outw)
template <int NT>
__device__ __forceinline__ void old_keys(const Tick& S, const LaneRec& R) {
    constexpr int KB = OBS_KEY_BITS, KPR = OKEY_PER_REG;
#pragma unroll
    for (int k = 0; k < MRTS_OBS_DELTA_CELLS; k++) {
        const int c = (int)threadIdx.x + k * NT;
        if (c < S.gd.HW) S.L.outw[c] = (R.okey[k / KPR] >> (k % KPR * KB)) & ((1u << KB) - 1u);
    }
}

// (2a) Rows that interact with nothing else this tick issue lane-parallel: a row (agent or device bot) whose
// target position, if a move or produce, no other row (either player) and no pending assignment claims, while
// no pending produce is over its owner's budget (`over`, which would make every new action inconsistent); a
// produce besides only while all of its player's produce rows this tick together with the player's dearest
// pending produce fit the player's resources (SC_PSUM + SC_PMAX): then no prefix of the PlayerAction's
// ResourceUsage exceeds them (fromVectorAction keeps it and every later row) and no pair of produces is over
// budget (issue() finds no candidate for it, nor does any later row find it).  Such a row meets no candidate in
// issue() and no other row in fromVectorAction's filter, and no ordered row of either player meets it, so
// issuing it out of order is exact: its LinkedHashMap rank is still its cell (agent rows) or its position in
// the bot's PlayerAction.  (A parallel produce is never a candidate of an ordered row, so it stays out of
// L.prod.)  Everything else takes the ordered path (2b).
// Reads from other lanes: L.claim, L.resv at the row's target, SC_PSUM / SC_PMAX, the resources.  Writes: its
// own cells' act / seq / aux, L.resv at a target only this row claims, the reward counters (atomics), SC_NLEFT.
// Relies on the decode's barrier.  Ends with one: these issues come before the ordered part.
template <int NT>
__device__ __forceinline__ void issue_parallel(const Tick& S, bool over) {
    const EngineParams& p = S.p;
    const Lds& L = S.L;
    const Grid& gd = S.gd;
    if (!over) {
        int left = 0;   // this lane's rows left to (2b)
        for (int c = threadIdx.x; c < gd.HW; c += NT) {
            const uint32_t nw = L.aux[c];
            if (!(nw & CAND)) continue;
            const uint32_t u = L.unit[c];
            const int q = u_owner(u);
            const bool botrow = !S.G.selfplay && (q != 0 || S.bot0);
            const int rank = botrow ? (int)((nw >> 12) & 0xFFFu) : c;
            const int code = (int)(nw & 0xFFFu), ty = code_type(code);
            if (ty == A_PRODUCE && L.sc[SC_PSUM + q] + L.sc[SC_PMAX + q] > res_of(L, q)) { left++; continue; }
            int n = -1;
            if (ty == A_MOVE || ty == A_PRODUCE) {
                const int b = unchecked_pos(gd, c, code_param(code)) + p.W;
                n = nb_cell(gd, c, code_param(code));
                if (((L.claim[S.posw + (b >> 5)] >> (b & 31)) & 1u) || (n >= 0 && L.resv[n] >= 0)) { left++; continue; }
            }
            int cur = code, dur = 0;
            if (ty == A_NONE) dur = code_param(code);
            else if (!(nw & LEGAL)) { dur = eta_code(code, u_type(u)); cur = code_make(A_NONE, 0, 0); }
            const int ct = code_type(cur);
            L.act[c] = act_make(cur, ct == A_NONE ? S.time + dur : S.time + eta_code(cur, u_type(u)));
            L.seq[c] = seq_make(S.time, q, rank);
            if (ct == A_MOVE || ct == A_PRODUCE) L.resv[n] = c;
            if (ct == A_HARVEST || ct == A_RETURN) atomicAdd(&L.sc[SC_R0 + 6 * q + 1], 1);
            if (ct == A_ATTACK) atomicAdd(&L.sc[SC_R0 + 6 * q + 4], 1);
            if (ct == A_PRODUCE) {   // ai.reward.ProduceWorker / ProduceBuilding / ProduceCombatUnit
                const int pu = code_utype(cur);
                atomicAdd(&L.sc[SC_R0 + 6 * q + (pu == WORKER ? 2 : (pu == BASE || pu == BARRACKS) ? 3 : 5)], 1);
            }
            L.aux[c] = nw & ~CAND;   // issued
        }
        if (left) atomicAdd(&L.sc[SC_NLEFT], left);
    }
    __syncthreads();
}

// (2b) The ordered path for the rest, p0 then p1 (bot envs: the passive bot issues only NONEs), on lane 0:
// the rows are listed (an ordered compaction, the ranks of agent rows being their cells) only when (2a) left
// any -- most ticks it leaves none.  Returns the rows listed.
// Reads from other lanes: L.aux of every cell (the compaction); lane 0 reads the whole state.  Writes:
// L.list, L.ballot; lane 0: act / seq / resv / prod / posbits / aux, SC_NPROD, the reward counters.
// Relies on (2a)'s barrier.  Ends with one.
template <int NT>
__device__ __forceinline__ int issue_ordered(const Tick& S, bool over, int nprod) {
    const EngineParams& p = S.p;
    const Lds& L = S.L;
    int nrows = 0;
    if (over || L.sc[SC_NLEFT]) nrows = compact_cells<NT>(S.gd.HW, [&](int c) { return (L.aux[c] & CAND) != 0; }, L.list, L.ballot);
    MRTS_STAMP(4, threadIdx.x == 0);
    if (threadIdx.x == 0) {
        L.sc[SC_NPROD] = nprod;
        if (S.bot0) issue_player(p, L, S.gd, 0, L.blist0, S.npa0, false);
        else issue_player(p, L, S.gd, 0, L.list, nrows, true);
        if (S.G.selfplay) issue_player(p, L, S.gd, 1, L.list, nrows, true);
        else if (S.npa > 0) issue_player(p, L, S.gd, 1, L.blist, S.npa, false);
    }
    __syncthreads();
    MRTS_STAMP(5, threadIdx.x == 0);
    return nrows;
}

// (3) fillWithNones(gs, player, 1) for every idle unit (both players), then (4) GameState.cycle(): time++,
// the ready assignments collected, ranked into issue order and executed -- serially on lane 0, or one lane
// per action when the set commutes.  `nrows` goes to the rollout statistics.
// Reads from other lanes: L.list / L.aux (the ready set's cells and sequence words), L.snap, the cells the
// actions touch.  Writes: act / seq of its own cells, claim[0, posw) (dead since the decode's claims:
// cleared here for the ready set's harvest-pile check), L.list / L.aux / L.snap, the cells the executed
// actions touch, the scalars (SC_NREADY / RPROD / SERIAL / UID / HAS / TIME / TICKS / ERR, resources).
// Relies on (2b)'s barrier; its first passes read each cell on the lane that wrote it.  Two barriers
// inside (ready set listed; ranked).  Ends with one.
template <int NT>
__device__ __forceinline__ void cycle(const Tick& S, int nrows) {
    const Lds& L = S.L;
    const Grid& gd = S.gd;
    const int HW = gd.HW, time = S.time;
    for (int i = threadIdx.x; i < S.posw; i += NT) L.claim[i] = 0;
    for (int c = threadIdx.x; c < HW; c += NT) {
        uint32_t u = L.unit[c];
        if (u != 0 && u_owner(u) >= 0 && L.act[c] == 0) {
            L.act[c] = act_make(A_NONE, time + 1);
            L.seq[c] = seq_make(time, u_owner(u), 4095);
        }
    }
    const int now = time + 1;
    for (int c = threadIdx.x; c < HW; c += NT) {
        uint32_t a = L.act[c];
        if (a && act_done(a) <= now && code_type(act_code(a)) == A_NONE) L.act[c] = 0;
    }
    // the ready cells in L.list, their sequence words in L.aux (dead since the issue),
    // appended in any order: they are ranked by sequence word below
    for (int c = threadIdx.x; c < HW; c += NT) {
        const uint32_t a = L.act[c];
        if (a != 0 && act_done(a) <= now) {
            const int pos = atomicAdd(&L.sc[SC_NREADY], 1);
            L.list[pos] = c;
            L.aux[pos] = L.seq[c];
        }
    }
    __syncthreads();
    const int nready = L.sc[SC_NREADY];
    // snapshots of the ready assignments in LinkedHashMap (issue-sequence)
    // order: lane-parallel rank by sequence word (unique among non-NONE actions);
    // in the same pass, unitActions.remove and whether the set commutes:
    // independent ready sets (no attack, no two harvests of one pile) do -- every
    // target cell is distinct (moves / produces hold reservations), resources only
    // add up, and produced units take ids in issue order.  (Attacks on cells no
    // other ready action touches would commute too; run in parallel that way they
    // measured neutral at 1024 and slower at 8192 envs: DESIGN.md §5.)
    int serial = 0, nprodr = 0;
    for (int i = threadIdx.x; i < nready; i += NT) {
        const int c = L.list[i];
        const uint32_t sq = L.aux[i];
        int rank = 0, j = 0;
        for (; j + 4 <= nready; j += 4) {   // four sequence words per LDS read, no pointer chase
            const uint4 v = *reinterpret_cast<const uint4*>(L.aux + j);
            rank += (v.x < sq) + (v.y < sq) + (v.z < sq) + (v.w < sq);
        }
        for (; j < nready; j++) rank += L.aux[j] < sq;
        const int code = act_code(L.act[c]), ty = code_type(code);
        L.snap[rank] = make_int4(c, (int)L.unit[c], code, L.uid[c]);
        L.act[c] = 0;   // unitActions.remove (each ready cell is read by its own lane only)
        if (ty == A_ATTACK) serial = 1;
        nprodr += ty == A_PRODUCE;
        if (ty == A_HARVEST) {
            const int n = nb_cell(gd, c, code_param(code));
            if (n >= 0 && (atomicOr(&L.claim[n >> 5], 1u << (n & 31)) >> (n & 31)) & 1u) serial = 1;
        }
    }
    if (nprodr) atomicAdd(&L.sc[SC_RPROD], nprodr);   // the ids the produced units take (SC_RPROD starts at 0)
    const int uid0 = L.sc[SC_UID];   // read before lane 0 may advance it (below)
    // (the OR over lanes through an LDS word: __syncthreads_or's static LDS would cost
    // every workgroup 256 B)
    if (serial) L.sc[SC_SERIAL] = 1;
    __syncthreads();
    serial = L.sc[SC_SERIAL];
    MRTS_STAMP(6, threadIdx.x == 0);
    if (serial) {
        if (threadIdx.x == 0)
            for (int i = 0; i < nready; i++) execute_one(L, gd, L.snap[i]);
    } else {
        for (int i = threadIdx.x; i < nready; i += NT) {
            const int4 sn = L.snap[i];
            int puid = -1;
            if (code_type(sn.z) == A_PRODUCE) {
                puid = uid0;
                for (int j = 0; j < i; j++) puid += code_type(L.snap[j].z) == A_PRODUCE;
            }
            execute_one<true>(L, gd, sn, puid);
        }
    }
    // (no barrier: the scalars below are lane 0's, SC_UID is no longer read, and the
    // unit counts -- kept by execute_one -- are read behind the next barrier)
    if (threadIdx.x == 0) {
        L.sc[SC_TIME] = now;
        L.sc[SC_TICKS]++;
        L.sc[MRTS_G_SERIAL] += serial;      // rollout statistics (mrts_game_stats)
        L.sc[MRTS_G_ORDERED] += nrows;
        if (now >= MRTS_MAX_TIME) atomicOr(&L.sc[SC_ERR], MRTS_ERR_TIME_OVERFLOW);   // the executing lanes may be ORing too
        if (!serial)
            L.sc[SC_UID] += L.sc[SC_RPROD];
    }
    __syncthreads();
}

// (5) PhysicalGameState.gameover / winner: the unit counts of the decode pass, less the units attacks
// removed, plus the produced ones (execute_one); (6) rewards / done (JNIGridnetVecClient.gameStep terminal
// handling) and the auto-reset.  steps0 / map_now: the loaded state's, read before any lane could rewrite them.
// Reads from other lanes: SC_HAS and the reward counters.  Writes: the reward / done outputs; on a reset
// its own cells and lane 0's scalars, else SC_STEPS.  Relies on the cycle's barrier; no barrier between the
// rewards and the reset (the rewards read only SC_R0.. words, which the reset leaves alone, and nothing
// here reads the cell arrays it rewrites).  Ends with one.
template <int NT, bool FULL>
__device__ __forceinline__ void finish_tick(const Tick& S, int steps0, int map_now) {
    const EngineParams& p = S.p;
    const Lds& L = S.L;
    const Game& G = S.G;
    const int has = L.sc[SC_HAS];
    const bool has0 = (has & 0xFFFF) != 0, has1 = (has >> 16) != 0;
    const bool gameover = !(has0 && has1);
    const int winner = (has0 && !has1) ? 0 : (has1 && !has0) ? 1 : -1;
    const int steps = steps0 + 1;
    const bool reset = gameover || steps >= p.max_steps;
    if (threadIdx.x < 6 * G.nviews) {
        int v = threadIdx.x / 6, k = threadIdx.x % 6;
        int env = G.env0 + v;
        double r = k == 0 ? (gameover ? (winner == v ? 1.0 : -1.0) : 0.0) : (double)L.sc[SC_R0 + 6 * v + k];
        p.raw_reward[(size_t)env * 6 + k] = r;
        p.done[(size_t)env * 6 + k] = (uint8_t)((gameover || (k == 0 && reset)) ? 1 : 0);
    }
    if (p.reward && threadIdx.x < G.nviews) {   // fused `reward @ reward_weight`, done[:, 0]
        const int v = threadIdx.x, env = G.env0 + v;
        double s = 0.0;
        for (int k = 0; k < 6; k++) {
            double r = k == 0 ? (gameover ? (winner == v ? 1.0 : -1.0) : 0.0) : (p.shaping ? (double)L.sc[SC_R0 + 6 * v + k] : 0.0);
            s = __dadd_rn(s, __dmul_rn(r, p.rw[k]));   // no FMA contraction: numpy's sequential dot
        }
        p.reward[env] = s;
        p.done0[env] = (uint8_t)(reset ? 1 : 0);
    }
    full_hw<FULL, NT>(p);
    if (reset) {
        reset_into_lds<NT>(p, L, map_now);
        if (threadIdx.x == 0) {
            L.sc[SC_AA_N] = L.sc[MRTS_G_AA_N0] = 0;   // ai1 / ai2.reset()
            L.sc[MRTS_G_EPISODES]++;
        }
    } else if (threadIdx.x == 0) {
        L.sc[SC_STEPS] = steps;
    }
    __syncthreads();
}

// (7) Write back, the delta marks, and all outputs: the one-hot observation of every view + getMasks of the
// next tick (bound mask outputs: every read of this game's source rows is behind the barriers above); in
// a bot-fused game wave 0 then runs the next tick's bot.
// Early bot (P == 29, p.early_bot: full observability, and for this size the bot writes none of the arrays
// phase A reads -- unit / act / wall stay as stored, the step's scalars and visibility words are left alone,
// its small arrays go to the tail region): once store_game has read the arrays the bot reuses, the workgroup
// builds the bot's setup, then wave 0 starts the next tick's bot at once while waves 1.. build the output
// words and stream them, meeting at an LDS counter instead of a workgroup barrier.  Otherwise wave 0 helps
// with phase A and starts the bot behind its barrier (the step's arrays are dead by then: only L.outw is read
// on).  One bot_game call site for both: the inlined bot is most of this kernel's code.
// Delta masks: the rows the bound buffer holds from the last tick (the loaded state's source rows, R.was_src)
// are marked in the mask words' region -- dead scratch lists, or a bot game's own region -- by the lane that
// met the cell in the decode; phase A reads the mark back on the same lane, or, on the early path, behind the
// barriers below.  Delta obs: old_keys, likewise.  On the early path L.outw is the uid array, which the bot's
// setup reads up to its inner barrier, and phase A runs on other lanes: the keys go in behind the setup (whose
// last loop does not touch the uid array) and ahead of the barrier that follows it.
// Reads from other lanes: the scalars (store_game, the resources); emit_outputs and the bot read the whole final
// state.  Writes: the game's global state, L.outm / L.outw marks on its own cells, then the output words'
// region (emit_outputs) and the bot's arrays.  Relies on finish_tick's barrier.  Early path: two barriers around
// the bot's setup; emit_outputs has its own.  The kernel's last phase.
template <int NT, int P, typename OT, bool FB, bool FULL>
__device__ __forceinline__ void write_back(const Tick& S, const LaneRec& R, const FusedLds& F, int odelta_w, bool botg, bool early,
                                           bool pf_ok) {
    const EngineParams& p = S.p;
    const Lds& L = S.L;
    const Game& G = S.G;
    const int g = S.g;
    MRTS_STAMP(7, threadIdx.x == 0);
    full_hw<FULL, NT>(p);
    const int HW = S.gd.HW;
    store_game<NT>(p, L, g);
    const int res0 = L.sc[SC_RES0], res1 = L.sc[SC_RES1];   // before the early bot may reuse the scalars' bytes
    const int deltas = flag_word((p.mask != nullptr && p.mask_delta != 0 ? 1 : 0) | (odelta_w ? 2 : 0));   // emit_outputs' flag word
    const bool odelta = (deltas & 2) != 0;
    if (deltas & 1)
        for (int c = threadIdx.x, k = 0; c < HW; c += NT, k++)
            for (int v = 0; v < G.nviews; v++) L.outm[3 * (v * HW + c) + 2] = ((R.was_src >> (2 * k + v)) & 1u) ? MASK_ROW_STORE : 0u;
    if (odelta && !early) old_keys<NT>(S, R);
    if (early) {
        __syncthreads();
        bot_setup_workgroup<NT>(p, F.B);
        if (odelta) old_keys<NT>(S, R);
        __syncthreads();
        MRTS_STAMP(14, threadIdx.x == 0);
    }
    if (!early || threadIdx.x >= 64)
        emit_outputs<NT, P, OT, FULL>(p, L, G, true, p.mask != nullptr, res0, res1, botg ? 64 : 0, early ? F.early_cnt : nullptr,
                                      deltas);
    if (FB && botg && threadIdx.x < 64) {
        if (early) __builtin_amdgcn_s_setprio(3);   // the latency-bound bot wave first; the streaming waves are memory-bound
        bots::bot_game<true>(p, g - p.nsp_games, 1, F.B, L.sc, pf_ok, R.aa, R.aa2, early);
        MRTS_STAMP(13, threadIdx.x == 0);
    }
}

// One game per workgroup.  A persistent variant looping over games measured slower, and still does not
// fit: hipcc allocates 153 VGPRs (3 waves / SIMD) for the looped general body and 115 (4 waves) for the
// looped full-workgroup one, against 68 and 55 for one game per workgroup (profiles/step_chain/README.md).
// FULL: HW == NT for every engine of the launch (full_hw).
// FB (bot fusion, p.fuse_bots): in a bot game's workgroup, wave 0 decides the
// NEXT tick's bot actions (bots::bot_game on the state just stored) while waves
// 1.. stream this tick's outputs; the workgroup's LDS is then the fused layout (fused_carve).
template <int NT, int P, typename OT, bool FB, bool FULL>
__device__ __forceinline__ void step_game(const EngineParams& p, const int g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    full_hw<FULL, NT>(p);
    const int HW = p.HW;
    const bool early_layout = FB && P == 29 && p.early_bot;
    const bool botg = FB && g >= p.nsp_games && NT > 64;   // the workgroup runs the next tick's bot
    const bool early = early_layout && botg;                // ... beside phase A
    const FusedLds F = FB ? fused_carve(smem, HW, p.W, NT, early_layout, botg) : FusedLds{carve(smem, HW, p.W, NT)};
    const Lds& L = F.L;
    if (FB && threadIdx.x == 0) *F.early_cnt = 0;   // read after several barriers below
    // issue priority: the game logic (latency-bound chains of LDS steps and
    // barriers) over other workgroups' output streams (memory-bound), which
    // drop to 0 in emit_outputs' phase B
    __builtin_amdgcn_s_setprio(2);
#ifdef MRTS_STAMPS
    if (threadIdx.x == 0) {   // rows by workgroup (no atomics: they would skew the start stamps);
        // maps of more than 256 cells launch apart from the others (mrts_step_group plans)
        // (no row counter: an atomic on one address by every workgroup sits in the vmcnt
        // queue ahead of the state loads and skewed the first round by ~10 us)
        mrts_stamp_row = (int)blockIdx.x + (HW > 256 ? MRTS_STAMP_ROWS / 2 : 0);
        if (mrts_stamp_row < MRTS_STAMP_ROWS) {
            g_stamp[mrts_stamp_row][0] = (unsigned long long)g | ((unsigned long long)HW << 32);
            g_stamp[mrts_stamp_row][1] = (unsigned long long)(g >= p.nsp_games) | ((unsigned long long)(FB && NT > 64) << 1) |
                                         ((unsigned long long)p.early_bot << 2);
        }
    }
    __syncthreads();
#endif
    MRTS_STAMP(2, threadIdx.x == 0);
    const Grid gd{p.W, p.H, HW};
    const bool pf_ok = HW <= NT;   // state, genv and source rows in one round trip
    const bool pf_wide = !pf_ok && HW <= 4 * NT;   // the same for up to four cells per lane
    StatePf pf;
    WidePf wpf;
    if (game_parked(p, g)) return;   // no tick: its outputs stay zero (mrts_park_games)
    if (pf_ok) prefetch_game<NT, FB>(p, g, pf);
    else if (pf_wide) prefetch_wide<NT>(p, game_of(p, g), g, wpf);
    MRTS_STAMP(15, threadIdx.x == 0);
    if (early)   // the early bot's tail arrays start zeroed
        for (int i = threadIdx.x; i < F.tail_words; i += NT) F.tail[i] = 0;
    const Game G = game_of(p, g);
    // (barriers: the paragraph above the phases)  Everything zeroed or initialised here is first read after
    // commit_game's barrier.
    if (threadIdx.x < SC_WORDS) L.sc[threadIdx.x] = 0;
    const int posw = pos_words(HW, p.W);
    for (int i = threadIdx.x; i < 2 * posw; i += NT) L.claim[i] = 0;
    // the source-unit rows of this lane's first cell, fetched in the same round
    // trip as the game state (the decode below needs both)
    int src_pre[2] = {0, 0};
    if (pf_ok) {
        src_pre[0] = pf.src0;
        src_pre[1] = pf.src1;
    } else if (!pf_wide && (int)threadIdx.x < HW) {
        for (int v = 0; v < G.nviews; v++) src_pre[v] = p.src[(size_t)(G.env0 + v) * HW + threadIdx.x];
    }
    if (pf_ok) {
        commit_game<NT>(p, L, pf);
    } else if (pf_wide) {
        commit_wide<NT>(p, L, wpf);
    } else {
        for (int c = threadIdx.x; c < HW; c += NT) L.resv[c] = -1;
        load_game<NT>(p, L, g);
    }
    MRTS_STAMP(3, threadIdx.x == 0);
    // delta obs: the keys of this lane's cells in the state just loaded (R.okey), kept until the tick is over
    LaneRec R{};
    int odelta_w = 0;   // (a flag word: flag_word)
    constexpr int KB = OBS_KEY_BITS, KPR = OKEY_PER_REG;   // bits per key, keys per register
    if constexpr (!obs_packed<OT> && obs_delta_built<P>) {
        odelta_w = flag_word(p.obs_delta);
        if (odelta_w) {
#pragma unroll
            for (int k = 0; k < MRTS_OBS_DELTA_CELLS; k++) {
                const int c = (int)threadIdx.x + k * NT;
                if (c < HW) {
                    const uint32_t u = L.unit[c], a = L.act[c];
                    const uint8_t wl = L.wall[c];
                    R.okey[k / KPR] |= obs_key(u, a, wl) << (k % KPR * KB);
                }
            }
        }
    }
    const int time = L.sc[SC_TIME];
    const int steps0 = L.sc[SC_STEPS], map_now = L.sc[SC_MAP];   // read before any lane can rewrite them (auto-reset)
    // bot-vs-bot game (MicroRTSBotVecEnv): player 0's PlayerAction comes from k_bot too
    const bool bot0 = !G.selfplay && p.bot_ai0 && p.bot_ai0[g - p.nsp_games] >= 0;

    // (1) decode the rows of every idle unit whose cell is in source_unit_mask
    //     (vec_env.py:972-974) + Unit.canExecuteAction, lane-parallel.
    // + pending move/produce reservations (ResourceUsage of unitActions) and whether
    //   a pending produce is over its owner's budget; + the target positions the
    //   agent's move / produce rows claim (step 2a)
    int units = 0;   // player 0's units + player 1's << 16 (SC_HAS)
    // (delta masks: cell_pass takes R.was_src, at most MRTS_MASK_DELTA_CELLS cells per lane: mrts_capi.cpp delta_ok)
    static_assert(2 * MRTS_MASK_DELTA_CELLS <= 32, "was_src: two bits per cell of a lane in one word");
    // per cell (the lane's k-th): unit counts, pending reservations / produce budgets;
    // returns the view whose agent row the cell's idle unit may take (-1: none)
    auto cell_pass = [&](int c, uint32_t u, int k) {
        const int ow = u_owner(u);
        if (u != 0 && (ow == 0 || ow == 1)) units += ow ? 1 << 16 : 1;
        const uint32_t pa = L.act[c];
        if (u != 0 && pa == 0 && ow >= 0 && ow < G.nviews) R.was_src |= 1u << ((2 * k + ow) & 31);
        if (pa) {
            const int code = act_code(pa), ty = code_type(code);
            if (ty == A_MOVE || ty == A_PRODUCE) {
                const int n = nb_cell(gd, c, code_param(code));
                if (n >= 0) L.resv[n] = c;
                if (ty == A_PRODUCE) {
                    const int cost = ut_cost(code_utype(code));
                    if (cost > res_of(L, u_owner(u))) L.sc[SC_OVER] = 1;
                    if (ow == 0 || ow == 1) atomicMax(&L.sc[SC_PMAX + ow], cost);
                    L.prod[atomicAdd(&L.sc[SC_NPEND], 1)] = c;   // (any order: issue() picks candidates by sequence)
                }
            }
        }
        return (u != 0 && ow >= 0 && pa == 0) ? (G.selfplay ? ow : (ow == 0 && !bot0 ? 0 : -1)) : -1;
    };
    // the agent's action row of cell c's idle unit (view v, owner ow): decode +
    // legality + the target claims; returns its aux word
    auto decode_row = [&](int c, int v, int ow) -> uint32_t {
        const size_t row = (size_t)(G.env0 + v) * HW + c;
        int64_t r[ACT_COMPONENTS];   // all 7 components in one round trip
        if (p.act_packed) {   // wave-uniform (an engine's setting): one word, the dense row it stands for (mrts_actions.h)
            const uint32_t w = (uint32_t)reinterpret_cast<const int32_t*>(p.actions)[row];
#pragma unroll
            for (int k = 0; k < ACT_COMPONENTS; k++) r[k] = act_word_get(w, k);
        } else {
            const int64_t* ra = p.actions + row * 7;
#pragma unroll
            for (int k = 0; k < ACT_COMPONENTS; k++) r[k] = ra[k];
        }
        int64_t ty = r[ACT_TYPE];
        int code = -1;
        if (ty == A_NONE) code = code_make(A_NONE, 1, 0);   // NONE(1): param = duration
        else if (ty >= A_MOVE && ty <= A_RETURN) {
            int64_t d = r[ty];   // the direction component of type ty is component ty (mrts_actions.h)
            if (d >= 0 && d < 4) code = code_make((int)ty, (int)d, 0);
        } else if (ty == A_PRODUCE) {
            int64_t d = r[ACT_PRODUCE_DIR], t2 = r[ACT_PRODUCE_TYPE];
            if (d >= 0 && d < 4 && t2 >= 0 && t2 < MRTS_NTYPES) code = code_make(A_PRODUCE, (int)d, (int)t2);
        } else if (ty == A_ATTACK) {
            int64_t a = r[ACT_ATTACK_CELL];
            if (a >= 0 && a < MRTS_ATTACK_GRID * MRTS_ATTACK_GRID) code = code_make(A_ATTACK, (int)a, 0);
        }
        if (code < 0) return 0u;
        const bool lg = legal_code(gd, c, code, L.unit, L.wall, res_of(L, ow));
        claim_target(L, gd, c, code, posw);
        if (code_type(code) == A_PRODUCE) atomicAdd(&L.sc[SC_PSUM + ow], ut_cost(code_utype(code)));
        return CAND | (lg ? LEGAL : 0u) | (uint32_t)code;
    };
    if (!pf_wide) {   // one cell per lane (maps of <= NT cells) or the unprefetched path
        for (int c = threadIdx.x, k = 0; c < HW; c += NT, k++) {
            const uint32_t u = L.unit[c];
            const int v = cell_pass(c, u, k);
            uint32_t nw = 0;
            if (v >= 0 && (c == (int)threadIdx.x ? src_pre[v] : p.src[(size_t)(G.env0 + v) * HW + c])) nw = decode_row(c, v, u_owner(u));
            L.aux[c] = nw;
        }
    } else {
        // wider maps: the rows to decode are gathered per wave first (ballots; the
        // source words came with the prefetch, in aux) and then loaded one per lane,
        // so the lane's two to four cells cost one action-row round trip, not one each.
        // The wave's list lives in the ready-set snapshots' array (4 HW words, first used
        // by the cycle): wave w takes [w K 64, (w + 1) K 64), K = cells per lane <= 4.
        const int K = (HW + NT - 1) / NT, lane = threadIdx.x & 63;
        int32_t* const wl = reinterpret_cast<int32_t*>(L.snap) + (threadIdx.x >> 6) * K * 64;
        int wn = 0;
        for (int k = 0; k < K; k++) {   // uniform trip count: every lane takes part in each ballot
            const int c = (int)threadIdx.x + k * NT;
            int e = -1;
            if (c < HW) {
                const uint32_t u = L.unit[c];
                const int v = cell_pass(c, u, k);
                if (v >= 0 && ((L.aux[c] >> v) & 1u)) e = c | (v << 16);
                L.aux[c] = 0;
            }
            const unsigned long long m = __ballot(e >= 0);
            if (e >= 0) wl[wn + __popcll(m & ((1ull << lane) - 1ull))] = e;
            wn += __popcll(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int j = lane; j < wn; j += 64) {
            const int e = wl[j], c = e & 0xFFFF, v = e >> 16;
            L.aux[c] = decode_row(c, v, u_owner(L.unit[c]));
        }
    }
    if (units) atomicAdd(&L.sc[SC_HAS], units);
    // the device bot's PlayerAction for player 1 (k_bot, computed on the state
    // before this tick's issues: JNIGridnetClient.gameStep order)
    const int npa = (!G.selfplay && p.botpa) ? L.sc[SC_NPA] : 0;
    const int npa0 = bot0 ? L.sc[MRTS_G_NPA0] : 0;
    if (npa | npa0) __syncthreads();   // the bot rows' aux words after the decode's (which zeroed them)
    // entry k of player q's PlayerAction: lane k's prefetched word (maps with HW <= NT),
    // else a load; its position in the PlayerAction (the LinkedHashMap rank) rides in aux
    for (int q = 0; q < 2; q++) {
        const int nq = q ? npa : npa0;
        for (int k = threadIdx.x; k < nq; k += NT) {
            const int e = (pf_ok && k == (int)threadIdx.x)     ? (q ? pf.bpa1 : pf.bpa0)
                          : (pf_wide && k == (int)threadIdx.x) ? (q ? wpf.bpa1 : wpf.bpa0)
                                                           : p.botpa[((size_t)(g - p.nsp_games) * 2 + q) * HW + k];
            const int c = e & 0xFFFF, code = e >> 16;
            (q ? L.blist : L.blist0)[k] = c;
            L.aux[c] = CAND | (legal_code(gd, c, code, L.unit, L.wall, res_of(L, q)) ? LEGAL : 0u) | ((uint32_t)k << 12) |
                       (uint32_t)code;
            claim_target(L, gd, c, code, posw);
            if (code_type(code) == A_PRODUCE) atomicAdd(&L.sc[SC_PSUM + q], ut_cost(code_utype(code)));
        }
    }
    // the pending produces (L.prod) were appended in the decode: issue() visits its
    // candidates by sequence word, so their order is free and no ordered compaction is
    // needed; this barrier orders the reservations, claims, SC_OVER / SC_PSUM / SC_PMAX,
    // L.prod and the bot rows before everything below
    __syncthreads();
    const int nprod = L.sc[SC_NPEND];
    const bool over = L.sc[SC_OVER] != 0;
    // the rest of the tick, phase by phase (above)
    const Tick S{p, L, gd, g, G, posw, time, bot0, npa, npa0};
    R.aa = pf.aa, R.aa2 = pf.aa2;   // (lanes < 64 of a fused bot game at one cell per lane; else never read)
    issue_parallel<NT>(S, over);                                            // (2a)
    const int nrows = issue_ordered<NT>(S, over, nprod);                    // (2b)
    cycle<NT>(S, nrows);                                                    // (3) (4)
    finish_tick<NT, FULL>(S, steps0, map_now);                              // (5) (6)
    write_back<NT, P, OT, FB, FULL>(S, R, F, odelta_w, botg, early, pf_ok); // (7)
}

// One step launch over the games of one or more engines (map-size buckets of one
// batch, mrts_step_group): the grid is cut into segments of consecutive games of
// one engine; a workgroup finds its segment with a scalar scan of the table (at
// most 2 * MRTS_STEP_GROUP_MAX entries) and runs that engine's game.  Each
// engine's arrays, map size and LDS carve are its own; the launch's dynamic LDS
// is the largest member's.  A single engine is a one-member, one-segment group.
// FULL: every member has HW == NT (full_hw; the launch checks), which brings the kernel to 8 waves per SIMD -- 8
// resident games per CU, 2048 of the headline's 4096, two rounds instead of 2.29 -- with no occupancy hint: asking
// for 8 waves (amdgpu_waves_per_eu) also cuts the scalar registers to 80 and the kernel then spills three of them.
template <int NT, int P, typename OT, bool FB = false, bool FULL = false>
__global__ __launch_bounds__(NT) void k_step(const StepGroup sg) {
    const int b = blockIdx.x;
    int k = 0;
    while (k + 1 < sg.nseg && b >= sg.seg_block[k + 1]) k++;
    step_game<NT, P, OT, FB, FULL>(sg.e[sg.seg_member[k]], sg.seg_game[k] + (b - sg.seg_block[k]));
}

// ---------------------------------------------------------------------------
// render("rgb_array") (vec_env.py:1075-1084): a size x size RGB frame of one
// game, one lane per pixel.  The Java PhysicalGameStatePanel is absent, so the
// drawing rules are this engine's own (restated pixel for pixel
// by oracle_py.render_frame): cells of cs = size / max(W, H) pixels centred in
// the frame, grid lines, walls, buildings / resources as inset squares, mobile
// units as discs, an owner-coloured rim (player 0 blue, player 1 red) and a
// hit-point bar on damaged units.
__device__ __forceinline__ uint32_t render_type_rgb(int t) {
    switch (t) {
    case RESOURCE: return 0x00A000u;
    case BASE: return 0xFFFFFFu;
    case BARRACKS: return 0xA0A0A0u;
    case WORKER: return 0x808080u;
    case LIGHT: return 0xFF8000u;
    case HEAVY: return 0xFFFF00u;
    default: return 0x00FFFFu;   // RANGED
    }
}

__global__ __launch_bounds__(256) void k_render(const int4* __restrict__ cells, const uint8_t* __restrict__ wall, int W, int H,
                                              int size, uint8_t* __restrict__ rgb) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= size * size) return;
    const int px = pix % size, py = pix / size;
    const int cs = size / max(W, H), ox = (size - cs * W) / 2, oy = (size - cs * H) / 2;
    uint32_t col = 0;
    const int gx = px - ox, gy = py - oy;
    if (gx >= 0 && gy >= 0 && gx < cs * W && gy < cs * H) {
        const int cx = gx / cs, cy = gy / cs, lx = gx - cx * cs, ly = gy - cy * cs, c = cy * W + cx;
        col = wall[c] ? 0x205020u : 0u;
        if (lx == 0 || ly == 0) col = 0x303030u;
        const uint32_t u = (uint32_t)cells[c].x;
        if (u != 0) {
            const int t = u_type(u), ow = u_owner(u), m = cs / 8, b = max(1, cs / 16);
            const bool building = t == RESOURCE || t == BASE || t == BARRACKS;
            bool inside, rim;
            if (building) {
                inside = lx >= m && ly >= m && lx < cs - m && ly < cs - m;
                rim = lx < m + b || ly < m + b || lx >= cs - m - b || ly >= cs - m - b;
            } else {
                const int r2 = cs * 3 / 4, dx = 2 * lx + 1 - cs, dy = 2 * ly + 1 - cs, d2 = dx * dx + dy * dy;
                inside = d2 <= r2 * r2;
                rim = d2 > (r2 - 2 * b) * (r2 - 2 * b);
            }
            if (inside) {
                col = render_type_rgb(t);
                if (rim && ow >= 0) col = ow == 0 ? 0x0000FFu : 0xFF0000u;
            }
            const int hp = u_hp(u), mhp = ut_hp(t);
            if (t != RESOURCE && hp < mhp && ly >= cs - m - 2 * b && ly < cs - m && lx >= m && lx < m + (cs - 2 * m) * hp / mhp)
                col = 0xFF0000u;
        }
    }
    rgb[3 * (size_t)pix] = (uint8_t)(col >> 16);
    rgb[3 * (size_t)pix + 1] = (uint8_t)(col >> 8);
    rgb[3 * (size_t)pix + 2] = (uint8_t)col;
}

// ---------------------------------------------------------------------------
// launchers

// Workgroup size of a map size: one lane per cell up to 256 lanes; the bot-fused
// step needs a wave besides the bot's, so maps of <= 64 cells take 128 lanes there.
__host__ __device__ inline int step_nt(int HW, bool fused) { return HW <= 64 && !fused ? 64 : HW <= 128 ? 128 : 256; }

// f(NT) with a step_nt value, f(planes, obs element) with an engine's obs planes and a value
// of its obs element type (the kernels' P and OT), as compile-time constants
template <int N>
using ic = std::integral_constant<int, N>;
template <typename F>
static auto with_nt(int NT, F&& f) {
    return NT == 64 ? f(ic<64>{}) : NT == 128 ? f(ic<128>{}) : f(ic<256>{});
}
template <typename F>
static auto with_obs(bool partial, int kind, F&& f) {
    auto planes = [&](auto ot) { return partial ? f(ic<31>{}, ot) : f(ic<29>{}, ot); };
    return kind == MRTS_OBS_PACKED ? planes(PackedObs{}) : kind == MRTS_OBS_FLOAT32 ? planes(float{}) : planes(int32_t{});
}

// The step kernel of a launch's (planes, obs type, bot fusion).  No 64-lane launch
// is fused (step_nt: the fused step needs a wave besides the bot's), so no fused
// 64-lane kernel is built.
// full: every member has HW == NT; built for the unfused 256-lane step (16x16), the flagship's.
template <int NT>
static void launch_step(const StepGroup& sg, int grid, size_t sh, hipStream_t s, bool partial, int kind, bool fb, bool full) {
    with_obs(partial, kind, [&](auto planes, auto ot) {
        constexpr int P = decltype(planes)::value;
        using OT = decltype(ot);
        if constexpr (NT == 256) {
            if (!fb && full) {
                hipLaunchKernelGGL((k_step<NT, P, OT, false, true>), dim3(grid), dim3(NT), sh, s, sg);
                return;
            }
        }
        if (!fb) hipLaunchKernelGGL((k_step<NT, P, OT>), dim3(grid), dim3(NT), sh, s, sg);
        else if constexpr (NT > 64) hipLaunchKernelGGL((k_step<NT, P, OT, true>), dim3(grid), dim3(NT), sh, s, sg);
    });
}

// The per-game kernels' launch: a workgroup per game (grid of them) at the unfused step's
// workgroup size and LDS carve.  kernel(NT as a compile-time constant) names the kernel,
// whose arguments are the engine and args.
template <typename F, typename... A>
static hipError_t per_game(const EngineParams& p, int grid, hipStream_t s, F&& kernel, A... args) {
    if (grid == 0) return hipSuccess;
    const mrts_step_layout_t l = mrts_engine_step_layout(p.HW, p.W, 0, 0, 0);
    hipLaunchKernelGGL(with_nt(l.NT, kernel), dim3(grid), dim3(l.NT), l.lds_bytes, s, p, args...);
    return hipGetLastError();
}

// One step launch over n engines of equal planes, obs type and bot fusion, at the
// widest member's workgroup size (a narrower map leaves lanes idle in the game
// logic; every wave still streams outputs).  A single engine's step is a group of one
// with bots_first.  bots_first: every member's bot games take the grid's first
// segments, then the selfplay games: workgroups start in grid order, and a bot game's
// chain (the fused bot after the tick) is the longest, so the short selfplay games fill
// the last round (4096 selfplay + 4096 bot envs, 16x16: step 215 -> 196 us,
// profiles/r03_ab/ab20_single_engine_bots_first/).
static hipError_t step_group(const EngineParams* ps, int n, hipStream_t s, bool bots_first) {
    if (n < 1 || n > MRTS_STEP_GROUP_MAX) return hipErrorInvalidValue;
    const EngineParams& p0 = ps[0];
    const bool fused = p0.fuse_bots != 0;
    int NT = 64;
    for (int i = 0; i < n; i++) {
        const EngineParams& p = ps[i];
        if (p.partial_obs != p0.partial_obs || p.obs_kind != p0.obs_kind || (p.fuse_bots != 0) != fused) return hipErrorInvalidValue;
        NT = std::max(NT, step_nt(p.HW, fused));
    }
    StepGroup sg{};
    size_t sh = 0;
    for (int i = 0; i < n; i++) {
        EngineParams& e = sg.e[i];
        e = ps[i];
        const mrts_step_layout_t l = mrts_engine_step_layout(e.HW, e.W, fused, e.partial_obs, NT);   // at this launch's NT
        e.early_bot = l.early;
        sh = std::max(sh, l.lds_bytes);
    }
    if (sh > MRTS_LDS_CAP_FUSED) return hipErrorInvalidValue;   // one workgroup's LDS on a CU
    int grid = 0;
    auto seg = [&](int m, int g0, int g1) {
        if (g1 <= g0) return;
        sg.seg_block[sg.nseg] = grid;
        sg.seg_member[sg.nseg] = m;
        sg.seg_game[sg.nseg] = g0;
        sg.nseg++;
        grid += g1 - g0;
    };
    for (int pass = 0; pass < (bots_first ? 2 : 1); pass++)
        for (int i = 0; i < n; i++) {
            const EngineParams& e = sg.e[i];
            if (!bots_first) seg(i, 0, e.G);
            else if (pass == 0) seg(i, e.nsp_games, e.G);
            else seg(i, 0, e.nsp_games);
        }
    sg.seg_block[sg.nseg] = grid;
    if (grid == 0) return hipSuccess;
    bool full = true;
    for (int i = 0; i < n; i++) full = full && sg.e[i].HW == NT;
    with_nt(NT, [&](auto nt) { launch_step<decltype(nt)::value>(sg, grid, sh, s, p0.partial_obs, p0.obs_kind, fused, full); });
    return hipGetLastError();
}

}  // namespace mrts

extern "C" {
#ifdef MRTS_STAMPS
// experiment builds: copy the stamp rows (every row; rows of workgroups that did not
// run since the last reset are zero) and, with reset != 0, zero them afterwards;
// returns the row count copied
int mrts_debug_stamps(unsigned long long* out, int max_rows, int reset) {
    const int rows = MRTS_STAMP_ROWS < max_rows ? MRTS_STAMP_ROWS : max_rows;
    if (out && rows > 0 &&
        hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamp), sizeof(unsigned long long) * MRTS_STAMP_COLS * rows, 0, hipMemcpyDeviceToHost))
        return -1;
    if (reset) {
        static unsigned long long zero[1024][MRTS_STAMP_COLS];
        for (int r = 0; r < MRTS_STAMP_ROWS; r += 1024)
            if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamp), zero, sizeof zero, sizeof zero * (r / 1024), hipMemcpyHostToDevice)) return -1;
    }
    return rows;
}
#endif
hipError_t mrts_engine_reset(const EngineParams* p, hipStream_t s, const int32_t* games, const int32_t* maps, int count) {
    return mrts::with_obs(p->partial_obs, p->obs_kind, [&](auto planes, auto ot) {
        auto k = [](auto nt) { return mrts::k_reset<decltype(nt)::value, decltype(planes)::value, decltype(ot)>; };
        return mrts::per_game(*p, games ? count : p->G, s, k, games, maps, count);
    });
}
hipError_t mrts_engine_outputs(const EngineParams* p, hipStream_t s) {
    return mrts::with_obs(p->partial_obs, p->obs_kind, [&](auto planes, auto ot) {
        return mrts::per_game(*p, p->G, s, [](auto nt) { return mrts::k_outputs<decltype(nt)::value, decltype(planes)::value, decltype(ot)>; });
    });
}
hipError_t mrts_engine_masks(const EngineParams* p, hipStream_t s) {
    return mrts::per_game(*p, p->G, s, [](auto nt) { return mrts::k_masks<decltype(nt)::value>; });
}
hipError_t mrts_engine_masks_packed(const EngineParams* p, hipStream_t s, int32_t* packed) {
    return mrts::per_game(*p, p->G, s, [](auto nt) { return mrts::k_masks_packed<decltype(nt)::value>; }, packed);
}
hipError_t mrts_engine_raw_obs(const EngineParams* p, hipStream_t s, int32_t* raw) {
    return mrts::per_game(*p, p->G, s, [](auto nt) { return mrts::k_raw<decltype(nt)::value>; }, raw);
}
hipError_t mrts_engine_step_group(const EngineParams* ps, int n, hipStream_t s, int bots_first) {
    return mrts::step_group(ps, n, s, bots_first != 0);
}
mrts_step_layout_t mrts_engine_step_layout(int HW, int W, int fused, int partial, int NT) {
    mrts_step_layout_t r{NT ? NT : mrts::step_nt(HW, fused != 0), 0, 0};
    r.early = fused && !partial && mrts::early_bot_disjoint(HW, W, r.NT);
    if (fused) {
        r.lds_bytes = mrts::fused_carve(mrts::lds_any_base(), HW, W, r.NT, r.early != 0, true).bytes;
    } else {
        mrts::Carver c{mrts::lds_any_base()};
        mrts::carve(c, HW, W, r.NT);
        r.lds_bytes = c.o;
    }
    return r;
}
hipError_t mrts_engine_render(const EngineParams* p, hipStream_t s, int game, int map, int size, uint8_t* rgb) {
    const int nblk = (size * size + 255) / 256;
    hipLaunchKernelGGL(mrts::k_render, dim3(nblk), dim3(256), 0, s, p->cells + (size_t)game * p->cstride, p->map_wall + (size_t)map * p->HW,
                       p->W, p->H, size, rgb);
    return hipGetLastError();
}
}
