// mrts_capi.cpp -- C ABI of libmicrorts_amd.so (include/microrts_amd.h).
//
// Host side of the replacement for tests.JNIGridnetVecClient
// (/root/reference/gym_microrts/envs/vec_env.py:256-276): config validation,
// PhysicalGameState XML loading into device map templates, workspace carving
// and kernel dispatch.  No torch types cross this boundary.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "microrts_amd.h"
#include "mrts_engine.h"
#include "mrts_layout.h"
#include "mrts_rollout.h"

namespace {

const char *kTypeNames[MRTS_NTYPES] = {"Resource", "Base", "Barracks", "Worker", "Light", "Heavy", "Ranged"};

struct MapData {
    int w = 0, h = 0;
    std::vector<uint8_t> wall;
    int res[2] = {0, 0};
    std::vector<int4> cells;  // template records (unit word, uid, 0, 0)
    int nunits = 0;
};

std::string attr(const std::string &tag, const char *name) {
    std::string key = std::string(" ") + name + "=\"";
    size_t p = tag.find(key);
    if (p == std::string::npos) return std::string();
    p += key.size();
    size_t q = tag.find('"', p);
    return q == std::string::npos ? std::string() : tag.substr(p, q - p);
}

bool to_int(const std::string &s, int *out) {
    if (s.empty()) return false;
    char *end = nullptr;
    long v = std::strtol(s.c_str(), &end, 10);
    if (*end) return false;
    *out = (int)v;
    return true;
}

uint32_t unit_word(int type, int owner, int hp, int res) {
    return (uint32_t)(type + 1) | ((uint32_t)(owner + 1) << 4) | ((uint32_t)hp << 6) | ((uint32_t)res << 16);
}

// rts.PhysicalGameState.load (XML form of /root/reference/PCG/maps/wall-1:1-16)
bool load_map(const char *path, MapData *m, std::string *err) {
    std::ifstream f(path);
    if (!f) { *err = std::string("cannot open map ") + path; return false; }
    std::stringstream ss;
    ss << f.rdbuf();
    std::string x = ss.str();
    size_t root = x.find("<rts.PhysicalGameState");
    if (root == std::string::npos) { *err = std::string("not a PhysicalGameState XML: ") + path; return false; }
    std::string rtag = x.substr(root, x.find('>', root) - root);
    if (!to_int(attr(rtag, "width"), &m->w) || !to_int(attr(rtag, "height"), &m->h) || m->w <= 0 || m->h <= 0) {
        *err = std::string("bad width/height in ") + path;
        return false;
    }
    const int HW = m->w * m->h;
    if (HW > MRTS_MAX_HW) { *err = "map larger than MRTS_MAX_HW cells"; return false; }
    size_t t0 = x.find("<terrain>"), t1 = x.find("</terrain>");
    if (t0 == std::string::npos || t1 == std::string::npos) { *err = "missing <terrain>"; return false; }
    std::string terr;
    for (size_t i = t0 + 9; i < t1; i++)
        if (x[i] == '0' || x[i] == '1') terr.push_back(x[i]);
    if ((int)terr.size() != HW) { *err = std::string("terrain length mismatch in ") + path; return false; }
    m->wall.assign(HW, 0);
    for (int i = 0; i < HW; i++) m->wall[i] = terr[i] == '1';
    size_t pos = 0;
    while ((pos = x.find("<rts.Player ", pos)) != std::string::npos) {
        std::string tag = x.substr(pos, x.find('>', pos) - pos);
        int id = -1, r = 0;
        if (!to_int(attr(tag, "ID"), &id) || !to_int(attr(tag, "resources"), &r) || id < 0 || id > 1) {
            *err = "bad <rts.Player>";
            return false;
        }
        m->res[id] = r;
        pos += 12;
    }
    m->cells.assign(HW, make_int4(0, 0, 0, 0));
    pos = 0;
    int idx = 0;
    while ((pos = x.find("<rts.units.Unit ", pos)) != std::string::npos) {
        std::string tag = x.substr(pos, x.find('>', pos) - pos);
        std::string tn = attr(tag, "type");
        int type = -1;
        for (int k = 0; k < MRTS_NTYPES; k++)
            if (tn == kTypeNames[k]) type = k;
        int player, ux, uy, ur, hp;
        if (type < 0 || !to_int(attr(tag, "player"), &player) || !to_int(attr(tag, "x"), &ux) ||
            !to_int(attr(tag, "y"), &uy) || !to_int(attr(tag, "resources"), &ur) || !to_int(attr(tag, "hitpoints"), &hp)) {
            *err = std::string("bad <rts.units.Unit> in ") + path;
            return false;
        }
        if (ux < 0 || uy < 0 || ux >= m->w || uy >= m->h || player < -1 || player > 1 || hp < 1 || hp > 1023 ||
            ur < 0 || ur > 65535) {
            *err = std::string("unit out of range in ") + path;
            return false;
        }
        int c = uy * m->w + ux;
        if (m->cells[c].x != 0) { *err = std::string("two units in one cell in ") + path; return false; }
        m->cells[c] = make_int4((int)unit_word(type, player, hp, ur), idx++, 0, 0);
        pos += 16;
    }
    m->nunits = idx;
    return true;
}

std::string utt_json() {
    // rts.units.UnitTypeTable.toJSON of UnitTypeTable() (VERSION_ORIGINAL)
    struct T { const char *n; int cost, hp, mind, maxd, range, pt, mt, at, ht, rt, ha, sight; int res, stock, harv, move, atk; const char *prod, *by; };
    static const T ts[] = {
        {"Resource", 1, 1, 1, 1, 1, 10, 10, 10, 10, 10, 1, 0, 1, 0, 0, 0, 0, "", ""},
        {"Base", 10, 10, 1, 1, 1, 250, 10, 10, 10, 10, 1, 5, 0, 1, 0, 0, 0, "\"Worker\"", "\"Worker\""},
        {"Barracks", 5, 4, 1, 1, 1, 200, 10, 10, 10, 10, 1, 3, 0, 0, 0, 0, 0, "\"Light\", \"Heavy\", \"Ranged\"", "\"Worker\""},
        {"Worker", 1, 1, 1, 1, 1, 50, 10, 5, 20, 10, 1, 3, 0, 0, 1, 1, 1, "\"Base\", \"Barracks\"", "\"Base\""},
        {"Light", 2, 4, 2, 2, 1, 80, 8, 5, 10, 10, 1, 2, 0, 0, 0, 1, 1, "", "\"Barracks\""},
        {"Heavy", 2, 4, 4, 4, 1, 120, 12, 5, 10, 10, 1, 2, 0, 0, 0, 1, 1, "", "\"Barracks\""},
        {"Ranged", 2, 1, 1, 1, 3, 100, 10, 5, 10, 10, 1, 3, 0, 0, 0, 1, 1, "", "\"Barracks\""},
    };
    std::string s = "{\"moveConflictResolutionStrategy\":3,\"unitTypes\":[";
    char buf[1024];
    for (int i = 0; i < MRTS_NTYPES; i++) {
        const T &t = ts[i];
        std::snprintf(buf, sizeof buf,
                      "%s{\"ID\":%d, \"name\":\"%s\", \"cost\":%d, \"hp\":%d, \"minDamage\":%d, \"maxDamage\":%d, "
                      "\"attackRange\":%d, \"produceTime\":%d, \"moveTime\":%d, \"attackTime\":%d, \"harvestTime\":%d, "
                      "\"returnTime\":%d, \"harvestAmount\":%d, \"sightRadius\":%d, \"isResource\":%s, \"isStockpile\":%s, "
                      "\"canHarvest\":%s, \"canMove\":%s, \"canAttack\":%s, \"produces\":[%s], \"producedBy\":[%s]}",
                      i ? ", " : "", i, t.n, t.cost, t.hp, t.mind, t.maxd, t.range, t.pt, t.mt, t.at, t.ht, t.rt, t.ha,
                      t.sight, t.res ? "true" : "false", t.stock ? "true" : "false", t.harv ? "true" : "false",
                      t.move ? "true" : "false", t.atk ? "true" : "false", t.prod, t.by);
        s += buf;
    }
    s += "]}";
    return s;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// int4 records between consecutive games' cell rows (a padded stride measured
// neutral, profiles/r04_ab/README.md)
int cell_stride(int HW) { return HW; }

}  // namespace

struct mrts_vec {
    int nsp = 0, nbot = 0, ngames = 0, nenvs = 0, max_steps = 0, partial_obs = 0, obs_kind = MRTS_OBS_INT32;
    int W = 0, H = 0, HW = 0;
    std::vector<MapData> maps;
    std::vector<std::string> map_path;   // as given to mrts_create / mrts_add_map
    int map_capacity = 0;                // map template slots carved in the workspace
    std::vector<int32_t> game_map;
    std::vector<int32_t> bot_ai;
    std::vector<int32_t> bot_ai0;   // -1: the agent plays player 0
    int nbot0 = 0;
    int game_offset = 0;
    // workspace carving
    size_t off_cells = 0, off_genv = 0, off_mcells = 0, off_mwall = 0, off_mscal = 0, off_scratch = 0, total = 0;
    size_t off_botai = 0, off_botai0 = 0, off_aa = 0, off_botpa = 0, off_parked = 0;
    std::vector<uint8_t> parked;   // host mirror of the device parked flags (mrts_park_games)
    int nbot_active = 0;
    unsigned char *ws = nullptr;
    std::vector<int32_t> scratch_host;
    std::string err, utt;
    double rw[6] = {0, 0, 0, 0, 0, 0};
    int shaping = 1;
    int32_t *next_mask = nullptr, *next_src = nullptr;   // mrts_bind_mask_outputs
    EngineParams base{};
    // bot fusion (mrts_set_bot_fusion): k_step decides the next tick's bot actions
    int fuse = 1;             // requested
    bool bots_ready = false;  // the bot decisions for the current state are in botpa / aa
    // delta masks (mrts_set_mask_delta): k_step stores only the mask rows that can differ
    // from what the bound buffer holds, which needs masks_synced: every row of next_mask
    // is getMasks(0) of the stored state (parked games: zeros).  Every entry point that
    // changes the game state or the binding, and its effect on masks_synced:
    //   mrts_bind_workspace      cleared (new state memory)
    //   mrts_bind_mask_outputs   cleared, also for the same pointers: the way a caller who wrote
    //                            into the buffer hands it back
    //   mrts_reset               set (k_reset writes every game's rows)
    //   mrts_step / _weighted / mrts_step_group
    //                            all through step_engines: dense step: set; delta step: stays set (it
    //                            ran because it was set); a failed bot or step launch: cleared
    //   mrts_get_masks           set when called with exactly the bound pointers (k_masks writes
    //                            every row); cleared when only one of the two is the bound one
    //   mrts_load_state          cleared once the state copy is queued, set by its outputs launch
    //   mrts_reset_games / mrts_park_games
    //                            left alone: k_reset writes the listed games' rows in full (zeros
    //                            for parked ones), the others are untouched; a parked game's
    //                            k_step returns before any write and its rows stay zero
    //   mrts_add_map, mrts_set_reward_weight, mrts_set_bot_fusion, mrts_set_mask_delta, mrts_save_state,
    //   mrts_get_raw_obs, mrts_get_masks_packed, mrts_render, mrts_game_stats, mrts_error_flags
    //                            no effect (neither the state nor the buffer changes; a caller who
    //                            passes the bound mask buffer as the packed output has written into
    //                            it and binds again, as after any write of its own)
    // and any of the launches above that fails while masks are bound clears it.
    int mask_delta = 1;          // requested
    bool masks_synced = false;
    // action format (mrts_set_action_format): what the steps' `actions` pointer holds.  A reader's setting:
    // it changes no game state and is not part of the configuration fingerprint.
    int act_packed = 0;
    // delta obs (mrts_set_obs_delta; dense obs kinds): k_step stores only the obs rows whose one-hot
    // word differs from the loaded state's, which needs every row of the step's obs buffer to be the
    // one-hot of the stored state (parked games: zeros).  The obs pointer arrives per call, so the engine
    // remembers obs_synced_ptr: the buffer it knows to be that, or null.  Every entry point that changes
    // the game state or writes obs, and its effect:
    //   mrts_bind_workspace      cleared (new state memory)
    //   mrts_reset               set to its obs (k_reset writes every game's rows)
    //   mrts_step / _weighted / mrts_step_group
    //                            all through step_engines: a step into obs_synced_ptr runs delta and leaves
    //                            it; a step into any other pointer, or with delta off, runs dense and sets
    //                            it to that pointer; a failed bot or step launch: cleared
    //   mrts_load_state          cleared once the state copy is queued, set to its obs by its outputs launch
    //   mrts_reset_games / mrts_park_games
    //                            left alone when given obs_synced_ptr: k_reset writes the listed games' rows
    //                            in full (zeros for parked ones), the others are untouched, and a parked
    //                            game's k_step returns before any write; cleared when given another pointer
    //                            (those games' rows in the remembered buffer are stale) or when they fail
    //   mrts_invalidate_obs      cleared: the way a caller who wrote into the buffer hands it back
    //   everything else          no effect (neither the state nor an obs buffer changes)
    int obs_delta = 1;           // requested
    const void *obs_synced_ptr = nullptr;
};

// the launches that write the bound mask buffers report here: `dense` = every game's rows
static void masks_written(mrts_vec *h, hipError_t e, bool dense) {
    if (!h->next_mask) return;
    if (e) h->masks_synced = false;
    else if (dense) h->masks_synced = true;
}
// delta needs a bit per cell and view in one register of the lane that owns the cell: at
// most 16 cells per lane of the narrowest step workgroup (every map mrts_create accepts)
static bool delta_ok(const mrts_vec *h) {
    return h->mask_delta && h->masks_synced && h->next_mask && h->HW <= MRTS_MASK_DELTA_CELLS * mrts_engine_step_layout(h->HW, h->W, 0, 0, 0).NT;
}

// the launches that write obs report here: `dense` = every game's rows, into `obs`
static void obs_written(mrts_vec *h, hipError_t e, const void *obs, bool dense) {
    if (e) h->obs_synced_ptr = nullptr;
    else if (dense) h->obs_synced_ptr = obs;
}
// delta obs needs the old one-hot words of a lane's cells in its registers: at most MRTS_OBS_DELTA_CELLS
// cells per lane of the map's own (narrowest) step workgroup, so k_step never sees a size it cannot
// serve; larger maps step dense.  Packed obs are 4 bytes per cell as it is: always in full.  Fog engines
// step dense too: their rows depend on the sight disks, and building the loaded state's disks cost more
// than the stores saved (partial_obs workload 78.5 -> 76.7 M env-steps/s, profiles/obs_delta/README.md).
static bool obs_delta_ok(const mrts_vec *h, const void *obs) {
    return h->obs_delta && h->obs_kind != MRTS_OBS_PACKED && !h->partial_obs && obs && h->obs_synced_ptr == obs &&
           h->HW <= MRTS_OBS_DELTA_CELLS * mrts_engine_step_layout(h->HW, h->W, 0, 0, 0).NT;
}

static int fail(mrts_vec *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    return code;
}
static int hip_fail(mrts_vec *h, hipError_t e, const char *what) {
    return fail(h, MRTS_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The templates of `count` maps into the workspace's slots first.. (walls, unit records, scalars),
// staged here and drained before this returns.
static hipError_t upload_maps(mrts_vec *h, hipStream_t s, const MapData *maps, int first, int count) {
    const size_t HW = (size_t)h->HW;
    std::vector<int4> mc(count * HW);
    std::vector<uint8_t> mw(count * HW);
    std::vector<int32_t> ms((size_t)count * MRTS_MAP_SCALARS, 0);
    for (int i = 0; i < count; i++) {
        std::memcpy(&mc[i * HW], maps[i].cells.data(), sizeof(int4) * HW);
        std::memcpy(&mw[i * HW], maps[i].wall.data(), HW);
        ms[i * MRTS_MAP_SCALARS + MRTS_M_RES0] = maps[i].res[0];
        ms[i * MRTS_MAP_SCALARS + MRTS_M_RES1] = maps[i].res[1];
        ms[i * MRTS_MAP_SCALARS + MRTS_M_NUNITS] = maps[i].nunits;
    }
    hipError_t e = hipMemcpyAsync(h->ws + h->off_mcells + first * HW * sizeof(int4), mc.data(), mc.size() * sizeof(int4), hipMemcpyHostToDevice, s);
    if (!e) e = hipMemcpyAsync(h->ws + h->off_mwall + first * HW, mw.data(), mw.size(), hipMemcpyHostToDevice, s);
    if (!e) e = hipMemcpyAsync(h->ws + h->off_mscal + (size_t)first * MRTS_MAP_SCALARS * sizeof(int32_t), ms.data(), ms.size() * sizeof(int32_t),
                               hipMemcpyHostToDevice, s);
    const hipError_t es = hipStreamSynchronize(s);   // a queued copy may still read the staging vectors after a later one failed
    return e ? e : es;
}

extern "C" {

const char *mrts_version(void) { return "microrts_amd 0.1 (gfx950)"; }

int mrts_create(const mrts_config *cfg, mrts_vec **out) {
    if (!cfg || !out) return MRTS_EINVAL;
    *out = nullptr;
    mrts_vec *h = new mrts_vec();
    h->utt = utt_json();
    *out = h;
    if (cfg->num_selfplay_envs < 0 || cfg->num_bot_envs < 0 || (cfg->num_selfplay_envs & 1))
        return fail(h, MRTS_EINVAL, "num_selfplay_envs must be even and >= 0, num_bot_envs >= 0");
    if (cfg->num_selfplay_envs + cfg->num_bot_envs <= 0) return fail(h, MRTS_EINVAL, "no envs");
    if (cfg->max_steps <= 0 || cfg->max_steps >= MRTS_MAX_TIME)
        return fail(h, MRTS_EINVAL, "max_steps must be in [1, 500000)");
    if (cfg->num_maps <= 0 || !cfg->map_paths) return fail(h, MRTS_EINVAL, "no maps");
    h->nsp = cfg->num_selfplay_envs;
    h->nbot = cfg->num_bot_envs;
    h->ngames = h->nsp / 2 + h->nbot;
    h->nenvs = h->nsp + h->nbot;
    h->max_steps = cfg->max_steps;
    h->partial_obs = cfg->partial_obs;
    h->obs_kind = cfg->obs_dtype == MRTS_OBS_FLOAT32 || cfg->obs_dtype == MRTS_OBS_PACKED ? cfg->obs_dtype : MRTS_OBS_INT32;
    if (cfg->map_capacity != 0 && cfg->map_capacity < cfg->num_maps)
        return fail(h, MRTS_EINVAL, "map_capacity must be 0 or >= num_maps");
    h->map_capacity = cfg->map_capacity ? cfg->map_capacity : cfg->num_maps;
    h->maps.resize(cfg->num_maps);
    for (int i = 0; i < cfg->num_maps; i++) {
        std::string e;
        if (!cfg->map_paths[i] || !load_map(cfg->map_paths[i], &h->maps[i], &e))
            return fail(h, MRTS_EIO, cfg->map_paths[i] ? e : "null map path");
        h->map_path.emplace_back(cfg->map_paths[i]);
        if (i > 0 && (h->maps[i].w != h->maps[0].w || h->maps[i].h != h->maps[0].h))
            return fail(h, MRTS_EINVAL, "all maps of one vec env must share height x width (vec_env.py:149-150)");
    }
    h->W = h->maps[0].w;
    h->H = h->maps[0].h;
    h->HW = h->W * h->H;
    if (mrts_engine_step_layout(h->HW, h->W, 0, 0, 0).lds_bytes > MRTS_LDS_CAP)
        return fail(h, MRTS_ENOTIMPL, "map too large: the step kernel's workgroup LDS carve exceeds 64 KB (maps up to "
                                      "about 1128 cells fit, e.g. 32x32, 33x33, 47x24; DESIGN.md §3)");
    h->game_map.assign(h->ngames, 0);
    for (int g = 0; g < h->ngames; g++) {
        int m = cfg->game_map ? cfg->game_map[g] : 0;
        if (m < 0 || m >= cfg->num_maps) return fail(h, MRTS_EINVAL, "game_map index out of range");
        h->game_map[g] = m;
    }
    h->bot_ai.assign(h->nbot, MRTS_AI_PASSIVE);
    h->nbot_active = 0;
    for (int j = 0; j < h->nbot; j++) {
        int a = cfg->bot_ai ? cfg->bot_ai[j] : MRTS_AI_PASSIVE;
        if (a < 0 || a >= MRTS_AI_COUNT) return fail(h, MRTS_EINVAL, "bot_ai: unknown MRTS_AI_* id");
        h->bot_ai[j] = a;
        h->nbot_active += a != MRTS_AI_PASSIVE;
    }
    if (cfg->game_offset < 0) return fail(h, MRTS_EINVAL, "game_offset must be >= 0");
    h->game_offset = cfg->game_offset;
    h->bot_ai0.assign(h->nbot, -1);
    h->nbot0 = 0;
    for (int j = 0; cfg->bot_ai0 && j < h->nbot; j++) {
        int a = cfg->bot_ai0[j];
        if (a < -1 || a >= MRTS_AI_COUNT) return fail(h, MRTS_EINVAL, "bot_ai0: unknown MRTS_AI_* id");
        h->bot_ai0[j] = a;
        h->nbot0 += a >= 0;
        h->nbot_active += a > MRTS_AI_PASSIVE;
    }
    if (h->nbot_active) {
        if (h->W > 32 || h->H > 64)
            return fail(h, MRTS_ENOTIMPL, "device bots need maps at most 32 wide and 64 high (one bit word per row)");
        if (mrts_engine_bot_lds_bytes(h->HW, h->W) > MRTS_LDS_CAP)
            return fail(h, MRTS_ENOTIMPL, "map too large for the bot kernel's LDS");
    }
    size_t o = 0;
    h->off_cells = o; o = align256(o + (size_t)h->ngames * cell_stride(h->HW) * sizeof(int4));
    h->off_genv = o; o = align256(o + (size_t)h->ngames * MRTS_GENV_WORDS * sizeof(int32_t));
    h->off_mcells = o; o = align256(o + (size_t)h->map_capacity * h->HW * sizeof(int4));
    h->off_mwall = o; o = align256(o + (size_t)h->map_capacity * h->HW);
    h->off_mscal = o; o = align256(o + (size_t)h->map_capacity * MRTS_MAP_SCALARS * sizeof(int32_t));
    h->off_scratch = o; o = align256(o + (size_t)2 * h->ngames * sizeof(int32_t));
    h->off_botai = o; o = align256(o + (size_t)(h->nbot + 1) * sizeof(int32_t));
    h->off_botai0 = o; o = align256(o + (size_t)(h->nbot + 1) * sizeof(int32_t));
    h->off_aa = o; o = align256(o + (h->nbot_active ? (size_t)h->nbot * 2 * h->HW * 2 * sizeof(int4) : 0));
    h->off_botpa = o; o = align256(o + (h->nbot_active ? (size_t)h->nbot * 2 * h->HW * sizeof(int32_t) : 0));
    h->off_parked = o; o = align256(o + (size_t)h->ngames);
    h->total = o;
    h->err.clear();
    return MRTS_OK;
}

int mrts_info(const mrts_vec *h, mrts_info_t *info) {
    if (!h || !info || h->HW == 0) return MRTS_EINVAL;
    info->height = h->H;
    info->width = h->W;
    info->num_envs = h->nenvs;
    info->num_games = h->ngames;
    info->obs_planes = h->partial_obs ? 31 : 29;
    info->mask_channels = MRTS_MASK_CH;
    info->action_components = 7;
    info->workspace_bytes = h->total;
    return MRTS_OK;
}

int mrts_bind_workspace(mrts_vec *h, void *dev, void *stream) {
    if (!h || !dev || h->HW == 0) return fail(h, MRTS_EINVAL, "bind_workspace: bad handle or pointer");
    if (((uintptr_t)dev & 255u) != 0) return fail(h, MRTS_EINVAL, "workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    h->bots_ready = false;
    h->masks_synced = false;
    h->obs_synced_ptr = nullptr;
    h->ws = (unsigned char *)dev;
    std::vector<int32_t> genv((size_t)h->ngames * MRTS_GENV_WORDS, 0);
    for (int g = 0; g < h->ngames; g++) genv[(size_t)g * MRTS_GENV_WORDS + MRTS_G_MAP] = h->game_map[g];
    hipError_t e;
    if ((e = upload_maps(h, s, h->maps.data(), 0, (int)h->maps.size())) ||
        (e = hipMemcpyAsync(h->ws + h->off_genv, genv.data(), genv.size() * sizeof(int32_t), hipMemcpyHostToDevice, s)) ||
        (h->nbot && (e = hipMemcpyAsync(h->ws + h->off_botai, h->bot_ai.data(), h->nbot * sizeof(int32_t), hipMemcpyHostToDevice, s))) ||
        (h->nbot && (e = hipMemcpyAsync(h->ws + h->off_botai0, h->bot_ai0.data(), h->nbot * sizeof(int32_t), hipMemcpyHostToDevice, s))) ||
        (e = hipStreamSynchronize(s)))
        return hip_fail(h, e, "bind_workspace upload");
    EngineParams &p = h->base;
    p = EngineParams{};
    p.cells = (int4 *)(h->ws + h->off_cells);
    p.cstride = cell_stride(h->HW);
    p.genv = (int32_t *)(h->ws + h->off_genv);
    p.map_cells = (const int4 *)(h->ws + h->off_mcells);
    p.map_wall = (const uint8_t *)(h->ws + h->off_mwall);
    p.map_scal = (const int32_t *)(h->ws + h->off_mscal);
    p.G = h->ngames;
    p.nmaps = (int)h->maps.size();
    p.HW = h->HW;
    p.W = h->W;
    p.H = h->H;
    p.nsp = h->nsp;
    p.nsp_games = h->nsp / 2;
    p.max_steps = h->max_steps;
    p.obs_kind = h->obs_kind;
    p.partial_obs = h->partial_obs;
    p.bot_ai = (const int32_t *)(h->ws + h->off_botai);
    p.bot_ai0 = h->nbot0 ? (const int32_t *)(h->ws + h->off_botai0) : nullptr;
    p.aa = h->nbot_active ? (int4 *)(h->ws + h->off_aa) : nullptr;
    p.botpa = h->nbot_active ? (int32_t *)(h->ws + h->off_botpa) : nullptr;
    p.nbot_active = h->nbot_active;
    p.game_offset = h->game_offset;
    p.parked = nullptr;   // until a game is parked
    h->parked.assign(h->ngames, 0);
    h->err.clear();
    return MRTS_OK;
}

// host flags -> device; the engine checks them from now on
static hipError_t upload_parked(mrts_vec *h, hipStream_t s) {
    uint8_t *d = h->ws + h->off_parked;
    hipError_t e = hipMemcpyAsync(d, h->parked.data(), h->parked.size(), hipMemcpyHostToDevice, s);
    if (!e) e = hipStreamSynchronize(s);   // the host vector may change before the copy would run
    if (!e) h->base.parked = d;
    return e;
}

static bool bound(mrts_vec *h) { return h && h->ws; }

// Bot fusion applies to games whose bots play player 1 only (bot-vs-bot games
// decide for both sides: separate k_bot), and when both LDS regions fit a
// workgroup (the fused step workgroup has at least two waves: maps of <= 64
// cells take 128 lanes, mrts_engine.hip step_nt).
static bool fused(const mrts_vec *h) {
    return h->fuse && h->nbot_active > 0 && h->nbot0 == 0 && mrts_engine_step_layout(h->HW, h->W, 1, h->partial_obs, 0).lds_bytes <= MRTS_LDS_CAP_FUSED;
}

// after a reset of every game (games == null) or of the listed ones: with
// fusion, decide their bot actions now (the next step will not launch k_bot)
static hipError_t bots_after_reset(mrts_vec *h, hipStream_t s, const int32_t *games, int count) {
    if (!fused(h)) {
        h->bots_ready = false;
        return hipSuccess;
    }
    if (games && !h->bots_ready) return hipSuccess;   // the next step decides for every game anyway
    EngineParams p = h->base;
    p.bot_games = games;
    p.bot_ngames = count;
    hipError_t e = mrts_engine_bots(&p, s);
    if (!e) h->bots_ready = true;
    return e;
}

int mrts_set_bot_fusion(mrts_vec *h, int32_t on) {
    if (!h) return fail(h, MRTS_EINVAL, "set_bot_fusion: null handle");
    h->fuse = on ? 1 : 0;   // bots_ready stays valid: decisions already made are used once either way
    return MRTS_OK;
}

int mrts_set_mask_delta(mrts_vec *h, int32_t on) {
    if (!h) return fail(h, MRTS_EINVAL, "set_mask_delta: null handle");
    h->mask_delta = on ? 1 : 0;   // masks_synced stays: a dense step keeps the buffer in sync too
    return MRTS_OK;
}

int mrts_set_action_format(mrts_vec *h, int32_t format) {
    if (!h) return fail(h, MRTS_EINVAL, "set_action_format: null handle");
    if (format != MRTS_ACT_DENSE && format != MRTS_ACT_PACKED)
        return fail(h, MRTS_EINVAL, "set_action_format: format must be MRTS_ACT_DENSE or MRTS_ACT_PACKED");
    h->act_packed = format == MRTS_ACT_PACKED ? 1 : 0;
    return MRTS_OK;
}

int mrts_set_obs_delta(mrts_vec *h, int32_t on) {
    if (!h) return fail(h, MRTS_EINVAL, "set_obs_delta: null handle");
    h->obs_delta = on ? 1 : 0;   // obs_synced_ptr stays: a dense step keeps the buffer in sync too
    return MRTS_OK;
}

int mrts_invalidate_obs(mrts_vec *h) {
    if (!h) return fail(h, MRTS_EINVAL, "invalidate_obs: null handle");
    h->obs_synced_ptr = nullptr;
    return MRTS_OK;
}

// the parameters of a launch that writes obs and, when bound, the next tick's masks and sources
static EngineParams out_params(const mrts_vec *h, void *obs) {
    EngineParams p = h->base;
    p.obs = obs;
    p.mask = h->next_mask;
    p.src_out = h->next_src;
    return p;
}

int mrts_reset(mrts_vec *h, void *stream, void *obs) {
    if (!bound(h) || !obs) return fail(h, MRTS_ESTATE, "reset: workspace not bound or obs null");
    EngineParams p = out_params(h, obs);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = mrts_engine_reset(&p, s, nullptr, nullptr, 0);
    masks_written(h, e, true);
    obs_written(h, e, obs, true);
    if (!e) e = bots_after_reset(h, s, nullptr, 0);
    return e ? hip_fail(h, e, "reset launch") : MRTS_OK;
}

int mrts_get_masks(mrts_vec *h, void *stream, int32_t *mask, int32_t *source) {
    if (!bound(h) || !mask || !source) return fail(h, MRTS_ESTATE, "get_masks: workspace not bound or null output");
    EngineParams p = h->base;
    p.mask = mask;
    p.src_out = source;
    hipError_t e = mrts_engine_masks(&p, (hipStream_t)stream);
    if (mask == h->next_mask && source == h->next_src) masks_written(h, e, true);
    else if (mask == h->next_mask || source == h->next_src) h->masks_synced = false;   // half the binding: not the engine's rows
    return e ? hip_fail(h, e, "masks launch") : MRTS_OK;
}

// A launch of its own into the caller's buffer: it reads the games, writes nothing the
// engine owns and leaves the bound dense buffers and masks_synced as they are.
int mrts_get_masks_packed(mrts_vec *h, void *stream, int32_t *packed) {
    if (!h || !packed) return fail(h, MRTS_EINVAL, "get_masks_packed: null handle or output");
    if (!bound(h)) return fail(h, MRTS_ESTATE, "get_masks_packed: workspace not bound");
    hipError_t e = mrts_engine_masks_packed(&h->base, (hipStream_t)stream, packed);
    return e ? hip_fail(h, e, "packed masks launch") : MRTS_OK;
}

// the step's parameters of one engine (mrts_step / mrts_step_weighted / mrts_step_group)
static EngineParams step_params(const mrts_vec *h, const mrts_step_io &io) {
    EngineParams p = out_params(h, io.obs);
    p.actions = io.actions;
    p.act_packed = h->act_packed;
    p.src = io.source;
    p.raw_reward = io.raw_reward;
    p.done = io.done;
    if (io.reward) {
        p.reward = io.reward;
        p.done0 = io.done0;
        for (int k = 0; k < 6; k++) p.rw[k] = h->rw[k];
        p.shaping = h->shaping;
    }
    p.mask_delta = delta_ok(h) ? 1 : 0;
    p.obs_delta = obs_delta_ok(h, io.obs) ? 1 : 0;
    return p;
}

static bool io_ok(const mrts_step_io &io, bool weighted) {
    return io.actions && io.source && io.obs && io.raw_reward && io.done && (!weighted || (io.reward && io.done0));
}
// a packed-action engine reads `actions` as int32 words: 4-byte alignment is all it needs
static bool actions_aligned(const mrts_vec *h, const mrts_step_io &io) { return !h->act_packed || ((uintptr_t)io.actions & 3u) == 0; }

int mrts_get_raw_obs(mrts_vec *h, void *stream, int32_t *raw) {
    if (!bound(h) || !raw) return fail(h, MRTS_ESTATE, "get_raw_obs: workspace not bound or raw null");
    hipError_t e = mrts_engine_raw_obs(&h->base, (hipStream_t)stream, raw);
    return e ? hip_fail(h, e, "raw obs launch") : MRTS_OK;
}

int mrts_set_reward_weight(mrts_vec *h, const double *w, int32_t shaping) {
    if (!h || !w) return fail(h, MRTS_EINVAL, "set_reward_weight: null argument");
    for (int k = 0; k < 6; k++) h->rw[k] = w[k];
    h->shaping = shaping ? 1 : 0;
    return MRTS_OK;
}

// A member may share a launch when its workgroup still leaves >= this many per CU
// at the widest workgroup size: the step kernels' own occupancy (6-7 workgroups
// per CU, register-limited), so that merging costs no member residency; a larger
// map keeps its own launch.  (configs[4], round 4: 24x24 apart at 40 KB 261 us per
// step vs 264 us all in one launch, profiles/r04_ab/.)
#ifndef MRTS_GROUP_MIN_WG_PER_CU
#define MRTS_GROUP_MIN_WG_PER_CU 6
#endif
static const size_t kGroupLdsCap = MRTS_LDS_CAP_FUSED / MRTS_GROUP_MIN_WG_PER_CU;

// Launch plan of a group: launch_of[i] = the launch (0, 1, ..) member i runs in.
// Members of equal planes / obs type / fusion share a launch (merge != 0), each
// launch in the caller's order of its first member.  Returns the launch count.
static int group_plan(const EngineParams *ps, int n, int policy, int *launch_of) {
    const int merge = policy & 3;
    auto lds = [&](const EngineParams &p, int NT) { return mrts_engine_step_layout(p.HW, p.W, p.fuse_bots, p.partial_obs, NT).lds_bytes; };
    auto compatible = [&](const EngineParams &a, const EngineParams &b) {
        return a.partial_obs == b.partial_obs && a.obs_kind == b.obs_kind && (a.fuse_bots != 0) == (b.fuse_bots != 0);
    };
    int own_nt[MRTS_STEP_GROUP_MAX];   // each member's own workgroup size, asked once
    for (int i = 0; i < n; i++) {
        launch_of[i] = -1;
        own_nt[i] = mrts_engine_step_layout(ps[i].HW, ps[i].W, ps[i].fuse_bots, ps[i].partial_obs, 0).NT;
    }
    int nl = 0;
    for (int i = 0; i < n; i++) {
        if (launch_of[i] >= 0) continue;
        int NT = own_nt[i];
        launch_of[i] = nl;
        for (int j = i + 1; merge && j < n; j++) {
            if (launch_of[j] >= 0 || !compatible(ps[i], ps[j])) continue;
            const int NT2 = std::max(NT, own_nt[j]);
            bool fits = true;
            if (merge == MRTS_GROUP_MERGE_FIT)
                for (int k = 0; k < n; k++)
                    if ((k == j || launch_of[k] == nl) && lds(ps[k], NT2) > kGroupLdsCap) fits = false;
            if (!fits) continue;
            launch_of[j] = nl;
            NT = NT2;
        }
        nl++;
    }
    return nl;
}

// A group call's error is recorded on the member it concerns AND on hs[0], the
// handle callers read mrts_last_error from (a failure of member i > 0
// used to leave hs[0]'s message empty or stale).
static int group_fail(mrts_vec *const *hs, int i, int code, const std::string &msg) {
    const std::string m = i > 0 ? msg + " (member " + std::to_string(i) + ")" : msg;
    if (hs && i >= 0 && hs[i]) hs[i]->err = m;
    if (hs && hs[0]) hs[0]->err = m;
    return code;
}

static int group_check(mrts_vec *const *hs, int32_t n, const mrts_step_io *io, int32_t policy, bool need_bound = true) {
    if (!hs || n < 1 || n > MRTS_STEP_GROUP_MAX) return fail(hs && n >= 1 ? hs[0] : nullptr, MRTS_EINVAL, "step_group: bad arguments");
    if ((policy & ~7) || (policy & 3) == 3) return group_fail(hs, 0, MRTS_EINVAL, "step_group: unknown policy bits");
    for (int i = 0; i < n; i++) {
        if (!hs[i]) return group_fail(hs, i, MRTS_EINVAL, "step_group: null handle");
        if ((need_bound && !bound(hs[i])) || (io && !io_ok(io[i], io[i].reward != nullptr)))
            return group_fail(hs, i, MRTS_ESTATE, "step_group: workspace not bound or null buffer");
        if (io && !actions_aligned(hs[i], io[i])) return group_fail(hs, i, MRTS_EINVAL, "step_group: packed action words must be 4-byte aligned");
        for (int j = 0; j < i; j++)
            if (hs[j] == hs[i]) return group_fail(hs, i, MRTS_EINVAL, "step_group: an engine listed twice");
        // int32 and float32 members only take separate launches; packed and dense obs are two formats of one
        // batch's obs list, which no caller means
        if ((hs[i]->obs_kind == MRTS_OBS_PACKED) != (hs[0]->obs_kind == MRTS_OBS_PACKED))
            return group_fail(hs, i, MRTS_EINVAL, "step_group: packed and dense obs engines in one group");
    }
    return MRTS_OK;
}

int mrts_step_group_plan(mrts_vec *const *hs, int32_t n, int32_t policy, int32_t *launch_of, int32_t *launches) {
    int rc = group_check(hs, n, nullptr, policy, false);   // a plan needs only the handles' configs
    if (rc) return rc;
    if (!launch_of || !launches) return fail(hs[0], MRTS_EINVAL, "step_group_plan: null output");
    EngineParams ps[MRTS_STEP_GROUP_MAX];
    int lo[MRTS_STEP_GROUP_MAX];
    for (int i = 0; i < n; i++) {
        ps[i] = EngineParams{};
        ps[i].HW = hs[i]->HW;
        ps[i].W = hs[i]->W;
        ps[i].partial_obs = hs[i]->partial_obs;
        ps[i].obs_kind = hs[i]->obs_kind;
        ps[i].fuse_bots = fused(hs[i]) ? 1 : 0;
    }
    *launches = group_plan(ps, n, policy, lo);
    for (int i = 0; i < n; i++) launch_of[i] = lo[i];
    return MRTS_OK;
}

// The one step path: n engines under a group policy.  Per member: its parameters, k_bot when
// the tick's bot decisions are not there yet, bot fusion; then the plan and, per launch, k_step
// and what it means for the members' masks_synced, obs_synced_ptr and bots_ready.  A failed bot or step
// launch clears that member's obs_synced_ptr and, while masks are bound, its masks_synced.  `what` opens the error text.
static int step_engines(mrts_vec *const *hs, int n, hipStream_t s, const mrts_step_io *io, int policy, const char *what) {
    EngineParams ps[MRTS_STEP_GROUP_MAX];
    for (int i = 0; i < n; i++) {
        mrts_vec *h = hs[i];
        ps[i] = step_params(h, io[i]);
        hipError_t e = h->bots_ready ? hipSuccess : mrts_engine_bots(&ps[i], s);
        if (e) {
            masks_written(h, e, false);
            obs_written(h, e, io[i].obs, false);
            return group_fail(hs, i, MRTS_EHIP, std::string(what) + " bot launch: " + hipGetErrorString(e));
        }
        h->bots_ready = true;   // this tick's decisions are in botpa now, whatever happens below
        ps[i].fuse_bots = fused(h) ? 1 : 0;
    }
    int launch_of[MRTS_STEP_GROUP_MAX];
    const int nl = group_plan(ps, n, policy, launch_of);
    for (int l = 0; l < nl; l++) {
        EngineParams grp[MRTS_STEP_GROUP_MAX];
        int m = 0, first = -1;
        for (int i = 0; i < n; i++)
            if (launch_of[i] == l) {
                if (first < 0) first = i;
                grp[m++] = ps[i];
            }
        hipError_t e = mrts_engine_step_group(grp, m, s, (policy & MRTS_GROUP_BOTS_FIRST) != 0);
        // not atomic: members of launches 0..l-1 have stepped, those of l.. have not
        // (include/microrts_amd.h); each member's mask and bot state follows its own launch
        for (int i = 0; i < n; i++)
            if (launch_of[i] == l) {
                masks_written(hs[i], e, !ps[i].mask_delta);
                obs_written(hs[i], e, io[i].obs, !ps[i].obs_delta);
                hs[i]->bots_ready = ps[i].fuse_bots != 0;   // a fused step decided the next tick's
            }
        if (e) return group_fail(hs, first, MRTS_EHIP, std::string(what) + " launch: " + hipGetErrorString(e));
    }
    return MRTS_OK;
}

int mrts_step(mrts_vec *h, void *stream, const int64_t *actions, const int32_t *source, void *obs, double *raw_reward,
              uint8_t *done) {
    const mrts_step_io io{actions, source, obs, raw_reward, done, nullptr, nullptr};
    if (!bound(h) || !io_ok(io, false)) return fail(h, MRTS_ESTATE, "step: workspace not bound or null buffer");
    if (!actions_aligned(h, io)) return fail(h, MRTS_EINVAL, "step: packed action words must be 4-byte aligned");
    return step_engines(&h, 1, (hipStream_t)stream, &io, MRTS_GROUP_BOTS_FIRST, "step");
}

int mrts_step_weighted(mrts_vec *h, void *stream, const int64_t *actions, const int32_t *source, void *obs,
                       double *raw_reward, uint8_t *done, double *reward, uint8_t *done0) {
    const mrts_step_io io{actions, source, obs, raw_reward, done, reward, done0};
    if (!bound(h) || !io_ok(io, true)) return fail(h, MRTS_ESTATE, "step_weighted: workspace not bound or null buffer");
    if (!actions_aligned(h, io)) return fail(h, MRTS_EINVAL, "step_weighted: packed action words must be 4-byte aligned");
    return step_engines(&h, 1, (hipStream_t)stream, &io, MRTS_GROUP_BOTS_FIRST, "step");
}

int mrts_step_group(mrts_vec *const *hs, int32_t n, void *stream, const mrts_step_io *io, int32_t policy) {
    int rc = group_check(hs, n, io, policy);
    if (rc) return rc;
    if (!io) return group_fail(hs, 0, MRTS_EINVAL, "step_group: null io");
    return step_engines(hs, n, (hipStream_t)stream, io, policy, "step_group");
}

// mrts_reset_games (maps: each listed game's new map) / mrts_park_games (maps == null): the
// whole list is validated before anything changes; then the host mirrors, the device's parked
// flags when one changed, the list into scratch, k_reset over it (a parked game writes zero
// obs / masks / sources) and a sync, for the host staging vector must outlive the copy.
static int reset_listed(mrts_vec *h, hipStream_t s, const int32_t *games, const int32_t *maps, int count, void *obs,
                        const std::string &what) {
    if (count == 0) return MRTS_OK;
    for (int i = 0; i < count; i++)
        if (games[i] < 0 || games[i] >= h->ngames || (maps && (maps[i] < 0 || maps[i] >= (int)h->maps.size())))
            return fail(h, MRTS_EINVAL, what + ": index out of range");
    const uint8_t park = maps ? 0 : 1;
    bool flags_changed = false;
    for (int i = 0; i < count; i++) {
        if (maps) h->game_map[games[i]] = maps[i];
        flags_changed |= h->parked[games[i]] != park;
        h->parked[games[i]] = park;
    }
    hipError_t e = flags_changed ? upload_parked(h, s) : hipSuccess;
    if (e) {
        h->obs_synced_ptr = nullptr;
        return hip_fail(h, e, (what + " parked flags upload").c_str());
    }
    h->scratch_host.assign(games, games + count);
    if (!maps) maps = games;   // (map list unused for parked games)
    h->scratch_host.insert(h->scratch_host.end(), maps, maps + count);
    int32_t *dg = (int32_t *)(h->ws + h->off_scratch);
    e = hipMemcpyAsync(dg, h->scratch_host.data(), sizeof(int32_t) * 2 * count, hipMemcpyHostToDevice, s);
    if (!e) {
        EngineParams p = out_params(h, obs);
        e = mrts_engine_reset(&p, s, dg, dg + count, count);
    }
    if (!e && !park) e = bots_after_reset(h, s, dg, count);
    const hipError_t es = hipStreamSynchronize(s);
    if (!e) e = es;
    masks_written(h, e, false);   // the listed games' rows only
    if (obs != h->obs_synced_ptr) h->obs_synced_ptr = nullptr;   // the games' rows in the remembered buffer are stale
    obs_written(h, e, obs, false);
    return e ? hip_fail(h, e, (what + " launch").c_str()) : MRTS_OK;
}

int mrts_reset_games(mrts_vec *h, void *stream, const int32_t *games, const int32_t *maps, int32_t count, void *obs) {
    if (!bound(h) || !obs || count < 0 || count > h->ngames || (count && (!games || !maps)))
        return fail(h, MRTS_EINVAL, "reset_games: bad arguments");
    return reset_listed(h, (hipStream_t)stream, games, maps, count, obs, "reset_games");
}

int mrts_add_map(mrts_vec *h, void *stream, const char *path, int32_t *index) {
    if (!bound(h) || !path || !index) return fail(h, MRTS_EINVAL, "add_map: not bound or null argument");
    for (size_t i = 0; i < h->map_path.size(); i++)
        if (h->map_path[i] == path) {
            *index = (int32_t)i;
            return MRTS_OK;
        }
    if ((int)h->maps.size() >= h->map_capacity) return fail(h, MRTS_EINVAL, "add_map: every map slot is taken (map_capacity)");
    MapData m;
    std::string err;
    if (!load_map(path, &m, &err)) return fail(h, MRTS_EIO, err);
    if (m.w != h->W || m.h != h->H)
        return fail(h, MRTS_EINVAL, "add_map: all maps of one vec env must share height x width (vec_env.py:149-150)");
    const int i = (int)h->maps.size();
    // a slot no game uses yet: nothing in flight reads it
    hipError_t e = upload_maps(h, (hipStream_t)stream, &m, i, 1);
    if (e) return hip_fail(h, e, "add_map upload");
    h->maps.push_back(std::move(m));
    h->map_path.emplace_back(path);
    h->base.nmaps = (int)h->maps.size();
    *index = i;
    return MRTS_OK;
}

int mrts_park_games(mrts_vec *h, void *stream, const int32_t *games, int32_t count, void *obs) {
    if (!bound(h) || !obs || count < 0 || count > h->ngames || (count && !games))
        return fail(h, MRTS_EINVAL, "park_games: bad arguments");
    return reset_listed(h, (hipStream_t)stream, games, nullptr, count, obs, "park_games");
}

// The samplers' and the action head's shared shape check: the kernels index the n * hw rows
// in 32 bits, a wave's 64-row group rounded up.
static bool sampler_rows_ok(int32_t n, int32_t hw) { return n >= 0 && hw >= 1 && (int64_t)n * hw <= (int64_t)INT32_MAX - 256; }
// The stand-in samplers write the action rows with 16-byte stores from an address derived
// from `actions` (the action head's sampler has a per-element path instead).
static bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

int mrts_sample_actions(void *stream, const int32_t *mask, int32_t n, int32_t hw, int32_t env0, uint64_t seed, uint32_t step,
                        int64_t *actions) {
    if (!mask || !actions || env0 < 0 || !sampler_rows_ok(n, hw) || !aligned16(actions)) return MRTS_EINVAL;
    return mrts_engine_sample(mask, n, hw, env0, seed, step, actions, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

int mrts_sample_actions_src(void *stream, const int32_t *mask, const int32_t *source, int32_t n, int32_t hw, int32_t env0,
                            uint64_t seed, uint32_t step, int64_t *actions) {
    if (!mask || !source || !actions || env0 < 0 || !sampler_rows_ok(n, hw) || !aligned16(actions)) return MRTS_EINVAL;
    return mrts_engine_sample_src(mask, source, n, hw, env0, seed, step, actions, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

static bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int mrts_sample_actions_src_packed(void *stream, const int32_t *mask, const int32_t *source, int32_t n, int32_t hw, int32_t env0,
                                   uint64_t seed, uint32_t step, int32_t *words) {
    if (!mask || !source || !words || env0 < 0 || !sampler_rows_ok(n, hw) || !aligned_to(words, 4)) return MRTS_EINVAL;
    return mrts_engine_sample_src_packed(mask, source, n, hw, env0, seed, step, words, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

// The action converters (mrts_sampler.hip): rows within the samplers' bound, each side aligned to its element.
static bool action_rows_ok(const void *actions, const void *words, int64_t rows) {
    return actions && words && rows >= 0 && rows <= (int64_t)INT32_MAX - 256 && aligned_to(actions, 8) && aligned_to(words, 4);
}
int mrts_pack_actions(void *stream, const int64_t *actions, int64_t rows, int32_t *words) {
    if (!action_rows_ok(actions, words, rows)) return MRTS_EINVAL;
    return mrts_engine_pack_actions(actions, rows, words, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}
int mrts_unpack_actions(void *stream, const int32_t *words, int64_t rows, int64_t *actions) {
    if (!action_rows_ok(actions, words, rows)) return MRTS_EINVAL;
    return mrts_engine_unpack_actions(words, rows, actions, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

// Episode statistics and GAE (mrts_rollout.hip): the reference's VecMonitor + MicroRTSStatsRecorder
// (ppo_gridnet.py:126-160, 384-385) and its advantage loop (ppo_gridnet.py:496-519) on the device.
static bool episode_shape_ok(int32_t n, int32_t capacity) { return n >= 1 && capacity >= 1; }
int64_t mrts_episode_stats_bytes(int32_t n, int32_t capacity) {
    if (!episode_shape_ok(n, capacity)) return MRTS_EINVAL;
    return mrts::rollout::layout(n, capacity).bytes;
}
int mrts_episode_stats_init(void *stream, void *state, int32_t n, int32_t capacity) {
    if (!episode_shape_ok(n, capacity) || !state || !aligned16(state)) return MRTS_EINVAL;
    return mrts_engine_episode_init(state, n, capacity, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}
int mrts_episode_stats_update(void *stream, void *state, int32_t n, int32_t capacity, double gamma, int64_t step, const double *reward,
                              const uint8_t *done0, const double *raw) {
    if (!episode_shape_ok(n, capacity) || !state || !aligned16(state) || step < 0 || !reward || !done0 || !raw ||
        !aligned_to(reward, 8) || !aligned_to(raw, 8))
        return MRTS_EINVAL;
    return mrts_engine_episode_update(state, n, capacity, gamma, step, reward, done0, raw, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}
int mrts_gae(void *stream, int32_t T, int32_t N, const float *rewards, const float *values, const void *dones, int32_t done_elem,
             const float *last_value, const void *last_done, double gamma, double lambda, int32_t mode, float *advantages,
             float *returns) {
    if (T < 1 || N < 1 || !rewards || !values || !dones || !last_value || !last_done || !advantages || !returns) return MRTS_EINVAL;
    if ((done_elem != MRTS_DONE_FLOAT32 && done_elem != MRTS_DONE_UINT8) || (mode != MRTS_GAE_ADVANTAGES && mode != MRTS_GAE_RETURNS))
        return MRTS_EINVAL;
    const uintptr_t da = done_elem == MRTS_DONE_FLOAT32 ? 4 : 1;
    if (!aligned_to(rewards, 4) || !aligned_to(values, 4) || !aligned_to(last_value, 4) || !aligned_to(advantages, 4) ||
        !aligned_to(returns, 4) || !aligned_to(dones, da) || !aligned_to(last_done, da))
        return MRTS_EINVAL;
    return mrts_engine_gae(T, N, rewards, values, dones, done_elem == MRTS_DONE_UINT8, last_value, last_done, (float)gamma,
                           (float)(gamma * lambda), mode, advantages, returns, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

int mrts_sample_actions_src_group(void *stream, const mrts_sample_seg *segs, int32_t nseg, uint64_t seed, uint32_t step) {
    if (!segs || nseg < 1 || nseg > MRTS_SAMPLE_GROUP_MAX) return MRTS_EINVAL;
    for (int k = 0; k < nseg; k++) {
        const mrts_sample_seg &q = segs[k];
        if (!q.mask || !q.source || !q.actions || q.env0 < 0 || !sampler_rows_ok(q.num_envs, q.hw) || !aligned16(q.actions))
            return MRTS_EINVAL;
    }
    return mrts_engine_sample_src_group(segs, nseg, seed, step, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

// The action head's entry points, dense (mask + source) and packed (the words, no source),
// over one check and one launcher each.
// `packed`: the mask format; `apacked`: the action format (0 / 1 each: formats_ok checked the public values).
static bool formats_ok(int32_t mask_format, int32_t action_format) {
    return (mask_format == MRTS_MASK_DENSE || mask_format == MRTS_MASK_PACKED) &&
           (action_format == MRTS_ACT_DENSE || action_format == MRTS_ACT_PACKED);
}
static bool actions_ok(int apacked, const void *actions) { return actions && ((uintptr_t)actions & (apacked ? 3u : 7u)) == 0; }
static int policy_sample(int packed, int apacked, void *stream, const float *logits, const int32_t *mask, const int32_t *source, int32_t n,
                         int32_t hw, int32_t env0, uint64_t seed, uint32_t step, void *actions, float *logprob, float *entropy) {
    if (!logits || !mask || (!packed && !source) || !actions_ok(apacked, actions) || !logprob || !entropy || env0 < 0 || !sampler_rows_ok(n, hw))
        return MRTS_EINVAL;
    return mrts_engine_policy_sample(packed, apacked, logits, mask, source, n, hw, env0, seed, step, actions, logprob, entropy,
                                     (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}
static int policy_evaluate(int packed, int apacked, void *stream, const float *logits, const int32_t *mask, const int32_t *source, int32_t n,
                           int32_t hw, const void *actions, float *logprob, float *entropy) {
    if (!logits || !mask || (!packed && !source) || !actions_ok(apacked, actions) || !logprob || !entropy || !sampler_rows_ok(n, hw))
        return MRTS_EINVAL;
    return mrts_engine_policy_eval(packed, apacked, logits, mask, source, n, hw, actions, logprob, entropy, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}
static int policy_evaluate_backward(int packed, int apacked, void *stream, const float *logits, const int32_t *mask, const int32_t *source,
                                    int32_t n, int32_t hw, const void *actions, const float *grad_logprob,
                                    const float *grad_entropy, float *grad_logits) {
    if (!logits || !mask || (!packed && !source) || !actions_ok(apacked, actions) || !grad_logprob || !grad_entropy || !grad_logits || !sampler_rows_ok(n, hw))
        return MRTS_EINVAL;
    return mrts_engine_policy_eval_bwd(packed, apacked, logits, mask, source, n, hw, actions, grad_logprob, grad_entropy, grad_logits,
                                       (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

int mrts_policy_sample(void *stream, const float *logits, const int32_t *mask, const int32_t *source, int32_t n, int32_t hw,
                       int32_t env0, uint64_t seed, uint32_t step, int64_t *actions, float *logprob, float *entropy) {
    return policy_sample(0, 0, stream, logits, mask, source, n, hw, env0, seed, step, actions, logprob, entropy);
}
int mrts_policy_sample_packed(void *stream, const float *logits, const int32_t *packed, int32_t n, int32_t hw, int32_t env0,
                              uint64_t seed, uint32_t step, int64_t *actions, float *logprob, float *entropy) {
    return policy_sample(1, 0, stream, logits, packed, nullptr, n, hw, env0, seed, step, actions, logprob, entropy);
}
int mrts_policy_evaluate(void *stream, const float *logits, const int32_t *mask, const int32_t *source, int32_t n, int32_t hw,
                         const int64_t *actions, float *logprob, float *entropy) {
    return policy_evaluate(0, 0, stream, logits, mask, source, n, hw, actions, logprob, entropy);
}
int mrts_policy_evaluate_packed(void *stream, const float *logits, const int32_t *packed, int32_t n, int32_t hw,
                                const int64_t *actions, float *logprob, float *entropy) {
    return policy_evaluate(1, 0, stream, logits, packed, nullptr, n, hw, actions, logprob, entropy);
}
int mrts_policy_evaluate_backward(void *stream, const float *logits, const int32_t *mask, const int32_t *source, int32_t n,
                                  int32_t hw, const int64_t *actions, const float *grad_logprob, const float *grad_entropy,
                                  float *grad_logits) {
    return policy_evaluate_backward(0, 0, stream, logits, mask, source, n, hw, actions, grad_logprob, grad_entropy, grad_logits);
}
int mrts_policy_evaluate_backward_packed(void *stream, const float *logits, const int32_t *packed, int32_t n, int32_t hw,
                                         const int64_t *actions, const float *grad_logprob, const float *grad_entropy,
                                         float *grad_logits) {
    return policy_evaluate_backward(1, 0, stream, logits, packed, nullptr, n, hw, actions, grad_logprob, grad_entropy, grad_logits);
}

// Both formats as arguments: `source` is read for dense masks only, `actions` is int64 rows or int32 words.
int mrts_policy_sample_fmt(void *stream, const float *logits, int32_t mask_format, const int32_t *mask, const int32_t *source, int32_t n,
                           int32_t hw, int32_t env0, uint64_t seed, uint32_t step, int32_t action_format, void *actions, float *logprob,
                           float *entropy) {
    if (!formats_ok(mask_format, action_format)) return MRTS_EINVAL;
    return policy_sample(mask_format == MRTS_MASK_PACKED, action_format == MRTS_ACT_PACKED, stream, logits, mask, source, n, hw, env0, seed,
                         step, actions, logprob, entropy);
}
int mrts_policy_evaluate_fmt(void *stream, const float *logits, int32_t mask_format, const int32_t *mask, const int32_t *source, int32_t n,
                             int32_t hw, int32_t action_format, const void *actions, float *logprob, float *entropy) {
    if (!formats_ok(mask_format, action_format)) return MRTS_EINVAL;
    return policy_evaluate(mask_format == MRTS_MASK_PACKED, action_format == MRTS_ACT_PACKED, stream, logits, mask, source, n, hw, actions,
                           logprob, entropy);
}
int mrts_policy_evaluate_backward_fmt(void *stream, const float *logits, int32_t mask_format, const int32_t *mask, const int32_t *source,
                                      int32_t n, int32_t hw, int32_t action_format, const void *actions, const float *grad_logprob,
                                      const float *grad_entropy, float *grad_logits) {
    if (!formats_ok(mask_format, action_format)) return MRTS_EINVAL;
    return policy_evaluate_backward(mask_format == MRTS_MASK_PACKED, action_format == MRTS_ACT_PACKED, stream, logits, mask, source, n, hw,
                                    actions, grad_logprob, grad_entropy, grad_logits);
}

int mrts_pack_masks(void *stream, const int32_t *mask, const int32_t *source, int32_t n, int32_t hw, int32_t *packed) {
    if (!mask || !source || !packed || !sampler_rows_ok(n, hw)) return MRTS_EINVAL;
    return mrts_engine_pack_masks(mask, source, (long long)n * hw, packed, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

int mrts_unpack_masks(void *stream, const int32_t *packed, int32_t n, int32_t hw, int32_t *mask, int32_t *source) {
    if (!packed || !mask || !source || !sampler_rows_ok(n, hw)) return MRTS_EINVAL;
    return mrts_engine_unpack_masks(packed, (long long)n * hw, mask, source, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

// The obs converters (mrts_obs.hip).  Per element type: its size, a stored one's bits, and the bits that make
// an element non-zero (a float's sign bit does not: -0.0 is zero).
namespace {
struct ObsElem {
    int bytes;
    uint32_t one, nonzero;
};
bool obs_elem(int32_t elem, ObsElem *e) {
    switch (elem) {
    case MRTS_ELEM_INT32: *e = {4, 1u, 0xffffffffu}; return true;
    case MRTS_ELEM_FLOAT32: *e = {4, 0x3f800000u, 0x7fffffffu}; return true;
    case MRTS_ELEM_FLOAT16: *e = {2, 0x3c00u, 0x7fffu}; return true;
    case MRTS_ELEM_BFLOAT16: *e = {2, 0x3f80u, 0x7fffu}; return true;
    }
    return false;
}
bool obs_args_ok(const void *packed, const void *obs, int64_t rows, int32_t planes, int32_t elem, ObsElem *e) {
    // (the samplers' row bound, 2^31 - 257: a grid below 2^23 workgroups of 256 rows)
    return packed && obs && rows >= 0 && rows <= 2147483391ll && (planes == 29 || planes == 31) && obs_elem(elem, e) &&
           ((uintptr_t)obs & (uintptr_t)(e->bytes - 1)) == 0 && ((uintptr_t)packed & 3u) == 0;
}
}  // namespace

int mrts_unpack_obs(void *stream, const int32_t *packed, int64_t rows, int32_t planes, int32_t elem, void *obs) {
    ObsElem e;
    if (!obs_args_ok(packed, obs, rows, planes, elem, &e)) return MRTS_EINVAL;
    return mrts_engine_unpack_obs(packed, rows, planes, e.bytes, e.one, obs, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

int mrts_pack_obs(void *stream, const void *obs, int64_t rows, int32_t planes, int32_t elem, int32_t *packed) {
    ObsElem e;
    if (!obs_args_ok(packed, obs, rows, planes, elem, &e)) return MRTS_EINVAL;
    return mrts_engine_pack_obs(obs, rows, planes, e.bytes, e.nonzero, packed, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

// The first encoder stage on the packed words (mrts_conv.hip): one shape check for the query and both launches.
static bool obs_conv_shape_ok(int32_t n, int32_t height, int32_t width, int32_t planes, int32_t channels) {
    return n >= 0 && height >= 1 && width >= 1 && (int64_t)height * width <= MRTS_MAX_HW && (planes == 29 || planes == 31) &&
           channels >= 1 && channels <= 64 && (int64_t)n * height * width <= 2147483391ll;
}

int64_t mrts_obs_conv_workspace_bytes(int32_t n, int32_t height, int32_t width, int32_t planes, int32_t channels) {
    if (!obs_conv_shape_ok(n, height, width, planes, channels)) return MRTS_EINVAL;
    const long long b = mrts_engine_obs_conv_workspace(n, height, width, planes, channels);
    return b < 0 ? MRTS_EINVAL : b;
}

int mrts_obs_conv_forward(void *stream, const int32_t *packed, int32_t n, int32_t height, int32_t width, int32_t planes,
                          const float *weight, const float *bias, int32_t channels, float *out) {
    if (!packed || !weight || !bias || !out || mrts_obs_conv_workspace_bytes(n, height, width, planes, channels) < 0) return MRTS_EINVAL;
    if (n == 0) return MRTS_OK;
    return mrts_engine_obs_conv_fwd(packed, n, height, width, planes, weight, bias, channels, out, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

int mrts_obs_conv_backward(void *stream, const int32_t *packed, int32_t n, int32_t height, int32_t width, int32_t planes,
                           const float *weight, const float *bias, int32_t channels, const float *grad_out,
                           void *workspace, int64_t workspace_bytes, float *grad_weight, float *grad_bias) {
    const int64_t need = mrts_obs_conv_workspace_bytes(n, height, width, planes, channels);
    if (!packed || !weight || !bias || !grad_out || !workspace || !grad_weight || !grad_bias || need < 0 || workspace_bytes < need ||
        !aligned16(workspace))
        return MRTS_EINVAL;
    if (n == 0) return MRTS_OK;
    return mrts_engine_obs_conv_bwd(packed, n, height, width, planes, weight, bias, channels, grad_out, (float *)workspace, grad_weight,
                                    grad_bias, (hipStream_t)stream) ? MRTS_EHIP : MRTS_OK;
}

int mrts_bind_mask_outputs(mrts_vec *h, int32_t *mask, int32_t *source) {
    if (!bound(h)) return fail(h, MRTS_ESTATE, "bind_mask_outputs: workspace not bound");
    if ((mask == nullptr) != (source == nullptr)) return fail(h, MRTS_EINVAL, "bind_mask_outputs: mask and source go together");
    if (mask && ((uintptr_t)mask & 15u)) return fail(h, MRTS_EINVAL, "bind_mask_outputs: mask must be 16-byte aligned");
    h->next_mask = mask;
    h->next_src = source;
    h->masks_synced = false;   // whatever the buffers hold is the caller's
    return MRTS_OK;
}

int mrts_render(mrts_vec *h, void *stream, int32_t env, uint8_t *rgb, int32_t size) {
    if (!bound(h) || !rgb) return fail(h, MRTS_ESTATE, "render: workspace not bound or rgb null");
    if (env < 0 || env >= h->nenvs) return fail(h, MRTS_EINVAL, "render: env out of range");
    if (size < h->W || size < h->H || size > 8192) return fail(h, MRTS_EINVAL, "render: size must be in [max(H, W), 8192]");
    const int game = env < h->nsp ? env / 2 : h->nsp / 2 + (env - h->nsp);
    hipError_t e = mrts_engine_render(&h->base, (hipStream_t)stream, game, h->game_map[game], size, rgb);
    return e ? hip_fail(h, e, "render launch") : MRTS_OK;
}

// Env-state checkpoint: [header | workspace bytes].  The header carries what the
// host holds beside the workspace (bots_ready, the games' map indices, parked flags),
// the shape the snapshot belongs to and a fingerprint of the configuration whose
// device tables the workspace copy brings along (bots, map templates): a snapshot
// loads only into a handle of the same shape AND configuration.
namespace {
struct StateHeader {
    uint32_t magic, version;
    int32_t ngames, HW, nmaps, bots_ready, parked_any;
    uint64_t total;
    uint64_t config;   // config_fingerprint
};
const uint32_t kStateMagic = 0x4d525453u;   // "MRTS"
const uint32_t kStateVersion = 3;
size_t state_header_bytes(const mrts_vec *h) {
    return align256(sizeof(StateHeader) + (size_t)h->ngames * (sizeof(int32_t) + 1));
}
struct Fnv {
    uint64_t v = 1469598103934665603ull;
    void bytes(const void *p, size_t n) {
        const unsigned char *b = (const unsigned char *)p;
        for (size_t i = 0; i < n; i++) v = (v ^ b[i]) * 1099511628211ull;
    }
    void i32(int32_t x) { bytes(&x, sizeof x); }
};
// FNV-1a over everything a workspace copy would carry in besides the game states:
// env split, obs layout, global game offset (bot RNG streams), the time limit, the
// bots of every bot env (both players), the map table's capacity and every map
// template (size, resources, walls, unit records).  Not the reward weights / shaping:
// the caller may reassign those between steps (vec_env.py reads reward_weight every step).
uint64_t config_fingerprint(const mrts_vec *h) {
    Fnv f;
    for (int32_t x : {h->nsp, h->nbot, h->partial_obs, h->obs_kind, h->game_offset, h->map_capacity, h->W, h->H,
                      h->max_steps})
        f.i32(x);
    f.i32((int32_t)h->bot_ai.size());
    f.bytes(h->bot_ai.data(), h->bot_ai.size() * sizeof(int32_t));
    f.i32((int32_t)h->bot_ai0.size());
    f.bytes(h->bot_ai0.data(), h->bot_ai0.size() * sizeof(int32_t));
    f.i32((int32_t)h->maps.size());
    for (const MapData &m : h->maps) {
        for (int32_t x : {m.w, m.h, m.res[0], m.res[1], m.nunits}) f.i32(x);
        f.bytes(m.wall.data(), m.wall.size());
        f.bytes(m.cells.data(), m.cells.size() * sizeof(int4));
    }
    return f.v;
}
}  // namespace

size_t mrts_state_bytes(const mrts_vec *h) { return bound(const_cast<mrts_vec *>(h)) ? state_header_bytes(h) + h->total : 0; }

int mrts_save_state(mrts_vec *h, void *stream, void *dst) {
    if (!bound(h) || !dst) return fail(h, MRTS_ESTATE, "save_state: workspace not bound or dst null");
    if (((uintptr_t)dst & 255u) != 0) return fail(h, MRTS_EINVAL, "save_state: dst must be 256-byte aligned");
    std::vector<unsigned char> hdr(state_header_bytes(h), 0);
    StateHeader sh{kStateMagic, kStateVersion, h->ngames, h->HW, (int32_t)h->maps.size(), h->bots_ready ? 1 : 0,
                   h->base.parked != nullptr ? 1 : 0, (uint64_t)h->total, config_fingerprint(h)};
    std::memcpy(hdr.data(), &sh, sizeof sh);
    std::memcpy(hdr.data() + sizeof sh, h->game_map.data(), (size_t)h->ngames * sizeof(int32_t));
    std::memcpy(hdr.data() + sizeof sh + (size_t)h->ngames * sizeof(int32_t), h->parked.data(), (size_t)h->ngames);
    hipStream_t s = (hipStream_t)stream;
    unsigned char *d = (unsigned char *)dst;
    hipError_t e = hipMemcpyAsync(d, hdr.data(), hdr.size(), hipMemcpyHostToDevice, s);
    if (!e) e = hipMemcpyAsync(d + hdr.size(), h->ws, h->total, hipMemcpyDeviceToDevice, s);
    // the host header buffer is this call's: drain the stream on every path (a queued
    // copy may still read it after a later enqueue failed)
    const hipError_t es = hipStreamSynchronize(s);
    if (!e) e = es;
    return e ? hip_fail(h, e, "save_state copy") : MRTS_OK;
}

int mrts_load_state(mrts_vec *h, void *stream, const void *src, void *obs) {
    if (!bound(h) || !src || !obs) return fail(h, MRTS_ESTATE, "load_state: workspace not bound or null buffer");
    if (((uintptr_t)src & 255u) != 0) return fail(h, MRTS_EINVAL, "load_state: src must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // the fixed header first: a snapshot of a smaller handle is shorter than this
    // handle's header, so nothing beyond sizeof(StateHeader) is read before it checks out
    StateHeader sh;
    hipError_t e = hipMemcpyAsync(&sh, src, sizeof sh, hipMemcpyDeviceToHost, s);
    if (!e) e = hipStreamSynchronize(s);
    if (e) return hip_fail(h, e, "load_state header");
    if (sh.magic != kStateMagic || sh.version != kStateVersion)
        return fail(h, MRTS_EINVAL, "load_state: not a snapshot of this library version (mrts_save_state)");
    if (sh.ngames != h->ngames || sh.HW != h->HW || sh.nmaps != (int32_t)h->maps.size() || sh.total != (uint64_t)h->total)
        return fail(h, MRTS_EINVAL, "load_state: the snapshot belongs to another configuration or map table");
    if (sh.config != config_fingerprint(h))
        return fail(h, MRTS_EINVAL, "load_state: the snapshot belongs to another configuration (bots, maps, obs layout, "
                                    "game offset or max_steps differ)");
    std::vector<unsigned char> hdr(state_header_bytes(h), 0);
    e = hipMemcpyAsync(hdr.data(), src, hdr.size(), hipMemcpyDeviceToHost, s);
    if (!e) e = hipStreamSynchronize(s);
    if (e) return hip_fail(h, e, "load_state header");
    e = hipMemcpyAsync(h->ws, (const unsigned char *)src + hdr.size(), h->total, hipMemcpyDeviceToDevice, s);
    h->masks_synced = false;   // the state is another one from here on, even if the copy failed
    h->obs_synced_ptr = nullptr;
    if (e) return hip_fail(h, e, "load_state copy");
    // the host mirrors only once the workspace copy is queued: a failed copy leaves them as they were
    std::memcpy(h->game_map.data(), hdr.data() + sizeof sh, (size_t)h->ngames * sizeof(int32_t));
    std::memcpy(h->parked.data(), hdr.data() + sizeof sh + (size_t)h->ngames * sizeof(int32_t), (size_t)h->ngames);
    h->bots_ready = sh.bots_ready != 0;
    h->base.parked = sh.parked_any ? (uint8_t *)(h->ws + h->off_parked) : nullptr;
    EngineParams p = out_params(h, obs);
    e = mrts_engine_outputs(&p, s);
    masks_written(h, e, true);
    obs_written(h, e, obs, true);
    return e ? hip_fail(h, e, "load_state outputs launch") : MRTS_OK;
}

// every game's genv words, read back and drained
static hipError_t read_genv(mrts_vec *h, void *stream, std::vector<int32_t> *genv) {
    genv->resize((size_t)h->ngames * MRTS_GENV_WORDS);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(genv->data(), h->ws + h->off_genv, genv->size() * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    return e ? e : hipStreamSynchronize(s);
}

int mrts_game_stats(mrts_vec *h, void *stream, int32_t *out) {
    if (!bound(h) || !out) return fail(h, MRTS_ESTATE, "game_stats: not bound or out null");
    std::vector<int32_t> genv;
    if (hipError_t e = read_genv(h, stream, &genv)) return hip_fail(h, e, "game_stats readback");
    static const int words[MRTS_GAME_STATS] = {MRTS_G_TIME, MRTS_G_STEPS, MRTS_G_TICKS, MRTS_G_SERIAL, MRTS_G_ORDERED, MRTS_G_EPISODES};
    for (int g = 0; g < h->ngames; g++)
        for (int k = 0; k < MRTS_GAME_STATS; k++) out[(size_t)g * MRTS_GAME_STATS + k] = genv[(size_t)g * MRTS_GENV_WORDS + words[k]];
    return MRTS_OK;
}

int mrts_error_flags(mrts_vec *h, void *stream, int32_t *flags_out) {
    if (!bound(h) || !flags_out) return fail(h, MRTS_ESTATE, "error_flags: not bound");
    std::vector<int32_t> genv;
    if (hipError_t e = read_genv(h, stream, &genv)) return hip_fail(h, e, "error_flags readback");
    int32_t f = 0;
    for (int g = 0; g < h->ngames; g++) f |= genv[(size_t)g * MRTS_GENV_WORDS + MRTS_G_ERR];
    *flags_out = f;
    return MRTS_OK;
}

int mrts_fused_layout_ok(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0 || width > 32 || height > 64) return -1;
    const int HW = width * height;
    const mrts_step_layout_t l = mrts_engine_step_layout(HW, width, 1, 0, 0);
    if (l.lds_bytes > MRTS_LDS_CAP_FUSED) return -1;
    if (mrts_engine_bot_lds_bytes(HW, width) > MRTS_LDS_CAP) return -1;   // mrts_create refuses such bot engines
    return l.early;
}

const char *mrts_utt_json(const mrts_vec *h) { return h ? h->utt.c_str() : ""; }
const char *mrts_last_error(const mrts_vec *h) { return h ? h->err.c_str() : "null handle"; }
void mrts_destroy(mrts_vec *h) { delete h; }

}  // extern "C"
