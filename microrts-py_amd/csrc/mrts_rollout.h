// mrts_rollout.h -- the episode-statistics buffer's layout (include/microrts_amd.h states it for callers)
// and the launchers of mrts_rollout.hip.  Shared by that unit and mrts_capi.cpp only.
#ifndef MRTS_ROLLOUT_H
#define MRTS_ROLLOUT_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "microrts_amd.h"

namespace mrts {
namespace rollout {

// gym_microrts/rollout.py `layout` and tests/rollout_ref.py restate these offsets and ROW: a change here is a change there
// (the library checks only the total size against the module's; tests/test_gpu_rollout.py compares every array).
// state: [header 32 B][ret f32 N][len i32 N][factor f64 N][rawsum f64 6 x N][disc f64 7 x N][pad to 16][ring capacity x 18 f64]
constexpr int HEADER_BYTES = 32;                    // int64 cnt[2], 16 reserved bytes
constexpr int ENV_BYTES = 4 + 4 + 8 + 6 * 8 + 7 * 8;   // 120
constexpr int ROW = MRTS_EPISODE_RECORD_DOUBLES;    // 18 doubles: 17 fields and a zero, rows 16-byte aligned
static_assert(ROW == 18 && (ROW * 8) % 16 == 0, "record rows are 16-byte aligned");

struct Layout {
    int64_t ret, len, factor, rawsum, disc, ring, bytes;   // byte offsets, and the whole size
};
__host__ __device__ inline Layout layout(int n, int capacity) {
    Layout L;
    L.ret = HEADER_BYTES;
    L.len = L.ret + 4ll * n;
    L.factor = L.len + 4ll * n;
    L.rawsum = L.factor + 8ll * n;
    L.disc = L.rawsum + 48ll * n;
    L.ring = (L.disc + 56ll * n + 15) & ~15ll;
    L.bytes = L.ring + (int64_t)capacity * ROW * 8;
    return L;
}

}  // namespace rollout
}  // namespace mrts

extern "C" {
// mrts_capi.cpp has checked the arguments: n, capacity, T >= 1, pointers non-null and aligned to their element,
// state 16-byte aligned, done_u8 / mode 0 or 1, step >= 0
hipError_t mrts_engine_episode_init(void *state, int n, int capacity, hipStream_t s);
hipError_t mrts_engine_episode_update(void *state, int n, int capacity, double gamma, long long step, const double *reward,
                                      const uint8_t *done0, const double *raw, hipStream_t s);
hipError_t mrts_engine_gae(int T, int n, const float *rewards, const float *values, const void *dones, int done_u8,
                           const float *last_value, const void *last_done, float g, float gl, int mode, float *adv, float *ret,
                           hipStream_t s);
}
#endif
