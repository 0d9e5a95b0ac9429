// mrts_rollout.hip -- the bookkeeping of a rollout on the tensor contract, on the device:
//   k_episode_update: per env-step, VecMonitor's episode return / length and MicroRTSStatsRecorder's
//     per-reward-function sums (ppo_gridnet.py:126-160, 384-385), with one record per finished episode
//     appended to a ring in the reference's scan order (ascending env within a call, call order across);
//   k_gae: GAE advantages and returns, or plain discounted returns (ppo_gridnet.py:496-519), one launch
//     for the whole [T][N] buffer.
// The arithmetic contract is include/microrts_amd.h's: every operation rounded on its own, none fused.
//
// Record positions without atomics or inter-workgroup traffic: every workgroup counts the set done0 bytes
// of ALL envs (at most N bytes from L2: 8 KB at 8192 envs) -- those before its own envs give its base, all of
// them the call's total -- and adds the in-block ballot prefix.  The counter of records since creation is
// double-buffered by the call's serial number: a launch reads cnt[step & 1] and workgroup 0 writes
// cnt[(step + 1) & 1], so no workgroup reads a value its own launch wrote.  When one call finishes more
// episodes than the ring holds, only the last `capacity` of them are written: no two lanes of a launch
// write one row, and the result is the same on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrts_rollout.h"

#pragma clang fp contract(off)   // no fused multiply-adds anywhere in this unit: the contract is numpy's and torch's op by op

namespace mrts {
namespace rollout {

constexpr int ET = 256;   // k_episode_update / k_episode_init: lanes per workgroup = envs per workgroup
constexpr int GT = 64;    // k_gae: one wave per workgroup, so 8192 envs spread over 128 CUs
constexpr int GU = 8;     // k_gae: time steps whose loads are issued together, one chunk ahead of the recurrence

// every 8-byte word of the buffer: zero, or 1.0 in the factor array
__global__ __launch_bounds__(ET) void k_episode_init(uint64_t* __restrict__ state, int n, int capacity) {
    const Layout L = layout(n, capacity);
    const int64_t words = L.bytes / 8, f0 = L.factor / 8, f1 = L.rawsum / 8;
    for (int64_t w = (int64_t)blockIdx.x * ET + threadIdx.x; w < words; w += (int64_t)gridDim.x * ET)
        state[w] = (w >= f0 && w < f1) ? 0x3ff0000000000000ull : 0ull;
}

// the number of non-zero bytes of x
__device__ __forceinline__ int nonzero_bytes(uint64_t x) {
    const uint64_t low7 = 0x7f7f7f7f7f7f7f7full;
    return __popcll((((x & low7) + low7) | x) & ~low7);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(ET) void k_episode_update(uint8_t* __restrict__ state, int n, int capacity, double gamma, long long step,
                                                       const double* __restrict__ reward, const uint8_t* __restrict__ done0,
                                                       const double* __restrict__ raw) {
    __shared__ int s_before[ET / 64], s_total[ET / 64], s_done[ET / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int own0 = blockIdx.x * ET, env = own0 + tid;
    const Layout L = layout(n, capacity);
    int64_t* cnt = reinterpret_cast<int64_t*>(state);
    const int64_t base = cnt[step & 1];

    // the set done0 bytes of the envs before this workgroup's, and of all envs
    int before = 0, total = 0;
    int i0 = 0;
    if (((uintptr_t)done0 & 7u) == 0) {   // own0 is a multiple of 8: no word straddles it
        const uint64_t* dw = reinterpret_cast<const uint64_t*>(done0);
        const int nw = n >> 3;
        for (int w = tid; w < nw; w += ET) {
            const int c = nonzero_bytes(dw[w]);
            total += c;
            before += (w << 3) < own0 ? c : 0;
        }
        i0 = nw << 3;
    }
    for (int i = i0 + tid; i < n; i += ET) {
        const int c = done0[i] != 0;
        total += c;
        before += i < own0 ? c : 0;
    }
    const bool in = env < n;
    const bool d = in && done0[env] != 0;
    const unsigned long long ball = __ballot(d);
    before = wave_sum(before);
    total = wave_sum(total);
    if (lane == 0) {
        s_before[wave] = before;
        s_total[wave] = total;
        s_done[wave] = __popcll(ball);
    }
    __syncthreads();
    before = total = 0;
    int mine = __popcll(ball & ((1ull << lane) - 1ull));   // finished envs of this workgroup before this one
#pragma unroll
    for (int w = 0; w < ET / 64; w++) {
        before += s_before[w];
        total += s_total[w];
        mine += w < wave ? s_done[w] : 0;
    }
    if (blockIdx.x == 0 && tid == 0) cnt[(step + 1) & 1] = base + total;
    if (!in) return;

    float* p_ret = reinterpret_cast<float*>(state + L.ret) + env;
    int32_t* p_len = reinterpret_cast<int32_t*>(state + L.len) + env;
    double* p_factor = reinterpret_cast<double*>(state + L.factor) + env;
    double* p_rawsum = reinterpret_cast<double*>(state + L.rawsum) + env;   // [6][n]
    double* p_disc = reinterpret_cast<double*>(state + L.disc) + env;       // [7][n]

    double x[6], rawsum[6], disc[7];
#pragma unroll
    for (int k = 0; k < 6; k++) x[k] = raw[(size_t)env * 6 + k];
    float ret = (float)((double)*p_ret + reward[env]);
    int32_t len = *p_len + 1;
    double factor = *p_factor;
#pragma unroll
    for (int k = 0; k < 6; k++) rawsum[k] = p_rawsum[(size_t)k * n] + x[k];
    const double tot = ((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) + x[5];
#pragma unroll
    for (int k = 0; k < 6; k++) disc[k] = p_disc[(size_t)k * n] + factor * x[k];
    disc[6] = p_disc[(size_t)6 * n] + factor * tot;
    factor = factor * gamma;

    if (d) {
        const int idx = before + mine;            // this episode's place among the call's finished ones
        if (idx >= total - capacity) {            // one of the call's last `capacity`: rows of one launch are distinct
            double* row = reinterpret_cast<double*>(state + L.ring) + ((base + idx) % capacity) * ROW;
            row[0] = (double)env;
            row[1] = (double)step;
            row[2] = (double)ret;
            row[3] = (double)len;
#pragma unroll
            for (int k = 0; k < 6; k++) row[4 + k] = rawsum[k];
#pragma unroll
            for (int k = 0; k < 7; k++) row[10 + k] = disc[k];
            row[17] = 0.0;
        }
        ret = 0.f;
        len = 0;
        factor = 1.0;
#pragma unroll
        for (int k = 0; k < 6; k++) rawsum[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) disc[k] = 0.0;
    }
    *p_ret = ret;
    *p_len = len;
    *p_factor = factor;
#pragma unroll
    for (int k = 0; k < 6; k++) p_rawsum[(size_t)k * n] = rawsum[k];
#pragma unroll
    for (int k = 0; k < 7; k++) p_disc[(size_t)k * n] = disc[k];
}

__device__ __forceinline__ float done_value(float d) { return d; }
__device__ __forceinline__ float done_value(uint8_t d) { return (float)d; }

// One lane per env walks t = T - 1 .. 0.  An iteration's three loads do not depend on the recurrence:
// they are issued GU time steps at a time, one chunk ahead of the chunk being computed (rows below
// t = 0 re-read row 0, so no load sits behind a branch).  MODE 0: GAE; MODE 1: discounted returns.
template <typename DT, int MODE>
__global__ __launch_bounds__(GT) void k_gae(int T, int n, const float* __restrict__ rewards, const float* __restrict__ values,
                                            const DT* __restrict__ dones, const float* __restrict__ last_value,
                                            const DT* __restrict__ last_done, float g, float gl, float* __restrict__ adv,
                                            float* __restrict__ ret) {
    const int e = blockIdx.x * GT + threadIdx.x;
    if (e >= n) return;
    float v_next = last_value[e], d_next = done_value(last_done[e]);
    float carry = MODE == 0 ? 0.f : v_next;   // A_{t+1}, or R_{t+1}
    float r[GU], v[GU], d[GU], rn[GU], vn[GU], dn[GU];
    auto load = [&](int t0, float (&lr)[GU], float (&lv)[GU], float (&ld)[GU]) {
#pragma unroll
        for (int i = 0; i < GU; i++) {
            const int t = t0 - 1 - i;
            const size_t at = (size_t)(t < 0 ? 0 : t) * n + e;
            lr[i] = rewards[at];
            lv[i] = values[at];
            ld[i] = done_value(dones[at]);
        }
    };
    load(T, r, v, d);
    for (int t0 = T; t0 > 0; t0 -= GU) {
        load(t0 - GU, rn, vn, dn);   // behind the last chunk: row 0 again, unused
#pragma unroll
        for (int i = 0; i < GU; i++) {
            const int t = t0 - 1 - i;
            if (t < 0) break;
            const size_t at = (size_t)t * n + e;
            const float nnt = 1.0f - d_next;
            if (MODE == 0) {
                const float delta = (r[i] + (g * v_next) * nnt) - v[i];
                carry = delta + (gl * nnt) * carry;
                adv[at] = carry;
                ret[at] = carry + v[i];
            } else {
                carry = r[i] + (g * nnt) * carry;
                ret[at] = carry;
                adv[at] = carry - v[i];
            }
            v_next = v[i];
            d_next = d[i];
        }
#pragma unroll
        for (int i = 0; i < GU; i++) {
            r[i] = rn[i];
            v[i] = vn[i];
            d[i] = dn[i];
        }
    }
}

}  // namespace rollout
}  // namespace mrts

// The launchers take the caller's stream, allocate nothing and synchronise nothing.
extern "C" {
using namespace mrts::rollout;
hipError_t mrts_engine_episode_init(void* state, int n, int capacity, hipStream_t s) {
    const int64_t words = layout(n, capacity).bytes / 8;
    const unsigned grid = (unsigned)((words + ET - 1) / ET < 2048 ? (words + ET - 1) / ET : 2048);
    hipLaunchKernelGGL(k_episode_init, dim3(grid), dim3(ET), 0, s, reinterpret_cast<uint64_t*>(state), n, capacity);
    return hipGetLastError();
}
hipError_t mrts_engine_episode_update(void* state, int n, int capacity, double gamma, long long step, const double* reward,
                                      const uint8_t* done0, const double* raw, hipStream_t s) {
    hipLaunchKernelGGL(k_episode_update, dim3((unsigned)((n + ET - 1) / ET)), dim3(ET), 0, s, reinterpret_cast<uint8_t*>(state), n,
                       capacity, gamma, step, reward, done0, raw);
    return hipGetLastError();
}
hipError_t mrts_engine_gae(int T, int n, const float* rewards, const float* values, const void* dones, int done_u8,
                           const float* last_value, const void* last_done, float g, float gl, int mode, float* adv, float* ret,
                           hipStream_t s) {
    const dim3 grid((unsigned)((n + GT - 1) / GT)), block(GT);
#define MRTS_GAE_LAUNCH(DT, MODE)                                                                                                 \
    hipLaunchKernelGGL((k_gae<DT, MODE>), grid, block, 0, s, T, n, rewards, values, reinterpret_cast<const DT*>(dones), last_value, \
                       reinterpret_cast<const DT*>(last_done), g, gl, adv, ret)
    if (done_u8) {
        if (mode == 0) MRTS_GAE_LAUNCH(uint8_t, 0);
        else MRTS_GAE_LAUNCH(uint8_t, 1);
    } else {
        if (mode == 0) MRTS_GAE_LAUNCH(float, 0);
        else MRTS_GAE_LAUNCH(float, 1);
    }
#undef MRTS_GAE_LAUNCH
    return hipGetLastError();
}
}
