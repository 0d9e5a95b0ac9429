// mrts_policy.hip -- the masked action head of a GridNet policy: the reference's
// CategoricalMasked per action component (experiments/ppo_gridnet.py:164-167, 215-247)
// as three launches -- sample, evaluate, and evaluate's backward to the logits.
//
// Per row (env e, cell c) and component k (offsets and lengths: mrts_actions.h), with
// V = the entries the mask allows (none when source == 0):
//   V empty : log-prob 0, entropy 0, gradient 0 (the reference's float32 result:
//             -1e8 + log L rounds to -1e8, the normalised logits are 0); the sampled
//             action is the stand-in sampler's no-valid-entry draw (draw_uniform, mrts_actions.h).
//   else    : M = max_V l, E_j = expf(l_j - M), S = sum_V E_j (float32, ascending j),
//             log p_a = (l_a - M) - logf(S) for a in V, exactly -1e8f for any other a
//             (out-of-range ones included: they are compared, never used as an index);
//             entropy H = logf(S) - (sum_V E_j (l_j - M)) / S  (= -sum_V p_j log p_j);
//             sampling: u = (r[k] >> 8) * 2^-24, the first j in V whose running sum
//             exceeds u * S, the last j in V if rounding leaves none.
// r[0..6] are philox_row's words (mrts_philox.h): the stand-in sampler's stream, exact
// under sharding by env0.
//
// Mapping: one workgroup per env, a wave per 64 consecutive cells.  The wave ballots the
// source word of its 64 rows and folds the source rows (getMasks leaves a few per cent
// of the rows with one) one after another, channel k on lane k: two coalesced loads
// each for the mask and the logits, the next source row's loads in flight while this
// one is folded.  The row goes through the wave's LDS slice in four steps: lane k < 7
// takes component k's max; every lane takes its channels' expf; lane k < 7 adds
// component k's S and T over the valid entries in ascending j (the order the contract
// above states -- a cross-lane scan would add in another order), picks or checks the
// action and keeps the component's log-prob and entropy; for the backward every lane
// then stores its channels' gradient, coalesced.  48-64 VGPRs, 8 waves per SIMD.
// Measured against one lane per source row with its 78 channels unrolled into registers
// (240 VGPRs; 168 and 3 waves per SIMD at its best): 8192 envs of 16x16, launch alone,
// sample 60 -> 28 us, evaluate 36 -> 16 us (profiles/policy_head/ab_fold.json).
// Per-env log-prob and entropy: lane k adds its component over the wave's rows in
// float64 in row order, then a wave shuffle, then LDS across the waves, rounded once
// to float32 -- no floating-point atomics, so two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrts_actions.h"
#include "mrts_engine.h"
#include "mrts_layout.h"
#include "mrts_philox.h"

namespace mrts {
namespace policy {

constexpr int PW = 4;          // waves per workgroup
constexpr int PT = 64 * PW;
constexpr float LP_INVALID = -1.0e8f;
static_assert(MRTS_MASK_CH > 64 && MRTS_MASK_CH <= 80, "a row is channels lane and 64 + lane of one wave; WaveRow holds 80");
static_assert(ACT_OFF[ACT_ATTACK_CELL] <= 64 && ACT_COMPONENTS <= 8, "channels 64.. are the last component's; 8 per-component slots");

enum Mode { SAMPLE, EVAL, BWD };

// the source row a wave is folding (its LDS slice)
struct WaveRow {
    float l[80], E[80];                // the row's logits and exp(l - M) (0 where masked)
    float M[8], S[8], logS[8], H[8];   // per component
    int a[8];                          // BWD: the component's action if it is a valid entry, -1 otherwise
    uint32_t rk[8];                    // SAMPLE: the row's Philox words
};

// a source row's words as loaded: channels lane and 64 + lane (lanes >= 14 re-read channel
// 77 and ignore it), and lane k < 7's action of component k (EVAL / BWD)
struct RowRegs {
    int m0, m1;
    float l0, l1;
    long long a;
};
template <Mode MODE>
__device__ __forceinline__ void load_row(RowRegs& R, size_t row, const int32_t* __restrict__ mask, const float* __restrict__ logits,
                                         const int64_t* __restrict__ act, int lane) {
    const int32_t* m = mask + row * MRTS_MASK_CH;
    const float* l = logits + row * MRTS_MASK_CH;
    const int c1 = 64 + min(lane, MRTS_MASK_CH - 65);   // unconditional loads: the compiler counts them, the next row's stay in flight
    R.m0 = m[lane];
    R.l0 = l[lane];
    R.m1 = m[c1];
    R.l1 = l[c1];
    R.a = MODE == SAMPLE ? 0 : act[row * 7 + min(lane, 6)];
}

// Fold one source row (wave-uniform index r of the wave's 64 rows).  SAMPLE: the picks
// go to s_out[r * 7 + k] over the no-valid-entry draw already there.  BWD: the valid
// channels' gradient goes to g (the masked ones keep the +0.0f of the fill).
template <Mode MODE>
__device__ __forceinline__ void fold_row(const RowRegs& R, int r, int lane, WaveRow& W, const uint32_t (&r8)[8], int64_t* __restrict__ s_out,
                                         double& slp, double& sent, float g_lp, float g_ent, float* __restrict__ g) {
#pragma clang fp contract(off)   // no fused multiply-adds: sample, evaluate and the backward round alike, bit for bit
    const bool hi = lane < MRTS_MASK_CH - 64;
    const uint64_t vlo = __ballot(R.m0 != 0), vhi = __ballot(hi && R.m1 != 0);
    W.l[lane] = R.l0;
    if (hi) W.l[64 + lane] = R.l1;
    if (MODE == SAMPLE && lane == r) {
#pragma unroll
        for (int k = 0; k < 7; k++) W.rk[k] = r8[k];
    }
    const int k = min(lane, 7), off = comp_off(k), len = comp_len(k);
    const uint64_t seg = comp_bits(vlo, vhi, off, len);   // component k's valid entries as bits (lanes >= 7: none)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    float M = -INFINITY;
    for (uint64_t b = seg; b; b &= b - 1ull) M = fmaxf(M, W.l[off + __builtin_ctzll(b)]);   // the valid entries only: few on real masks
    if (lane < 7) W.M[lane] = M;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int c0 = comp_of(lane), c1 = ACT_ATTACK_CELL;   // channels 64.. belong to the last component
    const bool v0 = (vlo >> lane) & 1, v1 = hi && ((vhi >> lane) & 1);
    const float d0 = R.l0 - W.M[c0], d1 = R.l1 - W.M[c1];
    const float E0 = v0 ? expf(d0) : 0.0f, E1 = v1 ? expf(d1) : 0.0f;
    W.E[lane] = E0;
    if (hi) W.E[64 + lane] = E1;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (seg != 0) {   // lane k < 7 with valid entries
        float S = 0.0f, T = 0.0f;
        for (uint64_t b = seg; b; b &= b - 1ull) {   // ascending j
            const int j = __builtin_ctzll(b);
            const float e = W.E[off + j];
            S += e;
            T += e * (W.l[off + j] - M);
        }
        long long a = R.a;
        if (MODE == SAMPLE) {
            const float th = (float)(W.rk[k] >> 8) * 0x1p-24f * S;
            float C = 0.0f;
            int pick = -1, last = 0;
            for (uint64_t b = seg; b && pick < 0; b &= b - 1ull) {
                last = __builtin_ctzll(b);
                C += W.E[off + last];
                if (C > th) pick = last;
            }
            a = pick < 0 ? last : pick;
            s_out[r * 7 + k] = a;
        }
        const bool ok = a >= 0 && a < len && ((seg >> a) & 1);   // compared first: an invalid action is never an index
        const float logS = logf(S);
        const float lp = ok ? (W.l[off + (ok ? (int)a : 0)] - M) - logS : LP_INVALID;
        const float H = logS - T / S;
        slp += (double)lp;
        sent += (double)H;
        if (MODE == BWD) {
            W.S[k] = S;
            W.logS[k] = logS;
            W.H[k] = H;
            W.a[k] = ok ? (int)a : -1;
        }
    }
    if (MODE == BWD) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (v0) {
            const float p = E0 / W.S[c0], logp = d0 - W.logS[c0];
            g[lane] = g_lp * ((W.a[c0] == lane - comp_off(c0) ? 1.0f : 0.0f) - p) - g_ent * p * (logp + W.H[c0]);
        }
        if (v1) {
            const float p = E1 / W.S[c1], logp = d1 - W.logS[c1];
            g[64 + lane] = g_lp * ((W.a[c1] == 64 + lane - comp_off(c1) ? 1.0f : 0.0f) - p) - g_ent * p * (logp + W.H[c1]);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the next row rewrites W
}

// The source rows `pending` (bits of the wave's 64 rows from row0) in ascending order,
// the next row's loads issued before the current one is folded.
template <Mode MODE>
__device__ __forceinline__ void fold_rows(uint64_t pending, size_t row0, int lane, const float* __restrict__ logits,
                                          const int32_t* __restrict__ mask, const int64_t* __restrict__ act, WaveRow& W,
                                          const uint32_t (&r8)[8], int64_t* __restrict__ s_out, double& slp, double& sent, float g_lp,
                                          float g_ent, float* __restrict__ grad) {
    if (!pending) return;
    int r = __builtin_ctzll(pending);
    pending &= pending - 1ull;
    RowRegs cur;
    load_row<MODE>(cur, row0 + r, mask, logits, act, lane);
    while (true) {
        const bool more = pending != 0;
        const int rn = more ? __builtin_ctzll(pending) : r;   // none left: a harmless re-read
        pending &= pending - 1ull;
        RowRegs nxt;
        load_row<MODE>(nxt, row0 + rn, mask, logits, act, lane);
        fold_row<MODE>(cur, r, lane, W, r8, s_out, slp, sent, g_lp, g_ent, MODE == BWD ? grad + (row0 + r) * MRTS_MASK_CH : nullptr);
        if (!more) break;
        cur = nxt;
        r = rn;
    }
}

// The env's two sums: wave shuffle (a fixed butterfly), LDS across the waves in wave
// order, one rounding to float32.  Every thread of the workgroup calls it.
__device__ __forceinline__ void reduce_env(double slp, double sent, float* __restrict__ logprob, float* __restrict__ entropy, int e) {
    __shared__ double s_red[2][PW];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        slp += __shfl_xor(slp, o);
        sent += __shfl_xor(sent, o);
    }
    if ((threadIdx.x & 63) == 0) {
        s_red[0][threadIdx.x >> 6] = slp;
        s_red[1][threadIdx.x >> 6] = sent;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int w = 0; w < PW; w++) {
            a += s_red[0][w];
            b += s_red[1][w];
        }
        logprob[e] = (float)a;
        entropy[e] = (float)b;
    }
}

// logits [N][HW][78] f32, mask [N][HW][78] i32, src [N][HW] i32 -> act [N][HW][7] i64
// (every row: a non-source row gets the no-valid-entry draw of all seven components),
// logprob [N] f32, entropy [N] f32.  A wave stages its 64 rows' actions in LDS and
// writes them with 16-byte stores when the env's first row is 16-byte aligned (56-byte
// rows: an odd hw with an odd env is not), per element otherwise.
__global__ __launch_bounds__(PT) void k_policy_sample(const float* __restrict__ logits, const int32_t* __restrict__ mask,
                                                      const int32_t* __restrict__ src, int hw, int env0, uint64_t seed, uint32_t step,
                                                      int64_t* __restrict__ act, float* __restrict__ logprob,
                                                      float* __restrict__ entropy) {
    __shared__ __attribute__((aligned(16))) int64_t s_out[PW][64 * 7];
    __shared__ WaveRow s_row[PW];
    const int e = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t base = (size_t)e * hw;
    const bool al16 = ((uintptr_t)(act + base * 7) & 15u) == 0;   // + 64 * 56 B per group keeps it
    double slp = 0.0, sent = 0.0;
    for (int c0 = w * 64; c0 < hw; c0 += PT) {
        const int rb = min(64, hw - c0);
        const bool in = lane < rb;
        const int s_raw = src[base + c0 + min(lane, rb - 1)];   // unconditional (tail lanes re-read the last row): the Philox words are drawn behind it
        uint32_t r8[8];
        philox_row(env0 + e, c0 + lane, seed, step, r8);
        if (in) {
#pragma unroll
            for (int k = 0; k < ACT_COMPONENTS; k++) s_out[w][lane * 7 + k] = draw_uniform(r8[k], ACT_LEN[k]);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        fold_rows<SAMPLE>(__ballot(in && s_raw != 0), base + c0, lane, logits, mask, nullptr, s_row[w], r8, s_out[w], slp, sent, 0.0f, 0.0f,
                          nullptr);
        int64_t* ob = act + (base + c0) * 7;
        const int onel = rb * 7;
        if (al16) {
            const int onv = onel >> 1;
            int4* o4 = reinterpret_cast<int4*>(ob);
            const int4* s4 = reinterpret_cast<const int4*>(s_out[w]);
            for (int k = lane; k < onv; k += 64) o4[k] = s4[k];
            if ((onel & 1) && lane == 0) ob[onel - 1] = s_out[w][onel - 1];
        } else {
            for (int k = lane; k < onel; k += 64) ob[k] = s_out[w][k];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the next group rewrites s_out[w]
    }
    reduce_env(slp, sent, logprob, entropy, e);
}

// The same inputs + the caller's actions -> logprob [N], entropy [N].
__global__ __launch_bounds__(PT) void k_policy_eval(const float* __restrict__ logits, const int32_t* __restrict__ mask,
                                                    const int32_t* __restrict__ src, int hw, const int64_t* __restrict__ act,
                                                    float* __restrict__ logprob, float* __restrict__ entropy) {
    __shared__ WaveRow s_row[PW];
    const int e = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t base = (size_t)e * hw;
    const uint32_t r8[8] = {};
    double slp = 0.0, sent = 0.0;
    for (int c0 = w * 64; c0 < hw; c0 += PT) {
        const int rb = min(64, hw - c0);
        const int s_raw = src[base + c0 + min(lane, rb - 1)];
        fold_rows<EVAL>(__ballot(lane < rb && s_raw != 0), base + c0, lane, logits, mask, act, s_row[w], r8, nullptr, slp, sent, 0.0f, 0.0f,
                        nullptr);
    }
    reduce_env(slp, sent, logprob, entropy, e);
}

// k_policy_eval's inputs + g_lp [N], g_ent [N] -> grad [N][HW][78] f32, all of it: the
// workgroup fills its env's rows with +0.0f (16-byte stores when the env's first row
// is 16-byte aligned -- 312-byte rows: an odd hw with an odd env is not -- per element
// otherwise), then the waves store the source rows' valid channels over the fill.
__global__ __launch_bounds__(PT) void k_policy_eval_bwd(const float* __restrict__ logits, const int32_t* __restrict__ mask,
                                                        const int32_t* __restrict__ src, int hw, const int64_t* __restrict__ act,
                                                        const float* __restrict__ g_lp, const float* __restrict__ g_ent,
                                                        float* __restrict__ grad) {
    __shared__ WaveRow s_row[PW];
    const int e = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t base = (size_t)e * hw;
    float* gb = grad + base * MRTS_MASK_CH;
    const int nel = hw * MRTS_MASK_CH;   // <= 1128 * 78
    if (((uintptr_t)gb & 15u) == 0) {
        const int nv = nel >> 2;
        float4* g4 = reinterpret_cast<float4*>(gb);
        for (int k = threadIdx.x; k < nv; k += PT) g4[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int k = 4 * nv + threadIdx.x; k < nel; k += PT) gb[k] = 0.0f;
    } else {
        for (int k = threadIdx.x; k < nel; k += PT) gb[k] = 0.0f;
    }
    __syncthreads();   // the fill is complete (and ordered) before a row's values land on it
    const float glp = g_lp[e], gent = g_ent[e];
    const uint32_t r8[8] = {};
    double slp = 0.0, sent = 0.0;
    for (int c0 = w * 64; c0 < hw; c0 += PT) {
        const int rb = min(64, hw - c0);
        const int s_raw = src[base + c0 + min(lane, rb - 1)];
        fold_rows<BWD>(__ballot(lane < rb && s_raw != 0), base + c0, lane, logits, mask, act, s_row[w], r8, nullptr, slp, sent, glp, gent,
                       grad);
    }
}

}  // namespace policy
}  // namespace mrts

// The launchers take the caller's stream, allocate nothing and synchronise nothing.
extern "C" {
hipError_t mrts_engine_policy_sample(const float* logits, const int32_t* mask, const int32_t* src, int n, int hw, int env0,
                                     uint64_t seed, uint32_t step, int64_t* act, float* logprob, float* entropy, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mrts::policy::k_policy_sample, dim3((unsigned)n), dim3(mrts::policy::PT), 0, s, logits, mask, src, hw, env0, seed,
                       step, act, logprob, entropy);
    return hipGetLastError();
}
hipError_t mrts_engine_policy_eval(const float* logits, const int32_t* mask, const int32_t* src, int n, int hw, const int64_t* act,
                                   float* logprob, float* entropy, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mrts::policy::k_policy_eval, dim3((unsigned)n), dim3(mrts::policy::PT), 0, s, logits, mask, src, hw, act, logprob,
                       entropy);
    return hipGetLastError();
}
hipError_t mrts_engine_policy_eval_bwd(const float* logits, const int32_t* mask, const int32_t* src, int n, int hw, const int64_t* act,
                                       const float* g_lp, const float* g_ent, float* grad, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mrts::policy::k_policy_eval_bwd, dim3((unsigned)n), dim3(mrts::policy::PT), 0, s, logits, mask, src, hw, act, g_lp,
                       g_ent, grad);
    return hipGetLastError();
}
}
