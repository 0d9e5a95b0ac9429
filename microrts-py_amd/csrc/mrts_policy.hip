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
//
// Packed masks (mrts_actions.h; k_policy_*_packed): the same bodies over the 79-bit
// words.  Each lane loads its own row's three words, one coalesced 768-byte pass per
// wave and group of 64 rows; the source ballot is bit 0; a source row's valid channels
// are read out of the owner lane's registers, so per source row only the logits (and
// the actions) are loaded and no load depends on another.  From the ballots on -- the
// fold proper -- both forms run the same code: the results are the same bits.
// In this unit too: the converters between the two forms (k_pack_masks, k_unpack_masks).
//
// Packed actions (mrts_actions.h; k_policy_*_words<PACKED>): the action format is one more
// template parameter of the same bodies.  sample stages its rows in LDS as before and each lane
// stores pack() of its row -- one 256-byte store per wave instead of 3.5 KB; evaluate and the
// backward load one word per source row and lane k < 7 takes component k of the row it stands
// for (-1 where the flag is set: forbidden like any out-of-range value).  Same arithmetic, same bits.
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
// 77 and ignore it), and lane k < 7's action of component k (EVAL / BWD).  Dense masks:
// the two mask words beside the logits.  Packed masks (mrts_actions.h): no mask load at
// all -- the row's words come out of the registers of the lane that owns the row.
// (-DMRTS_PACKED_ROW_LOADS, A/B builds only: the wave keeps word 0 of its 64 rows and
// loads a source row's three words beside its logits, as the dense form does.)
template <bool PACKED>
struct RowRegs {
    int m0, m1;
    float l0, l1;
    long long a;
};
template <>
struct RowRegs<true> {
    uint32_t w0, w1, w2;   // the row's packed words, the same in every lane
    float l0, l1;
    long long a;
};
// a wave's 64 packed rows, one per lane (dense masks: unused)
struct GroupWords {
    uint32_t w0, w1, w2;
};
template <Mode MODE, bool PACKED, bool AWORDS>
__device__ __forceinline__ void load_row(RowRegs<PACKED>& R, size_t row, int r, const GroupWords& gw, const int32_t* __restrict__ mask,
                                         const float* __restrict__ logits, const int64_t* __restrict__ act, int lane) {
    if constexpr (PACKED) {
        const float* l = logits + row * MRTS_MASK_CH;
        const int c1 = 64 + min(lane, MRTS_MASK_CH - 65);
#ifdef MRTS_PACKED_ROW_LOADS
        const int32_t* pr = mask + row * MASK_PACKED_WORDS;   // one address for the wave
        R.w0 = (uint32_t)pr[0];
        R.w1 = (uint32_t)pr[1];
        R.w2 = (uint32_t)pr[2];
#else
        // r is wave-uniform: three readlanes, the row's words in scalar registers
        R.w0 = (uint32_t)__builtin_amdgcn_readlane((int)gw.w0, r);
        R.w1 = (uint32_t)__builtin_amdgcn_readlane((int)gw.w1, r);
        R.w2 = (uint32_t)__builtin_amdgcn_readlane((int)gw.w2, r);
#endif
        R.l0 = l[lane];
        R.l1 = l[c1];
    } else {
        const int32_t* m = mask + row * MRTS_MASK_CH;
        const float* l = logits + row * MRTS_MASK_CH;
        const int c1 = 64 + min(lane, MRTS_MASK_CH - 65);   // unconditional loads: the compiler counts them, the next row's stay in flight
        R.m0 = m[lane];
        R.l0 = l[lane];
        R.m1 = m[c1];
        R.l1 = l[c1];
    }
    if constexpr (AWORDS) {   // `act` is the packed action words [rows]: lane k < 7 takes component k of the row the word stands for
        R.a = MODE == SAMPLE ? 0 : act_word_get((uint32_t) reinterpret_cast<const int32_t*>(act)[row], min(lane, 6));
    } else {
        R.a = MODE == SAMPLE ? 0 : act[row * 7 + min(lane, 6)];
    }
}

// Fold one source row (wave-uniform index r of the wave's 64 rows).  SAMPLE: the picks
// go to s_out[r * 7 + k] over the no-valid-entry draw already there.  BWD: the valid
// channels' gradient goes to g (the masked ones keep the +0.0f of the fill).
template <Mode MODE, bool PACKED>
__device__ __forceinline__ void fold_row(const RowRegs<PACKED>& R, int r, int lane, WaveRow& W, const uint32_t (&r8)[8], int64_t* __restrict__ s_out,
                                         double& slp, double& sent, float g_lp, float g_ent, float* __restrict__ g) {
#pragma clang fp contract(off)   // no fused multiply-adds: sample, evaluate and the backward round alike, bit for bit
    const bool hi = lane < MRTS_MASK_CH - 64;
    uint64_t vlo, vhi;
    if constexpr (PACKED) {
        const uint32_t w0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)R.w0), w1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)R.w1),
                       w2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)R.w2);
        vlo = packed_lo(w0, w1, w2);
        vhi = packed_hi(w2);
    } else {
        vlo = __ballot(R.m0 != 0);
        vhi = __ballot(hi && R.m1 != 0);
    }
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
template <Mode MODE, bool PACKED, bool AWORDS>
__device__ __forceinline__ void fold_rows(uint64_t pending, size_t row0, int lane, const float* __restrict__ logits,
                                          const int32_t* __restrict__ mask, const GroupWords& gw, const int64_t* __restrict__ act,
                                          WaveRow& W, const uint32_t (&r8)[8], int64_t* __restrict__ s_out, double& slp, double& sent,
                                          float g_lp, float g_ent, float* __restrict__ grad) {
    if (!pending) return;
    int r = __builtin_ctzll(pending);
    pending &= pending - 1ull;
    RowRegs<PACKED> cur;
    load_row<MODE, PACKED, AWORDS>(cur, row0 + r, r, gw, mask, logits, act, lane);
    while (true) {
        const bool more = pending != 0;
        const int rn = more ? __builtin_ctzll(pending) : r;   // none left: a harmless re-read
        pending &= pending - 1ull;
        RowRegs<PACKED> nxt;
        load_row<MODE, PACKED, AWORDS>(nxt, row0 + rn, rn, gw, mask, logits, act, lane);
        fold_row<MODE, PACKED>(cur, r, lane, W, r8, s_out, slp, sent, g_lp, g_ent,
                               MODE == BWD ? grad + (row0 + r) * MRTS_MASK_CH : nullptr);
        if (!more) break;
        cur = nxt;
        r = rn;
    }
}

// The source word of this lane's row among the wave's 64 rows from row0 (rb of them
// exist; tail lanes re-read the last row: unconditional loads).  Packed masks: the row's
// three words, each lane its own row in one coalesced 768-byte pass -- the source word
// is bit 0, and the mask of every row the wave will fold is in registers from here on.
template <bool PACKED>
__device__ __forceinline__ int group_source(const int32_t* __restrict__ mask, const int32_t* __restrict__ src, size_t row0, int rb,
                                            int lane, GroupWords& gw) {
    const size_t row = row0 + min(lane, rb - 1);
    if constexpr (PACKED) {
        const int32_t* pr = mask + row * MASK_PACKED_WORDS;
        gw.w0 = (uint32_t)pr[0];
#ifdef MRTS_PACKED_ROW_LOADS
        gw.w1 = gw.w2 = 0;
#else
        gw.w1 = (uint32_t)pr[1];
        gw.w2 = (uint32_t)pr[2];
#endif
        return (int)(gw.w0 & 1u);
    } else {
        gw.w0 = gw.w1 = gw.w2 = 0;
        return src[row];
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
// PACKED (the three bodies below): `mask` is packed [N][HW][3] and `src` is not read.
// AWORDS: `act` is the packed action words [N][HW] int32 (mrts_actions.h) behind the int64 pointer: sample
// stores pack() of the staged rows, evaluate and its backward read the row a word stands for.
template <bool PACKED, bool AWORDS>
__device__ __forceinline__ void policy_sample(const float* __restrict__ logits, const int32_t* __restrict__ mask,
                                              const int32_t* __restrict__ src, int hw, int env0, uint64_t seed, uint32_t step,
                                              int64_t* __restrict__ act, float* __restrict__ logprob, float* __restrict__ entropy) {
    __shared__ __attribute__((aligned(16))) int64_t s_out[PW][64 * 7];
    __shared__ WaveRow s_row[PW];
    const int e = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t base = (size_t)e * hw;
    const bool al16 = ((uintptr_t)(act + base * 7) & 15u) == 0;   // + 64 * 56 B per group keeps it
    double slp = 0.0, sent = 0.0;
    for (int c0 = w * 64; c0 < hw; c0 += PT) {
        const int rb = min(64, hw - c0);
        const bool in = lane < rb;
        GroupWords gw;
        const int s_raw = group_source<PACKED>(mask, src, base + c0, rb, lane, gw);   // unconditional: the Philox words are drawn behind it
        uint32_t r8[8];
        philox_row(env0 + e, c0 + lane, seed, step, r8);
        if (in) {
#pragma unroll
            for (int k = 0; k < ACT_COMPONENTS; k++) s_out[w][lane * 7 + k] = draw_uniform(r8[k], ACT_LEN[k]);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        fold_rows<SAMPLE, PACKED, AWORDS>(__ballot(in && s_raw != 0), base + c0, lane, logits, mask, gw, nullptr, s_row[w], r8, s_out[w], slp, sent,
                                  0.0f, 0.0f, nullptr);
        int64_t* ob = act + (base + c0) * 7;
        const int onel = rb * 7;
        if constexpr (AWORDS) {   // each lane packs its staged row: one coalesced 256-byte store per wave
            if (in) reinterpret_cast<int32_t*>(act)[base + c0 + lane] = (int32_t)act_word_pack(s_out[w] + lane * 7);
        } else if (al16) {
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
template <bool PACKED, bool AWORDS>
__device__ __forceinline__ void policy_eval(const float* __restrict__ logits, const int32_t* __restrict__ mask,
                                            const int32_t* __restrict__ src, int hw, const int64_t* __restrict__ act,
                                            float* __restrict__ logprob, float* __restrict__ entropy) {
    __shared__ WaveRow s_row[PW];
    const int e = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t base = (size_t)e * hw;
    const uint32_t r8[8] = {};
    double slp = 0.0, sent = 0.0;
    for (int c0 = w * 64; c0 < hw; c0 += PT) {
        const int rb = min(64, hw - c0);
        GroupWords gw;
        const int s_raw = group_source<PACKED>(mask, src, base + c0, rb, lane, gw);
        fold_rows<EVAL, PACKED, AWORDS>(__ballot(lane < rb && s_raw != 0), base + c0, lane, logits, mask, gw, act, s_row[w], r8, nullptr, slp, sent,
                                0.0f, 0.0f, nullptr);
    }
    reduce_env(slp, sent, logprob, entropy, e);
}

// k_policy_eval's inputs + g_lp [N], g_ent [N] -> grad [N][HW][78] f32, all of it: the
// workgroup fills its env's rows with +0.0f (16-byte stores when the env's first row
// is 16-byte aligned -- 312-byte rows: an odd hw with an odd env is not -- per element
// otherwise), then the waves store the source rows' valid channels over the fill.
template <bool PACKED, bool AWORDS>
__device__ __forceinline__ void policy_eval_bwd(const float* __restrict__ logits, const int32_t* __restrict__ mask,
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
        GroupWords gw;
        const int s_raw = group_source<PACKED>(mask, src, base + c0, rb, lane, gw);
        fold_rows<BWD, PACKED, AWORDS>(__ballot(lane < rb && s_raw != 0), base + c0, lane, logits, mask, gw, act, s_row[w], r8, nullptr, slp, sent,
                               glp, gent, grad);
    }
}

// The six kernels: the bodies above over dense masks (mask + src) and over packed ones.
__global__ __launch_bounds__(PT) void k_policy_sample(const float* __restrict__ logits, const int32_t* __restrict__ mask,
                                                      const int32_t* __restrict__ src, int hw, int env0, uint64_t seed, uint32_t step,
                                                      int64_t* __restrict__ act, float* __restrict__ logprob,
                                                      float* __restrict__ entropy) {
    policy_sample<false, false>(logits, mask, src, hw, env0, seed, step, act, logprob, entropy);
}
__global__ __launch_bounds__(PT) void k_policy_eval(const float* __restrict__ logits, const int32_t* __restrict__ mask,
                                                    const int32_t* __restrict__ src, int hw, const int64_t* __restrict__ act,
                                                    float* __restrict__ logprob, float* __restrict__ entropy) {
    policy_eval<false, false>(logits, mask, src, hw, act, logprob, entropy);
}
__global__ __launch_bounds__(PT) void k_policy_eval_bwd(const float* __restrict__ logits, const int32_t* __restrict__ mask,
                                                        const int32_t* __restrict__ src, int hw, const int64_t* __restrict__ act,
                                                        const float* __restrict__ g_lp, const float* __restrict__ g_ent,
                                                        float* __restrict__ grad) {
    policy_eval_bwd<false, false>(logits, mask, src, hw, act, g_lp, g_ent, grad);
}
__global__ __launch_bounds__(PT) void k_policy_sample_packed(const float* __restrict__ logits, const int32_t* __restrict__ packed, int hw,
                                                             int env0, uint64_t seed, uint32_t step, int64_t* __restrict__ act,
                                                             float* __restrict__ logprob, float* __restrict__ entropy) {
    policy_sample<true, false>(logits, packed, nullptr, hw, env0, seed, step, act, logprob, entropy);
}
__global__ __launch_bounds__(PT) void k_policy_eval_packed(const float* __restrict__ logits, const int32_t* __restrict__ packed, int hw,
                                                           const int64_t* __restrict__ act, float* __restrict__ logprob,
                                                           float* __restrict__ entropy) {
    policy_eval<true, false>(logits, packed, nullptr, hw, act, logprob, entropy);
}
__global__ __launch_bounds__(PT) void k_policy_eval_bwd_packed(const float* __restrict__ logits, const int32_t* __restrict__ packed, int hw,
                                                               const int64_t* __restrict__ act, const float* __restrict__ g_lp,
                                                               const float* __restrict__ g_ent, float* __restrict__ grad) {
    policy_eval_bwd<true, false>(logits, packed, nullptr, hw, act, g_lp, g_ent, grad);
}

// The same three over packed action words, either mask format (PACKED: `mask` is the packed masks, `src` unused).
template <bool PACKED>
__global__ __launch_bounds__(PT) void k_policy_sample_words(const float* __restrict__ logits, const int32_t* __restrict__ mask,
                                                            const int32_t* __restrict__ src, int hw, int env0, uint64_t seed, uint32_t step,
                                                            int32_t* __restrict__ words, float* __restrict__ logprob,
                                                            float* __restrict__ entropy) {
    policy_sample<PACKED, true>(logits, mask, src, hw, env0, seed, step, reinterpret_cast<int64_t*>(words), logprob, entropy);
}
template <bool PACKED>
__global__ __launch_bounds__(PT) void k_policy_eval_words(const float* __restrict__ logits, const int32_t* __restrict__ mask,
                                                          const int32_t* __restrict__ src, int hw, const int32_t* __restrict__ words,
                                                          float* __restrict__ logprob, float* __restrict__ entropy) {
    policy_eval<PACKED, true>(logits, mask, src, hw, reinterpret_cast<const int64_t*>(words), logprob, entropy);
}
template <bool PACKED>
__global__ __launch_bounds__(PT) void k_policy_eval_bwd_words(const float* __restrict__ logits, const int32_t* __restrict__ mask,
                                                              const int32_t* __restrict__ src, int hw, const int32_t* __restrict__ words,
                                                              const float* __restrict__ g_lp, const float* __restrict__ g_ent,
                                                              float* __restrict__ grad) {
    policy_eval_bwd<PACKED, true>(logits, mask, src, hw, reinterpret_cast<const int64_t*>(words), g_lp, g_ent, grad);
}

// ---------------------------------------------------------------------------
// Converters between the dense masks and the packed words (mrts_actions.h), over
// rows = N * HW flat rows: neither looks at env boundaries.
constexpr int CV_ROWS = 256;   // rows per workgroup: PW waves of 64 (pack), an even count (unpack's 16-byte chunks)
static_assert(CV_ROWS == 64 * PW && CV_ROWS % 2 == 0, "a wave per 64 rows; row pairs are 156 elements = 39 16-byte chunks");

// mask [rows][78] i32, src [rows] i32 -> packed [rows][3].  A wave takes 64 rows: per
// row two coalesced loads and two ballots (the fold's own first step), the row's owner
// lane keeps the words, then one coalesced pass of 12-byte rows.  Every row is read:
// a non-source row's bits are kept.
__global__ __launch_bounds__(PT) void k_pack_masks(const int32_t* __restrict__ mask, const int32_t* __restrict__ src, long long rows,
                                                   int32_t* __restrict__ packed) {
    const int lane = threadIdx.x & 63;
    const long long row0 = (long long)blockIdx.x * CV_ROWS + (threadIdx.x >> 6) * 64;
    if (row0 >= rows) return;   // wave-uniform
    const int rb = (int)min(64ll, rows - row0);
    const int c1 = 64 + min(lane, MRTS_MASK_CH - 65);
    const bool hi = lane < MRTS_MASK_CH - 64;
    const int s_raw = src[row0 + min(lane, rb - 1)];
    uint64_t lo_own = 0, hi_own = 0;
#pragma unroll 8
    for (int r = 0; r < 64; r++) {   // tail rows re-read the last one: unconditional loads, several rows in flight
        const int32_t* m = mask + (size_t)(row0 + min(r, rb - 1)) * MRTS_MASK_CH;
        const uint64_t vlo = __ballot(m[lane] != 0), vhi = __ballot(hi && m[c1] != 0);
        if (lane == r) {
            lo_own = vlo;
            hi_own = vhi;
        }
    }
    if (lane < rb) {
        int32_t* o = packed + (size_t)(row0 + lane) * MASK_PACKED_WORDS;
        o[0] = (int32_t)((uint32_t)(lo_own << 1) | (s_raw != 0 ? 1u : 0u));
        o[1] = (int32_t)(uint32_t)(lo_own >> 31);
        o[2] = (int32_t)((uint32_t)(lo_own >> 63) | (uint32_t)(hi_own << 1));
    }
}

// packed [rows][3] -> mask [rows][78] i32, src [rows] i32, every element 0 or 1.  A
// workgroup stages its CV_ROWS rows' words in LDS and streams the mask rows with
// 16-byte stores (stream_masks' bit arithmetic, mrts_engine.hip): elements 4k .. 4k + 3
// are channels ch .. ch + 3 of row r = bits ch + 1 .. ch + 4 of its word; ch is even and
// only ch = 76, on an even row, runs into the next row's channels 0, 1.  An odd row
// count leaves the last row's channels 76, 77 to a per-element tail; a mask pointer
// that is not 16-byte aligned takes the per-element path throughout.
__global__ __launch_bounds__(PT) void k_unpack_masks(const int32_t* __restrict__ packed, long long rows, int32_t* __restrict__ mask,
                                                     int32_t* __restrict__ src) {
    static_assert(MRTS_MASK_CH == 78, "mask row layout");
    __shared__ uint32_t s_w[MASK_PACKED_WORDS * CV_ROWS + 2];   // + the word pair read behind the last row (never used)
    const long long row0 = (long long)blockIdx.x * CV_ROWS;
    const int nr = (int)min((long long)CV_ROWS, rows - row0);
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(packed) + (size_t)row0 * MASK_PACKED_WORDS;
    for (int i = threadIdx.x; i < MASK_PACKED_WORDS * CV_ROWS + 2; i += PT) s_w[i] = i < MASK_PACKED_WORDS * nr ? pw[i] : 0u;
    __syncthreads();
    for (int r = threadIdx.x; r < nr; r += PT) src[row0 + r] = (int32_t)(s_w[MASK_PACKED_WORDS * r] & 1u);
    int32_t* out = mask + (size_t)row0 * MRTS_MASK_CH;   // CV_ROWS * 312 B per workgroup: aligned as `mask` is
    const int total = nr * MRTS_MASK_CH;
    if (((uintptr_t)mask & 15u) == 0) {
        for (int k = threadIdx.x; k < total / 4; k += PT) {
            const int r = 4 * k / MRTS_MASK_CH, ch = 4 * k - r * MRTS_MASK_CH, b0 = ch + 1;
            const int wr = MASK_PACKED_WORDS * r + (b0 >> 5);
            const uint32_t lo = s_w[wr], hi = s_w[wr + 1];
            const uint32_t fun = (uint32_t)((((uint64_t)hi << 32) | lo) >> (b0 & 31));
            const uint32_t bits = ch == 76 ? ((fun & 3u) | ((hi << 1) & 0xCu)) : fun;
            v4i v = {(int)(bits & 1u), (int)((bits >> 1) & 1u), (int)((bits >> 2) & 1u), (int)((bits >> 3) & 1u)};
            *reinterpret_cast<v4i*>(out + 4 * k) = v;
        }
        for (int e = 4 * (total / 4) + threadIdx.x; e < total; e += PT) {
            const int r = e / MRTS_MASK_CH, b = e % MRTS_MASK_CH + 1;
            out[e] = (int)((s_w[MASK_PACKED_WORDS * r + (b >> 5)] >> (b & 31)) & 1u);
        }
    } else {
        for (int e = threadIdx.x; e < total; e += PT) {
            const int r = e / MRTS_MASK_CH, b = e % MRTS_MASK_CH + 1;
            out[e] = (int)((s_w[MASK_PACKED_WORDS * r + (b >> 5)] >> (b & 31)) & 1u);
        }
    }
}

}  // namespace policy
}  // namespace mrts

// The launchers take the caller's stream, allocate nothing and synchronise nothing.
// `packed` picks the packed-mask kernel, which takes no src; `act_packed` the kernel over packed action words.
extern "C" {
using namespace mrts::policy;
hipError_t mrts_engine_policy_sample(int packed, int act_packed, const float* logits, const int32_t* mask, const int32_t* src, int n, int hw,
                                     int env0, uint64_t seed, uint32_t step, void* act, float* logprob, float* entropy, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 g((unsigned)n), b(PT);
    int64_t* const rows = static_cast<int64_t*>(act);
    int32_t* const words = static_cast<int32_t*>(act);
    if (act_packed && packed) hipLaunchKernelGGL(k_policy_sample_words<true>, g, b, 0, s, logits, mask, src, hw, env0, seed, step, words, logprob, entropy);
    else if (act_packed) hipLaunchKernelGGL(k_policy_sample_words<false>, g, b, 0, s, logits, mask, src, hw, env0, seed, step, words, logprob, entropy);
    else if (packed) hipLaunchKernelGGL(k_policy_sample_packed, g, b, 0, s, logits, mask, hw, env0, seed, step, rows, logprob, entropy);
    else hipLaunchKernelGGL(k_policy_sample, g, b, 0, s, logits, mask, src, hw, env0, seed, step, rows, logprob, entropy);
    return hipGetLastError();
}
hipError_t mrts_engine_policy_eval(int packed, int act_packed, const float* logits, const int32_t* mask, const int32_t* src, int n, int hw,
                                   const void* act, float* logprob, float* entropy, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 g((unsigned)n), b(PT);
    const int64_t* const rows = static_cast<const int64_t*>(act);
    const int32_t* const words = static_cast<const int32_t*>(act);
    if (act_packed && packed) hipLaunchKernelGGL(k_policy_eval_words<true>, g, b, 0, s, logits, mask, src, hw, words, logprob, entropy);
    else if (act_packed) hipLaunchKernelGGL(k_policy_eval_words<false>, g, b, 0, s, logits, mask, src, hw, words, logprob, entropy);
    else if (packed) hipLaunchKernelGGL(k_policy_eval_packed, g, b, 0, s, logits, mask, hw, rows, logprob, entropy);
    else hipLaunchKernelGGL(k_policy_eval, g, b, 0, s, logits, mask, src, hw, rows, logprob, entropy);
    return hipGetLastError();
}
hipError_t mrts_engine_policy_eval_bwd(int packed, int act_packed, const float* logits, const int32_t* mask, const int32_t* src, int n, int hw,
                                       const void* act, const float* g_lp, const float* g_ent, float* grad, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 g((unsigned)n), b(PT);
    const int64_t* const rows = static_cast<const int64_t*>(act);
    const int32_t* const words = static_cast<const int32_t*>(act);
    if (act_packed && packed) hipLaunchKernelGGL(k_policy_eval_bwd_words<true>, g, b, 0, s, logits, mask, src, hw, words, g_lp, g_ent, grad);
    else if (act_packed) hipLaunchKernelGGL(k_policy_eval_bwd_words<false>, g, b, 0, s, logits, mask, src, hw, words, g_lp, g_ent, grad);
    else if (packed) hipLaunchKernelGGL(k_policy_eval_bwd_packed, g, b, 0, s, logits, mask, hw, rows, g_lp, g_ent, grad);
    else hipLaunchKernelGGL(k_policy_eval_bwd, g, b, 0, s, logits, mask, src, hw, rows, g_lp, g_ent, grad);
    return hipGetLastError();
}
// rows = n * hw >= 1 (mrts_capi.cpp: within the samplers' row bound, so the grid is below 2^23)
static dim3 converter_grid(long long rows) { return dim3((unsigned)((rows + CV_ROWS - 1) / CV_ROWS)); }
hipError_t mrts_engine_pack_masks(const int32_t* mask, const int32_t* src, long long rows, int32_t* packed, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pack_masks, converter_grid(rows), dim3(PT), 0, s, mask, src, rows, packed);
    return hipGetLastError();
}
hipError_t mrts_engine_unpack_masks(const int32_t* packed, long long rows, int32_t* mask, int32_t* src, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(k_unpack_masks, converter_grid(rows), dim3(PT), 0, s, packed, rows, mask, src);
    return hipGetLastError();
}
}
