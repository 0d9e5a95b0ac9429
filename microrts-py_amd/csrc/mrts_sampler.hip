// mrts_sampler.hip -- the stand-in policy's samplers (mrts_sample_actions, _src, _src_packed,
// _src_group) and the converters between the int64 action rows and the packed action words:
// the kernels and their launchers.  They share the Philox stream and the
// action-row layout with the masked action head, and nothing with the game step.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mrts_actions.h"
#include "mrts_engine.h"
#include "mrts_layout.h"
#include "mrts_philox.h"

namespace mrts {

// Counter-based masked sampler (hello_world.py:27-64 semantics), Philox4x32-10
// keyed (seed) with counter (cell, env, step, half) -- identical stream to the
// oracle's ovec_sample_actions.  `env` is the GLOBAL env index (env0 + local
// row), so a shard of envs [env0, env0 + n) draws exactly the actions of that
// slice of one larger run (multi-GPU sharding).
// philox / philox_row (the row's eight random words): mrts_philox.h, shared with
// the masked action head (mrts_policy.hip).
//
// One row (env e, cell c): the 78 mask channels as bits lo (0..63) | hi (64..77);
// per component k, a uniform pick among the valid entries (uniform over all
// entries when none is valid), from two Philox4x32-10 blocks of counter
// (c, e, step, 0|1) -- the oracle's ovec_sample_actions stream.
__device__ __forceinline__ void select_row(uint64_t lo, uint64_t hi, const uint32_t r[8], int64_t* out) {
#pragma unroll
    for (int k = 0; k < ACT_COMPONENTS; k++) {
        uint64_t seg = comp_bits(lo, hi, ACT_OFF[k], ACT_LEN[k]);
        const int nvalid = __popcll(seg);
        int pick;
        if (nvalid == 0) {
            pick = draw_uniform(r[k], ACT_LEN[k]);
        } else {
            int t = draw_uniform(r[k], nvalid);
            for (; t > 0; t--) seg &= seg - 1ull;   // drop the t lowest set bits
            pick = __builtin_ctzll(seg);
        }
        out[k] = pick;
    }
}
__device__ __forceinline__ void sample_row(uint64_t lo, uint64_t hi, int e, int c, uint64_t seed, uint32_t step, int64_t* out) {
    uint32_t r[8];
    philox_row(e, c, seed, step, r);
    select_row(lo, hi, r, out);
}

// Persistent, software-pipelined: every WAVE owns groups of SW = 32 consecutive
// (env, cell) rows (32 x 312 B of int32 mask, contiguous).  While a group is
// folded into 78-bit words in the wave's LDS slice and sampled (one lane per
// row), the NEXT group's 10 dwordx4 loads per lane are already in flight in a
// second register buffer, so the HBM stream never idles behind the Philox /
// selection arithmetic.  The 7 int64 components per row are staged in LDS and
// written back with coalesced 16-byte stores.  No block barriers: a wave's own
// LDS operations complete in order.
constexpr int SW = 32;                                   // rows per group (one wave)
constexpr int SWAVES = 4;                                // waves per workgroup
constexpr int SNV = (SW * MRTS_MASK_CH / 4 + 63) / 64;   // dwordx4 loads per lane per group (10)

struct SampleBuf {
    int4 v[SNV];
};

__device__ __forceinline__ void sample_load(SampleBuf& B, const int32_t* __restrict__ mask, long long grp, long long rows) {
    const long long row0 = grp * SW;
    const int rb = (int)min((long long)SW, rows - row0);
    const int nv = rb * MRTS_MASK_CH / 4;
    const int4* m4 = reinterpret_cast<const int4*>(mask + row0 * MRTS_MASK_CH);
    // Unconditional loads (tail lanes re-read the group's last int4 and are
    // masked when consumed): no branch around a load, so hipcc can count them and
    // wait with vmcnt(SNV) for this group while the next one stays in flight.
#pragma unroll
    for (int j = 0; j < SNV; j++) {
        const int k = min(j * 64 + (int)(threadIdx.x & 63), nv - 1);
        const v4i t = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(m4 + k));   // streamed once
        B.v[j] = make_int4(t.x, t.y, t.z, t.w);
    }
}

__device__ __forceinline__ void sample_group(const SampleBuf& B, const int32_t* __restrict__ mask, long long grp, long long rows,
                                             int hw, int env0, uint64_t seed, uint32_t step, int64_t* __restrict__ act,
                                             uint32_t* s_bits, int64_t* s_out) {
    const int lane = threadIdx.x & 63;
    const long long row0 = grp * SW;
    const int rb = (int)min((long long)SW, rows - row0);
    const int nel = rb * MRTS_MASK_CH, nv = nel >> 2;
    for (int i = lane; i < SW * 3; i += 64) s_bits[i] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
    for (int j = 0; j < SNV; j++) {
        const int k = j * 64 + lane;
        const int4 v = B.v[j];
        if (k >= nv || (v.x | v.y | v.z | v.w) == 0) continue;   // most cells hold no idle unit
        int e = 4 * k;
        int r = e / MRTS_MASK_CH, ch = e - r * MRTS_MASK_CH;
        const int vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (vv[q]) atomicOr(&s_bits[3 * r + (ch >> 5)], 1u << (ch & 31));
            if (++ch == MRTS_MASK_CH) { ch = 0; r++; }
        }
    }
    for (int e = 4 * nv + lane; e < nel; e += 64) {   // odd row count: the last 2 int32
        if (mask[row0 * MRTS_MASK_CH + e]) {
            int r = e / MRTS_MASK_CH, ch = e - r * MRTS_MASK_CH;
            atomicOr(&s_bits[3 * r + (ch >> 5)], 1u << (ch & 31));
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane < rb) {
        const long long idx = row0 + lane;
        const int e = (int)(idx / hw), c = (int)(idx - (long long)e * hw);
        const uint64_t lo = (uint64_t)s_bits[3 * lane] | ((uint64_t)s_bits[3 * lane + 1] << 32);
        const uint64_t hi = s_bits[3 * lane + 2];
        sample_row(lo, hi, env0 + e, c, seed, step, s_out + lane * 7);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    int64_t* ob = act + row0 * 7;   // 16-B aligned: SW * 56 B per group
    const int onel = rb * 7, onv = onel >> 1;
    int4* o4 = reinterpret_cast<int4*>(ob);
    const int4* s4 = reinterpret_cast<const int4*>(s_out);
    for (int k = lane; k < onv; k += 64) o4[k] = s4[k];
    if ((onel & 1) && lane == 0) ob[onel - 1] = s_out[onel - 1];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

constexpr int SAMPLE_BLOCKS_PER_CU = 16;   // measured best (round 1: 2 -> 151 us, 4 -> 138, 8 -> 133, 16 -> 127, 64 -> 178)
__global__ __launch_bounds__(64 * SWAVES) void k_sample(const int32_t* __restrict__ mask, int n, int hw, int env0,
                                                        uint64_t seed, uint32_t step, int64_t* __restrict__ act) {
    __shared__ uint32_t s_bits[SWAVES][SW * 3];
    __shared__ __attribute__((aligned(16))) int64_t s_out[SWAVES][SW * 7];
    const int w = threadIdx.x >> 6;
    const long long rows = (long long)n * hw;
    const long long ngrp = (rows + SW - 1) / SW;
    const long long stride = (long long)gridDim.x * SWAVES;
    long long grp = (long long)blockIdx.x * SWAVES + w;
    if (grp >= ngrp) return;
    SampleBuf A, B;
    sample_load(A, mask, grp, rows);
    while (true) {   // two groups per trip: A is consumed while B loads, then the reverse
        const long long g1 = grp + stride;   // past the end: a harmless re-read of the last group
        sample_load(B, mask, min(g1, ngrp - 1), rows);
        sample_group(A, mask, grp, rows, hw, env0, seed, step, act, s_bits[w], s_out[w]);
        if (g1 >= ngrp) break;
        const long long g2 = g1 + stride;
        sample_load(A, mask, min(g2, ngrp - 1), rows);
        sample_group(B, mask, g1, rows, hw, env0, seed, step, act, s_bits[w], s_out[w]);
        if (g2 >= ngrp) break;
        grp = g2;
    }
}

// Source-guided variant: the same stream and output, given the source channel
// as well.  getMasks sets no channel of a cell whose source bit is 0 (no idle
// unit of the player: UnitAction.getValidActionArray is all zero), so only the
// mask rows of source cells are read -- a few per cent of the 78-channel rows
// on basesWorkers -- while every row's 7 components are still drawn and
// written.  One wave per 64 consecutive rows: the wave reads the rows of its
// active lanes cooperatively (channel k on lane k, two coalesced loads per row,
// up to SRC_ROWS (4) rows in flight) and folds each with two ballots.  Measured
// and refuted in round 5 (profiles/r05_ab/): writing every row's no-valid-entry
// draw first and patching the source rows after (sampler 32.6 -> 35.6 us, and the
// next k_step +8 us); two 64-row groups per wave sharing one chain of round trips
// (32.7 -> 32.4 us, configs[1] 2 % slower).
constexpr int SR_WAVES = 4;
constexpr int SRC_ROWS = 4;   // source rows per round trip (8 and 16 measured slower, profiles/r04_ab/r04v)
// one block's 4 x 64 rows of one batch (k_sample_src: block = blockIdx.x; the grouped
// launch: the block's index inside its segment).  WORDS (k_sample_src_packed): the same picks
// as packed action words (mrts_actions.h), `act` is int32 [rows] -- each lane packs its row in
// registers and the wave makes one coalesced 256-byte store; no LDS staging (s_out unused).
template <bool WORDS>
__device__ __forceinline__ void sample_src_block(const int32_t* __restrict__ mask, const int32_t* __restrict__ src, int n, int hw,
                                                 int env0, uint64_t seed, uint32_t step, void* __restrict__ act_out, long long blk,
                                                 int64_t (*s_out)[64 * 7]) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long rows = (long long)n * hw;
    const long long row0 = (blk * SR_WAVES + w) * 64;
    if (row0 >= rows) return;
    const int rb = (int)min(64ll, rows - row0);
    const bool in = lane < rb;
    // unconditional load (tail lanes re-read the last row): no branch around it, so
    // its wait falls after the row's Philox words, which are drawn while the source
    // word (and then the mask rows) are in flight
    const int s_raw = src[row0 + min(lane, rb - 1)];
    uint32_t r8[8];
    const unsigned idx = (unsigned)(row0 + lane);   // rows = n * hw < 2^31 (the C ABI's sampler_rows_ok checks)
    const int e = (int)(idx / (unsigned)hw), c = (int)(idx - (unsigned)e * (unsigned)hw);
    philox_row(env0 + e, c, seed, step, r8);
#pragma unroll
    for (int k = 0; k < 8; k++) asm volatile("" : "+v"(r8[k]));   // computed here, not sunk to their use after the loads
    const int s = in ? s_raw : 0;
    uint64_t pending = __ballot(s != 0);
    uint64_t lo = 0, hi = 0;   // this lane's row as 78 bits
    while (pending) {          // wave-uniform; SRC_ROWS source rows per round trip
        int r[SRC_ROWS];
#pragma unroll
        for (int k = 0; k < SRC_ROWS; k++) {
            r[k] = pending ? __builtin_ctzll(pending) : r[0];   // repeats r[0]
            pending &= pending - 1ull;
        }
        int v0[SRC_ROWS], v1[SRC_ROWS];
#pragma unroll
        for (int k = 0; k < SRC_ROWS; k++) {   // all the loads in flight before the first ballot
            const int32_t* m = mask + (row0 + r[k]) * MRTS_MASK_CH;   // (a repeated row re-reads the same bits)
            v0[k] = __builtin_nontemporal_load(m + lane);
            v1[k] = __builtin_nontemporal_load(m + 64 + min(lane, MRTS_MASK_CH - 65));
        }
#pragma unroll
        for (int k = 0; k < SRC_ROWS; k++) {
            const uint64_t b0 = __ballot(v0[k] != 0);
            const uint64_t b1 = __ballot(lane < MRTS_MASK_CH - 64 && v1[k] != 0);
            if (lane == r[k]) { lo = b0; hi = b1; }
        }
    }
    if constexpr (WORDS) {
        if (in) {
            int64_t o[ACT_COMPONENTS];
            select_row(lo, hi, r8, o);
            // non-temporal like the dense rows: k_step reads ~2 % of the words back
            __builtin_nontemporal_store((int32_t)act_word_pack(o), static_cast<int32_t*>(act_out) + row0 + lane);
        }
        return;
    }
    int64_t* const act = static_cast<int64_t*>(act_out);
    if (in) select_row(lo, hi, r8, s_out[w] + lane * 7);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    int64_t* ob = act + row0 * 7;   // 16-B aligned: 64 * 56 B per wave
    const int onel = rb * 7, onv = onel >> 1;
    int4* o4 = reinterpret_cast<int4*>(ob);
    const int4* s4 = reinterpret_cast<const int4*>(s_out[w]);
    for (int k = lane; k < onv; k += 64) {   // non-temporal: k_step reads ~2 % of the rows back
        const int4 t = s4[k];
        const v4i v = {t.x, t.y, t.z, t.w};
        __builtin_nontemporal_store(v, reinterpret_cast<v4i*>(o4 + k));
    }
    if ((onel & 1) && lane == 0) ob[onel - 1] = s_out[w][onel - 1];
}
__global__ __launch_bounds__(64 * SR_WAVES) void k_sample_src(const int32_t* __restrict__ mask, const int32_t* __restrict__ src, int n,
                                                           int hw, int env0, uint64_t seed, uint32_t step,
                                                           int64_t* __restrict__ act) {
    __shared__ __attribute__((aligned(16))) int64_t s_out[SR_WAVES][64 * 7];
    sample_src_block<false>(mask, src, n, hw, env0, seed, step, act, blockIdx.x, s_out);
}
__global__ __launch_bounds__(64 * SR_WAVES) void k_sample_src_packed(const int32_t* __restrict__ mask, const int32_t* __restrict__ src,
                                                                  int n, int hw, int env0, uint64_t seed, uint32_t step,
                                                                  int32_t* __restrict__ words) {
    sample_src_block<true>(mask, src, n, hw, env0, seed, step, words, blockIdx.x, nullptr);
}
// Several batches (a mixed batch's size buckets) in one launch: segment k owns blocks
// [end[k-1], end[k]); a block finds its segment with a scalar scan of the table.
struct SampleSeg {
    const int32_t* mask;
    const int32_t* src;
    int64_t* act;
    int n, hw, env0;
};
struct SampleGroup {
    SampleSeg seg[MRTS_SAMPLE_GROUP_MAX];
    long long end[MRTS_SAMPLE_GROUP_MAX];
    int nseg;
};
__global__ __launch_bounds__(64 * SR_WAVES) void k_sample_src_group(const SampleGroup g, uint64_t seed, uint32_t step) {
    __shared__ __attribute__((aligned(16))) int64_t s_out[SR_WAVES][64 * 7];
    const long long b = blockIdx.x;
    int k = 0;
    while (k + 1 < g.nseg && b >= g.end[k]) k++;
    const SampleSeg& sg = g.seg[k];
    sample_src_block<false>(sg.mask, sg.src, sg.n, sg.hw, sg.env0, seed, step, sg.act, b - (k ? g.end[k - 1] : 0), s_out);
}

// ---------------------------------------------------------------------------
// Converters between the int64 action rows [rows][7] and the packed words [rows] (mrts_actions.h),
// over flat rows.  The int64 side is 56 bytes a row: a workgroup's AC_ROWS rows are 896 16-byte
// chunks, moved coalesced through LDS when the int64 pointer is 16-byte aligned (then every
// workgroup's slice is), per element otherwise.
constexpr int AC_ROWS = 256;   // rows per workgroup, one lane each on the word side
static_assert(AC_ROWS * ACT_COMPONENTS % 2 == 0, "a workgroup's rows are whole 16-byte chunks");

// act [rows][7] i64 -> words [rows].  Eight lanes' worth of loads per row either way (the row is
// read whole); the word store is one coalesced pass.
__global__ __launch_bounds__(AC_ROWS) void k_pack_actions(const int64_t* __restrict__ act, long long rows, int32_t* __restrict__ words) {
    __shared__ __attribute__((aligned(16))) int64_t s_a[AC_ROWS * ACT_COMPONENTS];
    const long long row0 = (long long)blockIdx.x * AC_ROWS;
    const int nr = (int)min((long long)AC_ROWS, rows - row0);
    const int nel = nr * ACT_COMPONENTS;
    const int64_t* in = act + row0 * ACT_COMPONENTS;
    if (((uintptr_t)act & 15u) == 0) {
        const v4i* i4 = reinterpret_cast<const v4i*>(in);
        v4i* s4 = reinterpret_cast<v4i*>(s_a);
        for (int k = threadIdx.x; k < nel / 2; k += AC_ROWS) s4[k] = __builtin_nontemporal_load(i4 + k);
        if ((nel & 1) && threadIdx.x == 0) s_a[nel - 1] = in[nel - 1];
    } else {
        for (int k = threadIdx.x; k < nel; k += AC_ROWS) s_a[k] = in[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < nr) words[row0 + threadIdx.x] = (int32_t)act_word_pack(s_a + threadIdx.x * ACT_COMPONENTS);
}

// words [rows] -> act [rows][7] i64: every element written, -1 where the component's flag is set.
__global__ __launch_bounds__(AC_ROWS) void k_unpack_actions(const int32_t* __restrict__ words, long long rows, int64_t* __restrict__ act) {
    __shared__ __attribute__((aligned(16))) int64_t s_a[AC_ROWS * ACT_COMPONENTS];
    const long long row0 = (long long)blockIdx.x * AC_ROWS;
    const int nr = (int)min((long long)AC_ROWS, rows - row0);
    const int nel = nr * ACT_COMPONENTS;
    if ((int)threadIdx.x < nr) {
        const uint32_t w = (uint32_t)words[row0 + threadIdx.x];
#pragma unroll
        for (int k = 0; k < ACT_COMPONENTS; k++) s_a[threadIdx.x * ACT_COMPONENTS + k] = act_word_get(w, k);
    }
    __syncthreads();
    int64_t* out = act + row0 * ACT_COMPONENTS;
    if (((uintptr_t)act & 15u) == 0) {
        v4i* o4 = reinterpret_cast<v4i*>(out);
        const v4i* s4 = reinterpret_cast<const v4i*>(s_a);
        for (int k = threadIdx.x; k < nel / 2; k += AC_ROWS) o4[k] = s4[k];
        if ((nel & 1) && threadIdx.x == 0) out[nel - 1] = s_a[nel - 1];
    } else {
        for (int k = threadIdx.x; k < nel; k += AC_ROWS) out[k] = s_a[k];
    }
}

}  // namespace mrts

// The launchers take the caller's stream, allocate and synchronise nothing.  n * hw fits 32 bits
// and the action pointers are 16-byte aligned: mrts_capi.cpp rejects anything else before these.
extern "C" {
hipError_t mrts_engine_sample(const int32_t* mask, int n, int hw, int env0, uint64_t seed, uint32_t step, int64_t* act, hipStream_t s) {
    int total = n * hw;
    if (total == 0) return hipSuccess;
    // persistent grid: enough waves to keep every CU streaming, each looping over row groups
    const long long groups = ((long long)total + mrts::SW - 1) / mrts::SW;
    const long long blocks = std::min<long long>((groups + mrts::SWAVES - 1) / mrts::SWAVES, 256 * mrts::SAMPLE_BLOCKS_PER_CU);   // resident blocks
    hipLaunchKernelGGL(mrts::k_sample, dim3((unsigned)blocks), dim3(64 * mrts::SWAVES), 0, s, mask, n, hw, env0, seed, step, act);
    return hipGetLastError();
}
hipError_t mrts_engine_sample_src(const int32_t* mask, const int32_t* src, int n, int hw, int env0, uint64_t seed, uint32_t step,
                                  int64_t* act, hipStream_t s) {
    const long long rows = (long long)n * hw;
    if (rows == 0) return hipSuccess;
    const long long blocks = (rows + 64 * mrts::SR_WAVES - 1) / (64 * mrts::SR_WAVES);
    hipLaunchKernelGGL(mrts::k_sample_src, dim3((unsigned)blocks), dim3(64 * mrts::SR_WAVES), 0, s, mask, src, n, hw, env0, seed, step, act);
    return hipGetLastError();
}
hipError_t mrts_engine_sample_src_packed(const int32_t* mask, const int32_t* src, int n, int hw, int env0, uint64_t seed, uint32_t step,
                                         int32_t* words, hipStream_t s) {
    const long long rows = (long long)n * hw;
    if (rows == 0) return hipSuccess;
    const long long blocks = (rows + 64 * mrts::SR_WAVES - 1) / (64 * mrts::SR_WAVES);
    hipLaunchKernelGGL(mrts::k_sample_src_packed, dim3((unsigned)blocks), dim3(64 * mrts::SR_WAVES), 0, s, mask, src, n, hw, env0, seed, step,
                       words);
    return hipGetLastError();
}
// rows within the samplers' row bound (mrts_capi.cpp): the grid is below 2^23
hipError_t mrts_engine_pack_actions(const int64_t* act, long long rows, int32_t* words, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(mrts::k_pack_actions, dim3((unsigned)((rows + mrts::AC_ROWS - 1) / mrts::AC_ROWS)), dim3(mrts::AC_ROWS), 0, s, act, rows, words);
    return hipGetLastError();
}
hipError_t mrts_engine_unpack_actions(const int32_t* words, long long rows, int64_t* act, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(mrts::k_unpack_actions, dim3((unsigned)((rows + mrts::AC_ROWS - 1) / mrts::AC_ROWS)), dim3(mrts::AC_ROWS), 0, s, words, rows, act);
    return hipGetLastError();
}
hipError_t mrts_engine_sample_src_group(const mrts_sample_seg* segs, int nseg, uint64_t seed, uint32_t step, hipStream_t s) {
    mrts::SampleGroup g{};
    long long blocks = 0;
    for (int k = 0; k < nseg; k++) {
        const mrts_sample_seg& q = segs[k];
        g.seg[k] = mrts::SampleSeg{q.mask, q.source, q.actions, q.num_envs, q.hw, q.env0};
        blocks += ((long long)q.num_envs * q.hw + 64 * mrts::SR_WAVES - 1) / (64 * mrts::SR_WAVES);
        g.end[k] = blocks;
    }
    g.nseg = nseg;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(mrts::k_sample_src_group, dim3((unsigned)blocks), dim3(64 * mrts::SR_WAVES), 0, s, g, seed, step);
    return hipGetLastError();
}
}
