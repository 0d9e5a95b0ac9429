// mrts_obs.hip -- the converters between the packed observation (one 32-bit one-hot word per
// env and cell: bit i = plane i, mrts_rules.h cell_onehot; what an engine of MRTS_OBS_PACKED
// writes and a rollout buffer keeps) and the dense planes a network reads.  Over rows = N * HW
// flat rows of P = 29 or 31 planes: neither kernel looks at env boundaries.
//
// k_unpack_obs is on the rollout's path (one launch per policy forward): 4 bytes in, 116 / 124
// (or half that, 2-byte elements) out per row, a pure store stream.  The dense array is written
// as the flat [rows * P] it is, in globally sequential order with 16-byte stores -- the pattern
// of k_unpack_masks (mrts_policy.hip) and of the step's own stream_obs.  k_pack_obs is off that
// path (the engine writes the words itself): a wave per 64 rows, nothing tuned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mrts_engine.h"

namespace mrts {
namespace obs {

constexpr int OT = 256;        // threads per workgroup
constexpr int OB_ROWS = 256;   // rows per workgroup: OB_ROWS * P elements are whole 16-byte chunks for either element size
static_assert(OB_ROWS % 8 == 0 && OB_ROWS == OT, "a workgroup's first element is 16-byte aligned when `obs` is; a pack wave per 64 rows");

template <int EB>
using Elem = std::conditional_t<EB == 2, uint16_t, uint32_t>;

// packed [rows] -> obs [rows][P] of Elem<EB>: `one` (the element type's 1 as stored bits) where
// the plane's bit is set, all-zero bits elsewhere; bits >= P of a word are ignored.  A workgroup
// stages its OB_ROWS words (masked to P bits) in LDS, then each lane writes 16-byte chunks of 4
// or 8 elements: elements e .. are planes pl .. of row r = e / P running on into row r + 1 (P >= 8:
// at most two rows), so (w[r] >> pl) | (w[r + 1] << (P - pl)) holds the chunk's bits.  The word
// behind the workgroup's last row is staged as zero and never used (a whole chunk ends inside the
// rows).  What is left behind the last whole chunk (2-byte elements with an odd rows * P, say)
// and a buffer that is not 16-byte aligned go per element.
// Staged by measurement: with the words read through L1 / L2 instead, the same kernel took 38.5 us
// against 37.0 us (float32, 8192 envs of 16x16; profiles/packed_obs/README.md §6).
template <int EB>
__global__ __launch_bounds__(OT) void k_unpack_obs(const uint32_t* __restrict__ packed, long long rows, int P, uint32_t one,
                                                    void* __restrict__ obs) {
    constexpr int EPC = 16 / EB;   // elements per 16-byte chunk
    const long long row0 = (long long)blockIdx.x * OB_ROWS;
    const int nr = (int)min((long long)OB_ROWS, rows - row0);
    const uint32_t keep = (1u << P) - 1u;
    __shared__ uint32_t s_w[OB_ROWS + 1];
    for (int i = threadIdx.x; i < OB_ROWS + 1; i += OT) s_w[i] = i < nr ? packed[row0 + i] & keep : 0u;
    __syncthreads();
    Elem<EB>* out = reinterpret_cast<Elem<EB>*>(obs) + (size_t)row0 * P;
    const int total = nr * P;
    auto elem = [&](int e) {
        const int r = P == 29 ? e / 29 : e / 31;
        return (Elem<EB>)((0u - ((s_w[r] >> (e - r * P)) & 1u)) & one);
    };
    if (((uintptr_t)obs & 15u) != 0) {
        for (int e = threadIdx.x; e < total; e += OT) out[e] = elem(e);
        return;
    }
    const int nch = total / EPC;
    for (int k = threadIdx.x; k < nch; k += OT) {
        const int e = k * EPC, r = P == 29 ? e / 29 : e / 31, pl = e - r * P;
        const uint32_t bits = (s_w[r] >> pl) | (s_w[r + 1] << (P - pl));
        auto on = [&](int i) { return (0u - ((bits >> i) & 1u)) & one; };
        v4i v;
        if (EB == 4) v = v4i{(int)on(0), (int)on(1), (int)on(2), (int)on(3)};
        else v = v4i{(int)(on(0) | on(1) << 16), (int)(on(2) | on(3) << 16), (int)(on(4) | on(5) << 16), (int)(on(6) | on(7) << 16)};
        *reinterpret_cast<v4i*>(out + e) = v;
    }
    for (int e = nch * EPC + threadIdx.x; e < total; e += OT) out[e] = elem(e);
}

// obs [rows][P] of Elem<EB> -> packed [rows]: bit i where element i has a bit of `nonzero` (every
// bit of an int32; all but the sign of a float: -0.0 is zero).  A wave takes 64 rows, two per
// trip: lanes 0..31 the planes of row 2 i, lanes 32..63 of row 2 i + 1 (coalesced over each row),
// one ballot, the rows' owner lanes keep its halves; then one coalesced 4-byte store per lane.
// Tail rows re-read the last one (unconditional loads).
template <int EB>
__global__ __launch_bounds__(OT) void k_pack_obs(const void* __restrict__ obs, long long rows, int P, uint32_t nonzero,
                                                  int32_t* __restrict__ packed) {
    const int lane = threadIdx.x & 63, half = lane >> 5, pl = lane & 31;
    const long long row0 = (long long)blockIdx.x * OB_ROWS + (threadIdx.x >> 6) * 64;
    if (row0 >= rows) return;   // wave-uniform
    const int rb = (int)min(64ll, rows - row0);
    const Elem<EB>* in = reinterpret_cast<const Elem<EB>*>(obs) + (size_t)row0 * P;
    uint32_t own = 0;
#pragma unroll 8
    for (int i = 0; i < 32; i++) {
        const int r = min(2 * i + half, rb - 1);
        const uint32_t x = in[r * P + min(pl, P - 1)];
        const unsigned long long b = __ballot(pl < P && (x & nonzero) != 0);
        if (lane == 2 * i) own = (uint32_t)b;
        if (lane == 2 * i + 1) own = (uint32_t)(b >> 32);
    }
    if (lane < rb) packed[row0 + lane] = (int32_t)own;
}

}  // namespace obs
}  // namespace mrts

// The launchers take the caller's stream, allocate nothing and synchronise nothing
// (mrts_capi.cpp has checked the arguments: planes 29 / 31, elem_bytes 2 / 4, rows within a grid).
extern "C" {
using namespace mrts::obs;
hipError_t mrts_engine_unpack_obs(const int32_t* packed, long long rows, int planes, int elem_bytes, uint32_t one, void* obs, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    const dim3 grid((unsigned)((rows + OB_ROWS - 1) / OB_ROWS));
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(packed);
    if (elem_bytes == 2) hipLaunchKernelGGL(k_unpack_obs<2>, grid, dim3(OT), 0, s, pw, rows, planes, one, obs);
    else hipLaunchKernelGGL(k_unpack_obs<4>, grid, dim3(OT), 0, s, pw, rows, planes, one, obs);
    return hipGetLastError();
}
hipError_t mrts_engine_pack_obs(const void* obs, long long rows, int planes, int elem_bytes, uint32_t nonzero, int32_t* packed, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    const dim3 grid((unsigned)((rows + OB_ROWS - 1) / OB_ROWS));
    if (elem_bytes == 2) hipLaunchKernelGGL(k_pack_obs<2>, grid, dim3(OT), 0, s, obs, rows, planes, nonzero, packed);
    else hipLaunchKernelGGL(k_pack_obs<4>, grid, dim3(OT), 0, s, obs, rows, planes, nonzero, packed);
    return hipGetLastError();
}
}
