// mrts_philox.h -- the Philox4x32-10 stream of the device samplers, one definition
// for the stand-in samplers (mrts_sampler.hip) and the masked action head
// (mrts_policy.hip): keyed by the seed, counter (cell, env, step, half) -- the
// oracle's ovec_sample_actions stream.  `env` is the GLOBAL env index (env0 + local
// row), so a shard of envs [env0, env0 + n) draws exactly the words of that slice of
// one larger run (multi-GPU sharding).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrts {

// (each round's two 32x32 products as 64-bit ones: one v_mad_u64_u32 each instead of
// a v_mul_hi_u32 + v_mul_lo_u32 pair, both quarter rate; the sampler's bound is its
// memory round trips, not these multiplies: one block per row measured 32.5 -> 32.0 us,
// profiles/r04_ab/r04u)
__device__ __forceinline__ void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// The eight random words of one row (env e, cell c), from two Philox4x32-10 blocks of
// counter (c, e, step, 0|1): they depend on (cell, env, step, seed) only, so a
// caller can draw them while the row's mask bits are still in flight.
__device__ __forceinline__ void philox_row(int e, int c, uint64_t seed, uint32_t step, uint32_t r[8]) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
        uint32_t ctr[4] = {(uint32_t)c, (uint32_t)e, step, (uint32_t)h};
        philox(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
        r[4 * h] = ctr[0]; r[4 * h + 1] = ctr[1]; r[4 * h + 2] = ctr[2]; r[4 * h + 3] = ctr[3];
    }
}

}  // namespace mrts
