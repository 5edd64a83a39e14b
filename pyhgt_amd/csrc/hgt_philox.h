// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the one generator of the library.
// Users: the counter-based dropout (hgt_dropout.hip: counter words 2 and 3 zero) and the device sampler (hgt_sampler.hip: word 3
// carries a non-zero domain tag, so its streams never meet a dropout stream of the same seed).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // key increments (golden ratio, sqrt(3) - 1)

struct Philox4 { uint32_t w[4]; };

// the full 128-bit counter (c0 .. c3) under the key (k0, k1)
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// a 64-bit counter in words 0 and 1, words 2 and 3 zero
__device__ __forceinline__ Philox4 philox4x32_10(uint64_t counter, uint32_t k0, uint32_t k1) {
    return philox4x32_10((uint32_t)counter, (uint32_t)(counter >> 32), 0u, 0u, k0, k1);
}
