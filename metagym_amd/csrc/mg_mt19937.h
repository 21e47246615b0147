// mg_mt19937.h — numpy's legacy MT19937 stream (RandomState) on the device: seeding, tempering, the block refill, the
// 53-bit double and the masked-rejection bound. Shared by metalm.hip (one stream per wave, key in LDS) and bandits.hip
// (one stream per lane, key in HBM, refilled by the whole wave through LDS).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mt {

constexpr int MTN = 624, MTM = 397, SEG = MTN - MTM;   // SEG = 227

__device__ __forceinline__ uint32_t temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

__device__ __forceinline__ uint32_t twist(uint32_t cur, uint32_t next, uint32_t far) {
    const uint32_t y = (cur & 0x80000000u) | (next & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// mt19937_seed (numpy.random.seed(s) for an integer s): key[i] for i in [0, 624); pos is then 624
__device__ __forceinline__ uint32_t seed_step(uint32_t prev, int i) {
    return 1812433253u * (prev ^ (prev >> 30)) + (uint32_t)i;
}

// the legacy double from two consecutive draws a, b: (a >> 5, b >> 6) as 53 bits
__device__ __forceinline__ double to_double(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

// Refill of a 624-word key held in LDS by one wave (a workgroup of 64), in three segments that are each independent
// inside themselves: [0,227) reads old words only, [227,454) reads the new words i-227 of the first segment, [454,624)
// those of the second and (word 623) the new word 0. Within a segment every read happens before any write (barrier),
// since lane i's `next` word is lane i+1's output.
template <int LO, int HI>
__device__ __forceinline__ void refill_segment(uint32_t *key, int lane) {
    constexpr int R = (HI - LO + 63) / 64;
    uint32_t v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = LO + lane + 64 * r;
        if (i < HI) {
            const uint32_t next = key[i + 1 == MTN ? 0 : i + 1];
            const uint32_t far = key[i + MTM >= MTN ? i + MTM - MTN : i + MTM];
            v[r] = twist(key[i], next, far);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = LO + lane + 64 * r;
        if (i < HI) key[i] = v[r];
    }
    __syncthreads();
}

__device__ __forceinline__ void refill(uint32_t *key, int lane) {
    refill_segment<0, SEG>(key, lane);
    refill_segment<SEG, 2 * SEG>(key, lane);
    refill_segment<2 * SEG, MTN>(key, lane);
}

// randint's mask for the range [0, rng]: the smallest 2^k - 1 >= rng
inline uint32_t bound_mask(uint32_t r) {
    r |= r >> 1; r |= r >> 2; r |= r >> 4; r |= r >> 8; r |= r >> 16;
    return r;
}

}  // namespace mt
