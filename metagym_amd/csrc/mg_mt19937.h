// mg_mt19937.h — numpy's legacy MT19937 stream (RandomState) on the device: seeding, tempering, the block refill, the
// 53-bit double and the masked-rejection bound. Shared by metalm.hip (one stream per wave, key in LDS) and bandits.hip
// (one stream per lane, key in HBM, refilled by the whole wave through LDS). CPython's `random` runs on the same generator:
// its seeding (init_by_array), getrandbits and _randbelow are here too, with the two-block lane stream of liftsim.hip.
// (maze_sampler.hip still has its own LDS-resident copies of the CPython pieces, pinned by its goldens; moving it onto
// these is a separate change.)
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

// numpy.random.seed(s): init_genrand into key[0..624)
__device__ __forceinline__ void init_genrand(uint32_t *key, uint32_t s) {
    key[0] = s;
    for (int i = 1; i < MTN; ++i) key[i] = seed_step(key[i - 1], i);
}

// CPython random.seed(s) for 0 <= s < 2^32: init_by_array with the one-word key {s}
__device__ inline void init_by_array1(uint32_t *key, uint32_t s) {
    init_genrand(key, 19650218u);
    int i = 1;
    for (int k = MTN; k > 0; --k) {
        const uint32_t p = key[i - 1];
        key[i] = (key[i] ^ ((p ^ (p >> 30)) * 1664525u)) + s;   // + key[j] + j with j = 0
        if (++i >= MTN) { key[0] = key[MTN - 1]; i = 1; }
    }
    for (int k = MTN - 1; k > 0; --k) {
        const uint32_t p = key[i - 1];
        key[i] = (key[i] ^ ((p ^ (p >> 30)) * 1566083941u)) - (uint32_t)i;
        if (++i >= MTN) { key[0] = key[MTN - 1]; i = 1; }
    }
    key[0] = 0x80000000u;
}

// dst[0..624) = the refill of src[0..624) (distinct blocks), one lane serially
__device__ inline void refill_into(const uint32_t *src, uint32_t *dst) {
    for (int i = 0; i < MTN; ++i) {
        const uint32_t next = i + 1 < MTN ? src[i + 1] : dst[0];
        const uint32_t far = i + MTM < MTN ? src[i + MTM] : dst[i + MTM - MTN];
        dst[i] = twist(src[i], next, far);
    }
}

// A lane's stream over a two-block record key[0..1248): the block being read and its refill. p is the next word
// (wrapping at 1248); `ready` says whether the block that starts at the next block boundary ahead of p holds the refill
// of the one before it. Crossing a boundary uses it up; the wave restores it between steps (refill_ahead), so a lane never
// refills while its neighbours draw. Crossing a second boundary before that sets `bad` (the draws would be wrong).
// numpy / CPython state: key = the block holding word p - 1, pos = (p - 1) % 624 + 1.
struct LaneStream {
    uint32_t *key;
    int p, ready;
    bool bad;

    __device__ __forceinline__ uint32_t next() {
        if (p == 0 || p == MTN) {
            bad |= !ready;
            ready = 0;
        }
        const uint32_t w = temper(key[p]);
        p = p + 1 == 2 * MTN ? 0 : p + 1;
        return w;
    }
    // random.random() / numpy's legacy double
    __device__ __forceinline__ double next_double() {
        const uint32_t a = next();
        return to_double(a, next());
    }
    // random.getrandbits(k), 1 <= k <= 32
    __device__ __forceinline__ uint32_t getrandbits(int k) { return next() >> (32 - k); }
    // random._randbelow(n) (_randbelow_with_getrandbits), n >= 1
    __device__ __forceinline__ uint32_t randbelow(uint32_t n) {
        const int k = 32 - __clz(n);
        uint32_t r = getrandbits(k);
        while (r >= n) r = getrandbits(k);
        return r;
    }
};

// Wave job (all 64 lanes call it): for every lane j in `bal` whose record is rec0 + j * stride and whose last read word
// lies in block src_j, write the refill of that block into the other one, through LDS (the three-segment refill).
__device__ inline void refill_ahead(uint32_t *lds, uint32_t *rec0, size_t stride, uint64_t bal, int src, int lane) {
    while (bal) {
        const int j = __builtin_ctzll(bal);
        bal &= bal - 1;
        const int sj = __shfl(src, j);
        uint32_t *k = rec0 + (size_t)j * stride;
        for (int i = lane; i < MTN; i += 64) lds[i] = k[sj * MTN + i];
        __syncthreads();
        refill(lds, lane);
        for (int i = lane; i < MTN; i += 64) k[(sj ^ 1) * MTN + i] = lds[i];
        __threadfence_block();   // lane j reads the block back through the same CU's cache
        __syncthreads();
    }
}

}  // namespace mt
