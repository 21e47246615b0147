// mg_sample.h — the exact float32 pieces of a random draw, shared by the units that sample inside a launch: log32 and u01
// (bandits_learner's Thompson sampler and UCB), and on top of them the Gumbel-max draw of the softmax-sampled policies
// (bandits_policy, maze_policy). Everything here is defined operation by operation in include/metagym_hip.h and holds only
// under -ffp-contract=off (metagym_amd/build.py): one rounding per operation, nothing fused. Not included by mg_common.h.
#pragma once
#include "mg_common.h"
#include "mg_philox.h"

namespace mg {

constexpr uint32_t SAMPLE_TAG = 0x53000000u;     // c3 of a sampling block: tag | (arm >> 2)

// fdlibm's single-precision log for a positive normal x, one operation at a time (the definition of the header)
__device__ __forceinline__ float log32(float x) {
    uint32_t i = __float_as_uint(x);
    i += 0x3f800000u - 0x3f3504f3u;
    const int k = (int)(i >> 23) - 127;
    const float m = __uint_as_float((i & 0x007fffffu) + 0x3f3504f3u);
    const float f = m - 1.0f;
    const float s = f / (2.0f + f);
    const float z = s * s;
    const float w = z * z;
    const float t1 = w * (__uint_as_float(0x3eccce13u) + w * __uint_as_float(0x3e789e26u));   // Lg2, Lg4
    const float t2 = z * (__uint_as_float(0x3f2aaaaau) + w * __uint_as_float(0x3e91e9eeu));   // Lg1, Lg3
    const float R = t2 + t1;
    const float hfsq = (0.5f * f) * f;
    const float dk = (float)k;
    return (((s * (hfsq + R) + dk * __uint_as_float(0x3717f7d1u)) - hfsq) + f) + dk * __uint_as_float(0x3f317180u);
}

// an odd 24-bit integer times 2^-24: exact, never 0, never 1
__device__ __forceinline__ float u01(uint32_t word) { return (float)(((word >> 9) << 1) | 1u) * 5.9604644775390625e-08f; }

// The standard Gumbel value of one Philox word: g = -log32(-log32(u01(word))). u is in [2^-24, 1 - 2^-24], so -log32(u) is a
// positive normal float in [5.96e-8, 16.64]: both applications meet log32's precondition, and g is finite, in
// [-2.8116, 16.6356] (checked on the host over all 2^23 values of u).
__device__ __forceinline__ float gumbel(uint32_t word) { return -log32(-log32(u01(word))); }

// The sampling block of env `env` at step counter `step` for arms 4 q .. 4 q + 3: word j belongs to arm 4 q + j.
__device__ __forceinline__ void sample_block(uint32_t env, uint64_t step, uint32_t q, uint64_t seed, uint32_t o[4]) {
    philox4x32_10(env, (uint32_t)step, (uint32_t)(step >> 32), SAMPLE_TAG | q, (uint32_t)seed, (uint32_t)(seed >> 32), o);
}

// score = l * inv_t + g: one multiply, then one add, each rounded once
__device__ __forceinline__ float sample_score(float l, float inv_t, uint32_t word) { return l * inv_t + gumbel(word); }

// The streaming argmax both the greedy and the sampled form end in: arm k with value v enters after arms 0 .. k - 1. Ties
// and NaN resolve to the lowest index (a NaN at arm 0 stays, a later NaN never wins).
__device__ __forceinline__ void take_if_greater(int k, float v, int &arg, float &best) {
    if (k == 0) best = v;
    else if (v > best) { arg = k; best = v; }
}

}  // namespace mg
