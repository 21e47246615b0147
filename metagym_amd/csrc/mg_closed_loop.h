// mg_closed_loop.h — what the closed-loop translation units (maze_policy, maze_expert, maze3d_policy, and liftsim_policy and
// liftsim_rpolicy through liftsim_policy_core.h) repeat around their own arithmetic: an index clamp, the exploration draw,
// the staging of a wave's one policy in LDS, and on the host the LDS limit and the opt-in above 64 KiB. bandits_policy takes
// the two host helpers only (its kernel keeps its own staging and draw); bandits_learner does not include it. Not included
// by mg_common.h.
#pragma once
#include "mg_common.h"
#include "mg_philox.h"

namespace mg {

constexpr size_t LDS_LIMIT = 160 * 1024;         // gfx950: LDS per CU, the most one workgroup can have

typedef float v4f __attribute__((ext_vector_type(4)));

// i clamped into [0, n)
__host__ __device__ __forceinline__ int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// The exploration draw of env `env` at step counter `step`: one Philox block keyed by `seed`, c3 = `tag`. True when the env
// explores (word 0 below `thr`; thr = 0 draws nothing); `word` is then the block's second word, which picks the action.
__device__ __forceinline__ bool explore_draw(uint32_t env, uint64_t step, uint32_t tag, uint64_t seed, uint32_t thr,
                                             uint32_t &word) {
    if (thr == 0u) return false;
    uint32_t o[4];
    philox4x32_10(env, (uint32_t)step, (uint32_t)(step >> 32), tag, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    word = o[1];
    return o[0] < thr;
}

// The policy of the lane's env: its id clamped, its block in global memory, and `staged` when the whole wave holds one id (a
// ballot: wave-uniform) and staging is `allowed`. That policy's `count` floats then go to `dst` in LDS, 16 bytes per lane
// and pass; the caller synchronises before it reads them.
struct StagedPolicy { int pid; bool staged; const float *own; };
__device__ __forceinline__ StagedPolicy stage_policy(const float *params, int count, int id, int n_policies, int lane,
                                                     bool allowed, v4f *dst) {
    const int pid = clamp_index(id, n_policies);
    const int pid0 = __builtin_amdgcn_readfirstlane(pid);
    const bool staged = allowed && __builtin_amdgcn_ballot_w64(pid != pid0) == 0;
    const float *own = params + (size_t)pid * (size_t)count;
    if (staged) {
        const v4f *src = reinterpret_cast<const v4f *>(params + (size_t)pid0 * (size_t)count);
        for (int i = lane; i < count / 4; i += WAVE) dst[i] = src[i];
    }
    return StagedPolicy{pid, staged, own};
}

// A launch with more than 64 KiB of dynamic LDS has to ask for it.
template <class Kernel>
inline int opt_in_dynamic_lds(Kernel kernel, int bytes, const char *name) {
    if (bytes <= 64 * 1024) return MG_OK;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return e == hipSuccess ? MG_OK : set_error(-(int)e, "hipFuncSetAttribute(%s): %s", name, hipGetErrorString(e));
}

}  // namespace mg
