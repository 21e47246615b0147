// liftsim_policy.hip — LiftSim closed-loop rollouts: learned dispatchers inside the launch (mg_liftsim_policy_*).
//
// A translation unit of its own on liftsim_policy_core.h: what it shares with liftsim_rpolicy.hip (the hall-call sets, the
// input gather, the head of a hidden unit, the logit loop and argmax, the decode, the record stores, the host checks), and
// through it liftsim_core.h (refill_streams, step_body, K, Lay, Records) and mg_closed_loop.h (stage_policy, the LDS limit
// and opt-in). Same flags (metagym_amd/build.py): -ffp-contract=off, which is what makes the policy definition of
// include/metagym_hip.h hold (one rounding per operation).
//
// Mapping: liftsim_rollout_kernel's — one lane per building, one wave per workgroup, {refill, policy, step_body} T times.
// The policy of a step runs between two step_body calls, when nothing of the step is live: per elevator the eight scaled
// inputs, the dispatch target and the reserved floors as a 128-bit set in registers; the two hall-call sets are built once
// per step. A hidden unit's pre-activation accumulates in a register, four units at a time; h lives in LDS lane-minor
// (h[j * 64 + lane]: H is a run-time value). The A logits are never stored: they are formed four at a time and compared in
// index order, so the running argmax holds one logit and one index. The elevators' actions wait in LDS columns (int16 target:
// -1 and 128 both occur) until step_body reads them. Weights: a wave whose lanes all hold one policy id stages that
// policy in LDS once, when the host found that the launch's LDS need fits a workgroup, and reads it with same-address
// reads; otherwise each lane reads its own block from global memory. Both inline lp_eval, so the bits are equal.
//
// All LDS is dynamic, carved at multiples of 16 bytes from a 16-byte aligned base (a static array ahead of it would shift
// the base of the 16-byte reads).
#include "liftsim_policy_core.h"

namespace {

// floats of one hidden unit's record: b[j] 0 0 0 | ws[j][0..7] | we[j][0..E-1] | wt[j][0..F] | wr[j][0..F-1] | wu | wd,
// every group zero-padded to a multiple of four floats: 12 + P4(E) + P4(F + 1) + 3 P4(F), as the sum unit_head's offsets
// form (with the product written out beside those sums the kernel grew a 68-byte private segment)
__host__ __device__ constexpr int lp_unit_record(int F, int E) { return unit_head(F, E).wd + pad4(F); }
// floats of one choice's record: bo[c] 0 0 0 | wo[c][0..H-1] and zeros up to HP
__host__ __device__ constexpr int lp_choice_record(int hidden) { return 4 + pad4(hidden); }
__host__ __device__ constexpr int lp_count(int hidden, int F, int E) {
    return hidden * lp_unit_record(F, E) + (2 * F + 2) * lp_choice_record(hidden);
}

// The dynamic LDS of one workgroup, in bytes from its 16-byte aligned base: the staged policy (or nothing), the lane-minor
// hidden layer, the 624 words of the stream refill, step_body's shuffle columns and the action columns. One function for
// the launch and the kernel; every offset is a multiple of 16.
struct LpLds { int policy, h, mt, order, atf, adir, bytes; };
__host__ __device__ inline LpLds lp_lds_layout(int hidden, int F, int E, bool stage) {
    LpLds l;
    l.policy = 0;
    l.h = stage ? lp_count(hidden, F, E) * (int)sizeof(float) : 0;
    l.mt = l.h + hidden * 64 * (int)sizeof(float);
    l.order = l.mt + MTN * (int)sizeof(uint32_t);
    l.atf = l.order + MG_LIFTSIM_MAX_ELEVATORS * 64;
    l.adir = l.atf + MG_LIFTSIM_MAX_ELEVATORS * 64 * (int)sizeof(int16_t);
    l.bytes = l.adir + MG_LIFTSIM_MAX_ELEVATORS * 64;
    return l;
}

struct LpPolicy {
    const float *__restrict__ params;       // [n_policies][count]
    const int32_t *__restrict__ ids;        // [n]
    int n_policies, hidden;
    float scale[8];
};

// The policy of include/metagym_hip.h for one elevator on one packed parameter block, from LDS (every lane the same block:
// same-address reads for the dense parts) or from global memory (each lane its own block). x: the eight scaled inputs;
// d: CurrentDispatchTarget; rt, up, dn: the three floor sets, bit f - 1 of word (f - 1) / 32; h: the lane's column of the
// LDS hidden layer. The loop over the records runs at run time. Returns the choice.
__device__ __forceinline__ int lp_eval(const float *__restrict__ p, int hidden, int F, int E, int el, const float (&x)[8], int d,
                                       const uint32_t (&rt)[4], const uint32_t (&up)[4], const uint32_t (&dn)[4], float *h) {
    const UnitHead o = unit_head(F, E);
    const int ur = lp_unit_record(F, E);
#pragma unroll 1
    for (int j = 0; j < hidden; j += 4) {
        const float *r[4];
        float z[4];
        unit_heads(p, ur, o, j, hidden, F, el, x, d, rt, up, dn, r, z);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (j + u < hidden) h[(j + u) * 64] = z[u] > 0.0f ? z[u] : 0.0f;
    }
    return argmax_choice(p + ur * hidden, hidden, F, h);
}

// The policy for every elevator of this lane's env, on the state as it stands: the actions into `out`.
__device__ __forceinline__ void lp_dispatch(const Env &s, const K &k, const LpPolicy &pa, const float *__restrict__ p, float *h,
                                            const PolicyActions &out) {
    const int F = k.F, E = k.E;
    uint32_t up[4], dn[4];
    hall_sets(s, F, up, dn);
#pragma unroll 1
    for (int el = 0; el < E; ++el) {
        float x[8];
        uint32_t rt[4];
        gather(s, F, el, pa.scale, x, rt);
        const int c = lp_eval(p, pa.hidden, F, E, el, x, s.i(MG_LS_DISPATCH, el), rt, up, dn, h);
        decode(out, el, c, F);
    }
}

// liftsim_rollout_kernel with the dispatcher a packed network: per step the wave's stream refill, then the policy for the
// live lanes that are not frozen, then step_body. Every lane stays in the loop for the next refill. Spare lanes shadow the
// last env's policy id and store nothing.
__global__ __launch_bounds__(64) void liftsim_policy_rollout_kernel(K k, Lay l, int n, uint8_t *arena, LpPolicy pa, int T,
                                                                    Records rec, int stage) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int H = pa.hidden;
    const LpLds lds = lp_lds_layout(H, k.F, k.E, stage != 0);
    const int lane = threadIdx.x, e0 = blockIdx.x * 64, e = e0 + lane;
    const bool live = e < n;
    const int ec = live ? e : n - 1;
    const Env s{arena, &l, n, ec};
    uint32_t *mtbuf = reinterpret_cast<uint32_t *>(smem + lds.mt);
    uint8_t (*order)[64] = reinterpret_cast<uint8_t (*)[64]>(smem + lds.order);
    const PolicyActions la{reinterpret_cast<int16_t (*)[64]>(smem + lds.atf), reinterpret_cast<int8_t (*)[64]>(smem + lds.adir),
                           lane};
    float *h = reinterpret_cast<float *>(smem + lds.h) + lane;             // the lane's column: h[j] at h[j * 64]
    const float *policy_lds = reinterpret_cast<const float *>(smem + lds.policy);

    // The env's policy, clamped. One id in the whole wave (a ballot: wave-uniform) and room for it: stage it in LDS once.
    const int count = lp_count(H, k.F, k.E);
    const mg::StagedPolicy sp = mg::stage_policy(pa.params, count, pa.ids[ec], pa.n_policies, lane, stage != 0,
                                                 reinterpret_cast<mg::v4f *>(smem + lds.policy));
    const bool staged = sp.staged;
    const float *__restrict__ own = sp.own;
    __syncthreads();                                                       // (one wave) the staged policy is in place

    double acc = 0.0;
    for (int t = 0; t < T; ++t) {
        refill_streams(s, l, arena, mtbuf, live, e0, lane);
        if (live) {
            const size_t at = (size_t)t * (size_t)n + (size_t)e;
            const bool frozen = s.b(MG_LS_OVERFLOW) || s.b(MG_LS_UNSUPPORTED);
            if (!frozen) {
                if (staged) lp_dispatch(s, k, pa, policy_lds, h, la);
                else lp_dispatch(s, k, pa, own, h, la);
            }
            step_body(s, k, lane, order, la);                              // a frozen env leaves before it reads an action
            const double reward = s.d(MG_LS_REWARD);
            acc += reward;
            store_records(rec, s, k, at, frozen, la, reward);
        }
    }
    if (live) rec.ret[e] = acc;
}

}  // namespace

extern "C" int32_t mg_liftsim_policy_param_count(int32_t hidden, int32_t floors, int32_t elevators) {
    if (int rc = check_policy_sizes(hidden, floors, elevators)) return rc;
    return lp_count(hidden, floors, elevators);
}

extern "C" int mg_liftsim_policy_rollout(const mg_liftsim_config *cfg, int32_t n_envs, void *arena, int32_t n_steps,
                                         const mg_liftsim_policy *policy, const int32_t *policy_ids, double *ret,
                                         double *rec_reward, double *rec_time_consume, double *rec_energy_consume,
                                         int32_t *rec_given_up, int32_t *rec_actions, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(arena);
    MG_REQUIRE_PTR(policy);
    MG_REQUIRE_PTR(policy_ids);
    MG_REQUIRE_PTR(ret);
    if (policy->params == nullptr) return mg::set_error(MG_ERR_NULL_POINTER, "mg_liftsim_policy needs params");
    if (int rc = check_policy_rollout("mg_liftsim_policy_rollout", "mg_liftsim_policy", cfg, n_envs, n_steps, policy)) return rc;
    // launch-uniform: the policy is staged when the whole need fits a workgroup's LDS; the rest always fits (< 27 KiB)
    const bool stage = (size_t)lp_lds_layout(policy->hidden, cfg->floors, cfg->elevators, true).bytes <= mg::LDS_LIMIT;
    const LpLds lds = lp_lds_layout(policy->hidden, cfg->floors, cfg->elevators, stage);
    mg::DeviceGuard guard(mg::device_of(arena));
    if (int rc = mg::opt_in_dynamic_lds(liftsim_policy_rollout_kernel, lds.bytes, "liftsim_policy_rollout_kernel")) return rc;
    LpPolicy pa{policy->params, policy_ids, policy->n_policies, policy->hidden, {}};
    for (int i = 0; i < 8; ++i) pa.scale[i] = policy->scale[i];
    const Records rec{ret, rec_reward, rec_time_consume, rec_energy_consume, rec_given_up, rec_actions};
    hipLaunchKernelGGL(liftsim_policy_rollout_kernel, grid(n_envs), dim3(64), (size_t)lds.bytes,
                       static_cast<hipStream_t>(stream), fold(cfg), lay(cfg, n_envs), n_envs, static_cast<uint8_t *>(arena), pa,
                       n_steps, rec, stage ? 1 : 0);
    return mg::check_launch("liftsim_policy_rollout_kernel");
}
