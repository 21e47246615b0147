// liftsim_rpolicy.hip — LiftSim closed-loop rollouts: recurrent dispatchers with a carry (mg_liftsim_rpolicy_*).
//
// A translation unit of its own on liftsim_policy_core.h: what it shares with liftsim_policy.hip (LiftPolicy's terms in
// LiftPolicy's order, the hall-call sets, the input gather, the logit loop and argmax, the decode, the record stores, the
// host checks), and through it liftsim_core.h (refill_streams, step_body, K, Lay, Records) and mg_closed_loop.h
// (stage_policy, the LDS limit and opt-in). Same flags (metagym_amd/build.py): -ffp-contract=off, which is what makes the
// policy definition of include/metagym_hip.h hold (one rounding per operation).
//
// Mapping: liftsim_policy_rollout_kernel's — one lane per building, one wave per workgroup, {refill, policy, step_body} T
// times. Per elevator and step: the elevator's memory h[el] comes from the carry ([E][H][N]: H coalesced loads) into the
// lane's column of a first LDS array; the new memory is formed four units at a time (each unit's chain in a register of its
// own, the floor walks shared) into a second column and written back to the carry; the logits are formed from the second
// column four choices at a time, the running argmax holding one logit and one index. The previous choice is read from and
// written to the carry ([E][N]) per elevator; the previous reward lives in a register for the launch. Weights: a wave with
// one policy id stages its policy in LDS when the host found that the launch's LDS need fits a workgroup; otherwise each
// lane reads its own block from global memory. Both inline lr_eval, so the bits are equal.
//
// All LDS is dynamic, carved at multiples of 16 bytes from a 16-byte aligned base.
#include "liftsim_policy_core.h"

namespace {

// floats of one hidden unit's record: b[j] wq[j] 0 0 | ws[j][0..7] | we[j][0..E-1] | wt[j][0..F] | wr[j][0..F-1] | wu | wd |
// wc[j][0..A-1] | wh[j][0..H-1], every group zero-padded to a multiple of four floats
__host__ __device__ constexpr int lr_unit_record(int hidden, int F, int E) {
    return 12 + pad4(E) + pad4(F + 1) + 3 * pad4(F) + pad4(2 * F + 2) + pad4(hidden);
}
// floats of one choice's record: bo[c] 0 0 0 | wo[c][0..H-1] and zeros up to HP
__host__ __device__ constexpr int lr_choice_record(int hidden) { return 4 + pad4(hidden); }
__host__ __device__ constexpr int lr_count(int hidden, int F, int E) {
    return hidden * lr_unit_record(hidden, F, E) + (2 * F + 2) * lr_choice_record(hidden);
}

// The dynamic LDS of one workgroup, in bytes from its 16-byte aligned base: the staged policy (or nothing), the two
// lane-minor memory columns (before and after the step), the 624 words of the stream refill, step_body's shuffle columns
// and the action columns. One function for the launch and the kernel; every offset is a multiple of 16.
struct LrLds { int policy, hold, hnew, mt, order, atf, adir, bytes; };
__host__ __device__ inline LrLds lr_lds_layout(int hidden, int F, int E, bool stage) {
    LrLds l;
    l.policy = 0;
    l.hold = stage ? lr_count(hidden, F, E) * (int)sizeof(float) : 0;
    l.hnew = l.hold + hidden * 64 * (int)sizeof(float);
    l.mt = l.hnew + hidden * 64 * (int)sizeof(float);
    l.order = l.mt + MTN * (int)sizeof(uint32_t);
    // the per-elevator columns are sized by E, not by the most a building can have: with the default building and H = 32
    // that is what lets four workgroups, one per SIMD, share a CU's 160 KiB with their policies staged
    l.atf = l.order + E * 64;
    l.adir = l.atf + E * 64 * (int)sizeof(int16_t);
    l.bytes = l.adir + E * 64;
    return l;
}

struct LrPolicy {
    const float *__restrict__ params;       // [n_policies][count]
    const int32_t *__restrict__ ids;        // [n]
    int n_policies, hidden;
    float scale[8];
};

// The carry: h [E][H][N], prev_choice [E][N], prev_reward [N], env index fastest.
struct LrCarry {
    float *h;
    int32_t *pc;
    float *pr;
};

// The recurrent policy of include/metagym_hip.h for one elevator on one packed parameter block, from LDS (every lane the same
// block: same-address reads for the dense parts) or from global memory (each lane its own block). x: the eight scaled
// inputs; d: CurrentDispatchTarget; rt, up, dn: the three floor sets, bit f - 1 of word (f - 1) / 32; pc, pr: the previous
// choice and reward; ho: the lane's column of the memory before the step; hn: the lane's column of the memory after it, also
// written to hc[j * n], the elevator's lines of the carry. The loops over the memory read four weights per 16-byte read and
// skip the padding (0 * h added to a sum of -0 would turn it into +0, and 0 * inf is NaN). Returns the choice.
__device__ __forceinline__ int lr_eval(const float *__restrict__ p, int hidden, int F, int E, int el, const float (&x)[8], int d,
                                       const uint32_t (&rt)[4], const uint32_t (&up)[4], const uint32_t (&dn)[4], int pc, float pr,
                                       const float *ho, float *hn, float *hc, size_t n) {
    const UnitHead o = unit_head(F, E);
    const int hp = pad4(hidden), ur = lr_unit_record(hidden, F, E);
    const int o_wc = o.wd + pad4(F), o_wh = o_wc + pad4(2 * F + 2);
    // The four units of a block also share the reads of the old memory.
#pragma unroll 1
    for (int j = 0; j < hidden; j += 4) {
        const float *r[4];
        float z[4];
        unit_heads(p, ur, o, j, hidden, F, el, x, d, rt, up, dn, r, z);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float a = z[u];
            if (pc >= 0) a = a + r[u][o_wc + pc];
            a = a + r[u][1] * pr;
            z[u] = a;
        }
#pragma unroll 1
        for (int i = 0; i < hp; i += 4) {
            const mg::v4f v0 = *reinterpret_cast<const mg::v4f *>(r[0] + o_wh + i), v1 = *reinterpret_cast<const mg::v4f *>(r[1] + o_wh + i);
            const mg::v4f v2 = *reinterpret_cast<const mg::v4f *>(r[2] + o_wh + i), v3 = *reinterpret_cast<const mg::v4f *>(r[3] + o_wh + i);
            const float h0 = ho[i * 64];
            z[0] = z[0] + v0.x * h0; z[1] = z[1] + v1.x * h0; z[2] = z[2] + v2.x * h0; z[3] = z[3] + v3.x * h0;
            if (i + 1 < hidden) {
                const float h1 = ho[(i + 1) * 64];
                z[0] = z[0] + v0.y * h1; z[1] = z[1] + v1.y * h1; z[2] = z[2] + v2.y * h1; z[3] = z[3] + v3.y * h1;
            }
            if (i + 2 < hidden) {
                const float h2 = ho[(i + 2) * 64];
                z[0] = z[0] + v0.z * h2; z[1] = z[1] + v1.z * h2; z[2] = z[2] + v2.z * h2; z[3] = z[3] + v3.z * h2;
            }
            if (i + 3 < hidden) {
                const float h3 = ho[(i + 3) * 64];
                z[0] = z[0] + v0.w * h3; z[1] = z[1] + v1.w * h3; z[2] = z[2] + v2.w * h3; z[3] = z[3] + v3.w * h3;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (j + u < hidden) {
                const float v = z[u] > 1.0f ? 1.0f : (z[u] < -1.0f ? -1.0f : z[u]);
                hn[(j + u) * 64] = v;
                hc[(size_t)(j + u) * n] = v;
            }
    }
    return argmax_choice(p + ur * hidden, hidden, F, hn);
}

// The policy for every elevator of this lane's env, on the state as it stands: the actions into `out`, the memories and the
// choices into the carry. Every elevator sees the same previous reward `pr`.
__device__ __forceinline__ void lr_dispatch(const Env &s, const K &k, const LrPolicy &pa, const float *__restrict__ p,
                                            const LrCarry &st, float pr, float *ho, float *hn, const PolicyActions &out) {
    const int F = k.F, E = k.E, H = pa.hidden;
    const size_t n = (size_t)s.n, e = (size_t)s.e;
    uint32_t up[4], dn[4];
    hall_sets(s, F, up, dn);
#pragma unroll 1
    for (int el = 0; el < E; ++el) {
        float *hc = st.h + (size_t)el * (size_t)H * n + e;               // the elevator's lines of the carry: hc[j * n]
        for (int j = 0; j < H; ++j) ho[j * 64] = hc[(size_t)j * n];
        int32_t *pcp = st.pc + (size_t)el * n + e;
        const int pc = min(*pcp, 2 * F + 1);                             // (never above: a choice this kernel wrote, or -1)
        float x[8];
        uint32_t rt[4];
        gather(s, F, el, pa.scale, x, rt);
        const int c = lr_eval(p, H, F, E, el, x, s.i(MG_LS_DISPATCH, el), rt, up, dn, pc, pr, ho, hn, hc, n);
        *pcp = c;
        decode(out, el, c, F);
    }
}

// liftsim_policy_rollout_kernel with a memory: per step the wave's stream refill, then the policy for the live lanes that are
// not frozen, then step_body, then the previous reward. Every lane stays in the loop for the next refill. Spare lanes shadow
// the last env's policy id and read and store nothing of the carry.
__global__ __launch_bounds__(64) void liftsim_rpolicy_rollout_kernel(K k, Lay l, int n, uint8_t *arena, LrPolicy pa, LrCarry st,
                                                                     int T, Records rec, int stage) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int H = pa.hidden;
    const LrLds lds = lr_lds_layout(H, k.F, k.E, stage != 0);
    const int lane = threadIdx.x, e0 = blockIdx.x * 64, e = e0 + lane;
    const bool live = e < n;
    const int ec = live ? e : n - 1;
    const Env s{arena, &l, n, ec};
    uint32_t *mtbuf = reinterpret_cast<uint32_t *>(smem + lds.mt);
    uint8_t (*order)[64] = reinterpret_cast<uint8_t (*)[64]>(smem + lds.order);
    const PolicyActions la{reinterpret_cast<int16_t (*)[64]>(smem + lds.atf), reinterpret_cast<int8_t (*)[64]>(smem + lds.adir),
                           lane};
    float *ho = reinterpret_cast<float *>(smem + lds.hold) + lane;         // the lane's columns: h[j] at [j * 64]
    float *hn = reinterpret_cast<float *>(smem + lds.hnew) + lane;
    const float *policy_lds = reinterpret_cast<const float *>(smem + lds.policy);

    // The env's policy, clamped. One id in the whole wave (a ballot: wave-uniform) and room for it: stage it in LDS once.
    const int count = lr_count(H, k.F, k.E);
    const mg::StagedPolicy sp = mg::stage_policy(pa.params, count, pa.ids[ec], pa.n_policies, lane, stage != 0,
                                                 reinterpret_cast<mg::v4f *>(smem + lds.policy));
    const bool staged = sp.staged;
    const float *__restrict__ own = sp.own;
    __syncthreads();                                                       // (one wave) the staged policy is in place

    float pr = live ? st.pr[e] : 0.0f;
    double acc = 0.0;
    for (int t = 0; t < T; ++t) {
        refill_streams(s, l, arena, mtbuf, live, e0, lane);
        if (live) {
            const size_t at = (size_t)t * (size_t)n + (size_t)e;
            const bool frozen = s.b(MG_LS_OVERFLOW) || s.b(MG_LS_UNSUPPORTED);
            if (!frozen) {
                if (staged) lr_dispatch(s, k, pa, policy_lds, st, pr, ho, hn, la);
                else lr_dispatch(s, k, pa, own, st, pr, ho, hn, la);
            }
            step_body(s, k, lane, order, la);                              // a frozen env leaves before it reads an action
            const double reward = s.d(MG_LS_REWARD);
            if (!frozen) pr = (float)reward;                               // the step's reward record (0 where it overflowed)
            acc += reward;
            store_records(rec, s, k, at, frozen, la, reward);
        }
    }
    if (live) {
        rec.ret[e] = acc;
        st.pr[e] = pr;
    }
}

}  // namespace

extern "C" int32_t mg_liftsim_rpolicy_param_count(int32_t hidden, int32_t floors, int32_t elevators) {
    if (int rc = check_policy_sizes(hidden, floors, elevators)) return rc;
    return lr_count(hidden, floors, elevators);
}

extern "C" int mg_liftsim_rpolicy_rollout(const mg_liftsim_config *cfg, int32_t n_envs, void *arena, int32_t n_steps,
                                          const mg_liftsim_rpolicy *policy, const int32_t *policy_ids,
                                          const mg_liftsim_policy_state *state, double *ret, double *rec_reward,
                                          double *rec_time_consume, double *rec_energy_consume, int32_t *rec_given_up,
                                          int32_t *rec_actions, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(arena);
    MG_REQUIRE_PTR(policy);
    MG_REQUIRE_PTR(policy_ids);
    MG_REQUIRE_PTR(state);
    MG_REQUIRE_PTR(ret);
    if (policy->params == nullptr) return mg::set_error(MG_ERR_NULL_POINTER, "mg_liftsim_rpolicy needs params");
    if (state->h == nullptr || state->prev_choice == nullptr || state->prev_reward == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_liftsim_policy_state needs h, prev_choice and prev_reward");
    if (int rc = check_policy_rollout("mg_liftsim_rpolicy_rollout", "mg_liftsim_rpolicy", cfg, n_envs, n_steps, policy)) return rc;
    if ((((uintptr_t)state->h | (uintptr_t)state->prev_choice | (uintptr_t)state->prev_reward) & 3u) != 0)
        return mg::set_error(MG_ERR_BAD_CONFIG, "the arrays of mg_liftsim_policy_state must be 4-byte aligned");
    // launch-uniform: the policy is staged when the whole need fits a workgroup's LDS; the rest always fits (< 44 KiB)
    const bool stage = (size_t)lr_lds_layout(policy->hidden, cfg->floors, cfg->elevators, true).bytes <= mg::LDS_LIMIT;
    const LrLds lds = lr_lds_layout(policy->hidden, cfg->floors, cfg->elevators, stage);
    mg::DeviceGuard guard(mg::device_of(arena));
    if (int rc = mg::opt_in_dynamic_lds(liftsim_rpolicy_rollout_kernel, lds.bytes, "liftsim_rpolicy_rollout_kernel")) return rc;
    LrPolicy pa{policy->params, policy_ids, policy->n_policies, policy->hidden, {}};
    for (int i = 0; i < 8; ++i) pa.scale[i] = policy->scale[i];
    const LrCarry st{state->h, state->prev_choice, state->prev_reward};
    const Records rec{ret, rec_reward, rec_time_consume, rec_energy_consume, rec_given_up, rec_actions};
    hipLaunchKernelGGL(liftsim_rpolicy_rollout_kernel, grid(n_envs), dim3(64), (size_t)lds.bytes,
                       static_cast<hipStream_t>(stream), fold(cfg), lay(cfg, n_envs), n_envs, static_cast<uint8_t *>(arena), pa,
                       st, n_steps, rec, stage ? 1 : 0);
    return mg::check_launch("liftsim_rpolicy_rollout_kernel");
}
