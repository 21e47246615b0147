// liftsim_policy.hip — LiftSim closed-loop rollouts: learned dispatchers inside the launch (mg_liftsim_policy_*).
//
// A translation unit of its own on liftsim_core.h (refill_streams, step_body, K, Lay, Records, the host checks). Same flags
// (metagym_amd/build.py): -ffp-contract=off, which is what makes the policy definition of include/metagym_hip.h hold (one
// rounding per operation).
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
#include "liftsim_core.h"

#include "mg_closed_loop.h"

namespace {

constexpr int LP_MAX_HIDDEN = 64;

typedef mg::v4f lp_v4f;

__host__ __device__ constexpr int lp_pad4(int n) { return (n + 3) & ~3; }
// floats of one hidden unit's record: b[j] 0 0 0 | ws[j][0..7] | we[j][0..E-1] | wt[j][0..F] | wr[j][0..F-1] | wu | wd,
// every group zero-padded to a multiple of four floats
__host__ __device__ constexpr int lp_unit_record(int F, int E) { return 12 + lp_pad4(E) + lp_pad4(F + 1) + 3 * lp_pad4(F); }
// floats of one choice's record: bo[c] 0 0 0 | wo[c][0..H-1] and zeros up to HP
__host__ __device__ constexpr int lp_choice_record(int hidden) { return 4 + lp_pad4(hidden); }
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

// The policy's actions of one step, the lane's column of two LDS arrays: step_body's Actions interface with a signed
// target (LaneActions' is uint8_t, where -1 would read back as 255).
struct PolicyActions {
    int16_t (*tf)[64];
    int8_t (*dir)[64];
    int lane;
    __device__ __forceinline__ int target(int el) const { return tf[el][lane]; }
    __device__ __forceinline__ int direction(int el) const { return dir[el][lane]; }
    __device__ __forceinline__ void set(int el, int t, int d) const { tf[el][lane] = (int16_t)t; dir[el][lane] = (int8_t)d; }
};

// for f ascending in the set: z = z + w[f - 1]  (a lookup per member: one add each, nothing for the others), for four
// hidden units at once: r[u] + off is unit u's group
__device__ __forceinline__ void lp_walk(float (&z)[4], const float *const (&r)[4], int off, const uint32_t (&set)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t bits = set[q];
        while (bits) {
            const int at = off + 32 * q + __builtin_ctz(bits);
            bits &= bits - 1;
#pragma unroll
            for (int u = 0; u < 4; ++u) z[u] = z[u] + r[u][at];
        }
    }
}

// The policy of include/metagym_hip.h for one elevator on one packed parameter block, from LDS (every lane the same block:
// same-address reads for the dense parts) or from global memory (each lane its own block). x: the eight scaled inputs;
// d: CurrentDispatchTarget; rt, up, dn: the three floor sets, bit f - 1 of word (f - 1) / 32; h: the lane's column of the
// LDS hidden layer. The loops over the records run at run time; the loops over h read four weights per 16-byte read and
// skip the padding (0 * h added to a sum of -0 would turn it into +0, and 0 * inf is NaN). Returns the choice.
__device__ __forceinline__ int lp_eval(const float *__restrict__ p, int hidden, int F, int E, int el, const float (&x)[8], int d,
                                       const uint32_t (&rt)[4], const uint32_t (&up)[4], const uint32_t (&dn)[4], float *h) {
    const int hp = lp_pad4(hidden), fp = lp_pad4(F);
    const int ur = lp_unit_record(F, E), cr = 4 + hp;
    const int o_we = 12, o_wt = o_we + lp_pad4(E), o_wr = o_wt + lp_pad4(F + 1), o_wu = o_wr + fp, o_wd = o_wu + fp;
    const bool looked_up = d >= 0 && d <= F;
    // Four hidden units at a time, each in a register of its own: every unit still adds its terms in the definition's
    // order; the four chains are independent and share the walks over the bit sets. A block's units past H - 1 are unit
    // H - 1 again (computed, never stored).
#pragma unroll 1
    for (int j = 0; j < hidden; j += 4) {
        const float *r[4];
        float z[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            r[u] = p + ur * min(j + u, hidden - 1);
            const lp_v4f w0 = *reinterpret_cast<const lp_v4f *>(r[u] + 4), w1 = *reinterpret_cast<const lp_v4f *>(r[u] + 8);
            float a = r[u][0];
            a = a + w0.x * x[0];
            a = a + w0.y * x[1];
            a = a + w0.z * x[2];
            a = a + w0.w * x[3];
            a = a + w1.x * x[4];
            a = a + w1.y * x[5];
            a = a + w1.z * x[6];
            a = a + w1.w * x[7];
            a = a + r[u][o_we + el];
            if (looked_up) a = a + r[u][o_wt + d];
            z[u] = a;
        }
        lp_walk(z, r, o_wr, rt);
        lp_walk(z, r, o_wu, up);
        lp_walk(z, r, o_wd, dn);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (j + u < hidden) h[(j + u) * 64] = z[u] > 0.0f ? z[u] : 0.0f;
    }
    const float *q = p + ur * hidden;
    const int A = 2 * F + 2;
    int choice = 0;                                                      // ties and NaN logits: the lowest index
    float best = 0.0f;
    // Four choices at a time: each logit still adds its H terms in order, one rounding per operation, but the four chains
    // are independent of one another and share every read of h. A is even; a block's rows past A - 1 are row A - 1 again
    // (read, never compared).
#pragma unroll 1
    for (int c = 0; c < A; c += 4) {
        const float *r0 = q + cr * c, *r1 = q + cr * (c + 1);
        const float *r2 = q + cr * min(c + 2, A - 1), *r3 = q + cr * min(c + 3, A - 1);
        float l0 = r0[0], l1 = r1[0], l2 = r2[0], l3 = r3[0];
#pragma unroll 1
        for (int i = 0; i < hp; i += 4) {
            const lp_v4f v0 = *reinterpret_cast<const lp_v4f *>(r0 + 4 + i), v1 = *reinterpret_cast<const lp_v4f *>(r1 + 4 + i);
            const lp_v4f v2 = *reinterpret_cast<const lp_v4f *>(r2 + 4 + i), v3 = *reinterpret_cast<const lp_v4f *>(r3 + 4 + i);
            const float h0 = h[i * 64];
            l0 = l0 + v0.x * h0; l1 = l1 + v1.x * h0; l2 = l2 + v2.x * h0; l3 = l3 + v3.x * h0;
            if (i + 1 < hidden) {
                const float h1 = h[(i + 1) * 64];
                l0 = l0 + v0.y * h1; l1 = l1 + v1.y * h1; l2 = l2 + v2.y * h1; l3 = l3 + v3.y * h1;
            }
            if (i + 2 < hidden) {
                const float h2 = h[(i + 2) * 64];
                l0 = l0 + v0.z * h2; l1 = l1 + v1.z * h2; l2 = l2 + v2.z * h2; l3 = l3 + v3.z * h2;
            }
            if (i + 3 < hidden) {
                const float h3 = h[(i + 3) * 64];
                l0 = l0 + v0.w * h3; l1 = l1 + v1.w * h3; l2 = l2 + v2.w * h3; l3 = l3 + v3.w * h3;
            }
        }
        if (c == 0) best = l0;
        else if (l0 > best) { choice = c; best = l0; }                   // best is l[choice]
        if (l1 > best) { choice = c + 1; best = l1; }
        if (c + 2 < A && l2 > best) { choice = c + 2; best = l2; }
        if (c + 3 < A && l3 > best) { choice = c + 3; best = l3; }
    }
    return choice;
}

// The policy for every elevator of this lane's env, on the state as it stands: the actions into `out`.
__device__ __forceinline__ void lp_dispatch(const Env &s, const K &k, const LpPolicy &pa, const float *__restrict__ p, float *h,
                                            const PolicyActions &out) {
    const int F = k.F, E = k.E;
    uint32_t up[4], dn[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        uint32_t u = 0, d = 0;
        const int nb = min(32, F - 32 * w);
        for (int b = 0; b < nb; ++b) {
            u |= (uint32_t)(s.b(MG_LS_UP, 32 * w + b) != 0) << b;
            d |= (uint32_t)(s.b(MG_LS_DOWN, 32 * w + b) != 0) << b;
        }
        up[w] = u; dn[w] = d;
    }
#pragma unroll 1
    for (int el = 0; el < E; ++el) {
        float x[8];
        x[0] = (float)s.d(MG_LS_FLOOR, el) * pa.scale[0];
        x[1] = (float)s.d(MG_LS_VEL, el) * pa.scale[1];
        x[2] = (float)s.i(MG_LS_DIR, el) * pa.scale[2];
        x[3] = (float)s.d(MG_LS_DOOR, el) * pa.scale[3];
        x[4] = (float)s.d(MG_LS_LOAD, el) * pa.scale[4];
        x[5] = (float)s.d(MG_LS_ALARM, el) * pa.scale[5];
        x[6] = (s.b(MG_LS_OPENING, el) != 0 ? 1.0f : 0.0f) * pa.scale[6];
        x[7] = (s.b(MG_LS_CLOSING, el) != 0 ? 1.0f : 0.0f) * pa.scale[7];
        uint32_t rt[4] = {0, 0, 0, 0};
        const int nt = min(s.i(MG_LS_NTARGET, el), F);
        for (int j = 0; j < nt; ++j) {
            const int t = s.i(MG_LS_TARGETS, (int64_t)el * F + j) - 1;
            if (t < 0 || t >= F) continue;                               // (never: the list holds floors 1..F)
#pragma unroll
            for (int w = 0; w < 4; ++w) rt[w] |= (t >> 5) == w ? 1u << (t & 31) : 0u;
        }
        const int c = lp_eval(p, pa.hidden, F, E, el, x, s.i(MG_LS_DISPATCH, el), rt, up, dn, h);
        if (c < F) out.set(el, c + 1, 1);
        else if (c < 2 * F) out.set(el, c - F + 1, -1);
        else if (c == 2 * F) out.set(el, 0, 1);
        else out.set(el, -1, 1);
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
                                                 reinterpret_cast<lp_v4f *>(smem + lds.policy));
    const bool staged = sp.staged;
    const float *__restrict__ own = sp.own;
    __syncthreads();                                                       // (one wave) the staged policy is in place

    const size_t A = (size_t)(2 * k.E);
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
            if (rec.actions != nullptr)
                for (int el = 0; el < k.E; ++el) {
                    rec.actions[at * A + 2 * el] = frozen ? 0 : la.target(el);
                    rec.actions[at * A + 2 * el + 1] = frozen ? 0 : la.direction(el);
                }
            acc += s.d(MG_LS_REWARD);
            if (rec.reward != nullptr) rec.reward[at] = s.d(MG_LS_REWARD);
            if (rec.timec != nullptr) rec.timec[at] = s.d(MG_LS_TIMEC);
            if (rec.energy != nullptr) rec.energy[at] = s.d(MG_LS_ENERGY);
            if (rec.given != nullptr) rec.given[at] = s.i(MG_LS_GIVEN);
        }
    }
    if (live) rec.ret[e] = acc;
}

}  // namespace

extern "C" int32_t mg_liftsim_policy_param_count(int32_t hidden, int32_t floors, int32_t elevators) {
    if (hidden < 1 || hidden > LP_MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", hidden, LP_MAX_HIDDEN);
    if (floors < 2 || floors > MG_LIFTSIM_MAX_FLOORS)
        return mg::set_error(MG_ERR_BAD_SIZE, "floors=%d is outside [2, %d]", floors, MG_LIFTSIM_MAX_FLOORS);
    if (elevators < 1 || elevators > MG_LIFTSIM_MAX_ELEVATORS)
        return mg::set_error(MG_ERR_BAD_SIZE, "elevators=%d is outside [1, %d]", elevators, MG_LIFTSIM_MAX_ELEVATORS);
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
    const int rc = check(cfg, n_envs, "mg_liftsim_policy_rollout");
    if (rc != MG_OK) return rc;
    if (n_steps < 1) return mg::set_error(MG_ERR_BAD_SIZE, "mg_liftsim_policy_rollout: n_steps = %d (at least 1)", n_steps);
    if (policy->n_policies < 1) return mg::set_error(MG_ERR_BAD_SIZE, "n_policies=%d", policy->n_policies);
    if (policy->hidden < 1 || policy->hidden > LP_MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", policy->hidden, LP_MAX_HIDDEN);
    if (policy->floors != cfg->floors || policy->elevators != cfg->elevators)
        return mg::set_error(MG_ERR_BAD_CONFIG, "the policy was built for floors=%d elevators=%d, the env has %d and %d",
                             policy->floors, policy->elevators, cfg->floors, cfg->elevators);
    if (((uintptr_t)policy->params & 15u) != 0)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_liftsim_policy.params must be 16-byte aligned");
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
