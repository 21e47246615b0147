// liftsim_rpolicy.hip — LiftSim closed-loop rollouts: recurrent dispatchers with a carry (mg_liftsim_rpolicy_*).
//
// A translation unit of its own on liftsim_core.h (refill_streams, step_body, K, Lay, Records, the host checks) and
// mg_closed_loop.h (stage_policy, the LDS limit and opt-in). Same flags (metagym_amd/build.py): -ffp-contract=off, which is
// what makes the policy definition of include/metagym_hip.h hold (one rounding per operation).
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
// The input gather, the floor walk, the action columns and the pad helper repeat liftsim_policy.hip's lines (lp_dispatch's
// gather, lp_walk, PolicyActions, lp_pad4): that unit is left as it is, byte for byte.
//
// All LDS is dynamic, carved at multiples of 16 bytes from a 16-byte aligned base.
#include "liftsim_core.h"

#include "mg_closed_loop.h"

namespace {

constexpr int LR_MAX_HIDDEN = 64;

typedef mg::v4f lr_v4f;

__host__ __device__ constexpr int lr_pad4(int n) { return (n + 3) & ~3; }
// floats of one hidden unit's record: b[j] wq[j] 0 0 | ws[j][0..7] | we[j][0..E-1] | wt[j][0..F] | wr[j][0..F-1] | wu | wd |
// wc[j][0..A-1] | wh[j][0..H-1], every group zero-padded to a multiple of four floats
__host__ __device__ constexpr int lr_unit_record(int hidden, int F, int E) {
    return 12 + lr_pad4(E) + lr_pad4(F + 1) + 3 * lr_pad4(F) + lr_pad4(2 * F + 2) + lr_pad4(hidden);
}
// floats of one choice's record: bo[c] 0 0 0 | wo[c][0..H-1] and zeros up to HP
__host__ __device__ constexpr int lr_choice_record(int hidden) { return 4 + lr_pad4(hidden); }
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

// The policy's actions of one step, the lane's column of two LDS arrays: step_body's Actions interface with a signed target.
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
__device__ __forceinline__ void lr_walk(float (&z)[4], const float *const (&r)[4], int off, const uint32_t (&set)[4]) {
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

// The recurrent policy of include/metagym_hip.h for one elevator on one packed parameter block, from LDS (every lane the same
// block: same-address reads for the dense parts) or from global memory (each lane its own block). x: the eight scaled
// inputs; d: CurrentDispatchTarget; rt, up, dn: the three floor sets, bit f - 1 of word (f - 1) / 32; pc, pr: the previous
// choice and reward; ho: the lane's column of the memory before the step; hn: the lane's column of the memory after it, also
// written to hc[j * n], the elevator's lines of the carry. The loops over the memory read four weights per 16-byte read and
// skip the padding (0 * h added to a sum of -0 would turn it into +0, and 0 * inf is NaN). Returns the choice.
__device__ __forceinline__ int lr_eval(const float *__restrict__ p, int hidden, int F, int E, int el, const float (&x)[8], int d,
                                       const uint32_t (&rt)[4], const uint32_t (&up)[4], const uint32_t (&dn)[4], int pc, float pr,
                                       const float *ho, float *hn, float *hc, size_t n) {
    const int hp = lr_pad4(hidden), fp = lr_pad4(F);
    const int ur = lr_unit_record(hidden, F, E), cr = 4 + hp;
    const int o_we = 12, o_wt = o_we + lr_pad4(E), o_wr = o_wt + lr_pad4(F + 1), o_wu = o_wr + fp, o_wd = o_wu + fp;
    const int o_wc = o_wd + fp, o_wh = o_wc + lr_pad4(2 * F + 2);
    const bool looked_up = d >= 0 && d <= F;
    // Four hidden units at a time, each in a register of its own: every unit still adds its terms in the definition's
    // order; the four chains are independent and share the walks over the bit sets and the reads of the old memory. A
    // block's units past H - 1 are unit H - 1 again (computed, never stored).
#pragma unroll 1
    for (int j = 0; j < hidden; j += 4) {
        const float *r[4];
        float z[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            r[u] = p + ur * min(j + u, hidden - 1);
            const lr_v4f w0 = *reinterpret_cast<const lr_v4f *>(r[u] + 4), w1 = *reinterpret_cast<const lr_v4f *>(r[u] + 8);
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
        lr_walk(z, r, o_wr, rt);
        lr_walk(z, r, o_wu, up);
        lr_walk(z, r, o_wd, dn);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float a = z[u];
            if (pc >= 0) a = a + r[u][o_wc + pc];
            a = a + r[u][1] * pr;
            z[u] = a;
        }
#pragma unroll 1
        for (int i = 0; i < hp; i += 4) {
            const lr_v4f v0 = *reinterpret_cast<const lr_v4f *>(r[0] + o_wh + i), v1 = *reinterpret_cast<const lr_v4f *>(r[1] + o_wh + i);
            const lr_v4f v2 = *reinterpret_cast<const lr_v4f *>(r[2] + o_wh + i), v3 = *reinterpret_cast<const lr_v4f *>(r[3] + o_wh + i);
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
    const float *q = p + ur * hidden;
    const int A = 2 * F + 2;
    int choice = 0;                                                      // ties and NaN logits: the lowest index
    float best = 0.0f;
    // Four choices at a time: each logit still adds its H terms in order, one rounding per operation, but the four chains
    // are independent of one another and share every read of the memory. A is even; a block's rows past A - 1 are row
    // A - 1 again (read, never compared).
#pragma unroll 1
    for (int c = 0; c < A; c += 4) {
        const float *r0 = q + cr * c, *r1 = q + cr * (c + 1);
        const float *r2 = q + cr * min(c + 2, A - 1), *r3 = q + cr * min(c + 3, A - 1);
        float l0 = r0[0], l1 = r1[0], l2 = r2[0], l3 = r3[0];
#pragma unroll 1
        for (int i = 0; i < hp; i += 4) {
            const lr_v4f v0 = *reinterpret_cast<const lr_v4f *>(r0 + 4 + i), v1 = *reinterpret_cast<const lr_v4f *>(r1 + 4 + i);
            const lr_v4f v2 = *reinterpret_cast<const lr_v4f *>(r2 + 4 + i), v3 = *reinterpret_cast<const lr_v4f *>(r3 + 4 + i);
            const float h0 = hn[i * 64];
            l0 = l0 + v0.x * h0; l1 = l1 + v1.x * h0; l2 = l2 + v2.x * h0; l3 = l3 + v3.x * h0;
            if (i + 1 < hidden) {
                const float h1 = hn[(i + 1) * 64];
                l0 = l0 + v0.y * h1; l1 = l1 + v1.y * h1; l2 = l2 + v2.y * h1; l3 = l3 + v3.y * h1;
            }
            if (i + 2 < hidden) {
                const float h2 = hn[(i + 2) * 64];
                l0 = l0 + v0.z * h2; l1 = l1 + v1.z * h2; l2 = l2 + v2.z * h2; l3 = l3 + v3.z * h2;
            }
            if (i + 3 < hidden) {
                const float h3 = hn[(i + 3) * 64];
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

// The policy for every elevator of this lane's env, on the state as it stands: the actions into `out`, the memories and the
// choices into the carry. Every elevator sees the same previous reward `pr`.
__device__ __forceinline__ void lr_dispatch(const Env &s, const K &k, const LrPolicy &pa, const float *__restrict__ p,
                                            const LrCarry &st, float pr, float *ho, float *hn, const PolicyActions &out) {
    const int F = k.F, E = k.E, H = pa.hidden;
    const size_t n = (size_t)s.n, e = (size_t)s.e;
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
        float *hc = st.h + (size_t)el * (size_t)H * n + e;               // the elevator's lines of the carry: hc[j * n]
        for (int j = 0; j < H; ++j) ho[j * 64] = hc[(size_t)j * n];
        int32_t *pcp = st.pc + (size_t)el * n + e;
        const int pc = min(*pcp, 2 * F + 1);                             // (never above: a choice this kernel wrote, or -1)
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
        const int c = lr_eval(p, H, F, E, el, x, s.i(MG_LS_DISPATCH, el), rt, up, dn, pc, pr, ho, hn, hc, n);
        *pcp = c;
        if (c < F) out.set(el, c + 1, 1);
        else if (c < 2 * F) out.set(el, c - F + 1, -1);
        else if (c == 2 * F) out.set(el, 0, 1);
        else out.set(el, -1, 1);
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
                                                 reinterpret_cast<lr_v4f *>(smem + lds.policy));
    const bool staged = sp.staged;
    const float *__restrict__ own = sp.own;
    __syncthreads();                                                       // (one wave) the staged policy is in place

    const size_t A = (size_t)(2 * k.E);
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
            if (rec.actions != nullptr)
                for (int el = 0; el < k.E; ++el) {
                    rec.actions[at * A + 2 * el] = frozen ? 0 : la.target(el);
                    rec.actions[at * A + 2 * el + 1] = frozen ? 0 : la.direction(el);
                }
            const double reward = s.d(MG_LS_REWARD);
            if (!frozen) pr = (float)reward;                               // the step's reward record (0 where it overflowed)
            acc += reward;
            if (rec.reward != nullptr) rec.reward[at] = reward;
            if (rec.timec != nullptr) rec.timec[at] = s.d(MG_LS_TIMEC);
            if (rec.energy != nullptr) rec.energy[at] = s.d(MG_LS_ENERGY);
            if (rec.given != nullptr) rec.given[at] = s.i(MG_LS_GIVEN);
        }
    }
    if (live) {
        rec.ret[e] = acc;
        st.pr[e] = pr;
    }
}

}  // namespace

extern "C" int32_t mg_liftsim_rpolicy_param_count(int32_t hidden, int32_t floors, int32_t elevators) {
    if (hidden < 1 || hidden > LR_MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", hidden, LR_MAX_HIDDEN);
    if (floors < 2 || floors > MG_LIFTSIM_MAX_FLOORS)
        return mg::set_error(MG_ERR_BAD_SIZE, "floors=%d is outside [2, %d]", floors, MG_LIFTSIM_MAX_FLOORS);
    if (elevators < 1 || elevators > MG_LIFTSIM_MAX_ELEVATORS)
        return mg::set_error(MG_ERR_BAD_SIZE, "elevators=%d is outside [1, %d]", elevators, MG_LIFTSIM_MAX_ELEVATORS);
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
    const int rc = check(cfg, n_envs, "mg_liftsim_rpolicy_rollout");
    if (rc != MG_OK) return rc;
    if (n_steps < 1) return mg::set_error(MG_ERR_BAD_SIZE, "mg_liftsim_rpolicy_rollout: n_steps = %d (at least 1)", n_steps);
    if (policy->n_policies < 1) return mg::set_error(MG_ERR_BAD_SIZE, "n_policies=%d", policy->n_policies);
    if (policy->hidden < 1 || policy->hidden > LR_MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", policy->hidden, LR_MAX_HIDDEN);
    if (policy->floors != cfg->floors || policy->elevators != cfg->elevators)
        return mg::set_error(MG_ERR_BAD_CONFIG, "the policy was built for floors=%d elevators=%d, the env has %d and %d",
                             policy->floors, policy->elevators, cfg->floors, cfg->elevators);
    if (((uintptr_t)policy->params & 15u) != 0)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_liftsim_rpolicy.params must be 16-byte aligned");
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
