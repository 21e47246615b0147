// liftsim_policy_core.h — what LiftSim's two learned dispatchers share: the part of the policy definition of
// include/metagym_hip.h that LiftPolicy and LiftRecurrentPolicy have in common, written once. liftsim_policy.hip and
// liftsim_rpolicy.hip include it and nothing else does; each keeps its own copy (anonymous namespace), its record and LDS
// layouts, its eval and dispatch, its kernel and its entry points.
#pragma once
#include "liftsim_core.h"

#include "mg_closed_loop.h"

namespace {

constexpr int MAX_HIDDEN = 64;

__host__ __device__ constexpr int pad4(int n) { return (n + 3) & ~3; }

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
__device__ __forceinline__ void walk(float (&z)[4], const float *const (&r)[4], int off, const uint32_t (&set)[4]) {
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

// The two hall-call sets of the env as it stands, bit f - 1 of word (f - 1) / 32: built once per step.
__device__ __forceinline__ void hall_sets(const Env &s, int F, uint32_t (&up)[4], uint32_t (&dn)[4]) {
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
}

// Elevator el's eight scaled inputs and its reserved floors as a set like the hall-call sets.
__device__ __forceinline__ void gather(const Env &s, int F, int el, const float (&scale)[8], float (&x)[8], uint32_t (&rt)[4]) {
    x[0] = (float)s.d(MG_LS_FLOOR, el) * scale[0];
    x[1] = (float)s.d(MG_LS_VEL, el) * scale[1];
    x[2] = (float)s.i(MG_LS_DIR, el) * scale[2];
    x[3] = (float)s.d(MG_LS_DOOR, el) * scale[3];
    x[4] = (float)s.d(MG_LS_LOAD, el) * scale[4];
    x[5] = (float)s.d(MG_LS_ALARM, el) * scale[5];
    x[6] = (s.b(MG_LS_OPENING, el) != 0 ? 1.0f : 0.0f) * scale[6];
    x[7] = (s.b(MG_LS_CLOSING, el) != 0 ? 1.0f : 0.0f) * scale[7];
#pragma unroll
    for (int w = 0; w < 4; ++w) rt[w] = 0;
    const int nt = min(s.i(MG_LS_NTARGET, el), F);
    for (int j = 0; j < nt; ++j) {
        const int t = s.i(MG_LS_TARGETS, (int64_t)el * F + j) - 1;
        if (t < 0 || t >= F) continue;                                   // (never: the list holds floors 1..F)
#pragma unroll
        for (int w = 0; w < 4; ++w) rt[w] |= (t >> 5) == w ? 1u << (t & 31) : 0u;
    }
}

// Where the groups that both unit records begin with sit in a record: b . . . | ws[8] | we | wt | wr | wu | wd, every
// group zero-padded to a multiple of four floats. (Each offset is the one before plus a width: with wr + 2 * fp for wd,
// liftsim_policy_rollout_kernel grew a 68-byte private segment.)
struct UnitHead { int we, wt, wr, wu, wd; };
__host__ __device__ constexpr UnitHead unit_head(int F, int E) {
    const int fp = pad4(F), we = 12, wt = we + pad4(E), wr = wt + pad4(F + 1), wu = wr + fp, wd = wu + fp;
    return UnitHead{we, wt, wr, wu, wd};
}

// LiftPolicy's terms in LiftPolicy's order, for the four hidden units j .. j + 3 of the block at p whose records are `ur`
// floats apart: r[u] becomes unit u's record and z[u] its bias, the eight ws terms, we, the wt lookup and the three floor
// walks. Each unit is in a register of its own and adds its terms in the definition's order; the four chains are
// independent and share the walks over the bit sets. A block's units past H - 1 are unit H - 1 again (the caller computes
// them and never stores them).
__device__ __forceinline__ void unit_heads(const float *__restrict__ p, int ur, const UnitHead &o, int j, int hidden, int F, int el,
                                           const float (&x)[8], int d, const uint32_t (&rt)[4], const uint32_t (&up)[4],
                                           const uint32_t (&dn)[4], const float *(&r)[4], float (&z)[4]) {
    const bool looked_up = d >= 0 && d <= F;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        r[u] = p + ur * min(j + u, hidden - 1);
        const mg::v4f w0 = *reinterpret_cast<const mg::v4f *>(r[u] + 4), w1 = *reinterpret_cast<const mg::v4f *>(r[u] + 8);
        float a = r[u][0];
        a = a + w0.x * x[0];
        a = a + w0.y * x[1];
        a = a + w0.z * x[2];
        a = a + w0.w * x[3];
        a = a + w1.x * x[4];
        a = a + w1.y * x[5];
        a = a + w1.z * x[6];
        a = a + w1.w * x[7];
        a = a + r[u][o.we + el];
        if (looked_up) a = a + r[u][o.wt + d];
        z[u] = a;
    }
    walk(z, r, o.wr, rt);
    walk(z, r, o.wu, up);
    walk(z, r, o.wd, dn);
}

// The choice: the index of the largest of the A = 2 F + 2 logits l[c] = bo[c] + sum_j wo[c][j] * h[j], whose records start
// at q; h is the lane's column of the hidden layer (h[j] at h[j * 64]). The loop over h reads four weights per 16-byte read
// and skips the padding (0 * h added to a sum of -0 would turn it into +0, and 0 * inf is NaN).
__device__ __forceinline__ int argmax_choice(const float *__restrict__ q, int hidden, int F, const float *h) {
    const int hp = pad4(hidden), cr = 4 + hp;
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
            const mg::v4f v0 = *reinterpret_cast<const mg::v4f *>(r0 + 4 + i), v1 = *reinterpret_cast<const mg::v4f *>(r1 + 4 + i);
            const mg::v4f v2 = *reinterpret_cast<const mg::v4f *>(r2 + 4 + i), v3 = *reinterpret_cast<const mg::v4f *>(r3 + 4 + i);
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

// Choice c as elevator el's action: up to floor c + 1, down to floor c - F + 1, target 0, or target -1.
__device__ __forceinline__ void decode(const PolicyActions &out, int el, int c, int F) {
    if (c < F) out.set(el, c + 1, 1);
    else if (c < 2 * F) out.set(el, c - F + 1, -1);
    else if (c == 2 * F) out.set(el, 0, 1);
    else out.set(el, -1, 1);
}

// The records of step `at` (t * n + e) that the caller asked for; a frozen env records the action (0, 0). `reward` is the
// env's reward record, read once by the caller. (k by reference: with E passed by value liftsim_policy_rollout_kernel took
// two more AGPRs.)
__device__ __forceinline__ void store_records(const Records &rec, const Env &s, const K &k, size_t at, bool frozen,
                                              const PolicyActions &la, double reward) {
    const size_t A = (size_t)(2 * k.E);
    if (rec.actions != nullptr)
        for (int el = 0; el < k.E; ++el) {
            rec.actions[at * A + 2 * el] = frozen ? 0 : la.target(el);
            rec.actions[at * A + 2 * el + 1] = frozen ? 0 : la.direction(el);
        }
    if (rec.reward != nullptr) rec.reward[at] = reward;
    if (rec.timec != nullptr) rec.timec[at] = s.d(MG_LS_TIMEC);
    if (rec.energy != nullptr) rec.energy[at] = s.d(MG_LS_ENERGY);
    if (rec.given != nullptr) rec.given[at] = s.i(MG_LS_GIVEN);
}

// Host: the hidden size both policies accept
int check_hidden(int32_t hidden) {
    if (hidden < 1 || hidden > MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", hidden, MAX_HIDDEN);
    return MG_OK;
}

// The sizes a *_param_count function accepts
int check_policy_sizes(int32_t hidden, int32_t floors, int32_t elevators) {
    if (int rc = check_hidden(hidden)) return rc;
    if (floors < 2 || floors > MG_LIFTSIM_MAX_FLOORS)
        return mg::set_error(MG_ERR_BAD_SIZE, "floors=%d is outside [2, %d]", floors, MG_LIFTSIM_MAX_FLOORS);
    if (elevators < 1 || elevators > MG_LIFTSIM_MAX_ELEVATORS)
        return mg::set_error(MG_ERR_BAD_SIZE, "elevators=%d is outside [1, %d]", elevators, MG_LIFTSIM_MAX_ELEVATORS);
    return MG_OK;
}

// The checks of a *_rollout entry point between its pointer checks and its launch plan: `who` is the entry point and
// `what` the descriptor (mg_liftsim_policy or mg_liftsim_rpolicy: same fields, different types).
template <class Policy>
int check_policy_rollout(const char *who, const char *what, const mg_liftsim_config *cfg, int32_t n_envs, int32_t n_steps,
                         const Policy *policy) {
    if (int rc = check(cfg, n_envs, who)) return rc;
    if (n_steps < 1) return mg::set_error(MG_ERR_BAD_SIZE, "%s: n_steps = %d (at least 1)", who, n_steps);
    if (policy->n_policies < 1) return mg::set_error(MG_ERR_BAD_SIZE, "n_policies=%d", policy->n_policies);
    if (int rc = check_hidden(policy->hidden)) return rc;
    if (policy->floors != cfg->floors || policy->elevators != cfg->elevators)
        return mg::set_error(MG_ERR_BAD_CONFIG, "the policy was built for floors=%d elevators=%d, the env has %d and %d",
                             policy->floors, policy->elevators, cfg->floors, cfg->elevators);
    if (((uintptr_t)policy->params & 15u) != 0) return mg::set_error(MG_ERR_BAD_CONFIG, "%s.params must be 16-byte aligned", what);
    return MG_OK;
}

}  // namespace
