// liftsim.hip — LiftSim elevator dispatch (reference metagym/liftsim/environment/) for N buildings at once, bit for bit.
//
// Env e is the reference's LiftSim after env.seed(s_e): it owns a CPython `random` stream (weights, the UNIFORM
// generator, the boarding shuffle) and a numpy legacy stream (the CUSTOM generator's poisson / multinomial). One step is,
// in the reference's order (mansion_manager.py run_mansion): time += dt; generate persons (appended on the NEW end of
// their floor's up / down queue); set the actions; run the elevators in index order (door, velocity planner, energy,
// unloading, loading); hall buttons from the queue lengths; random.shuffle of the elevator indices; boarding in that
// order, oldest person first, deleting from the middle; give-ups from the old end; the sums, the reward and one slot of
// the statistics ring.
//
// libm in draw decisions: poisson's exp(-lambda) and the binomial inversion's exp(n log q) come from host tables built
// with glibc (mg_liftsim_config); the one call left on the device is normalvariate's log(u2) (OCML), see DESIGN.md §3.10.
//
// Mapping: one lane per building, one wave per workgroup. State is structure-of-arrays, [item][N], so the wave's lanes
// touch neighbouring words whenever they touch the same item (elevator scalars, queue heads and lengths, the oldest
// person of a queue); the stream records are [N][1248] (two key blocks per stream). A stream never refills inside a
// step: between steps the wave writes the refill of every lane's current block into its other block (refill_ahead), so
// draws are lane-local reads however divergent the lanes are.
//
// The step is a device function (step_body) shared by liftsim_step_kernel and liftsim_rollout_kernel; the latter runs
// {refill, actions, step} T times in one launch, the actions read from actions[t] or made on the spot by rule_policy, the
// reference's rule-based dispatcher (tests/rule_benchmark/dispatcher.py Rule_dispatcher.policy) as a lane-local function.
//
// This file: the kernels it launches, the reset, the rule-based dispatcher and the C entry points. step_body, the stream
// refill and the host checks, which liftsim_policy.hip shares, are in liftsim_core.h.
#include "liftsim_core.h"

namespace {

constexpr double HUGE_PRIORITY = 1.0e8;   // mansion/utils.py HUGE

__device__ void reset_env(const Env &s, const K &k) {
    for (int el = 0; el < k.E; ++el) {
        s.d(MG_LS_POS, el) = 0.0; s.d(MG_LS_VEL, el) = 0.0; s.d(MG_LS_LOAD, el) = 0.0; s.d(MG_LS_DOOR, el) = 0.0;
        s.d(MG_LS_KEEP, el) = 0.0; s.d(MG_LS_ALARM, el) = 0.0; s.d(MG_LS_FLOOR, el) = 1.0;
        s.i(MG_LS_DIR, el) = 0; s.i(MG_LS_DISPATCH, el) = 0; s.i(MG_LS_DISPATCH_DIR, el) = 1;
        s.i(MG_LS_NTARGET, el) = 0; s.i(MG_LS_EFLAGS, el) = 0;
        s.b(MG_LS_OPENING, el) = 0; s.b(MG_LS_CLOSING, el) = 0;
        for (int w = 0; w < 4; ++w) s.at<uint32_t>(MG_LS_CLICKED, el * 4 + w) = 0;
        s.i(MG_LS_NLOADED, el) = 0; s.i(MG_LS_NENT, el) = 0; s.i(MG_LS_NEXIT, el) = 0;
        for (int f = 0; f < k.F; ++f) s.i(MG_LS_TARGETS, (int64_t)el * k.F + f) = 0;
    }
    for (int q = 0; q < 2 * k.F; ++q) { s.i(MG_LS_QHEAD, q) = 0; s.i(MG_LS_QLEN, q) = 0; }
    for (int f = 0; f < k.F; ++f) { s.b(MG_LS_UP, f) = 0; s.b(MG_LS_DOWN, f) = 0; }
    s.d(MG_LS_TIME) = 0.0;
    s.d(MG_LS_LASTGEN) = 0.0;
    s.b(MG_LS_INVALID) = 0;
}

__global__ __launch_bounds__(64) void liftsim_seed_kernel(K k, Lay l, int n, uint8_t *arena, uint32_t seed_base,
                                                          const uint32_t *seeds) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    const Env s{arena, &l, n, e};
    const uint32_t sd = seeds != nullptr ? seeds[e] : seed_base + (uint32_t)e;
    uint32_t *py = s.key(MG_LS_PYKEY), *np = s.key(MG_LS_NPKEY);
    mt::init_by_array1(py, sd);
    mt::refill_into(py, py + MTN);
    mt::init_genrand(np, sd);
    mt::refill_into(np, np + MTN);
    s.i(MG_LS_PYP) = MTN; s.i(MG_LS_PYV) = 1; s.i(MG_LS_NPP) = MTN; s.i(MG_LS_NPV) = 1;
    s.i(MG_LS_TIDX) = 0; s.i(MG_LS_SHEAD) = 0; s.i(MG_LS_SCOUNT) = 0;
    s.b(MG_LS_OVERFLOW) = 0; s.b(MG_LS_UNSUPPORTED) = 0;
    for (int q = 0; q < 2 * k.F; ++q) { s.at<int8_t>(MG_LS_RP_HOLDER, q) = 0; s.d(MG_LS_RP_PRIORITY, q) = 0.0; }
    reset_env(s, k);
    zero_outputs(s);
}

__global__ __launch_bounds__(64) void liftsim_reset_kernel(K k, Lay l, int n, uint8_t *arena, const uint8_t *mask) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n || (mask != nullptr && mask[e] == 0)) return;
    reset_env(Env{arena, &l, n, e}, k);
}

// Where a step's actions come from: the caller's int32 [2E] row, or the lane's column of the dispatcher's LDS output.
struct RowActions {
    const int32_t *a;
    __device__ __forceinline__ int target(int el) const { return a[2 * el]; }
    __device__ __forceinline__ int direction(int el) const { return a[2 * el + 1]; }
};

struct LaneActions {
    uint8_t (*tf)[64];
    int8_t (*dir)[64];
    int lane;
    __device__ __forceinline__ int target(int el) const { return tf[el][lane]; }
    __device__ __forceinline__ int direction(int el) const { return dir[el][lane]; }
    __device__ __forceinline__ void set(int el, int t, int d) const { tf[el][lane] = (uint8_t)t; dir[el][lane] = (int8_t)d; }
};

// Rule_dispatcher.policy(env.state) (tests/rule_benchmark/dispatcher.py) for this lane's env: the actions into `out`.
//
// Every hall call (floor, side) has a holder and the holder's priority (the reference's two address dictionaries):
// RP_HOLDER / RP_PRIORITY, [side * F + floor - 1][N] in the arena. The elevators wait in a FIFO, 0..E-1 at first; the one
// in front bids by its Direction, and an elevator that loses its call joins the FIFO again. The quirks are the
// reference's: the down branch emits indicator +1; a fallback writes a priority without comparing one and displaces
// nobody; the Direction == 0 branch does not put the loser's action back to (0, 1); Velocity < EPSILON is signed.
//
// The FIFO is a ring of MG_LIFTSIM_MAX_ELEVATORS entries in LDS. It cannot overrun: with c_i the copies of elevator i in
// the FIFO and h_i the calls it holds, c_i + h_i starts at 1 and never grows (a dequeue takes one copy and gives at
// most one call, a displacement takes one call and gives one copy), so the FIFO holds at most E entries at any time.
// It ends: a call's priority strictly rises with every take after the first, and an elevator's bid for a call is a
// fixed number. A push on a full ring returns false all the same (the caller flags `unsupported`).
__device__ bool rule_policy(const Env &s, const K &k, uint8_t (*ring)[64], const LaneActions &out) {
    const int F = k.F, E = k.E, lane = out.lane;
    constexpr int RING = MG_LIFTSIM_MAX_ELEVATORS;
    uint32_t up[4], dn[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        uint32_t u = 0, d = 0;
        const int nb = min(32, F - 32 * w);
        for (int b = 0; b < nb; ++b) {
            const int f = 32 * w + b;
            u |= (uint32_t)(s.b(MG_LS_UP, f) != 0) << b;
            d |= (uint32_t)(s.b(MG_LS_DOWN, f) != 0) << b;
            s.at<int8_t>(MG_LS_RP_HOLDER, f) = -1; s.at<int8_t>(MG_LS_RP_HOLDER, F + f) = -1;
            s.d(MG_LS_RP_PRIORITY, f) = -HUGE_PRIORITY; s.d(MG_LS_RP_PRIORITY, F + f) = -HUGE_PRIORITY;
        }
        up[w] = u; dn[w] = d;
    }
    for (int el = 0; el < E; ++el) { ring[el][lane] = (uint8_t)el; out.set(el, 0, 1); }
    int head = 0, cnt = E;
    bool ok = true;
    auto push = [&](int el) {
        if (cnt == RING) { ok = false; return; }
        ring[(head + cnt) & (RING - 1)][lane] = (uint8_t)el;
        ++cnt;
    };
    while (cnt > 0 && ok) {
        const int el = ring[head][lane];
        head = (head + 1) & (RING - 1);
        --cnt;
        const int dir = s.i(MG_LS_DIR, el);
        const double fl = s.d(MG_LS_FLOOR, el);
        if (dir != 0) {
            const bool upw = dir > 0;
            const int side = upw ? 0 : F, other = upw ? F : 0;
            const bool slow = s.d(MG_LS_VEL, el) < EPS;
            // ReservedTargetFloors as a bit set
            uint32_t tm[4] = {0, 0, 0, 0};
            const int nt = s.i(MG_LS_NTARGET, el);
            for (int j = 0; j < nt; ++j) {
                const int t = s.i(MG_LS_TARGETS, (int64_t)el * F + j) - 1;
#pragma unroll
                for (int w = 0; w < 4; ++w) tm[w] |= (t >> 5) == w ? 1u << (t & 31) : 0u;
            }
            double sel_p = -HUGE_PRIORITY;
            int sel = -1;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                uint32_t bits = upw ? up[w] : dn[w];
                while (bits) {
                    const int b = __builtin_ctz(bits);
                    bits &= bits - 1;
                    const int f = 32 * w + b + 1;
                    const double ff = (double)f;
                    if (upw ? ff < fl - EPS : ff > fl + EPS) continue;
                    double p = upw ? fl - ff : -fl + ff;
                    if ((tm[w] >> b) & 1u) { p = p + 5.0; p = p < 0.0 ? p : 0.0; }
                    if (slow) p -= 5.0;
                    if (p > s.d(MG_LS_RP_PRIORITY, side + f - 1) && p > sel_p) { sel_p = p; sel = f; }
                }
            }
            if (sel > 0) {
                out.set(el, sel, 1);
                const int h = s.at<int8_t>(MG_LS_RP_HOLDER, side + sel - 1);
                if (h >= 0) { out.set(h, 0, 1); push(h); }
                s.at<int8_t>(MG_LS_RP_HOLDER, side + sel - 1) = (int8_t)el;
                s.d(MG_LS_RP_PRIORITY, side + sel - 1) = sel_p;
            } else {
                // nothing to take on its own side: the highest unheld down call (moving up), the lowest unheld up call
                int found = -1;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    uint32_t bits = upw ? dn[w] : up[w];
                    while (bits) {
                        const int b = __builtin_ctz(bits);
                        bits &= bits - 1;
                        const int f = 32 * w + b + 1;
                        if (s.at<int8_t>(MG_LS_RP_HOLDER, other + f - 1) < 0 && (upw || found < 0)) found = f;
                    }
                }
                if (found >= 0) {
                    out.set(el, found, upw ? -1 : 1);
                    s.at<int8_t>(MG_LS_RP_HOLDER, other + found - 1) = (int8_t)el;
                    s.d(MG_LS_RP_PRIORITY, other + found - 1) = upw ? -fl - EPS + (double)found : fl + EPS - (double)found;
                }
            }
        } else {
            double sel_p = -HUGE_PRIORITY;
            int sel = -1, side = 0;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    uint32_t bits = half == 0 ? up[w] : dn[w];
                    while (bits) {
                        const int b = __builtin_ctz(bits);
                        bits &= bits - 1;
                        const int f = 32 * w + b + 1;
                        const double p = -fabs((double)f - fl);
                        if (p > s.d(MG_LS_RP_PRIORITY, half * F + f - 1) && p > sel_p) { sel_p = p; sel = f; side = half * F; }
                    }
                }
            }
            if (sel > 0) {
                out.set(el, sel, side == 0 ? 1 : -1);
                const int h = s.at<int8_t>(MG_LS_RP_HOLDER, side + sel - 1);
                if (h >= 0) push(h);   // its action stays as it is
                s.at<int8_t>(MG_LS_RP_HOLDER, side + sel - 1) = (int8_t)el;
                s.d(MG_LS_RP_PRIORITY, side + sel - 1) = sel_p;
            }
        }
    }
    return ok;
}

__global__ __launch_bounds__(64) void liftsim_step_kernel(K k, Lay l, int n, uint8_t *arena, const int32_t *actions) {
    __shared__ uint32_t lds[MTN];
    __shared__ uint8_t order[MG_LIFTSIM_MAX_ELEVATORS][64];   // the lane's shuffled elevator indices, in its own column
    const int lane = threadIdx.x, e0 = blockIdx.x * 64, e = e0 + lane;
    const bool live = e < n;
    const Env s{arena, &l, n, live ? e : e0};
    refill_streams(s, l, arena, lds, live, e0, lane);
    if (!live) return;
    step_body(s, k, lane, order, RowActions{actions + (size_t)e * (size_t)(2 * k.E)});
}

// T steps in one launch: per step the wave's stream refill, then the actions (row t of `actions`, or rule_policy on the
// state as it stands), then the step. Every lane stays in the loop for the next refill: a frozen or invalid env leaves
// step_body early, not the kernel. ret[e] adds the T rewards in step order from 0.0.
template <bool RULE>
__global__ __launch_bounds__(64) void liftsim_rollout_kernel(K k, Lay l, int n, uint8_t *arena, const int32_t *actions,
                                                             int T, Records rec) {
    __shared__ uint32_t lds[MTN];
    __shared__ uint8_t order[MG_LIFTSIM_MAX_ELEVATORS][64];
    __shared__ uint8_t ring[RULE ? MG_LIFTSIM_MAX_ELEVATORS : 1][64];
    __shared__ uint8_t atf[RULE ? MG_LIFTSIM_MAX_ELEVATORS : 1][64];
    __shared__ int8_t adir[RULE ? MG_LIFTSIM_MAX_ELEVATORS : 1][64];
    const int lane = threadIdx.x, e0 = blockIdx.x * 64, e = e0 + lane;
    const bool live = e < n;
    const Env s{arena, &l, n, live ? e : e0};
    const size_t A = (size_t)(2 * k.E);
    double acc = 0.0;
    for (int t = 0; t < T; ++t) {
        refill_streams(s, l, arena, lds, live, e0, lane);
        if (live) {
            const size_t at = (size_t)t * (size_t)n + (size_t)e;
            if (RULE) {
                const LaneActions la{atf, adir, lane};
                const bool frozen = s.b(MG_LS_OVERFLOW) || s.b(MG_LS_UNSUPPORTED);
                if (!frozen && !rule_policy(s, k, ring, la)) s.b(MG_LS_UNSUPPORTED) = 1;
                step_body(s, k, lane, order, la);
                if (rec.actions != nullptr)
                    for (int el = 0; el < k.E; ++el) {
                        rec.actions[at * A + 2 * el] = frozen ? 0 : la.target(el);
                        rec.actions[at * A + 2 * el + 1] = frozen ? 0 : la.direction(el);
                    }
            } else {
                step_body(s, k, lane, order, RowActions{actions + at * A});
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

// Rule_dispatcher.policy for every env, the actions as int32 [N][2E]
__global__ __launch_bounds__(64) void liftsim_rule_policy_kernel(K k, Lay l, int n, uint8_t *arena, int32_t *actions) {
    __shared__ uint8_t ring[MG_LIFTSIM_MAX_ELEVATORS][64];
    __shared__ uint8_t atf[MG_LIFTSIM_MAX_ELEVATORS][64];
    __shared__ int8_t adir[MG_LIFTSIM_MAX_ELEVATORS][64];
    const int lane = threadIdx.x, e = blockIdx.x * 64 + lane;
    if (e >= n) return;
    const Env s{arena, &l, n, e};
    const LaneActions la{atf, adir, lane};
    const bool ok = rule_policy(s, k, ring, la);
    if (!ok) s.b(MG_LS_UNSUPPORTED) = 1;
    int32_t *row = actions + (size_t)e * (size_t)(2 * k.E);
    for (int el = 0; el < k.E; ++el) {
        row[2 * el] = ok ? la.target(el) : 0;
        row[2 * el + 1] = ok ? la.direction(el) : 1;
    }
}

__global__ __launch_bounds__(64) void liftsim_statistics_kernel(K k, Lay l, int n, uint8_t *arena) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    const Env s{arena, &l, n, e};
    const int head = s.i(MG_LS_SHEAD), cnt = s.i(MG_LS_SCOUNT);
    int64_t sd = 0, sg = 0, sa = 0;
    double sw = 0.0, se = 0.0;
    for (int j = 0, r = head; j < cnt; ++j, r = r + 1 == k.W ? 0 : r + 1) {
        sd += s.i(MG_LS_SD, r); sg += s.i(MG_LS_SG, r); sa += s.i(MG_LS_SA, r);
        sw = sw + s.d(MG_LS_SW, r); se = se + s.d(MG_LS_SE, r);
    }
    s.at<int64_t>(MG_LS_ST_D, 0) = sd; s.at<int64_t>(MG_LS_ST_G, 0) = sg; s.at<int64_t>(MG_LS_ST_A, 0) = sa;
    s.d(MG_LS_ST_W) = sw; s.d(MG_LS_ST_E) = se;
}

}  // namespace

extern "C" int mg_liftsim_layout(const mg_liftsim_config *cfg, int32_t n_envs, int64_t *offsets, int64_t *total_bytes) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(offsets);
    MG_REQUIRE_PTR(total_bytes);
    const int rc = check(cfg, n_envs, "mg_liftsim_layout");
    if (rc != MG_OK) return rc;
    const Lay l = lay(cfg, n_envs);
    for (int f = 0; f < MG_LS_NFIELDS; ++f) offsets[f] = l.off[f];
    *total_bytes = l.total;
    return MG_OK;
}

extern "C" int mg_liftsim_seed(const mg_liftsim_config *cfg, int32_t n_envs, void *arena, uint32_t seed_base,
                               const uint32_t *seeds, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(arena);
    const int rc = check(cfg, n_envs, "mg_liftsim_seed");
    if (rc != MG_OK) return rc;
    mg::DeviceGuard guard(mg::device_of(arena));
    hipLaunchKernelGGL(liftsim_seed_kernel, grid(n_envs), dim3(64), 0, static_cast<hipStream_t>(stream), fold(cfg),
                       lay(cfg, n_envs), n_envs, static_cast<uint8_t *>(arena), seed_base, seeds);
    return mg::check_launch("liftsim_seed_kernel");
}

extern "C" int mg_liftsim_reset(const mg_liftsim_config *cfg, int32_t n_envs, void *arena, const uint8_t *mask,
                                void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(arena);
    const int rc = check(cfg, n_envs, "mg_liftsim_reset");
    if (rc != MG_OK) return rc;
    mg::DeviceGuard guard(mg::device_of(arena));
    hipLaunchKernelGGL(liftsim_reset_kernel, grid(n_envs), dim3(64), 0, static_cast<hipStream_t>(stream), fold(cfg),
                       lay(cfg, n_envs), n_envs, static_cast<uint8_t *>(arena), mask);
    return mg::check_launch("liftsim_reset_kernel");
}

extern "C" int mg_liftsim_step(const mg_liftsim_config *cfg, int32_t n_envs, void *arena, const int32_t *actions,
                               void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(arena);
    MG_REQUIRE_PTR(actions);
    const int rc = check(cfg, n_envs, "mg_liftsim_step");
    if (rc != MG_OK) return rc;
    mg::DeviceGuard guard(mg::device_of(arena));
    hipLaunchKernelGGL(liftsim_step_kernel, grid(n_envs), dim3(64), 0, static_cast<hipStream_t>(stream), fold(cfg),
                       lay(cfg, n_envs), n_envs, static_cast<uint8_t *>(arena), actions);
    return mg::check_launch("liftsim_step_kernel");
}

extern "C" int mg_liftsim_statistics(const mg_liftsim_config *cfg, int32_t n_envs, void *arena, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(arena);
    const int rc = check(cfg, n_envs, "mg_liftsim_statistics");
    if (rc != MG_OK) return rc;
    mg::DeviceGuard guard(mg::device_of(arena));
    hipLaunchKernelGGL(liftsim_statistics_kernel, grid(n_envs), dim3(64), 0, static_cast<hipStream_t>(stream), fold(cfg),
                       lay(cfg, n_envs), n_envs, static_cast<uint8_t *>(arena));
    return mg::check_launch("liftsim_statistics_kernel");
}

extern "C" int mg_liftsim_rule_policy(const mg_liftsim_config *cfg, int32_t n_envs, void *arena, int32_t *actions_out,
                                      void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(arena);
    MG_REQUIRE_PTR(actions_out);
    const int rc = check(cfg, n_envs, "mg_liftsim_rule_policy");
    if (rc != MG_OK) return rc;
    mg::DeviceGuard guard(mg::device_of(arena));
    hipLaunchKernelGGL(liftsim_rule_policy_kernel, grid(n_envs), dim3(64), 0, static_cast<hipStream_t>(stream), fold(cfg),
                       lay(cfg, n_envs), n_envs, static_cast<uint8_t *>(arena), actions_out);
    return mg::check_launch("liftsim_rule_policy_kernel");
}

extern "C" int mg_liftsim_rollout(const mg_liftsim_config *cfg, int32_t n_envs, void *arena, int32_t policy,
                                  const int32_t *actions, int32_t n_steps, double *ret, double *rec_reward,
                                  double *rec_time_consume, double *rec_energy_consume, int32_t *rec_given_up,
                                  int32_t *rec_actions, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(arena);
    MG_REQUIRE_PTR(ret);
    if (policy == MG_LIFTSIM_POLICY_ACTIONS) MG_REQUIRE_PTR(actions);
    const int rc = check(cfg, n_envs, "mg_liftsim_rollout");
    if (rc != MG_OK) return rc;
    if (n_steps < 1) return mg::set_error(MG_ERR_BAD_SIZE, "mg_liftsim_rollout: n_steps = %d", n_steps);
    if (policy != MG_LIFTSIM_POLICY_ACTIONS && policy != MG_LIFTSIM_POLICY_RULE)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_liftsim_rollout: policy = %d", policy);
    if (policy == MG_LIFTSIM_POLICY_ACTIONS && rec_actions != nullptr)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_liftsim_rollout: rec_actions records the rule policy's actions only");
    mg::DeviceGuard guard(mg::device_of(arena));
    const Records rec{ret, rec_reward, rec_time_consume, rec_energy_consume, rec_given_up, rec_actions};
    if (policy == MG_LIFTSIM_POLICY_RULE)
        hipLaunchKernelGGL(liftsim_rollout_kernel<true>, grid(n_envs), dim3(64), 0, static_cast<hipStream_t>(stream),
                           fold(cfg), lay(cfg, n_envs), n_envs, static_cast<uint8_t *>(arena), actions, n_steps, rec);
    else
        hipLaunchKernelGGL(liftsim_rollout_kernel<false>, grid(n_envs), dim3(64), 0, static_cast<hipStream_t>(stream),
                           fold(cfg), lay(cfg, n_envs), n_envs, static_cast<uint8_t *>(arena), actions, n_steps, rec);
    return mg::check_launch("liftsim_rollout_kernel");
}
