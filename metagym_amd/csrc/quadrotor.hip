// quadrotor.hip — batched Quadrotor engine for gfx950: one lane per environment.
//
// Replaces, for N environments per launch, the reference's per-object Python hot path
//   QuadrotorSim._run_internal   metagym/quadrotor/quadrotorsim.py:122-210  (substep())
//   QuadrotorSim._check_failure  quadrotorsim.py:212-221                    (fail test in substep loop)
//   QuadrotorSim.step            quadrotorsim.py:295-304                    (sub-step loop)
//   get_sensor / get_state / _get_pitch_roll_yaw  quadrotorsim.py:111-120,260-293  (observe())
//   Quadrotor.step / _get_reward / _check_collision  env.py:127-165,211-260 (finish_step())
//   Quadrotor.reset / QuadrotorSim.reset  env.py:116-125, quadrotorsim.py:239-258 (reset kernel)
//
// Design (MI355X): the state of one env is 116 B of SoA (pos f32x3, vel f64x3, omega f64x3,
// propw f32x4, R f32x9, ct i32). A lane loads its env's state with 23 coalesced loads (lane e reads
// base[c*N + e]), runs all int(dt/precision)=10 Euler sub-steps in registers, and writes state,
// obs, reward and done back once. The 16-float observation row is transposed through LDS so the
// wave stores 4 KiB contiguous as dwordx4. No MFMA: the work is ~4 kflop of small-vector f32/f64
// algebra per env-step with no contraction dimension to tile.
//
// Precision: the reference mixes f32 arrays, f64 arrays and python floats; the dtype NumPy (NEP 50)
// evaluates each expression in is mirrored exactly (see oracle/quadrotor_oracle.c for the annotated
// restatement this kernel is tested against). The translation unit is compiled with
// -ffp-contract=off so no a*b+c is fused — NumPy never fuses — which makes this kernel bit-identical
// to the CPU oracle for everything except atan2f (OCML vs glibc, <= 2 ulp).
//
// This file: the kernels it launches (targets, step, reset), what only they use (range_safe, collision_flat, the lean fold,
// config_is_xframe), the plan and the C entry points. The device functions and the host-side folding that
// quadrotor_tasks.hip and quadrotor_policy.hip share are in quadrotor_core.h.
#include "quadrotor_core.h"

namespace {

// The range test of STEP_STOCK_SHADOW's main path: m = max |p_c| over the tested positions, S = fail_range_sq32 with
// 2^-100 <= S < +inf (fold_lean). range_safe(m, S) implies sumsq3(p) <= S for every p with |p_c| <= m:
//   q = fl(m * m) >= fl(p_c * p_c) (rounding is monotone), the double sum of the three products is at most 3q (2q and 3q
//   are doubles, so neither addition rounds above them) and its f32 rounding at most 3q * (1 + 2^-24) + 2^-150.
//   t = fl(q * K) >= q * K * (1 - 2^-24) - 2^-150 with K = 3 + 2^-18, and K * (1 - 2^-24) - 3 * (1 + 2^-24) > 2^-19,
//   so t - sumsq3(p) > q * 2^-19 - 2^-149 >= 0 for q >= 2^-130: sumsq3(p) <= t < S. For q < 2^-130, sumsq3(p) < 2^-128 < S.
// It is false for m = NaN, m = +inf and an overflowing product. It is monotone in m, so it is `m < pos_safe32` for the
// least float32 at which it fails: fold_pos_safe finds that value for mg_quadrotor_plan_fold and the tests. The kernel
// holds the product form because its argument block has no free word for pos_safe32 (see QuadK): two v_mul_f32 per step.
__host__ __device__ __forceinline__ bool range_safe(float m, float S) {
    const float q = m * m;
    return q * 0x1.80002p+1f < S;
}

// collision() for k.map == nullptr, established on the host (FLAT): any is 0 and the x and y extents are never read,
// so the test is (long)floor(lo_z) < 0 || (long)ceil(hi_z) < 0 with lo_z, hi_z as selected above. It equals lo_z < 0:
//   lo_z, hi_z not NaN: lo_z <= hi_z, floor(lo_z) <= ceil(hi_z), and the conversion is monotone (it saturates: the
//     high word is v_cvt_i32_f64 of floor(x * 2^-32)), so the first test decides. floor(x) < 0 exactly when x < 0
//     (-0.0 -> -0 -> 0, a tiny negative -> -1, -inf and every finite x below -2^63 -> a negative long).
//   new z NaN: both selects return the new z, and (long)NaN is 0 here (v_cvt_i32_f64 and v_cvt_u32_f64 of NaN are
//     0): no hit. NaN < 0 is false as well.
//   old z NaN (new z not): both selects return the new z, so lo_z = hi_z = new z: the first case.
__device__ __forceinline__ bool collision_flat(double op_z, double np_z) {
    const double lo = op_z < np_z ? op_z : np_z;
    return lo < 0.0;
}

// ---- pre-reset, all-float32 sub-step: define_velocity_control_task, quadrotorsim.py:306-319 -------
// Before reset() every simulator array is float32 (quadrotorsim.py:20-28), so _run_internal runs
// entirely in float32 there (python floats are weak). Only used once per env object to roll the
// velocity_control target trajectory; general (non-specialised) formulation, one lane.
struct Lane32 {
    float p[3], v[3], w[3], pw[4], R[9], Ri[9];
};

__device__ void substep_f32state(const QuadK &k, Lane32 &s, const float *eff32) {
    float prop_force_z = 0.0f, prop_torque[3] = {0.0f, 0.0f, 0.0f}, me[4];
    const float ct2_32 = (float)k.ct2;
    for (int i = 0; i < 4; ++i) {
        const float e32 = eff32[i];
        float phi_w = k.phi32 * s.pw[i];
        me[i] = k.phi_over_ra32 * (e32 - phi_w);
        float d_prop_w = k.inv_jm32 * (me[i] - k.mm32);
        float w_m = s.pw[i] + k.prec32 * d_prop_w;
        const float *pc = &k.pc[3 * i];
        float bv[3], cr[3];
        mv_f32(s.Ri, s.v, bv);
        cross_f32(s.w, pc, cr);
        float v_1 = bv[2] + cr[2] * k.lm[i];
        float sign = v_1 > 0 ? 1.0f : -1.0f;
        float thrust = ((k.ct0_32 * w_m) * w_m + (k.ct1_32 * w_m) * v_1) + ((ct2_32 * v_1) * v_1) * sign;
        s.pw[i] = w_m;
        prop_force_z = prop_force_z + thrust;
        float a[3] = {-0.0f, -0.0f, -thrust};
        cross_f32(a, pc, cr);
        prop_torque[0] += cr[0]; prop_torque[1] += cr[1]; prop_torque[2] += cr[2];
    }
    prop_torque[2] += ((-me[0] + me[1]) - me[2]) + me[3];
    float DfRi[9], tmp[3], f_drag[3], t_drag[3];
    mm_f32(k.df, s.Ri, DfRi);
    mv_f32(DfRi, s.v, tmp);
    const float nv = -sqrtf(sumsq3(s.v));
    for (int c = 0; c < 3; ++c) f_drag[c] = nv * tmp[c];
    mv_f32(k.dm, s.w, tmp);
    const float nw = -sqrtf(sumsq3(s.w));
    for (int c = 0; c < 3; ++c) t_drag[c] = nw * tmp[c];
    const float g[3] = {0.0f, 0.0f, -9.8f};
    float f_grav[3], t_grav[3], body_acc[3], t_all[3], acc[3];
    mv_f32(s.Ri, g, f_grav);
    for (int c = 0; c < 3; ++c) f_grav[c] = f_grav[c] * k.quality32;
    cross_f32(f_grav, k.cog, t_grav);
    for (int c = 0; c < 3; ++c) {
        const float pf = (c == 2) ? prop_force_z : 0.0f;
        const float f_all = (pf + f_grav[c]) + f_drag[c];
        t_all[c] = (prop_torque[c] + (-t_grav[c])) + t_drag[c];
        body_acc[c] = f_all / k.quality32;
    }
    mv_f32(s.R, body_acc, acc);
    const float half_dt2 = (float)k.half_dt2, half_dt = (float)k.half_dt;
    for (int c = 0; c < 3; ++c) s.p[c] = s.p[c] + (s.v[c] * k.prec32 + half_dt2 * acc[c]);
    for (int c = 0; c < 3; ++c) s.v[c] = s.v[c] + k.prec32 * acc[c];
    float alpha[3], tw[3];
    mv_f32(k.iinv, t_all, alpha);
    for (int c = 0; c < 3; ++c) tw[c] = s.w[c] + half_dt * alpha[c];
    float S[9] = {0.0f, -tw[2], tw[1], tw[2], 0.0f, -tw[0], -tw[1], tw[0], 0.0f};
    float RS[9];
    mm_f32(s.R, S, RS);
    for (int c = 0; c < 9; ++c) s.R[c] = s.R[c] + k.prec32 * RS[c];
    for (int c = 0; c < 3; ++c) s.w[c] = s.w[c] + k.prec32 * alpha[c];
    double Rd[9];
    inv3(s.R, s.Ri, Rd);
}

__global__ void quadrotor_targets_kernel(QuadK k, int nt, const float *actions, float *targets) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Lane32 s;
    for (int c = 0; c < 3; ++c) { s.p[c] = 0.0f; s.v[c] = 0.0f; s.w[c] = 0.0f; }
    for (int c = 0; c < 4; ++c) s.pw[c] = 0.0f;
    for (int c = 0; c < 9; ++c) { s.R[c] = (c % 4 == 0) ? 1.0f : 0.0f; s.Ri[c] = s.R[c]; }
    for (int t = 0; t < nt; ++t) {
        float eff32[4];
        for (int i = 0; i < 4; ++i) {
            double d = (double)actions[4 * t + i];
            d = d > k.max_v ? k.max_v : (d < k.min_v ? k.min_v : d);
            eff32[i] = (float)d;
        }
        for (int it = 0; it < k.times; ++it) substep_f32state(k, s, eff32);
        targets[3 * t] = s.v[0]; targets[3 * t + 1] = s.v[1]; targets[3 * t + 2] = s.v[2];
    }
}

// ---- kernels ---------------------------------------------------------------------------------------

// The step kernel's argument block as the kernarg segment lays it out, and a pointer to it that the
// optimiser cannot relate to the kernel's own argument loads (see the epilogue of the step kernel).
struct KArgs { QuadK k; mg_quadrotor_state st; StepIO io; int n; int n_steps; };
static_assert(sizeof(QuadK) == 448 && sizeof(KArgs) == 560, "kernel argument layout (the prologue touches its nine 64-byte lines)");
typedef const __attribute__((address_space(4))) KArgs KArgsC;
__device__ __forceinline__ KArgsC *kernargs_fresh() {
    KArgsC *p = (KArgsC *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// Forms of the step kernel (launch_plan picks one per launch):
//   STEP_GENERIC       every configuration: k.times sub-steps in a loop, each guarded by the failure freeze.
//   STEP_STOCK         the stock configuration, resolved on the host: SIMPLE, quality a power of two,
//                      times == 10, fused auto-reset. The ten sub-steps are straight-line code (no branch):
//                      with auto-reset a failed env restarts in the same launch, so its state after the failing
//                      sub-step is never stored, observed or rewarded, and the sub-steps can run unconditionally.
//                      A failed lane's later sub-steps may reach inf / NaN; nothing converts them to an integer or
//                      an address (collision() runs only for fail == 0) and the reset overwrites them.
//   STEP_STOCK_SHADOW  STEP_STOCK for one-step launches of at most one wave per SIMD: the lane's reset draw is made
//                      for every lane while the prologue loads are in flight, so the restart only moves values.
//                      With more than one wave per SIMD the VALU is busy during the loads, and ~150 extra VALU on
//                      every wave would cost more than the branch it saves.
//                      Its sub-steps take sqrt and 1/det without the library's range steps (update_derived_fast);
//                      a wave with an argument out of range redoes the step with the library's (see the kernel).
//                      The three failure tests are part of that range (fold_lean), so its sub-steps hold no
//                      failure_code(); a plan whose thresholds cannot be folded takes STEP_STOCK instead.
// Four options, also resolved on the host:
//   XF   (both stock forms) the stock X frame of propellers (config_is_xframe, substep<>); any other SIMPLE layout
//        keeps XF = false.
//   BUF  (STEP_STOCK_SHADOW) state, action and outputs addressed through buffer resources (ld_soa / st_soa) when
//        every array of the launch spans less than 2^31 bytes. Not in STEP_STOCK: there the step loop keeps the resources
//        live across the sub-steps and the scalar file spills (14 / 36 SGPR spills with / without XF).
//   FLAT (both stock forms) no collision map (k.map == nullptr): the collision test is the z test of collision_flat().
//        A configuration with a map keeps collision().
//   HOVER (STEP_STOCK_SHADOW) the hovering task, so the epilogue holds no test of k.task.
enum StepForm { STEP_GENERIC = 0, STEP_STOCK = 1, STEP_STOCK_SHADOW = 2 };

// Phase timeline (diagnostic builds only, -DMG_QUAD_PHASE_STAMPS; scripts/quad_phase_timeline.py reads it): lane 0 of
// every wave of the STEP_STOCK_SHADOW kernel records the 100 MHz wall clock at entry, after the state loads, after
// sub-step 10, after the state stores and after the obs stores are issued (slots 0-4), the shader clock at entry (5),
// HW_ID | XCC_ID << 32 (6) and the number of fast-path fallbacks << 32 (7). mg_quadrotor_phase_stamps copies the
// buffer to the host. The default library has neither the stamps nor the symbol.
#ifdef MG_QUAD_PHASE_STAMPS
constexpr int PHASE_STAMPS = 5, PHASE_SLOTS = 8, PHASE_MAX_WAVES = 4096;
__device__ uint64_t g_phase_stamps[PHASE_MAX_WAVES * PHASE_SLOTS];
#define MG_PHASE_STAMP(i)                                                                 \
    do {                                                                                  \
        if (SHADOW) {                                                                     \
            __builtin_amdgcn_sched_barrier(0);                                            \
            stamp[i] = __builtin_amdgcn_s_memrealtime();                                  \
            __builtin_amdgcn_sched_barrier(0);                                            \
        }                                                                                 \
    } while (0)
#else
#define MG_PHASE_STAMP(i) \
    do {                  \
    } while (0)
#endif
constexpr int STOCK_TIMES = 10;
#ifndef MG_QUAD_FASTPATH
#define MG_QUAD_FASTPATH 1         // STEP_STOCK_SHADOW: in-range sqrt and 1/det in the sub-steps (0: the library's, A/B)
#endif
#ifndef MG_QUAD_SUBSTEP_UNROLL
#define MG_QUAD_SUBSTEP_UNROLL 9   // of the first nine stock sub-steps (the tenth is peeled): 9 = straight-line, 1 = rolled
#endif

template <bool SIMPLE, int FORM, bool XF = false, bool BUF = false, bool FLAT = false, bool HOVER = false>
__global__ __launch_bounds__(BLOCK) void quadrotor_step_kernel(QuadK k, mg_quadrotor_state st, StepIO io,
                                                               int n, int n_steps_arg) {
    constexpr bool STOCK = FORM != STEP_GENERIC;
    constexpr bool SHADOW = FORM == STEP_STOCK_SHADOW;
    static_assert(!STOCK || SIMPLE, "the stock forms are SIMPLE");
    static_assert(STOCK || !XF, "XF is an option of the stock forms");
    static_assert(SHADOW || !BUF, "BUF is an option of STEP_STOCK_SHADOW");
    static_assert(STOCK || !FLAT, "FLAT is an option of the stock forms");
    static_assert(SHADOW || !HOVER, "HOVER is an option of STEP_STOCK_SHADOW");
    constexpr bool FAST = SHADOW && MG_QUAD_FASTPATH;   // in-range sqrt / 1/det (update_derived_fast), whole-step fallback below
    const int n_steps = SHADOW ? 1 : n_steps_arg;
    __shared__ float tiles[WAVES_PER_BLOCK][mg::WAVE * (OBS_DIM + 1)];
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = e < n;
    const int el = live ? e : n - 1;  // out-of-range lanes shadow the last env, stores are masked
    float *tile = tiles[threadIdx.x / mg::WAVE];

    // Latency, not bandwidth, bounds a 65 536-env launch (one wave per SIMD). Three round trips used to
    // run back to back: state loads, then ~9 scalar kernarg-line misses scattered through the prologue,
    // then the action load. Issue them together: touch every 64-byte line of the 560-byte kernarg
    // segment now (later s_loads hit the scalar cache) and fetch the first action before the state.
    {
        const uint32_t *ka = (const uint32_t *)__builtin_amdgcn_kernarg_segment_ptr();
        uint32_t touch = 0;
#pragma unroll
        for (int line = 0; line < (int)((sizeof(QuadK) + sizeof(mg_quadrotor_state) + sizeof(StepIO) + 8 + 63) / 64); ++line)
            touch |= ka[line * 16];
        asm volatile("" ::"s"(touch));
    }
#ifdef MG_QUAD_PHASE_STAMPS
    uint64_t stamp[PHASE_STAMPS];
    uint32_t fallbacks = 0;
    const uint64_t clock_in = __builtin_readcyclecounter();
#endif
    MG_PHASE_STAMP(0);   // entry
    bool ok = true;   // FAST: every argument of every update_derived so far was in range
    float4 a_next;
    Lane s;
    int ct;
    uint32_t episode = 0;
    ResetDraw rd;
    if (SHADOW) {
        // Loads in the order of their use: the episode counter (the reset draw needs nothing else), the action,
        // then rot / vel / omega (inv3 and the norms), then the rest. The VALU would otherwise idle through the
        // ~2-3 k cycles of the prologue burst; the draw and the derived values fill it, each behind a partial
        // vmcnt wait. The sched_barriers keep the compiler from sinking the work to its first use.
        episode = ld_soa<BUF>(st.episode, 1, n, 0, el);
        a_next = ld_soa<BUF>(reinterpret_cast<const float4 *>(io.action), 1, n, 0, el);
        load_state<true, BUF>(st, n, el, s, ct);
        __builtin_amdgcn_sched_barrier(0);
        rd = reset_draw(k, el, episode);
#pragma unroll
        for (int c = 0; c < 3; ++c) asm volatile("" : "+v"(rd.v[c]), "+v"(rd.w[c]));   // not sunk into the restart branch
        asm volatile("" : "+v"(rd.nv), "+v"(rd.nw));
        __builtin_amdgcn_sched_barrier(0);
        derive_lane(s);   // the library's sqrt / 1/det: hidden behind the loads, and exact for reset states (v = w = 0)
        __builtin_amdgcn_sched_barrier(0);
    } else {
        a_next = reinterpret_cast<const float4 *>(io.action)[el];
        __builtin_amdgcn_sched_barrier(0);   // keep this load ahead of the state loads (it would be sunk to its first use)
        if (STOCK || k.auto_reset) episode = st.episode[el];
        load_lane(st, n, el, s, ct);
    }
    const uint32_t episode_in = episode;
    // All prologue loads land here (vmcnt = 0), not at their first use inside the step loop: there the wait
    // would be re-executed by every later step of a rollout and would also drain that step's freshly issued
    // action prefetch and the previous step's stores (2.5 us per step at K > 1; free at K = 1).
    __builtin_amdgcn_s_waitcnt(0x0F70);
    MG_PHASE_STAMP(1);   // state loaded (and derived)

    for (int t = 0; t < n_steps; ++t) {
        const size_t off = (size_t)t * n;
        const float4 a = a_next;
        if (t + 1 < n_steps)      // prefetch the next step's action behind this step's arithmetic
            a_next = reinterpret_cast<const float4 *>(io.action)[off + n + el];
        // quadrotorsim.py:130-134: clamp the (f32-valued) python float against python floats
        const float av[4] = {a.x, a.y, a.z, a.w};
        float eff32[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double d = (double)av[i];
            d = d > k.max_v ? k.max_v : (d < k.min_v ? k.min_v : d);
            eff32[i] = (float)d;
        }
        ct += 1;                                                            // env.py:128
        const double old_pos[3] = {(double)s.p[0] + k.xoff, (double)s.p[1] + k.yoff,
                                   (double)(s.p[2] + k.zoff32)};            // env.py:131-133
        int fail = 0;
        if (FAST) {
            // Straight-line sub-steps without the failure tests: fold_lean has moved them into `ok`. The velocity and the
            // body-rate test are the upper edges of all_in_range's windows. The range test is a running max-norm: pmax is
            // the largest |p_c| of the ten tested positions, and range_safe(pmax) implies sumsq3(p) <= fail_range_sq32 at
            // each of them (see range_safe). A NaN component is dropped by the max; it makes sumsq3(p) NaN and the
            // reference's test `NaN > S` false, so it cannot fail that sample either, and the other components cannot
            // alone: each is at most pmax. (If every |p_c| of every sample is NaN, pmax is NaN, the compare is false and
            // the wave takes the fallback, which is always right.) So a lane with `ok` set has failed no test at any
            // sub-step: fail = 0. A lane that fails one has `ok` clear, and the wave redoes the step below with the full
            // tests.
            float pmax = 0.0f;
#pragma unroll MG_QUAD_SUBSTEP_UNROLL
            for (int it = 0; it < STOCK_TIMES - 1; ++it) {
                substep<SIMPLE, true, XF, true>(k, s, eff32, false, ok);
                const float m3 = fmaxf(fmaxf(fabsf(s.p[0]), fabsf(s.p[1])), fabsf(s.p[2]));
                pmax = it == 0 ? m3 : fmaxf(pmax, m3);
            }
            substep<SIMPLE, true, XF, true>(k, s, eff32, true, ok);
            pmax = fmaxf(pmax, fmaxf(fmaxf(fabsf(s.p[0]), fabsf(s.p[1])), fabsf(s.p[2])));
            ok = ok & range_safe(pmax, k.fail_range_sq32);
        } else if (STOCK) {      // straight-line sub-steps (see StepForm); the first failure code is kept
#pragma unroll MG_QUAD_SUBSTEP_UNROLL
            for (int it = 0; it < STOCK_TIMES - 1; ++it) {
                substep<SIMPLE, true, XF, FAST>(k, s, eff32, false, ok);
                const int code = failure_code(k, s);
                fail = fail ? fail : code;
            }
            substep<SIMPLE, true, XF, FAST>(k, s, eff32, true, ok);
            const int code = failure_code(k, s);
            fail = fail ? fail : code;
        }
        if (STOCK) {
            if (FAST && __builtin_expect(__builtin_amdgcn_ballot_w64(!ok) != 0, 0)) {
                // Some lane of the wave met a sqrt or 1/det argument outside the fast path's window (a tiny velocity or
                // body rate, inf or NaN, a singular R), or came near a failure threshold (a squared norm at its window's
                // upper edge, |p|_inf >= pos_safe32): redo the step for the whole wave from the loaded
                // state with the library's sqrt and division. The state is still in memory (stores come later); the
                // step's inputs are re-read through kernargs_fresh so that none is held in SGPRs across the sub-steps.
                const KArgsC *kaf = kernargs_fresh();
                const QuadK &kf = *(const QuadK *)&kaf->k;
                int ct_loaded;
                load_state<true, BUF>(*(const mg_quadrotor_state *)&kaf->st, n, el, s, ct_loaded);
                derive_lane(s);
                fail = 0;
#pragma unroll 1
                for (int it = 0; it < STOCK_TIMES; ++it) {
                    substep<SIMPLE, true, XF, false>(kf, s, eff32, it == STOCK_TIMES - 1, ok);
                    const int code = failure_code(kf, s);
                    fail = fail ? fail : code;
                }
#ifdef MG_QUAD_PHASE_STAMPS
                fallbacks += 1;
#endif
            }
        } else {
            for (int it = 0; it < k.times; ++it) {                          // quadrotorsim.py:302-304
                if (fail == 0) {  // a failed env freezes at the failing sub-step (reference raises)
                    substep<SIMPLE>(k, s, eff32, it == k.times - 1, ok);
                    fail = failure_code(k, s);
                }
            }
        }
        MG_PHASE_STAMP(2);   // sub-step 10 done
        // The reward / observation constants and the output pointers are used only from here on. Held in
        // SGPRs across the sub-step loop they overflow the scalar file and get spilled to VGPR lanes
        // (125 spills, ~200 v_writelane/v_readlane on the hot path); re-reading them from the kernarg
        // segment (scalar-cache hits, the prologue touched every line) through a pointer the compiler
        // cannot connect to the prologue's loads keeps the loop's SGPR budget for the loop.
        const KArgsC *kae = kernargs_fresh();
        const QuadK &ke = *(const QuadK *)&kae->k;
        const StepIO &ioe = *(const StepIO *)&kae->io;
        // STEP_STOCK_SHADOW: never the velocity task (make_plan: stock needs simple, and simple excludes it), so its
        // arm, tn and the three target entries of the observation are not compiled. STEP_STOCK keeps the test.
        const bool vel_task = !SHADOW && ke.task == MG_QUADROTOR_TASK_VELOCITY_CONTROL;
        const bool hover_task = HOVER || ke.task == MG_QUADROTOR_TASK_HOVERING_CONTROL;
        // _update_state env.py:262-273: the observation's target entries come from min(ct, nt-1) with ct
        // already incremented and not yet cleared by the episode end
        const int tn_step = ct < ke.nt - 1 ? ct : ke.nt - 1;
        double reward = 0.0;
        int done = 1;
        if (fail == 0 && vel_task) {
            // env.py:150-157: body-frame target = Rinv(f32) @ target(f32); reward -0.001 * L1 difference
            float bt[3];
            mv_f32(s.Ri, &ke.vtargets[3 * (ct - 1)], bt);
            double b_v[3];
            mv_f32f64(s.Ri, s.v, b_v);
            const double diff = (fabs((double)bt[0] - b_v[0]) + fabs((double)bt[1] - b_v[1])) + fabs((double)bt[2] - b_v[2]);
            const float energy = ke.dt32 * s.power;
            const double r = (ke.healthy32 < energy) ? -ke.healthy : -(double)energy;
            reward = r + (-0.001 * diff);
            done = 0;
            if (ct == ke.nt) { done = 1; ct = 0; }
        } else if (fail == 0) {
            const double new_pos[3] = {(double)s.p[0] + ke.xoff, (double)s.p[1] + ke.yoff,
                                       (double)(s.p[2] + ke.zoff32)};
            const bool hit = FLAT ? collision_flat(old_pos[2], new_pos[2]) : collision(ke, old_pos, new_pos);   // env.py:145
            // _get_reward env.py:211-246
            const float energy = ke.dt32 * s.power;
            double r = (ke.healthy32 < energy) ? -ke.healthy : -(double)energy;   // -min(energy, healthy)
            double task_reward = hit ? 0.0 : ke.healthy;
            if (hover_task) {
                task_reward -= 1.0 * s.nv + 1.0 * s.nw;
                const float z_move = fabsf(0.0f - s.p[2]);   // pos_0 is the reset position = 0 (env.py:123)
                if (z_move < 0.5f) task_reward += 10;
                else {
                    const float o = 0.5f - z_move;
                    task_reward += (o > -20.0f) ? (double)o : -20.0;
                }
            }
            if (hover_task || ke.healthy32 < energy)
                reward = r + task_reward;     // np.float64 task_reward, or python floats on both sides
            else                              // no_collision: np.float32 + weak python float -> f32 add (env.py:220-221)
                reward = (double)((float)r + (float)task_reward);
            done = 0;
            if (hit) { done = 1; ct = 0; }                                  // env.py:147-149
            if (ct == ke.nt) { done = 1; ct = 0; }                           // env.py:159-161
        } else {
            ct = 0;
        }
        // Reward / done above read the stepped state only, so the observation is computed ONCE, after the
        // optional in-place reset: stepped state for running envs, and — vector-env convention — the first
        // observation of the next episode for the envs that just finished.
        int tn = tn_step;
        if ((STOCK || ke.auto_reset) && done) {
            if (SHADOW) reset_apply(s, rd);
            else reset_apply(s, reset_draw(ke, el, episode));
            episode += 1;
            tn = ct < ke.nt - 1 ? ct : ke.nt - 1;
        }
        // The next step's action (requested at the top of this step) is taken out of flight here, before this
        // step's stores are issued: vmcnt counts loads and stores in one queue, so a wait placed at the top of
        // the next step would also wait for every store below.
        if (t + 1 < n_steps) asm volatile("" : "+v"(a_next.x), "+v"(a_next.y), "+v"(a_next.z), "+v"(a_next.w));
        // The state is final here. Its stores (63 % of the bytes this launch writes) go out before the
        // observation arithmetic so that they drain behind it instead of after it.
        if (t == n_steps - 1 && live) {
            const mg_quadrotor_state &ste = *(const mg_quadrotor_state *)&kae->st;
            store_lane<BUF>(ste, n, e, s, ct);
            if (episode != episode_in) st_soa<BUF, ST_STATE>(ste.episode, 1, n, 0, e, episode);   // rare: only lanes that restarted
        }
        MG_PHASE_STAMP(3);   // state stores issued
        __builtin_amdgcn_sched_barrier(0);   // pure arithmetic would otherwise be hoisted above the stores
        float obs[OBS_DIM + 3];
        observe(ke, s, obs);
        if (vel_task) { obs[16] = ke.vtargets[3 * tn]; obs[17] = ke.vtargets[3 * tn + 1]; obs[18] = ke.vtargets[3 * tn + 2]; }
        store_obs_wave<BUF>(tile, obs, ioe.obs + off * ke.obs_dim, n, e, ke.obs_dim);
        MG_PHASE_STAMP(4);   // obs stores issued
        if (live) {
            if (BUF) {   // one-step form: off == 0
                if (ioe.reward) st_soa<true, ST_SCALAR>(ioe.reward + off, 1, n, 0, e, (float)reward);
                if (ioe.reward64) st_soa<true, ST_SCALAR>(ioe.reward64 + off, 1, n, 0, e, reward);
                st_soa<true, ST_SCALAR>(ioe.done + off, 1, n, 0, e, (uint8_t)done);
                if (ioe.failed) st_soa<true, ST_SCALAR>(ioe.failed + off, 1, n, 0, e, (uint8_t)fail);
            } else {
                if (ioe.reward) st_stream<st_policy<false, ST_SCALAR>()>(&ioe.reward[off + e], (float)reward);
                if (ioe.reward64) st_stream<st_policy<false, ST_SCALAR>()>(&ioe.reward64[off + e], reward);
                st_stream<st_policy<false, ST_SCALAR>()>(&ioe.done[off + e], (uint8_t)done);
                if (ioe.failed) st_stream<st_policy<false, ST_SCALAR>()>(&ioe.failed[off + e], (uint8_t)fail);
            }
        }
    }
#ifdef MG_QUAD_PHASE_STAMPS
    if (SHADOW) {   // lane 0 of each wave, plain vector stores
        const uint32_t wave = (blockIdx.x * BLOCK + threadIdx.x) / mg::WAVE;
        if ((threadIdx.x & (mg::WAVE - 1)) == 0 && wave < PHASE_MAX_WAVES) {
            uint64_t *out = &g_phase_stamps[(size_t)wave * PHASE_SLOTS];
#pragma unroll
            for (int i = 0; i < PHASE_STAMPS; ++i) out[i] = stamp[i];
            out[5] = clock_in;
            out[6] = (uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 4) |                 // HW_ID: wave, SIMD, CU, SE
                     ((uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);        // XCC_ID
            out[7] = (uint64_t)fallbacks << 32;
        }
    }
#endif
}

__global__ __launch_bounds__(BLOCK) void quadrotor_reset_kernel(QuadK k, mg_quadrotor_state st,
                                                                const uint8_t *mask, const double *init_vel,
                                                                const double *init_omega, float *obs_out, int n) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= n) return;
    if (mask != nullptr && mask[e] == 0) return;
    Lane s;
    // _zero_state quadrotorsim.py:20-28, then the injected noise :241-254
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s.p[c] = 0.0f;
        s.v[c] = init_vel ? init_vel[(size_t)c * n + e] : 0.0;
        s.w[c] = init_omega ? init_omega[(size_t)c * n + e] : 0.0;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) s.pw[c] = 0.0f;
#pragma unroll
    for (int c = 0; c < 9; ++c) s.R[c] = (c % 4 == 0) ? 1.0f : 0.0f;
    inv3(s.R, s.Ri, s.Rd);
    s.nv = norm3(s.v);
    s.nw = norm3(s.w);
    s.power = 0.0f;
    const int ct = st.ct[e];
    store_lane(st, n, e, s, ct);   // ct is not cleared by reset() (env.py:116-125)
    if (obs_out != nullptr) {
        float obs[OBS_DIM + 3];
        observe(k, s, obs);
        if (k.task == MG_QUADROTOR_TASK_VELOCITY_CONTROL) {
            const int tn = ct < k.nt - 1 ? ct : k.nt - 1;
            obs[16] = k.vtargets[3 * tn]; obs[17] = k.vtargets[3 * tn + 1]; obs[18] = k.vtargets[3 * tn + 2];
        }
        for (int c = 0; c < k.obs_dim; ++c) obs_out[(size_t)e * k.obs_dim + c] = obs[c];
    }
}

// ---- host: the failure tests of STEP_STOCK_SHADOW folded into its range window (see all_in_range, the step kernel) --
double from_hi_word(uint32_t h) { const uint64_t b = (uint64_t)h << 32; double x; memcpy(&x, &b, sizeof x); return x; }
uint32_t host_hi_word(double x) { uint64_t b; memcpy(&b, &x, sizeof b); return (uint32_t)(b >> 32); }

// The exclusive upper edge (a high word) of the window for x = norm^2 under the test `norm > thr`: the double Y with
// that high word and a zero low word has Y <= thr^2 * (1 - 2^-19), Y <= 2^233 and sqrt(Y) <= thr. A lane with
// hi_word(x) below the edge has x < Y, so sqrt(x) <= sqrt(Y) <= thr: it does not fail. The slack of 2^-19 is there for
// a device sqrt that is not the host's correctly rounded one; the loop, as the search for fail_range_sq32, makes the
// statement about the host's sqrt unconditional. 0: the test cannot be folded. That is a NaN threshold (`>` is false
// for ever, but a window has an edge), a negative one or -0.0 / +0.0 (a zero norm fails or sits on the threshold, and
// zeros are mapped into the window), and one whose edge is below 2^1: then base = edge - LEAN_SPAN would lie below 2^-767,
// the least argument of sqrt_newton. thr = +inf folds: nothing fails, the edge is that of the sqrt window.
uint32_t fold_norm_edge(double thr) {
    if (!(thr > 0.0)) return 0;
    const double y = (thr * thr) * (1.0 - 0x1p-19);          // +inf for a large threshold
    uint32_t e = y < 0x1p+233 ? host_hi_word(y) : SQRT_HI_HI;
    while (e > 0 && sqrt(from_hi_word(e)) > thr) e -= 1;
    return e >= SQRT_LO_HI + LEAN_SPAN ? e : 0;
}

// pos_safe32: the least float32 m >= 0 with !range_safe(m, S), so that the kernel's test is m < pos_safe32 (range_safe is
// monotone in m: both products round monotonically). 0: the range test cannot be folded, for S = NaN (no position
// fails), -inf (a negative range: every position fails), +inf (a range of FLT_MAX's square root and up, or +inf) and
// S < 2^-100, where range_safe's argument needs normal products. Bisection on the bit patterns of the non-negative floats.
float fold_pos_safe(float S) {
    if (!(S >= 0x1p-100f) || S == INFINITY) return 0.0f;
    uint32_t lo = 0, hi = 0x7f800000u;   // range_safe(+0) holds (0 < S), range_safe(+inf) does not
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        float m;
        memcpy(&m, &mid, sizeof m);
        if (range_safe(m, S)) lo = mid; else hi = mid;
    }
    float P;
    memcpy(&P, &hi, sizeof P);
    return P;
}

// Fills the folded constants; false when one of the three tests cannot be folded, or when ct0_32 > 0 does not
// hold (substep<FAST> relies on it). launch_plan then takes STEP_STOCK, which keeps failure_code() per sub-step.
bool fold_lean(QuadK *k) {
    const uint32_t ev = fold_norm_edge(k->fail_velocity), ew = fold_norm_edge(k->fail_w);
    const float P = fold_pos_safe(k->fail_range_sq32);
    if (ev == 0 || ew == 0 || P == 0.0f || !(k->ct0_32 > 0.0f)) return false;
    k->lean_base_v = ev - LEAN_SPAN;
    k->lean_base_w = ew - LEAN_SPAN;
    return true;
}

// the stock X frame of substep<XF>: prop_coord[i] = (sx_i c, sy_i c, 0), signs (+,+), (-,+), (-,-), (+,-), one c > 0
// (then every lm[i] is the same number: the same three products summed in the same order)
bool config_is_xframe(const mg_quadrotor_config *cfg) {
    const float *pc = cfg->prop_coord;
    const float c = pc[1];
    const float sx[4] = {1.0f, -1.0f, -1.0f, 1.0f}, sy[4] = {1.0f, 1.0f, -1.0f, -1.0f};
    if (!(c > 0.0f && c < INFINITY)) return false;
    for (int i = 0; i < 4; ++i)
        if (pc[3 * i] != sx[i] * c || pc[3 * i + 1] != sy[i] * c || pc[3 * i + 2] != 0.0f) return false;
    return true;
}

// What mg_quadrotor_plan holds (caller-owned host memory, see the header): everything a step launch needs
// except the per-call I/O pointers.
struct Plan {
    uint32_t magic;
    int32_t n, device, simple;
    int32_t stock;   // STEP_STOCK applies (see StepForm)
    int32_t xframe;  // ... with the X-frame option (see StepForm)
    int32_t simds;   // SIMDs of the device (0: unknown, STEP_STOCK_SHADOW is not used)
    int32_t lean;    // the failure tests fold into the range window (fold_lean); 0: STEP_STOCK_SHADOW is not used
    QuadK k;
    mg_quadrotor_state st;
};
constexpr uint32_t PLAN_MAGIC = 0x4d475150u;   // "MGQP"
static_assert(sizeof(Plan) <= sizeof(mg_quadrotor_plan), "mg_quadrotor_plan is too small for the folded constants");

int make_plan(Plan *p, const mg_quadrotor_config *cfg, const mg_quadrotor_autoreset *ar, int32_t n,
              const mg_quadrotor_state *state) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(state);
    if (n <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_envs=%d", n);
    if (int rc = check_state(state)) return rc;
    if (int rc = fold_config(cfg, &p->k)) return rc;
    if (ar != nullptr) {
        if (state->episode == nullptr)
            return mg::set_error(MG_ERR_NULL_POINTER, "fused auto-reset needs mg_quadrotor_state.episode");
        QuadK &k = p->k;
        k.auto_reset = 1;
        for (int i = 0; i < 3; ++i) { k.init_v_base[i] = ar->init_velocity[i]; k.init_w_base[i] = ar->init_angular_velocity[i]; }
        k.init_v_noisy = ar->init_velocity_noisy;
        k.init_w_noisy = ar->init_angular_velocity_noisy;
        k.seed = ar->seed;
        k.env_id_base = ar->env_id_base;
    }
    p->magic = PLAN_MAGIC;
    p->n = n;
    p->device = mg::device_of(state->pos);
    p->simple = (config_is_simple(cfg) && cfg->task != MG_QUADROTOR_TASK_VELOCITY_CONTROL) ? 1 : 0;
    // MG_QUAD_GENERIC=1 forces the generic kernel (A/B timing and tests); read per plan, so one process can hold both
    const bool force_generic = getenv("MG_QUAD_GENERIC") != nullptr;
    p->stock = (!force_generic && p->simple && p->k.quality_recip_exact && p->k.times == STOCK_TIMES && p->k.auto_reset) ? 1 : 0;
    p->xframe = (p->stock && config_is_xframe(cfg)) ? 1 : 0;
    // lm > 0 with the X frame: c > 0 does not give it (c * c can underflow to 0 in float32), and substep<XF, FAST> states it
    p->lean = (p->stock && fold_lean(&p->k) && (!p->xframe || p->k.lm[0] > 0.0f)) ? 1 : 0;
    p->simds = 0;
    int cus = 0;
    if (p->device >= 0 && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->device) == hipSuccess)
        p->simds = 4 * cus;
    else
        (void)hipGetLastError();
    p->st = *state;
    return MG_OK;
}

typedef decltype(&quadrotor_step_kernel<false, STEP_GENERIC>) StepKernel;
// the STEP_STOCK_SHADOW kernel for the four host-resolved options (see StepForm)
template <bool... B>
StepKernel pick_shadow() { return quadrotor_step_kernel<true, STEP_STOCK_SHADOW, B...>; }
template <bool... B, typename... Rest>
StepKernel pick_shadow(bool b, Rest... rest) { return b ? pick_shadow<B..., true>(rest...) : pick_shadow<B..., false>(rest...); }

int launch_plan(const Plan *p, int32_t n_steps, const float *action, float *obs, float *reward, double *reward64,
                uint8_t *done, uint8_t *failed, void *stream) {
    MG_REQUIRE_PTR(action);
    MG_REQUIRE_PTR(obs);
    MG_REQUIRE_PTR(done);
    if (n_steps <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_steps=%d", n_steps);
    mg::DeviceGuard guard(p->device);
    StepIO io{action, obs, reward, reward64, done, failed};
    const int n = p->n, grid = (n + BLOCK - 1) / BLOCK;
    const int waves = (n + mg::WAVE - 1) / mg::WAVE;
    // BUF: 32-bit buffer offsets; the [n][16] f32 observation is the largest array a one-step launch touches
    const bool buf = (uint64_t)n * (OBS_DIM * sizeof(float)) < (1ull << 31);
    // FLAT / HOVER: no collision map / the hovering task, both properties of the folded configuration
    const bool flat = p->k.map == nullptr, hover = p->k.task == MG_QUADROTOR_TASK_HOVERING_CONTROL;
    StepKernel kern;
    if (p->stock && p->lean && n_steps == 1 && waves <= p->simds) {
        kern = pick_shadow(p->xframe != 0, buf, flat, hover);
    } else if (p->stock) {
        if (p->xframe) kern = flat ? quadrotor_step_kernel<true, STEP_STOCK, true, false, true> : quadrotor_step_kernel<true, STEP_STOCK, true>;
        else kern = flat ? quadrotor_step_kernel<true, STEP_STOCK, false, false, true> : quadrotor_step_kernel<true, STEP_STOCK>;
    } else if (p->simple) {
        kern = quadrotor_step_kernel<true, STEP_GENERIC>;
    } else {
        kern = quadrotor_step_kernel<false, STEP_GENERIC>;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, p->k, p->st, io, n, n_steps);
    return mg::check_launch("quadrotor_step_kernel");
}

int launch_steps(const mg_quadrotor_config *cfg, int32_t n, int32_t n_steps, const mg_quadrotor_state *state,
                 const float *action, float *obs, float *reward, double *reward64, uint8_t *done,
                 uint8_t *failed, void *stream, const mg_quadrotor_autoreset *ar = nullptr) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(state);
    MG_REQUIRE_PTR(action);
    MG_REQUIRE_PTR(obs);
    MG_REQUIRE_PTR(done);
    Plan p;
    if (int rc = make_plan(&p, cfg, ar, n, state)) return rc;
    return launch_plan(&p, n_steps, action, obs, reward, reward64, done, failed, stream);
}

}  // namespace

extern "C" int mg_quadrotor_default_config(mg_quadrotor_config *c) {
    MG_REQUIRE_PTR(c);
    // metagym/quadrotor/config.json:1-59 and Quadrotor.__init__ defaults env.py:46-114
    *c = mg_quadrotor_config{};
    c->precision = 0.001;
    c->quality = 0.5;
    c->ct0 = 1.538e-5; c->ct1 = -2.5e-4; c->ct2 = 0.0;
    c->mm = 0.010; c->jm = 2.573e-4; c->ra = 0.2010; c->phi = 0.017242179827506;
    c->fail_velocity = 100.0; c->fail_w = 1000.0; c->fail_range = 1000.0;
    c->min_voltage = 0.10; c->max_voltage = 15.0;
    c->dt = 0.01; c->healthy_reward = 1.0; c->z_offset = 5.0;
    c->x_offset = 50; c->y_offset = 50;
    c->nt = 1000;
    c->task = MG_QUADROTOR_TASK_NO_COLLISION;
    c->inertia[0] = 0.0135f; c->inertia[4] = 0.0135f; c->inertia[8] = 0.024f;
    c->drag_m[0] = 0.074f; c->drag_m[4] = 0.074f; c->drag_m[8] = 0.0506f;
    c->drag_f[0] = 0.12f; c->drag_f[4] = 0.12f; c->drag_f[8] = 0.10f;
    const float pc[12] = {0.18f, 0.18f, 0.f, -0.18f, 0.18f, 0.f, -0.18f, -0.18f, 0.f, 0.18f, -0.18f, 0.f};
    for (int i = 0; i < 12; ++i) c->prop_coord[i] = pc[i];
    c->map_d = nullptr; c->map_h = 100; c->map_w = 100;
    return MG_OK;
}

extern "C" int mg_quadrotor_velocity_targets(const mg_quadrotor_config *cfg, int32_t nt, const float *actions_d,
                                             float *targets_d, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(actions_d);
    MG_REQUIRE_PTR(targets_d);
    if (nt <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "nt=%d", nt);
    QuadK k;
    if (int rc = fold_config(cfg, &k, false)) return rc;
    mg::DeviceGuard guard(mg::device_of(targets_d));
    hipLaunchKernelGGL(quadrotor_targets_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, k, nt, actions_d, targets_d);
    return mg::check_launch("quadrotor_targets_kernel");
}

extern "C" int mg_quadrotor_reset(const mg_quadrotor_config *cfg, int32_t n, const mg_quadrotor_state *state,
                                  const uint8_t *mask, const double *init_vel, const double *init_omega,
                                  float *obs, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(state);
    if (n <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_envs=%d", n);
    if (int rc = check_state(state)) return rc;
    QuadK k;
    if (int rc = fold_config(cfg, &k)) return rc;
    const int grid = (n + BLOCK - 1) / BLOCK;
    mg::DeviceGuard guard(mg::device_of(state->pos));
    hipLaunchKernelGGL(quadrotor_reset_kernel, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, k, *state, mask,
                       init_vel, init_omega, obs, n);
    return mg::check_launch("quadrotor_reset_kernel");
}

extern "C" int mg_quadrotor_step(const mg_quadrotor_config *cfg, int32_t n, const mg_quadrotor_state *state,
                                 const float *action, float *obs, float *reward, double *reward64,
                                 uint8_t *done, uint8_t *failed, void *stream) {
    return launch_steps(cfg, n, 1, state, action, obs, reward, reward64, done, failed, stream);
}

extern "C" int mg_quadrotor_step_autoreset(const mg_quadrotor_config *cfg, int32_t n, int32_t n_steps,
                                           const mg_quadrotor_state *state, const mg_quadrotor_autoreset *ar,
                                           const float *action, float *obs, float *reward, double *reward64,
                                           uint8_t *done, uint8_t *failed, void *stream) {
    MG_REQUIRE_PTR(ar);
    return launch_steps(cfg, n, n_steps, state, action, obs, reward, reward64, done, failed, stream, ar);
}

extern "C" int mg_quadrotor_rollout(const mg_quadrotor_config *cfg, int32_t n, int32_t n_steps,
                                    const mg_quadrotor_state *state, const float *action, float *obs,
                                    float *reward, double *reward64, uint8_t *done, uint8_t *failed,
                                    void *stream) {
    return launch_steps(cfg, n, n_steps, state, action, obs, reward, reward64, done, failed, stream);
}

extern "C" int mg_quadrotor_plan_init(mg_quadrotor_plan *plan, const mg_quadrotor_config *cfg,
                                      const mg_quadrotor_autoreset *ar, int32_t n_envs,
                                      const mg_quadrotor_state *state) {
    MG_REQUIRE_PTR(plan);
    Plan *p = reinterpret_cast<Plan *>(plan);
    p->magic = 0;
    return make_plan(p, cfg, ar, n_envs, state);
}

extern "C" int mg_quadrotor_plan_fold(const mg_quadrotor_plan *plan, mg_quadrotor_fold *out) {
    MG_REQUIRE_PTR(plan);
    MG_REQUIRE_PTR(out);
    const Plan *p = reinterpret_cast<const Plan *>(plan);
    if (p->magic != PLAN_MAGIC) return mg::set_error(MG_ERR_BAD_CONFIG, "mg_quadrotor_plan is not initialised");
    *out = mg_quadrotor_fold{};
    out->one_wave_form = !p->stock ? STEP_GENERIC : (p->lean ? STEP_STOCK_SHADOW : STEP_STOCK);
    out->span = LEAN_SPAN;
    out->fail_velocity = p->k.fail_velocity;
    out->fail_w = p->k.fail_w;
    out->fail_range_sq32 = p->k.fail_range_sq32;
    if (p->lean) {
        out->base_v = p->k.lean_base_v;
        out->base_w = p->k.lean_base_w;
        out->edge_v = p->k.lean_base_v + LEAN_SPAN;
        out->edge_w = p->k.lean_base_w + LEAN_SPAN;
        out->pos_safe32 = fold_pos_safe(p->k.fail_range_sq32);
    }
    return MG_OK;
}

#ifdef MG_QUAD_PHASE_STAMPS
// diagnostic builds only: the phase timeline of the last STEP_STOCK_SHADOW launch (see g_phase_stamps)
extern "C" int mg_quadrotor_phase_stamps(uint64_t *host, int32_t max_waves) {
    MG_REQUIRE_PTR(host);
    const int32_t w = max_waves < PHASE_MAX_WAVES ? max_waves : PHASE_MAX_WAVES;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_phase_stamps), (size_t)w * PHASE_SLOTS * sizeof(uint64_t)) != hipSuccess)
        return mg::set_error(MG_ERR_UNSUPPORTED, "hipMemcpyFromSymbol(g_phase_stamps) failed");
    return MG_OK;
}
#endif

extern "C" int mg_quadrotor_plan_step(const mg_quadrotor_plan *plan, int32_t n_steps, const float *action, float *obs,
                                      float *reward, double *reward64, uint8_t *done, uint8_t *failed, void *stream) {
    MG_REQUIRE_PTR(plan);
    const Plan *p = reinterpret_cast<const Plan *>(plan);
    if (p->magic != PLAN_MAGIC) return mg::set_error(MG_ERR_BAD_CONFIG, "mg_quadrotor_plan is not initialised");
    return launch_plan(p, n_steps, action, obs, reward, reward64, done, failed, stream);
}
