// quadrotor_core.h — the quadrotor family's shared core: QuadK and Lane, the sub-step, the observation, the collision test,
// the SoA loads and stores with their cache policies, the auto-reset draw, StepIO and the host-side folding (fold_config,
// config_is_simple, check_state). The one-wave stock step's own pieces (range_safe, collision_flat, fold_lean and what it
// calls, config_is_xframe) are in quadrotor.hip, their only user. quadrotor.hip, quadrotor_tasks.hip and quadrotor_policy.hip include it; each keeps its own copy
// (anonymous namespace) and defines the kernels it launches. The design and the precision notes are in quadrotor.hip.
#pragma once
#include <cstdlib>
#include <cstring>

#include "mg_common.h"
#include "mg_philox.h"

namespace {

#ifndef MG_QUAD_BLOCK
#define MG_QUAD_BLOCK 256     // launch-shape experiments (scripts/quad_variants.py; profiles/r05/quad_launch_shapes.txt): 64 / 128 / 256
#endif
constexpr int BLOCK = MG_QUAD_BLOCK;
constexpr int WAVES_PER_BLOCK = BLOCK / mg::WAVE;
constexpr int OBS_DIM = 16;

// Derived constants: everything the reference computes from python floats before touching an
// array is folded on the host, in the same double arithmetic, then "weak"-cast where NumPy would.
struct QuadK {
    // weak python floats that meet f32 operands first (quadrotorsim.py:136-145,154-156)
    float phi32, phi_over_ra32, inv_jm32, mm32, prec32, ct0_32, ct1_32;
    float quality32, dt32, zoff32, healthy32, fail_range_sq32;
    float lm[4];        // ||prop_coord[i]||, quadrotorsim.py:146
    float pc[12];       // prop_coord
    float iinv[9];      // inverse inertia (f32), quadrotorsim.py:64
    float df[9], dm[9]; // drag matrices
    float cog[3];
    // doubles used against f64 operands
    double prec, half_dt2, half_dt, ct2, quality, inv_quality;
    double min_v, max_v, fail_velocity, fail_w, healthy, xoff, yoff;
    int quality_recip_exact;  // 1/quality is a power of two -> x / quality == x * inv_quality bit-for-bit
    int times, nt, task;
    // fused auto-reset (not in the reference: replaces the user's `if done: env.reset()` round trip)
    int auto_reset;
    float init_v_base[3], init_w_base[3];   // cfg['init_velocity'] / ['init_angular_velocity'] x,y,z (f32 arrays)
    // STEP_STOCK_SHADOW's velocity and body-rate tests folded into its range window (fold_lean): all_in_range's bases for
    // |v|^2 and |w|^2. Zero in a plan that cannot fold. The two words sit where the struct had padding: the layout of the
    // kernel arguments is the same for every form, and the other forms' code depends on it (see KArgs).
    uint32_t lean_base_v;
    double init_v_noisy, init_w_noisy;      // ... ['noisy']
    uint64_t seed, env_id_base;
    const int32_t *map;
    int map_h, map_w;
    const float *vtargets;   // velocity_control target trajectory [nt][3]
    int obs_dim;             // 16, or 19 for velocity_control
    uint32_t lean_base_w;    // see lean_base_v
};

struct Lane {       // one environment, in registers
    float p[3];
    double v[3];
    double w[3];
    float pw[4];
    float R[9];
    double Rd[9];   // R widened to f64, exactly (double)R[i]: inv3 produces it, the next sub-step's R @ a reuses it
    float Ri[9];    // inv(R): _coordination_converter_to_body
    double nv, nw;  // ||v||, ||w|| of the current state (shared by drag and the failure test)
    float power;
};

// ---- f32 / f64 3x3 helpers -------------------------------------------------------------------------
// NumPy's elementwise ops never fuse, but np.matmul / np.linalg.norm run OpenBLAS kernels that do.
// The associations below are the ones that reproduce NumPy bit-for-bit (oracle/quadrotor_oracle.c
// documents the probe); the file is compiled with -ffp-contract=off so only these explicit FMAs fuse.

__device__ __forceinline__ double dot_row_f32f64(const float *row, const double *x) {
    // np.matmul(f32[3,3], f64[3]): matrix widened, dgemv association fma(M2,x2, fma(M0,x0, M1*x1))
    return fma((double)row[2], x[2], fma((double)row[0], x[0], (double)row[1] * x[1]));
}

__device__ __forceinline__ void mv_f32f64(const float *M, const double *x, double *y) {
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = dot_row_f32f64(&M[3 * r], x);
}

__device__ __forceinline__ void mv_f32(const float *M, const float *x, float *y) {
    // np.matmul(f32[3,3], f32[3]) -> OpenBLAS sgemv: rows 0 and 1 (a SIMD pair) are the plain sum without
    // FMA, row 2 (scalar tail) uses the dgemv-style association (oracle/quadrotor_oracle.c documents the probe)
#pragma unroll
    for (int r = 0; r < 2; ++r) y[r] = (M[3 * r] * x[0] + M[3 * r + 1] * x[1]) + M[3 * r + 2] * x[2];
    y[2] = fmaf(M[8], x[2], fmaf(M[6], x[0], M[7] * x[1]));
}

__device__ __forceinline__ void mm_f32(const float *A, const float *B, float *C) {
    // sgemm association: left-to-right FMA chain over k
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            C[3 * r + c] = fmaf(A[3 * r + 2], B[6 + c], fmaf(A[3 * r + 1], B[3 + c], A[3 * r] * B[c]));
}

__device__ __forceinline__ void cross_f32(const float *a, const float *b, float *c) {
    // numpy.cross: every product rounded, then subtracted
    float t0 = a[1] * b[2], t1 = a[2] * b[1];
    float t2 = a[2] * b[0], t3 = a[0] * b[2];
    float t4 = a[0] * b[1], t5 = a[1] * b[0];
    c[0] = t0 - t1;
    c[1] = t2 - t3;
    c[2] = t4 - t5;
}

__device__ __forceinline__ double sumsq3(const double *x) {
    return fma(x[2], x[2], fma(x[1], x[1], x[0] * x[0]));
}
__device__ __forceinline__ double norm3(const double *x) { return sqrt(sumsq3(x)); }

// ---- in-range sqrt and reciprocal (the sub-steps of STEP_STOCK_SHADOW, update_derived_fast) --------------------
// For f64, the compiler expands sqrt(x) and 1.0 / d into a Newton sequence wrapped in range steps. The two functions
// below are those sequences without the range steps. They are used only where the range steps are the identity,
// which is what all_in_range tests.
//   sqrt(x): s = ldexp(x, x < 2^-767 ? 256 : 0); rsq Newton on s; ldexp(result, x < 2^-767 ? -128 : 0); then
//     x itself if class(s) is zero or inf. For 2^-767 <= x < +inf both ldexp are by 0 (exact for the finite x and
//     the finite positive result) and s is neither zero nor inf: the result is the Newton value below. The one
//     addition, rsq clamped to 2^512, is the identity there (rsq(x) <= 2^383.5). It makes x = +0 exact as well:
//     rsq(+0) = +inf becomes 2^512, then s = +0, h = 2^511, r = 0.5, s = +0, h = 1.5 * 2^511 (finite), and the two
//     corrections are fma(+0, h, +0) = +0: the result is +0, which is what the class step returns. Exact zeros are
//     ordinary states (a reset with no velocity noise, a hover at rest on equal rotor voltages keeps w = 0), so they
//     stay on the fast path; everything else below 2^-767 (denormals included) goes to the fallback.
//   1.0 / d: v_div_scale_f64 of d and of 1.0, rcp Newton, v_div_fmas_f64, v_div_fixup_f64. By the ISA's rules
//     V_DIV_SCALE_F64(S0, d, 1.0) returns S0 unscaled with VCC = 0 unless d is 0, d is denormal, 1/d is denormal,
//     exponent(1.0) - exponent(d) >= 768 or exponent(1.0) <= 53; none holds for 2^-500 <= |d| <= 2^500. Then
//     the scaled numerator is 1.0 and the product 1.0 * y is y (exact), V_DIV_FMAS_F64 with VCC = 0 is the plain
//     fma, and V_DIV_FIXUP_F64 (d finite, normal and non-zero, numerator 1.0, exponent difference within +-500)
//     returns the quotient with the sign of d, which it already has.
// The test is one u32 range check on the high words, for all three arguments of an update at once: h - base < LEAN_SPAN,
// one span of 768 exponents for all three, so that one max and one compare serve. For x = |v|^2 or |w|^2 (never negative; a
// NaN may carry the sign bit) the window is x = +0 (mapped to 0) or B <= x < Y, where Y is the double whose high word is the
// plan's edge (low word 0) and B = Y * 2^-768; a set sign bit or an exponent of 2047 (inf, NaN) lands above it. The edge is
// where the failure tests come in (fold_lean): Y <= min(threshold^2 * (1 - 2^-19), 2^233) with sqrt(Y) <= threshold checked
// on the host, so a lane inside the window cannot fail the velocity or the body-rate test at this update: x < Y, sqrt is
// monotone, and sqrt_newton is the library's value here. fold_lean admits only edges of 2^1 and above, so B >= 2^-767, the
// least argument the Newton sequence is good for (stock: B = 2^-755 for |v|^2, 2^-749 for |w|^2). For d the sign is
// masked off and the window is 2^-384 <= |d| < 2^384, inside the +-500 exponents that rcp_newton is good for. With R in f32
// a non-zero det is a sum of multiples of 2^-447 below 2^387; besides det = 0, inf and NaN, only the dets below 2^-384
// or from 2^384 up leave it, which R reaches long after |w| has failed.
constexpr uint32_t LEAN_SPAN = 768u << 20;
constexpr uint32_t SQRT_LO_HI = 256u << 20, SQRT_HI_HI = (1023u + 233u) << 20;   // high words of 2^-767 and 2^233
__device__ __forceinline__ uint32_t hi_word(double x) { return (uint32_t)(__builtin_bit_cast(uint64_t, x) >> 32); }
__device__ __forceinline__ bool all_in_range(uint32_t base_v, uint32_t base_w, double xv, double xw, double d) {
    constexpr uint32_t RCP_BASE = (1023u - 384u) << 20;
    const uint32_t tv = xv == 0.0 ? 0u : hi_word(xv) - base_v, tw = xw == 0.0 ? 0u : hi_word(xw) - base_w;
    const uint32_t td = (hi_word(d) & 0x7fffffffu) - RCP_BASE;
    return max(tv, max(tw, td)) < LEAN_SPAN;
}
__device__ __forceinline__ double sqrt_newton(double x) {
    const double g = fmin(__builtin_amdgcn_rsq(x), 0x1p+512);   // the identity in the window; x = +0: see above
    double s = x * g, h = g * 0.5;
    const double r = fma(-h, s, 0.5);
    s = fma(s, r, s);
    h = fma(h, r, h);
    const double d0 = fma(-s, s, x);
    s = fma(d0, h, s);
    const double d1 = fma(-s, s, x);
    return fma(d1, h, s);
}
__device__ __forceinline__ double rcp_newton(double d) {
    double y = __builtin_amdgcn_rcp(d);
    y = fma(y, fma(-d, y, 1.0), y);
    y = fma(y, fma(-d, y, 1.0), y);
    return fma(fma(-d, y, 1.0), y, y);   // v_div_fmas_f64(1.0 - d * (1.0 * y), y, 1.0 * y)
}
// np.linalg.norm(f32[3])^2 = OpenBLAS sdot(x, x): every product rounded to float32, the three products
// accumulated in double, the sum rounded to float32
__device__ __forceinline__ float sumsq3(const float *x) {
    const float p0 = x[0] * x[0], p1 = x[1] * x[1], p2 = x[2] * x[2];
    return (float)(((double)p0 + (double)p1) + (double)p2);
}

// np.linalg.inv on a float32 matrix (quadrotorsim.py:207): numpy promotes to float64, solves, and
// casts back, i.e. it returns the correctly rounded f32 inverse. Same here: adjugate / det in f64
// (branch-free, ~60 f64 ops, one division), rounded to f32. R drifts away from orthonormal (the
// reference never re-normalises it), so R^T is NOT a substitute.
struct Cof { double c00, c01, c02, det; };
__device__ __forceinline__ Cof inv3_cof(const float *Af, double *A) {   // A: out, the widened input
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = (double)Af[i];
    // a*b - c*d as fma(a, b, -(c*d)): one rounding less per cofactor and one instruction less; this is OUR
    // way of reaching the correctly rounded float32 inverse, not an operation of the reference, so fusing
    // is free as long as oracle and kernel do the same
    Cof c;
    c.c00 = fma(A[4], A[8], -(A[5] * A[7]));
    c.c01 = fma(A[5], A[6], -(A[3] * A[8]));
    c.c02 = fma(A[3], A[7], -(A[4] * A[6]));
    c.det = fma(A[2], c.c02, fma(A[1], c.c01, A[0] * c.c00));
    return c;
}
__device__ __forceinline__ void inv3_scale(const double *A, const Cof &c, double r, float *Ainv) {   // r = 1.0 / det
    Ainv[0] = (float)(c.c00 * r);
    Ainv[3] = (float)(c.c01 * r);
    Ainv[6] = (float)(c.c02 * r);
    Ainv[1] = (float)(fma(A[2], A[7], -(A[1] * A[8])) * r);
    Ainv[4] = (float)(fma(A[0], A[8], -(A[2] * A[6])) * r);
    Ainv[7] = (float)(fma(A[1], A[6], -(A[0] * A[7])) * r);
    Ainv[2] = (float)(fma(A[1], A[5], -(A[2] * A[4])) * r);
    Ainv[5] = (float)(fma(A[2], A[3], -(A[0] * A[5])) * r);
    Ainv[8] = (float)(fma(A[0], A[4], -(A[1] * A[3])) * r);
}
__device__ __forceinline__ void inv3(const float *Af, float *Ainv, double *A) {
    const Cof c = inv3_cof(Af, A);
    inv3_scale(A, c, 1.0 / c.det, Ainv);
}

// Ri, Rd, nv and nw of the lane's current R, v and w (inv3 and the two norms). update_derived_fast: the in-range sequences above, and
// `ok` cleared for a lane whose arguments leave their window. The caller redoes the whole step with the library's sqrt
// and division when any lane of the wave has a cleared flag: one wave-uniform branch per step, which costs the wave about
// 60 % more time when taken. A masked recompute behind a branch after each update bounds that cost, but splits the
// straight-line sub-steps into scheduling regions: it doubled the VGPRs and took back the whole gain (profiles/r09/).
// The two forms are separate functions so that the fast one cannot be called without its plan's window bases.
__device__ __forceinline__ void update_derived(Lane &s) {
    inv3(s.R, s.Ri, s.Rd);
    s.nv = norm3(s.v);
    s.nw = norm3(s.w);
}
__device__ __forceinline__ void update_derived_fast(Lane &s, bool &ok, uint32_t base_v, uint32_t base_w) {
    const Cof c = inv3_cof(s.R, s.Rd);
    const double xv = sumsq3(s.v), xw = sumsq3(s.w);
    const double r = rcp_newton(c.det), nv = sqrt_newton(xv), nw = sqrt_newton(xw);
    ok = ok & all_in_range(base_v, base_w, xv, xw, c.det);
    inv3_scale(s.Rd, c, r, s.Ri);
    s.nv = nv;
    s.nw = nw;
}

// ---- one 1 ms Euler sub-step, quadrotorsim.py:122-210 ------------------------------------------
// eff32[i]: the clamped voltage already rounded to f32 (quadrotorsim.py:130-134 + weak cast).
// SIMPLE = the structure of the stock config.json: diagonal drag / inertia matrices, zero centre of
// gravity offset, CT[2] == 0, propellers in the z = 0 plane. Multiplying by those structural zeros
// only ever adds +-0 to a finite sum, so the SIMPLE path is bit-identical to the general one while
// needing ~40 fewer scalar constants and ~70 fewer VALU ops per sub-step.
// want_power: self.power (:139,:188) is overwritten by every sub-step and read only by the reward
// after the last one (env.py:217), so the four f32 divisions behind it run in the last sub-step only.
// RECIP: the host has established k.quality_recip_exact (stock quality 0.5), so f / quality is the multiply
// by its exact reciprocal with no test in the sub-step.
// XF: the host has established the stock X frame (config_is_xframe): prop_coord[i] = (sx_i c, sy_i c, 0) with signs
// (+,+), (-,+), (-,-), (+,-) and one c > 0, so every lm[i] is the same. IEEE products are sign-symmetric
// (x*(-c) == -(x*c) bit for bit), so the eight products of the four cz collapse to A = w0*c and B = w1*c, and the
// eight torque products to the four T_i*c. The sums are written as the reference's own: w0*pc1 - w1*pc0 is A - B,
// A - (-B) = A + B, (-A) - (-B) = B - A and (-A) - B, never a negated sum (-(A-B) differs from B-A in the sign of
// a zero result).
// FAST: update_derived_fast (STEP_STOCK_SHADOW).
template <bool SIMPLE, bool RECIP = false, bool XF = false, bool FAST = false>
__device__ __forceinline__ void substep(const QuadK &k, Lane &s, const float *eff32, bool want_power, bool &ok) {
    static_assert(!XF || SIMPLE, "the X frame is a SIMPLE configuration");
    float prop_force_z = 0.0f;
    float prop_torque[3] = {0.0f, 0.0f, 0.0f};
    float me[4], pp[4];

    // :147-148 body_velocity = Rinv @ v is identical for all four propellers; only [2] is used
    const double bvz = dot_row_f32f64(&s.Ri[6], s.v);
    double xcz[4];
    if (XF) {
        const double c = (double)k.pc[1];
        const double A = s.w[0] * c, B = s.w[1] * c;
        xcz[0] = A - B;
        xcz[1] = A + B;
        if (!FAST) {
            xcz[2] = B - A;
            xcz[3] = (-A) - B;
        }
    }
    // FAST (make_plan has established ct0_32 > 0 and, for the X frame, lm > 0): propellers 2 and 3 reuse the products
    // m_i = xcz[i] * lm of propellers 0 and 1, v_1 = bvz - m_{i-2}, two v_mul_f64 and two v_add_f64 fewer per sub-step.
    //   B - A is -(A - B) and (-A) - B is -(A + B) bit for bit unless the result is an exact zero (x - x is +0 either way
    //   round, and so are the sums of signed zeros that differ), and a product by lm keeps that: the only difference is
    //   the sign of a zero m. bvz - m then differs from bvz + (-m) only when bvz is -0 as well, and only in the sign of a
    //   zero v_1 (a non-zero or +0 bvz absorbs a zero of either sign). v_1 enters t1 = (double)(ct1 * w_m) * v_1 alone,
    //   so t1 is a zero of either sign (or NaN in both forms, for a non-finite factor). t0 = (ct0 * w_m) * w_m is
    //   +0 or positive for ct0 > 0: the two factors w_m carry the same sign, a product that underflows is +0, and
    //   (ct0 * -0) * -0 is +0 (a NaN w_m gives NaN in both forms). So thrust = t0 + t1 is t0 for a positive t0 and
    //   +0 + (+-0) = +0 otherwise: the same bits in both forms.
    //   The same fact serves prop_force_z: thrust is never -0 (t0 + t1 with t0 >= +0 gives -0 only from -0 + -0), so
    //   0.0 + thrust is thrust and the first propeller's (float)(0.0 + thrust) is T = (float)thrust.
    double m01[2];

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float e32 = eff32[i];
        float phi_w = k.phi32 * s.pw[i];                         // :136
        me[i] = k.phi_over_ra32 * (e32 - phi_w);                 // :137-138
        if (want_power) pp[i] = fabsf(me[i] / k.phi32 * e32);    // :139
        float d_prop_w = k.inv_jm32 * (me[i] - k.mm32);          // :141-142
        float w_m = s.pw[i] + k.prec32 * d_prop_w;               // :144-145
        const float *pc = &k.pc[3 * i];
        // :149-151 (omega x coord)[2] * l_m, f64
        double v_1;
        if (XF && FAST) {
            if (i < 2) m01[i] = xcz[i] * (double)k.lm[0];
            v_1 = i < 2 ? bvz + m01[i] : bvz - m01[i - 2];
        } else {
            double cz = XF ? xcz[i] : s.w[0] * (double)pc[1] - s.w[1] * (double)pc[0];
            v_1 = bvz + cz * (double)(XF ? k.lm[0] : k.lm[i]);
        }
        float t0 = (k.ct0_32 * w_m) * w_m;                       // :154 f32 chain
        double t1 = (double)(k.ct1_32 * w_m) * v_1;              // :155 f32 product, widened
        double thrust = (double)t0 + t1;
        if (!SIMPLE) {
            double sign = v_1 > 0 ? 1.0 : -1.0;                  // :152
            thrust = thrust + ((k.ct2 * v_1) * v_1) * sign;      // :156 f64
        }
        s.pw[i] = w_m;                                           // :158
        const float T = (float)thrust;                           // :160-162 cross(-[0,0,T], coord)
        if (FAST && i == 0) prop_force_z = T;                    // (float)(0.0 + thrust), see above
        else prop_force_z = (float)((double)prop_force_z + thrust);   // :159 f64 add, f32 store
        if (XF) {                                                // T*(+-c) = +-(T*c), the sums as above
            const float Tc = T * k.pc[1];
            prop_torque[0] = (i < 2) ? prop_torque[0] + Tc : prop_torque[0] - Tc;
            prop_torque[1] = (i == 1 || i == 2) ? prop_torque[1] + Tc : prop_torque[1] - Tc;
        } else if (SIMPLE) {
            prop_torque[0] += T * pc[1];
            prop_torque[1] += (-T) * pc[0];
        } else {
            float a[3] = {-0.0f, -0.0f, -T};
            float cr[3];
            cross_f32(a, pc, cr);
            prop_torque[0] += cr[0];
            prop_torque[1] += cr[1];
            prop_torque[2] += cr[2];
        }
    }
    prop_torque[2] += ((-me[0] + me[1]) - me[2]) + me[3];        // :164

    // :166-172 drag: -||v|| * ((Df @ Rinv) @ v), -||w|| * (Dm @ w)
    float DfRi[9];
    double tmp[3], f_drag[3], t_drag[3];
    if (SIMPLE) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) DfRi[3 * r + c] = k.df[4 * r] * s.Ri[3 * r + c];
    } else {
        mm_f32(k.df, s.Ri, DfRi);
    }
    mv_f32f64(DfRi, s.v, tmp);
    const double mnv = -s.nv;
#pragma unroll
    for (int c = 0; c < 3; ++c) f_drag[c] = mnv * tmp[c];
    if (SIMPLE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) tmp[c] = (double)k.dm[4 * c] * s.w[c];
    } else {
        mv_f32f64(k.dm, s.w, tmp);
    }
    const double mnw = -s.nw;
#pragma unroll
    for (int c = 0; c < 3; ++c) t_drag[c] = mnw * tmp[c];

    // :174-178 gravity, f32: Rinv @ [0,0,-9.8] * quality
    float f_grav[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) f_grav[c] = (s.Ri[3 * c + 2] * -9.8f) * k.quality32;

    // :180-184
    double t_all[3], body_acc[3], acc[3];
    float t_grav_neg[3] = {0.0f, 0.0f, 0.0f};
    if (!SIMPLE) {
        float t_grav[3];
        cross_f32(f_grav, k.cog, t_grav);
#pragma unroll
        for (int c = 0; c < 3; ++c) t_grav_neg[c] = -t_grav[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float pf = (c == 2) ? prop_force_z : 0.0f;
        double f_all = (double)(pf + f_grav[c]) + f_drag[c];
        t_all[c] = (double)(SIMPLE ? prop_torque[c] : prop_torque[c] + t_grav_neg[c]) + t_drag[c];
        body_acc[c] = (RECIP || k.quality_recip_exact) ? f_all * k.inv_quality : f_all / k.quality;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)   // mv_f32f64(s.R, body_acc, acc) on the already widened matrix
        acc[r] = fma(s.Rd[3 * r + 2], body_acc[2], fma(s.Rd[3 * r], body_acc[0], s.Rd[3 * r + 1] * body_acc[1]));
    // :185-188
#pragma unroll
    for (int c = 0; c < 3; ++c)
        s.p[c] = (float)((double)s.p[c] + (s.v[c] * k.prec + k.half_dt2 * acc[c]));
#pragma unroll
    for (int c = 0; c < 3; ++c) s.v[c] = s.v[c] + k.prec * acc[c];
    if (want_power) s.power = ((pp[0] + pp[1]) + pp[2]) + pp[3];

    // :190-204 attitude
    double alpha[3], tw[3];
    if (SIMPLE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) alpha[c] = (double)k.iinv[4 * c] * t_all[c];
    } else {
        mv_f32f64(k.iinv, t_all, alpha);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) tw[c] = s.w[c] + k.half_dt * alpha[c];
    // skew(tw) rounded to f32 (:193-199); R += dt * (R @ S) with the sgemm FMA association. The diagonal of S is a
    // structural zero, but its three terms per row are real instructions: without fast-math the compiler keeps
    // x * 0.0f and fmaf(x, 0.0f, y) (signed zeros, inf * 0 = NaN). FAST writes the rows without them, 3 v_mul_f32
    // and 6 v_fma_f32 fewer per sub-step, and the new R is bit-identical wherever the step's result is used:
    //   Finite row (r0, r1, r2). In column j the dropped term is rj * 0 = +-0 with the sign of rj, and column j's sum
    //   rs_j is added to that same rj. Adding +-0 to the partner sum changes nothing unless that sum is an exact
    //   zero, and then only the sign of rs_j can differ. prec32 * (+-0) = +-0, and rj + (+-0) = rj for rj != 0 and
    //   +0 for rj = +0, whichever sign. For rj = -0 the dropped term is -0, and x + (-0) = x for every x, so rs_j
    //   itself is unchanged. A non-finite s entry gives the same inf / NaN with or without the +-0.
    //   Non-finite row. Any non-finite entry of R makes det non-finite in either formulation (every entry of R is a
    //   factor of a term of det; a non-finite factor makes the term inf or NaN, and so the sum), and a finite entry
    //   becomes non-finite only through rs, which then is non-finite in both. all_in_range() clears `ok` and the
    //   wave redoes the whole step with FAST = false, which keeps the full products, as do STEP_STOCK and
    //   STEP_GENERIC. This covers the loaded, unchecked R too: sub-step 1 takes det on the updated R, and a
    //   non-finite loaded entry leaves its updated entry non-finite (r + x, r non-finite) in both forms.
    const float s01 = (float)(-tw[2]), s02 = (float)(tw[1]);
    const float s10 = (float)(tw[2]), s12 = (float)(-tw[0]);
    const float s20 = (float)(-tw[1]), s21 = (float)(tw[0]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float r0 = s.R[3 * r], r1 = s.R[3 * r + 1], r2 = s.R[3 * r + 2];
        const float rs0 = FAST ? fmaf(r2, s20, r1 * s10) : fmaf(r2, s20, fmaf(r1, s10, r0 * 0.0f));
        const float rs1 = FAST ? fmaf(r2, s21, r0 * s01) : fmaf(r2, s21, fmaf(r1, 0.0f, r0 * s01));
        const float rs2 = FAST ? fmaf(r1, s12, r0 * s02) : fmaf(r2, 0.0f, fmaf(r1, s12, r0 * s02));
        s.R[3 * r] = r0 + k.prec32 * rs0;
        s.R[3 * r + 1] = r1 + k.prec32 * rs1;
        s.R[3 * r + 2] = r2 + k.prec32 * rs2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s.w[c] = s.w[c] + k.prec * alpha[c];
    if (FAST) update_derived_fast(s, ok, k.lean_base_v, k.lean_base_w);   // :206-208, and the norms
    else update_derived(s);
}

// quadrotorsim.py:212-221. A select chain, not early returns: all three tests are cheap and the early returns
// compiled into a divergent branch per test. Precedence as in the reference: range, velocity, body rate.
__device__ __forceinline__ int failure_code(const QuadK &k, const Lane &s) {
    const int c3 = (s.nw > k.fail_w) ? 3 : 0;
    const int c2 = (s.nv > k.fail_velocity) ? 2 : c3;
    return (sumsq3(s.p) > k.fail_range_sq32) ? 1 : c2;   // sumsq > S == sqrtf(sumsq) > fail_range32, see fold_config
}

// quadrotorsim.py:260-293, :111-120; env.py:193-209
__device__ __forceinline__ void observe(const QuadK &k, const Lane &s, float *obs) {
    double b_v[3];
    float b_pos[3], imu[3];
    const float g[3] = {0.0f, 0.0f, -9.8f};
    mv_f32f64(s.Ri, s.v, b_v);
    mv_f32(s.Ri, s.p, b_pos);
    mv_f32(s.Ri, g, imu);
    float roll = atan2f(s.R[7], s.R[8]);
    float pitch = atan2f(-s.R[6], sqrtf(s.R[7] * s.R[7] + s.R[8] * s.R[8]));
    float yaw = atan2f(s.R[3], s.R[0]);
    obs[0] = (float)b_v[0]; obs[1] = (float)b_v[1]; obs[2] = (float)b_v[2];
    obs[3] = b_pos[0]; obs[4] = b_pos[1]; obs[5] = b_pos[2];
    obs[6] = 0.0f + imu[0]; obs[7] = 0.0f + imu[1]; obs[8] = 0.0f + imu[2];
    obs[9] = (float)s.w[0]; obs[10] = (float)s.w[1]; obs[11] = (float)s.w[2];
    obs[12] = pitch; obs[13] = roll; obs[14] = yaw;
    obs[15] = s.p[2] + k.zoff32;
}

// python slice normalisation map[a:b] for a dimension of length len
__device__ __forceinline__ void py_slice(long a, long b, long len, long &lo, long &hi) {
    if (a < 0) { a += len; if (a < 0) a = 0; } else if (a > len) a = len;
    if (b < 0) { b += len; if (b < 0) b = 0; } else if (b > len) b = len;
    lo = a; hi = b;
}

// env.py:248-260
__device__ __forceinline__ bool collision(const QuadK &k, const double *op, const double *np_) {
    long mn[3], mx[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double lo = op[i] < np_[i] ? op[i] : np_[i];
        double hi = op[i] > np_[i] ? op[i] : np_[i];
        mn[i] = (long)floor(lo);
        mx[i] = (long)ceil(hi);
    }
    int any = 0;
    if (k.map != nullptr) {
        long y0, y1, x0, x1;
        py_slice(mn[1], mx[1] + 1, k.map_h, y0, y1);
        py_slice(mn[0], mx[0] + 1, k.map_w, x0, x1);
        for (long y = y0; y < y1; ++y)
            for (long x = x0; x < x1; ++x) any |= (k.map[y * k.map_w + x] != 0);
    }
    return (mn[2] < any) || (mx[2] < any);  // heights compared with the *bool* np.any(...)
}

// ---- SoA load / store ----------------------------------------------------------------------------

// Cache policy of a global access = the aux operand of a buffer instruction (gfx950 cache bits: sc0 = 1, nt = 2, sc1 = 16).
// plain and nt leave the written line dirty in the XCD's L2 until the end-of-kernel write-back (nt is a streaming hint in
// a write-back cache, not a write-through); sc1 and sc0 sc1 write through as the store is issued; sc1 nt is both.
constexpr int AUX_PLAIN = 0, AUX_NT = 2, AUX_SC1 = 16, AUX_SC0_SC1 = 17, AUX_SC1_NT = 18;
constexpr bool st_policy_ok(int aux) {
    return aux == AUX_PLAIN || aux == AUX_NT || aux == AUX_SC1 || aux == AUX_SC0_SC1 || aux == AUX_SC1_NT;
}
constexpr bool ld_policy_ok(int aux) { return aux == AUX_PLAIN || aux == AUX_NT; }
// Every output of a step is written once and next read by a later launch (or by the caller), never by this one. Its
// stores fall into three classes, each with a policy of its own, per addressing path: MG_QUAD_ST_* for the buffer path
// (BUF: the one-wave form at the headline size), MG_QUAD_STP_* for the pointer path (st_stream: STEP_STOCK, the generic
// forms, the reset and the task-table kernels, and the one-wave form past 2^31 bytes). -D values are the aux numbers
// above, for A/B builds (scripts/build_variant.sh NAME REV -DMG_QUAD_ST_STATE=16 ...).
//   STATE   pos / vel / omega / propw / rot / ct (store_lane) and the rare episode store: read back by the next launch
//   OBS     the [n][16] observation rows (store_obs_wave)
//   SCALAR  reward, reward64, done, failed: 1 to 8 bytes per env
// MG_QUAD_LD_STATE is the policy of the state loads (plain or nt).
// Measured on MI355X at 65 536 envs (profiles/r12/trace_gaps.jsonl, bench_ab_eager400.jsonl; EXPERIMENTS.md round 12),
// kernel duration plus the gap to the next launch, 4 040 launches each: nt 12.02 / 12.05 us (two runs), plain 12.16,
// sc1 on the state alone 11.75, on state and observation 11.50, on all three classes 11.32, sc0 sc1 11.43, sc1 nt 11.47.
// nt was 1 % better than plain and still left the lines dirty for the end-of-kernel write-back; written through, they
// leave under the arithmetic of the waves that entered later. WRITE_SIZE per launch is the same to 0.05 % (byte-wide
// done / failed included: profiles/r12/pmc_traffic.jsonl). So the buffer path ships sc1 for every class. nt state loads on
// top of it gained nothing (11.32 against 11.70, profiles/r12/timelines.jsonl: load phase 1.08 us either way) and stay plain.
// The pointer path keeps nt: its kernels are the parent's instruction for instruction (profiles/r12/isa_quadrotor.txt).
#ifndef MG_QUAD_ST_STATE
#define MG_QUAD_ST_STATE 16
#endif
#ifndef MG_QUAD_ST_OBS
#define MG_QUAD_ST_OBS 16
#endif
#ifndef MG_QUAD_ST_SCALAR
#define MG_QUAD_ST_SCALAR 16
#endif
#ifndef MG_QUAD_STP_STATE
#define MG_QUAD_STP_STATE 2
#endif
#ifndef MG_QUAD_STP_OBS
#define MG_QUAD_STP_OBS 2
#endif
#ifndef MG_QUAD_STP_SCALAR
#define MG_QUAD_STP_SCALAR 2
#endif
#ifndef MG_QUAD_LD_STATE
#define MG_QUAD_LD_STATE 0
#endif
static_assert(st_policy_ok(MG_QUAD_ST_STATE) && st_policy_ok(MG_QUAD_ST_OBS) && st_policy_ok(MG_QUAD_ST_SCALAR) &&
              st_policy_ok(MG_QUAD_STP_STATE) && st_policy_ok(MG_QUAD_STP_OBS) && st_policy_ok(MG_QUAD_STP_SCALAR),
              "store policy: 0 plain, 2 nt, 16 sc1, 17 sc0 sc1, 18 sc1 nt");
static_assert(ld_policy_ok(MG_QUAD_LD_STATE), "load policy: 0 plain, 2 nt");
enum StoreClass { ST_STATE = 0, ST_OBS = 1, ST_SCALAR = 2 };
template <bool BUF, int CLS> constexpr int st_policy() {
    return CLS == ST_STATE ? (BUF ? MG_QUAD_ST_STATE : MG_QUAD_STP_STATE)
         : CLS == ST_OBS   ? (BUF ? MG_QUAD_ST_OBS : MG_QUAD_STP_OBS)
                           : (BUF ? MG_QUAD_ST_SCALAR : MG_QUAD_STP_SCALAR);
}
typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// BUF: element c of lane e in a [comps][n] array through a buffer resource over the whole array. The lane's byte
// offset e*sizeof(T) is one VGPR per element size and the component's c*n*sizeof(T) a scalar soffset, so an access
// costs no VALU; a flat address is two 64-bit VALU ops per access (v_mad_u64_u32 / v_lshl_add_u64), ~120 per step
// on the prologue's and the epilogue's critical paths. Offsets are 32-bit: launch_plan picks BUF only when the
// largest array of the launch (the [n][16] observation of a one-step launch) spans less than 2^31 bytes. The policy of
// a store is a bit of the instruction (aux), so changing it moves no address arithmetic: sc1 (write-through) by default,
// which measured 0.7 us per step better than nt at 65 536 envs (see MG_QUAD_ST_* above; profiles/r12/trace_gaps.jsonl).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void *base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, (int)bytes, 0x00020000);
}
template <typename T, int AUX = AUX_PLAIN> __device__ __forceinline__ T buf_ld(__amdgpu_buffer_rsrc_t r, uint32_t vo, uint32_t so) {
    static_assert(ld_policy_ok(AUX), "load policy");
    if constexpr (sizeof(T) == 4) return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(r, vo, so, AUX));
    else if constexpr (sizeof(T) == 8) return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(r, vo, so, AUX));
    else return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b128(r, vo, so, AUX));
}
template <int AUX, typename T> __device__ __forceinline__ void buf_st(T v, __amdgpu_buffer_rsrc_t r, uint32_t vo, uint32_t so) {
    static_assert(st_policy_ok(AUX), "store policy");
    if constexpr (sizeof(T) == 1) __builtin_amdgcn_raw_buffer_store_b8(__builtin_bit_cast(uint8_t, v), r, vo, so, AUX);
    else if constexpr (sizeof(T) == 4) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, vo, so, AUX);
    else if constexpr (sizeof(T) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), r, vo, so, AUX);
    else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), r, vo, so, AUX);
}
// The pointer path. plain is a C++ store and nt the nontemporal builtin. sc1 on up to 8 bytes is a relaxed agent-scope
// atomic store (global_store ... sc1). Everything else (the 16-byte observation quads, sc0 sc1, sc1 nt) has no builtin on
// a flat pointer and goes out as a buffer store: the resource starts at the address of the wave's first active lane and
// the lane's offset is its distance from it. Every caller stores one element or one observation quad per lane at
// addresses that rise with the lane, at most 64 bytes apart (one observation row), so a wave spans at most 4 KiB.
template <typename T> struct same_size_uint;
template <> struct same_size_uint<uint8_t> { typedef uint8_t type; };
template <> struct same_size_uint<int> { typedef uint32_t type; };
template <> struct same_size_uint<uint32_t> { typedef uint32_t type; };
template <> struct same_size_uint<float> { typedef uint32_t type; };
template <> struct same_size_uint<double> { typedef uint64_t type; };
template <int AUX, typename T> __device__ __forceinline__ void st_stream(T *p, T v) {
    static_assert(st_policy_ok(AUX), "store policy");
    if constexpr (AUX == AUX_NT) __builtin_nontemporal_store(v, p);
    else if constexpr (AUX == AUX_PLAIN) *p = v;
    else if constexpr (AUX == AUX_SC1 && sizeof(T) <= 8) {
        typedef typename same_size_uint<T>::type U;
        __hip_atomic_store(reinterpret_cast<U *>(p), __builtin_bit_cast(U, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        const uint64_t a = (uint64_t)p;
        // (the builtin returns int: through uint32_t, or a low word with bit 31 set would sign-extend into the high word)
        const uint64_t base = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)) << 32) |
                              (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)a);
        buf_st<AUX>(v, rsrc_of((const void *)base, mg::WAVE * OBS_DIM * 4), (uint32_t)(a - base), 0);
    }
}
template <bool BUF, int AUX = AUX_PLAIN, typename T> __device__ __forceinline__ T ld_soa(const T *a, int comps, int n, int c, int e) {
    if (!BUF) {
        if constexpr (AUX == AUX_NT) return __builtin_nontemporal_load(&a[(size_t)c * n + e]);
        else return a[(size_t)c * n + e];
    }
    return buf_ld<T, AUX>(rsrc_of(a, (uint32_t)comps * (uint32_t)n * sizeof(T)), (uint32_t)e * sizeof(T),
                          (uint32_t)c * (uint32_t)n * sizeof(T));
}
template <bool BUF, int CLS, typename T> __device__ __forceinline__ void st_soa(T *a, int comps, int n, int c, int e, T v) {
    if (!BUF) return st_stream<st_policy<false, CLS>()>(&a[(size_t)c * n + e], v);
    buf_st<st_policy<true, CLS>()>(v, rsrc_of(a, (uint32_t)comps * (uint32_t)n * sizeof(T)), (uint32_t)e * sizeof(T),
                                   (uint32_t)c * (uint32_t)n * sizeof(T));
}

// ROT_FIRST: issue rot, vel and omega ahead of the rest, in the order the derived values below consume them
template <bool ROT_FIRST = false, bool BUF = false>
__device__ __forceinline__ void load_state(const mg_quadrotor_state &st, int n, int e, Lane &s, int &ct) {
    if (ROT_FIRST) {
#pragma unroll
        for (int c = 0; c < 9; ++c) s.R[c] = ld_soa<BUF, MG_QUAD_LD_STATE>(st.rot, 9, n, c, e);
    }
    if (!ROT_FIRST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s.p[c] = ld_soa<BUF, MG_QUAD_LD_STATE>(st.pos, 3, n, c, e);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s.v[c] = ld_soa<BUF, MG_QUAD_LD_STATE>(st.vel, 3, n, c, e);
#pragma unroll
    for (int c = 0; c < 3; ++c) s.w[c] = ld_soa<BUF, MG_QUAD_LD_STATE>(st.omega, 3, n, c, e);
    if (ROT_FIRST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s.p[c] = ld_soa<BUF, MG_QUAD_LD_STATE>(st.pos, 3, n, c, e);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) s.pw[c] = ld_soa<BUF, MG_QUAD_LD_STATE>(st.propw, 4, n, c, e);
    if (!ROT_FIRST) {
#pragma unroll
        for (int c = 0; c < 9; ++c) s.R[c] = ld_soa<BUF, MG_QUAD_LD_STATE>(st.rot, 9, n, c, e);
    }
    ct = ld_soa<BUF, MG_QUAD_LD_STATE>(st.ct, 1, n, 0, e);
}

__device__ __forceinline__ void derive_lane(Lane &s) {   // the library's sqrt and division
    update_derived(s);
    s.power = 0.0f;
}

template <bool BUF = false>
__device__ __forceinline__ void load_lane(const mg_quadrotor_state &st, int n, int e, Lane &s, int &ct) {
    load_state<false, BUF>(st, n, e, s, ct);
    derive_lane(s);
}

template <bool BUF = false>
__device__ __forceinline__ void store_lane(const mg_quadrotor_state &st, int n, int e, const Lane &s, int ct) {
#pragma unroll
    for (int c = 0; c < 3; ++c) st_soa<BUF, ST_STATE>(st.pos, 3, n, c, e, s.p[c]);
#pragma unroll
    for (int c = 0; c < 3; ++c) st_soa<BUF, ST_STATE>(st.vel, 3, n, c, e, s.v[c]);
#pragma unroll
    for (int c = 0; c < 3; ++c) st_soa<BUF, ST_STATE>(st.omega, 3, n, c, e, s.w[c]);
#pragma unroll
    for (int c = 0; c < 4; ++c) st_soa<BUF, ST_STATE>(st.propw, 4, n, c, e, s.pw[c]);
#pragma unroll
    for (int c = 0; c < 9; ++c) st_soa<BUF, ST_STATE>(st.rot, 9, n, c, e, s.R[c]);
    st_soa<BUF, ST_STATE>(st.ct, 1, n, 0, e, ct);
}

// Transpose the wave's 64 x 16 observation rows through LDS and store them as 4 coalesced
// dwordx4 sweeps (each wave instruction writes 1 KiB contiguous). Rows are padded to 17 floats so
// the per-lane row writes hit distinct banks; a partial last wave falls back to per-row stores, which take the OBS
// policy without its nt bit (a row per lane, 16 bytes at a time, is not a stream: under nt they are plain stores).
// BUF (STEP_STOCK_SHADOW, where obs_dim is 16): the same stores through a buffer resource over the step's n rows.
template <bool BUF = false>
__device__ __forceinline__ void store_obs_wave(float *tile, const float *obs, float *out, int n, int e, int obs_dim) {
    if (!BUF && obs_dim != OBS_DIM) {   // velocity_control rows (19 floats) are not 16-byte aligned: plain row stores
        if (e < n)
            for (int c = 0; c < obs_dim; ++c) out[(size_t)e * obs_dim + c] = obs[c];
        return;
    }
    const int lane = threadIdx.x & (mg::WAVE - 1);
    const int wave_base = e - lane;                 // first env of this wave
    const bool full = (wave_base + mg::WAVE) <= n;  // wave-uniform
    if (full) {
#pragma unroll
        for (int c = 0; c < OBS_DIM; ++c) tile[lane * (OBS_DIM + 1) + c] = obs[c];
        __builtin_amdgcn_wave_barrier();
        float4 *dst = reinterpret_cast<float4 *>(out + (size_t)wave_base * OBS_DIM);
        const __amdgpu_buffer_rsrc_t r = rsrc_of(out, (uint32_t)n * (OBS_DIM * 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = j * mg::WAVE + lane;      // float4 index inside the wave's 4 KiB block
            const int row = q >> 2, col = (q & 3) * 4;
            const float *src = &tile[row * (OBS_DIM + 1) + col];
            const v4f v{src[0], src[1], src[2], src[3]};
            if (BUF) buf_st<st_policy<true, ST_OBS>()>(v, r, (uint32_t)(wave_base * OBS_DIM + 4 * lane) * 4 + j * (mg::WAVE * 16), 0);
            else st_stream<st_policy<false, ST_OBS>()>(reinterpret_cast<v4f *>(dst + q), v);
        }
        __builtin_amdgcn_wave_barrier();
    } else if (e < n) {
        float4 *dst = reinterpret_cast<float4 *>(out + (size_t)e * OBS_DIM);
        const __amdgpu_buffer_rsrc_t r = rsrc_of(out, (uint32_t)n * (OBS_DIM * 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const v4f v{obs[4 * j], obs[4 * j + 1], obs[4 * j + 2], obs[4 * j + 3]};
            if (BUF) buf_st<st_policy<true, ST_OBS>() & ~AUX_NT>(v, r, (uint32_t)e * (OBS_DIM * 4) + j * 16, 0);
            else if constexpr ((st_policy<false, ST_OBS>() & ~AUX_NT) == AUX_PLAIN) dst[j] = make_float4(v.x, v.y, v.z, v.w);
            else st_stream<st_policy<false, ST_OBS>() & ~AUX_NT>(reinterpret_cast<v4f *>(dst + j), v);
        }
    }
}

// QuadrotorSim.reset quadrotorsim.py:239-258 with the noise drawn on the device:
// value = base + noisy * U[0,1) * (+1 if U' > 0.5 else -1), per component.
// The draw depends on the seed, the env id and the episode counter only, so it can be made before the
// sub-steps (reset_draw) and applied after them (reset_apply).
struct ResetDraw {
    double v[3], w[3], nv, nw;
};

__device__ __forceinline__ ResetDraw reset_draw(const QuadK &k, int e, uint32_t episode) {
    // two Philox blocks = 8 words: six 32-bit magnitudes and one word of sign bits (the reset sits on the
    // critical path of every wave that holds a finished env, so a third block is worth avoiding).
    // counter = (global env id lo, hi, episode, block), key = seed: the k-th auto-reset of a given env draws
    // the same noise whatever the sharding, the launch shape (steps per launch) or the host did in between,
    // and no launch argument changes from step to step (hipGraph replay; oracle: qo_reset_random)
    uint32_t r[8];
    const uint64_t gid = k.env_id_base + (uint64_t)e;
#pragma unroll
    for (int b = 0; b < 2; ++b)
        philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), episode, (uint32_t)b, (uint32_t)k.seed,
                      (uint32_t)(k.seed >> 32), &r[4 * b]);
    const double inv32 = 1.0 / 4294967296.0;
    ResetDraw d;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double sv = ((r[6] >> c) & 1u) ? 1.0 : -1.0;
        const double sw = ((r[6] >> (3 + c)) & 1u) ? 1.0 : -1.0;
        d.v[c] = (double)k.init_v_base[c] + (k.init_v_noisy * ((double)r[c] * inv32)) * sv;
        d.w[c] = (double)k.init_w_base[c] + (k.init_w_noisy * ((double)r[3 + c] * inv32)) * sw;
    }
    d.nv = norm3(d.v);
    d.nw = norm3(d.w);
    return d;
}

__device__ __forceinline__ void reset_apply(Lane &s, const ResetDraw &d) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s.p[c] = 0.0f;
        s.v[c] = d.v[c];
        s.w[c] = d.w[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) s.pw[c] = 0.0f;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        s.R[c] = (c % 4 == 0) ? 1.0f : 0.0f;
        s.Ri[c] = s.R[c];
        s.Rd[c] = (double)s.R[c];
    }
    s.nv = d.nv;
    s.nw = d.nw;
    s.power = 0.0f;
}

struct StepIO {
    const float *action;   // [T][n][4]
    float *obs;            // [T][n][16]
    float *reward;         // [T][n] or null
    double *reward64;      // [T][n] or null
    uint8_t *done;         // [T][n]
    uint8_t *failed;       // [T][n] or null
};

// ---- host: fold the config into kernel constants ----------------------------------------------

void host_inv3_f32(const float *Af, float *Ainv) {
    // np.linalg.inv(self._inertia) quadrotorsim.py:64: f64 solve, cast back to f32; same formula as the
    // device inv3 and the oracle's qo_inv3_f32 (explicit FMAs)
    double A[9];
    for (int i = 0; i < 9; ++i) A[i] = (double)Af[i];
    const double c00 = fma(A[4], A[8], -(A[5] * A[7])), c01 = fma(A[5], A[6], -(A[3] * A[8])),
                 c02 = fma(A[3], A[7], -(A[4] * A[6]));
    const double det = fma(A[2], c02, fma(A[1], c01, A[0] * c00));
    const double r = 1.0 / det;
    Ainv[0] = (float)(c00 * r); Ainv[3] = (float)(c01 * r); Ainv[6] = (float)(c02 * r);
    Ainv[1] = (float)(fma(A[2], A[7], -(A[1] * A[8])) * r);
    Ainv[4] = (float)(fma(A[0], A[8], -(A[2] * A[6])) * r);
    Ainv[7] = (float)(fma(A[1], A[6], -(A[0] * A[7])) * r);
    Ainv[2] = (float)(fma(A[1], A[5], -(A[2] * A[4])) * r);
    Ainv[5] = (float)(fma(A[2], A[3], -(A[0] * A[5])) * r);
    Ainv[8] = (float)(fma(A[0], A[4], -(A[1] * A[3])) * r);
}

int fold_config(const mg_quadrotor_config *c, QuadK *k, bool need_targets = true) {
    if (!(c->precision >= 1e-8) || c->precision > c->dt)   // quadrotorsim.py:299-300
        return mg::set_error(MG_ERR_BAD_CONFIG, "precision %g must be in [1e-8, dt=%g]", c->precision, c->dt);
    if (c->task != MG_QUADROTOR_TASK_NO_COLLISION && c->task != MG_QUADROTOR_TASK_HOVERING_CONTROL &&
        c->task != MG_QUADROTOR_TASK_VELOCITY_CONTROL)
        return mg::set_error(MG_ERR_UNSUPPORTED, "quadrotor task %d is not implemented", c->task);
    if (c->task == MG_QUADROTOR_TASK_VELOCITY_CONTROL && need_targets && c->velocity_targets_d == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "velocity_control needs cfg->velocity_targets_d");
    if (c->map_d != nullptr && (c->map_h <= 0 || c->map_w <= 0))
        return mg::set_error(MG_ERR_BAD_SIZE, "map shape %d x %d", c->map_h, c->map_w);
    k->phi32 = (float)c->phi;
    k->phi_over_ra32 = (float)(c->phi / c->ra);
    k->inv_jm32 = (float)(1.0 / c->jm);
    k->mm32 = (float)c->mm;
    k->prec32 = (float)c->precision;
    k->ct0_32 = (float)c->ct0;
    k->ct1_32 = (float)c->ct1;
    k->quality32 = (float)c->quality;
    k->dt32 = (float)c->dt;
    k->zoff32 = (float)c->z_offset;
    k->healthy32 = (float)c->healthy_reward;
    {
        // np.linalg.norm(pos) > fail_range, both f32 (quadrotorsim.py:213). sqrtf is monotone and
        // correctly rounded, so  sqrtf(s) > T  <=>  s > S  with S = max{ x : sqrtf(x) <= T }.
        // The search cannot reach two ends: T < 0 (every sum fails; sqrtf(0) > T holds for ever) and T = +inf
        // (nothing fails; nextafterf(inf, inf) is inf). T = -0.0 gives S = 0 and NaN gives S = NaN, as they should.
        const float T = (float)c->fail_range;
        float S;
        if (T < 0.0f) {
            S = -INFINITY;
        } else if (T == INFINITY) {
            S = INFINITY;
        } else {
            S = T * T;
            while (sqrtf(S) > T) S = nextafterf(S, 0.0f);
            while (sqrtf(nextafterf(S, INFINITY)) <= T) S = nextafterf(S, INFINITY);
        }
        k->fail_range_sq32 = S;
    }
    for (int i = 0; i < 4; ++i) {
        const float *p = &c->prop_coord[3 * i];
        const float p0 = p[0] * p[0], p1 = p[1] * p[1], p2 = p[2] * p[2];      // sdot: f32 products, double sum
        k->lm[i] = sqrtf((float)(((double)p0 + (double)p1) + (double)p2));
    }
    for (int i = 0; i < 12; ++i) k->pc[i] = c->prop_coord[i];
    host_inv3_f32(c->inertia, k->iinv);
    for (int i = 0; i < 9; ++i) { k->df[i] = c->drag_f[i]; k->dm[i] = c->drag_m[i]; }
    for (int i = 0; i < 3; ++i) k->cog[i] = c->gravity_center[i];
    k->prec = c->precision;
    k->half_dt2 = 0.5 * c->precision * c->precision;   // python: 0.5 * p * p, left to right
    k->half_dt = 0.5 * c->precision;
    k->ct2 = c->ct2;
    k->quality = c->quality;
    k->inv_quality = 1.0 / c->quality;
    int ex = 0;
    (void)frexp(c->quality, &ex);
    k->quality_recip_exact = (frexp(c->quality, &ex) == 0.5) ? 1 : 0;   // power of two
    k->min_v = c->min_voltage;
    k->max_v = c->max_voltage;
    k->fail_velocity = c->fail_velocity;
    k->fail_w = c->fail_w;
    k->healthy = c->healthy_reward;
    k->xoff = (double)c->x_offset;
    k->yoff = (double)c->y_offset;
    k->times = (int)(c->dt / c->precision);            // quadrotorsim.py:302
    k->nt = c->nt;
    k->task = c->task;
    k->map = c->map_d;
    k->map_h = c->map_h;
    k->map_w = c->map_w;
    k->vtargets = c->velocity_targets_d;
    k->obs_dim = c->task == MG_QUADROTOR_TASK_VELOCITY_CONTROL ? 19 : 16;
    k->auto_reset = 0;
    for (int i = 0; i < 3; ++i) { k->init_v_base[i] = 0.0f; k->init_w_base[i] = 0.0f; }
    k->init_v_noisy = k->init_w_noisy = 0.0;
    k->seed = k->env_id_base = 0;
    k->lean_base_v = k->lean_base_w = 0;
    return MG_OK;
}

// structure test for the SIMPLE kernel specialisation (see substep<>)
bool config_is_simple(const mg_quadrotor_config *c) {
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 3; ++col)
            if (r != col && (c->drag_f[3 * r + col] != 0.0f || c->drag_m[3 * r + col] != 0.0f ||
                             c->inertia[3 * r + col] != 0.0f))
                return false;
    for (int i = 0; i < 3; ++i)
        if (c->gravity_center[i] != 0.0f) return false;
    for (int i = 0; i < 4; ++i)
        if (c->prop_coord[3 * i + 2] != 0.0f) return false;
    return c->ct2 == 0.0;
}

int check_state(const mg_quadrotor_state *s) {
    if (!s->pos || !s->vel || !s->omega || !s->propw || !s->rot || !s->ct)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_quadrotor_state has a NULL array");
    return MG_OK;
}

}  // namespace
