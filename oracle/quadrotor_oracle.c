/*
 * oracle/quadrotor_oracle.c — CPU restatement of the reference Quadrotor hot path.
 *
 * TEST INFRASTRUCTURE. This file is the *checker*, never the product: only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load the library built from it.
 * metagym_amd/ never imports, links or falls back to it.
 *
 * What it restates (reference paths relative to /root/reference/metagym/quadrotor):
 *   qo_substep()  <- QuadrotorSim._run_internal      quadrotorsim.py:122-210
 *   qo_failed()   <- QuadrotorSim._check_failure     quadrotorsim.py:212-221
 *   qo_sim_step() <- QuadrotorSim.step               quadrotorsim.py:295-304
 *   qo_observe()  <- get_sensor/get_state/_get_pitch_roll_yaw + _convert_state_to_ndarray
 *                                                    quadrotorsim.py:111-120,260-293; env.py:193-209
 *   qo_env_step() <- Quadrotor.step (hovering_control / no_collision)   env.py:127-165
 *                    with _check_collision env.py:248-260 and _get_reward env.py:211-246
 *
 * Pinning: tests/test_oracle_quadrotor.py checks this file against tests/golden/quadrotor_*.npz,
 * which oracle/gen_golden.py produced by running the unmodified reference in the build container
 * (python 3.10, numpy 2.2.6).
 *
 * Precision choreography. The reference mixes float32 arrays with python floats and float64
 * arrays; under NumPy-2 promotion (NEP 50) a python float is "weak" (adopts the other operand's
 * dtype) while numpy scalars/arrays are strong. Every expression below is annotated with the dtype
 * NumPy evaluates it in. State dtypes after reset(): position f32, velocity f64, body rate f64,
 * propeller speed f32, rotation matrix f32 (quadrotorsim.py:20-28,239-258).
 * Compile with -ffp-contract=off: NumPy's elementwise ops never fuse a*b+c; the FMAs that the
 * BLAS-backed ops do use are written out explicitly (see the helpers below).
 * What is not restated bit-for-bit: libm's atan2f (three observation angles, <= 1 ulp). Everything
 * else — the simulator STATE (pos, vel, omega, propw, R), power, reward, done, the other 13
 * observation entries and the velocity_control target trajectory — is bit-identical to the reference
 * over the golden rollouts and over 300 random simulator configs (oracle/fuzz_vs_reference.py).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "quadrotor_oracle.h"

/* ---- small helpers ---------------------------------------------------------------------------
 * NumPy's elementwise ops never fuse a*b+c, but np.matmul / np.linalg.norm go through OpenBLAS,
 * whose x86-64 kernels do. The association used below for each BLAS-backed op is the one that
 * reproduced NumPy 2.2.6 + its bundled OpenBLAS bit-for-bit on 1000/1000 random inputs in the
 * build container (probe recorded in DESIGN.md §Oracle): sgemm 3x3@3x3 and dnrm via ddot are
 * left-to-right FMA chains; dgemv on a widened f32 matrix is fma(M2,x2, fma(M0,x0, M1*x1)).
 * sgemv 3x3@3 (OpenBLAS 0.3.29 Haswell kernel) treats the rows differently: rows 0 and 1 (a SIMD
 * pair) are the plain (M0*x0 + M1*x1) + M2*x2 without FMA, row 2 (scalar tail) is
 * fmaf(M2,x2, fmaf(M0,x0, M1*x1)) — 2000/2000 per row. np.linalg.norm of a float32 vector is
 * sqrt(x.dot(x)) with OpenBLAS sdot, which rounds each product to float32 and accumulates the
 * products in DOUBLE before rounding the sum to float32 (5000/5000). Both were found by
 * oracle/fuzz_vs_reference.py (random propeller geometry makes the arm length l_m sensitive to it;
 * the stock +-0.18 arms are not). All of this is at the 1-ulp level. */

static void mat3_vec_f32f64(const float *M, const double *x, double *y) {
    /* np.matmul(f32[3,3], f64[3]) -> f64: M is widened, then dgemv */
    for (int r = 0; r < 3; ++r)
        y[r] = fma((double)M[3 * r + 2], x[2], fma((double)M[3 * r + 0], x[0], (double)M[3 * r + 1] * x[1]));
}

static void mat3_vec_f32(const float *M, const float *x, float *y) {
    /* np.matmul(f32[3,3], f32[3]) -> sgemv: rows 0, 1 plain; row 2 with the dgemv-style FMA association */
    for (int r = 0; r < 2; ++r)
        y[r] = (M[3 * r + 0] * x[0] + M[3 * r + 1] * x[1]) + M[3 * r + 2] * x[2];
    y[2] = fmaf(M[8], x[2], fmaf(M[6], x[0], M[7] * x[1]));
}

static void mat3_mul_f32(const float *A, const float *B, float *C) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            C[3 * r + c] = fmaf(A[3 * r + 2], B[6 + c], fmaf(A[3 * r + 1], B[3 + c], A[3 * r + 0] * B[0 + c]));
}

static void cross_f32(const float *a, const float *b, float *c) {
    /* numpy.cross for 3-vectors: each product rounded, then subtracted */
    float t0 = a[1] * b[2], t1 = a[2] * b[1];
    float t2 = a[2] * b[0], t3 = a[0] * b[2];
    float t4 = a[0] * b[1], t5 = a[1] * b[0];
    c[0] = t0 - t1;
    c[1] = t2 - t3;
    c[2] = t4 - t5;
}

static double norm3_f64(const double *x) { return sqrt(fma(x[2], x[2], fma(x[1], x[1], x[0] * x[0]))); }
static float norm3_f32(const float *x) {
    /* np.linalg.norm(f32[3]) = sqrt(sdot(x, x)): float32 products summed in double, sum rounded to float32 */
    const float p0 = x[0] * x[0], p1 = x[1] * x[1], p2 = x[2] * x[2];
    return sqrtf((float)(((double)p0 + (double)p1) + (double)p2));
}

/* 3x3 inverse of a float32 matrix (np.linalg.inv, quadrotorsim.py:207).
 * numpy.linalg.inv does NOT run LAPACK in float32: linalg._commonType promotes float32 input to
 * float64, calls dgesv, and casts the result back to float32. The f64 result carries ~1e-16 of
 * error, so what reaches the caller is the correctly rounded float32 inverse (up to rare
 * double-rounding ties). Restated as the closed form adjugate/det evaluated in float64 and
 * rounded to float32: bit-identical to the reference on every sub-step of every golden rollout
 * (tests/test_oracle_quadrotor.py). */
void qo_inv3_f32(const float *Af, float *Ainv) {
    double A[9];
    for (int i = 0; i < 9; ++i) A[i] = (double)Af[i];
    /* a*b - c*d as fma(a, b, -(c*d)): one rounding less per cofactor and one instruction less; this is OUR
     * way of reaching the correctly rounded float32 inverse, not an operation of the reference, so fusing
     * is free as long as oracle and kernel do the same */
    const double c00 = fma(A[4], A[8], -(A[5] * A[7]));
    const double c01 = fma(A[5], A[6], -(A[3] * A[8]));
    const double c02 = fma(A[3], A[7], -(A[4] * A[6]));
    const double det = fma(A[2], c02, fma(A[1], c01, A[0] * c00));
    const double r = 1.0 / det;
    Ainv[0] = (float)(c00 * r);
    Ainv[3] = (float)(c01 * r);
    Ainv[6] = (float)(c02 * r);
    Ainv[1] = (float)(fma(A[2], A[7], -(A[1] * A[8])) * r);
    Ainv[4] = (float)(fma(A[0], A[8], -(A[2] * A[6])) * r);
    Ainv[7] = (float)(fma(A[1], A[6], -(A[0] * A[7])) * r);
    Ainv[2] = (float)(fma(A[1], A[5], -(A[2] * A[4])) * r);
    Ainv[5] = (float)(fma(A[2], A[3], -(A[0] * A[5])) * r);
    Ainv[8] = (float)(fma(A[0], A[4], -(A[1] * A[3])) * r);
}

/* ---- constants -------------------------------------------------------------------------- */

void qo_default_consts(qo_consts *c) {
    /* metagym/quadrotor/config.json:1-59 as parsed by _parse_cfg quadrotorsim.py:50-109 */
    memset(c, 0, sizeof(*c));
    c->precision = 0.001;
    c->quality = 0.5;
    float inertia[9] = {0.0135f, 0, 0, 0, 0.0135f, 0, 0, 0, 0.024f};
    qo_inv3_f32(inertia, c->inertia_inv);
    c->drag_m[0] = 0.074f; c->drag_m[4] = 0.074f; c->drag_m[8] = 0.0506f;
    c->drag_f[0] = 0.12f;  c->drag_f[4] = 0.12f;  c->drag_f[8] = 0.10f;
    c->ct0 = 1.538e-5; c->ct1 = -2.5e-4; c->ct2 = 0.0;
    c->mm = 0.010; c->jm = 2.573e-4; c->ra = 0.2010; c->phi = 0.017242179827506;
    const float pc[12] = {0.18f, 0.18f, 0, -0.18f, 0.18f, 0, -0.18f, -0.18f, 0, 0.18f, -0.18f, 0};
    memcpy(c->prop_coord, pc, sizeof(pc));
    c->fail_velocity = 100.0; c->fail_w = 1000.0; c->fail_range = 1000.0;
    c->min_voltage = 0.10; c->max_voltage = 15.0;
    c->dt = 0.01; c->nt = 1000; c->healthy_reward = 1.0;
    c->x_offset = 50; c->y_offset = 50; c->z_offset = 5.0;   /* env.py:104-114 default 100x100 map */
    c->map = 0; c->map_h = 100; c->map_w = 100;
    c->task = QO_TASK_HOVERING;
    c->velocity_targets = 0;
}

void qo_zero_state(qo_state *s) {
    /* _zero_state quadrotorsim.py:20-28 */
    memset(s, 0, sizeof(*s));
    s->R[0] = s->R[4] = s->R[8] = 1.0f;
    s->Rinv[0] = s->Rinv[4] = s->Rinv[8] = 1.0f;
}

void qo_refresh_inverse(qo_state *s) { qo_inv3_f32(s->R, s->Rinv); }

/* ---- one 1 ms sub-step: quadrotorsim.py:122-210 ------------------------------------------ */

int qo_failed(const qo_consts *c, const qo_state *s) {
    /* quadrotorsim.py:212-221; norms in the array's own dtype */
    /* np.float32 > python float: the python float is weak, the comparison runs in f32 */
    if (norm3_f32(s->pos) > (float)c->fail_range) return 1;
    if (norm3_f64(s->vel) > c->fail_velocity) return 2;
    if (norm3_f64(s->omega) > c->fail_w) return 3;
    return 0;
}

/* NumPy-pin switch (test infrastructure of test infrastructure). Everything in this file is the reference as NumPy >= 2
 * (NEP 50) evaluates it — the only way it runs in the build container. The reference's own pin is numpy==1.22
 * (requirements.txt:4), whose value-based casting differs in ONE kind of expression: a python float combined with a
 * float32 SCALAR (an element read out of an array, np.sum's result) gives float64 there and float32 here; python float
 * with a float32 ARRAY is float32 under both. With the switch on, those scalar mixes are evaluated in float64, hand-derived
 * line by line from quadrotorsim.py:136-156 and env.py:217,237-241 (the motor chain phi_w, me, power, d_prop_w, w_m and the
 * thrust polynomial; dt * power, hovering_range - z_move). tests/test_oracle_quadrotor.py bounds the gap between the two
 * readings over every golden rollout (north_star tolerance 1e-5). Not thread-safe; never set outside that test. */
static int qo_legacy_promotion = 0;
void qo_set_legacy_promotion(int on) { qo_legacy_promotion = on; }

void qo_substep(const qo_consts *c, qo_state *s, const double act[4]) {
    float prop_force_z = 0.0f;               /* prop_force[0], [1] stay 0 (:124,159) */
    float prop_torque[3] = {0, 0, 0};
    float prop_powers[4];
    float me[4];

    const float phi32 = (float)c->phi;                    /* python float -> weak -> f32 */
    const float phi_over_ra32 = (float)(c->phi / c->ra);  /* python double division, then weak */
    const float inv_jm32 = (float)(1.0 / c->jm);
    const float mm32 = (float)c->mm;
    const float prec32 = (float)c->precision;
    const float ct0_32 = (float)c->ct0, ct1_32 = (float)c->ct1;

    for (int i = 0; i < 4; ++i) {
        double eff_act = act[i];                                           /* :130-134 */
        if (eff_act > c->max_voltage) eff_act = c->max_voltage;
        else if (eff_act < c->min_voltage) eff_act = c->min_voltage;
        const float eff32 = (float)eff_act;

        float w_m;
        double w_m64 = 0.0;
        if (!qo_legacy_promotion) {
            float phi_w = phi32 * s->propw[i];                             /* :136 f32 */
            me[i] = phi_over_ra32 * (eff32 - phi_w);                       /* :137-138 f32 */
            prop_powers[i] = fabsf(me[i] / phi32 * eff32);                 /* :139 f32 */
            float d_prop_w = inv_jm32 * (me[i] - mm32);                    /* :141-142 f32 */
            w_m = s->propw[i] + prec32 * d_prop_w;                         /* :144-145 f32 */
        } else {        /* numpy 1.22: python float (op) float32 scalar -> float64; the f32 arrays round on store */
            const double phi_w = c->phi * (double)s->propw[i];
            me[i] = (float)(c->phi / c->ra * (eff_act - phi_w));
            prop_powers[i] = (float)fabs((double)me[i] / c->phi * eff_act);
            const double d_prop_w = 1.0 / c->jm * ((double)me[i] - c->mm);
            w_m64 = (double)s->propw[i] + c->precision * d_prop_w;
            w_m = (float)w_m64;                                            /* what :158 stores */
        }
        float l_m = norm3_f32(&c->prop_coord[3 * i]);                      /* :146 f32 */

        double body_velocity[3];                                           /* :147-148 f64 */
        mat3_vec_f32f64(s->Rinv, s->vel, body_velocity);
        /* :149-150 np.cross(f64 omega, f32 coord)[2] * l_m -> f64 */
        const float *pc = &c->prop_coord[3 * i];
        double cz = s->omega[0] * (double)pc[1] - s->omega[1] * (double)pc[0];
        double bw_to_v_z = cz * (double)l_m;
        double v_1 = body_velocity[2] + bw_to_v_z;                         /* :151 */
        double sign = v_1 > 0 ? 1.0 : -1.0;                                /* :152 */

        /* :154-156: ct0*w*w is an f32 chain, ct1*w is f32 then widened, ct2 term all f64 */
        float t0 = (ct0_32 * w_m) * w_m;
        double t1 = (double)(ct1_32 * w_m) * v_1;
        double t2 = ((c->ct2 * v_1) * v_1) * sign;
        double thrust = ((double)t0 + t1) + t2;
        if (qo_legacy_promotion)                                          /* w_m is a float64 scalar there: all three terms f64 */
            thrust = ((c->ct0 * w_m64) * w_m64 + (c->ct1 * w_m64) * v_1) + t2;

        s->propw[i] = w_m;                                                 /* :158 */
        prop_force_z = (float)((double)prop_force_z + thrust);             /* :159 f64 add, f32 store */
        float a[3] = {-0.0f, -0.0f, -(float)thrust};                       /* :160-162 */
        float cr[3];
        cross_f32(a, pc, cr);
        prop_torque[0] += cr[0]; prop_torque[1] += cr[1]; prop_torque[2] += cr[2];
    }
    prop_torque[2] += ((-me[0] + me[1]) - me[2]) + me[3];                  /* :164 */

    /* :166-170 f_drag = -||v|| * ((Df @ Rinv) @ v): f32 3x3 product, then f64 */
    float DfRinv[9];
    mat3_mul_f32(c->drag_f, s->Rinv, DfRinv);
    double tmpv[3], f_drag[3], t_drag[3];
    mat3_vec_f32f64(DfRinv, s->vel, tmpv);
    double nv = -norm3_f64(s->vel);
    for (int k = 0; k < 3; ++k) f_drag[k] = nv * tmpv[k];
    /* :171-172 */
    mat3_vec_f32f64(c->drag_m, s->omega, tmpv);
    double nw = -norm3_f64(s->omega);
    for (int k = 0; k < 3; ++k) t_drag[k] = nw * tmpv[k];

    /* :174-178 gravity in the body frame, f32 */
    const float gravity_acc[3] = {0.0f, 0.0f, -9.8f};
    float f_grav[3], t_grav[3];
    mat3_vec_f32(s->Rinv, gravity_acc, f_grav);
    for (int k = 0; k < 3; ++k) f_grav[k] = f_grav[k] * (float)c->quality;
    cross_f32(f_grav, c->gravity_center, t_grav);
    for (int k = 0; k < 3; ++k) t_grav[k] = -t_grav[k];

    /* :180-181 (f32 + f32) + f64 */
    const float prop_force[3] = {0.0f, 0.0f, prop_force_z};
    double f_all[3], t_all[3], body_acc[3], acc[3];
    for (int k = 0; k < 3; ++k) {
        f_all[k] = (double)(prop_force[k] + f_grav[k]) + f_drag[k];
        t_all[k] = (double)(prop_torque[k] + t_grav[k]) + t_drag[k];
        body_acc[k] = f_all[k] / c->quality;                               /* :183 */
    }
    mat3_vec_f32f64(s->R, body_acc, acc);                                  /* :184 */
    const double half_dt2 = 0.5 * c->precision * c->precision;             /* python doubles */
    for (int k = 0; k < 3; ++k) {
        /* :185-186 f64 add, rounded into the f32 position array; uses the OLD velocity */
        s->pos[k] = (float)((double)s->pos[k] + (s->vel[k] * c->precision + half_dt2 * acc[k]));
    }
    for (int k = 0; k < 3; ++k) s->vel[k] = s->vel[k] + c->precision * acc[k];   /* :187 */
    /* :188 np.sum over 4 f32: add.reduce = a0 + (a1 + a2 + a3 accumulated left to right) */
    s->power = ((prop_powers[0] + prop_powers[1]) + prop_powers[2]) + prop_powers[3];

    double alpha[3], tmp_w[3];
    mat3_vec_f32f64(c->inertia_inv, t_all, alpha);                         /* :190-191 */
    const double half_dt = 0.5 * c->precision;
    for (int k = 0; k < 3; ++k) tmp_w[k] = s->omega[k] + half_dt * alpha[k];
    float S[9] = {0};                                                      /* :193-199 f32 */
    S[1] = (float)(-tmp_w[2]); S[2] = (float)(tmp_w[1]);
    S[3] = (float)(tmp_w[2]);  S[5] = (float)(-tmp_w[0]);
    S[6] = (float)(-tmp_w[1]); S[7] = (float)(tmp_w[0]);
    float RS[9];
    mat3_mul_f32(s->R, S, RS);                                             /* :201-202 f32 */
    for (int k = 0; k < 9; ++k) s->R[k] = s->R[k] + prec32 * RS[k];
    for (int k = 0; k < 3; ++k) s->omega[k] = s->omega[k] + c->precision * alpha[k];  /* :203-204 */
    qo_inv3_f32(s->R, s->Rinv);                                            /* :206-208 */
}

/* ---- the same sub-step while the simulator is still in its pre-reset, ALL-float32 state -----------
 * QuadrotorSim._zero_state (quadrotorsim.py:20-28) makes every array float32; only reset() turns
 * velocity and body rate into float64. define_velocity_control_task (quadrotorsim.py:306-319) rolls
 * the target trajectory from that state at Quadrotor.__init__ time (env.py:99-102), so there every
 * expression of _run_internal is float32 (python floats are weak). vel32 / omega32 carry the state. */
typedef struct { float pos[3], vel[3], omega[3], propw[4], R[9], Rinv[9]; } qo_state32;

static void mat3_vec_f32_plain(const float *M, const float *x, float *y) { mat3_vec_f32(M, x, y); }

static void qo_substep_f32state(const qo_consts *c, qo_state32 *s, const float act[4]) {
    float prop_force_z = 0.0f, prop_torque[3] = {0, 0, 0}, me[4];   /* self.power is not part of the recorded targets */
    const float phi32 = (float)c->phi, phi_over_ra32 = (float)(c->phi / c->ra), inv_jm32 = (float)(1.0 / c->jm);
    const float mm32 = (float)c->mm, prec32 = (float)c->precision, ct0_32 = (float)c->ct0, ct1_32 = (float)c->ct1;
    const float ct2_32 = (float)c->ct2;
    for (int i = 0; i < 4; ++i) {
        double eff_act = act[i];
        if (eff_act > c->max_voltage) eff_act = c->max_voltage;
        else if (eff_act < c->min_voltage) eff_act = c->min_voltage;
        const float eff32 = (float)eff_act;
        float phi_w = phi32 * s->propw[i];
        me[i] = phi_over_ra32 * (eff32 - phi_w);
        float d_prop_w = inv_jm32 * (me[i] - mm32);
        float w_m = s->propw[i] + prec32 * d_prop_w;
        const float *pc = &c->prop_coord[3 * i];
        float l_m = norm3_f32(pc);
        float bv[3], cr[3];
        mat3_vec_f32_plain(s->Rinv, s->vel, bv);
        cross_f32(s->omega, pc, cr);
        float v_1 = bv[2] + cr[2] * l_m;
        float sign = v_1 > 0 ? 1.0f : -1.0f;
        float thrust = ((ct0_32 * w_m) * w_m + (ct1_32 * w_m) * v_1) + ((ct2_32 * v_1) * v_1) * sign;
        s->propw[i] = w_m;
        prop_force_z = prop_force_z + thrust;
        float a[3] = {-0.0f, -0.0f, -thrust};
        cross_f32(a, pc, cr);
        prop_torque[0] += cr[0]; prop_torque[1] += cr[1]; prop_torque[2] += cr[2];
    }
    prop_torque[2] += ((-me[0] + me[1]) - me[2]) + me[3];
    float DfRinv[9], tmp[3], f_drag[3], t_drag[3];
    mat3_mul_f32(c->drag_f, s->Rinv, DfRinv);
    mat3_vec_f32_plain(DfRinv, s->vel, tmp);
    float nv = -norm3_f32(s->vel);
    for (int k = 0; k < 3; ++k) f_drag[k] = nv * tmp[k];
    mat3_vec_f32_plain(c->drag_m, s->omega, tmp);
    float nw = -norm3_f32(s->omega);
    for (int k = 0; k < 3; ++k) t_drag[k] = nw * tmp[k];
    const float gravity_acc[3] = {0.0f, 0.0f, -9.8f};
    float f_grav[3], t_grav[3];
    mat3_vec_f32(s->Rinv, gravity_acc, f_grav);
    for (int k = 0; k < 3; ++k) f_grav[k] = f_grav[k] * (float)c->quality;
    cross_f32(f_grav, c->gravity_center, t_grav);
    const float prop_force[3] = {0.0f, 0.0f, prop_force_z};
    float f_all[3], t_all[3], body_acc[3], acc[3];
    for (int k = 0; k < 3; ++k) {
        f_all[k] = (prop_force[k] + f_grav[k]) + f_drag[k];
        t_all[k] = (prop_torque[k] + (-t_grav[k])) + t_drag[k];
        body_acc[k] = f_all[k] / (float)c->quality;
    }
    mat3_vec_f32_plain(s->R, body_acc, acc);
    const float half_dt2 = (float)(0.5 * c->precision * c->precision);
    for (int k = 0; k < 3; ++k) s->pos[k] = s->pos[k] + (s->vel[k] * prec32 + half_dt2 * acc[k]);
    for (int k = 0; k < 3; ++k) s->vel[k] = s->vel[k] + prec32 * acc[k];
    float alpha[3], tmp_w[3];
    mat3_vec_f32_plain(c->inertia_inv, t_all, alpha);
    const float half_dt = (float)(0.5 * c->precision);
    for (int k = 0; k < 3; ++k) tmp_w[k] = s->omega[k] + half_dt * alpha[k];
    float S[9] = {0};
    S[1] = -tmp_w[2]; S[2] = tmp_w[1]; S[3] = tmp_w[2]; S[5] = -tmp_w[0]; S[6] = -tmp_w[1]; S[7] = tmp_w[0];
    float RS[9];
    mat3_mul_f32(s->R, S, RS);
    for (int k = 0; k < 9; ++k) s->R[k] = s->R[k] + prec32 * RS[k];
    for (int k = 0; k < 3; ++k) s->omega[k] = s->omega[k] + prec32 * alpha[k];
    qo_inv3_f32(s->R, s->Rinv);
}

/* define_velocity_control_task quadrotorsim.py:306-319: nt steps from the zero state with the given
 * (already float32) random actions; records global_velocity after every step. */
void qo_velocity_targets(const qo_consts *c, int nt, const float *actions, float *targets) {
    qo_state32 s;
    memset(&s, 0, sizeof(s));
    s.R[0] = s.R[4] = s.R[8] = 1.0f;
    s.Rinv[0] = s.Rinv[4] = s.Rinv[8] = 1.0f;
    const int times = (int)(c->dt / c->precision);
    for (int t = 0; t < nt; ++t) {
        for (int k = 0; k < times; ++k) qo_substep_f32state(c, &s, &actions[4 * t]);
        targets[3 * t] = s.vel[0]; targets[3 * t + 1] = s.vel[1]; targets[3 * t + 2] = s.vel[2];
    }
}

int qo_sim_step(const qo_consts *c, qo_state *s, const float act[4]) {
    /* quadrotorsim.py:295-304; env.py:129,135 hands over f32 values widened to python floats */
    double a[4] = {act[0], act[1], act[2], act[3]};
    int times = (int)(c->dt / c->precision);
    for (int t = 0; t < times; ++t) {
        qo_substep(c, s, a);
        int f = qo_failed(c, s);
        if (f) return f;                     /* the reference raises here, state stays as is */
    }
    return 0;
}

/* ---- observation: quadrotorsim.py:260-293, :111-120; env.py:193-209 ---------------------- */

void qo_observe(const qo_consts *c, const qo_state *s, float obs[16]) {
    double b_v[3];
    float b_pos[3], imu[3];
    const float gravity_acc[3] = {0.0f, 0.0f, -9.8f};
    mat3_vec_f32f64(s->Rinv, s->vel, b_v);        /* :261-262 f64 */
    mat3_vec_f32(s->Rinv, s->pos, b_pos);         /* :263-264 f32 */
    mat3_vec_f32(s->Rinv, gravity_acc, imu);      /* :277-278 body_acceleration is always 0 */
    const float *R = s->R;
    float roll = atan2f(R[7], R[8]);                                   /* :112-113 */
    float pitch = atan2f(-R[6], sqrtf(R[7] * R[7] + R[8] * R[8]));     /* :114-117 */
    float yaw = atan2f(R[3], R[0]);                                    /* :118-119 */
    obs[0] = (float)b_v[0]; obs[1] = (float)b_v[1]; obs[2] = (float)b_v[2];
    obs[3] = b_pos[0]; obs[4] = b_pos[1]; obs[5] = b_pos[2];
    obs[6] = 0.0f + imu[0]; obs[7] = 0.0f + imu[1]; obs[8] = 0.0f + imu[2];
    obs[9] = (float)s->omega[0]; obs[10] = (float)s->omega[1]; obs[11] = (float)s->omega[2];
    obs[12] = pitch; obs[13] = roll; obs[14] = yaw;
    obs[15] = s->pos[2] + (float)c->z_offset;     /* env.py:203-204 f32 + weak python float */
}

/* ---- collision: env.py:248-260 with python slice semantics ------------------------------- */

static void py_slice(long a, long b, long len, long *lo, long *hi) {
    /* normalise map[a:b] exactly like CPython (negative indices wrap once, then clamp) */
    if (a < 0) { a += len; if (a < 0) a = 0; } else if (a > len) a = len;
    if (b < 0) { b += len; if (b < 0) b = 0; } else if (b > len) b = len;
    *lo = a; *hi = b;
}

/* (long)x is undefined in C for a NaN and for values outside long's range (UBSan: float-cast-overflow). The reference raises there
 * (math.floor of a NaN or an infinity); x86-64's conversion returns LONG_MIN, which is what this file has always computed for the
 * state of an env whose position is no longer finite. Kept, as a defined result. */
static long to_long(double x) {
    return (x >= -9223372036854775808.0 && x < 9223372036854775808.0) ? (long)x : (long)(-9223372036854775807L - 1);
}

static int collision(const qo_consts *c, const double old_pos[3], const double new_pos[3]) {
    long mn[3], mx[3];
    for (int i = 0; i < 3; ++i) {
        double lo = old_pos[i] < new_pos[i] ? old_pos[i] : new_pos[i];  /* min(x[i], y[i]) */
        double hi = old_pos[i] > new_pos[i] ? old_pos[i] : new_pos[i];
        /* python min/max return the first argument on ties; values equal either way */
        mn[i] = to_long(floor(lo));
        mx[i] = to_long(ceil(hi));
    }
    int any = 0;
    if (c->map) {
        long y0, y1, x0, x1;
        py_slice(mn[1], mx[1] + 1, c->map_h, &y0, &y1);
        py_slice(mn[0], mx[0] + 1, c->map_w, &x0, &x1);
        for (long y = y0; y < y1 && !any; ++y)
            for (long x = x0; x < x1; ++x)
                if (c->map[y * c->map_w + x] != 0) { any = 1; break; }
    }
    /* env.py:257 compares heights against the *bool* np.any(taken_pos) */
    return (mn[2] < any) || (mx[2] < any);
}

/* ---- one env.step: env.py:127-165 -------------------------------------------------------- */

int qo_env_step(const qo_consts *c, qo_state *s, int *ct, const float act[4],
                float obs[16], double *reward, int *done) {
    *ct += 1;                                                           /* :128 */
    /* :131-133 f32 + np.int64 offset -> f64 for x,y; f32 + python float -> f32 for z */
    double old_pos[3] = {(double)s->pos[0] + (double)c->x_offset, (double)s->pos[1] + (double)c->y_offset,
                         (double)(s->pos[2] + (float)c->z_offset)};
    int failed = qo_sim_step(c, s, act);                                /* :135 */
    qo_observe(c, s, obs);                                              /* :136-138 */
    if (failed) {               /* reference raises out of step(); batched engine reports a flag */
        *reward = 0.0;
        *done = 1;
        *ct = 0;
        return failed;
    }
    double new_pos[3] = {(double)s->pos[0] + (double)c->x_offset, (double)s->pos[1] + (double)c->y_offset,
                         (double)(s->pos[2] + (float)c->z_offset)};
    int is_collision = collision(c, old_pos, new_pos);                  /* :145 */

    /* _get_reward env.py:211-246 */
    float energy = (float)c->dt * s->power;                  /* python float * np.float32 -> f32 */
    double r;
    /* -min(energy, healthy): python's min keeps `energy` unless `healthy < energy`, which NumPy
       evaluates in f32 (weak python float); the picked object keeps its own precision */
    if ((float)c->healthy_reward < energy) r = -c->healthy_reward;
    else r = -(double)energy;
    const double energy64 = c->dt * (double)s->power;        /* numpy 1.22: float64 */
    if (qo_legacy_promotion) r = (c->healthy_reward < energy64) ? -c->healthy_reward : -energy64;
    double task_reward = is_collision ? 0.0 : c->healthy_reward;
    if (c->task == QO_TASK_HOVERING) {
        double velocity_norm = norm3_f64(s->vel);
        double angular_velocity_norm = norm3_f64(s->omega);
        task_reward -= 1.0 * velocity_norm + 1.0 * angular_velocity_norm;
        float z_move = fabsf(s->pos0_z - s->pos[2]);         /* pos_0[2] - state['z'], f32 */
        if (z_move < 0.5f) task_reward += 10;
        else {
            float o = 0.5f - z_move;                          /* weak 0.5 - f32 -> f32 */
            const double o64 = qo_legacy_promotion ? 0.5 - (double)z_move : (double)o;    /* numpy 1.22: float64 */
            task_reward += (-20.0 > o64) ? -20.0 : o64;       /* max(-20, o) */
        }
    }
    if (c->task == QO_TASK_HOVERING || qo_legacy_promotion || ((float)c->healthy_reward < energy)) {
        r += task_reward;                 /* np.float64 task_reward (hovering) or python floats only */
    } else {
        /* no_collision: np.float32(-energy) + python float -> the python float is weak, f32 add */
        r = (double)((float)r + (float)task_reward);
    }
    *reward = r;

    int reset = 0;
    if (is_collision) { reset = 1; *ct = 0; }                           /* :147-149 */
    if (*ct == c->nt) { reset = 1; *ct = 0; }                           /* :159-161 */
    *done = reset;
    return 0;
}

/* Quadrotor.step for task='velocity_control' (env.py:127-165 with the :150-157 branch). obs has 19
 * entries: the 16 of qo_observe (z_offset is 0 for this task) + next_target_g_v (env.py:262-273). */
int qo_env_step_velocity(const qo_consts *c, qo_state *s, int *ct, const float act[4], float obs[19],
                         double *reward, int *done) {
    *ct += 1;
    int failed = qo_sim_step(c, s, act);
    qo_observe(c, s, obs);
    const int tn = *ct < c->nt - 1 ? *ct : c->nt - 1;                   /* _update_state :268-269 */
    for (int k = 0; k < 3; ++k) obs[16 + k] = c->velocity_targets[3 * tn + k];
    if (failed) { *reward = 0.0; *done = 1; *ct = 0; return failed; }
    /* :152-157 body-frame target = Rinv(f32) @ target(f32) -> f32 gemv */
    float bt[3];
    mat3_vec_f32(s->Rinv, &c->velocity_targets[3 * (*ct - 1)], bt);
    double b_v[3];
    mat3_vec_f32f64(s->Rinv, s->vel, b_v);
    /* _get_velocity_diff env.py:275-280: np.float32 - np.float64 -> f64 */
    double diff = (fabs((double)bt[0] - b_v[0]) + fabs((double)bt[1] - b_v[1])) + fabs((double)bt[2] - b_v[2]);
    float energy = (float)c->dt * s->power;
    double r = ((float)c->healthy_reward < energy) ? -c->healthy_reward : -(double)energy;
    r += -0.001 * diff;                                                  /* :222-224 */
    *reward = r;
    int reset = 0;
    if (*ct == c->nt) { reset = 1; *ct = 0; }
    *done = reset;
    return 0;
}

/* ---- batch drivers used by the tests and by bench.py's cpu_baseline leg ------------------ */

void qo_batch_env_step(const qo_consts *c, int n, qo_state *states, int *ct, const float *actions,
                       float *obs, double *reward, int *done, int *failed) {
    for (int e = 0; e < n; ++e)
        failed[e] = qo_env_step(c, &states[e], &ct[e], &actions[4 * e], &obs[16 * e], &reward[e], &done[e]);
}

/* ---- fused auto-reset --------------------------------------------------------------------------
 * The reference has no such operation (the user calls env.reset() after done and the noise comes from
 * numpy's global RNG, quadrotorsim.py:239-258). metagym_amd resets a finished env inside the step launch
 * and draws the noise on the device; this is the CPU restatement of THAT definition (include/metagym_hip.h,
 * mg_quadrotor_autoreset), so the path bench.py times has a checker. The generator is Philox4x32-10
 * (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), pinned by the
 * Random123 known-answer vectors in tests/test_oracle_quadrotor.py. */
void qo_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }          /* Weyl key schedule */
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

/* Noise of the `episode`-th auto-reset of global env `gid`: two Philox blocks, key = seed (lo, hi),
 * counter = (gid lo, gid hi, episode, block). Words 0..2 / 3..5 are the magnitudes U[0,1) = w / 2^32 of
 * velocity / body rate, bits 0..2 / 3..5 of word 6 the signs (set -> +1), mirroring
 *   base(f32) + noisy * random(3) * (+-1)        quadrotorsim.py:242-254
 * with python-float `noisy` times a float64 array, times a float64 sign, added to a float32 array -> f64. */
void qo_reset_noise(const qo_autoreset *ar, uint64_t gid, uint32_t episode, double vel[3], double omega[3]) {
    uint32_t w[8];
    const uint32_t key[2] = {(uint32_t)ar->seed, (uint32_t)(ar->seed >> 32)};
    for (uint32_t d = 0; d < 2; ++d) {
        const uint32_t ctr[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), episode, d};
        qo_philox4x32_10(ctr, key, &w[4 * d]);
    }
    const double inv32 = 1.0 / 4294967296.0;
    for (int k = 0; k < 3; ++k) {
        const double sv = ((w[6] >> k) & 1u) ? 1.0 : -1.0;
        const double sw = ((w[6] >> (3 + k)) & 1u) ? 1.0 : -1.0;
        vel[k] = (double)ar->init_velocity[k] + (ar->init_velocity_noisy * ((double)w[k] * inv32)) * sv;
        omega[k] = (double)ar->init_angular_velocity[k] + (ar->init_angular_velocity_noisy * ((double)w[3 + k] * inv32)) * sw;
    }
}

void qo_reset_random(const qo_autoreset *ar, qo_state *s, uint64_t gid, uint32_t episode) {
    qo_zero_state(s);                                                   /* quadrotorsim.py:240 */
    qo_reset_noise(ar, gid, episode, s->vel, s->omega);                 /* :241-254 */
    qo_refresh_inverse(s);                                              /* :256-258 */
    s->pos0_z = s->pos[2];                                              /* env.py:123 */
}

/* One env.step for every env with the fused reset: reward / done / failed describe the step that ended,
 * the obs row of a finished env is the first observation of its next episode (Quadrotor.reset env.py:116-125:
 * ct is left as the done rule set it, i.e. 0), and episode[e] counts the resets. hovering_control / no_collision. */
void qo_batch_env_step_autoreset(const qo_consts *c, const qo_autoreset *ar, int n, qo_state *states, int *ct,
                                 uint32_t *episode, const float *actions, float *obs, double *reward, int *done,
                                 int *failed) {
    for (int e = 0; e < n; ++e) {
        failed[e] = qo_env_step(c, &states[e], &ct[e], &actions[4 * e], &obs[16 * e], &reward[e], &done[e]);
        if (done[e]) {
            qo_reset_random(ar, &states[e], ar->env_id_base + (uint64_t)e, episode[e]);
            episode[e] += 1;
            qo_observe(c, &states[e], &obs[16 * e]);
        }
    }
}

/* iters env-steps for every env, cycling through n_batches action batches [n_batches][n][4];
 * outputs are discarded. An env whose episode ends (collision, ct == nt, failure) restarts from
 * its entry in `init` (the reset states), like the GPU bench's fused auto-reset, so the timed work
 * per env-step stays the full 10 sub-steps. Used by bench.py's cpu_baseline. */
long qo_batch_run(const qo_consts *c, int n, qo_state *states, const qo_state *init, int *ct,
                  const float *actions, int n_batches, int iters) {
    float obs[16];
    double reward;
    int done;
    long count = 0;
    for (int k = 0; k < iters; ++k) {
        const float *a = actions + (size_t)(k % n_batches) * n * 4;
        for (int e = 0; e < n; ++e) {
            qo_env_step(c, &states[e], &ct[e], &a[4 * e], obs, &reward, &done);
            if (done) states[e] = init[e];
            ++count;
        }
    }
    return count;
}

size_t qo_sizeof_state(void) { return sizeof(qo_state); }
size_t qo_sizeof_consts(void) { return sizeof(qo_consts); }
