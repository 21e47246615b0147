/* oracle/walker_oracle.c — plain-C restatement of the articulated-body env step (MetaLocomotion humanoid / ant, BASELINE
 * config C4). TEST INFRASTRUCTURE (oracle/__init__.py): the native CPU baseline of bench.py's C4 entry and the place the
 * per-env-step flop count comes from (-DWO_COUNT_FLOPS, oracle/count_walker_flops.py). Never on the product path.
 *
 * PARITY UNPINNED like everything on this path: the reference calls pybullet.stepSimulation()
 * (metalocomotion/envs/utils/scene_bases.py:45-50), which is not in its tree. What is restated is this repo's own engine,
 * the algorithm of metagym_amd/csrc/walker_core.h's wave kernel step for step — composite-rigid-body M and bias about the
 * base origin, Cholesky, free motion, ground / self-collision / joint-limit rows, projected Gauss-Seidel in Cholesky-whitened
 * velocities, semi-implicit Euler — so the flop count is that of the algorithm the GPU executes (the kernel reaches the
 * same kinematics and subtree sums by parallel scans, which spend redundant lane-operations a serial count does not have:
 * the count is the algorithm's work, a lower bound on the kernel's). It is pinned to the
 * numpy restatement oracle/abd.py (same physics in Jacobian form) to 1e-12 by tests/test_oracle_walker_c.py, and abd.py to
 * physical invariants and the HIP kernels.
 * The Python-side rules around the physics ARE the reference's and are restated exactly like abd.WalkerEnv:
 * torques humanoids.py:50-54 / walker_base.py:26-29, calc_state walker_base.py:31-64, reward / done walker_base_env.py:43-82.
 * Body velocity damping (btMultiBody's 0.04 / 0.04, part of the envs' default "bullet" preset) is here; terrain boxes and
 * per-proxy friction (the shape-generic kernel's extras) are not part of C4 and not here. */
#include "walker_oracle.h"

#include <math.h>
#include <string.h>

#ifdef WO_COUNT_FLOPS
unsigned long long wo_flop_count[9];      /* add/sub, mul, fma (counts once), div, sqrt, sin/cos/atan2/asin; then the solver's
                                           * load: [6] sub-steps, [7] constraint rows summed over them, [8] contacts (ground + self) */
#define FL(k, n) (wo_flop_count[k] += (unsigned long long)(n))
#else
#define FL(k, n) ((void)0)
#endif
#ifdef WO_COUNT_CAPS
unsigned long long wo_cap_count[4];       /* how close the fixed-size contact tables came to their caps (oracle/replay_main.c prints them): [0] most
                                           * candidates in one sub-step, [1] ground candidates dropped because the candidate table was full,
                                           * [2] self-collision pairs left untested for the same reason, [3] most contacts kept in one sub-step */
#define CAP(k, n) (wo_cap_count[k] += (unsigned long long)(n))
#define CAP_MAX(k, n) (wo_cap_count[k] = wo_cap_count[k] > (unsigned long long)(n) ? wo_cap_count[k] : (unsigned long long)(n))
#else
#define CAP(k, n) ((void)0)
#define CAP_MAX(k, n) ((void)0)
#endif
enum { F_ADD = 0, F_MUL = 1, F_FMA = 2, F_DIV = 3, F_SQRT = 4, F_TRIG = 5 };

typedef struct { double x, y, z; } v3;
static inline v3 V(double x, double y, double z) { v3 r = {x, y, z}; return r; }
static inline v3 vadd(v3 a, v3 b) { FL(F_ADD, 3); return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline v3 vsub(v3 a, v3 b) { FL(F_ADD, 3); return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 vscale(double s, v3 a) { FL(F_MUL, 3); return V(s * a.x, s * a.y, s * a.z); }
static inline double vdot(v3 a, v3 b) { FL(F_MUL, 1); FL(F_FMA, 2); return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline v3 vcross(v3 a, v3 b) {
    FL(F_MUL, 3); FL(F_FMA, 3);
    return V(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
static inline v3 ld3(const double *p) { return V(p[0], p[1], p[2]); }
static inline v3 mulMv(const double *R, v3 v) {
    FL(F_MUL, 3); FL(F_FMA, 6);
    return V(R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z, R[6] * v.x + R[7] * v.y + R[8] * v.z);
}
static inline void mulMM(const double *A, const double *B, double *C) {
    FL(F_MUL, 9); FL(F_FMA, 18);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
static inline void rodrigues_sc(v3 k, double s, double c, double *R) {
    const double v = 1.0 - c;
    FL(F_ADD, 1); FL(F_MUL, 15); FL(F_FMA, 9);
    R[0] = c + k.x * k.x * v;       R[1] = k.x * k.y * v - k.z * s; R[2] = k.x * k.z * v + k.y * s;
    R[3] = k.y * k.x * v + k.z * s; R[4] = c + k.y * k.y * v;       R[5] = k.y * k.z * v - k.x * s;
    R[6] = k.z * k.x * v - k.y * s; R[7] = k.z * k.y * v + k.x * s; R[8] = c + k.z * k.z * v;
}

/* ---- model table accessors (layout of mg_walker_models, include/metagym_hip.h) --------------------------------------- */
#define NB (m->nb)
#define NJ (m->nj)
static inline const double *t_body_pos(const wo_model *m) { return m->table; }
static inline const double *t_body_rot(const wo_model *m) { return m->table + 3 * NB; }
static inline const double *t_body_mass(const wo_model *m) { return m->table + 12 * NB; }
static inline const double *t_body_com(const wo_model *m) { return m->table + 13 * NB; }
static inline const double *t_body_inertia(const wo_model *m) { return m->table + 16 * NB; }
static inline const double *t_joint_anchor(const wo_model *m) { return m->table + 25 * NB; }
static inline const double *t_joint_axis(const wo_model *m) { return m->table + 25 * NB + 3 * NJ; }
static inline const double *t_joint_lo(const wo_model *m) { return m->table + 25 * NB + 6 * NJ; }
static inline const double *t_joint_hi(const wo_model *m) { return m->table + 25 * NB + 7 * NJ; }
static inline const double *t_joint_arm(const wo_model *m) { return m->table + 25 * NB + 8 * NJ; }
static inline const double *t_joint_damp(const wo_model *m) { return m->table + 25 * NB + 9 * NJ; }
static inline const double *t_joint_stiff(const wo_model *m) { return m->table + 25 * NB + 10 * NJ; }
static inline const double *t_motor(const wo_model *m) { return m->table + 25 * NB + 11 * NJ; }
static inline const double *t_sph_pos(const wo_model *m) { return m->table + 25 * NB + 12 * NJ; }
static inline const double *t_sph_r(const wo_model *m) { return m->table + 25 * NB + 12 * NJ + 3 * m->ns; }
static inline const double *t_geom_p0(const wo_model *m) { return m->table + 25 * NB + 12 * NJ + 4 * m->ns; }
static inline const double *t_geom_p1(const wo_model *m) { return m->table + 25 * NB + 12 * NJ + 4 * m->ns + 3 * m->ng; }
static inline const double *t_geom_r(const wo_model *m) { return m->table + 25 * NB + 12 * NJ + 4 * m->ns + 6 * m->ng; }

typedef struct {
    double R[WO_MAX_BODIES][9];
    v3 o[WO_MAX_BODIES], c[WO_MAX_BODIES];
    v3 p[WO_MAX_JOINTS], a[WO_MAX_JOINTS];
    v3 fw[WO_MAX_BODIES], fal[WO_MAX_BODIES], fxr[WO_MAX_BODIES], far_[WO_MAX_BODIES];   /* velocity-product frames */
    v3 fvr[WO_MAX_BODIES];                                                               /* velocity of the frame's reference point (with_frames == 2) */
    unsigned mask[WO_MAX_BODIES];
    int dbody[WO_MAX_DOF];
} kin_t;

/* world frames + (with_frames) the velocity-product accelerations, bodies in index order (parents first) */
static void kinematics(const wo_model *m, const wo_state *s, kin_t *k, int with_frames) {
    int j = 0;
    for (int d = 0; d < 6; ++d) k->dbody[d] = 0;
    for (int b = 0; b < NB; ++b) {
        double Rc[9];
        v3 oc, w, al, xr, ar, vr = V(0, 0, 0);
        unsigned mk = 0;
        const int pb = m->body_parent[b];
        if (pb < 0) {
            memcpy(Rc, s->rot, sizeof(Rc));
            oc = ld3(s->pos);
            w = ld3(s->omega); al = V(0, 0, 0); xr = oc; ar = V(0, 0, 0); vr = ld3(s->vel);
        } else {
            mulMM(k->R[pb], t_body_rot(m) + 9 * b, Rc);
            oc = vadd(k->o[pb], mulMv(k->R[pb], ld3(t_body_pos(m) + 3 * b)));
            mk = k->mask[pb];
            w = k->fw[pb]; al = k->fal[pb]; xr = k->fxr[pb]; ar = k->far_[pb];
            if (with_frames == 2) vr = k->fvr[pb];
        }
        for (; j < NJ && m->joint_body[j] == b; ++j) {
            const v3 anchor = ld3(t_joint_anchor(m) + 3 * j), axis = ld3(t_joint_axis(m) + 3 * j);
            const v3 pj = vadd(oc, mulMv(Rc, anchor)), aj = mulMv(Rc, axis);
            k->p[j] = pj; k->a[j] = aj;
            double Rj[9], Rn[9];
            FL(F_TRIG, 2);
            rodrigues_sc(axis, sin(s->q[j]), cos(s->q[j]), Rj);
            mulMM(Rc, Rj, Rn);
            oc = vsub(pj, mulMv(Rn, anchor));
            memcpy(Rc, Rn, sizeof(Rc));
            mk |= 1u << j;
            k->dbody[6 + j] = b;
            if (with_frames) {
                const v3 r = vsub(pj, xr);
                ar = vadd(vadd(ar, vcross(al, r)), vcross(w, vcross(w, r)));
                if (with_frames == 2) vr = vadd(vr, vcross(w, r));
                xr = pj;
                const v3 wj = vscale(s->qd[j], aj);
                al = vadd(al, vcross(w, wj));
                w = vadd(w, wj);
            }
        }
        memcpy(k->R[b], Rc, sizeof(Rc));
        k->o[b] = oc;
        k->c[b] = vadd(oc, mulMv(Rc, ld3(t_body_com(m) + 3 * b)));
        k->mask[b] = mk;
        k->fw[b] = w; k->fal[b] = al; k->fxr[b] = xr; k->far_[b] = ar; k->fvr[b] = vr;
    }
}

static inline v3 jac_lin(const kin_t *k, unsigned mk, v3 x, int d) {
    if (d < 3) return V(d == 0, d == 1, d == 2);
    if (d < 6) return vcross(V(d == 3, d == 4, d == 5), vsub(x, k->o[0]));
    const int j = d - 6;
    if (!((mk >> j) & 1u)) return V(0, 0, 0);
    return vcross(k->a[j], vsub(x, k->p[j]));
}

static void segment_closest(v3 p1, v3 q1, v3 p2, v3 q2, v3 *c1, v3 *c2) {    /* Ericson 5.1.9 */
    const v3 d1 = vsub(q1, p1), d2 = vsub(q2, p2), r = vsub(p1, p2);
    const double a = vdot(d1, d1), e = vdot(d2, d2), f = vdot(d2, r), eps = 1e-12;
    double sc, tc;
    if (a <= eps && e <= eps) { *c1 = p1; *c2 = p2; return; }
    if (a <= eps) { sc = 0.0; FL(F_DIV, 1); tc = fmin(fmax(f / e, 0.0), 1.0); }
    else {
        const double c = vdot(d1, r);
        if (e <= eps) { tc = 0.0; FL(F_DIV, 1); sc = fmin(fmax(-c / a, 0.0), 1.0); }
        else {
            const double b = vdot(d1, d2), den = a * e - b * b;
            FL(F_MUL, 5); FL(F_ADD, 3); FL(F_DIV, 2);
            sc = den > eps ? fmin(fmax((b * f - c * e) / den, 0.0), 1.0) : 0.0;
            tc = (b * sc + f) / e;
            if (tc < 0.0) { tc = 0.0; FL(F_DIV, 1); sc = fmin(fmax(-c / a, 0.0), 1.0); }
            else if (tc > 1.0) { tc = 1.0; FL(F_DIV, 1); FL(F_ADD, 1); sc = fmin(fmax((b - c) / a, 0.0), 1.0); }
        }
    }
    *c1 = vadd(p1, vscale(sc, d1));
    *c2 = vadd(p2, vscale(tc, d2));
}

static void tangent_basis(v3 n, v3 *t1, v3 *t2) {
    const v3 ref = fabs(n.x) < 0.9 ? V(1, 0, 0) : V(0, 1, 0);
    v3 t = vcross(n, ref);
    FL(F_SQRT, 1); FL(F_DIV, 1);
    t = vscale(1.0 / sqrt(vdot(t, t)), t);
    *t1 = t;
    *t2 = vcross(n, t);
}

#define TRI(r, c) ((r) * ((r) + 1) / 2 + (c))

int wo_substep(const wo_model *m, const wo_params *prm, wo_state *s, const double *tau_motor, unsigned long long touch[2]) {
    const int n = 6 + NJ, maxc = WO_MAX_CONTACTS;
    const double dt = prm->dt;
    kin_t k;
    const int damped = prm->body_linear_damping != 0.0 || prm->body_angular_damping != 0.0;
    kinematics(m, s, &k, damped ? 2 : 1);
    /* ---- M and h by the composite-rigid-body algorithm about the base origin O (walker_core.h wave_substep) ---- */
    double comp[WO_MAX_BODIES][16];
    const v3 O = k.o[0];
    for (int b = 0; b < NB; ++b) {
        const v3 w = k.fw[b], al = k.fal[b], xr = k.fxr[b], ar = k.far_[b], cb = k.c[b];
        const v3 rx = vsub(cb, xr);
        const v3 a_c = vadd(vadd(ar, vcross(al, rx)), vcross(w, vcross(w, rx)));
        double RI[9], Ic[9];
        const double *R = k.R[b];
        mulMM(R, t_body_inertia(m) + 9 * b, RI);
        double Rt[9] = {R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]};
        mulMM(RI, Rt, Ic);
        const double mass = t_body_mass(m)[b];
        FL(F_ADD, 1);
        v3 F = vscale(mass, V(a_c.x, a_c.y, a_c.z + prm->gravity));
        v3 N = vadd(mulMv(Ic, al), vcross(w, mulMv(Ic, w)));
        if (damped) {   /* btMultiBody's velocity damping: force -m v_c (k + k |v_c|) at the centre of mass, torque -I w (k + k |w|);
                         * their negatives join the bias wrench (walker_core.h wave_substep, oracle/abd.py mass_matrix_and_bias) */
            const v3 vc = vadd(k.fvr[b], vcross(w, rx));
            const double kl = prm->body_linear_damping, ka = prm->body_angular_damping;
            FL(F_SQRT, 2); FL(F_MUL, 3); FL(F_ADD, 2);
            F = vadd(F, vscale(mass * (kl + kl * sqrt(vdot(vc, vc))), vc));
            N = vadd(N, vscale(ka + ka * sqrt(vdot(w, w)), mulMv(Ic, w)));
        }
        const v3 r = vsub(cb, O);
        const v3 NO = vadd(N, vcross(r, F));
        const double rr = vdot(r, r);
        double *cp = comp[b];
        FL(F_MUL, 12); FL(F_ADD, 9);
        cp[0] = mass; cp[1] = mass * r.x; cp[2] = mass * r.y; cp[3] = mass * r.z;
        cp[4] = Ic[0] + mass * (rr - r.x * r.x); cp[5] = Ic[1] - mass * r.x * r.y; cp[6] = Ic[2] - mass * r.x * r.z;
        cp[7] = Ic[4] + mass * (rr - r.y * r.y); cp[8] = Ic[5] - mass * r.y * r.z; cp[9] = Ic[8] + mass * (rr - r.z * r.z);
        cp[10] = F.x; cp[11] = F.y; cp[12] = F.z; cp[13] = NO.x; cp[14] = NO.y; cp[15] = NO.z;
    }
    for (int b = NB - 1; b > 0; --b) {          /* subtree sums: children have larger indices than their parents */
        double *pp = comp[m->body_parent[b]];
        FL(F_ADD, 16);
        for (int i = 0; i < 16; ++i) pp[i] += comp[b][i];
    }
    double Sd[WO_MAX_DOF][6], Fd[WO_MAX_DOF][6], h[WO_MAX_DOF], M[WO_MAX_DOF * (WO_MAX_DOF + 1) / 2];
    for (int d = 0; d < n; ++d) {
        v3 v = V(0, 0, 0), w = V(0, 0, 0);
        if (d < 3) v = V(d == 0, d == 1, d == 2);
        else if (d < 6) w = V(d == 3, d == 4, d == 5);
        else { w = k.a[d - 6]; v = vcross(w, vsub(O, k.p[d - 6])); }
        const double *cp = comp[k.dbody[d]];
        const v3 hc = V(cp[1], cp[2], cp[3]);
        const v3 pl = vadd(vscale(cp[0], v), vcross(w, hc));
        FL(F_MUL, 3); FL(F_FMA, 6);
        const v3 Iw = V(cp[4] * w.x + cp[5] * w.y + cp[6] * w.z, cp[5] * w.x + cp[7] * w.y + cp[8] * w.z, cp[6] * w.x + cp[8] * w.y + cp[9] * w.z);
        const v3 Lo = vadd(vcross(hc, v), Iw);
        Sd[d][0] = v.x; Sd[d][1] = v.y; Sd[d][2] = v.z; Sd[d][3] = w.x; Sd[d][4] = w.y; Sd[d][5] = w.z;
        Fd[d][0] = pl.x; Fd[d][1] = pl.y; Fd[d][2] = pl.z; Fd[d][3] = Lo.x; Fd[d][4] = Lo.y; Fd[d][5] = Lo.z;
        FL(F_ADD, 1);
        h[d] = vdot(v, V(cp[10], cp[11], cp[12])) + vdot(w, V(cp[13], cp[14], cp[15]));
    }
    for (int d = 0; d < n; ++d)
        for (int e = 0; e <= d; ++e) {
            double acc = 0.0;
            if (e < 6 || ((k.mask[k.dbody[d]] >> (e - 6)) & 1u)) {
                FL(F_MUL, 1); FL(F_FMA, 5);
                acc = (Sd[e][0] * Fd[d][0] + Sd[e][1] * Fd[d][1] + Sd[e][2] * Fd[d][2]) + (Sd[e][3] * Fd[d][3] + Sd[e][4] * Fd[d][4] + Sd[e][5] * Fd[d][5]);
            }
            if (d == e && d >= 6) { FL(F_ADD, 1); acc += t_joint_arm(m)[d - 6]; }
            M[TRI(d, e)] = acc;
        }
    /* ---- Cholesky M = L L^T (packed lower), 1 / diag kept ---- */
    double idg[WO_MAX_DOF];
    for (int c = 0; c < n; ++c) {
        double v = M[TRI(c, c)];
        for (int kk = 0; kk < c; ++kk) { FL(F_FMA, 1); v -= M[TRI(c, kk)] * M[TRI(c, kk)]; }
        FL(F_SQRT, 1); FL(F_DIV, 1);
        const double l = sqrt(v);
        M[TRI(c, c)] = l;
        idg[c] = 1.0 / l;
        for (int r = c + 1; r < n; ++r) {
            double a = M[TRI(r, c)];
            for (int kk = 0; kk < c; ++kk) { FL(F_FMA, 1); a -= M[TRI(r, kk)] * M[TRI(c, kk)]; }
            FL(F_MUL, 1);
            M[TRI(r, c)] = a * idg[c];
        }
    }
    /* ---- free motion in whitened coordinates: y* = L^T u + dt L^-1 (tau - h) ---- */
    double u[WO_MAX_DOF], x[WO_MAX_DOF], y[WO_MAX_DOF];
    for (int d = 0; d < n; ++d) {
        x[d] = -h[d];
        if (d >= 6) {
            const int j = d - 6;
            FL(F_ADD, 1); FL(F_FMA, 2);
            x[d] += tau_motor[j] - t_joint_damp(m)[j] * s->qd[j] - t_joint_stiff(m)[j] * s->q[j];
            u[d] = s->qd[j];
        } else u[d] = d < 3 ? s->vel[d] : s->omega[d - 3];
    }
    for (int d = 0; d < n; ++d) {                /* L z = b */
        double v = x[d];
        for (int kk = 0; kk < d; ++kk) { FL(F_FMA, 1); v -= M[TRI(d, kk)] * x[kk]; }
        FL(F_MUL, 1);
        x[d] = v * idg[d];
    }
    for (int d = 0; d < n; ++d) {                /* y = L^T u + dt z */
        double v = 0.0;
        for (int r = d; r < n; ++r) { FL(F_FMA, 1); v += M[TRI(r, d)] * u[r]; }
        FL(F_FMA, 1);
        y[d] = v + dt * x[d];
    }
    /* ---- constraint detection: contact CANDIDATES in candidate order — ground plane per collision sphere (sphere order; inside
     *      the contact margin: depth > -contact_margin), then self-collision pairs (pair order; penetration only) — at most
     *      WO_MAX_CANDIDATES (later ones dropped); of those the maxc DEEPEST are kept (ties: the earlier candidate), in candidate
     *      order (abd.select_contacts); then joint limits. touch = every sphere with a ground candidate, kept or not: what
     *      getContactPoints reports (walker_base_env.py:57-63). Bias: abd.contact_bias. ---- */
    double cx[WO_MAX_CONTACTS][6], bias[WO_MAX_ROWS], Jh[WO_MAX_ROWS][WO_MAX_DOF];
    int csph[WO_MAX_CONTACTS][2], kind[WO_MAX_ROWS], partner[WO_MAX_ROWS];
    double qx[WO_MAX_CANDIDATES][6], qdepth[WO_MAX_CANDIDATES];
    int qid[WO_MAX_CANDIDATES][2];
    int ncand = 0;
    touch[0] = touch[1] = 0ull;
    for (int g = 0; g < m->ns; ++g) {
        const int b = m->sphere_body[g];
        const v3 xw = vadd(k.o[b], mulMv(k.R[b], ld3(t_sph_pos(m) + 3 * g)));
        FL(F_ADD, 1);
        const double depth = t_sph_r(m)[g] - xw.z;
        if (depth > -(m->sph_margin ? m->sph_margin[g] : prm->contact_margin)) {
            touch[g >> 6] |= 1ull << (g & 63);
            if (ncand < WO_MAX_CANDIDATES) {
                qx[ncand][0] = xw.x; qx[ncand][1] = xw.y; qx[ncand][2] = depth;
                qid[ncand][0] = g; qid[ncand][1] = -1; qdepth[ncand] = depth;
                ++ncand;
            } else CAP(1, 1);
        }
    }
    if (prm->self_collision)
        for (int pr = 0; pr < m->npairs; ++pr) {
            if (ncand >= WO_MAX_CANDIDATES) { CAP(2, m->npairs - pr); break; }
            const int ga = m->pair_a[pr], gb = m->pair_b[pr], ba = m->geom_body[ga], bb = m->geom_body[gb];
            v3 ca, cb;
            segment_closest(vadd(k.o[ba], mulMv(k.R[ba], ld3(t_geom_p0(m) + 3 * ga))), vadd(k.o[ba], mulMv(k.R[ba], ld3(t_geom_p1(m) + 3 * ga))),
                            vadd(k.o[bb], mulMv(k.R[bb], ld3(t_geom_p0(m) + 3 * gb))), vadd(k.o[bb], mulMv(k.R[bb], ld3(t_geom_p1(m) + 3 * gb))), &ca, &cb);
            const v3 dv = vsub(ca, cb);
            FL(F_SQRT, 1); FL(F_ADD, 2);
            const double dist = sqrt(vdot(dv, dv));
            const double ra = t_geom_r(m)[ga], rb = t_geom_r(m)[gb], depth = ra + rb - dist;
            if (depth > 0.0 && dist > 1e-9) {
                FL(F_DIV, 1);
                const v3 nrm = vscale(1.0 / dist, dv);
                const v3 xc = vscale(0.5, vadd(vsub(ca, vscale(ra, nrm)), vadd(cb, vscale(rb, nrm))));
                qx[ncand][0] = xc.x; qx[ncand][1] = xc.y; qx[ncand][2] = xc.z; qx[ncand][3] = nrm.x; qx[ncand][4] = nrm.y; qx[ncand][5] = nrm.z;
                qid[ncand][0] = ba; qid[ncand][1] = bb; qdepth[ncand] = depth;
                ++ncand;
            }
        }
    int ncont = 0;
    for (int c = 0; c < ncand; ++c) {
        if (ncand > maxc) {                      /* rank among the candidates: deeper ones, and equally deep earlier ones — depths on
                                                  * abd.depth_key's 2^-20 m grid, so that points equally deep by symmetry tie */
            int rank = 0;
            const double kc = floor(qdepth[c] * 1048576.0);
            for (int o = 0; o < ncand; ++o) { const double ko = floor(qdepth[o] * 1048576.0); rank += (ko > kc) || (ko == kc && o < c); }
            if (rank >= maxc) continue;
        }
        memcpy(cx[ncont], qx[c], sizeof(cx[ncont]));
        csph[ncont][0] = qid[c][0]; csph[ncont][1] = qid[c][1];
        const double depth = qdepth[c];
        FL(F_MUL, 1); FL(F_DIV, 1);
        bias[3 * ncont] = (depth >= 0.0 ? prm->erp * depth : depth) / dt; kind[3 * ncont] = 0; partner[3 * ncont] = -1;
        const int fk = qid[c][1] == -1 ? 1 : 3;
        bias[3 * ncont + 1] = 0.0; kind[3 * ncont + 1] = fk; partner[3 * ncont + 1] = 3 * ncont;
        bias[3 * ncont + 2] = 0.0; kind[3 * ncont + 2] = fk == 1 ? 2 : 3; partner[3 * ncont + 2] = 3 * ncont;
        ++ncont;
    }
    CAP_MAX(0, ncand); CAP_MAX(3, ncont);
    int nr = 3 * ncont;
    for (int c = 0; c < ncont; ++c)
        for (int d = 0; d < n; ++d) {
            if (csph[c][1] == -1) {
                const v3 jc = jac_lin(&k, k.mask[m->sphere_body[csph[c][0]]], V(cx[c][0], cx[c][1], 0.0), d);
                Jh[3 * c][d] = jc.z; Jh[3 * c + 1][d] = jc.x; Jh[3 * c + 2][d] = jc.y;
            } else {
                const v3 xc = V(cx[c][0], cx[c][1], cx[c][2]), nrm = V(cx[c][3], cx[c][4], cx[c][5]);
                const v3 jd = vsub(jac_lin(&k, k.mask[csph[c][0]], xc, d), jac_lin(&k, k.mask[csph[c][1]], xc, d));
                v3 t1, t2;
                tangent_basis(nrm, &t1, &t2);
                Jh[3 * c][d] = vdot(nrm, jd); Jh[3 * c + 1][d] = vdot(t1, jd); Jh[3 * c + 2][d] = vdot(t2, jd);
            }
        }
    for (int j = 0; j < NJ; ++j) {
        const double qj = s->q[j], lo = t_joint_lo(m)[j], hi = t_joint_hi(m)[j];
        double sg = 0.0, viol = 0.0;
        if (qj < lo) { sg = 1.0; viol = lo - qj; } else if (qj > hi) { sg = -1.0; viol = qj - hi; }
        if (sg != 0.0) {
            FL(F_ADD, 1); FL(F_MUL, 1); FL(F_DIV, 1);
            for (int d = 0; d < n; ++d) Jh[nr][d] = d == 6 + j ? sg : 0.0;
            bias[nr] = prm->limit_erp * viol / dt; kind[nr] = 4; partner[nr] = j;
            ++nr;
        }
    }
    /* ---- whiten: Jh_r <- J_r L^-T (forward substitution per row), diag_r = 1 / (Jh_r . Jh_r) ---- */
    double rdiag[WO_MAX_ROWS], lam[WO_MAX_ROWS];
    for (int r = 0; r < nr; ++r) {
        double dd = 0.0;
        for (int d = 0; d < n; ++d) {
            double v = Jh[r][d];
            for (int kk = 0; kk < d; ++kk) { FL(F_FMA, 1); v -= M[TRI(d, kk)] * Jh[r][kk]; }
            FL(F_MUL, 1); FL(F_FMA, 1);
            v *= idg[d];
            Jh[r][d] = v;
            dd += v * v;
        }
        if (dd > 0.0) FL(F_DIV, 1);
        rdiag[r] = dd > 0.0 ? 1.0 / dd : 0.0;
        lam[r] = 0.0;
    }
    /* ---- projected Gauss-Seidel on the whitened velocity (natural row order, zero warm start) ---- */
    for (int it = 0; it < prm->iterations; ++it)
        for (int r = 0; r < nr; ++r) {
            if (!(rdiag[r] > 0.0)) continue;
            double jv = 0.0;
            for (int d = 0; d < n; ++d) { FL(F_FMA, 1); jv += Jh[r][d] * y[d]; }
            FL(F_ADD, 2); FL(F_MUL, 1);
            double xr = lam[r] - (jv - bias[r]) * rdiag[r];
            if (kind[r] == 0 || kind[r] >= 4) xr = xr > 0.0 ? xr : 0.0;
            else {
                FL(F_MUL, 1);
                const double lim = (kind[r] == 3 ? prm->self_friction : prm->friction) * lam[partner[r]];
                xr = xr < -lim ? -lim : (xr > lim ? lim : xr);
            }
            FL(F_ADD, 1);
            const double dl = xr - lam[r];
            for (int d = 0; d < n; ++d) { FL(F_FMA, 1); y[d] += Jh[r][d] * dl; }
            lam[r] = xr;
        }
    /* ---- u = L^-T y, integrate ---- */
    for (int r = n - 1; r >= 0; --r) {
        double v = y[r];
        for (int kk = r + 1; kk < n; ++kk) { FL(F_FMA, 1); v -= M[TRI(kk, r)] * u[kk]; }
        FL(F_MUL, 1);
        u[r] = v * idg[r];
    }
#ifdef WO_COUNT_FLOPS
    wo_flop_count[6] += 1; wo_flop_count[7] += (unsigned long long)nr; wo_flop_count[8] += (unsigned long long)ncont;
#endif
    if (prm->max_coordinate_velocity > 0.0)      /* btMultiBody::applyDeltaVeeMultiDof's clamp of every generalized velocity */
        for (int d = 0; d < n; ++d) {             /* two comparisons like btClamp: a NaN stays a NaN (fmin / fmax would drop it) */
            const double mv = prm->max_coordinate_velocity;
            u[d] = u[d] < -mv ? -mv : (u[d] > mv ? mv : u[d]);
        }
    for (int i = 0; i < 3; ++i) { s->vel[i] = u[i]; s->omega[i] = u[3 + i]; FL(F_FMA, 1); s->pos[i] += dt * u[i]; }
    for (int j = 0; j < NJ; ++j) { s->qd[j] = u[6 + j]; FL(F_FMA, 1); s->q[j] += dt * u[6 + j]; }
    const v3 om = ld3(s->omega);
    FL(F_SQRT, 1); FL(F_MUL, 1);
    const double wn = sqrt(vdot(om, om));
    if (wn * dt > 0.0) {
        double Rw[9], Rn[9];
        FL(F_TRIG, 2); FL(F_DIV, 1);
        rodrigues_sc(vscale(1.0 / wn, om), sin(wn * dt), cos(wn * dt), Rw);
        mulMM(Rw, s->rot, Rn);
        memcpy(s->rot, Rn, sizeof(Rn));
    }
    return nr;
}

/* ---- the reference's Python side (abd.WalkerEnv) ------------------------------------------------------------------- */
static double calc_state(const wo_model *m, const wo_params *prm, wo_env *e, float *obs, int *at_limit, int *finite) {
    kin_t k;
    kinematics(m, &e->s, &k, 0);
    const int nj = NJ, nf = m->nf;
    int lim = 0, fin = 1;
    for (int j = 0; j < nj; ++j) {
        const double lo = t_joint_lo(m)[j], hi = t_joint_hi(m)[j];
        FL(F_ADD, 3); FL(F_MUL, 3); FL(F_DIV, 1);
        const float jp = (float)(2 * (e->s.q[j] - 0.5 * (lo + hi)) / (hi - lo)), jv = (float)(0.1 * e->s.qd[j]);
        if (fabsf(jp) > 0.99f) ++lim;
        obs[8 + 2 * j] = jp < -5.0f ? -5.0f : (jp > 5.0f ? 5.0f : jp);
        obs[9 + 2 * j] = jv < -5.0f ? -5.0f : (jv > 5.0f ? 5.0f : jv);
        fin = fin && isfinite(obs[8 + 2 * j]) && isfinite(obs[9 + 2 * j]);      /* the clipped values (walker_base_env.py:46-48) */
    }
    double sx = 0, sy = 0, cnt = e->floor_known ? 1.0 : 0.0;
    for (int b = 0; b < NB; ++b) {       /* mean over robot.parts: the base once, every other body once per hinge (min. 1) */
        int wgt = 1;
        if (b > 0) {
            int c = 0;
            for (int j = 0; j < nj; ++j) c += m->joint_body[j] == b;
            wgt = c > 1 ? c : 1;
        }
        FL(F_FMA, 2); FL(F_ADD, 1);
        sx += wgt * k.o[b].x; sy += wgt * k.o[b].y; cnt += wgt;
    }
    FL(F_DIV, 2);
    const double bx = sx / cnt, by = sy / cnt, z = k.o[0].z;
    const double *R = k.R[0];
    FL(F_TRIG, 8); FL(F_SQRT, 1); FL(F_ADD, 4); FL(F_MUL, 9);
    const double roll = atan2(R[7], R[8]);
    double sp = -R[6];
    sp = sp < -1.0 ? -1.0 : (sp > 1.0 ? 1.0 : sp);
    const double pitch = asin(sp), yaw = atan2(R[3], R[0]);
    const double dx = prm->walk_target_x - bx, dy = prm->walk_target_y - by;
    const double theta = atan2(dy, dx), dist = sqrt(dy * dy + dx * dx);
    const double ang = theta - yaw, c = cos(-yaw), sn = sin(-yaw);
    const double vx = c * e->s.vel[0] - sn * e->s.vel[1], vy = sn * e->s.vel[0] + c * e->s.vel[1], vz = e->s.vel[2];
    if (e->initial_z_unset) { e->initial_z = z; e->initial_z_unset = 0; }
    const float head[8] = {(float)(z - e->initial_z), (float)sin(ang), (float)cos(ang), (float)(0.3 * vx), (float)(0.3 * vy), (float)(0.3 * vz),
                           (float)roll, (float)pitch};
    for (int i = 0; i < 8; ++i) {
        obs[i] = head[i] < -5.0f ? -5.0f : (head[i] > 5.0f ? 5.0f : head[i]);
        fin = fin && isfinite(obs[i]);
    }
    for (int f = 0; f < nf; ++f) obs[8 + 2 * nj + f] = e->feet_contact[f] < -5.0f ? -5.0f : (e->feet_contact[f] > 5.0f ? 5.0f : e->feet_contact[f]);
    *at_limit = lim;
    *finite = fin;
    return dist;
}

void wo_env_reset(const wo_model *m, const wo_params *prm, wo_env *e, const double *joint_noise, float *obs) {
    memset(&e->s, 0, sizeof(e->s));
    for (int i = 0; i < 3; ++i) e->s.pos[i] = t_body_pos(m)[i];
    for (int i = 0; i < 9; ++i) e->s.rot[i] = t_body_rot(m)[i];
    for (int j = 0; j < NJ; ++j) e->s.q[j] = joint_noise ? joint_noise[j] : 0.0;
    e->steps = 0;
    for (int f = 0; f < WO_MAX_FEET; ++f) e->feet_contact[f] = 0.0f;
    e->initial_z_unset = prm->initial_z_from_state;
    e->initial_z = prm->initial_z;
    float tmp[8 + 2 * WO_MAX_JOINTS + WO_MAX_FEET];
    int lim, fin;
    const double dist = calc_state(m, prm, e, obs ? obs : tmp, &lim, &fin);
    e->potential = -dist / (prm->dt * prm->substeps);
    e->floor_known = prm->floor_in_parts;
}

int wo_env_step(const wo_model *m, const wo_params *prm, wo_env *e, const float *action, float *obs, double *reward, double *rewards5) {
    double tau[WO_MAX_JOINTS];
    for (int j = 0; j < NJ; ++j) {
        float a = action[j];
        a = a < -1.0f ? -1.0f : (a > 1.0f ? 1.0f : a);
        FL(F_MUL, 1);
        tau[j] = prm->torque_f32 ? (double)((float)t_motor(m)[j] * a) : t_motor(m)[j] * (double)a;
    }
    unsigned long long touch[2] = {0, 0};
    for (int it = 0; it < prm->substeps; ++it) wo_substep(m, prm, &e->s, tau, touch);
    int lim, fin;
    const double dist = calc_state(m, prm, e, obs, &lim, &fin);          /* carries the PREVIOUS step's feet flags */
    for (int f = 0; f < m->nf; ++f) {
        float c = 0.0f;
        for (int g = 0; g < m->ns; ++g)
            if (((touch[g >> 6] >> (g & 63)) & 1ull) && m->sphere_body[g] == m->foot_body[f]) c = 1.0f;
        e->feet_contact[f] = c;
    }
    const double height = prm->height_f32 ? (double)(obs[0] + (float)e->initial_z) : (double)obs[0] + e->initial_z;
    const double alive = height > prm->alive_z ? prm->alive_bonus : -1.0;
    const double pot = -dist / (prm->dt * prm->substeps), progress = pot - e->potential;
    e->potential = pot;
    const double limit_cost = -0.1 * lim;
    e->steps += 1;
    if (rewards5) { rewards5[0] = alive; rewards5[1] = progress; rewards5[2] = 0.0; rewards5[3] = limit_cost; rewards5[4] = 0.0; }
    *reward = alive + progress + 0.0 + limit_cost + 0.0;
    return (alive < 0) || !fin || e->steps >= prm->max_steps;
}

/* n_envs independent envs (env i runs model task_id[i]), n_steps env steps each, finished episodes restart from zero joint
 * noise: the timed loop of bench.py's C4 cpu_baseline (called from one Python thread per core; ctypes drops the GIL). */
long wo_run(const wo_model *models, const int *task_id, const wo_params *prm, wo_env *envs, int n_envs, int n_steps,
            const float *actions /* [n_action_rows][nj] */, int n_action_rows) {
    long done_steps = 0;
    float obs[8 + 2 * WO_MAX_JOINTS + WO_MAX_FEET];
    double reward;
    for (int t = 0; t < n_steps; ++t)
        for (int i = 0; i < n_envs; ++i) {
            const wo_model *m = models + task_id[i];
            const float *a = actions + (size_t)((t * 31 + i) % n_action_rows) * m->nj;
            if (wo_env_step(m, prm, envs + i, a, obs, &reward, 0)) wo_env_reset(m, prm, envs + i, 0, 0);
            ++done_steps;
        }
    return done_steps;
}

int wo_flops_read(unsigned long long *out6 /* [9] */, int clear) {
#ifdef WO_COUNT_FLOPS
    memcpy(out6, wo_flop_count, sizeof(wo_flop_count));
    if (clear) memset(wo_flop_count, 0, sizeof(wo_flop_count));
    return 1;
#else
    (void)out6; (void)clear;
    return 0;
#endif
}
