// walker.hip — batched MetaLocomotion walker (humanoid / ant) engine for gfx950.
//
// Replaces, for N environments per launch, WalkerBaseEnv.step
// (metagym/metalocomotion/envs/utils/walker_base_env.py:43-82):
//   robot.apply_action        humanoids.py:50-54 / walker_base.py:26-29   (motor torques)
//   scene.global_step         scene_bases.py:45-50 -> pybullet.stepSimulation()   (substep() below)
//   robot.calc_state          walker_base.py:31-64, robot_bases.py:317-332        (observe())
//   alive / progress / limits walker_base_env.py:46-82, walker_base.py:66-82      (finish)
//
// PARITY UNPINNED for the physics: the reference delegates it to PyBullet, which is not in the
// reference tree. substep() is a from-scratch reduced-coordinate multibody step with the
// reference's parameters (4 x 5 ms semi-implicit Euler, 5 PGS iterations, ERP 0.9, g = 9.8,
// friction 0.8 x 0.8): joint-space inertia matrix M(q) from world-frame body Jacobians, bias forces
// from a world-frame Newton-Euler pass, Cholesky solve, then projected Gauss-Seidel over ground
// contacts (normal + 2 friction rows per penetrating collision sphere) and joint-limit rows,
// iterated in velocity space (u += M^-1 J_r^T dlambda). oracle/abd.py is the independent numpy
// restatement it is tested against; both are checked by physical invariants.
//
// Two mappings (mg_walker_params.mapping), float64. Wave (the default): one wavefront per env, work set in LDS, walker_step_wave_kernel
// instantiated per robot shape or dof count (wave_plan picks one). Lane: one lane per env, work set in private memory, walker_step_kernel,
// the cross-check and the route for robots the wave scratch cannot hold. mg_walker_reset runs walker_reset_kernel (lane per env) for both.
//
// This file holds the lane engine and the entry points of the step, the rollout and the reset. The wave engine, the arithmetic
// both mappings share and the host planner are in walker_core.h, which walker_policy.hip and walker_rpolicy.hip include too.
#include "walker_core.h"

// As in walker_core.h (said again, so that this file's contraction does not hang on how the header ends): the engine is
// compared with its oracle to a tolerance, so the compiler may fuse a*b+c.
#pragma clang fp contract(fast)

namespace {

constexpr int WK_BLOCK = 64;
constexpr int MAXC = 12;            // contacts the solver keeps per env: the MAXC deepest of the candidates
constexpr int LANE_MAXCAND = 48;    // = W_MAXCAND of walker_core.h: contact candidates recorded per sub-step before the selection
constexpr int MAXR = 3 * MAXC + NJ; // max constraint rows

struct ModelRef {   // offsets into one task's table row
    const double *body_pos, *body_rot, *body_mass, *body_com, *body_inertia;
    const double *joint_anchor, *joint_axis, *joint_lo, *joint_hi, *joint_arm, *joint_damp, *joint_stiff, *motor;
    const double *sph_pos, *sph_r;
    const double *geom_p0, *geom_p1, *geom_r;
    const double *sph_margin;     // per-proxy contact margins, behind geom_r in rows that carry them
};

__device__ __forceinline__ ModelRef model_ref(const mg_walker_topology &tp, const mg_walker_models &ms, int task) {
    const double *p = ms.table + (size_t)task * ms.model_stride;
    const int nb = tp.n_bodies, nj = tp.n_joints, ns = tp.n_spheres;
    ModelRef r;
    r.body_pos = p; p += 3 * nb;
    r.body_rot = p; p += 9 * nb;
    r.body_mass = p; p += nb;
    r.body_com = p; p += 3 * nb;
    r.body_inertia = p; p += 9 * nb;
    r.joint_anchor = p; p += 3 * nj;
    r.joint_axis = p; p += 3 * nj;
    r.joint_lo = p; p += nj;
    r.joint_hi = p; p += nj;
    r.joint_arm = p; p += nj;
    r.joint_damp = p; p += nj;
    r.joint_stiff = p; p += nj;
    r.motor = p; p += nj;
    r.sph_pos = p; p += 3 * ns;
    r.sph_r = p; p += ns;
    r.geom_p0 = p; p += 3 * tp.n_geoms;
    r.geom_p1 = p; p += 3 * tp.n_geoms;
    r.geom_r = p; p += tp.n_geoms;
    r.sph_margin = p;             // (only read when mg_walker_params.sphere_margin_in_table says the rows carry them)
    return r;
}

// Rodrigues rotation matrix about unit axis k by angle t
__device__ __forceinline__ void rodrigues(V3 k, double t, double *R) {
    const double s = sin(t), c = cos(t), v = 1.0 - c;
    R[0] = c + k.x * k.x * v;       R[1] = k.x * k.y * v - k.z * s; R[2] = k.x * k.z * v + k.y * s;
    R[3] = k.y * k.x * v + k.z * s; R[4] = c + k.y * k.y * v;       R[5] = k.y * k.z * v - k.x * s;
    R[6] = k.z * k.x * v - k.y * s; R[7] = k.z * k.y * v + k.x * s; R[8] = c + k.z * k.z * v;
}

struct Env {   // per-lane simulation state
    V3 pos, vel, omega;
    double rot[9];
    double q[NJ], qd[NJ];
};

struct Kin {   // world-frame kinematics of the current configuration
    double R[NB][9];
    V3 o[NB], c[NB];
    V3 p[NJ], a[NJ];
    unsigned mask[NB];   // joints between the base and body b (bit j)
};

__device__ void kinematics(const mg_walker_topology &tp, const ModelRef &m, const Env &s, Kin &k) {
    const int nb = tp.n_bodies, nj = tp.n_joints;
    int j = 0;
    for (int b = 0; b < nb; ++b) {
        double Rc[9];
        V3 oc;
        unsigned mk = 0;
        const int pb = tp.body_parent[b];
        if (pb < 0) {
            for (int i = 0; i < 9; ++i) Rc[i] = s.rot[i];
            oc = s.pos;
        } else {
            mulMM(k.R[pb], m.body_rot + 9 * b, Rc);
            oc = k.o[pb] + mulMv(k.R[pb], ld3(m.body_pos + 3 * b));
            mk = k.mask[pb];
        }
        for (; j < nj && tp.joint_body[j] == b; ++j) {
            const V3 anchor = ld3(m.joint_anchor + 3 * j), axis = ld3(m.joint_axis + 3 * j);
            k.p[j] = oc + mulMv(Rc, anchor);
            k.a[j] = mulMv(Rc, axis);
            double Rj[9], Rn[9];
            rodrigues(axis, s.q[j], Rj);
            mulMM(Rc, Rj, Rn);
            oc = k.p[j] - mulMv(Rn, anchor);
            for (int i = 0; i < 9; ++i) Rc[i] = Rn[i];
            mk |= 1u << j;
        }
        for (int i = 0; i < 9; ++i) k.R[b][i] = Rc[i];
        k.o[b] = oc;
        k.c[b] = oc + mulMv(Rc, ld3(m.body_com + 3 * b));
        k.mask[b] = mk;
    }
}

// column `d` of the Jacobian of point x on a body with joint mask `mk`: velocity of x per unit u_d
__device__ __forceinline__ V3 jac_lin(const Kin &k, unsigned mk, V3 x, int d) {
    if (d < 3) return V3{d == 0 ? 1.0 : 0.0, d == 1 ? 1.0 : 0.0, d == 2 ? 1.0 : 0.0};
    if (d < 6) {
        const V3 e{d == 3 ? 1.0 : 0.0, d == 4 ? 1.0 : 0.0, d == 5 ? 1.0 : 0.0};
        return cross(e, x - k.o[0]);
    }
    const int j = d - 6;
    if (!((mk >> j) & 1u)) return V3{0, 0, 0};
    return cross(k.a[j], x - k.p[j]);
}
__device__ __forceinline__ V3 jac_ang(const Kin &k, unsigned mk, int d) {
    if (d < 3) return V3{0, 0, 0};
    if (d < 6) return V3{d == 3 ? 1.0 : 0.0, d == 4 ? 1.0 : 0.0, d == 5 ? 1.0 : 0.0};
    const int j = d - 6;
    if (!((mk >> j) & 1u)) return V3{0, 0, 0};
    return k.a[j];
}

// M (lower triangle, row-major n x n) and bias h, Featherstone RBDA ch. 3/6 written with world-frame
// Jacobians: M = sum_b m Jv^T Jv + Jw^T I Jw (+ armature), h = sum_b Jv^T m (a_c - g) + Jw^T (I alpha + w x I w)
// where (alpha, a_c) are the velocity-product accelerations (du/dt = 0).
__device__ void mass_and_bias(const mg_walker_topology &tp, const ModelRef &m, const Env &s, const Kin &k,
                              double gravity, double k_lin, double k_ang, double *M, double *h, int n) {
    const int nb = tp.n_bodies, nj = tp.n_joints;
    for (int i = 0; i < n * n; ++i) M[i] = 0.0;
    for (int i = 0; i < n; ++i) h[i] = 0.0;
    V3 fw[NB], fal[NB], fxr[NB], far_[NB];   // frame after each body's joints: w, alpha, ref point, its accel
    int j = 0;
    for (int b = 0; b < nb; ++b) {
        V3 w, al, xr, ar;
        const int pb = tp.body_parent[b];
        if (pb < 0) { w = s.omega; al = v3(0, 0, 0); xr = k.o[0]; ar = v3(0, 0, 0); }
        else { w = fw[pb]; al = fal[pb]; xr = fxr[pb]; ar = far_[pb]; }
        for (; j < nj && tp.joint_body[j] == b; ++j) {
            const V3 r = k.p[j] - xr;
            ar = ar + cross(al, r) + cross(w, cross(w, r));
            xr = k.p[j];
            const V3 wj = s.qd[j] * k.a[j];
            al = al + cross(w, wj);
            w = w + wj;
        }
        fw[b] = w; fal[b] = al; fxr[b] = xr; far_[b] = ar;
        const V3 r = k.c[b] - xr;
        const V3 a_c = ar + cross(al, r) + cross(w, cross(w, r));
        // world inertia Iw = R I R^T
        double RI[9], Iw[9], Rt[9];
        mulMM(k.R[b], m.body_inertia + 9 * b, RI);
        for (int r0 = 0; r0 < 3; ++r0)
            for (int c0 = 0; c0 < 3; ++c0) Rt[3 * r0 + c0] = k.R[b][3 * c0 + r0];
        mulMM(RI, Rt, Iw);
        const double mass = m.body_mass[b];
        V3 F = mass * (a_c - v3(0, 0, -gravity));
        const V3 Iw_w = mulMv(Iw, w);
        V3 Nn = mulMv(Iw, al) + cross(w, Iw_w);
        const unsigned mk = k.mask[b];
        if (k_lin != 0.0 || k_ang != 0.0) {
            // btMultiBody's velocity damping (mg_walker_params.body_*_damping): force -m v_c (k + k |v_c|) at the centre of mass,
            // torque -I w (k + k |w|); their negatives join the bias wrench. v_c = Jv(c_b) u.
            V3 vc = s.vel + cross(s.omega, k.c[b] - k.o[0]);
            for (int jj = 0; jj < nj; ++jj)
                if ((mk >> jj) & 1u) vc = vc + s.qd[jj] * cross(k.a[jj], k.c[b] - k.p[jj]);
            F = F + (mass * (k_lin + k_lin * sqrt(dot(vc, vc)))) * vc;
            Nn = Nn + (k_ang + k_ang * sqrt(dot(w, w))) * Iw_w;
        }
        for (int d = 0; d < n; ++d) {
            if (d >= 6 && !((mk >> (d - 6)) & 1u)) continue;
            const V3 jv = jac_lin(k, mk, k.c[b], d), jw = jac_ang(k, mk, d);
            h[d] += dot(jv, F) + dot(jw, Nn);
            const V3 mjv = mass * jv, Ijw = mulMv(Iw, jw);
            for (int e = 0; e <= d; ++e) {
                if (e >= 6 && !((mk >> (e - 6)) & 1u)) continue;
                const V3 ev = jac_lin(k, mk, k.c[b], e), ew = jac_ang(k, mk, e);
                M[d * n + e] += dot(mjv, ev) + dot(Ijw, ew);
            }
        }
    }
    for (int jj = 0; jj < nj; ++jj) M[(6 + jj) * n + 6 + jj] += m.joint_arm[jj];
}

// in-place Cholesky of the lower triangle: M = L L^T
__device__ void cholesky(double *M, int n) {
    for (int c = 0; c < n; ++c) {
        double d = M[c * n + c];
        for (int k = 0; k < c; ++k) d -= M[c * n + k] * M[c * n + k];
        d = sqrt(d);
        M[c * n + c] = d;
        const double inv = 1.0 / d;
        for (int r = c + 1; r < n; ++r) {
            double v = M[r * n + c];
            for (int k = 0; k < c; ++k) v -= M[r * n + k] * M[c * n + k];
            M[r * n + c] = v * inv;
        }
    }
}
__device__ void chol_solve(const double *L, int n, double *x) {   // x <- (L L^T)^-1 x
    for (int r = 0; r < n; ++r) {
        double v = x[r];
        for (int k = 0; k < r; ++k) v -= L[r * n + k] * x[k];
        x[r] = v / L[r * n + r];
    }
    for (int r = n - 1; r >= 0; --r) {
        double v = x[r];
        for (int k = r + 1; k < n; ++k) v -= L[k * n + r] * x[k];
        x[r] = v / L[r * n + r];
    }
}

// One physics sub-step. touch[g] = 1 for collision spheres in contact this sub-step.
__device__ void substep(const mg_walker_topology &tp, const ModelRef &m, const mg_walker_params &prm, Env &s,
                        const double *tau_motor, unsigned long long &touch_mask) {
    const int nj = tp.n_joints, ns = tp.n_spheres, n = 6 + nj;
    const double dt = prm.time_step;
    Kin k;
    kinematics(tp, m, s, k);
    double M[ND * ND], h[ND], u[ND];
    mass_and_bias(tp, m, s, k, prm.gravity, prm.body_linear_damping, prm.body_angular_damping, M, h, n);
    cholesky(M, n);
    // free motion: u* = u + dt M^-1 (tau - h); explicit damping / spring torques like the oracle
    double rhs[ND];
    for (int d = 0; d < 6; ++d) rhs[d] = -h[d];
    for (int j = 0; j < nj; ++j)
        rhs[6 + j] = tau_motor[j] - m.joint_damp[j] * s.qd[j] - m.joint_stiff[j] * s.q[j] - h[6 + j];
    chol_solve(M, n, rhs);
    u[0] = s.vel.x; u[1] = s.vel.y; u[2] = s.vel.z;
    u[3] = s.omega.x; u[4] = s.omega.y; u[5] = s.omega.z;
    for (int j = 0; j < nj; ++j) u[6 + j] = s.qd[j];
    for (int d = 0; d < n; ++d) u[d] += dt * rhs[d];

    // ---- constraint rows ---------------------------------------------------------------------
    double J[MAXR][ND], W[MAXR][ND];   // W_r = M^-1 J_r^T
    double bias[MAXR], diag[MAXR], lam[MAXR];
    int kind[MAXR], partner[MAXR];
    // contact candidates in candidate order (ground per proxy, then self pairs; at most W_MAXCAND), then the MAXC deepest of them
    // in candidate order — the wave kernel's two steps (and oracle/abd.py contact_candidates / select_contacts), serially
    int nr = 0;
    touch_mask = 0ull;
    double qx[LANE_MAXCAND][6], qdepth[LANE_MAXCAND];
    int qid[LANE_MAXCAND][2];
    int ncand = 0;
    for (int g = 0; g < ns; ++g) {
        const int b = tp.sphere_body[g];
        const V3 x = k.o[b] + mulMv(k.R[b], ld3(m.sph_pos + 3 * g));
        const double depth = m.sph_r[g] - x.z;
        if (depth > -(prm.sphere_margin_in_table ? m.sph_margin[g] : prm.contact_margin)) {
            touch_mask |= 1ull << g;                   // every proxy inside the margin: what getContactPoints reports
            if (ncand < LANE_MAXCAND) {
                qx[ncand][0] = x.x; qx[ncand][1] = x.y; qx[ncand][2] = 0.0;
                qid[ncand][0] = g; qid[ncand][1] = -1; qdepth[ncand] = depth;
                ++ncand;
            }
        }
    }
    if (prm.self_collision)
        for (int pr = 0; pr < tp.n_pairs && ncand < LANE_MAXCAND; ++pr) {
            const int ga = tp.pair_a[pr], gb = tp.pair_b[pr], ba = tp.geom_body[ga], bb = tp.geom_body[gb];
            V3 ca, cb;
            segment_closest(k.o[ba] + mulMv(k.R[ba], ld3(m.geom_p0 + 3 * ga)), k.o[ba] + mulMv(k.R[ba], ld3(m.geom_p1 + 3 * ga)),
                            k.o[bb] + mulMv(k.R[bb], ld3(m.geom_p0 + 3 * gb)), k.o[bb] + mulMv(k.R[bb], ld3(m.geom_p1 + 3 * gb)),
                            ca, cb);
            const V3 dv = ca - cb;
            const double dist = sqrt(dot(dv, dv)), depth = m.geom_r[ga] + m.geom_r[gb] - dist;
            if (depth > 0.0 && dist > 1e-9) {
                const V3 nrm = (1.0 / dist) * dv;
                const V3 xc = 0.5 * ((ca - m.geom_r[ga] * nrm) + (cb + m.geom_r[gb] * nrm));
                qx[ncand][0] = xc.x; qx[ncand][1] = xc.y; qx[ncand][2] = xc.z; qx[ncand][3] = nrm.x; qx[ncand][4] = nrm.y; qx[ncand][5] = nrm.z;
                qid[ncand][0] = ba; qid[ncand][1] = bb; qdepth[ncand] = depth;
                ++ncand;
            }
        }
    for (int c = 0; c < ncand; ++c) {
        if (ncand > MAXC) {
            int rank = 0;
            const double kc = floor(qdepth[c] * 1048576.0);      // (depths on a 2^-20 m grid: see the wave kernel's selection)
            for (int o = 0; o < ncand; ++o) { const double ko = floor(qdepth[o] * 1048576.0); rank += (ko > kc || (ko == kc && o < c)) ? 1 : 0; }
            if (rank >= MAXC) continue;
        }
        const V3 xc{qx[c][0], qx[c][1], qx[c][2]};
        const double depth = qdepth[c];
        if (qid[c][1] == -1) {                         // ground: point on the plane under the proxy
            const unsigned mk = k.mask[tp.sphere_body[qid[c][0]]];
            for (int d = 0; d < n; ++d) {
                const V3 jc = jac_lin(k, mk, xc, d);
                J[nr][d] = jc.z;
                J[nr + 1][d] = jc.x;
                J[nr + 2][d] = jc.y;
            }
        } else {
            const V3 nrm{qx[c][3], qx[c][4], qx[c][5]};
            const int ba = qid[c][0], bb = qid[c][1];
            V3 t1, t2;
            tangent_basis(nrm, t1, t2);
            for (int d = 0; d < n; ++d) {
                const V3 jd = jac_lin(k, k.mask[ba], xc, d) - jac_lin(k, k.mask[bb], xc, d);
                J[nr][d] = dot(nrm, jd);
                J[nr + 1][d] = dot(t1, jd);
                J[nr + 2][d] = dot(t2, jd);
            }
        }
        const int fk = qid[c][1] == -1 ? 1 : 3;
        bias[nr] = (depth >= 0.0 ? prm.erp * depth : depth) / dt; kind[nr] = 0; partner[nr] = -1;
        bias[nr + 1] = 0.0; kind[nr + 1] = fk; partner[nr + 1] = nr;
        bias[nr + 2] = 0.0; kind[nr + 2] = fk == 1 ? 2 : 3; partner[nr + 2] = nr;
        nr += 3;
    }
    for (int j = 0; j < nj; ++j) {
        double sgn = 0.0, viol = 0.0;
        if (s.q[j] < m.joint_lo[j]) { sgn = 1.0; viol = m.joint_lo[j] - s.q[j]; }
        else if (s.q[j] > m.joint_hi[j]) { sgn = -1.0; viol = s.q[j] - m.joint_hi[j]; }
        if (sgn != 0.0) {
            for (int d = 0; d < n; ++d) J[nr][d] = 0.0;
            J[nr][6 + j] = sgn;
            bias[nr] = prm.limit_erp * viol / dt; kind[nr] = 0; partner[nr] = -1;
            ++nr;
        }
    }
    for (int r = 0; r < nr; ++r) {
        for (int d = 0; d < n; ++d) W[r][d] = J[r][d];
        chol_solve(M, n, W[r]);
        double dd = 0.0;
        for (int d = 0; d < n; ++d) dd += J[r][d] * W[r][d];
        diag[r] = dd;
        lam[r] = 0.0;
    }
    // projected Gauss-Seidel in velocity space: identical iterates to PGS on A = J M^-1 J^T
    for (int it = 0; it < prm.solver_iterations; ++it)
        for (int r = 0; r < nr; ++r) {
            if (!(diag[r] > 0.0)) continue;
            double jv = 0.0;
            for (int d = 0; d < n; ++d) jv += J[r][d] * u[d];
            double x = lam[r] - (jv - bias[r]) / diag[r];
            if (kind[r] == 0) x = x > 0.0 ? x : 0.0;
            else {
                const double lim = (kind[r] == 3 ? prm.self_friction : prm.friction) * lam[partner[r]];
                x = x < -lim ? -lim : (x > lim ? lim : x);
            }
            const double dl = x - lam[r];
            lam[r] = x;
            for (int d = 0; d < n; ++d) u[d] += W[r][d] * dl;
        }
    // ---- integrate ------------------------------------------------------------------------------
    if (prm.max_coordinate_velocity > 0.0)        // btMultiBody::applyDeltaVeeMultiDof's clamp (mg_walker_params.max_coordinate_velocity)
        for (int d = 0; d < n; ++d) u[d] = clamp_keep_nan(u[d], prm.max_coordinate_velocity);
    s.vel = v3(u[0], u[1], u[2]);
    s.omega = v3(u[3], u[4], u[5]);
    for (int j = 0; j < nj; ++j) { s.qd[j] = u[6 + j]; s.q[j] += dt * s.qd[j]; }
    s.pos = s.pos + dt * s.vel;
    const double wn = sqrt(dot(s.omega, s.omega));
    if (wn * dt > 0.0) {
        double Rw[9], Rn[9];
        rodrigues((1.0 / wn) * s.omega, wn * dt, Rw);
        mulMM(Rw, s.rot, Rn);
        for (int i = 0; i < 9; ++i) s.rot[i] = Rn[i];
    }
}

// ---- state I/O ---------------------------------------------------------------------------------------

__device__ void load_env(const mg_walker_state &st, int n_envs, int nj, int e, Env &s) {
    s.pos = v3(st.pos[e], st.pos[n_envs + e], st.pos[2 * (size_t)n_envs + e]);
    s.vel = v3(st.vel[e], st.vel[n_envs + e], st.vel[2 * (size_t)n_envs + e]);
    s.omega = v3(st.omega[e], st.omega[n_envs + e], st.omega[2 * (size_t)n_envs + e]);
    for (int i = 0; i < 9; ++i) s.rot[i] = st.rot[(size_t)i * n_envs + e];
    for (int j = 0; j < nj; ++j) { s.q[j] = st.q[(size_t)j * n_envs + e]; s.qd[j] = st.qd[(size_t)j * n_envs + e]; }
}
__device__ void store_env(const mg_walker_state &st, int n_envs, int nj, int e, const Env &s) {
    st.pos[e] = s.pos.x; st.pos[n_envs + e] = s.pos.y; st.pos[2 * (size_t)n_envs + e] = s.pos.z;
    st.vel[e] = s.vel.x; st.vel[n_envs + e] = s.vel.y; st.vel[2 * (size_t)n_envs + e] = s.vel.z;
    st.omega[e] = s.omega.x; st.omega[n_envs + e] = s.omega.y; st.omega[2 * (size_t)n_envs + e] = s.omega.z;
    for (int i = 0; i < 9; ++i) st.rot[(size_t)i * n_envs + e] = s.rot[i];
    for (int j = 0; j < nj; ++j) { st.q[(size_t)j * n_envs + e] = s.q[j]; st.qd[(size_t)j * n_envs + e] = s.qd[j]; }
}

// WalkerBase.calc_state walker_base.py:31-64. Returns walk_target_dist and joints_at_limit.
__device__ void observe(const mg_walker_topology &tp, const ModelRef &m, const mg_walker_params &prm, const Env &s,
                        const float *feet_contact, float *obs, double &target_dist, int &at_limit) {
    const int nb = tp.n_bodies, nj = tp.n_joints, nf = tp.n_feet;
    Kin k;
    kinematics(tp, m, s, k);
    double sx = 0.0, sy = 0.0;
    int parts = prm.floor_in_parts ? 1 : 0;                           // the floor link sits at the origin
    for (int b = 0; b < nb; ++b) {
        const int w = part_weight(tp, b);
        sx += w * k.o[b].x; sy += w * k.o[b].y;
        parts += w;
    }
    const double cnt = (double)parts;
    const double bx = sx / cnt, by = sy / cnt, z = k.o[0].z;
    const double *R = k.R[0];
    const double roll = atan2(R[7], R[8]);
    double sp = -R[6];
    sp = sp < -1.0 ? -1.0 : (sp > 1.0 ? 1.0 : sp);
    const double pitch = asin(sp);
    const double yaw = atan2(R[3], R[0]);
    const double theta = atan2(prm.walk_target_y - by, prm.walk_target_x - bx);
    const double dx = prm.walk_target_x - bx, dy = prm.walk_target_y - by;
    target_dist = sqrt(dy * dy + dx * dx);
    const double ang = theta - yaw;
    const double c = cos(-yaw), sn = sin(-yaw);
    const double vx = c * s.vel.x - sn * s.vel.y, vy = sn * s.vel.x + c * s.vel.y, vz = s.vel.z;
    auto clip5 = [](float v) { return v < -5.0f ? -5.0f : (v > 5.0f ? 5.0f : v); };
    obs[0] = clip5((float)(z - prm.initial_z));
    obs[1] = clip5((float)sin(ang));
    obs[2] = clip5((float)cos(ang));
    obs[3] = clip5((float)(0.3 * vx));
    obs[4] = clip5((float)(0.3 * vy));
    obs[5] = clip5((float)(0.3 * vz));
    obs[6] = clip5((float)roll);
    obs[7] = clip5((float)pitch);
    at_limit = 0;
    for (int j = 0; j < nj; ++j) {
        const double lo = m.joint_lo[j], hi = m.joint_hi[j];
        const float p = (float)(2 * (s.q[j] - 0.5 * (lo + hi)) / (hi - lo));   // robot_bases.py:317-323
        const float v = (float)(0.1 * s.qd[j]);                               // :327-328
        if (fabsf(p) > 0.99f) ++at_limit;
        obs[8 + 2 * j] = clip5(p);
        obs[9 + 2 * j] = clip5(v);
    }
    for (int f = 0; f < nf; ++f) obs[8 + 2 * nj + f] = clip5(feet_contact[f]);
}

__global__ __launch_bounds__(WK_BLOCK) void walker_step_kernel(mg_walker_topology tp, mg_walker_models ms,
                                                               mg_walker_params prm, mg_walker_state st, int n_envs,
                                                               const float *action, float *obs, float *reward,
                                                               float *rewards5, uint8_t *done) {
    const int e = blockIdx.x * WK_BLOCK + threadIdx.x;
    if (e >= n_envs) return;
    const int nj = tp.n_joints, nf = tp.n_feet, obs_dim = 8 + 2 * nj + nf;
    const ModelRef m = model_ref(tp, ms, st.task_id[e]);
    Env s;
    load_env(st, n_envs, nj, e, s);
    double tau[NJ];
    for (int j = 0; j < nj; ++j) {
        tau[j] = motor_torque(prm, m.motor[j], action[(size_t)e * nj + j]);
    }
    unsigned long long touch = 0ull;
    for (int it = 0; it < prm.frame_skip; ++it) substep(tp, m, prm, s, tau, touch);   // scene_bases.py:45-50
    // calc_state runs before the feet flags are refreshed (walker_base_env.py:46 vs :57-63)
    float fc[MG_WALKER_MAX_FEET];
    for (int f = 0; f < nf; ++f) fc[f] = st.feet_contact[(size_t)f * n_envs + e];
    float ob[8 + 2 * NJ + MG_WALKER_MAX_FEET];
    double dist;
    int at_limit;
    observe(tp, m, prm, s, fc, ob, dist, at_limit);
    for (int f = 0; f < nf; ++f) {        // which flag a proxy reports to: mg_walker_topology.sphere_foot, like the wave kernels
        float c = 0.0f;
        for (int g = 0; g < tp.n_spheres; ++g)
            if (((touch >> g) & 1ull) && tp.sphere_foot[g] == f) c = 1.0f;
        st.feet_contact[(size_t)f * n_envs + e] = c;
    }
    if (st.bad_contacts != nullptr) {     // a1.py:314-323 GetBadFootContacts: contact points on links that are no foot
        int bad = 0;
        for (int g = 0; g < tp.n_spheres; ++g) bad += (((touch >> g) & 1ull) && tp.sphere_foot[g] < 0) ? 1 : 0;
        st.bad_contacts[e] = bad;
    }
    const double alive = (alive_height(prm, ob[0]) > prm.alive_z) ? prm.alive_bonus : prm.dead_bonus;   // :47
    bool finite = true;
    for (int i = 0; i < obs_dim; ++i) finite = finite && isfinite(ob[i]);
    const double pot_old = st.potential[e];
    const double pot = -dist / (prm.time_step * prm.frame_skip);        // walker_base.py:66-82
    const double progress = pot - pot_old;
    const double limit_cost = prm.joints_at_limit_cost * at_limit;
    st.potential[e] = pot;
    const int steps = st.steps[e] + 1;
    st.steps[e] = steps;
    const bool d = (alive < 0) || !finite || (steps >= prm.max_steps);
    if (prm.auto_reset && d) {
        // vector-env convention: the returned obs is the first observation of the next episode
        s.pos = ld3(m.body_pos);
        for (int i = 0; i < 9; ++i) s.rot[i] = m.body_rot[i];
        s.vel = v3(0, 0, 0);
        s.omega = v3(0, 0, 0);
        for (int j = 0; j < nj; ++j) { s.q[j] = reset_joint_noise(prm, prm.step_index, e, j); s.qd[j] = 0.0; }
        for (int f = 0; f < nf; ++f) { fc[f] = 0.0f; st.feet_contact[(size_t)f * n_envs + e] = 0.0f; }
        observe(tp, m, prm, s, fc, ob, dist, at_limit);
        st.potential[e] = -dist / (prm.time_step * prm.frame_skip);
        st.steps[e] = 0;
    }
    for (int i = 0; i < obs_dim; ++i) obs[(size_t)e * obs_dim + i] = ob[i];
    reward[e] = (float)(alive + progress + 0.0 + limit_cost + 0.0);      // :69-77
    if (rewards5) {
        float *r5 = rewards5 + (size_t)e * 5;
        r5[0] = (float)alive; r5[1] = (float)progress; r5[2] = 0.0f; r5[3] = (float)limit_cost; r5[4] = 0.0f;
    }
    done[e] = (uint8_t)d;
    store_env(st, n_envs, nj, e, s);
}

__global__ __launch_bounds__(WK_BLOCK) void walker_reset_kernel(mg_walker_topology tp, mg_walker_models ms,
                                                                mg_walker_params prm, mg_walker_state st, int n_envs,
                                                                const uint8_t *mask, const double *joint_noise,
                                                                float *obs) {
    const int e = blockIdx.x * WK_BLOCK + threadIdx.x;
    if (e >= n_envs) return;
    if (mask != nullptr && mask[e] == 0) return;
    const int nj = tp.n_joints, nf = tp.n_feet, obs_dim = 8 + 2 * nj + nf;
    const ModelRef m = model_ref(tp, ms, st.task_id[e]);
    Env s;
    s.pos = ld3(m.body_pos);
    for (int i = 0; i < 9; ++i) s.rot[i] = m.body_rot[i];
    if (prm.reset_pos != nullptr)       // the caller's start pose (mg_walker_params.reset_pos / reset_rot)
        s.pos = v3(prm.reset_pos[e], prm.reset_pos[(size_t)n_envs + e], prm.reset_pos[2 * (size_t)n_envs + e]);
    if (prm.reset_rot != nullptr)
        for (int i = 0; i < 9; ++i) s.rot[i] = prm.reset_rot[(size_t)i * n_envs + e];
    s.vel = v3(0, 0, 0);
    s.omega = v3(0, 0, 0);
    for (int j = 0; j < nj; ++j) {
        s.q[j] = joint_noise ? joint_noise[(size_t)j * n_envs + e] : 0.0;   // walker_base.py:15
        s.qd[j] = 0.0;
    }
    float fc[MG_WALKER_MAX_FEET];
    for (int f = 0; f < nf; ++f) { fc[f] = 0.0f; st.feet_contact[(size_t)f * n_envs + e] = 0.0f; }
    if (prm.reset_pos != nullptr || prm.reset_rot != nullptr) {            // a robot placed by its caller: no contact points yet
        if (st.bad_contacts != nullptr) st.bad_contacts[e] = 0;
        if (st.foot_force != nullptr)
            for (int f = 0; f < nf; ++f) st.foot_force[(size_t)f * n_envs + e] = 0.0;
    }
    float ob[8 + 2 * NJ + MG_WALKER_MAX_FEET];
    double dist;
    int at_limit;
    observe(tp, m, prm, s, fc, ob, dist, at_limit);
    st.potential[e] = -dist / (prm.time_step * prm.frame_skip);
    st.steps[e] = 0;
    if (obs)
        for (int i = 0; i < obs_dim; ++i) obs[(size_t)e * obs_dim + i] = ob[i];
    store_env(st, n_envs, nj, e, s);
}

}  // namespace

#ifdef MG_WALKER_PROFILE
extern "C" int mg_walker_profile_read(unsigned long long *out16, int clear) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(mg_walker_phase_cycles), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (clear) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(mg_walker_phase_cycles), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

extern "C" int mg_walker_reset(const mg_walker_topology *tp, const mg_walker_models *ms, const mg_walker_params *prm,
                               int32_t n, const mg_walker_state *st, const uint8_t *mask, const double *joint_noise,
                               float *obs, void *stream) {
    if (int rc = check_walker(tp, ms, prm, st, n)) return rc;
    mg::DeviceGuard guard(mg::device_of(st->pos));
    hipLaunchKernelGGL(walker_reset_kernel, dim3((n + WK_BLOCK - 1) / WK_BLOCK), dim3(WK_BLOCK), 0, (hipStream_t)stream,
                       *tp, *ms, *prm, *st, n, mask, joint_noise, obs);
    return mg::check_launch("walker_reset_kernel");
}

extern "C" int mg_walker_step(const mg_walker_topology *tp, const mg_walker_models *ms, const mg_walker_params *prm,
                              int32_t n, const mg_walker_state *st, const float *action, float *obs, float *reward,
                              float *rewards5, uint8_t *done, void *stream) {
    if (int rc = check_walker(tp, ms, prm, st, n)) return rc;
    if (prm->actuation == 0) MG_REQUIRE_PTR(action);
    else {
        if (prm->actuation < 1 || prm->actuation > 4) return mg::set_error(MG_ERR_BAD_CONFIG, "walker actuation %d", prm->actuation);
        if (prm->mapping == 0) return mg::set_error(MG_ERR_UNSUPPORTED, "in-launch actuators need the wave mapping");
        MG_REQUIRE_PTR(prm->pd_command);
    }
    if (int rc = check_walker_terrain(prm)) return rc;
    MG_REQUIRE_PTR(obs);
    MG_REQUIRE_PTR(reward);
    MG_REQUIRE_PTR(done);
    mg::DeviceGuard guard(mg::device_of(st->pos));
    if (prm->mapping == 0) {   // lane-per-env reference mapping (private-memory work set)
        if (tp->n_spheres > 64 || prm->sphere_friction != nullptr || st->foot_force != nullptr || prm->ext_wrench != nullptr ||
            prm->gravity_env != nullptr)
            return mg::set_error(MG_ERR_UNSUPPORTED, "per-proxy friction, foot forces, pushes, per-robot gravity and > 64 collision proxies need the wave mapping");
        hipLaunchKernelGGL(walker_step_kernel, dim3((n + WK_BLOCK - 1) / WK_BLOCK), dim3(WK_BLOCK), 0,
                           (hipStream_t)stream, *tp, *ms, *prm, *st, n, action, obs, reward, rewards5, done);
        return mg::check_launch("walker_step_kernel");
    }
    WaveLaunch<WAVE_STEP> w;
    if (int rc = wave_plan(tp, prm, st, &w)) return rc;
    const WavePlanArgs a = pack(w.plan);
    hipLaunchKernelGGL(w.kernel, dim3(n), dim3(WV), w.lds, (hipStream_t)stream, *tp, *ms, *prm, *st, n, a.rows, a.scan, action, obs,
                       reward, rewards5, done, WaveRoll<WAVE_STEP>{});
    return mg::check_launch("walker_step_wave_kernel");
}

extern "C" int mg_walker_rollout(const mg_walker_topology *tp, const mg_walker_models *ms, const mg_walker_params *prm,
                                 int32_t n, const mg_walker_state *st, int32_t n_steps, int32_t obs_every,
                                 const float *actions, float *obs, float *reward, float *rewards5, uint8_t *done,
                                 void *stream) {
    if (int rc = check_walker(tp, ms, prm, st, n)) return rc;
    if (int rc = check_walker_rollout("mg_walker_rollout", prm, n_steps, obs_every, "the in-launch actuators take one pd_command "
                                      "per launch; rollouts run torque actions, actuation = 0"))
        return rc;
    MG_REQUIRE_PTR(actions);
    MG_REQUIRE_PTR(obs);
    MG_REQUIRE_PTR(reward);
    MG_REQUIRE_PTR(done);
    WaveLaunch<WAVE_ROLLOUT> w;
    if (int rc = wave_plan(tp, prm, st, &w)) return rc;
    mg::DeviceGuard guard(mg::device_of(st->pos));
    const WavePlanArgs a = pack(w.plan);
    hipLaunchKernelGGL(w.kernel, dim3(n), dim3(WV), w.lds, (hipStream_t)stream, *tp, *ms, *prm, *st, n, a.rows, a.scan, actions, obs,
                       reward, rewards5, done, WaveRoll<WAVE_ROLLOUT>{n_steps, obs_every});
    return mg::check_launch("walker_step_wave_kernel (rollout)");
}
