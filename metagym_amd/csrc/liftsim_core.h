// liftsim_core.h — the LiftSim family's shared core: the arena layout (Lay, Env), one env.step as a device function
// (step_body and what it calls), the wave's stream refill (refill_streams), Records and the host checks. liftsim.hip,
// liftsim_policy.hip and liftsim_rpolicy.hip include it; each keeps its own copy (anonymous namespace) and defines the
// kernels it launches. The step's order and the mapping are described in liftsim.hip.
#pragma once
#include <cmath>

#include "mg_common.h"
#include "mg_mt19937.h"

namespace {

using mt::MTN;
constexpr int REC = 2 * MTN;   // u32 words of one lane's stream record
constexpr double EPS = 1.0e-2, GRAV = 9.80, MAX_ACC = 1.0, MAX_SPD = 2.0, ENTER_T = 2.0, DOOR_V = 0.5;
constexpr double DOOR_P = 350.0, STANDBY_P = 100.0, MAX_LOAD = 1600.0, RATED = 600.0, NET = 300.0, PULLEY = 0.27;
constexpr double MOTOR_EFF = 0.8, GIVE_UP = 300.0;
constexpr int MPEE = 2, LCAP = MG_LIFTSIM_LOAD_CAP, QN = MG_LIFTSIM_QN;

struct Lay {
    int64_t off[MG_LS_NFIELDS];
    int64_t total;
};

Lay layout(int F, int E, int Q, int W, int64_t n) {
    int64_t sz[MG_LS_NFIELDS];
    const int64_t e8 = 8 * E * n, e4 = 4 * E * n;
    for (int f : {MG_LS_POS, MG_LS_VEL, MG_LS_LOAD, MG_LS_DOOR, MG_LS_KEEP, MG_LS_ALARM, MG_LS_FLOOR}) sz[f] = e8;
    for (int f : {MG_LS_DIR, MG_LS_DISPATCH, MG_LS_DISPATCH_DIR, MG_LS_NTARGET, MG_LS_EFLAGS, MG_LS_NLOADED, MG_LS_NENT,
                  MG_LS_NEXIT})
        sz[f] = e4;
    sz[MG_LS_TARGETS] = e4 * F;
    sz[MG_LS_OPENING] = sz[MG_LS_CLOSING] = E * n;
    sz[MG_LS_CLICKED] = e4 * 4;
    sz[MG_LS_LW] = e8 * LCAP;
    sz[MG_LS_LT] = e4 * LCAP;
    sz[MG_LS_EW] = sz[MG_LS_EL] = sz[MG_LS_XW] = sz[MG_LS_XL] = e8 * 2;
    sz[MG_LS_ET] = e4 * 2;
    sz[MG_LS_QHEAD] = sz[MG_LS_QLEN] = 4 * 2 * F * n;
    sz[MG_LS_QW] = sz[MG_LS_QA] = 8 * 2 * (int64_t)F * Q * n;
    sz[MG_LS_QT] = 4 * 2 * (int64_t)F * Q * n;
    sz[MG_LS_UP] = sz[MG_LS_DOWN] = F * n;
    sz[MG_LS_TIME] = sz[MG_LS_LASTGEN] = 8 * n;
    sz[MG_LS_TIDX] = 4 * n;
    sz[MG_LS_INVALID] = sz[MG_LS_OVERFLOW] = sz[MG_LS_UNSUPPORTED] = n;
    sz[MG_LS_SHEAD] = sz[MG_LS_SCOUNT] = 4 * n;
    sz[MG_LS_SD] = sz[MG_LS_SG] = sz[MG_LS_SA] = 4 * (int64_t)W * n;
    sz[MG_LS_SW] = sz[MG_LS_SE] = 8 * (int64_t)W * n;
    sz[MG_LS_PYKEY] = sz[MG_LS_NPKEY] = 4 * (int64_t)REC * n;
    sz[MG_LS_PYP] = sz[MG_LS_PYV] = sz[MG_LS_NPP] = sz[MG_LS_NPV] = 4 * n;
    sz[MG_LS_REWARD] = sz[MG_LS_TIMEC] = sz[MG_LS_ENERGY] = 8 * n;
    sz[MG_LS_GIVEN] = 4 * n;
    sz[MG_LS_ST_D] = sz[MG_LS_ST_G] = sz[MG_LS_ST_A] = sz[MG_LS_ST_E] = sz[MG_LS_ST_W] = 8 * n;
    sz[MG_LS_RP_HOLDER] = 2 * F * n;
    sz[MG_LS_RP_PRIORITY] = 8 * 2 * F * n;
    Lay l{};
    int64_t o = 0;
    for (int f = 0; f < MG_LS_NFIELDS; ++f) {
        l.off[f] = o;
        o += (sz[f] + 255) / 256 * 256;
    }
    l.total = o;
    return l;
}

struct K {
    int F, E, gen, Q, W, particles, T;
    double h, dt, interval, nv_magic;
    float dt32;
    const double *times, *enlam, *pp, *logq, *qn;
    const float *dens;
    const int32_t *flip;
};

// One lane's view of its env: field accessors over the arena, [item][N] with this env's column.
struct Env {
    uint8_t *a;
    const Lay *l;
    int64_t n;
    int e;

    template <class T> __device__ __forceinline__ T &at(int f, int64_t item) const {
        return reinterpret_cast<T *>(a + l->off[f])[item * n + e];
    }
    __device__ __forceinline__ double &d(int f, int64_t i = 0) const { return at<double>(f, i); }
    __device__ __forceinline__ int32_t &i(int f, int64_t i = 0) const { return at<int32_t>(f, i); }
    __device__ __forceinline__ uint8_t &b(int f, int64_t i = 0) const { return at<uint8_t>(f, i); }
    __device__ __forceinline__ uint32_t *key(int f) const {
        return reinterpret_cast<uint32_t *>(a + l->off[f]) + (size_t)e * REC;
    }
};

// Elevator k's scalars in registers while it runs (elevator.py).
struct Elev {
    double pos, vel, load, door, keep, alarm;
    int dir, dispatch, ddir, opening, closing, entering, unloading;
};

__device__ __forceinline__ bool is_stopped(const Elev &v) { return fabs(v.vel) < EPS; }

__device__ bool valid_target(const K &k, const Elev &v, int f) {
    if (f < 1 || f > k.F) return false;
    const double cf = v.pos / k.h + 1.0;
    if (fabs(cf - (double)f) < EPS && fabs(v.vel) < EPS) return true;
    const double sign = v.vel < 0.0 ? -1.0 : 1.0;
    const double stop = v.pos + sign * (0.5 * v.vel * v.vel / MAX_ACC);
    const double tp = (double)(f - 1) * k.h;
    if (v.dir > 0) return !(tp + 0.5 * EPS < stop);
    if (v.dir < 0) return !(tp > stop + 0.5 * EPS);
    return true;
}

__device__ __forceinline__ double clipv(double a, double m) { return fmax(-m, fmin(m, a)); }

// utils.velocity_planner with max_acc = 1, max_spd = 2
__device__ double plan(double v, double x, double dt, double &eff) {
    const double acc = MAX_ACC, spd = MAX_SPD;
    const double sv = v > 0 ? 1.0 : -1.0;
    eff = dt;
    if (0.1 * EPS > fabs(x)) {
        if (fabs(v) < fabs(acc * dt)) eff = fabs(v) / fabs(acc);
        return v - sv * acc * eff;
    }
    const double sx = x > 0 ? 1.0 : -1.0;
    const double rs = 0.5 * v * fabs(v) / acc + v * dt;
    const double ve = clipv(v + sx * acc * dt, spd);
    const double re = 0.5 * ve * fabs(ve) / acc + 0.5 * (ve + v) * dt;
    if ((sx > 0 && x > re - 0.1 * EPS) || (sx < 0 && x < re + 0.1 * EPS)) return ve;
    if ((sx > 0 && x > rs - 0.1 * EPS) || (sx < 0 && x < rs + 0.1 * EPS)) {
        double fs = 0.0, fe = 1.0, fm = 0.5, out = v;
        for (int it = 0; it < 5; ++it) {
            const double tv = clipv(v + sx * fm * acc * dt, spd);
            const double r = 0.5 * tv * fabs(tv) / acc + 0.5 * (tv + v) * dt;
            if ((x > 0 && x > r) || (x < 0 && x < r)) { fs = fm; out = tv; }
            else fe = fm;
            fm = 0.5 * (fs + fe);
        }
        return out;
    }
    const double ra = clipv(-0.5 * fabs(v * v / x) * sv, acc);
    if (fabs(v) < fabs(ra * dt)) eff = fabs(v) / fabs(ra);
    return v + ra * eff;
}

__device__ int find_target(const Env &s, const K &k, int el, int nt, int f) {
    for (int j = 0; j < nt; ++j)
        if (s.i(MG_LS_TARGETS, (int64_t)el * k.F + j) == f) return j;
    return -1;
}

// delete entry j; the slot vacated at the end goes back to 0, so the list stays 0-padded past its count
__device__ void remove_target(const Env &s, const K &k, int el, int &nt, int j) {
    for (int m = j; m + 1 < nt; ++m)
        s.i(MG_LS_TARGETS, (int64_t)el * k.F + m) = s.i(MG_LS_TARGETS, (int64_t)el * k.F + m + 1);
    --nt;
    s.i(MG_LS_TARGETS, (int64_t)el * k.F + nt) = 0;
}

__device__ __forceinline__ void request_close(Elev &v) {
    if (v.door > EPS && !v.opening && !v.unloading && !v.entering && v.keep < EPS) v.closing = 1;
}

__device__ __forceinline__ Elev load_elev(const Env &s, int el) {
    Elev v;
    v.pos = s.d(MG_LS_POS, el); v.vel = s.d(MG_LS_VEL, el); v.load = s.d(MG_LS_LOAD, el);
    v.door = s.d(MG_LS_DOOR, el); v.keep = s.d(MG_LS_KEEP, el); v.alarm = s.d(MG_LS_ALARM, el);
    v.dir = s.i(MG_LS_DIR, el); v.dispatch = s.i(MG_LS_DISPATCH, el); v.ddir = s.i(MG_LS_DISPATCH_DIR, el);
    v.opening = s.b(MG_LS_OPENING, el); v.closing = s.b(MG_LS_CLOSING, el);
    const int fl = s.i(MG_LS_EFLAGS, el);
    v.entering = fl & 1; v.unloading = (fl >> 1) & 1;
    return v;
}

__device__ __forceinline__ void store_elev(const Env &s, const K &k, int el, const Elev &v) {
    s.d(MG_LS_POS, el) = v.pos; s.d(MG_LS_VEL, el) = v.vel; s.d(MG_LS_LOAD, el) = v.load;
    s.d(MG_LS_DOOR, el) = v.door; s.d(MG_LS_KEEP, el) = v.keep; s.d(MG_LS_ALARM, el) = v.alarm;
    s.i(MG_LS_DIR, el) = v.dir; s.i(MG_LS_DISPATCH, el) = v.dispatch; s.i(MG_LS_DISPATCH_DIR, el) = v.ddir;
    s.b(MG_LS_OPENING, el) = (uint8_t)v.opening; s.b(MG_LS_CLOSING, el) = (uint8_t)v.closing;
    s.i(MG_LS_EFLAGS, el) = v.entering | (v.unloading << 1);
    s.d(MG_LS_FLOOR, el) = v.pos / k.h + 1.0;
}

// Elevator.run_elevator for elevator el: returns its energy; adds its delivered persons and its load count.
__device__ double run_elevator(const Env &s, const K &k, int el, int &delivered, int &loaded_total) {
    Elev v = load_elev(s, el);
    const double dt = k.dt, lag = 2.0 + k.dt;
    int nt = s.i(MG_LS_NTARGET, el);
    const int64_t tb = (int64_t)el * k.F;
    // _get_true_target
    const int first = nt > 0 ? s.i(MG_LS_TARGETS, tb) : 0;
    int tf;
    if (v.alarm > EPS || !valid_target(k, v, v.dispatch)) tf = first;
    else if (nt == 0) tf = v.dispatch;
    else if (v.dir >= 0) tf = v.dispatch < first ? v.dispatch : first;
    else tf = v.dispatch > first ? v.dispatch : first;
    const double offset = tf <= 0 ? 0.0 : (double)(tf - 1) * k.h - v.pos;
    const bool no_reserved = nt < 1;
    if (is_stopped(v) && tf > 0 && fabs(offset) < EPS) {
        if (v.door > 1.0 - EPS) {
            if (tf <= k.F) s.at<uint32_t>(MG_LS_CLICKED, el * 4 + ((tf - 1) >> 5)) &= ~(1u << ((tf - 1) & 31));
            const int j = find_target(s, k, el, nt, tf);
            if (j >= 0) remove_target(s, k, el, nt, j);
            v.dispatch = 0;
        }
        if (is_stopped(v) && v.door < 1.0 - EPS && v.alarm < EPS) { v.opening = 1; v.keep = lag; v.closing = 0; }
    }
    const double digit = v.pos / k.h + 1.0;
    if (no_reserved && is_stopped(v) && v.door < EPS) v.dir = 0;
    if (v.dir == 0 && is_stopped(v) && v.dispatch > 0 && fabs((double)v.dispatch - digit) < EPS &&
        (v.ddir == 1 || v.ddir == -1))
        v.dir = v.ddir;
    if (is_stopped(v) && v.pos <= EPS) v.dir = 1;
    if (is_stopped(v) && v.pos >= (double)(k.F - 1) * k.h - EPS) v.dir = -1;
    if (nt > 0 && v.dir == 0) {
        const double t0 = (double)s.i(MG_LS_TARGETS, tb);
        if (t0 > digit) v.dir = -1;
        else if (t0 < digit) v.dir = 1;
    }
    // clicked buttons missing from the targets: _insert_target keeps the list sorted and deduplicated, so the set's
    // iteration order does not matter; ascending here
    for (int w = 0; w < 4; ++w) {
        uint32_t bits = s.at<uint32_t>(MG_LS_CLICKED, el * 4 + w);
        while (bits) {
            const int f = w * 32 + __builtin_ctz(bits) + 1;
            bits &= bits - 1;
            if (find_target(s, k, el, nt, f) >= 0 || !valid_target(k, v, f)) continue;
            int at = nt;
            for (int j = 0; j < nt; ++j) {
                const int x = s.i(MG_LS_TARGETS, tb + j);
                if ((v.dir >= 0 && x > f) || (v.dir < 0 && x < f)) { at = j; break; }
            }
            for (int j = nt; j > at; --j) s.i(MG_LS_TARGETS, tb + j) = s.i(MG_LS_TARGETS, tb + j - 1);
            s.i(MG_LS_TARGETS, tb + at) = f;
            ++nt;
        }
    }
    if (tf > 0) {
        const double df = (double)tf - 1.0 - v.pos / k.h;
        if (df * (double)v.dir < -EPS) {
            const int j = find_target(s, k, el, nt, tf);
            if (j >= 0) remove_target(s, k, el, nt, j);
        }
    }
    if (fabs(v.vel) > EPS) {
        if (v.opening) v.opening = 0;
        else if (v.door > EPS) v.closing = 1;
    }
    if (v.door < EPS) v.closing = 0;
    else if (v.door > 1.0 - EPS) v.opening = 0;
    int nent = s.i(MG_LS_NENT, el), nexit = s.i(MG_LS_NEXIT, el);
    if (nent > 0 || nexit > 0) {
        v.closing = 0;
        if (v.door < 1.0 - EPS) { v.opening = 1; v.keep = lag; }
    }
    if (v.opening) v.door = fmin(1.0, v.door + DOOR_V);
    else if (v.closing) v.door = fmax(0.0, v.door - DOOR_V);
    const bool hold = v.opening || v.closing || v.door > EPS;
    double eff = dt, nv;
    if (hold) {
        if (fabs(v.vel) < dt * MAX_ACC) { nv = 0.0; eff = fabs(v.vel) / MAX_ACC; }
        else if (v.vel > 0) nv = v.vel - dt * MAX_ACC;
        else nv = v.vel + dt * MAX_ACC;
    } else {
        nv = plan(v.vel, offset, dt, eff);
    }
    v.pos += 0.5 * (nv + v.vel) * eff + nv * (dt - eff);
    const double acc = (nv - v.vel) / fmax(eff, EPS);
    const double f1 = (NET + v.load) * (GRAV + acc);
    const double f2 = RATED * (GRAV - acc);
    const double m = fabs(f1 - f2) * PULLEY / 1.0 / 1.0;
    double energy = m * fabs((v.vel + nv) / 2) / 1.0 * 1.0 / MOTOR_EFF * eff + STANDBY_P * dt;
    v.vel = nv;
    if (v.opening || v.closing) energy += DOOR_P * dt;
    v.alarm = fmax(0.0, v.alarm - dt);
    if (v.door > 1.0 - EPS) v.keep = fmax(0.0, v.keep - dt);
    // unloading: the exiting persons whose time is up leave, highest index first (at most MPEE = 2 of them)
    {
        const double w0 = nexit > 0 ? s.d(MG_LS_XW, el * 2) : 0.0, l0 = nexit > 0 ? s.d(MG_LS_XL, el * 2) - dt : 0.0;
        const double w1 = nexit > 1 ? s.d(MG_LS_XW, el * 2 + 1) : 0.0, l1 = nexit > 1 ? s.d(MG_LS_XL, el * 2 + 1) - dt : 0.0;
        const bool g0 = nexit > 0 && l0 < EPS, g1 = nexit > 1 && l1 < EPS;
        if (g1) { v.load -= w1; ++delivered; }
        if (g0) { v.load -= w0; ++delivered; }
        int keep = 0;
        if (nexit > 0 && !g0) { s.d(MG_LS_XW, el * 2) = w0; s.d(MG_LS_XL, el * 2) = l0; ++keep; }
        if (nexit > 1 && !g1) { s.d(MG_LS_XW, el * 2 + keep) = w1; s.d(MG_LS_XL, el * 2 + keep) = l1; ++keep; }
        nexit = keep;
    }
    const double cf = v.pos / k.h + 1.0;
    const int floor = (int)(cf + 0.5);
    const double dd = (double)floor - cf;
    int nl = s.i(MG_LS_NLOADED, el);
    // loading: the entering persons whose time is up join the loaded list, highest index first
    {
        const double w0 = nent > 0 ? s.d(MG_LS_EW, el * 2) : 0.0, l0 = nent > 0 ? s.d(MG_LS_EL, el * 2) - dt : 0.0;
        const double w1 = nent > 1 ? s.d(MG_LS_EW, el * 2 + 1) : 0.0, l1 = nent > 1 ? s.d(MG_LS_EL, el * 2 + 1) - dt : 0.0;
        const int t0 = nent > 0 ? s.i(MG_LS_ET, el * 2) : 0, t1 = nent > 1 ? s.i(MG_LS_ET, el * 2 + 1) : 0;
        const bool g0 = nent > 0 && l0 < EPS, g1 = nent > 1 && l1 < EPS;
        auto board_in = [&](double w, int t) {
            s.d(MG_LS_LW, (int64_t)el * LCAP + nl) = w;
            s.i(MG_LS_LT, (int64_t)el * LCAP + nl) = t;
            ++nl;
            v.load += w;
            if (t > 0 && t <= k.F) s.at<uint32_t>(MG_LS_CLICKED, el * 4 + ((t - 1) >> 5)) |= 1u << ((t - 1) & 31);
        };
        if (g1) board_in(w1, t1);
        if (g0) board_in(w0, t0);
        int keep = 0;
        if (nent > 0 && !g0) {
            s.d(MG_LS_EW, el * 2) = w0; s.i(MG_LS_ET, el * 2) = t0; s.d(MG_LS_EL, el * 2) = l0; ++keep;
        }
        if (nent > 1 && !g1) {
            s.d(MG_LS_EW, el * 2 + keep) = w1; s.i(MG_LS_ET, el * 2 + keep) = t1; s.d(MG_LS_EL, el * 2 + keep) = l1; ++keep;
        }
        nent = keep;
    }
    // the oldest loaded person for this floor starts to exit
    int at_floor = -1;
    for (int j = 0; j < nl; ++j)
        if (s.i(MG_LS_LT, (int64_t)el * LCAP + j) == floor) { at_floor = j; break; }
    if (is_stopped(v) && v.door > 1.0 - EPS && fabs(dd) < EPS && at_floor >= 0 && nexit < MPEE) {
        s.d(MG_LS_XW, el * 2 + nexit) = s.d(MG_LS_LW, (int64_t)el * LCAP + at_floor);
        s.d(MG_LS_XL, el * 2 + nexit) = ENTER_T;
        ++nexit;
        for (int j = at_floor; j + 1 < nl; ++j) {
            s.d(MG_LS_LW, (int64_t)el * LCAP + j) = s.d(MG_LS_LW, (int64_t)el * LCAP + j + 1);
            s.i(MG_LS_LT, (int64_t)el * LCAP + j) = s.i(MG_LS_LT, (int64_t)el * LCAP + j + 1);
        }
        --nl;
        at_floor = -1;
        for (int j = 0; j < nl; ++j)
            if (s.i(MG_LS_LT, (int64_t)el * LCAP + j) == floor) { at_floor = j; break; }
    }
    v.entering = nent > 0;
    v.unloading = nexit > 0 || at_floor >= 0;
    if (v.door > 1.0 - EPS) request_close(v);
    s.i(MG_LS_NTARGET, el) = nt;
    s.i(MG_LS_NENT, el) = nent;
    s.i(MG_LS_NEXIT, el) = nexit;
    s.i(MG_LS_NLOADED, el) = nl;
    store_elev(s, k, el, v);
    loaded_total += nl;
    return energy;
}

// ---------------------------------------------------------------- draws

// random.normalvariate(50, 10) redrawn until it lies in [20, 100] (custom_generator.py _weight_generator)
__device__ double weight_normal(mt::LaneStream &py, const K &k) {
    for (;;) {
        double z;
        for (;;) {
            const double u1 = py.next_double();
            const double u2 = 1.0 - py.next_double();
            z = k.nv_magic * (u1 - 0.5) / u2;
            const double zz = z * z / 4.0;
            if (zz <= -log(u2)) break;
        }
        const double w = 50.0 + z * 10.0;
        if (!(w < 20.0 || w > 100.0)) return w;
    }
}

// numpy random_binomial for category c of the table row (n >= 1); inversion only
__device__ int64_t binomial(mt::LaneStream &g, const K &k, int64_t row, int64_t n, bool &unsupported) {
    const double p = k.pp[row];
    if (p == 0.0 && !k.flip[row]) return 0;
    if (p * (double)n > 30.0) { unsupported = true; return 0; }
    const double q = 1.0 - p;
    const double qn = n <= QN ? k.qn[row * QN + (n - 1)] : exp((double)n * k.logq[row]);
    const double np = (double)n * p;
    const double bd = fmin((double)n, np + 10.0 * sqrt(np * q + 1));
    const int64_t bound = (int64_t)bd;
    int64_t X = 0;
    double px = qn, U = g.next_double();
    while (U > px) {
        ++X;
        if (X > bound) { X = 0; px = qn; U = g.next_double(); }
        else { U -= px; px = ((double)(n - X + 1) * p * px) / ((double)X * q); }
        if (g.bad) break;
    }
    return k.flip[row] ? n - X : X;
}

struct Person { double w; int src, dst; };

// append a person on the new end of its queue; false = the queue is full (overflow)
__device__ bool enqueue(const Env &s, const K &k, const Person &p, double now) {
    if (p.src == p.dst) return true;
    const int qd = (p.src - 1) * 2 + (p.src < p.dst ? 0 : 1);
    const int len = s.i(MG_LS_QLEN, qd);
    if (len >= k.Q) return false;
    int slot = s.i(MG_LS_QHEAD, qd) + len;
    if (slot >= k.Q) slot -= k.Q;
    const int64_t it = (int64_t)qd * k.Q + slot;
    s.d(MG_LS_QW, it) = p.w;
    s.d(MG_LS_QA, it) = now;
    s.i(MG_LS_QT, it) = p.dst;
    s.i(MG_LS_QLEN, qd) = len + 1;
    return true;
}

// the generators; false = a queue overflowed
__device__ bool generate(const Env &s, const K &k, mt::LaneStream &py, mt::LaneStream &npg, double now, double gap,
                         int &generated, bool &unsupported) {
    generated = 0;
    if (k.gen == MG_LIFTSIM_UNIFORM) {
        const double thr = gap / k.interval;
        for (int i = 0; i < k.particles; ++i) {
            if (py.next_double() < thr) {
                Person p;
                p.src = 1 + (int)py.randbelow((uint32_t)k.F);
                p.dst = 1 + (int)py.randbelow((uint32_t)k.F);
                while (p.src == p.dst) {
                    p.src = 1 + (int)py.randbelow((uint32_t)k.F);
                    p.dst = 1 + (int)py.randbelow((uint32_t)k.F);
                }
                p.w = 20.0 + (100.0 - 20.0) * py.next_double();
                ++generated;
                if (!enqueue(s, k, p, now)) return false;
            }
        }
        return true;
    }
    // CUSTOM: _check_time_index mirrored literally (binary search as a loop)
    const int T = k.T;
    const double t = (double)((int64_t)now % 86400);
    int idx = s.i(MG_LS_TIDX);
    auto search = [&](int beg, int end) {
        for (;;) {
            if (beg >= T - 1 || !(k.times[beg + 1] < t)) return beg;
            if (!(k.times[end] > t)) return end;
            const int m = (beg + end) / 2;
            if (k.times[m] < t) { beg = m; end = end - 1; }
            else { beg = beg + 1; end = m; }
        }
    };
    if (idx + 1 < T && k.times[idx + 1] < t) idx = search(idx + 1, T - 1);
    if (k.times[idx] > t) idx = search(0, idx);
    s.i(MG_LS_TIDX) = idx;
    const float gap32 = (float)gap;
    uint64_t cnt[2] = {0, 0};   // poisson counts, 8 bits per floor (F <= 16 for CUSTOM; a count above 255 is unsupported)
    for (int f = 0; f < k.F; ++f) {
        const float lam = k.dens[(int64_t)idx * k.F + f] * gap32;
        uint64_t x = 0;
        if (lam >= 10.0f) { unsupported = true; return true; }
        if (lam != 0.0f) {
            const double en = gap32 == k.dt32 ? k.enlam[(int64_t)idx * k.F + f] : exp(-(double)lam);
            double prod = 1.0;
            for (;;) {
                prod *= npg.next_double();
                if (prod > en) ++x;
                else break;
                if (npg.bad || x > 255) { unsupported = true; return true; }
            }
        }
        if (f < 8) cnt[0] |= x << (8 * f);
        else cnt[1] |= x << (8 * (f - 8));
    }
    for (int f = 0; f < k.F; ++f) {
        const int n = (int)(((f < 8 ? cnt[0] : cnt[1]) >> (8 * (f & 7))) & 255u);
        if (n <= 0) continue;
        int64_t dn = n;
        const int64_t row0 = ((int64_t)idx * k.F + f) * k.F;
        // multinomial: the binomials on the numpy stream, each category's weights on the Python stream right away
        for (int j = 0; j < k.F; ++j) {
            int64_t x;
            bool last = false;
            if (j < k.F - 1) {
                x = binomial(npg, k, row0 + j, dn, unsupported);
                dn -= x;
                last = dn <= 0;
            } else {
                x = dn > 0 ? dn : 0;
                last = true;
            }
            for (int64_t c = 0; c < x; ++c) {
                Person p{weight_normal(py, k), f + 1, j + 1};
                ++generated;
                if (!enqueue(s, k, p, now)) return false;
            }
            if (last) break;
        }
    }
    return true;
}

// Elevator.person_request_in for the person at slot it of a queue
__device__ bool person_in(const Env &s, const K &k, int el, Elev &v, int &nent, double w, int dst, int src) {
    const double cf = v.pos / k.h + 1.0;
    if (fabs((double)src - cf) > EPS || fabs(v.vel) > EPS || v.door < 1.0 - 2.0 * EPS) return false;
    if (nent >= MPEE) return false;
    double ex = v.load;
    for (int j = 0; j < nent; ++j) ex += s.d(MG_LS_EW, el * 2 + j);
    if (ex + w > MAX_LOAD) {
        v.alarm = 2.0;
        request_close(v);
        return false;
    }
    s.d(MG_LS_EW, el * 2 + nent) = w;
    s.i(MG_LS_ET, el * 2 + nent) = dst;
    s.d(MG_LS_EL, el * 2 + nent) = ENTER_T;
    ++nent;
    return true;
}

__device__ void board(const Env &s, const K &k, int el) {
    Elev v = load_elev(s, el);
    const double cf = v.pos / k.h + 1.0;
    const int floor = (int)(cf + 0.5);
    const double dd = (double)floor - cf;
    const bool is_open = v.door > 1.0 - EPS && fabs(dd) < 0.05;
    const bool ready = !v.unloading && !v.entering;
    const int fi = floor - 1;
    if (is_open) {
        if (v.dir == 1) s.b(MG_LS_UP, fi) = 0;
        else if (v.dir == -1) s.b(MG_LS_DOWN, fi) = 0;
    }
    if (!(ready && is_open) || v.dir == 0) return;
    const int qd = fi * 2 + (v.dir == 1 ? 0 : 1);
    const int len = s.i(MG_LS_QLEN, qd), head = s.i(MG_LS_QHEAD, qd);
    int nent = s.i(MG_LS_NENT, el);
    bool scanning = true;
    int w = 0;   // compaction: kept persons move down over the boarded ones, oldest first
    for (int i = 0; i < len; ++i) {
        int si = head + i; if (si >= k.Q) si -= k.Q;
        const int64_t it = (int64_t)qd * k.Q + si;
        const double pw = s.d(MG_LS_QW, it);
        const int pt = s.i(MG_LS_QT, it);
        bool gone = false;
        if (scanning) {
            if (person_in(s, k, el, v, nent, pw, pt, floor)) gone = true;
            else if (!(v.alarm != 0.0)) scanning = false;
        }
        if (!gone) {
            if (w != i) {
                int sw = head + w; if (sw >= k.Q) sw -= k.Q;
                const int64_t iw = (int64_t)qd * k.Q + sw;
                s.d(MG_LS_QW, iw) = pw;
                s.d(MG_LS_QA, iw) = s.d(MG_LS_QA, it);
                s.i(MG_LS_QT, iw) = pt;
            }
            ++w;
        }
    }
    s.i(MG_LS_QLEN, qd) = w;
    s.i(MG_LS_NENT, el) = nent;
    // person_request_in may ring the alarm and request the door closing
    s.d(MG_LS_ALARM, el) = v.alarm;
    s.b(MG_LS_CLOSING, el) = (uint8_t)v.closing;
}

__device__ void zero_outputs(const Env &s) {
    s.d(MG_LS_REWARD) = 0.0; s.d(MG_LS_TIMEC) = 0.0; s.d(MG_LS_ENERGY) = 0.0; s.i(MG_LS_GIVEN) = 0;
}

// Wave job (all 64 lanes): restore both streams' next key block for the lanes that used theirs up.
__device__ void refill_streams(const Env &s, const Lay &l, uint8_t *arena, uint32_t *lds, bool live, int e0, int lane) {
    int p = 0, r = 1;
    if (live) { p = s.i(MG_LS_PYP); r = s.i(MG_LS_PYV); }
    uint64_t bal = __ballot(live && !r);
    uint32_t *base = reinterpret_cast<uint32_t *>(arena + l.off[MG_LS_PYKEY]) + (size_t)e0 * REC;
    if (bal) mt::refill_ahead(lds, base, REC, bal, ((p + REC - 1) % REC) / MTN, lane);
    if (live && !r) s.i(MG_LS_PYV) = 1;
    p = 0; r = 1;
    if (live) { p = s.i(MG_LS_NPP); r = s.i(MG_LS_NPV); }
    bal = __ballot(live && !r);
    base = reinterpret_cast<uint32_t *>(arena + l.off[MG_LS_NPKEY]) + (size_t)e0 * REC;
    if (bal) mt::refill_ahead(lds, base, REC, bal, ((p + REC - 1) % REC) / MTN, lane);
    if (live && !r) s.i(MG_LS_NPV) = 1;
}

// One env.step(action) of this lane's env (the wave's stream refill comes first, outside). Frozen and invalid envs leave
// early with zero outputs.
template <class Actions>
__device__ void step_body(const Env &s, const K &k, int lane, uint8_t (*order)[64], const Actions &act) {
    if (s.b(MG_LS_OVERFLOW) || s.b(MG_LS_UNSUPPORTED)) { zero_outputs(s); return; }
    bool bad = false;
    for (int el = 0; el < k.E; ++el) {
        const int tf = act.target(el), d = act.direction(el);
        bad |= tf < -1 || tf > k.F || d < -1 || d > 1;
    }
    s.b(MG_LS_INVALID) = bad;
    if (bad) { zero_outputs(s); return; }

    mt::LaneStream py{s.key(MG_LS_PYKEY), s.i(MG_LS_PYP), 1, false};
    mt::LaneStream npg{s.key(MG_LS_NPKEY), s.i(MG_LS_NPP), 1, false};
    const double now = s.d(MG_LS_TIME) + k.dt;
    s.d(MG_LS_TIME) = now;
    const double gap = now - s.d(MG_LS_LASTGEN);
    bool unsupported = false;
    int generated = 0;
    const bool fits = generate(s, k, py, npg, now, gap, generated, unsupported);
    s.d(MG_LS_LASTGEN) = now;
    if (!fits || unsupported || npg.bad || py.bad) {
        if (!fits) s.b(MG_LS_OVERFLOW) = 1;
        else s.b(MG_LS_UNSUPPORTED) = 1;
        zero_outputs(s);
        return;
    }
    for (int el = 0; el < k.E; ++el) {
        const int tf = act.target(el);
        if (tf >= 0) { s.i(MG_LS_DISPATCH, el) = tf; s.i(MG_LS_DISPATCH_DIR, el) = act.direction(el); }
    }
    double energy = 0.0;   // Python's sum() from int 0, in index order
    int delivered = 0, loaded = 0;
    for (int el = 0; el < k.E; ++el) energy = energy + run_elevator(s, k, el, delivered, loaded);
    for (int f = 0; f < k.F; ++f) {
        s.b(MG_LS_UP, f) = s.i(MG_LS_QLEN, 2 * f) > 0;
        s.b(MG_LS_DOWN, f) = s.i(MG_LS_QLEN, 2 * f + 1) > 0;
    }
    // random.shuffle of the elevator indices, then boarding in that order
    for (int el = 0; el < k.E; ++el) order[el][lane] = (uint8_t)el;
    for (int i = k.E - 1; i > 0; --i) {
        const int j = (int)py.randbelow((uint32_t)(i + 1));
        const uint8_t t = order[i][lane]; order[i][lane] = order[j][lane]; order[j][lane] = t;
    }
    if (py.bad) {   // the shuffle read past the next key block: flag and freeze before anything else is written
        s.b(MG_LS_UNSUPPORTED) = 1;
        zero_outputs(s);
        return;
    }
    for (int i = 0; i < k.E; ++i) board(s, k, order[i][lane]);
    int given_up = 0;
    for (int qd = 0; qd < 2 * k.F; ++qd) {
        int len = s.i(MG_LS_QLEN, qd), head = s.i(MG_LS_QHEAD, qd);
        while (len > 0 && now - s.d(MG_LS_QA, (int64_t)qd * k.Q + head) > GIVE_UP) {
            head = head + 1 == k.Q ? 0 : head + 1;
            --len;
            ++given_up;
        }
        s.i(MG_LS_QLEN, qd) = len;
        s.i(MG_LS_QHEAD, qd) = len == 0 ? 0 : head;
    }
    double waiting = 0.0;
    for (int f = 0; f < k.F; ++f) {
        waiting += k.dt * (double)s.i(MG_LS_QLEN, 2 * f);
        waiting += k.dt * (double)s.i(MG_LS_QLEN, 2 * f + 1);
    }
    waiting += (double)loaded * k.dt;
    const double reward = -(waiting + 5e-4 * energy + (double)(300 * given_up)) * 1.0e-4;
    s.d(MG_LS_REWARD) = reward;
    s.d(MG_LS_TIMEC) = waiting;
    s.d(MG_LS_ENERGY) = energy;
    s.i(MG_LS_GIVEN) = given_up;
    // statistics ring: slot head is the newest
    int head = s.i(MG_LS_SHEAD) - 1;
    if (head < 0) head += k.W;
    s.i(MG_LS_SHEAD) = head;
    s.i(MG_LS_SCOUNT) = min(s.i(MG_LS_SCOUNT) + 1, k.W);
    s.i(MG_LS_SD, head) = delivered; s.i(MG_LS_SG, head) = generated; s.i(MG_LS_SA, head) = given_up;
    s.d(MG_LS_SW, head) = waiting; s.d(MG_LS_SE, head) = energy;
    s.i(MG_LS_PYP) = py.p; s.i(MG_LS_PYV) = py.ready;
    s.i(MG_LS_NPP) = npg.p; s.i(MG_LS_NPV) = npg.ready;
}

struct Records {
    double *ret, *reward, *timec, *energy;
    int32_t *given, *actions;
};

int check(const mg_liftsim_config *c, int32_t n, const char *fn) {
    if (n <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "%s: n_envs = %d", fn, n);
    if (c->floors < 2 || c->floors > MG_LIFTSIM_MAX_FLOORS)
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: floors = %d (need 2..%d)", fn, c->floors, MG_LIFTSIM_MAX_FLOORS);
    if (c->elevators < 1 || c->elevators > MG_LIFTSIM_MAX_ELEVATORS)
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: elevators = %d (need 1..%d)", fn, c->elevators,
                             MG_LIFTSIM_MAX_ELEVATORS);
    if (!(c->dt > 0.0 && c->dt <= 1.0))
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: dt = %g (need 0 < dt <= 1)", fn, c->dt);
    if (!(c->floor_height > 0.0)) return mg::set_error(MG_ERR_BAD_CONFIG, "%s: floor_height = %g", fn, c->floor_height);
    if (c->queue_capacity < 1 || c->queue_capacity > 4096)
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: queue_capacity = %d (need 1..4096)", fn, c->queue_capacity);
    if (c->window < 1 || c->window > (1 << 20))
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: window = %d", fn, c->window);
    if (c->generator == MG_LIFTSIM_UNIFORM) {
        if (c->particle_number < 0 || !(c->generation_interval > 0.0))
            return mg::set_error(MG_ERR_BAD_CONFIG, "%s: particle_number = %d, generation_interval = %g", fn,
                                 c->particle_number, c->generation_interval);
    } else if (c->generator == MG_LIFTSIM_CUSTOM) {
        if (c->floors > 16) return mg::set_error(MG_ERR_BAD_CONFIG, "%s: CUSTOM floors = %d (need <= 16)", fn, c->floors);
        if (c->table_len < 1) return mg::set_error(MG_ERR_BAD_CONFIG, "%s: table_len = %d", fn, c->table_len);
        if (!c->times || !c->dens || !c->enlam || !c->pp || !c->flip || !c->logq || !c->qn)
            return mg::set_error(MG_ERR_BAD_CONFIG, "%s: a CUSTOM table is NULL", fn);
    } else {
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: generator = %d", fn, c->generator);
    }
    return MG_OK;
}

K fold(const mg_liftsim_config *c) {
    K k{};
    k.F = c->floors; k.E = c->elevators; k.gen = c->generator; k.Q = c->queue_capacity; k.W = c->window;
    k.particles = c->particle_number; k.T = c->table_len;
    k.h = c->floor_height; k.dt = c->dt; k.interval = c->generation_interval; k.nv_magic = c->nv_magic;
    k.dt32 = (float)c->dt;
    k.times = c->times; k.enlam = c->enlam; k.pp = c->pp; k.logq = c->logq; k.qn = c->qn; k.dens = c->dens;
    k.flip = c->flip;
    return k;
}

Lay lay(const mg_liftsim_config *c, int32_t n) { return layout(c->floors, c->elevators, c->queue_capacity, c->window, n); }

dim3 grid(int32_t n) { return dim3((unsigned)(((int64_t)n + 63) / 64)); }

}  // namespace
