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
#include <cmath>

#include "mg_common.h"
#include "mg_mt19937.h"

namespace {

using mt::MTN;
constexpr int REC = 2 * MTN;   // u32 words of one lane's stream record
constexpr double EPS = 1.0e-2, GRAV = 9.80, MAX_ACC = 1.0, MAX_SPD = 2.0, ENTER_T = 2.0, DOOR_V = 0.5;
constexpr double DOOR_P = 350.0, STANDBY_P = 100.0, MAX_LOAD = 1600.0, RATED = 600.0, NET = 300.0, PULLEY = 0.27;
constexpr double MOTOR_EFF = 0.8, GIVE_UP = 300.0;
constexpr double HUGE_PRIORITY = 1.0e8;   // mansion/utils.py HUGE
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

struct Records {
    double *ret, *reward, *timec, *energy;
    int32_t *given, *actions;
};

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

#ifndef MG_LIFTSIM_CORE_ONLY   // liftsim_policy.hip takes the device functions and the host checks above, and none of what follows
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
#endif   // MG_LIFTSIM_CORE_ONLY
