/* oracle/replay_main.c — stand-alone replay of the three C oracles. TEST INFRASTRUCTURE (see oracle/__init__.py).
 *
 *     replay CASES RESULTS
 *
 * reads a case file, calls quadrotor_oracle.c / maze_oracle.c / walker_oracle.c exactly as the ctypes front ends
 * (oracle/quadrotor.py, oracle/maze.py, oracle/walker_c.py) do, and writes every output array to a result file. It has its
 * own main so that the oracles can run under AddressSanitizer / UBSan / MemorySanitizer and be compiled by several compilers
 * at several optimisation levels (oracle/Makefile: asan, msan, replay); tests/test_oracle_replay.py builds the cases with
 * tests/oracle_replay_cases.py and holds the result files of all builds against each other byte for byte.
 *
 * File format (cases and results alike; everything little-endian, every blob padded with zeros to a multiple of 8 bytes):
 *     char magic[8]        "MGRPLY01" (cases) / "MGRRES01" (results)
 *     u32  n_calls, u32 0
 *     n_calls x { u32 op, u32 n_blobs, n_blobs x { u64 n_bytes, n_bytes of raw array or struct (+ padding) } }
 * A result call carries the op of its case call and the output blobs in the order the op's comment below lists them.
 * Every input blob is copied into a heap block of exactly its size before the oracle sees it, so that a sanitizer sees the
 * bounds the Python caller's arrays have. Structs travel as the raw bytes of the ctypes structures; their pointer members
 * are meaningless in the file and are set here: qo_consts.map / .velocity_targets, every pointer of mo_task / mo_state /
 * mo_view, and wo_model.table / .sph_margin (one array, the margins behind the table at element `margin_off`, as
 * walker_c.make_model lays them out; margin_off < 0: NULL). An empty blob stands for a NULL pointer.
 * The first blob of a call, P, is an int64 array of the op's integer parameters; D is a float64 array.
 *
 * ops (inputs -> outputs):
 *   1 Q_STEP         P{n,T,legacy,autoreset} consts map vt states ct actions[T][n][4] ar episode
 *                    -> T x {obs[n][16] reward[n] done[n] failed[n]} states ct episode
 *                    (qo_set_legacy_promotion(legacy), then T x qo_batch_env_step or qo_batch_env_step_autoreset)
 *   2 Q_VEL_STEP     P{T} consts map vt state ct actions[T][4] -> T x {obs[19] reward done failed} state ct
 *   3 Q_VEL_TARGETS  P{nt} consts actions[nt][4] -> targets[nt][3]
 *   4 Q_DEFAULTS     P{} -> consts sizes{sizeof state, sizeof consts}
 *   5 Q_INV3         P{} A[9] -> Ainv[9]
 *   6 Q_PHILOX       P{} ctr[4] key[2] -> out[4]
 *   7 Q_RESET_NOISE  P{gid,episode} ar -> vel[3] omega[3]
 *   8 Q_OBSERVE      P{n,refresh} consts states -> obs[n][16] states      (refresh: qo_refresh_inverse first, make_states)
 *   9 Q_BATCH_RUN    P{n,n_batches,iters} consts map vt states init ct actions -> count states ct
 *  16 M_EPISODE      P{task_type,max_steps,mode,view_grid,T,observe} D{collision_dist} task walls texts food_rewards
 *                    food_interval start actions[T][2] view textures ceil sin4 cos4
 *                    -> [obs] T x {reward done state [obs]} cur_food wait_refresh revival
 *                    (mo_reset; a non-empty `start` mo_state replaces grid / steps / ori_idx / ori / loc / life; mode 0:
 *                    mo_step_2d + mo_observe_2d, 1: mo_step_disc3d, 2: mo_step_cont3d, both + mo_observe_3d)
 *  17 M_VIEW         P{} D{pos0,pos1,s_ori,c_ori} task walls texts view textures ceil transparents -> rgb[H][V][3]
 *  32 W_EPISODE      P{T,reset,margin_off} model table prm env noise actions[T][nj]
 *                    -> [obs env] T x {obs rewards{reward,rewards5[5]} done env}
 *  33 W_SUBSTEP      P{n_sub,margin_off} model table prm state tau -> n_sub x {nr touch[2] state}
 *  34 W_RUN          P{k,n_envs,n_steps,n_rows,margin_off[k]} models task_id prm envs actions table[k]
 *                    -> count envs flops{wo_flops_read's return}
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "maze_oracle.h"
#include "quadrotor_oracle.h"
#include "walker_oracle.h"

#ifdef WO_COUNT_CAPS
extern unsigned long long wo_cap_count[4];
#endif

enum { Q_STEP = 1, Q_VEL_STEP, Q_VEL_TARGETS, Q_DEFAULTS, Q_INV3, Q_PHILOX, Q_RESET_NOISE, Q_OBSERVE, Q_BATCH_RUN,
       M_EPISODE = 16, M_VIEW, W_EPISODE = 32, W_SUBSTEP, W_RUN };
#define MAX_BLOBS 40

typedef struct { void *p; size_t n; } blob;

static FILE *g_out;
static uint32_t g_blocks;

static void die(const char *what) {
    fprintf(stderr, "replay: %s\n", what);
    exit(2);
}

static void *xmalloc(size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p) die("out of memory");
    return p;
}

static void need(const blob *b, size_t n, const char *what) {
    if (b->n != n) { fprintf(stderr, "replay: blob %s has %zu bytes, expected %zu\n", what, b->n, n); exit(2); }
}

static void emit(const void *p, size_t n) {
    static const char zeros[8] = {0};
    const uint64_t n64 = n;
    if (fwrite(&n64, 8, 1, g_out) != 1 || (n && fwrite(p, 1, n, g_out) != n) || ((n & 7) && fwrite(zeros, 1, 8 - (n & 7), g_out) != 8 - (n & 7)))
        die("write failed");
    ++g_blocks;
}

static const void *or_null(const blob *b) { return b->n ? b->p : NULL; }

/* ---- quadrotor ----------------------------------------------------------------------------------------------------- */

static void load_consts(qo_consts *c, const blob *consts, const blob *map, const blob *vt) {
    need(consts, sizeof(*c), "qo_consts");
    memcpy(c, consts->p, sizeof(*c));
    c->map = map ? (const int32_t *)or_null(map) : NULL;
    c->velocity_targets = vt ? (const float *)or_null(vt) : NULL;
    if (c->map) need(map, sizeof(int32_t) * (size_t)c->map_h * (size_t)c->map_w, "map");
}

static void q_step(const blob *a) {
    const int64_t *P = a[0].p;
    const int n = (int)P[0], T = (int)P[1], autoreset = (int)P[3];
    qo_consts c;
    load_consts(&c, &a[1], &a[2], &a[3]);
    need(&a[4], sizeof(qo_state) * n, "states"); need(&a[5], sizeof(int) * n, "ct");
    need(&a[6], sizeof(float) * 4 * n * T, "actions");
    qo_state *states = a[4].p;
    int *ct = a[5].p;
    float *obs = xmalloc(sizeof(float) * 16 * n);
    double *reward = xmalloc(sizeof(double) * n);
    int *done = xmalloc(sizeof(int) * n), *failed = xmalloc(sizeof(int) * n);
    if (autoreset) { need(&a[7], sizeof(qo_autoreset), "ar"); need(&a[8], sizeof(uint32_t) * n, "episode"); }
    qo_set_legacy_promotion((int)P[2]);
    for (int t = 0; t < T; ++t) {
        const float *act = (const float *)a[6].p + (size_t)4 * n * t;
        if (autoreset) qo_batch_env_step_autoreset(&c, a[7].p, n, states, ct, a[8].p, act, obs, reward, done, failed);
        else qo_batch_env_step(&c, n, states, ct, act, obs, reward, done, failed);
        emit(obs, sizeof(float) * 16 * n); emit(reward, sizeof(double) * n); emit(done, sizeof(int) * n); emit(failed, sizeof(int) * n);
    }
    qo_set_legacy_promotion(0);
    emit(states, a[4].n); emit(ct, a[5].n); emit(a[8].p, autoreset ? a[8].n : 0);
    free(obs); free(reward); free(done); free(failed);
}

static void q_vel_step(const blob *a) {
    const int T = (int)((const int64_t *)a[0].p)[0];
    qo_consts c;
    load_consts(&c, &a[1], &a[2], &a[3]);
    need(&a[3], sizeof(float) * 3 * (size_t)c.nt, "velocity_targets");
    need(&a[4], sizeof(qo_state), "state"); need(&a[5], sizeof(int), "ct"); need(&a[6], sizeof(float) * 4 * T, "actions");
    for (int t = 0; t < T; ++t) {
        float *obs = xmalloc(sizeof(float) * 19);
        double reward;
        int done;
        const int failed = qo_env_step_velocity(&c, a[4].p, a[5].p, (const float *)a[6].p + 4 * t, obs, &reward, &done);
        emit(obs, sizeof(float) * 19); emit(&reward, sizeof(reward)); emit(&done, sizeof(done)); emit(&failed, sizeof(failed));
        free(obs);
    }
    emit(a[4].p, a[4].n); emit(a[5].p, a[5].n);
}

static void q_vel_targets(const blob *a) {
    const int nt = (int)((const int64_t *)a[0].p)[0];
    qo_consts c;
    load_consts(&c, &a[1], NULL, NULL);
    need(&a[2], sizeof(float) * 4 * nt, "actions");
    float *targets = xmalloc(sizeof(float) * 3 * nt);
    qo_velocity_targets(&c, nt, a[2].p, targets);
    emit(targets, sizeof(float) * 3 * nt);
    free(targets);
}

static void q_small(uint32_t op, const blob *a) {
    const int64_t *P = a[0].p;
    if (op == Q_DEFAULTS) {
        qo_consts c;
        qo_default_consts(&c);
        const uint64_t sizes[2] = {qo_sizeof_state(), qo_sizeof_consts()};
        emit(&c, sizeof(c)); emit(sizes, sizeof(sizes));
    } else if (op == Q_INV3) {
        need(&a[1], sizeof(float) * 9, "A");
        float *inv = xmalloc(sizeof(float) * 9);
        qo_inv3_f32(a[1].p, inv);
        emit(inv, sizeof(float) * 9);
        free(inv);
    } else if (op == Q_PHILOX) {
        need(&a[1], 16, "ctr"); need(&a[2], 8, "key");
        uint32_t *out = xmalloc(16);
        qo_philox4x32_10(a[1].p, a[2].p, out);
        emit(out, 16);
        free(out);
    } else if (op == Q_RESET_NOISE) {
        need(&a[1], sizeof(qo_autoreset), "ar");
        double *v = xmalloc(24), *w = xmalloc(24);
        qo_reset_noise(a[1].p, (uint64_t)P[0], (uint32_t)P[1], v, w);
        emit(v, 24); emit(w, 24);
        free(v); free(w);
    } else if (op == Q_OBSERVE) {
        const int n = (int)P[0];
        qo_consts c;
        load_consts(&c, &a[1], NULL, NULL);
        need(&a[2], sizeof(qo_state) * n, "states");
        qo_state *states = a[2].p;
        float *obs = xmalloc(sizeof(float) * 16 * n);
        for (int e = 0; e < n; ++e) {
            if (P[1]) qo_refresh_inverse(&states[e]);
            qo_observe(&c, &states[e], obs + 16 * e);
        }
        emit(obs, sizeof(float) * 16 * n); emit(states, a[2].n);
        free(obs);
    } else {                                             /* Q_BATCH_RUN */
        const int n = (int)P[0], nb = (int)P[1], iters = (int)P[2];
        qo_consts c;
        load_consts(&c, &a[1], &a[2], &a[3]);
        need(&a[4], sizeof(qo_state) * n, "states"); need(&a[5], sizeof(qo_state) * n, "init"); need(&a[6], sizeof(int) * n, "ct");
        need(&a[7], sizeof(float) * 4 * n * nb, "actions");
        const int64_t count = qo_batch_run(&c, n, a[4].p, a[5].p, a[6].p, a[7].p, nb, iters);
        emit(&count, sizeof(count)); emit(a[4].p, a[4].n); emit(a[6].p, a[6].n);
    }
}

/* ---- maze ---------------------------------------------------------------------------------------------------------- */

static void load_task(mo_task *t, const blob *task, const blob *walls, const blob *texts, const blob *fr, const blob *fi) {
    need(task, sizeof(*t), "mo_task");
    memcpy(t, task->p, sizeof(*t));
    const size_t nn = (size_t)t->n * (size_t)t->n;
    need(walls, 4 * nn, "walls"); need(texts, 4 * nn, "texts"); need(fr, 8 * nn, "food_rewards"); need(fi, 4 * nn, "food_interval");
    t->walls = walls->p; t->texts = texts->p; t->food_rewards = fr->p; t->food_interval = fi->p;
}

static void load_view(mo_view *v, const blob *view, const blob *tex, const blob *ceil) {
    need(view, sizeof(*v), "mo_view");
    memcpy(v, view->p, sizeof(*v));
    if (tex->n % (sizeof(float) * 3 * (size_t)v->tex_size * (size_t)v->tex_size)) die("textures: not a whole number of textures");
    need(ceil, 3 * (size_t)v->tex_size * (size_t)v->tex_size, "ceil_tex");
    v->textures = tex->p; v->ceil_tex = ceil->p;
}

static void m_episode(const blob *a) {
    const int64_t *P = a[0].p;
    const int task_type = (int)P[0], max_steps = (int)P[1], mode = (int)P[2], vg = (int)P[3], T = (int)P[4], observe = (int)P[5];
    need(&a[1], 8, "D");
    const double collision_dist = *(const double *)a[1].p;
    mo_task task;
    load_task(&task, &a[2], &a[3], &a[4], &a[5], &a[6]);
    const size_t nn = (size_t)task.n * (size_t)task.n;
    mo_state s;
    memset(&s, 0, sizeof(s));                            /* ctypes zero-fills CState and maze.State its arrays */
    s.cur_food = calloc(nn, sizeof(double)); s.wait_refresh = calloc(nn, sizeof(int32_t)); s.revival = calloc(nn, sizeof(int32_t));
    if (!s.cur_food || !s.wait_refresh || !s.revival) die("out of memory");
    need(&a[8], sizeof(double) * 2 * T, "actions");
    mo_view view;
    size_t obs_bytes = 0;
    if (observe && mode == 0) obs_bytes = sizeof(float) * (2 * vg + 1) * (2 * vg + 1);
    if (observe && mode != 0) {
        load_view(&view, &a[9], &a[10], &a[11]);
        need(&a[12], 16, "sin4"); need(&a[13], 16, "cos4");
        obs_bytes = sizeof(int32_t) * 3 * (size_t)view.H * (size_t)view.V;
    }
    mo_reset(&task, task_type, &s);
    if (a[7].n) {
        need(&a[7], sizeof(mo_state), "start");
        const mo_state *st = a[7].p;
        s.grid[0] = st->grid[0]; s.grid[1] = st->grid[1]; s.steps = st->steps; s.ori_idx = st->ori_idx; s.ori = st->ori;
        s.loc[0] = st->loc[0]; s.loc[1] = st->loc[1]; s.life = st->life;
    }
    for (int t = -1; t < T; ++t) {
        if (t >= 0) {
            const double *act = (const double *)a[8].p + 2 * t;
            double reward;
            int32_t done;
            if (mode == 0) done = mo_step_2d(&task, task_type, max_steps, &s, (int)act[0], &reward);
            else if (mode == 1) done = mo_step_disc3d(&task, task_type, max_steps, &s, (int)act[0], &reward);
            else done = mo_step_cont3d(&task, task_type, max_steps, collision_dist, &s, act[0], act[1], &reward);
            mo_state plain = s;
            plain.cur_food = NULL; plain.wait_refresh = NULL; plain.revival = NULL;
            emit(&reward, sizeof(reward)); emit(&done, sizeof(done)); emit(&plain, sizeof(plain));
        }
        if (observe) {
            void *obs = xmalloc(obs_bytes);
            if (mode == 0) mo_observe_2d(&task, task_type, &s, vg, obs);
            else mo_observe_3d(&task, task_type, &view, &s, mode == 2, a[12].p, a[13].p, obs);
            emit(obs, obs_bytes);
            free(obs);
        }
    }
    emit(s.cur_food, 8 * nn); emit(s.wait_refresh, 4 * nn); emit(s.revival, 4 * nn);
    free(s.cur_food); free(s.wait_refresh); free(s.revival);
}

static void m_view(const blob *a) {
    need(&a[1], 32, "D");
    const double *D = a[1].p;
    mo_task task;
    mo_view view;
    need(&a[2], sizeof(task), "mo_task");
    memcpy(&task, a[2].p, sizeof(task));
    const size_t nn = (size_t)task.n * (size_t)task.n;
    need(&a[3], 4 * nn, "walls"); need(&a[4], 4 * nn, "texts"); need(&a[8], 8 * nn, "transparents");
    task.walls = a[3].p; task.texts = a[4].p; task.food_rewards = NULL; task.food_interval = NULL;
    load_view(&view, &a[5], &a[6], &a[7]);
    const size_t bytes = sizeof(int32_t) * 3 * (size_t)view.H * (size_t)view.V;
    int32_t *rgb = xmalloc(bytes);
    mo_maze_view(&task, &view, D, D[2], D[3], a[8].p, rgb);
    emit(rgb, bytes);
    free(rgb);
}

/* ---- walker -------------------------------------------------------------------------------------------------------- */

static void load_model(wo_model *m, const void *bytes, const blob *table, int64_t margin_off) {
    memcpy(m, bytes, sizeof(*m));
    m->table = table->p;
    m->sph_margin = margin_off < 0 ? NULL : (const double *)table->p + margin_off;
    const size_t rows = 25 * (size_t)m->nb + 12 * (size_t)m->nj + 4 * (size_t)m->ns + 7 * (size_t)m->ng;
    if (table->n != 8 * (rows + (margin_off < 0 ? 0 : (size_t)m->ns)) || (margin_off >= 0 && (size_t)margin_off != rows))
        die("walker table: size does not match the model's counts");
}

static void w_episode(const blob *a) {
    const int64_t *P = a[0].p;
    const int T = (int)P[0];
    wo_model m;
    need(&a[1], sizeof(m), "wo_model"); need(&a[3], sizeof(wo_params), "wo_params"); need(&a[4], sizeof(wo_env), "wo_env");
    load_model(&m, a[1].p, &a[2], P[2]);
    const wo_params *prm = a[3].p;
    wo_env *e = a[4].p;
    const size_t obs_bytes = sizeof(float) * (8 + 2 * (size_t)m.nj + (size_t)m.nf);
    need(&a[6], sizeof(float) * (size_t)m.nj * T, "actions");
    if (P[1]) {
        if (a[5].n) need(&a[5], sizeof(double) * (size_t)m.nj, "joint_noise");
        float *obs = xmalloc(obs_bytes);
        wo_env_reset(&m, prm, e, or_null(&a[5]), obs);
        emit(obs, obs_bytes); emit(e, sizeof(*e));
        free(obs);
    }
    for (int t = 0; t < T; ++t) {
        float *obs = xmalloc(obs_bytes);
        double *r = xmalloc(sizeof(double) * 6);
        const int32_t done = wo_env_step(&m, prm, e, (const float *)a[6].p + (size_t)m.nj * t, obs, r, r + 1);
        emit(obs, obs_bytes); emit(r, sizeof(double) * 6); emit(&done, sizeof(done)); emit(e, sizeof(*e));
        free(obs); free(r);
    }
}

static void w_substep(const blob *a) {
    const int64_t *P = a[0].p;
    wo_model m;
    need(&a[1], sizeof(m), "wo_model"); need(&a[3], sizeof(wo_params), "wo_params"); need(&a[4], sizeof(wo_state), "wo_state");
    load_model(&m, a[1].p, &a[2], P[1]);
    need(&a[5], sizeof(double) * (size_t)m.nj, "tau");
    for (int t = 0; t < (int)P[0]; ++t) {
        unsigned long long *touch = xmalloc(16);
        const int32_t nr = wo_substep(&m, a[3].p, a[4].p, a[5].p, touch);
        emit(&nr, sizeof(nr)); emit(touch, 16); emit(a[4].p, a[4].n);
        free(touch);
    }
}

static void w_run(const blob *a) {
    const int64_t *P = a[0].p;
    const int k = (int)P[0], n_envs = (int)P[1], n_steps = (int)P[2], n_rows = (int)P[3];
    need(&a[1], sizeof(wo_model) * k, "models"); need(&a[2], sizeof(int) * n_envs, "task_id"); need(&a[3], sizeof(wo_params), "wo_params");
    need(&a[4], sizeof(wo_env) * n_envs, "envs");
    wo_model *models = xmalloc(sizeof(wo_model) * k);
    int nj = 0;
    for (int i = 0; i < k; ++i) {
        load_model(&models[i], (const char *)a[1].p + sizeof(wo_model) * i, &a[6 + i], P[4 + i]);
        nj = models[i].nj > nj ? models[i].nj : nj;
    }
    if (a[5].n < sizeof(float) * (size_t)nj * n_rows) die("wo_run: action table too small");
    const int64_t count = wo_run(models, a[2].p, a[3].p, a[4].p, n_envs, n_steps, a[5].p, n_rows);
    unsigned long long flops[9] = {0};
    const int32_t counted = wo_flops_read(flops, 0);
    emit(&count, sizeof(count)); emit(a[4].p, a[4].n); emit(&counted, sizeof(counted));
    free(models);
}

/* ---- driver -------------------------------------------------------------------------------------------------------- */

static void read_exact(FILE *f, void *p, size_t n) {
    if (n && fread(p, 1, n, f) != n) die("case file truncated");
}

int main(int argc, char **argv) {
    if (argc != 3) die("usage: replay CASES RESULTS");
    FILE *in = fopen(argv[1], "rb");
    if (!in) die("cannot open the case file");
    g_out = fopen(argv[2], "wb");
    if (!g_out) die("cannot open the result file");
    char magic[8];
    uint32_t head[2];
    read_exact(in, magic, 8);
    read_exact(in, head, 8);
    if (memcmp(magic, "MGRPLY01", 8)) die("not a case file");
    if (fwrite("MGRRES01", 8, 1, g_out) != 1 || fwrite(head, 8, 1, g_out) != 1) die("write failed");
    for (uint32_t call = 0; call < head[0]; ++call) {
        uint32_t oh[2];
        blob a[MAX_BLOBS];
        memset(a, 0, sizeof(a));
        read_exact(in, oh, 8);
        if (oh[1] < 1 || oh[1] > MAX_BLOBS) die("bad blob count");
        for (uint32_t i = 0; i < oh[1]; ++i) {
            uint64_t n;
            char pad[8];
            read_exact(in, &n, 8);
            a[i].n = (size_t)n;
            a[i].p = xmalloc(a[i].n);
            read_exact(in, a[i].p, a[i].n);
            read_exact(in, pad, (8 - (a[i].n & 7)) & 7);
        }
        /* the result call's header is patched once its block count is known */
        const long at = ftell(g_out);
        g_blocks = 0;
        if (fwrite(oh, 8, 1, g_out) != 1) die("write failed");
        switch (oh[0]) {
        case Q_STEP: q_step(a); break;
        case Q_VEL_STEP: q_vel_step(a); break;
        case Q_VEL_TARGETS: q_vel_targets(a); break;
        case Q_DEFAULTS: case Q_INV3: case Q_PHILOX: case Q_RESET_NOISE: case Q_OBSERVE: case Q_BATCH_RUN: q_small(oh[0], a); break;
        case M_EPISODE: m_episode(a); break;
        case M_VIEW: m_view(a); break;
        case W_EPISODE: w_episode(a); break;
        case W_SUBSTEP: w_substep(a); break;
        case W_RUN: w_run(a); break;
        default: die("unknown op");
        }
        const long end = ftell(g_out);
        const uint32_t n_in = oh[1];
        oh[1] = g_blocks;
        if (at < 0 || end < 0 || fseek(g_out, at, SEEK_SET) || fwrite(oh, 8, 1, g_out) != 1 || fseek(g_out, end, SEEK_SET)) die("write failed");
        for (uint32_t i = 0; i < n_in; ++i) free(a[i].p);
    }
    fclose(in);
    if (fclose(g_out)) die("write failed");
#ifdef WO_COUNT_CAPS
    printf("caps max_candidates=%llu ground_dropped=%llu pairs_cut=%llu max_contacts=%llu\n", wo_cap_count[0], wo_cap_count[1],
           wo_cap_count[2], wo_cap_count[3]);
#endif
    return 0;
}
