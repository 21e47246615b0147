// maze_core.h — the MetaMaze family's shared core: task and agent access, evaluation_rule and the reset, the 2-D move and
// observation, the 3-D transitions, the step every stepping kernel shares (step_tail, Returns) and the host checks. maze.hip,
// maze_policy.hip, maze_expert.hip and maze3d_policy.hip include it; each keeps its own copy (anonymous namespace) and
// defines the kernels it launches. The renderer and the design notes are in maze.hip.
#pragma once
#include "mg_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// task / state access
// ------------------------------------------------------------------------------------------------

struct Task {   // one row of the task table, resolved for an env
    int n, nn;
    const int8_t *walls;
    const uint8_t *texts;
    const double *food;
    const int32_t *interval;
    const int16_t *food_cells;   // optional compact list of the cells that can hold food (NULL = all cells)
    int n_food;
    const int16_t *cell_slot;    // (slot layout) inverse of food_cells for this task: slot of a cell, -1 = never holds food
    const double *slot_food;     // (slot layout) [k * slot_stride]: food_rewards of the task's k-th listed cell
    const int32_t *slot_interval;
    int slot_stride;
    int sx, sy, gx, gy;
    double cell_size, wall_h, agent_h, init_life, max_life, step_reward, goal_reward;
};

__device__ __forceinline__ Task load_task(const mg_maze_tasks &T, int tid) {
    Task t;
    t.n = T.n;
    t.nn = T.n * T.n;
    const size_t off = (size_t)tid * t.nn;
    t.walls = T.walls + off;
    t.texts = T.texts + off;
    t.food = T.food_rewards ? T.food_rewards + off : nullptr;
    t.interval = T.food_interval ? T.food_interval + off : nullptr;
    t.food_cells = (T.food_cells != nullptr && T.n_food != nullptr) ? T.food_cells + (size_t)tid * T.max_food : nullptr;
    t.n_food = t.food_cells ? T.n_food[tid] : t.nn;
    t.cell_slot = T.cell_slot ? T.cell_slot + off : nullptr;
    t.slot_food = T.slot_food ? T.slot_food + tid : nullptr;
    t.slot_interval = T.slot_interval ? T.slot_interval + tid : nullptr;
    t.slot_stride = T.n_tasks;
    t.sx = T.start[2 * tid];
    t.sy = T.start[2 * tid + 1];
    t.gx = T.goal[2 * tid];
    t.gy = T.goal[2 * tid + 1];
    const double *s = T.scalars + (size_t)tid * 8;
    t.cell_size = s[0]; t.wall_h = s[1]; t.agent_h = s[2]; t.init_life = s[3];
    t.max_life = s[4]; t.step_reward = s[5]; t.goal_reward = s[6];
    return t;
}

struct Agent {   // scalar per-env state
    int gx, gy, steps, ori_idx;
    double ori, life;
    float lx, ly;
};

__device__ __forceinline__ Agent load_agent(const mg_maze_state &st, int n_envs, int e) {
    Agent a;
    a.gx = st.grid[e];
    a.gy = st.grid[n_envs + e];
    a.steps = st.steps[e];
    a.ori_idx = st.ori_idx ? st.ori_idx[e] : 0;
    a.ori = st.ori ? st.ori[e] : 0.0;
    a.lx = st.loc ? st.loc[e] : 0.0f;
    a.ly = st.loc ? st.loc[n_envs + e] : 0.0f;
    a.life = st.life ? st.life[e] : 0.0;
    return a;
}

__device__ __forceinline__ void store_agent(const mg_maze_state &st, int n_envs, int e, const Agent &a) {
    st.grid[e] = a.gx;
    st.grid[n_envs + e] = a.gy;
    st.steps[e] = a.steps;
    if (st.ori_idx) st.ori_idx[e] = a.ori_idx;
    if (st.ori) st.ori[e] = a.ori;
    if (st.loc) { st.loc[e] = a.lx; st.loc[n_envs + e] = a.ly; }
    if (st.life) st.life[e] = a.life;
}

// MazeBase.reset maze_base.py:40-63 — scalar part
__device__ __forceinline__ void reset_agent(const Task &t, int task_type, Agent &a) {
    a.gx = t.sx;
    a.gy = t.sy;
    a.lx = (float)(t.sx * t.cell_size + 0.5 * t.cell_size);   // get_cell_center maze_base.py:194-197
    a.ly = (float)(t.sy * t.cell_size + 0.5 * t.cell_size);
    a.ori = 0.0;
    a.ori_idx = 0;
    a.steps = 0;
    if (task_type == MG_MAZE_SURVIVAL) a.life = t.init_life;
}

// index of cell c of env e in the SURVIVAL arrays: [N][n*n] (cell_stride 1) for the workgroup-per-env
// 3-D kernel, [n*n][N] (env_stride 1) for the lane-per-env 2-D kernel, so both access them coalesced
__device__ __forceinline__ size_t fidx(const mg_maze_state &st, int e, int c) {
    return (size_t)e * st.food_env_stride + (size_t)c * st.food_cell_stride;
}

// MazeBase.reset — per-cell part (SURVIVAL), cells c = first, first+stride, ...
// full = true (mg_maze_reset): every cell is written. full = false (fused auto-reset): with a food-cell list
// only those cells are rewritten — the others still hold the values the last full reset gave them, because
// nothing ever changes a cell whose food is <= 1e-2 and whose interval is 0.
__device__ __forceinline__ void reset_cells(const Task &t, const mg_maze_state &st, int e, int first, int stride,
                                            bool full) {
    if (st.food_by_slot) {            // slot layout: the listed cells are all there is
        for (int k = first; k < t.n_food; k += stride) {
            const size_t i = fidx(st, e, k);
            st.wait_refresh[i] = 0;
            st.cur_food[i] = t.slot_food[(size_t)k * t.slot_stride];
            st.revival[i] = t.slot_interval[(size_t)k * t.slot_stride];
        }
        return;
    }
    const bool listed = !full && t.food_cells != nullptr;
    const int count = listed ? t.n_food : t.nn;
    for (int k = first; k < count; k += stride) {
        const int c = listed ? (int)t.food_cells[k] : k;
        const size_t i = fidx(st, e, c);
        st.wait_refresh[i] = 0;
        st.cur_food[i] = t.food[c];
        st.revival[i] = t.interval[c];
    }
}

// evaluation_rule maze_base.py:65-95 — scalar part. Returns done; touches the agent's cell only.
__device__ __forceinline__ int eval_scalar(const Task &t, const mg_maze_state &st, int e, int task_type,
                                           int max_steps, Agent &a, double &reward) {
    a.steps += 1;
    if (task_type == MG_MAZE_SURVIVAL) {
        int c = a.gx * t.n + a.gy;
        if (st.food_by_slot) c = t.cell_slot[c];            // a cell outside the list never holds more than 1e-2: nothing to eat
        const size_t g = c >= 0 ? fidx(st, e, c) : 0;
        double r = 0.0;
        const double f = c >= 0 ? st.cur_food[g] : 0.0;
        if (f > 1.0e-2) {                                   // :71-75
            r = f;
            st.wait_refresh[g] = 1;
            st.cur_food[g] = 0.0;
        }
        a.life += r + t.step_reward;                        // :78
        if (t.max_life < a.life) a.life = t.max_life;       // :79
        reward = r;
        return (a.life < 0.0) || (a.steps > max_steps - 1); // :80, :191-192
    }
    const int goal = (t.gx == a.gx) && (t.gy == a.gy);
    reward = t.step_reward + goal * t.goal_reward;          // :92
    return goal || (a.steps > max_steps - 1);
}

// evaluation_rule :83-88 — food revival over the cells c = first, first+stride, ...
// A cell whose task entry has food_interval == 0 can never hold food (food_interval =
// interval * (food_rewards > 1e-3), maze_task.py:172): its wait flag stays 0 and its counter stays
// 0, so skipping it is exact and saves the HBM round trip for the ~95 % of cells that are empty.
__device__ __forceinline__ void eval_cells(const Task &t, const mg_maze_state &st, int e, int first, int stride) {
    if (st.food_by_slot) {
        // Only a WAITING slot changes: revival -= wait leaves a slot that is not waiting as it is, and its counter cannot be
        // negative (it is >= 0 after every reset and renewal and only counts down while waiting; mg_maze_state documents the
        // invariant and load_state_dict checks it). So the common case is one byte read per slot — no counter read, no store.
        for (int k = first; k < t.n_food; k += stride) {
            const size_t i = fidx(st, e, k);
            if (st.wait_refresh[i] == 0) continue;
            int rv = st.revival[i] - 1;
            if (rv < 0) {
                st.cur_food[i] = t.slot_food[(size_t)k * t.slot_stride];
                rv = t.slot_interval[(size_t)k * t.slot_stride];
                st.wait_refresh[i] = 0;
            }
            st.revival[i] = rv;
        }
        return;
    }
    for (int k = first; k < t.n_food; k += stride) {
        const int c = t.food_cells ? (int)t.food_cells[k] : k;
        const int interval = t.interval[c];
        if (interval == 0 && !(t.food[c] > 1.0e-2)) continue;
        const size_t i = fidx(st, e, c);
        int rv = st.revival[i] - (int)st.wait_refresh[i];
        if (rv < 0) {
            st.cur_food[i] = t.food[c];
            rv = interval;
            st.wait_refresh[i] = 0;
        }
        st.revival[i] = rv;
    }
}

// ------------------------------------------------------------------------------------------------
// one env step: what every kernel that steps shares
// ------------------------------------------------------------------------------------------------

// MazeCore2D.do_action maze_2d.py:24-29
__device__ __forceinline__ void move_2d(const Task &t, int act, Agent &a) {
    // DISCRETE_ACTIONS maze_env.py:14 = [(-1,0),(1,0),(0,-1),(0,1)]
    const int ti = a.gx + (act == 0 ? -1 : (act == 1 ? 1 : 0));
    const int tj = a.gy + (act == 2 ? -1 : (act == 3 ? 1 : 0));
    const int wi = ti < 0 ? ti + t.n : ti, wj = tj < 0 ? tj + t.n : tj;   // python negative index
    if (wi < t.n && wj < t.n && t.walls[wi * t.n + wj] < 1) { a.gx = ti; a.gy = tj; }
}

struct RolloutOut {                         // the per-env results of a closed-loop launch
    float *obs_last;                        // [n][w][w] (2-D only)
    double *ret_total, *ret_episode;        // [n]
    int32_t *episode_len, *episodes;        // [n]
};
struct RolloutRec {                         // [T][n] each, obs [K][n][w][w] (2-D only); each may be null
    void *actions;                          // int32, or float32 [T][n][2] for the continuous maze
    float *reward;
    double *reward64;
    uint8_t *done;
    float *obs;
};

// The returns of a launch: float64 sums in step order; the episode's stops with the first done ("the episode has ended" is
// episodes > 0). A kernel that steps a stretch of a rollout picks them up from `po` and leaves them there.
struct Returns {
    double ret_total = 0.0, ret_episode = 0.0;
    int episode_len = 0, episodes = 0;
    __device__ __forceinline__ void add(double r, int d) {
        ret_total = ret_total + r;
        if (episodes == 0) {
            ret_episode = ret_episode + r;
            episode_len += 1;
        }
        episodes += d;
    }
    __device__ __forceinline__ void load(const RolloutOut &po, int e) {
        ret_total = po.ret_total[e];
        ret_episode = po.ret_episode[e];
        episode_len = po.episode_len[e];
        episodes = po.episodes[e];
    }
    __device__ __forceinline__ void store(const RolloutOut &po, int e) const {
        po.ret_total[e] = ret_total;
        po.ret_episode[e] = ret_episode;
        po.episode_len[e] = episode_len;
        po.episodes[e] = episodes;
    }
};

// The step after the move, by the lane that owns env e alone: evaluation_rule (maze_base.py:65-95), the records that are asked
// for at index `at`, and the auto-reset. reset_agent writes only the Agent in registers; reset_cells(..., false) reads only the
// task and writes only the SURVIVAL arrays: the two commute, and this is the one order. Returns done, the reward in `r`.
__device__ __forceinline__ int step_tail(const Task &t, const mg_maze_state &st, int e, int task_type, int max_steps,
                                         int auto_reset, Agent &a, size_t at, float *reward, double *reward64, uint8_t *done,
                                         double &r) {
    const int d = eval_scalar(t, st, e, task_type, max_steps, a, r);
    if (task_type == MG_MAZE_SURVIVAL) eval_cells(t, st, e, 0, 1);          // :83-88
    if (reward) reward[at] = (float)r;
    if (reward64) reward64[at] = r;
    if (done) done[at] = (uint8_t)d;
    if (d && auto_reset) {
        reset_agent(t, task_type, a);
        if (task_type == MG_MAZE_SURVIVAL) reset_cells(t, st, e, 0, 1, false);
    }
    return d;
}

// Which steps of a rollout leave an observation: obs_every = 0 the last one only, k >= 1 the steps t with (t + 1) % k == 0 and
// always the last one (metamaze/maze_env.py rollout_obs_steps restates the rule for the host).
__host__ __device__ __forceinline__ bool rollout_records(int t, int n_steps, int obs_every) {
    return t == n_steps - 1 || (obs_every > 0 && (t + 1) % obs_every == 0);
}

// update_observation maze_2d.py:89-121; `put(i, v)` receives window entry i.
template <class Put>
__device__ __forceinline__ void observe_2d(const Task &t, const mg_maze_state &st, int e, int task_type, int vg, const Agent &a,
                                           Put &&put) {
    const int w = 2 * vg + 1;
    for (int p = 0; p < w; ++p)
        for (int q = 0; q < w; ++q) {
            const int x = a.gx - vg + p, y = a.gy - vg + q;
            float v = -1.0f;
            if (x >= 0 && x < t.n && y >= 0 && y < t.n) {
                v = (float)(-(int)t.walls[x * t.n + y]);                                   // :113
                if (task_type == MG_MAZE_SURVIVAL) {                                       // :117
                    double food;
                    if (st.food_by_slot) {
                        // (-1: not a food cell and its task value is exactly 0.0 — nothing to read; -2: not a food cell, a
                        // nonzero value <= 1e-2 that never changes)
                        const int k = t.cell_slot[x * t.n + y];
                        food = k >= 0 ? st.cur_food[fidx(st, e, k)] : (k == -1 ? 0.0 : t.food[x * t.n + y]);
                    } else food = st.cur_food[fidx(st, e, x * t.n + y)];
                    v = (float)((double)v + food);
                }
                else v = (float)((double)v + ((x == t.gx && y == t.gy) ? 1.0 : 0.0));       // :120
            }
            if (task_type == MG_MAZE_SURVIVAL && p == vg && q == vg) v = (float)a.life;     // :118
            put(p * w + q, v);
        }
}

// ------------------------------------------------------------------------------------------------
// 3-D transitions (executed by one thread of the env's workgroup)
// ------------------------------------------------------------------------------------------------

__device__ __forceinline__ void transition_discrete(const Task &t, int act, Agent &a) {
    const int turn = act == 0 ? -1 : (act == 1 ? 1 : 0);      // maze_env.py:14
    const int step = act == 2 ? -1 : (act == 3 ? 1 : 0);
    a.ori_idx = (a.ori_idx + turn) & 3;                        // maze_discrete_3d.py:69-72
    int g0 = a.gx, g1 = a.gy;                                  // :51-67
    if (a.ori_idx == 0) g0 += step;
    else if (a.ori_idx == 1) g1 += step;
    else if (a.ori_idx == 2) g0 -= step;
    else g1 -= step;
    if (g0 >= 0 && g0 < t.n && g1 >= 0 && g1 < t.n && t.walls[g0 * t.n + g1] == 0) { a.gx = g0; a.gy = g1; }
}

__device__ __forceinline__ float nearest_point(const float *pos, const float *l1, const float *l2, float *np_out) {
    // dynamics.py:17-29
    float u0 = l2[0] - l1[0], u1 = l2[1] - l1[1];
    const float edge_norm = sqrtf(u0 * u0 + u1 * u1);
    const double m = (1.0e-6 > (double)edge_norm) ? 1.0e-6 : (double)edge_norm;
    u0 = (float)((double)u0 / m);
    u1 = (float)((double)u1 / m);
    const float dist_1 = (pos[0] - l1[0]) * u0 + (pos[1] - l1[1]) * u1;
    float p0, p1;
    if (dist_1 > edge_norm) { p0 = l2[0]; p1 = l2[1]; }
    else if (dist_1 < 0) { p0 = l1[0]; p1 = l1[1]; }
    else { p0 = l1[0] + dist_1 * u0; p1 = l1[1] + dist_1 * u1; }
    const float d0 = pos[0] - p0, d1 = pos[1] - p1;
    np_out[0] = p0;
    np_out[1] = p1;
    return sqrtf(d0 * d0 + d1 * d1);
}

__device__ __forceinline__ void collision_force(const float *dv, double cell_size, double col_dist, float *out) {
    // dynamics.py:32-56
    const double dist = (double)sqrtf(dv[0] * dv[0] + dv[1] * dv[1]);
    const double eff = col_dist / cell_size;
    out[0] = out[1] = 0.0f;
    if (dist > 0.708 + eff) return;
    if (fabsf(dv[0]) < 0.5f && fabsf(dv[1]) < 0.5f) {
        const double mx = dist > 1.0e-6 ? dist : 1.0e-6;
        const float k = (float)(0.50 / mx * (0.708 + eff - dist) * cell_size);
        out[0] = k * dv[0];
        out[1] = k * dv[1];
        return;
    }
    const bool x_pos = (dv[0] + dv[1]) > 0, y_pos = (dv[1] - dv[0]) > 0;
    const float A[2] = {0.5f, 0.5f}, B[2] = {-0.5f, 0.5f}, C[2] = {-0.5f, -0.5f}, D[2] = {0.5f, -0.5f};
    float np_[2], d;
    if (x_pos && y_pos) d = nearest_point(dv, A, B, np_);
    else if (!x_pos && y_pos) d = nearest_point(dv, B, C, np_);
    else if (!x_pos && !y_pos) d = nearest_point(dv, C, D, np_);
    else d = nearest_point(dv, D, A, np_);
    if (eff < (double)d) return;
    float o0 = dv[0] - np_[0], o1 = dv[1] - np_[1];
    const float on = sqrtf(o0 * o0 + o1 * o1);
    const double r = 1.0 / ((1.0e-6 > (double)on) ? 1.0e-6 : (double)on);
    o0 = (float)((double)o0 * r);
    o1 = (float)((double)o1 * r);
    const float k = (float)(0.50 * (eff - (double)d) * cell_size);
    out[0] = k * o0;
    out[1] = k * o1;
}

__device__ __forceinline__ void transition_continuous(const Task &t, double col_dist, float turn, float walk,
                                                      Agent &a) {
    // maze_continuous_3d.py:47-56 + dynamics.py:59-92
    const double PI = 3.1415926, t_PI = 6.2831852;
    const double tr = (double)turn, ws = (double)walk;
    const double turn_rate = (tr < -1 ? -1 : (tr > 1 ? 1 : tr)) * PI;
    double walk_speed = ws < -1 ? -1 : (ws > 1 ? 1 : ws);
    if (walk_speed < 0) walk_speed *= 0.50;
    double ori = a.ori;
    float p0 = a.lx, p1 = a.ly;
    const float cs32 = (float)t.cell_size;
    for (int it = 0; it < 10; ++it) {   // int(100 * 0.10)
        double fin = ori + turn_rate * 0.01;
        const double off_ori = 0.5 * (fin + ori);
        const double off = walk_speed * 0.01;
        const float d_x = (float)(cos(off_ori) * off), d_y = (float)(sin(off_ori) * off);
        while (fin > t_PI) fin -= t_PI;
        while (fin < 0) fin += t_PI;
        ori = fin;
        const float e0 = p0 + d_x, e1 = p1 + d_y;
        const float c0 = e0 / cs32, c1 = e1 / cs32;
        float col0 = 0.0f, col1 = 0.0f;
        for (int i = -1; i < 2; ++i)
            for (int j = -1; j < 2; ++j) {
                const int w_i = i + (int)c0, w_j = j + (int)c1;
                if (w_i > -1 && w_i < t.n && w_j > -1 && w_j < t.n && t.walls[w_i * t.n + w_j] > 0) {
                    float cd[2], f[2];
                    cd[0] = (c0 - floorf(c0)) - ((float)i + 0.5f);
                    cd[1] = (c1 - floorf(c1)) - ((float)j + 0.5f);
                    collision_force(cd, t.cell_size, col_dist, f);
                    col0 += f[0];
                    col1 += f[1];
                }
            }
        p0 = col0 + e0;
        p1 = col1 + e1;
    }
    a.ori = ori;
    a.lx = p0;
    a.ly = p1;
    a.gx = (int)(p0 / cs32);   // get_loc_grid maze_base.py:199-202
    a.gy = (int)(p1 / cs32);
}

int check_tasks(const mg_maze_tasks *T, int task_type) {
    if (T->n < 3 || T->n > 255 || T->n_tasks < 1) return mg::set_error(MG_ERR_BAD_SIZE, "maze n=%d n_tasks=%d", T->n, T->n_tasks);
    if (!T->start || !T->goal || !T->walls || !T->texts || !T->scalars)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_maze_tasks has a NULL array");
    if (task_type == MG_MAZE_SURVIVAL && (!T->food_rewards || !T->food_interval))
        return mg::set_error(MG_ERR_NULL_POINTER, "SURVIVAL needs food_rewards and food_interval");
    if (task_type != MG_MAZE_SURVIVAL && task_type != MG_MAZE_ESCAPE)
        return mg::set_error(MG_ERR_BAD_CONFIG, "task_type %d", task_type);
    // food_cells / cell_slot hold int16 cell indices: past 32 768 cells they would wrap negative and the kernels would index
    // the food arrays out of bounds
    if ((T->food_cells || T->cell_slot) && T->n * T->n > 32768)
        return mg::set_error(MG_ERR_BAD_SIZE, "maze n=%d has %d cells: mg_maze_tasks.food_cells / cell_slot index at most 32 768 "
                             "(n <= 181); pass NULL lists and the SURVIVAL arrays by cell", T->n, T->n * T->n);
    return MG_OK;
}

int check_mstate(const mg_maze_state *s, int task_type) {
    if (!s->task_id || !s->grid || !s->steps) return mg::set_error(MG_ERR_NULL_POINTER, "mg_maze_state has a NULL array");
    if (task_type == MG_MAZE_SURVIVAL && (!s->life || !s->cur_food || !s->wait_refresh || !s->revival))
        return mg::set_error(MG_ERR_NULL_POINTER, "SURVIVAL needs life / cur_food / wait_refresh / revival");
    return MG_OK;
}

int check_slots(const mg_maze_tasks *T, const mg_maze_state *s, int task_type) {
    if (task_type == MG_MAZE_SURVIVAL && s->food_by_slot &&
        (!T->food_cells || !T->n_food || !T->cell_slot || !T->slot_food || !T->slot_interval || T->max_food < 1))
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_maze_state.food_by_slot needs mg_maze_tasks.food_cells / n_food / cell_slot / "
                             "slot_food / slot_interval");
    return MG_OK;
}

}  // namespace
