// maze_expert.hip — MetaMaze shortest-path fields and the expert that descends them (mg_maze_distance_field,
// mg_maze_expert_action, mg_maze2d_expert_rollout, mg_maze_steer_action, mg_maze3d_expert_rollout).
//
// A translation unit of its own on maze_core.h (load_task, load_agent, transition_discrete, transition_continuous, move_2d,
// step_tail, eval_scalar, eval_cells, reset_cells, reset_agent, Returns, observe_2d, rollout_records, the host checks). Same
// flags (metagym_amd/build.py).
//
// The field. dist[t][k][c] is the length of the shortest action sequence that takes state (k, c) of task t onto a source cell
// under the step's own passability rule (include/metagym_hip.h states the three rules). One workgroup per task runs a
// level-synchronous breadth-first search BACKWARDS from the sources: level L holds the states at distance L, and every state
// of it claims its still unreached predecessors for level L + 1 with a compare-and-swap of -1 -> L + 1 on the field, so each
// state is claimed by exactly one lane and enters the next level's queue exactly once. Two queues and three counters rotate
// in LDS; one barrier ends a level. A level that outgrows the queue is not stored: the lanes then find it by scanning the
// field for the value L (every state of the level carries it, queued or not), so nothing is ever dropped. The loop runs at
// most K * n * n levels and leaves earlier only when a level is empty, which is exact: an empty level has no successors.
// The field lives in LDS while K * n * n int32 fit beside the queues and is copied out at the end; above that it lives in
// `dist` itself, read and written with agent-scope atomics only (they are served by the L2 the workgroup's CU hangs on, so no
// lane ever meets a stale vector-L1 line). No workgroup talks to another.
//
// The expert. One lane per env looks at the (at most four) successors of the env's state under the step's own rule and takes
// the lowest action whose successor is one step nearer; mg_maze2d_expert_rollout is maze2d_rollout_kernel's step (move_2d,
// step_tail) with the action load replaced by that choice.
//
// The 3-D demonstrations (mg_maze_steer_action, mg_maze3d_expert_rollout). The continuous maze's expert steers: towards the
// centre of the first neighbour cell one step nearer in a CELLS_3D field, walking inside a +-9 degree dead band and turning
// otherwise, every decision a comparison (me_steer_pick). mg_maze3d_expert_rollout follows mg_maze3d_rollout's launch pattern:
// per recorded frame one lane-per-env launch of maze3d_advance_kernel's body with the action load replaced by the pick
// (maze3d_expert_advance_kernel), then the untouched renderer through mg_maze3d_step's observe-only form.
#include "maze_core.h"

#include "mg_closed_loop.h"

namespace {

constexpr int ME_BLOCK = 256;                    // threads of a field workgroup
constexpr int ME_QUEUE_CAP = 2048;               // states one level's queue holds (mg_maze_distance_queue_capacity)
constexpr int ME_ROLL_BLOCK = mg::WAVE;

__host__ __device__ constexpr int me_orientations(int kind) { return kind == MG_MAZE_FIELD_TURNS ? 4 : 1; }

// The dynamic LDS of one field workgroup, in bytes from its 16-byte aligned base: three level counters, two queues, and the
// field when it fits. One function for the launch and the kernel.
struct MeLds { int count, queue0, queue1, field, bytes; bool field_in_lds; };
__host__ __device__ inline MeLds me_lds_layout(int states) {
    MeLds l;
    l.count = 0;
    l.queue0 = 16;
    l.queue1 = l.queue0 + ME_QUEUE_CAP * (int)sizeof(int32_t);
    l.field = l.queue1 + ME_QUEUE_CAP * (int)sizeof(int32_t);
    l.field_in_lds = (size_t)l.field + (size_t)states * sizeof(int32_t) <= mg::LDS_LIMIT;
    l.bytes = l.field + (l.field_in_lds ? states * (int)sizeof(int32_t) : 0);
    return l;
}

// The field of one task while it is built: LDS words, or the task's slice of `dist` behind agent-scope atomics.
template <bool IN_LDS>
struct Field {
    int32_t *p;
    __device__ __forceinline__ void put(int s, int32_t v) const {
        if (IN_LDS) p[s] = v;
        else __hip_atomic_store(p + s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ int32_t get(int s) const {
        if (IN_LDS) return p[s];
        return __hip_atomic_load(p + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // true for the one lane that turns s from unreached into level `v`
    __device__ __forceinline__ bool claim(int s, int32_t v) const {
        int32_t expected = -1;
        return __hip_atomic_compare_exchange_strong(p + s, &expected, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                    IN_LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT);
    }
    // every lane's field accesses of this level are done before any lane starts the next one
    __device__ __forceinline__ void level_barrier() const {
        if (!IN_LDS) __threadfence();
        __syncthreads();
    }
};

// MOVES_2D: maze_2d.py:27 (walls < 1); CELLS_3D and TURNS: maze_discrete_3d.py:63-65 (walls == 0)
__device__ __forceinline__ bool me_passable(int kind, int8_t w) { return kind == MG_MAZE_FIELD_MOVES_2D ? w < 1 : w == 0; }

template <bool IN_LDS>
__global__ __launch_bounds__(ME_BLOCK) void maze_distance_field_kernel(mg_maze_tasks T, int kind, const uint8_t *sources,
                                                                       int32_t *dist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = T.n, nn = n * n, K = me_orientations(kind), S = K * nn;
    const MeLds lds = me_lds_layout(S);
    int32_t *count = reinterpret_cast<int32_t *>(smem + lds.count);          // [3]: the level's, the next one's, a spare at 0
    int32_t *queue[2] = {reinterpret_cast<int32_t *>(smem + lds.queue0), reinterpret_cast<int32_t *>(smem + lds.queue1)};
    const int t = blockIdx.x, tid = threadIdx.x;
    const int8_t *walls = T.walls + (size_t)t * nn;
    int32_t *out = dist + (size_t)t * S;
    const Field<IN_LDS> f{IN_LDS ? reinterpret_cast<int32_t *>(smem + lds.field) : out};

    // put state s into the queue of the level that `slot` counts; past the capacity only the count grows
    auto enqueue = [&](int slot, int32_t *q, int s) {
        const int i = atomicAdd(&count[slot], 1);
        if (i < ME_QUEUE_CAP) q[i] = s;
    };

    if (tid < 3) count[tid] = 0;
    for (int s = tid; s < S; s += ME_BLOCK) f.put(s, -1);
    f.level_barrier();
    // level 0: the source cells in every orientation (a cell belongs to one lane, so no claim is needed)
    if (sources != nullptr) {
        const uint8_t *src = sources + (size_t)t * nn;
        for (int c = tid; c < nn; c += ME_BLOCK)
            if (src[c] != 0)
                for (int k = 0; k < K; ++k) { f.put(k * nn + c, 0); enqueue(0, queue[0], k * nn + c); }
    } else if (tid < K) {
        const int gx = T.goal[2 * t], gy = T.goal[2 * t + 1];
        if (gx >= 0 && gx < n && gy >= 0 && gy < n) { f.put(tid * nn + gx * n + gy, 0); enqueue(0, queue[0], tid * nn + gx * n + gy); }
    }
    f.level_barrier();

    // A state of level L claims its predecessors: the states from which ONE action leads to it. Entering a cell needs the
    // cell passable; where the agent comes from does not matter to the step, so a wall cell next to a free one has a distance.
    for (int L = 0; L < S; ++L) {
        const int cur = L % 3, nxt = (L + 1) % 3;
        const int n_cur = count[cur];
        if (n_cur == 0) break;                                               // (uniform) nothing is at distance L: done
        if (tid == 0) count[(L + 2) % 3] = 0;                                // level L - 1's count: every lane read it before the last barrier
        int32_t *q_cur = queue[L & 1], *q_nxt = queue[(L + 1) & 1];
        auto expand = [&](int s) {
            const int o = s / nn, c = s - o * nn, x = c / n, y = c - x * n;
            auto pred = [&](int ps) { if (f.claim(ps, L + 1)) enqueue(nxt, q_nxt, ps); };
            if (kind == MG_MAZE_FIELD_TURNS) {
                pred(((o + 1) & 3) * nn + c);                                // turn -1 ends here from o + 1
                pred(((o + 3) & 3) * nn + c);                                // turn +1 from o - 1
                if (!me_passable(kind, walls[c])) return;
                // maze_discrete_3d.py:51-60: heading 0 is +x, 1 +y, 2 -x, 3 -y; forward came from c - d, backward from c + d
                const int dx = o == 0 ? 1 : (o == 2 ? -1 : 0), dy = o == 1 ? 1 : (o == 3 ? -1 : 0);
                if (x - dx >= 0 && x - dx < n && y - dy >= 0 && y - dy < n) pred(o * nn + (x - dx) * n + (y - dy));
                if (x + dx >= 0 && x + dx < n && y + dy >= 0 && y + dy < n) pred(o * nn + (x + dx) * n + (y + dy));
            } else {
                if (!me_passable(kind, walls[c])) return;
                if (x > 0) pred(c - n);
                if (x < n - 1) pred(c + n);
                if (y > 0) pred(c - 1);
                if (y < n - 1) pred(c + 1);
            }
        };
        if (n_cur <= ME_QUEUE_CAP) {
            for (int i = tid; i < n_cur; i += ME_BLOCK) expand(q_cur[i]);
        } else {                                                             // the level did not fit the queue: find it in the field
            for (int s = tid; s < S; s += ME_BLOCK)
                if (f.get(s) == L) expand(s);
        }
        f.level_barrier();
    }
    if (IN_LDS) {
        __syncthreads();
        for (int s = tid; s < S; s += ME_BLOCK) out[s] = f.p[s];
    }
}

// The expert's action in state (ori, gx, gy): the lowest a whose successor under the step's own rule is one step nearer in
// `field` ([K][n*n], the task's slice). 0 when there is none, when the state is off the grid, on a source or unreachable.
// The four actions are looked at from the highest down, whatever d0 is, with loads that do not wait for one another; the
// lowest descending action is the last one kept.
__device__ __forceinline__ int me_expert_pick(const Task &t, int kind, const int32_t *field, int gx, int gy, int ori) {
    if (gx < 0 || gx >= t.n || gy < 0 || gy >= t.n) return 0;
    int best = 0;
    if (kind == MG_MAZE_FIELD_TURNS) {
        ori &= 3;
        const int d0 = field[ori * t.nn + gx * t.n + gy];
#pragma unroll
        for (int act = 3; act >= 0; --act) {
            Agent a;
            a.gx = gx; a.gy = gy; a.ori_idx = ori;
            transition_discrete(t, act, a);                                  // (stays on the grid)
            if (field[a.ori_idx * t.nn + a.gx * t.n + a.gy] == d0 - 1) best = act;
        }
        return d0 > 0 ? best : 0;
    }
    // maze_2d.py:24-29 as maze2d_step_kernel states it: the move into (ti, tj) happens iff walls < 1 there, else the agent
    // stays (and is no nearer). A target off the grid is no candidate: through python's negative index the step would take
    // it where the border cell opposite is free, but the field knows no such state. So a candidate's target is on the grid,
    // and its wall and its distance are read at once, from an address that does not depend on either.
    const int c = gx * t.n + gy, d0 = field[c];
#pragma unroll
    for (int act = 3; act >= 0; --act) {
        const int ti = gx + (act == 0 ? -1 : (act == 1 ? 1 : 0));
        const int tj = gy + (act == 2 ? -1 : (act == 3 ? 1 : 0));
        const bool in = ti >= 0 && ti < t.n && tj >= 0 && tj < t.n;
        const int tc = in ? ti * t.n + tj : c;
        const int8_t w = t.walls[tc];
        const int ds = field[tc];
        if (in && w < 1 && ds == d0 - 1) best = act;
    }
    return d0 > 0 ? best : 0;
}

__global__ __launch_bounds__(ME_BLOCK) void maze_expert_action_kernel(mg_maze_tasks T, int kind, const int32_t *dist, int n_envs,
                                                                      mg_maze_state st, int32_t *action) {
    const int e = blockIdx.x * ME_BLOCK + threadIdx.x;
    if (e >= n_envs) return;
    const int tid = mg::clamp_index(st.task_id[e], T.n_tasks);
    const Task t = load_task(T, tid);
    const int32_t *field = dist + (size_t)tid * me_orientations(kind) * t.nn;
    action[e] = me_expert_pick(t, kind, field, st.grid[e], st.grid[n_envs + e], st.ori_idx ? st.ori_idx[e] : 0);
}

// maze2d_rollout_kernel's step (move_2d, step_tail), one lane per env, one wave per workgroup, the action chosen from the field
// on the state the lane holds. Inside the step loop the kernel stores only what `rec` asks for.
__global__ __launch_bounds__(ME_ROLL_BLOCK) void maze2d_expert_rollout_kernel(mg_maze_tasks T, mg_maze_state st, int task_type,
                                                                              int max_steps, int vg, int auto_reset, int n_envs,
                                                                              int n_steps, int obs_every, const int32_t *dist,
                                                                              RolloutOut po, RolloutRec rec) {
    const int e = blockIdx.x * ME_ROLL_BLOCK + threadIdx.x;
    if (e >= n_envs) return;
    const int tid = mg::clamp_index(st.task_id[e], T.n_tasks);
    const Task t = load_task(T, tid);
    const int32_t *field = dist + (size_t)tid * t.nn;
    Agent a = load_agent(st, n_envs, e);
    const int ww = (2 * vg + 1) * (2 * vg + 1);
    const size_t slice = (size_t)n_envs * ww;
    float *out = rec.obs;
    Returns ret;
    for (int s = 0; s < n_steps; ++s) {
        const size_t r_at = (size_t)s * n_envs + e;
        const int act = me_expert_pick(t, MG_MAZE_FIELD_MOVES_2D, field, a.gx, a.gy, 0);
        if (rec.actions) static_cast<int32_t *>(rec.actions)[r_at] = act;
        move_2d(t, act, a);
        double r;
        const int d = step_tail(t, st, e, task_type, max_steps, auto_reset, a, r_at, rec.reward, rec.reward64, rec.done, r);
        ret.add(r, d);
        if (out == nullptr || !rollout_records(s, n_steps, obs_every)) continue;
        float *o = out + (size_t)e * ww;
        observe_2d(t, st, e, task_type, vg, a, [&](int i, float v) { o[i] = v; });
        out += slice;
    }
    store_agent(st, n_envs, e, a);
    float *o = po.obs_last + (size_t)e * ww;
    observe_2d(t, st, e, task_type, vg, a, [&](int i, float v) { o[i] = v; });
    ret.store(po, e);
}

// The steering expert's action in the state `a` holds (include/metagym_hip.h states the rule; metamaze/expert.py
// steer_action_reference is the definition): (0, 0), (0, 1) or (+-1, 0), every decision a comparison. `field` is the task's
// [n*n] slice of a CELLS_3D field. d0 and the four neighbours' walls and distances are read at once, from addresses that
// depend on the cell alone, as in me_expert_pick; the lowest descending neighbour is the last one kept.
__device__ __forceinline__ void me_steer_pick(const Task &t, const int32_t *field, const Agent &a, float &turn, float &walk) {
    turn = 0.0f;
    walk = 0.0f;
    if (a.gx < 0 || a.gx >= t.n || a.gy < 0 || a.gy >= t.n) return;
    const int c = a.gx * t.n + a.gy, d0 = field[c];
    int best = -1;
#pragma unroll
    for (int act = 3; act >= 0; --act) {
        const int ti = a.gx + (act == 0 ? -1 : (act == 1 ? 1 : 0));
        const int tj = a.gy + (act == 2 ? -1 : (act == 3 ? 1 : 0));
        const bool in = ti >= 0 && ti < t.n && tj >= 0 && tj < t.n;
        const int tc = in ? ti * t.n + tj : c;
        const int8_t w = t.walls[tc];
        const int ds = field[tc];
        if (in && w == 0 && ds == d0 - 1) best = act;
    }
    if (d0 <= 0 || best < 0) return;
    const int tx = a.gx + (best == 0 ? -1 : (best == 1 ? 1 : 0));
    const int ty = a.gy + (best == 2 ? -1 : (best == 3 ? 1 : 0));
    const float cs = (float)t.cell_size;
    const float px = ((float)tx + 0.5f) * cs, py = ((float)ty + 0.5f) * cs;   // the target cell's centre
    const double vx = (double)(px - a.lx), vy = (double)(py - a.ly);
    // the heading as the renderer takes it (es->s_ori = sin(a.ori)), rounded to float32: a last-bit difference between two
    // libms cannot move a comparison, and the four products below are exact in float64
    const double hx = (double)(float)cos(a.ori), hy = (double)(float)sin(a.ori);
    const double cr = hx * vy - hy * vx, dt = hx * vx + hy * vy;
    const double TAN9 = (double)0.15838444f;                                  // tan(9 deg): half of one step's 18 deg turn
    if (dt > 0.0 && fabs(cr) <= TAN9 * dt) walk = 1.0f;
    else turn = cr >= 0.0 ? 1.0f : -1.0f;
}

__global__ __launch_bounds__(ME_BLOCK) void maze_steer_action_kernel(mg_maze_tasks T, const int32_t *dist, int n_envs,
                                                                     mg_maze_state st, float *action) {
    const int e = blockIdx.x * ME_BLOCK + threadIdx.x;
    if (e >= n_envs) return;
    const int tid = mg::clamp_index(st.task_id[e], T.n_tasks);
    const Task t = load_task(T, tid);
    Agent a;
    a.gx = st.grid[e];
    a.gy = st.grid[n_envs + e];
    a.lx = st.loc[e];
    a.ly = st.loc[n_envs + e];
    a.ori = st.ori[e];
    float turn, walk;
    me_steer_pick(t, dist + (size_t)tid * t.nn, a, turn, walk);
    action[2 * (size_t)e] = turn;
    action[2 * (size_t)e + 1] = walk;
}

struct Me3Out {
    double *ret_total, *ret_episode;        // [n]
    int32_t *episode_len, *episodes;        // [n]
};
struct Me3Rec {                             // [T][n] each (continuous actions [T][n][2]); each may be null
    void *actions;
    float *reward;
    double *reward64;
    uint8_t *done;
};

// maze3d_advance_kernel's body in its order (step_tail and Returns written out: through the helpers the continuous form
// measured 1.6 % slower than before) for the steps s0 .. s1-1 of a demonstration, one lane per env, one wave per
// workgroup, the agent in registers, the action chosen from the field on the state the lane holds. The returns travel from
// stretch to stretch through `po`: the stretch that starts at step 0 begins them, a later one picks them up; "the episode has
// ended" is episodes > 0. Inside the step loop the kernel stores only what `rec` asks for.
template <bool CONT>
__global__ __launch_bounds__(ME_ROLL_BLOCK) void maze3d_expert_advance_kernel(mg_maze_tasks T, mg_maze_state st, double col_dist,
                                                                              int task_type, int max_steps, int auto_reset,
                                                                              int n_envs, int s0, int s1, const int32_t *dist,
                                                                              Me3Out po, Me3Rec rec) {
    const int e = blockIdx.x * ME_ROLL_BLOCK + threadIdx.x;
    if (e >= n_envs) return;
    const int tid = mg::clamp_index(st.task_id[e], T.n_tasks);
    const Task t = load_task(T, tid);
    const int32_t *field = dist + (size_t)tid * (CONT ? 1 : 4) * t.nn;
    Agent a = load_agent(st, n_envs, e);
    double ret_total = 0.0, ret_episode = 0.0;
    int episode_len = 0, episodes = 0;
    if (s0 > 0) {
        ret_total = po.ret_total[e];
        ret_episode = po.ret_episode[e];
        episode_len = po.episode_len[e];
        episodes = po.episodes[e];
    }
    for (int s = s0; s < s1; ++s) {
        const size_t r_at = (size_t)s * n_envs + e;
        if (CONT) {
            float turn, walk;
            me_steer_pick(t, field, a, turn, walk);
            if (rec.actions) {
                float *ac = static_cast<float *>(rec.actions) + 2 * r_at;
                ac[0] = turn;
                ac[1] = walk;
            }
            transition_continuous(t, col_dist, turn, walk, a);
        } else {
            const int act = me_expert_pick(t, MG_MAZE_FIELD_TURNS, field, a.gx, a.gy, a.ori_idx);
            if (rec.actions) static_cast<int32_t *>(rec.actions)[r_at] = act;
            transition_discrete(t, act, a);
        }
        double r;
        const int d = eval_scalar(t, st, e, task_type, max_steps, a, r);
        if (task_type == MG_MAZE_SURVIVAL) eval_cells(t, st, e, 0, 1);
        if (rec.reward) rec.reward[r_at] = (float)r;
        if (rec.reward64) rec.reward64[r_at] = r;
        if (rec.done) rec.done[r_at] = (uint8_t)d;
        if (d && auto_reset) {
            if (task_type == MG_MAZE_SURVIVAL) reset_cells(t, st, e, 0, 1, false);
            reset_agent(t, task_type, a);
        }
        // the returns: float64 sums in step order; the episode's stops with the first done
        ret_total = ret_total + r;
        if (episodes == 0) {
            ret_episode = ret_episode + r;
            episode_len += 1;
        }
        episodes += d;
    }
    store_agent(st, n_envs, e, a);
    po.ret_total[e] = ret_total;
    po.ret_episode[e] = ret_episode;
    po.episode_len[e] = episode_len;
    po.episodes[e] = episodes;
}

int check_kind(int32_t kind, const char *who) {
    if (kind != MG_MAZE_FIELD_MOVES_2D && kind != MG_MAZE_FIELD_CELLS_3D && kind != MG_MAZE_FIELD_TURNS)
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: kind=%d is none of MG_MAZE_FIELD_MOVES_2D / CELLS_3D / TURNS", who, kind);
    return MG_OK;
}

}  // namespace

extern "C" int32_t mg_maze_distance_queue_capacity(void) { return ME_QUEUE_CAP; }

extern "C" int mg_maze_distance_field(const mg_maze_tasks *T, int32_t kind, const uint8_t *sources, int32_t *dist, void *stream) {
    MG_REQUIRE_PTR(T);
    MG_REQUIRE_PTR(dist);
    if (int rc = check_kind(kind, "mg_maze_distance_field")) return rc;
    if (int rc = check_tasks(T, MG_MAZE_ESCAPE)) return rc;
    const MeLds lds = me_lds_layout(me_orientations(kind) * T->n * T->n);
    const auto kernel = lds.field_in_lds ? maze_distance_field_kernel<true> : maze_distance_field_kernel<false>;
    mg::DeviceGuard guard(mg::device_of(dist));
    if (int rc = mg::opt_in_dynamic_lds(kernel, lds.bytes, "maze_distance_field_kernel")) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)T->n_tasks), dim3(ME_BLOCK), (size_t)lds.bytes, (hipStream_t)stream, *T, kind, sources,
                       dist);
    return mg::check_launch("maze_distance_field_kernel");
}

extern "C" int mg_maze_expert_action(const mg_maze_tasks *T, int32_t kind, const int32_t *dist, int32_t n,
                                     const mg_maze_state *st, int32_t *action, void *stream) {
    MG_REQUIRE_PTR(T);
    MG_REQUIRE_PTR(dist);
    MG_REQUIRE_PTR(st);
    MG_REQUIRE_PTR(action);
    if (int rc = check_kind(kind, "mg_maze_expert_action")) return rc;
    if (kind == MG_MAZE_FIELD_CELLS_3D)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_maze_expert_action: the continuous maze has no expert (kind MG_MAZE_FIELD_CELLS_3D)");
    if (n <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_envs=%d", n);
    if (int rc = check_tasks(T, MG_MAZE_ESCAPE)) return rc;
    if (int rc = check_mstate(st, MG_MAZE_ESCAPE)) return rc;
    if (kind == MG_MAZE_FIELD_TURNS && st->ori_idx == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_maze_expert_action: MG_MAZE_FIELD_TURNS needs mg_maze_state.ori_idx");
    mg::DeviceGuard guard(mg::device_of(st->grid));
    hipLaunchKernelGGL(maze_expert_action_kernel, dim3((unsigned)((n + ME_BLOCK - 1) / ME_BLOCK)), dim3(ME_BLOCK), 0,
                       (hipStream_t)stream, *T, kind, dist, n, *st, action);
    return mg::check_launch("maze_expert_action_kernel");
}

extern "C" int mg_maze2d_expert_rollout(const mg_maze_tasks *T, int32_t task_type, int32_t max_steps, int32_t view_grid,
                                        int32_t auto_reset, int32_t n, const mg_maze_state *st, int32_t n_steps,
                                        int32_t obs_every, const int32_t *dist, float *obs_last, double *ret_total,
                                        double *ret_episode, int32_t *episode_len, int32_t *episodes, int32_t *actions,
                                        float *reward, double *reward64, uint8_t *done, float *obs, void *stream) {
    MG_REQUIRE_PTR(T);
    MG_REQUIRE_PTR(st);
    MG_REQUIRE_PTR(dist);
    MG_REQUIRE_PTR(obs_last);
    MG_REQUIRE_PTR(ret_total);
    MG_REQUIRE_PTR(ret_episode);
    MG_REQUIRE_PTR(episode_len);
    MG_REQUIRE_PTR(episodes);
    if (n <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_envs=%d", n);
    if (n_steps < 1) return mg::set_error(MG_ERR_BAD_SIZE, "mg_maze2d_expert_rollout: n_steps=%d (at least 1)", n_steps);
    if (obs_every < 0) return mg::set_error(MG_ERR_BAD_SIZE, "mg_maze2d_expert_rollout: obs_every=%d (0 = the last step only, k >= 1 = every k-th)", obs_every);
    if (view_grid < 0) return mg::set_error(MG_ERR_BAD_CONFIG, "mg_maze2d_expert_rollout: view_grid=%d", view_grid);
    if (int rc = check_tasks(T, task_type)) return rc;
    if (int rc = check_mstate(st, task_type)) return rc;
    if (int rc = check_slots(T, st, task_type)) return rc;
    mg::DeviceGuard guard(mg::device_of(st->grid));
    RolloutOut po{obs_last, ret_total, ret_episode, episode_len, episodes};
    RolloutRec rec{actions, reward, reward64, done, obs};
    hipLaunchKernelGGL(maze2d_expert_rollout_kernel, dim3((unsigned)((n + ME_ROLL_BLOCK - 1) / ME_ROLL_BLOCK)), dim3(ME_ROLL_BLOCK),
                       0, (hipStream_t)stream, *T, *st, task_type, max_steps, view_grid, auto_reset, n, n_steps, obs_every, dist, po,
                       rec);
    return mg::check_launch("maze2d_expert_rollout_kernel");
}

extern "C" int mg_maze_steer_action(const mg_maze_tasks *T, const int32_t *dist, int32_t n, const mg_maze_state *st, float *action,
                                    void *stream) {
    MG_REQUIRE_PTR(T);
    MG_REQUIRE_PTR(dist);
    MG_REQUIRE_PTR(st);
    MG_REQUIRE_PTR(action);
    if (n <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_envs=%d", n);
    if (int rc = check_tasks(T, MG_MAZE_ESCAPE)) return rc;
    if (int rc = check_mstate(st, MG_MAZE_ESCAPE)) return rc;
    if (st->loc == nullptr || st->ori == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_maze_steer_action needs mg_maze_state.loc and ori");
    mg::DeviceGuard guard(mg::device_of(st->grid));
    hipLaunchKernelGGL(maze_steer_action_kernel, dim3((unsigned)((n + ME_BLOCK - 1) / ME_BLOCK)), dim3(ME_BLOCK), 0,
                       (hipStream_t)stream, *T, dist, n, *st, action);
    return mg::check_launch("maze_steer_action_kernel");
}

extern "C" int mg_maze3d_expert_rollout(const mg_maze_tasks *T, const mg_maze_view *view, int32_t task_type, int32_t max_steps,
                                        int32_t continuous, int32_t auto_reset, int32_t n, const mg_maze_state *st,
                                        int32_t n_steps, int32_t obs_every, const int32_t *dist, void *obs, double *ret_total,
                                        double *ret_episode, int32_t *episode_len, int32_t *episodes, void *actions,
                                        float *reward, double *reward64, uint8_t *done, void *stream) {
    MG_REQUIRE_PTR(dist);
    MG_REQUIRE_PTR(ret_total);
    MG_REQUIRE_PTR(ret_episode);
    MG_REQUIRE_PTR(episode_len);
    MG_REQUIRE_PTR(episodes);
    if (n_steps < 1) return mg::set_error(MG_ERR_BAD_SIZE, "mg_maze3d_expert_rollout: n_steps=%d (at least 1)", n_steps);
    if (obs_every < 0) return mg::set_error(MG_ERR_BAD_SIZE, "mg_maze3d_expert_rollout: obs_every=%d (0 = the last step only, k >= 1 = every k-th)", obs_every);
    // everything mg_maze3d_step refuses (NULL tasks / view / state / obs, n_envs < 1, ...), before the first launch
    if (int rc = mg_maze3d_step_check(T, view, task_type, max_steps, continuous, auto_reset, n, st, obs, stream)) return rc;
    const size_t frame = (size_t)n * view->res_h * view->res_v * 3 * (view->obs_format == 1 ? 1 : sizeof(int32_t));
    unsigned char *slice = static_cast<unsigned char *>(obs);
    const Me3Out po{ret_total, ret_episode, episode_len, episodes};
    const Me3Rec rec{actions, reward, reward64, done};
    const dim3 grid((unsigned)((n + ME_ROLL_BLOCK - 1) / ME_ROLL_BLOCK)), block(ME_ROLL_BLOCK);
    for (int s0 = 0; s0 < n_steps;) {
        int s1 = s0;
        while (!rollout_records(s1, n_steps, obs_every)) ++s1;      // the stretch ends with the next recorded step
        ++s1;
        {
            mg::DeviceGuard guard(mg::device_of(st->grid));
            if (continuous)
                hipLaunchKernelGGL(maze3d_expert_advance_kernel<true>, grid, block, 0, (hipStream_t)stream, *T, *st,
                                   view->collision_dist, task_type, max_steps, auto_reset, n, s0, s1, dist, po, rec);
            else
                hipLaunchKernelGGL(maze3d_expert_advance_kernel<false>, grid, block, 0, (hipStream_t)stream, *T, *st,
                                   view->collision_dist, task_type, max_steps, auto_reset, n, s0, s1, dist, po, rec);
            if (int rc = mg::check_launch("maze3d_expert_advance_kernel")) return rc;
        }
        // the frame of the state the stretch left: mg_maze3d_step's observe-only form, renderer untouched
        if (int rc = mg_maze3d_step(T, view, task_type, max_steps, continuous, auto_reset, n, st, nullptr, slice, nullptr, nullptr,
                                    nullptr, stream)) return rc;
        slice += frame;
        s0 = s1;
    }
    return MG_OK;
}
