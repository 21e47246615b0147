// quadrotor_tasks.hip — the quadrotor task table: per-env simulator parameters in one launch (mg_quadrotor_tasks_*).
//
// A translation unit of its own on quadrotor_core.h (substep<>, failure_code, observe, collision, reset_draw, ..., and the
// host-side folding: fold_config, config_is_simple), next to quadrotor.hip and not inside it: a kernel added to
// quadrotor.hip itself perturbs the register allocation of its neighbours, and those kernels are tuned.
// Same flags as quadrotor.hip (metagym_amd/build.py): -ffp-contract=off, no SLP vectoriser.
#include "quadrotor_core.h"

#include "quadrotor_task_table.h"

namespace {

// One wave per block: a lane holds its state (Lane) and its row, and with one wave the compiler may use the whole
// register file of a SIMD lane (512 VGPRs and AGPRs) before it would touch scratch.
constexpr int TASKS_BLOCK = mg::WAVE;

// The generic form (quadrotor_step_kernel<SIMPLE, STEP_GENERIC>) on lane-local constants: the same device functions in
// the same order, so a table of identical rows gives the uniform env's bits. The sub-step loop runs each lane for its
// own `times` (a divergent trip count: the wave goes on until its longest lane is done), with the failure test and the
// freeze after every sub-step.
template <bool SIMPLE>
__global__ __launch_bounds__(TASKS_BLOCK) void quadrotor_tasks_step_kernel(QuadK k, mg_quadrotor_state st, StepIO io,
                                                                           TaskTable tt, int n, int n_steps) {
    __shared__ float tile[mg::WAVE * (OBS_DIM + 1)];
    const int e = blockIdx.x * TASKS_BLOCK + threadIdx.x;
    const bool live = e < n;
    const int el = live ? e : n - 1;   // out-of-range lanes shadow the last env, stores are masked
    float4 a_next = reinterpret_cast<const float4 *>(io.action)[el];
    const QuadK kl = lane_constants(k, tt, task_of(tt, el));
    bool ok = true;
    Lane s;
    int ct;
    uint32_t episode = 0;
    if (k.auto_reset) episode = st.episode[el];
    load_lane(st, n, el, s, ct);
    const uint32_t episode_in = episode;
    const bool vel_task = k.task == MG_QUADROTOR_TASK_VELOCITY_CONTROL;
    const bool hover_task = k.task == MG_QUADROTOR_TASK_HOVERING_CONTROL;

    for (int t = 0; t < n_steps; ++t) {
        const size_t off = (size_t)t * n;
        const float4 a = a_next;
        if (t + 1 < n_steps) a_next = reinterpret_cast<const float4 *>(io.action)[off + n + el];
        const float av[4] = {a.x, a.y, a.z, a.w};
        float eff32[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double d = (double)av[i];
            d = d > kl.max_v ? kl.max_v : (d < kl.min_v ? kl.min_v : d);
            eff32[i] = (float)d;
        }
        ct += 1;
        const double old_pos[3] = {(double)s.p[0] + k.xoff, (double)s.p[1] + k.yoff, (double)(s.p[2] + k.zoff32)};
        int fail = 0;
        for (int it = 0; it < kl.times; ++it) {
            if (fail == 0) {
                substep<SIMPLE>(kl, s, eff32, it == kl.times - 1, ok);
                fail = failure_code(kl, s);
            }
        }
        const int tn_step = ct < k.nt - 1 ? ct : k.nt - 1;
        double reward = 0.0;
        int done = 1;
        if (fail == 0 && vel_task) {
            float bt[3];
            mv_f32(s.Ri, &kl.vtargets[3 * (ct - 1)], bt);
            double b_v[3];
            mv_f32f64(s.Ri, s.v, b_v);
            const double diff = (fabs((double)bt[0] - b_v[0]) + fabs((double)bt[1] - b_v[1])) + fabs((double)bt[2] - b_v[2]);
            const float energy = k.dt32 * s.power;
            const double r = (k.healthy32 < energy) ? -k.healthy : -(double)energy;
            reward = r + (-0.001 * diff);
            done = 0;
            if (ct == k.nt) { done = 1; ct = 0; }
        } else if (fail == 0) {
            const double new_pos[3] = {(double)s.p[0] + k.xoff, (double)s.p[1] + k.yoff, (double)(s.p[2] + k.zoff32)};
            const bool hit = collision(k, old_pos, new_pos);
            const float energy = k.dt32 * s.power;
            double r = (k.healthy32 < energy) ? -k.healthy : -(double)energy;
            double task_reward = hit ? 0.0 : k.healthy;
            if (hover_task) {
                task_reward -= 1.0 * s.nv + 1.0 * s.nw;
                const float z_move = fabsf(0.0f - s.p[2]);
                if (z_move < 0.5f) task_reward += 10;
                else {
                    const float o = 0.5f - z_move;
                    task_reward += (o > -20.0f) ? (double)o : -20.0;
                }
            }
            if (hover_task || k.healthy32 < energy)
                reward = r + task_reward;
            else
                reward = (double)((float)r + (float)task_reward);
            done = 0;
            if (hit) { done = 1; ct = 0; }
            if (ct == k.nt) { done = 1; ct = 0; }
        } else {
            ct = 0;
        }
        int tn = tn_step;
        if (k.auto_reset && done) {
            reset_apply(s, reset_draw(kl, el, episode));
            episode += 1;
            tn = ct < k.nt - 1 ? ct : k.nt - 1;
        }
        if (t == n_steps - 1 && live) {
            store_lane(st, n, e, s, ct);
            if (episode != episode_in) st.episode[e] = episode;
        }
        float obs[OBS_DIM + 3];
        observe(k, s, obs);
        if (vel_task) { obs[16] = kl.vtargets[3 * tn]; obs[17] = kl.vtargets[3 * tn + 1]; obs[18] = kl.vtargets[3 * tn + 2]; }
        store_obs_wave(tile, obs, io.obs + off * k.obs_dim, n, e, k.obs_dim);
        if (live) {
            if (io.reward) st_stream<st_policy<false, ST_SCALAR>()>(&io.reward[off + e], (float)reward);
            if (io.reward64) st_stream<st_policy<false, ST_SCALAR>()>(&io.reward64[off + e], reward);
            st_stream<st_policy<false, ST_SCALAR>()>(&io.done[off + e], (uint8_t)done);
            if (io.failed) st_stream<st_policy<false, ST_SCALAR>()>(&io.failed[off + e], (uint8_t)fail);
        }
    }
}

// quadrotor_reset_kernel for a table: observe() reads shared fields only, the velocity task's three target entries come
// from the env's own trajectory.
__global__ __launch_bounds__(BLOCK) void quadrotor_tasks_reset_kernel(QuadK k, mg_quadrotor_state st, TaskTable tt,
                                                                      const uint8_t *mask, const double *init_vel,
                                                                      const double *init_omega, float *obs_out, int n) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= n) return;
    if (mask != nullptr && mask[e] == 0) return;
    Lane s;
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
    store_lane(st, n, e, s, ct);
    if (obs_out != nullptr) {
        float obs[OBS_DIM + 3];
        observe(k, s, obs);
        if (k.task == MG_QUADROTOR_TASK_VELOCITY_CONTROL) {
            const float *vt = tt.vtargets + (size_t)task_of(tt, e) * (size_t)k.nt * 3;
            const int tn = ct < k.nt - 1 ? ct : k.nt - 1;
            obs[16] = vt[3 * tn]; obs[17] = vt[3 * tn + 1]; obs[18] = vt[3 * tn + 2];
        }
        for (int c = 0; c < k.obs_dim; ++c) obs_out[(size_t)e * k.obs_dim + c] = obs[c];
    }
}

// ---- host: task table ------------------------------------------------------------------------------------------------
void row_from_k(const QuadK &k, const mg_quadrotor_config *cfg, const mg_quadrotor_autoreset *ar, TaskRow *r) {
    memset(r, 0, sizeof *r);
    r->magic = TASK_ROW_MAGIC;
    r->quality_recip_exact = k.quality_recip_exact;
    r->times = k.times;
    r->simple = config_is_simple(cfg) ? 1 : 0;
    r->phi32 = k.phi32; r->phi_over_ra32 = k.phi_over_ra32; r->inv_jm32 = k.inv_jm32; r->mm32 = k.mm32;
    r->prec32 = k.prec32; r->ct0_32 = k.ct0_32; r->ct1_32 = k.ct1_32; r->quality32 = k.quality32;
    r->fail_range_sq32 = k.fail_range_sq32;
    for (int i = 0; i < 4; ++i) r->lm[i] = k.lm[i];
    for (int i = 0; i < 12; ++i) r->pc[i] = k.pc[i];
    for (int i = 0; i < 9; ++i) { r->iinv[i] = k.iinv[i]; r->df[i] = k.df[i]; r->dm[i] = k.dm[i]; }
    for (int i = 0; i < 3; ++i) r->cog[i] = k.cog[i];
    r->prec = k.prec; r->half_dt2 = k.half_dt2; r->half_dt = k.half_dt; r->ct2 = k.ct2;
    r->quality = k.quality; r->inv_quality = k.inv_quality;
    r->min_v = k.min_v; r->max_v = k.max_v; r->fail_velocity = k.fail_velocity; r->fail_w = k.fail_w;
    r->dt = cfg->dt;
    if (ar != nullptr) {
        for (int i = 0; i < 3; ++i) { r->init_v_base[i] = ar->init_velocity[i]; r->init_w_base[i] = ar->init_angular_velocity[i]; }
        r->init_v_noisy = ar->init_velocity_noisy;
        r->init_w_noisy = ar->init_angular_velocity_noisy;
    }
}

// the shared constants of a table launch and the table's device view
int fold_tasks(const mg_quadrotor_config *cfg, const mg_quadrotor_tasks *tasks, int32_t n, const mg_quadrotor_state *state,
               QuadK *k, TaskTable *tt) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(tasks);
    MG_REQUIRE_PTR(state);
    if (n <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_envs=%d", n);
    if (tasks->n_tasks <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_tasks=%d", tasks->n_tasks);
    if (tasks->rows_d == nullptr || tasks->task_id_d == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_quadrotor_tasks needs rows_d and task_id_d");
    if (int rc = check_state(state)) return rc;
    if (int rc = fold_config(cfg, k, false)) return rc;
    if (!(tasks->dt == cfg->dt))
        return mg::set_error(MG_ERR_BAD_CONFIG, "the task rows were folded for dt=%g, the call has dt=%g", tasks->dt, cfg->dt);
    if (cfg->task == MG_QUADROTOR_TASK_VELOCITY_CONTROL) {
        if (tasks->velocity_targets_d == nullptr)
            return mg::set_error(MG_ERR_NULL_POINTER, "velocity_control needs tasks->velocity_targets_d");
        k->vtargets = tasks->velocity_targets_d;   // non-NULL marks the task; lanes take their own slice
    } else {
        k->vtargets = nullptr;
    }
    tt->rows = static_cast<const TaskRow *>(tasks->rows_d);
    tt->task_id = tasks->task_id_d;
    tt->vtargets = tasks->velocity_targets_d;
    tt->n_tasks = tasks->n_tasks;
    return MG_OK;
}

}  // namespace

extern "C" int32_t mg_quadrotor_tasks_row_bytes(void) { return (int32_t)sizeof(TaskRow); }

extern "C" int mg_quadrotor_tasks_fold(const mg_quadrotor_config *cfg, const mg_quadrotor_autoreset *ar, void *row_out_host) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(row_out_host);
    QuadK k;
    if (int rc = fold_config(cfg, &k, false)) return rc;
    TaskRow r;
    row_from_k(k, cfg, ar, &r);
    memcpy(row_out_host, &r, sizeof r);
    return MG_OK;
}

extern "C" int mg_quadrotor_tasks_describe(const void *row_host, mg_quadrotor_task_fold *out) {
    MG_REQUIRE_PTR(row_host);
    MG_REQUIRE_PTR(out);
    TaskRow r;
    memcpy(&r, row_host, sizeof r);
    if (r.magic != TASK_ROW_MAGIC) return mg::set_error(MG_ERR_BAD_CONFIG, "not a row of mg_quadrotor_tasks_fold");
    *out = mg_quadrotor_task_fold{};
    for (int i = 0; i < 9; ++i) out->inertia_inv[i] = r.iinv[i];
    for (int i = 0; i < 4; ++i) out->lm[i] = r.lm[i];
    out->fail_range_sq32 = r.fail_range_sq32;
    out->prec32 = r.prec32;
    out->times = r.times;
    out->simple = r.simple;
    out->precision = r.prec;
    out->half_dt2 = r.half_dt2;
    out->dt = r.dt;
    for (int i = 0; i < 3; ++i) { out->init_velocity[i] = r.init_v_base[i]; out->init_angular_velocity[i] = r.init_w_base[i]; }
    out->init_velocity_noisy = r.init_v_noisy;
    out->init_angular_velocity_noisy = r.init_w_noisy;
    return MG_OK;
}

extern "C" int mg_quadrotor_tasks_step(const mg_quadrotor_config *cfg, const mg_quadrotor_tasks *tasks, int32_t n,
                                       int32_t n_steps, const mg_quadrotor_state *state, const mg_quadrotor_autoreset *ar,
                                       const float *action, float *obs, float *reward, double *reward64, uint8_t *done,
                                       uint8_t *failed, void *stream) {
    MG_REQUIRE_PTR(action);
    MG_REQUIRE_PTR(obs);
    MG_REQUIRE_PTR(done);
    if (n_steps <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_steps=%d", n_steps);
    QuadK k;
    TaskTable tt;
    if (int rc = fold_tasks(cfg, tasks, n, state, &k, &tt)) return rc;
    if (ar != nullptr) {
        if (state->episode == nullptr)
            return mg::set_error(MG_ERR_NULL_POINTER, "fused auto-reset needs mg_quadrotor_state.episode");
        k.auto_reset = 1;
        k.seed = ar->seed;
        k.env_id_base = ar->env_id_base;
    }
    // the SIMPLE specialisation when every row has the stock structure (and, as in make_plan, not for the velocity task)
    const bool simple = tasks->all_simple != 0 && cfg->task != MG_QUADROTOR_TASK_VELOCITY_CONTROL;
    StepIO io{action, obs, reward, reward64, done, failed};
    const int grid = (n + TASKS_BLOCK - 1) / TASKS_BLOCK;
    mg::DeviceGuard guard(mg::device_of(state->pos));
    if (simple)
        hipLaunchKernelGGL(quadrotor_tasks_step_kernel<true>, dim3(grid), dim3(TASKS_BLOCK), 0, (hipStream_t)stream, k,
                           *state, io, tt, n, n_steps);
    else
        hipLaunchKernelGGL(quadrotor_tasks_step_kernel<false>, dim3(grid), dim3(TASKS_BLOCK), 0, (hipStream_t)stream, k,
                           *state, io, tt, n, n_steps);
    return mg::check_launch("quadrotor_tasks_step_kernel");
}

extern "C" int mg_quadrotor_tasks_reset(const mg_quadrotor_config *cfg, const mg_quadrotor_tasks *tasks, int32_t n,
                                        const mg_quadrotor_state *state, const uint8_t *mask, const double *init_vel,
                                        const double *init_omega, float *obs, void *stream) {
    QuadK k;
    TaskTable tt;
    if (int rc = fold_tasks(cfg, tasks, n, state, &k, &tt)) return rc;
    const int grid = (n + BLOCK - 1) / BLOCK;
    mg::DeviceGuard guard(mg::device_of(state->pos));
    hipLaunchKernelGGL(quadrotor_tasks_reset_kernel, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, k, *state, tt, mask,
                       init_vel, init_omega, obs, n);
    return mg::check_launch("quadrotor_tasks_reset_kernel");
}
