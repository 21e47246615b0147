// quadrotor_task_table.h — the quadrotor task table's device view: the folded row, the table and the lane's constants.
// Included by quadrotor_tasks.hip (the table step) and quadrotor_policy.hip (the closed-loop rollout), each after
// quadrotor_core.h, whose QuadK the row overlays. Not a header for anything else.
#pragma once

namespace {

// ---- task table: per-env simulator parameters (mg_quadrotor_tasks_step) ---------------------------------------------
// One folded row per task in device memory: the fields of QuadK that come from a config.json key, in QuadK's own
// types, written by fold_config on the host (mg_quadrotor_tasks_fold). dt, nt, task, healthy_reward, the map and its
// offsets, seed and env_id_base stay in the launch's one QuadK.
struct alignas(16) TaskRow {
    uint32_t magic;
    int32_t quality_recip_exact, times, simple;
    float phi32, phi_over_ra32, inv_jm32, mm32, prec32, ct0_32, ct1_32, quality32, fail_range_sq32;
    float lm[4], pc[12], iinv[9], df[9], dm[9], cog[3];
    float init_v_base[3], init_w_base[3];
    float pad;
    double prec, half_dt2, half_dt, ct2, quality, inv_quality;
    double min_v, max_v, fail_velocity, fail_w, init_v_noisy, init_w_noisy;
    double dt;   // the env step the row was folded for (times = int(dt / precision)); the host compares it with the call's
};
constexpr uint32_t TASK_ROW_MAGIC = 0x4d475154u;   // "MGQT"
static_assert(sizeof(TaskRow) % 16 == 0 && sizeof(TaskRow) == 368, "task row layout");

struct TaskTable {
    const TaskRow *rows;     // [n_tasks]
    const int32_t *task_id;  // [n]
    const float *vtargets;   // [n_tasks][nt][3], velocity_control only
    int n_tasks;
};

// The env's task id, clamped into the table: ids are validated by the caller, and a bad one must not become an address.
__device__ __forceinline__ int task_of(const TaskTable &tt, int e) {
    const int t = tt.task_id[e];
    return t < 0 ? 0 : (t >= tt.n_tasks ? tt.n_tasks - 1 : t);
}

// The lane's own constants: the launch's QuadK with the row's fields on top. Everything is inlined, so the shared fields
// stay scalar (kernel arguments) and the row's become VGPRs, loaded once per launch: the step is VALU-bound, and a
// reload per sub-step would cost more than the registers.
__device__ __forceinline__ QuadK lane_constants(const QuadK &k, const TaskTable &tt, int task) {
    const TaskRow &r = tt.rows[task];
    QuadK kl = k;
    kl.phi32 = r.phi32; kl.phi_over_ra32 = r.phi_over_ra32; kl.inv_jm32 = r.inv_jm32; kl.mm32 = r.mm32;
    kl.prec32 = r.prec32; kl.ct0_32 = r.ct0_32; kl.ct1_32 = r.ct1_32; kl.quality32 = r.quality32;
    kl.fail_range_sq32 = r.fail_range_sq32;
#pragma unroll
    for (int i = 0; i < 4; ++i) kl.lm[i] = r.lm[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) kl.pc[i] = r.pc[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) { kl.iinv[i] = r.iinv[i]; kl.df[i] = r.df[i]; kl.dm[i] = r.dm[i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) { kl.cog[i] = r.cog[i]; kl.init_v_base[i] = r.init_v_base[i]; kl.init_w_base[i] = r.init_w_base[i]; }
    kl.prec = r.prec; kl.half_dt2 = r.half_dt2; kl.half_dt = r.half_dt; kl.ct2 = r.ct2;
    kl.quality = r.quality; kl.inv_quality = r.inv_quality;
    kl.min_v = r.min_v; kl.max_v = r.max_v; kl.fail_velocity = r.fail_velocity; kl.fail_w = r.fail_w;
    kl.init_v_noisy = r.init_v_noisy; kl.init_w_noisy = r.init_w_noisy;
    kl.quality_recip_exact = r.quality_recip_exact;
    kl.times = r.times;
    if (k.vtargets != nullptr) kl.vtargets = tt.vtargets + (size_t)task * (size_t)k.nt * 3;
    return kl;
}

}  // namespace
