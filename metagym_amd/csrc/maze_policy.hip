// maze_policy.hip — MetaMaze 2-D closed-loop rollouts: per-env recurrent policies inside the launch (mg_maze2d_policy_*).
//
// A translation unit of its own on maze_core.h (load_task, load_agent, move_2d, step_tail, Returns, observe_2d,
// rollout_records, the host checks). Same flags (metagym_amd/build.py): -ffp-contract=off, which is what makes the policy
// definition of include/metagym_hip.h hold (one rounding per operation).
//
// Mapping: maze2d_rollout_kernel's — one lane per env, one wave per workgroup, task and agent in registers for n_steps steps.
// The policy input x (the window, the previous action one-hot, the previous reward and done) lives in registers (the kernel is
// templated on view_grid, so D is a compile-time constant); the recurrent state h and its successor live in LDS lane-minor
// (buf[j * 64 + lane]: the 64 lanes of a ds_read_b32 fall on 64 consecutive dwords, no bank is hit twice in a 32-lane group).
// Weights: a wave whose lanes all hold one policy id stages that policy in LDS once and reads it with same-address
// (broadcast) 16-byte reads; a wave with mixed ids reads per lane from global memory. Both inline policy_eval, so the bits
// are equal.
#include "maze_core.h"

#include "mg_closed_loop.h"
#include "mg_sample.h"

namespace {

constexpr int MP_BLOCK = mg::WAVE;
constexpr int MP_MAX_HIDDEN = 64;
constexpr uint32_t MP_PHILOX_TAG = 0x4D5Au;      // c3 of the exploration draw

typedef mg::v4f mp_v4f;

__host__ __device__ constexpr int mp_input_dim(int vg) { return (2 * vg + 1) * (2 * vg + 1) + 6; }
__host__ __device__ constexpr int mp_hidden_pad(int hidden) { return (hidden + 3) & ~3; }
// floats of one hidden unit's record: wx[j][0..D-1], b[j], wh[j][0..H-1], zeros up to a multiple of four, wo[0..3][j]
__host__ __device__ constexpr int mp_record(int hidden, int d) { return d + 1 + mp_hidden_pad(hidden) + 4; }
// floats of one packed policy: bo[0..3], then H records (D + 1 is a multiple of four for every view_grid: 16, 32, 56)
__host__ __device__ constexpr int mp_count(int hidden, int d) { return 4 + hidden * mp_record(hidden, d); }

// The dynamic LDS of one workgroup, in bytes from its 16-byte aligned base: the staged policy, the two lane-minor state
// buffers, and (only when observation slices are recorded) the wave's 64 windows. One function for the launch and the kernel.
struct MpLds { int policy, h0, h1, tile, bytes; };
__host__ __device__ inline MpLds mp_lds_layout(int hidden, int vg, bool tile) {
    const int ww = (2 * vg + 1) * (2 * vg + 1);
    MpLds l;
    l.policy = 0;
    l.h0 = mp_count(hidden, mp_input_dim(vg)) * (int)sizeof(float);           // (a multiple of 16)
    l.h1 = l.h0 + hidden * MP_BLOCK * (int)sizeof(float);
    l.tile = l.h1 + hidden * MP_BLOCK * (int)sizeof(float);
    l.bytes = l.tile + (tile ? MP_BLOCK * ww * (int)sizeof(float) : 0);
    return l;
}

struct MpPolicy {
    const float *__restrict__ params;       // [n_policies][count]
    const uint32_t *__restrict__ thr;       // [n_policies] or null (no exploration)
    const int32_t *__restrict__ ids;        // [n]
    int n_policies, hidden;
};

// The policy of include/metagym_hip.h on one packed parameter block, from LDS (every lane the same address: broadcast reads)
// or from global memory (each lane its own block). h and hn are the lane's columns of the two LDS state buffers. The j loop
// runs at run time; the x loop is unrolled, the h loop reads four recurrent weights per 16-byte read and skips the padding
// (0 * h added to a pre-activation of -0 would turn it into +0). hn[j] goes into the four logits as soon as it is known: for
// every k that is the sum over j in ascending order, as defined. Returns the greedy action; SAMPLED: the Gumbel-max draw, the
// same argmax over score[k] = l[k] * inv_t + g[k] (mg_sample.h), the four words of one Philox block.
template <int D, bool SAMPLED>
__device__ __forceinline__ int policy_eval(const float *__restrict__ p, int hidden, const float *x, const float *h, float *hn,
                                           float inv_t, uint32_t env, uint64_t step, uint64_t seed) {
    static_assert((D + 1) % 4 == 0, "the x part of a record is read in 16-byte pieces");
    const int hp = mp_hidden_pad(hidden), rec = mp_record(hidden, D);
    const mp_v4f bo = *reinterpret_cast<const mp_v4f *>(p);
    float l0 = bo.x, l1 = bo.y, l2 = bo.z, l3 = bo.w;
#pragma unroll 1
    for (int j = 0; j < hidden; ++j) {
        const float *r = p + 4 + rec * j;
        float w[D + 1];
#pragma unroll
        for (int q = 0; q < (D + 1) / 4; ++q) {
            const mp_v4f v = *reinterpret_cast<const mp_v4f *>(r + 4 * q);
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
        float z = w[D];
#pragma unroll
        for (int i = 0; i < D; ++i) z = z + w[i] * x[i];
        const float *rh = r + D + 1;
#pragma unroll 1
        for (int i = 0; i < hp; i += 4) {
            const mp_v4f v = *reinterpret_cast<const mp_v4f *>(rh + i);
            z = z + v.x * h[i * MP_BLOCK];
            if (i + 1 < hidden) z = z + v.y * h[(i + 1) * MP_BLOCK];
            if (i + 2 < hidden) z = z + v.z * h[(i + 2) * MP_BLOCK];
            if (i + 3 < hidden) z = z + v.w * h[(i + 3) * MP_BLOCK];
        }
        const float a = z > 1.0f ? 1.0f : (z < -1.0f ? -1.0f : z);      // a NaN stays NaN, -0 stays -0
        hn[j * MP_BLOCK] = a;
        const mp_v4f wo = *reinterpret_cast<const mp_v4f *>(rh + hp);
        l0 = l0 + wo.x * a; l1 = l1 + wo.y * a; l2 = l2 + wo.z * a; l3 = l3 + wo.w * a;
    }
    if (SAMPLED) {
        uint32_t o[4];
        mg::sample_block(env, step, 0u, seed, o);
        l0 = mg::sample_score(l0, inv_t, o[0]);
        l1 = mg::sample_score(l1, inv_t, o[1]);
        l2 = mg::sample_score(l2, inv_t, o[2]);
        l3 = mg::sample_score(l3, inv_t, o[3]);
    }
    int g = 0;                                                           // ties and NaN logits: the lowest index
    float best = l0;
    if (l1 > best) { g = 1; best = l1; }
    if (l2 > best) { g = 2; best = l2; }
    if (l3 > best) { g = 3; }
    return g;
}

// maze2d_rollout_kernel's step (move_2d, step_tail) with the action load replaced by the policy. x is computed from the state
// the lane holds (observe_2d into registers) before the loop and after every step: the observation buffer is never read.
// Inside the step loop the kernel stores only what `rec` asks for; the agent, the carry, the four per-env results and the
// last window go out once, at the end. SAMPLED: the action is drawn from softmax(l / temperature) (inv_t [n_policies], read
// once per env); an exploratory draw still overrides it. The greedy instantiations read no inv_t (they are passed NULL).
template <int VG, bool SAMPLED>
__global__ __launch_bounds__(MP_BLOCK) void maze2d_policy_rollout_kernel(mg_maze_tasks T, mg_maze_state st, int task_type,
                                                                         int max_steps, int auto_reset, int n_envs, int n_steps,
                                                                         int obs_every, MpPolicy pa, mg_maze_policy_carry ca,
                                                                         uint64_t seed, uint64_t step0, int episodic, RolloutOut po,
                                                                         RolloutRec rec, const float *__restrict__ inv_temperature) {
    constexpr int W = 2 * VG + 1, WW = W * W, D = WW + 6;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int H = pa.hidden;
    const MpLds lds = mp_lds_layout(H, VG, rec.obs != nullptr);
    const int lane = threadIdx.x;
    const float *policy_lds = reinterpret_cast<const float *>(smem + lds.policy);
    float *hc = reinterpret_cast<float *>(smem + lds.h0) + lane;           // the lane's column: h[j] at hc[j * 64]
    float *hx = reinterpret_cast<float *>(smem + lds.h1) + lane;
    float *tile = reinterpret_cast<float *>(smem + lds.tile);              // [64][WW] lane-major, as maze2d_rollout_kernel's
    const int e0 = blockIdx.x * MP_BLOCK;
    const int e = e0 + lane;
    const bool live = e < n_envs;
    const int el = live ? e : n_envs - 1;   // spare lanes shadow the last env and its policy id; they step nothing and store nothing

    // The env's policy, clamped. One id in the whole wave (a ballot: wave-uniform): stage it in LDS once.
    const int count = mp_count(H, D);
    const mg::StagedPolicy sp = mg::stage_policy(pa.params, count, pa.ids[el], pa.n_policies, lane, true,
                                                 reinterpret_cast<mp_v4f *>(smem + lds.policy));
    const bool staged = sp.staged;
    const float *__restrict__ own = sp.own;
    const uint32_t thr = pa.thr != nullptr ? pa.thr[sp.pid] : 0u;
    const float inv_t = SAMPLED ? inv_temperature[sp.pid] : 0.0f;

    const Task t = load_task(T, st.task_id[el]);
    Agent a = load_agent(st, n_envs, el);
    for (int j = 0; j < H; ++j) hc[j * MP_BLOCK] = ca.h[(size_t)el * H + j];
    int prev_action = ca.prev_action[el];
    float prev_reward = ca.prev_reward[el];
    int prev_done = ca.prev_done[el] != 0;
    __syncthreads();                                                       // (one wave) the staged policy is in place

    float x[D];
    observe_2d(t, st, el, task_type, VG, a, [&](int i, float v) { x[i] = v; });
    Returns ret;
    const int run = min(MP_BLOCK, n_envs - e0) * WW;                       // floats this wave owns in a slice of obs
    const size_t slice = (size_t)n_envs * WW;
    float *out = rec.obs;

    for (int s = 0; s < n_steps; ++s) {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[WW + k] = prev_action == k ? 1.0f : 0.0f;
        x[WW + 4] = prev_reward;
        x[WW + 5] = prev_done ? 1.0f : 0.0f;
        int act = staged ? policy_eval<D, SAMPLED>(policy_lds, H, x, hc, hx, inv_t, (uint32_t)el, step0 + (uint64_t)s, seed)
                         : policy_eval<D, SAMPLED>(own, H, x, hc, hx, inv_t, (uint32_t)el, step0 + (uint64_t)s, seed);
        { float *sw = hc; hc = hx; hx = sw; }                              // h = hn
        uint32_t word;
        if (mg::explore_draw((uint32_t)el, step0 + (uint64_t)s, MP_PHILOX_TAG, seed, thr, word)) act = (int)(word & 3u);
        if (live) {
            const size_t r_at = (size_t)s * n_envs + e;
            if (rec.actions) static_cast<int32_t *>(rec.actions)[r_at] = act;
            move_2d(t, act, a);
            double r;
            const int d = step_tail(t, st, e, task_type, max_steps, auto_reset, a, r_at, rec.reward, rec.reward64, rec.done, r);
            ret.add(r, d);
            prev_action = act;
            prev_reward = (float)r;
            prev_done = d;
            if (episodic && d && auto_reset) {                             // the next episode starts from a fresh carry
                for (int j = 0; j < H; ++j) hc[j * MP_BLOCK] = 0.0f;
                prev_action = -1;
                prev_reward = 0.0f;
                prev_done = 0;
            }
        }
        // this step's window is the next step's x (with auto_reset, the next episode's first window)
        observe_2d(t, st, el, task_type, VG, a, [&](int i, float v) { x[i] = v; });
        if (out == nullptr || !rollout_records(s, n_steps, obs_every)) continue;   // (uniform: every lane is at step s)
        if (live) {
#pragma unroll
            for (int i = 0; i < WW; ++i) tile[lane * WW + i] = x[i];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float *dst = out + (size_t)e0 * WW;
        for (int i = lane; i < run; i += MP_BLOCK) dst[i] = tile[i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");             // the next recorded step overwrites the tile
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        out += slice;
    }
    if (!live) return;
    store_agent(st, n_envs, e, a);
    for (int j = 0; j < H; ++j) ca.h[(size_t)e * H + j] = hc[j * MP_BLOCK];
    ca.prev_action[e] = prev_action;
    ca.prev_reward[e] = prev_reward;
    ca.prev_done[e] = (uint8_t)prev_done;
    float *o = po.obs_last + (size_t)e * WW;
#pragma unroll
    for (int i = 0; i < WW; ++i) o[i] = x[i];
    ret.store(po, e);
}

typedef decltype(&maze2d_policy_rollout_kernel<1, false>) MpKernel;
template <bool SAMPLED>
MpKernel pick_policy_kernel(int vg) {
    return vg == 1 ? maze2d_policy_rollout_kernel<1, SAMPLED>
                   : (vg == 2 ? maze2d_policy_rollout_kernel<2, SAMPLED> : maze2d_policy_rollout_kernel<3, SAMPLED>);
}

extern "C" int32_t mg_maze2d_policy_param_count(int32_t hidden, int32_t view_grid) {
    if (hidden < 1 || hidden > MP_MAX_HIDDEN) return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", hidden, MP_MAX_HIDDEN);
    if (view_grid < 1 || view_grid > 3) return mg::set_error(MG_ERR_BAD_CONFIG, "view_grid=%d is outside [1, 3]", view_grid);
    return mp_count(hidden, mp_input_dim(view_grid));
}

// The two entry points: every check, then the launch of a greedy or a sampled instantiation. `name` is the entry point's.
template <bool SAMPLED>
int maze2d_policy_rollout(const char *name, const mg_maze_tasks *T, int32_t task_type, int32_t max_steps, int32_t view_grid,
                          int32_t auto_reset, int32_t n, const mg_maze_state *st, int32_t n_steps, int32_t obs_every,
                          const mg_maze_policy *policy, const int32_t *policy_ids, const mg_maze_policy_carry *carry,
                          const float *inv_temperature, uint64_t seed, uint64_t step0, int32_t episodic, float *obs_last,
                          double *ret_total, double *ret_episode, int32_t *episode_len, int32_t *episodes, int32_t *actions,
                          float *reward, double *reward64, uint8_t *done, float *obs, void *stream) {
    MG_REQUIRE_PTR(T);
    MG_REQUIRE_PTR(st);
    MG_REQUIRE_PTR(policy);
    MG_REQUIRE_PTR(policy_ids);
    MG_REQUIRE_PTR(carry);
    if (SAMPLED) MG_REQUIRE_PTR(inv_temperature);
    MG_REQUIRE_PTR(obs_last);
    MG_REQUIRE_PTR(ret_total);
    MG_REQUIRE_PTR(ret_episode);
    MG_REQUIRE_PTR(episode_len);
    MG_REQUIRE_PTR(episodes);
    if (policy->params == nullptr) return mg::set_error(MG_ERR_NULL_POINTER, "mg_maze_policy needs params");
    if (!carry->h || !carry->prev_action || !carry->prev_reward || !carry->prev_done)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_maze_policy_carry has a NULL array");
    if (n <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_envs=%d", n);
    if (n_steps < 1) return mg::set_error(MG_ERR_BAD_SIZE, "%s: n_steps=%d (at least 1)", name, n_steps);
    if (obs_every < 0) return mg::set_error(MG_ERR_BAD_SIZE, "%s: obs_every=%d (0 = the last step only, k >= 1 = every k-th)", name, obs_every);
    if (view_grid < 1 || view_grid > 3)
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: view_grid=%d is outside [1, 3]", name, view_grid);
    if (policy->n_policies < 1) return mg::set_error(MG_ERR_BAD_SIZE, "n_policies=%d", policy->n_policies);
    if (policy->hidden < 1 || policy->hidden > MP_MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", policy->hidden, MP_MAX_HIDDEN);
    if (policy->view_grid != view_grid)
        return mg::set_error(MG_ERR_BAD_CONFIG, "the policy was built for view_grid=%d, the env has %d", policy->view_grid, view_grid);
    if (((uintptr_t)policy->params & 15u) != 0)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_maze_policy.params must be 16-byte aligned");
    if (int rc = check_tasks(T, task_type)) return rc;
    if (int rc = check_mstate(st, task_type)) return rc;
    if (int rc = check_slots(T, st, task_type)) return rc;
    const MpLds lds = mp_lds_layout(policy->hidden, view_grid, obs != nullptr);
    if ((size_t)lds.bytes > mg::LDS_LIMIT)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d view_grid=%d needs %d B of LDS (> 160 KiB)", policy->hidden, view_grid, lds.bytes);
    const MpKernel kernel = pick_policy_kernel<SAMPLED>(view_grid);
    mg::DeviceGuard guard(mg::device_of(st->grid));
    if (int rc = mg::opt_in_dynamic_lds(kernel, lds.bytes, "maze2d_policy_rollout_kernel")) return rc;
    MpPolicy pa{policy->params, policy->eps_threshold, policy_ids, policy->n_policies, policy->hidden};
    RolloutOut po{obs_last, ret_total, ret_episode, episode_len, episodes};
    RolloutRec rec{actions, reward, reward64, done, obs};
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + MP_BLOCK - 1) / MP_BLOCK)), dim3(MP_BLOCK), (size_t)lds.bytes,
                       (hipStream_t)stream, *T, *st, task_type, max_steps, auto_reset, n, n_steps, obs_every, pa, *carry, seed, step0,
                       episodic, po, rec, inv_temperature);
    return mg::check_launch("maze2d_policy_rollout_kernel");
}

}  // namespace

extern "C" int mg_maze2d_policy_rollout(const mg_maze_tasks *T, int32_t task_type, int32_t max_steps, int32_t view_grid,
                                        int32_t auto_reset, int32_t n, const mg_maze_state *st, int32_t n_steps,
                                        int32_t obs_every, const mg_maze_policy *policy, const int32_t *policy_ids,
                                        const mg_maze_policy_carry *carry, uint64_t seed, uint64_t step0, int32_t episodic,
                                        float *obs_last, double *ret_total, double *ret_episode, int32_t *episode_len,
                                        int32_t *episodes, int32_t *actions, float *reward, double *reward64, uint8_t *done,
                                        float *obs, void *stream) {
    return maze2d_policy_rollout<false>("mg_maze2d_policy_rollout", T, task_type, max_steps, view_grid, auto_reset, n, st, n_steps,
                                        obs_every, policy, policy_ids, carry, nullptr, seed, step0, episodic, obs_last, ret_total,
                                        ret_episode, episode_len, episodes, actions, reward, reward64, done, obs, stream);
}

extern "C" int mg_maze2d_policy_rollout_sampled(const mg_maze_tasks *T, int32_t task_type, int32_t max_steps, int32_t view_grid,
                                                int32_t auto_reset, int32_t n, const mg_maze_state *st, int32_t n_steps,
                                                int32_t obs_every, const mg_maze_policy *policy, const int32_t *policy_ids,
                                                const mg_maze_policy_carry *carry, const float *inv_temperature, uint64_t seed,
                                                uint64_t step0, int32_t episodic, float *obs_last, double *ret_total,
                                                double *ret_episode, int32_t *episode_len, int32_t *episodes, int32_t *actions,
                                                float *reward, double *reward64, uint8_t *done, float *obs, void *stream) {
    return maze2d_policy_rollout<true>("mg_maze2d_policy_rollout_sampled", T, task_type, max_steps, view_grid, auto_reset, n, st,
                                       n_steps, obs_every, policy, policy_ids, carry, inv_temperature, seed, step0, episodic,
                                       obs_last, ret_total, ret_episode, episode_len, episodes, actions, reward, reward64, done,
                                       obs, stream);
}
