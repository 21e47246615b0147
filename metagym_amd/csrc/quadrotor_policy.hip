// quadrotor_policy.hip — quadrotor closed-loop rollouts: per-env MLP policies inside the launch (mg_quadrotor_policy_*), and
// per-env recurrent policies with a carry between launches (mg_quadrotor_rpolicy_*, the RECURRENT instantiations).
//
// A translation unit of its own on quadrotor_core.h (the device functions and the host-side folding), like
// quadrotor_tasks.hip and for the same reason. Same flags (metagym_amd/build.py): -ffp-contract=off, which is what makes
// the policy definition of include/metagym_hip.h hold (one rounding per operation), and no SLP vectoriser.
#include "quadrotor_core.h"

#include "quadrotor_task_table.h"

namespace {

constexpr int POLICY_BLOCK = mg::WAVE;     // one wave per block, as the table step (quadrotor_tasks.hip)
constexpr int POLICY_MAX_HIDDEN = 256;
constexpr int POLICY_HEAD = 4;             // b2[0..3] (b[0..3] of a linear policy)
constexpr int POLICY_REC = 24;             // floats per hidden unit: w1 row, b1, zeros up to 20, w2 column
constexpr int POLICY_W2_AT = 20;

struct PolicyArgs {
    const float *__restrict__ params;      // [n_policies][count]
    const int32_t *__restrict__ policy_id; // [n]
    int n_policies, hidden, count;
};
// The recurrent form (RECURRENT = true): PolicyArgs, then the carry of include/metagym_hip.h, updated in place.
struct RPolicyArgs {
    const float *__restrict__ params;      // [n_policies][count], the recurrent layout (rp_count)
    const int32_t *__restrict__ policy_id; // [n]
    int n_policies, hidden, count;
    float *h, *prev_action, *prev_reward;  // [n][hidden], [n][4], [n]
    uint8_t *prev_done;                    // [n]
    int episodic;
};
template <bool RECURRENT> struct PolicyArgsOf { typedef PolicyArgs type; };
template <> struct PolicyArgsOf<true> { typedef RPolicyArgs type; };
struct PolicyOut {
    double *ret_total, *ret_episode;       // [n]
    int32_t *episode_len;                  // [n]
};
struct PolicyRec {                         // [T][n][...], each may be null
    float *actions, *obs, *reward;
    double *reward64;
    uint8_t *done, *failed;
};

constexpr int RPOLICY_MAX_HIDDEN = 64;
#ifndef RP_H_GROUP
#define RP_H_GROUP 32                      // memory entries (and their recurrent weights) read ahead of the sum; a power of two >= 4
#endif
__host__ __device__ constexpr int rp_pad4(int v) { return (v + 3) & ~3; }
// floats of one hidden unit's record: wx[j][0..D-1] padded to DP, (b[j], wr[j], wd[j], 0), wa[j][0..3], wh[j][0..H-1] padded to
// HP, wo[0..3][j]. Every piece starts on a multiple of four floats.
__host__ __device__ constexpr int rp_record(int hidden, int d) { return rp_pad4(d) + rp_pad4(hidden) + 12; }
// floats of one packed recurrent policy: bo[0..3], then H records
__host__ __device__ constexpr int rp_count(int hidden, int d) { return POLICY_HEAD + hidden * rp_record(hidden, d); }
// The dynamic LDS of one workgroup of a recurrent launch, in bytes from its 16-byte aligned base: the staged policy and
// the two lane-minor memory buffers (buf[j * 64 + lane]). One function for the launch and the kernel. The static
// observation tile (64 x 17 floats, 4 352 bytes, where the instantiation uses it) comes on top. The largest case, H = 64
// and D = 19: 4 * (4 + 64 * 96) = 24 592 bytes of policy, 2 * 64 * 64 * 4 = 32 768 of memory, 57 360 dynamic, 61 712
// with the tile: under the 64 KiB a launch gets without asking for more.
struct RpLds { int policy, h0, h1, bytes; };
__host__ __device__ constexpr RpLds rp_lds_layout(int hidden, int d) {
    const int h0 = rp_count(hidden, d) * (int)sizeof(float);            // (a multiple of 16)
    const int col = hidden * POLICY_BLOCK * (int)sizeof(float);
    return RpLds{0, h0, h0 + col, h0 + 2 * col};
}
constexpr int RPOLICY_STATIC_LDS = mg::WAVE * (OBS_DIM + 1) * (int)sizeof(float);
static_assert(rp_lds_layout(RPOLICY_MAX_HIDDEN, OBS_DIM + 3).h0 == 24592 && rp_lds_layout(RPOLICY_MAX_HIDDEN, OBS_DIM + 3).bytes == 57360 &&
              rp_lds_layout(RPOLICY_MAX_HIDDEN, OBS_DIM + 3).bytes + RPOLICY_STATIC_LDS == 61712 &&
              rp_lds_layout(RPOLICY_MAX_HIDDEN, OBS_DIM + 3).bytes + RPOLICY_STATIC_LDS <= 64 * 1024,
              "the largest recurrent policy fits the default dynamic-LDS limit");

int policy_count(int hidden, int obs_dim) { return hidden > 0 ? POLICY_HEAD + POLICY_REC * hidden : POLICY_HEAD + 4 * obs_dim; }

// The policy of include/metagym_hip.h on one packed parameter block, from LDS (every lane the same address: broadcast
// reads) or from global memory (each lane its own block). The j loop runs at run time and the D loop is unrolled; h_j
// goes into the four accumulators as soon as it is known, so nothing of size H is held. One text for both address
// spaces: the association is the same, and so are the bits.
template <int D>
__device__ __forceinline__ void policy_eval(const float *__restrict__ p, int hidden, const float *x, float *a) {
    const v4f b = *reinterpret_cast<const v4f *>(p);
    a[0] = b.x; a[1] = b.y; a[2] = b.z; a[3] = b.w;
    if (hidden == 0) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const v4f w = *reinterpret_cast<const v4f *>(p + POLICY_HEAD + 4 * i);
            a[0] = a[0] + w.x * x[i]; a[1] = a[1] + w.y * x[i]; a[2] = a[2] + w.z * x[i]; a[3] = a[3] + w.w * x[i];
        }
        return;
    }
#pragma unroll 1
    for (int j = 0; j < hidden; ++j) {
        const float *r = p + POLICY_HEAD + POLICY_REC * j;
        float w[POLICY_W2_AT];
#pragma unroll
        for (int q = 0; q < POLICY_W2_AT / 4; ++q) {
            const v4f v = *reinterpret_cast<const v4f *>(r + 4 * q);
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
        const v4f w2 = *reinterpret_cast<const v4f *>(r + POLICY_W2_AT);
        float z = w[D];
#pragma unroll
        for (int i = 0; i < D; ++i) z = z + w[i] * x[i];
        const float h = (z > 0.0f) ? z : 0.0f;      // a NaN or negative pre-activation gives +0.0
        a[0] = a[0] + w2.x * h; a[1] = a[1] + w2.y * h; a[2] = a[2] + w2.z * h; a[3] = a[3] + w2.w * h;
    }
}

// The recurrent policy of include/metagym_hip.h on one packed parameter block, from LDS (broadcast reads) or from global
// memory (each lane its own block). pa, pr, pd: the previous unclamped action, reward and done. h and hn are the lane's
// columns of the two LDS memory buffers (entry j at [j * 64]). The j loop runs at run time; the x loop is unrolled, the h
// loop reads four recurrent weights per 16-byte read and skips the padding (0 * h added to a pre-activation of -0 would
// turn it into +0). hn[j] goes into the four accumulators as soon as it is known: for every k that is the sum over j in
// ascending order, as defined.
template <int D>
__device__ __forceinline__ void rpolicy_eval(const float *__restrict__ p, int hidden, const float *x, const float *pa, float pr,
                                             float pd, const float *h, float *hn, float *a) {
    constexpr int DP = rp_pad4(D);
    const int hp = rp_pad4(hidden), hfull = hidden & ~3, hgroup = hidden & ~(RP_H_GROUP - 1), rec = rp_record(hidden, D);
    const v4f bo = *reinterpret_cast<const v4f *>(p);
    a[0] = bo.x; a[1] = bo.y; a[2] = bo.z; a[3] = bo.w;
#pragma unroll 1
    for (int j = 0; j < hidden; ++j) {
        const float *r = p + POLICY_HEAD + rec * j;
        float w[DP];
#pragma unroll
        for (int q = 0; q < DP / 4; ++q) {
            const v4f v = *reinterpret_cast<const v4f *>(r + 4 * q);
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
        const v4f m = *reinterpret_cast<const v4f *>(r + DP);           // b[j], wr[j], wd[j], 0
        const v4f wa = *reinterpret_cast<const v4f *>(r + DP + 4);
        float z = m.x;
#pragma unroll
        for (int i = 0; i < D; ++i) z = z + w[i] * x[i];
        z = z + wa.x * pa[0]; z = z + wa.y * pa[1]; z = z + wa.z * pa[2]; z = z + wa.w * pa[3];
        z = z + m.y * pr;
        z = z + m.z * pd;
        const float *rh = r + DP + 8;
        // Whole groups of RP_H_GROUP memory entries first: their weights and the entries are all read before the first
        // term is added (the scheduling barrier keeps the reads up there; at one wave per SIMD nothing else hides the LDS
        // latency, and left alone the compiler reads two entries at a time, just ahead of their use). Then whole quads,
        // then the last, partial quad. The sum itself stays one term at a time, in order.
        int i = 0;
#pragma unroll 1
        for (; i < hgroup; i += RP_H_GROUP) {
            v4f wv[RP_H_GROUP / 4];
            float hv[RP_H_GROUP];
#pragma unroll
            for (int q = 0; q < RP_H_GROUP / 4; ++q) wv[q] = *reinterpret_cast<const v4f *>(rh + i + 4 * q);
#pragma unroll
            for (int q = 0; q < RP_H_GROUP; ++q) hv[q] = h[(i + q) * POLICY_BLOCK];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < RP_H_GROUP / 4; ++q) {
                z = z + wv[q].x * hv[4 * q];
                z = z + wv[q].y * hv[4 * q + 1];
                z = z + wv[q].z * hv[4 * q + 2];
                z = z + wv[q].w * hv[4 * q + 3];
            }
        }
#pragma unroll 1
        for (; i < hfull; i += 4) {
            const v4f v = *reinterpret_cast<const v4f *>(rh + i);
            z = z + v.x * h[i * POLICY_BLOCK];
            z = z + v.y * h[(i + 1) * POLICY_BLOCK];
            z = z + v.z * h[(i + 2) * POLICY_BLOCK];
            z = z + v.w * h[(i + 3) * POLICY_BLOCK];
        }
        if (hfull < hidden) {                                            // its padding is skipped
            const v4f v = *reinterpret_cast<const v4f *>(rh + hfull);
            z = z + v.x * h[hfull * POLICY_BLOCK];
            if (hfull + 1 < hidden) z = z + v.y * h[(hfull + 1) * POLICY_BLOCK];
            if (hfull + 2 < hidden) z = z + v.z * h[(hfull + 2) * POLICY_BLOCK];
        }
        const float c = z > 1.0f ? 1.0f : (z < -1.0f ? -1.0f : z);      // a NaN stays NaN, -0 stays -0
        hn[j * POLICY_BLOCK] = c;
        const v4f wo = *reinterpret_cast<const v4f *>(rh + hp);
        a[0] = a[0] + wo.x * c; a[1] = a[1] + wo.y * c; a[2] = a[2] + wo.z * c; a[3] = a[3] + wo.w * c;
    }
}

template <bool TABLE>
__device__ __forceinline__ QuadK policy_lane_constants(const QuadK &k, const TaskTable &tt, int el) {
    if constexpr (TABLE) return lane_constants(k, tt, task_of(tt, el));
    else return k;
}

// The generic form's step body (quadrotor_tasks_step_kernel: substep<>, failure_code, collision, reward, reset_draw /
// reset_apply, in that order) with the action computed from observe() at the top of each step instead of loaded.
// TABLE: each lane carries its own TaskRow; else the launch's one QuadK stays scalar.
// D = 19 is the velocity task (its three target entries are part of x), D = 16 the other two.
// Inside the step loop the kernel stores only what `rec` asks for; the state, the returns and the last step's outputs
// go out once, at the end.
// RECURRENT: the policy is rpolicy_eval, fed the previous unclamped action, reward and done besides x; its memory lives
// in two lane-minor LDS buffers behind the staged policy (rp_lds_layout), swapped after every step; the carry is loaded
// before the loop and stored after it. Everything the recurrent form adds is under `if constexpr (RECURRENT)`: the six
// RECURRENT = false instantiations are compiled from the text they were compiled from before.
template <bool SIMPLE, bool TABLE, int D, bool RECURRENT = false>
__global__ __launch_bounds__(POLICY_BLOCK) void quadrotor_policy_rollout_kernel(QuadK k, mg_quadrotor_state st, TaskTable tt,
                                                                                typename PolicyArgsOf<RECURRENT>::type pa,
                                                                                PolicyOut po, PolicyRec rec, StepIO last, int n,
                                                                                int n_steps) {
    static_assert(D == OBS_DIM || D == OBS_DIM + 3, "observation width");
    constexpr bool VEL = D == OBS_DIM + 3;
    static_assert(!(SIMPLE && VEL), "SIMPLE excludes the velocity task (make_plan)");
    __shared__ float tile[mg::WAVE * (OBS_DIM + 1)];
    extern __shared__ v4f policy_lds[];          // pa.count floats, sized by the launch
    const int lane = threadIdx.x;
    const int e = blockIdx.x * POLICY_BLOCK + lane;
    const bool live = e < n;
    const int el = live ? e : n - 1;   // out-of-range lanes shadow the last env (and its policy id), stores are masked

    // The env's policy, clamped as task_of clamps. One id in the whole wave (a ballot: wave-uniform): stage it in LDS once.
    int pid = pa.policy_id[el];
    pid = pid < 0 ? 0 : (pid >= pa.n_policies ? pa.n_policies - 1 : pid);
    const int pid0 = __builtin_amdgcn_readfirstlane(pid);
    const bool staged = __builtin_amdgcn_ballot_w64(pid != pid0) == 0;
    const float *__restrict__ own = pa.params + (size_t)pid * (size_t)pa.count;
    if (staged) {
        const v4f *src = reinterpret_cast<const v4f *>(pa.params + (size_t)pid0 * (size_t)pa.count);
        for (int i = lane; i < pa.count / 4; i += POLICY_BLOCK) policy_lds[i] = src[i];
    }
    __syncthreads();
    // the carry: the lane's memory column (h[j] at hc[j * 64]; no lane reads another's), previous action, reward, done
    float *hc = nullptr, *hx = nullptr;
    float prev_a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, prev_r = 0.0f, prev_d = 0.0f;
    if constexpr (RECURRENT) {
        const RpLds lds = rp_lds_layout(pa.hidden, D);
        hc = reinterpret_cast<float *>(reinterpret_cast<char *>(policy_lds) + lds.h0) + lane;
        hx = reinterpret_cast<float *>(reinterpret_cast<char *>(policy_lds) + lds.h1) + lane;
        for (int j = 0; j < pa.hidden; ++j) hc[j * POLICY_BLOCK] = pa.h[(size_t)el * pa.hidden + j];
        const v4f v = *reinterpret_cast<const v4f *>(pa.prev_action + 4 * (size_t)el);
        prev_a[0] = v.x; prev_a[1] = v.y; prev_a[2] = v.z; prev_a[3] = v.w;
        prev_r = pa.prev_reward[el];
        prev_d = pa.prev_done[el] != 0 ? 1.0f : 0.0f;
    }

    const QuadK kl = policy_lane_constants<TABLE>(k, tt, el);
    bool ok = true;
    Lane s;
    int ct;
    uint32_t episode = 0;
    if (k.auto_reset) episode = st.episode[el];
    load_lane(st, n, el, s, ct);
    const uint32_t episode_in = episode;
    const bool hover_task = k.task == MG_QUADROTOR_TASK_HOVERING_CONTROL;

    // x: the observation of the state the lane holds = the row the last step or reset returned
    float x[OBS_DIM + 3];
    observe(k, s, x);
    if (VEL) {
        const int tn = ct < k.nt - 1 ? ct : k.nt - 1;
        x[16] = kl.vtargets[3 * tn]; x[17] = kl.vtargets[3 * tn + 1]; x[18] = kl.vtargets[3 * tn + 2];
    }
    double ret_total = 0.0, ret_episode = 0.0;
    int episode_len = 0;
    bool ended = false;

    for (int t = 0; t < n_steps; ++t) {
        const size_t off = (size_t)t * n;
        const bool last_step = t == n_steps - 1;
        float av[4];
        if constexpr (RECURRENT) {
            if (staged) rpolicy_eval<D>(reinterpret_cast<const float *>(policy_lds), pa.hidden, x, prev_a, prev_r, prev_d, hc, hx, av);
            else rpolicy_eval<D>(own, pa.hidden, x, prev_a, prev_r, prev_d, hc, hx, av);
            float *sw = hc; hc = hx; hx = sw;                              // h = hn
        } else {
            if (staged) policy_eval<D>(reinterpret_cast<const float *>(policy_lds), pa.hidden, x, av);
            else policy_eval<D>(own, pa.hidden, x, av);
        }
        if (rec.actions != nullptr && live)
            st_stream<st_policy<false, ST_OBS>()>(reinterpret_cast<v4f *>(rec.actions) + off + e, v4f{av[0], av[1], av[2], av[3]});
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
        if (fail == 0 && VEL) {
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
        // the returns: float64 sums in step order; the episode's stops with the first done
        ret_total = ret_total + reward;
        if (!ended) {
            ret_episode = ret_episode + reward;
            episode_len += 1;
            ended = done != 0;
        }
        if constexpr (RECURRENT) {
            // what the next step's policy sees: this step's unclamped action, the float32 of its reward record, its done
            prev_a[0] = av[0]; prev_a[1] = av[1]; prev_a[2] = av[2]; prev_a[3] = av[3];
            prev_r = (float)reward;
            prev_d = done ? 1.0f : 0.0f;
            if (pa.episodic && k.auto_reset && done) {                     // the next episode starts from a fresh carry
                for (int j = 0; j < pa.hidden; ++j) hc[j * POLICY_BLOCK] = 0.0f;
                prev_a[0] = 0.0f; prev_a[1] = 0.0f; prev_a[2] = 0.0f; prev_a[3] = 0.0f;
                prev_r = 0.0f;
                prev_d = 0.0f;
            }
        }
        if (last_step && live) {
            store_lane(st, n, e, s, ct);
            if (episode != episode_in) st.episode[e] = episode;
        }
        // this step's observation is the next step's x
        observe(k, s, x);
        if (VEL) { x[16] = kl.vtargets[3 * tn]; x[17] = kl.vtargets[3 * tn + 1]; x[18] = kl.vtargets[3 * tn + 2]; }
        if (rec.obs != nullptr) store_obs_wave(tile, x, rec.obs + off * D, n, e, D);
        if (last_step) store_obs_wave(tile, x, last.obs, n, e, D);
        if (live) {
            if (rec.reward) st_stream<st_policy<false, ST_SCALAR>()>(&rec.reward[off + e], (float)reward);
            if (rec.reward64) st_stream<st_policy<false, ST_SCALAR>()>(&rec.reward64[off + e], reward);
            if (rec.done) st_stream<st_policy<false, ST_SCALAR>()>(&rec.done[off + e], (uint8_t)done);
            if (rec.failed) st_stream<st_policy<false, ST_SCALAR>()>(&rec.failed[off + e], (uint8_t)fail);
            if (last_step) {
                if (last.reward) st_stream<st_policy<false, ST_SCALAR>()>(&last.reward[e], (float)reward);
                if (last.reward64) st_stream<st_policy<false, ST_SCALAR>()>(&last.reward64[e], reward);
                st_stream<st_policy<false, ST_SCALAR>()>(&last.done[e], (uint8_t)done);
                if (last.failed) st_stream<st_policy<false, ST_SCALAR>()>(&last.failed[e], (uint8_t)fail);
            }
        }
    }
    if (live) {
        st_stream<st_policy<false, ST_SCALAR>()>(&po.ret_total[e], ret_total);
        st_stream<st_policy<false, ST_SCALAR>()>(&po.ret_episode[e], ret_episode);
        st_stream<st_policy<false, ST_SCALAR>()>(&po.episode_len[e], episode_len);
        if constexpr (RECURRENT) {
            for (int j = 0; j < pa.hidden; ++j) pa.h[(size_t)e * pa.hidden + j] = hc[j * POLICY_BLOCK];
            *reinterpret_cast<v4f *>(pa.prev_action + 4 * (size_t)e) = v4f{prev_a[0], prev_a[1], prev_a[2], prev_a[3]};
            pa.prev_reward[e] = prev_r;
            pa.prev_done[e] = (uint8_t)(prev_d != 0.0f);
        }
    }
}

typedef decltype(&quadrotor_policy_rollout_kernel<false, false, OBS_DIM>) PolicyKernel;
PolicyKernel pick_policy_kernel(bool simple, bool table, bool vel) {
    if (vel) return table ? quadrotor_policy_rollout_kernel<false, true, OBS_DIM + 3> : quadrotor_policy_rollout_kernel<false, false, OBS_DIM + 3>;
    if (table) return simple ? quadrotor_policy_rollout_kernel<true, true, OBS_DIM> : quadrotor_policy_rollout_kernel<false, true, OBS_DIM>;
    return simple ? quadrotor_policy_rollout_kernel<true, false, OBS_DIM> : quadrotor_policy_rollout_kernel<false, false, OBS_DIM>;
}

// What both entry points do with cfg, tasks, state and ar after their own checks: the state's pointers, the folded constants
// (shared ones of a table launch, or the uniform env's), the table's device view and the fused reset. Host only.
int fold_policy_launch(const mg_quadrotor_config *cfg, const mg_quadrotor_tasks *tasks, const mg_quadrotor_state *state,
                       const mg_quadrotor_autoreset *ar, QuadK &k, TaskTable &tt, bool &simple) {
    if (int rc = check_state(state)) return rc;
    const bool vel = cfg->task == MG_QUADROTOR_TASK_VELOCITY_CONTROL;
    tt = TaskTable{nullptr, nullptr, nullptr, 0};
    if (tasks != nullptr) {
        // as fold_tasks of quadrotor_tasks.hip: the shared constants of a table launch and the table's device view
        if (tasks->n_tasks <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_tasks=%d", tasks->n_tasks);
        if (tasks->rows_d == nullptr || tasks->task_id_d == nullptr)
            return mg::set_error(MG_ERR_NULL_POINTER, "mg_quadrotor_tasks needs rows_d and task_id_d");
        if (int rc = fold_config(cfg, &k, false)) return rc;
        if (!(tasks->dt == cfg->dt))
            return mg::set_error(MG_ERR_BAD_CONFIG, "the task rows were folded for dt=%g, the call has dt=%g", tasks->dt, cfg->dt);
        if (vel && tasks->velocity_targets_d == nullptr)
            return mg::set_error(MG_ERR_NULL_POINTER, "velocity_control needs tasks->velocity_targets_d");
        k.vtargets = vel ? tasks->velocity_targets_d : nullptr;
        tt.rows = static_cast<const TaskRow *>(tasks->rows_d);
        tt.task_id = tasks->task_id_d;
        tt.vtargets = tasks->velocity_targets_d;
        tt.n_tasks = tasks->n_tasks;
        simple = tasks->all_simple != 0 && !vel;
    } else {
        if (int rc = fold_config(cfg, &k)) return rc;
        simple = config_is_simple(cfg) && !vel;
    }
    if (ar != nullptr) {
        if (state->episode == nullptr)
            return mg::set_error(MG_ERR_NULL_POINTER, "fused auto-reset needs mg_quadrotor_state.episode");
        k.auto_reset = 1;
        if (tasks == nullptr) {
            for (int i = 0; i < 3; ++i) { k.init_v_base[i] = ar->init_velocity[i]; k.init_w_base[i] = ar->init_angular_velocity[i]; }
            k.init_v_noisy = ar->init_velocity_noisy;
            k.init_w_noisy = ar->init_angular_velocity_noisy;
        }
        k.seed = ar->seed;
        k.env_id_base = ar->env_id_base;
    }
    return 0;
}

typedef decltype(&quadrotor_policy_rollout_kernel<false, false, OBS_DIM, true>) RPolicyKernel;
RPolicyKernel pick_rpolicy_kernel(bool simple, bool table, bool vel) {
    if (vel) return table ? quadrotor_policy_rollout_kernel<false, true, OBS_DIM + 3, true> : quadrotor_policy_rollout_kernel<false, false, OBS_DIM + 3, true>;
    if (table) return simple ? quadrotor_policy_rollout_kernel<true, true, OBS_DIM, true> : quadrotor_policy_rollout_kernel<false, true, OBS_DIM, true>;
    return simple ? quadrotor_policy_rollout_kernel<true, false, OBS_DIM, true> : quadrotor_policy_rollout_kernel<false, false, OBS_DIM, true>;
}

}  // namespace

extern "C" int32_t mg_quadrotor_policy_param_count(int32_t hidden, int32_t obs_dim) {
    if (hidden < 0 || hidden > POLICY_MAX_HIDDEN) return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [0, %d]", hidden, POLICY_MAX_HIDDEN);
    if (obs_dim != OBS_DIM && obs_dim != OBS_DIM + 3) return mg::set_error(MG_ERR_BAD_CONFIG, "obs_dim=%d is neither 16 nor 19", obs_dim);
    return policy_count(hidden, obs_dim);
}

extern "C" int mg_quadrotor_policy_rollout(const mg_quadrotor_config *cfg, const mg_quadrotor_tasks *tasks, int32_t n,
                                           int32_t n_steps, const mg_quadrotor_state *state, const mg_quadrotor_autoreset *ar,
                                           const mg_quadrotor_policy *policy, double *ret_total, double *ret_episode,
                                           int32_t *episode_len, const mg_quadrotor_policy_records *records,
                                           const mg_quadrotor_policy_last *last, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(state);
    MG_REQUIRE_PTR(policy);
    MG_REQUIRE_PTR(ret_total);
    MG_REQUIRE_PTR(ret_episode);
    MG_REQUIRE_PTR(episode_len);
    MG_REQUIRE_PTR(last);
    if (last->obs == nullptr || last->done == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_quadrotor_policy_last needs obs and done");
    if (policy->params_d == nullptr || policy->policy_id_d == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_quadrotor_policy needs params_d and policy_id_d");
    if (n <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_envs=%d", n);
    if (n_steps <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_steps=%d", n_steps);
    if (policy->n_policies < 1) return mg::set_error(MG_ERR_BAD_SIZE, "n_policies=%d", policy->n_policies);
    if (policy->hidden < 0 || policy->hidden > POLICY_MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [0, %d]", policy->hidden, POLICY_MAX_HIDDEN);
    const bool vel = cfg->task == MG_QUADROTOR_TASK_VELOCITY_CONTROL;
    const int obs_dim = vel ? OBS_DIM + 3 : OBS_DIM;
    if (policy->obs_dim != obs_dim)
        return mg::set_error(MG_ERR_BAD_CONFIG, "policy obs_dim=%d, the task's observation has %d entries", policy->obs_dim, obs_dim);
    if (((uintptr_t)policy->params_d & 15u) != 0)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_quadrotor_policy.params_d must be 16-byte aligned");
    QuadK k;
    TaskTable tt;
    bool simple;
    if (int rc = fold_policy_launch(cfg, tasks, state, ar, k, tt, simple)) return rc;
    PolicyArgs pa{policy->params_d, policy->policy_id_d, policy->n_policies, policy->hidden, policy_count(policy->hidden, obs_dim)};
    PolicyOut po{ret_total, ret_episode, episode_len};
    PolicyRec rec{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (records != nullptr) rec = PolicyRec{records->actions, records->obs, records->reward, records->reward64, records->done, records->failed};
    StepIO io{nullptr, last->obs, last->reward, last->reward64, last->done, last->failed};
    const int grid = (n + POLICY_BLOCK - 1) / POLICY_BLOCK;
    const size_t lds = (size_t)pa.count * sizeof(float);   // at most 4 + 24 * 256 floats = 24 592 bytes
    mg::DeviceGuard guard(mg::device_of(state->pos));
    hipLaunchKernelGGL(pick_policy_kernel(simple, tasks != nullptr, vel), dim3(grid), dim3(POLICY_BLOCK), lds, (hipStream_t)stream,
                       k, *state, tt, pa, po, rec, io, n, n_steps);
    return mg::check_launch("quadrotor_policy_rollout_kernel");
}

extern "C" int32_t mg_quadrotor_rpolicy_param_count(int32_t hidden, int32_t obs_dim) {
    if (hidden < 1 || hidden > RPOLICY_MAX_HIDDEN) return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", hidden, RPOLICY_MAX_HIDDEN);
    if (obs_dim != OBS_DIM && obs_dim != OBS_DIM + 3) return mg::set_error(MG_ERR_BAD_CONFIG, "obs_dim=%d is neither 16 nor 19", obs_dim);
    return rp_count(hidden, obs_dim);
}

extern "C" int mg_quadrotor_rpolicy_rollout(const mg_quadrotor_config *cfg, const mg_quadrotor_tasks *tasks, int32_t n,
                                            int32_t n_steps, const mg_quadrotor_state *state, const mg_quadrotor_autoreset *ar,
                                            const mg_quadrotor_policy *policy, const mg_quadrotor_rpolicy_carry *carry,
                                            int32_t episodic, double *ret_total, double *ret_episode, int32_t *episode_len,
                                            const mg_quadrotor_policy_records *records, const mg_quadrotor_policy_last *last,
                                            void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_PTR(state);
    MG_REQUIRE_PTR(policy);
    MG_REQUIRE_PTR(carry);
    MG_REQUIRE_PTR(ret_total);
    MG_REQUIRE_PTR(ret_episode);
    MG_REQUIRE_PTR(episode_len);
    MG_REQUIRE_PTR(last);
    if (last->obs == nullptr || last->done == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_quadrotor_policy_last needs obs and done");
    if (policy->params_d == nullptr || policy->policy_id_d == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_quadrotor_policy needs params_d and policy_id_d");
    if (!carry->h || !carry->prev_action || !carry->prev_reward || !carry->prev_done)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_quadrotor_rpolicy_carry has a NULL array");
    if (n <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_envs=%d", n);
    if (n_steps <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_steps=%d", n_steps);
    if (policy->n_policies < 1) return mg::set_error(MG_ERR_BAD_SIZE, "n_policies=%d", policy->n_policies);
    if (policy->hidden < 1 || policy->hidden > RPOLICY_MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", policy->hidden, RPOLICY_MAX_HIDDEN);
    const bool vel = cfg->task == MG_QUADROTOR_TASK_VELOCITY_CONTROL;
    const int obs_dim = vel ? OBS_DIM + 3 : OBS_DIM;
    if (policy->obs_dim != obs_dim)
        return mg::set_error(MG_ERR_BAD_CONFIG, "policy obs_dim=%d, the task's observation has %d entries", policy->obs_dim, obs_dim);
    if (((uintptr_t)policy->params_d & 15u) != 0)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_quadrotor_policy.params_d must be 16-byte aligned");
    if (((uintptr_t)carry->prev_action & 15u) != 0)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_quadrotor_rpolicy_carry.prev_action must be 16-byte aligned");
    if (episodic != 0 && ar == nullptr)
        return mg::set_error(MG_ERR_BAD_CONFIG, "episodic clears the carry at a fused reset: it needs ar");
    QuadK k;
    TaskTable tt;
    bool simple;
    if (int rc = fold_policy_launch(cfg, tasks, state, ar, k, tt, simple)) return rc;
    const RpLds lds = rp_lds_layout(policy->hidden, obs_dim);
    RPolicyArgs pa{policy->params_d, policy->policy_id_d, policy->n_policies, policy->hidden, rp_count(policy->hidden, obs_dim),
                   carry->h, carry->prev_action, carry->prev_reward, carry->prev_done, episodic != 0};
    PolicyOut po{ret_total, ret_episode, episode_len};
    PolicyRec rec{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (records != nullptr) rec = PolicyRec{records->actions, records->obs, records->reward, records->reward64, records->done, records->failed};
    StepIO io{nullptr, last->obs, last->reward, last->reward64, last->done, last->failed};
    const int grid = (n + POLICY_BLOCK - 1) / POLICY_BLOCK;
    mg::DeviceGuard guard(mg::device_of(state->pos));
    hipLaunchKernelGGL(pick_rpolicy_kernel(simple, tasks != nullptr, vel), dim3(grid), dim3(POLICY_BLOCK), (size_t)lds.bytes,
                       (hipStream_t)stream, k, *state, tt, pa, po, rec, io, n, n_steps);
    return mg::check_launch("quadrotor_policy_rollout_kernel<RECURRENT>");
}
