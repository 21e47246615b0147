// maze3d_policy.hip — MetaMaze 3-D closed-loop rollouts: per-env recurrent policies that read the rendered frame
// (mg_maze3d_policy_param_count, mg_maze3d_pool_features, mg_maze3d_policy_rollout).
//
// A translation unit of its own on maze_core.h (load_task, load_agent, transition_discrete, transition_continuous, step_tail,
// Returns, rollout_records, the host checks). Same flags (metagym_amd/build.py): -ffp-contract=off, which is what makes the
// policy definition of include/metagym_hip.h hold (one rounding per operation).
//
// Launch pattern: mg_maze3d_expert_rollout's, one step per stretch. The host loop renders the frame of the state the envs
// hold (mg_maze3d_step's observe-only form, renderer untouched), then alternates one maze3d_policy_advance_kernel launch,
// which reads that frame, with one render.
//
// Mapping of the advance kernel: one wave per env, four envs per workgroup, no workgroup barrier (a wave never waits for
// another; the waves of a workgroup only share its LDS allocation).
//   pooling   the env's frame is one contiguous run of res_h * res_v * 3 elements. The lanes read it in 16-byte pieces, lane
//             q takes pieces q, q + 64, ... (a wave's read is 1 KiB contiguous), walk the 4 (int32) or 16 (uint8) elements of a
//             piece with running (row, column, channel, block) counters, add what falls into one grid block in registers
//             and flush a block's three sums into the wave's LDS bins with integer LDS adds when the block changes. Wrapping
//             integer addition is associative, so the order does not matter. A frame whose byte size is no multiple of 16
//             takes the element-by-element form of the same walk.
//   x, h      in LDS, as bit patterns in one int32 array (the bins become x in place); broadcast reads.
//   hidden    lane j < H owns unit j and walks the D + H inputs in ascending order; the weights are packed j-minor, so the
//             wave's read of one input's H weights is one coalesced line, served by L2 for every env after the first.
//   outputs   lanes k < K (4 logits or 2 steering outputs) walk j in ascending order.
//   env step  lane 0 runs maze3d_advance_kernel's step (the transition, step_tail) with the action taken from the outputs.
#include "maze_core.h"

#include "mg_closed_loop.h"

namespace {

constexpr int M3_WAVES = 4;                       // envs (waves) of a workgroup
constexpr int M3_BLOCK = M3_WAVES * mg::WAVE;
constexpr int M3_MAX_HIDDEN = 64;
constexpr int M3_MAX_GRID = 16;
constexpr int M3_MAX_INPUT = 3 * M3_MAX_GRID * M3_MAX_GRID + 6;   // 774
constexpr uint32_t M3_PHILOX_TAG = 0x4D33u;       // c3 of the exploration draw

__host__ __device__ constexpr int m3_pad4(int v) { return (v + 3) & ~3; }
__host__ __device__ constexpr int m3_features(int gh, int gv) { return 3 * gh * gv; }
__host__ __device__ constexpr int m3_outputs(bool cont) { return cont ? 2 : 4; }
__host__ __device__ constexpr int m3_input_dim(int gh, int gv, bool cont) { return m3_features(gh, gv) + (cont ? 4 : 6); }
// floats of one packed policy (include/metagym_hip.h writes the layout out): bo padded to 4, then with HS = H rounded up to a
// multiple of 4 the rows b, wx[.][0] .. wx[.][D-1], wh[.][0] .. wh[.][H-1], wo[0][.] .. wo[K-1][.] of HS floats each
__host__ __device__ constexpr int m3_count(int hidden, int d, int k) { return 4 + m3_pad4(hidden) * (1 + d + hidden + k); }

struct M3Wave {                                   // the LDS of one wave (one env)
    int32_t xb[M3_MAX_INPUT + 2];                 // the pooling bins, then the input x as float32 bit patterns
    float h[M3_MAX_HIDDEN], hn[M3_MAX_HIDDEN];
    float out[4];                                 // the logits / steering outputs
    int32_t clear;                                // episodic: the env's carry is cleared after this step
};

struct M3Frame {
    int res_h, res_v, gh, gv;
    int vec;                                      // the frames are 16-byte aligned and a multiple of 16 bytes long
    int fast;                                     // res_h * res_v < 2^22: m3_div may estimate in float32
    float r_res_v, r_bh, r_bv;                    // 1.0f / res_v, 1.0f / bh, 1.0f / bv
    float scale;
};
struct M3Policy {
    const float *__restrict__ params;             // [n_policies][count]
    const uint32_t *__restrict__ thr;             // [n_policies] or null (no exploration)
    const int32_t *__restrict__ ids;              // [n]
    int n_policies, hidden;
};

// what one lane wrote to the wave's LDS is there for the others (one wave: no s_barrier)
__device__ __forceinline__ void m3_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// z + w[0] * x(0) + w[1] * x(1) + ... in that order, one rounding per operation, w[i] at wp[i * stride]. The weights of U
// terms are loaded before the first of them is used, so the loads of a batch are in flight together; the sum itself is the
// sequential one of the definition.
template <int U, class X>
__device__ __forceinline__ float m3_dot(float z, const float *__restrict__ wp, int stride, int count, X &&x) {
    int i = 0;
    for (; i + U <= count; i += U) {
        float wv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) wv[u] = wp[(size_t)(i + u) * stride];
#pragma unroll
        for (int u = 0; u < U; ++u) z = z + wv[u] * x(i + u);
    }
    for (; i < count; ++i) z = z + wp[(size_t)i * stride] * x(i);
    return z;
}

// n / d for 0 <= n < 2^22 and d >= 1 without the integer division sequence: the float32 quotient estimate is within one of
// the truth (n and the product carry a relative error below 2^-22), the remainder says which way. `fast` = 0: plain division.
__device__ __forceinline__ int m3_div(int n, int d, float rd, int fast) {
    if (!fast) return n / d;
    int q = (int)((float)n * rd);
    const int r = n - q * d;
    q += r >= d ? 1 : (r < 0 ? -1 : 0);
    return q;
}

__device__ __forceinline__ void m3_bin_add(int32_t *xb, int at, int limit, uint32_t v) {
    if (v != 0u && at >= 0 && at < limit) atomicAdd(reinterpret_cast<unsigned int *>(xb) + at, v);
}

// The features of one env, by its wave: xb[(gh * Gv + gv) * 3 + c] = bits of float32(S[gh][gv][c]) * scale, S the int32 sum
// of the frame's block modulo 2^32. `f` is the env's frame, [res_h][res_v][3]. The caller synchronises the wave afterwards.
template <typename E>
__device__ __forceinline__ void m3_pool(const E *__restrict__ f, const M3Frame &fr, int lane, int32_t *xb) {
    constexpr int PER = 16 / (int)sizeof(E);
    const int nf = m3_features(fr.gh, fr.gv);
    const int bh = fr.res_h / fr.gh, bv = fr.res_v / fr.gv;
    const int total = fr.res_h * fr.res_v * 3;
    for (int i = lane; i < nf; i += mg::WAVE) xb[i] = 0;
    m3_wave_sync();
    if (fr.vec) {
        const uint4 *src = reinterpret_cast<const uint4 *>(f);
        const int pieces = total / PER;
        // one piece of a lane: its elements walked with running counters
        auto walk = [&](const uint4 &v, int q) {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const int p0 = q * PER;
            const int pix = p0 / 3;
            int c = p0 - pix * 3;
            int hh = m3_div(pix, fr.res_v, fr.r_res_v, fr.fast), vv = pix - hh * fr.res_v;
            int gh = m3_div(hh, bh, fr.r_bh, fr.fast), hb = hh - gh * bh;
            int gv = m3_div(vv, bv, fr.r_bv, fr.fast), vb = vv - gv * bv;
            uint32_t a0 = 0u, a1 = 0u, a2 = 0u;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const uint32_t val = sizeof(E) == 4 ? w[k & 3] : ((w[(k >> 2) & 3] >> (8 * (k & 3))) & 0xFFu);
                a0 += c == 0 ? val : 0u;
                a1 += c == 1 ? val : 0u;
                a2 += c == 2 ? val : 0u;
                if (++c < 3) continue;
                c = 0;                                                     // the next pixel
                ++vv;
                if (++vb < bv) continue;
                const int at = (gh * fr.gv + gv) * 3;                      // the next block: this one's sums go out
                m3_bin_add(xb, at, nf, a0);
                m3_bin_add(xb, at + 1, nf, a1);
                m3_bin_add(xb, at + 2, nf, a2);
                a0 = a1 = a2 = 0u;
                vb = 0;
                ++gv;
                if (vv < fr.res_v) continue;
                vv = 0;                                                    // the next row
                gv = 0;
                if (++hb == bh) { hb = 0; ++gh; }
            }
            const int at = (gh * fr.gv + gv) * 3;
            m3_bin_add(xb, at, nf, a0);
            m3_bin_add(xb, at + 1, nf, a1);
            m3_bin_add(xb, at + 2, nf, a2);
        };
        // four pieces per lane are loaded before the first is walked: 4 KiB of the frame in flight per wave
        constexpr int B = 4;
        for (int q0 = lane; q0 < pieces; q0 += B * mg::WAVE) {
            uint4 v[B];
#pragma unroll
            for (int u = 0; u < B; ++u) {
                const int q = q0 + u * mg::WAVE;
                v[u] = q < pieces ? src[q] : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int u = 0; u < B; ++u) {
                const int q = q0 + u * mg::WAVE;
                if (q < pieces) walk(v[u], q);
            }
        }
    } else {
        for (int p = lane; p < total; p += mg::WAVE) {
            const int pix = p / 3, c = p - pix * 3;
            const int hh = pix / fr.res_v, vv = pix - hh * fr.res_v;
            m3_bin_add(xb, ((hh / bh) * fr.gv + vv / bv) * 3 + c, nf, (uint32_t)f[p]);
        }
    }
    m3_wave_sync();
    for (int i = lane; i < nf; i += mg::WAVE) xb[i] = __float_as_int((float)xb[i] * fr.scale);   // int -> float32: nearest even
}

template <typename E>
__global__ __launch_bounds__(M3_BLOCK) void maze3d_pool_kernel(int n_envs, M3Frame fr, const E *__restrict__ frame,
                                                               float *__restrict__ out) {
    __shared__ int32_t bins[M3_WAVES][m3_features(M3_MAX_GRID, M3_MAX_GRID)];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int e = blockIdx.x * M3_WAVES + wave;
    if (e >= n_envs) return;                                               // (a whole wave; nothing waits for it)
    const int nf = m3_features(fr.gh, fr.gv);
    m3_pool<E>(frame + (size_t)e * ((size_t)fr.res_h * fr.res_v * 3), fr, lane, bins[wave]);
    m3_wave_sync();
    for (int i = lane; i < nf; i += mg::WAVE) out[(size_t)e * nf + i] = __int_as_float(bins[wave][i]);
}

// Step s of a closed-loop rollout for every env: the policy on the frame `frame` holds (the frame of the state the env is
// in), then maze3d_advance_kernel's step (the transition, step_tail). The returns travel from launch to launch through `po`
// (step 0 begins them: Returns), the policy's memory through `ca`.
template <bool CONT, typename E>
__global__ __launch_bounds__(M3_BLOCK) void maze3d_policy_advance_kernel(mg_maze_tasks T, mg_maze_state st, double col_dist,
                                                                         int task_type, int max_steps, int auto_reset, int n_envs,
                                                                         int s, M3Frame fr, const E *__restrict__ frame,
                                                                         M3Policy pa, mg_maze_policy_carry ca, uint64_t seed,
                                                                         uint64_t step0, int episodic, RolloutOut po, RolloutRec rec) {
    __shared__ M3Wave lds[M3_WAVES];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int e = blockIdx.x * M3_WAVES + wave;
    if (e >= n_envs) return;                                               // (a whole wave; nothing waits for it)
    M3Wave &w = lds[wave];
    constexpr int K = m3_outputs(CONT);
    const int H = pa.hidden, HS = m3_pad4(H);
    const int NF = m3_features(fr.gh, fr.gv), D = m3_input_dim(fr.gh, fr.gv, CONT);

    // The env's policy id, clamped, and its carry are asked for before the pooling, so these round trips run under it. The
    // task row and the agent are not: some thirty live values across the pooling and the hidden layer cost two waves per
    // SIMD, and the kernel is bound by latency inside a wave, where occupancy is what hides it.
    const int pid = mg::clamp_index(pa.ids[e], pa.n_policies);
    const float *__restrict__ p = pa.params + (size_t)pid * (size_t)m3_count(H, D, K);
    const uint32_t thr = (!CONT && pa.thr != nullptr) ? pa.thr[pid] : 0u;
    float *prev_cont = static_cast<float *>(static_cast<void *>(ca.prev_action)) + 2 * (size_t)e;   // CONT: f32 [N][2]
    const float prev_a0 = CONT ? prev_cont[0] : 0.0f, prev_a1 = CONT ? prev_cont[1] : 0.0f;
    const int prev_act = CONT ? 0 : ca.prev_action[e];
    const float prev_reward = ca.prev_reward[e];
    const int prev_done = ca.prev_done[e] != 0;
    const float h_in = lane < H ? ca.h[(size_t)e * H + lane] : 0.0f;
    const float b_in = lane < H ? p[4 + lane] : 0.0f;

    m3_pool<E>(frame + (size_t)e * ((size_t)fr.res_h * fr.res_v * 3), fr, lane, w.xb);
    if (lane == 0) {
        if (CONT) {
            w.xb[NF] = __float_as_int(prev_a0);
            w.xb[NF + 1] = __float_as_int(prev_a1);
        } else {
            for (int k = 0; k < 4; ++k) w.xb[NF + k] = __float_as_int(prev_act == k ? 1.0f : 0.0f);
        }
        w.xb[D - 2] = __float_as_int(prev_reward);
        w.xb[D - 1] = __float_as_int(prev_done ? 1.0f : 0.0f);
        w.clear = 0;
    }
    if (lane < H) w.h[lane] = h_in;
    m3_wave_sync();

    float hn = 0.0f;
    if (lane < H) {
        const float *__restrict__ wp = p + 4 + HS + lane;                  // wx[lane][i] at wp[i * HS]
        float z = b_in;
        z = m3_dot<16>(z, wp, HS, D, [&](int i) { return __int_as_float(w.xb[i]); });
        wp += (size_t)D * HS;                                              // wh[lane][i] at wp[i * HS]
        z = m3_dot<16>(z, wp, HS, H, [&](int i) { return w.h[i]; });
        hn = z > 1.0f ? 1.0f : (z < -1.0f ? -1.0f : z);                    // a NaN stays NaN, -0 stays -0
        w.hn[lane] = hn;
    }
    m3_wave_sync();
    if (lane < K) {
        const float *__restrict__ wo = p + 4 + (size_t)HS * (1 + D + H) + (size_t)lane * HS;
        w.out[lane] = m3_dot<16>(p[lane], wo, 1, H, [&](int j) { return w.hn[j]; });
    }
    m3_wave_sync();

    if (lane == 0) {
        const Task t = load_task(T, mg::clamp_index(st.task_id[e], T.n_tasks));
        Agent a = load_agent(st, n_envs, e);
        const size_t r_at = (size_t)s * n_envs + e;
        int act = 0;
        float turn = 0.0f, walk = 0.0f;
        if (CONT) {
            const float l0 = w.out[0], l1 = w.out[1];
            turn = l0 != l0 ? 0.0f : (l0 > 1.0f ? 1.0f : (l0 < -1.0f ? -1.0f : l0));
            walk = l1 != l1 ? 0.0f : (l1 > 1.0f ? 1.0f : (l1 < -1.0f ? -1.0f : l1));
            if (rec.actions) {
                float *ac = static_cast<float *>(rec.actions) + 2 * r_at;
                ac[0] = turn;
                ac[1] = walk;
            }
            transition_continuous(t, col_dist, turn, walk, a);
        } else {
            float best = w.out[0];                                         // ties and NaN logits: the lowest index
            if (w.out[1] > best) { act = 1; best = w.out[1]; }
            if (w.out[2] > best) { act = 2; best = w.out[2]; }
            if (w.out[3] > best) { act = 3; }
            uint32_t word;
            if (mg::explore_draw((uint32_t)e, step0 + (uint64_t)s, M3_PHILOX_TAG, seed, thr, word)) act = (int)(word & 3u);
            if (rec.actions) static_cast<int32_t *>(rec.actions)[r_at] = act;
            transition_discrete(t, act, a);
        }
        double r;
        const int d = step_tail(t, st, e, task_type, max_steps, auto_reset, a, r_at, rec.reward, rec.reward64, rec.done, r);
        Returns ret;
        if (s > 0) ret.load(po, e);
        ret.add(r, d);
        store_agent(st, n_envs, e, a);
        ret.store(po, e);
        // the carry: the action as it was stepped with, the reward as the record holds it
        const bool clear = episodic && d && auto_reset;                    // the next episode starts from a fresh carry
        if (CONT) {
            prev_cont[0] = clear ? 0.0f : turn;
            prev_cont[1] = clear ? 0.0f : walk;
        } else {
            ca.prev_action[e] = clear ? -1 : act;
        }
        ca.prev_reward[e] = clear ? 0.0f : (float)r;
        ca.prev_done[e] = clear ? (uint8_t)0 : (uint8_t)d;
        w.clear = clear ? 1 : 0;
    }
    m3_wave_sync();
    if (lane < H) ca.h[(size_t)e * H + lane] = w.clear ? 0.0f : hn;
}

int m3_check_grid(const mg_maze_view *view, int gh, int gv, const char *who) {
    if (view->res_h < 1 || view->res_v < 1) return mg::set_error(MG_ERR_BAD_SIZE, "%s: resolution %d x %d", who, view->res_h, view->res_v);
    if (gh < 1 || gh > M3_MAX_GRID || gv < 1 || gv > M3_MAX_GRID)
        return mg::set_error(MG_ERR_BAD_SIZE, "%s: grid %d x %d is outside [1, %d]", who, gh, gv, M3_MAX_GRID);
    if (view->res_h % gh != 0 || view->res_v % gv != 0)
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: grid %d x %d does not divide the resolution %d x %d", who, gh, gv, view->res_h,
                             view->res_v);
    return MG_OK;
}

M3Frame m3_frame(const mg_maze_view *view, int gh, int gv, float scale, const void *frame) {
    const size_t bytes = (size_t)view->res_h * view->res_v * 3 * (view->obs_format == 1 ? 1 : sizeof(int32_t));
    M3Frame fr;
    fr.res_h = view->res_h;
    fr.res_v = view->res_v;
    fr.gh = gh;
    fr.gv = gv;
    fr.vec = (bytes % 16 == 0 && ((uintptr_t)frame & 15u) == 0) ? 1 : 0;
    fr.fast = (long long)view->res_h * view->res_v < (1LL << 22) ? 1 : 0;
    fr.r_res_v = 1.0f / (float)view->res_v;
    fr.r_bh = 1.0f / (float)(view->res_h / gh);
    fr.r_bv = 1.0f / (float)(view->res_v / gv);
    fr.scale = scale;
    return fr;
}

}  // namespace

extern "C" int32_t mg_maze3d_policy_param_count(int32_t hidden, int32_t grid_h, int32_t grid_v, int32_t continuous) {
    if (hidden < 1 || hidden > M3_MAX_HIDDEN) return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", hidden, M3_MAX_HIDDEN);
    if (grid_h < 1 || grid_h > M3_MAX_GRID || grid_v < 1 || grid_v > M3_MAX_GRID)
        return mg::set_error(MG_ERR_BAD_SIZE, "grid %d x %d is outside [1, %d]", grid_h, grid_v, M3_MAX_GRID);
    return m3_count(hidden, m3_input_dim(grid_h, grid_v, continuous != 0), m3_outputs(continuous != 0));
}

extern "C" int mg_maze3d_pool_features(const mg_maze_view *view, int32_t n, const void *frame, int32_t grid_h, int32_t grid_v,
                                       float scale, float *out, void *stream) {
    MG_REQUIRE_PTR(view);
    MG_REQUIRE_PTR(frame);
    MG_REQUIRE_PTR(out);
    if (n <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "n_envs=%d", n);
    if (int rc = m3_check_grid(view, grid_h, grid_v, "mg_maze3d_pool_features")) return rc;
    const M3Frame fr = m3_frame(view, grid_h, grid_v, scale, frame);
    const dim3 grid((unsigned)((n + M3_WAVES - 1) / M3_WAVES)), block(M3_BLOCK);
    mg::DeviceGuard guard(mg::device_of(out));
    if (view->obs_format == 1)
        hipLaunchKernelGGL(maze3d_pool_kernel<uint8_t>, grid, block, 0, (hipStream_t)stream, n, fr, static_cast<const uint8_t *>(frame), out);
    else
        hipLaunchKernelGGL(maze3d_pool_kernel<int32_t>, grid, block, 0, (hipStream_t)stream, n, fr, static_cast<const int32_t *>(frame), out);
    return mg::check_launch("maze3d_pool_kernel");
}

extern "C" int mg_maze3d_policy_rollout(const mg_maze_tasks *T, const mg_maze_view *view, int32_t task_type, int32_t max_steps,
                                        int32_t continuous, int32_t auto_reset, int32_t n, const mg_maze_state *st,
                                        int32_t n_steps, int32_t obs_every, const mg_maze3d_policy *policy,
                                        const int32_t *policy_ids, const mg_maze_policy_carry *carry, uint64_t seed,
                                        uint64_t step0, int32_t episodic, void *frame, void *obs, double *ret_total,
                                        double *ret_episode, int32_t *episode_len, int32_t *episodes, void *actions,
                                        float *reward, double *reward64, uint8_t *done, void *stream) {
    MG_REQUIRE_PTR(policy);
    MG_REQUIRE_PTR(policy_ids);
    MG_REQUIRE_PTR(carry);
    MG_REQUIRE_PTR(frame);
    MG_REQUIRE_PTR(ret_total);
    MG_REQUIRE_PTR(ret_episode);
    MG_REQUIRE_PTR(episode_len);
    MG_REQUIRE_PTR(episodes);
    if (policy->params == nullptr) return mg::set_error(MG_ERR_NULL_POINTER, "mg_maze3d_policy needs params");
    if (!carry->h || !carry->prev_action || !carry->prev_reward || !carry->prev_done)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_maze_policy_carry has a NULL array");
    if (n_steps < 1) return mg::set_error(MG_ERR_BAD_SIZE, "mg_maze3d_policy_rollout: n_steps=%d (at least 1)", n_steps);
    if (obs_every < 0) return mg::set_error(MG_ERR_BAD_SIZE, "mg_maze3d_policy_rollout: obs_every=%d (0 = the last step only, k >= 1 = every k-th)", obs_every);
    if (policy->n_policies < 1) return mg::set_error(MG_ERR_BAD_SIZE, "n_policies=%d", policy->n_policies);
    if (policy->hidden < 1 || policy->hidden > M3_MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", policy->hidden, M3_MAX_HIDDEN);
    if ((policy->continuous != 0) != (continuous != 0))
        return mg::set_error(MG_ERR_BAD_CONFIG, "the policy has the %s form, the env is %s", policy->continuous ? "steering" : "discrete",
                             continuous ? "continuous" : "discrete");
    if (((uintptr_t)policy->params & 15u) != 0)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_maze3d_policy.params must be 16-byte aligned");
    MG_REQUIRE_PTR(view);
    if (int rc = m3_check_grid(view, policy->grid_h, policy->grid_v, "mg_maze3d_policy_rollout")) return rc;
    const int bh = view->res_h / policy->grid_h, bv = view->res_v / policy->grid_v;
    if (policy->scale != (float)(1.0 / (255.0 * (double)bh * (double)bv)))
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_maze3d_policy.scale=%.9g is not float32(1 / (255 * %d * %d))", (double)policy->scale, bh, bv);
    // everything mg_maze3d_step refuses (NULL tasks / state, n_envs < 1, ...), before the first launch
    if (int rc = mg_maze3d_step_check(T, view, task_type, max_steps, continuous, auto_reset, n, st, frame, stream)) return rc;
    const size_t frame_bytes = (size_t)n * view->res_h * view->res_v * 3 * (view->obs_format == 1 ? 1 : sizeof(int32_t));
    unsigned char *slice = static_cast<unsigned char *>(obs);
    const M3Policy pa{policy->params, policy->eps_threshold, policy_ids, policy->n_policies, policy->hidden};
    const RolloutOut po{nullptr, ret_total, ret_episode, episode_len, episodes};
    const RolloutRec rec{actions, reward, reward64, done, nullptr};
    const dim3 grid((unsigned)((n + M3_WAVES - 1) / M3_WAVES)), block(M3_BLOCK);
    const bool u8 = view->obs_format == 1;
    // the frame of the state the envs hold now: the buffer may be stale (load_state_dict, a rollout that kept slices)
    if (int rc = mg_maze3d_step(T, view, task_type, max_steps, continuous, auto_reset, n, st, nullptr, frame, nullptr, nullptr,
                                nullptr, stream)) return rc;
    const void *cur = frame;
    for (int s = 0; s < n_steps; ++s) {
        {
            mg::DeviceGuard guard(mg::device_of(st->grid));
            // (a slice of obs is n frames past a 16-byte aligned base: whether it is aligned is decided per launch)
            const M3Frame fr = m3_frame(view, policy->grid_h, policy->grid_v, policy->scale, cur);
#define MG_M3_LAUNCH(CONT_, E_)                                                                                              \
    hipLaunchKernelGGL((maze3d_policy_advance_kernel<CONT_, E_>), grid, block, 0, (hipStream_t)stream, *T, *st,                \
                       view->collision_dist, task_type, max_steps, auto_reset, n, s, fr, static_cast<const E_ *>(cur), pa, *carry, \
                       seed, step0, episodic, po, rec)
            if (continuous) { if (u8) MG_M3_LAUNCH(true, uint8_t); else MG_M3_LAUNCH(true, int32_t); }
            else { if (u8) MG_M3_LAUNCH(false, uint8_t); else MG_M3_LAUNCH(false, int32_t); }
#undef MG_M3_LAUNCH
            if (int rc = mg::check_launch("maze3d_policy_advance_kernel")) return rc;
        }
        // the frame of the state the step left: into the next slice when the step is recorded, else the persistent buffer
        void *dst = frame;
        if (obs != nullptr && rollout_records(s, n_steps, obs_every)) {
            dst = slice;
            slice += frame_bytes;
        }
        if (int rc = mg_maze3d_step(T, view, task_type, max_steps, continuous, auto_reset, n, st, nullptr, dst, nullptr, nullptr,
                                    nullptr, stream)) return rc;
        cur = dst;
    }
    return MG_OK;
}
