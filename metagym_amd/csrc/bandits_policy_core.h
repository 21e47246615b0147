// bandits_policy_core.h — what the two bandits policy units share: bandits_policy.hip (mg_bandits_policy_rollout, the greedy
// instantiation) and bandits_policy_sampled.hip (mg_bandits_policy_rollout_sampled, the softmax-sampled one). The packed
// layout, the LDS layout, the policy evaluation, the rollout kernel as a template on SAMPLED and the host checks with the
// launch. The kernel is a template: a unit emits the instantiation it launches and no other, so each of the two units still
// carries exactly one kernel (a non-template __global__ stays in the .hip that launches it). Everything is in
// the anonymous namespace. Include bandits_core.h first.
#pragma once
#include "bandits_core.h"

#include "mg_closed_loop.h"
#include "mg_sample.h"

namespace {

constexpr int BP_BLOCK = mg::WAVE;
constexpr int BP_MAX_HIDDEN = 64;
constexpr int BP_MAX_ARMS = 64;
constexpr uint32_t BP_PHILOX_TAG = 0x4241u;      // c3 of the exploration draw

typedef float bp_v4f __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int bp_pad4(int n) { return (n + 3) & ~3; }
// floats of one hidden unit's record: b[j], wr[j], wd[j], 0, wa[j][0..K-1] and zeros up to KP, wh[j][0..H-1] and zeros up to HP
__host__ __device__ constexpr int bp_unit_record(int hidden, int arms) { return 4 + bp_pad4(arms) + bp_pad4(hidden); }
// floats of one arm's record: bo[k], 0, 0, 0, wo[k][0..H-1] and zeros up to HP
__host__ __device__ constexpr int bp_arm_record(int hidden) { return 4 + bp_pad4(hidden); }
// floats of one packed policy: H unit records, then K arm records (every record is a multiple of four floats)
__host__ __device__ constexpr int bp_count(int hidden, int arms) {
    return hidden * bp_unit_record(hidden, arms) + arms * bp_arm_record(hidden);
}

// The dynamic LDS of one workgroup, in bytes from its 16-byte aligned base: the staged policy, the two lane-minor state
// buffers and the 624 words of the stream refill (Streams::lds). One function for the launch and the kernel.
struct BpLds { int policy, h0, h1, mt, bytes; };
__host__ __device__ inline BpLds bp_lds_layout(int hidden, int arms) {
    BpLds l;
    l.policy = 0;
    l.h0 = bp_count(hidden, arms) * (int)sizeof(float);                       // (a multiple of 16)
    l.h1 = l.h0 + hidden * BP_BLOCK * (int)sizeof(float);
    l.mt = l.h1 + hidden * BP_BLOCK * (int)sizeof(float);
    l.bytes = l.mt + MTN * (int)sizeof(uint32_t);
    return l;
}

struct BpPolicy {
    const float *__restrict__ params;       // [n_policies][count]
    const uint32_t *__restrict__ thr;       // [n_policies] or null (no exploration)
    const int32_t *__restrict__ ids;        // [n]
    int n_policies, hidden;
};
struct BpOut {                              // [n] each
    double *ret_total, *ret_episode;
    int32_t *episode_len, *episodes;
    double *regret;
};
struct BpRec {                              // [T][n] each; each may be null
    int32_t *actions;
    float *reward;
    uint8_t *done;
    int32_t *info_steps;
    double *expected_gain, *best_gain;
    uint8_t *invalid;
};

// The policy of include/metagym_hip.h on one packed parameter block, from LDS (every lane the same address: broadcast reads,
// but for wa[j][prev_action], which is the lane's own) or from global memory (each lane its own block). h and hn are the
// lane's columns of the two LDS state buffers. Both loops over the records run at run time; the loops over h read four
// weights per 16-byte read and skip the padding (0 * h added to a sum of -0 would turn it into +0, and 0 * NaN is NaN).
// Returns the greedy action; SAMPLED: the Gumbel-max draw, the same running argmax over score[k] = l[k] * inv_t + g[k]
// (mg_sample.h), with one Philox block per four arms. Neither the logits nor the scores are stored.
template <bool SAMPLED>
__device__ __forceinline__ int bp_eval(const float *__restrict__ p, int hidden, int arms, int prev_action, float prev_reward,
                                       float prev_done, const float *h, float *hn, float inv_t, uint32_t env, uint64_t step,
                                       uint64_t seed) {
    const int hp = bp_pad4(hidden), kp = bp_pad4(arms);
    const int ur = 4 + kp + hp, ar = 4 + hp;
    const bool looked_up = prev_action >= 0 && prev_action < arms;     // the one-hot is a lookup: one add, or none
#pragma unroll 1
    for (int j = 0; j < hidden; ++j) {
        const float *r = p + ur * j;
        const bp_v4f c = *reinterpret_cast<const bp_v4f *>(r);          // b, wr, wd, 0
        float z = c.x;
        if (looked_up) z = z + r[4 + prev_action];
        z = z + c.y * prev_reward;
        z = z + c.z * prev_done;
        const float *rh = r + 4 + kp;
#pragma unroll 1
        for (int i = 0; i < hp; i += 4) {
            const bp_v4f v = *reinterpret_cast<const bp_v4f *>(rh + i);
            z = z + v.x * h[i * BP_BLOCK];
            if (i + 1 < hidden) z = z + v.y * h[(i + 1) * BP_BLOCK];
            if (i + 2 < hidden) z = z + v.z * h[(i + 2) * BP_BLOCK];
            if (i + 3 < hidden) z = z + v.w * h[(i + 3) * BP_BLOCK];
        }
        hn[j * BP_BLOCK] = z > 1.0f ? 1.0f : (z < -1.0f ? -1.0f : z);  // a NaN stays NaN, -0 stays -0
    }
    const float *q = p + ur * hidden;
    int g = 0;                                                           // ties and NaN logits: the lowest index
    float best = 0.0f;
    uint32_t o[4] = {0u, 0u, 0u, 0u};                                    // SAMPLED: o[0] is the word of arm k
#pragma unroll 1
    for (int k = 0; k < arms; ++k) {
        const float *r = q + ar * k;
        float l = r[0];
#pragma unroll 1
        for (int i = 0; i < hp; i += 4) {
            const bp_v4f v = *reinterpret_cast<const bp_v4f *>(r + 4 + i);
            l = l + v.x * hn[i * BP_BLOCK];
            if (i + 1 < hidden) l = l + v.y * hn[(i + 1) * BP_BLOCK];
            if (i + 2 < hidden) l = l + v.z * hn[(i + 2) * BP_BLOCK];
            if (i + 3 < hidden) l = l + v.w * hn[(i + 3) * BP_BLOCK];
        }
        if (SAMPLED) {
            if ((k & 3) == 0) mg::sample_block(env, step, (uint32_t)k >> 2, seed, o);
            l = mg::sample_score(l, inv_t, o[0]);
            o[0] = o[1]; o[1] = o[2]; o[2] = o[3];
        }
        mg::take_if_greater(k, l, g, best);                               // best is l[greedy] (score[action])
    }
    return g;
}

// best = row[0]; for k >= 1: if row[k] > best
__device__ __forceinline__ double bp_best(const double *row, int arms) {
    double best = row[0];
    for (int i = 1; i < arms; ++i) {
        const double v = row[i];
        if (v > best) best = v;
    }
    return best;
}

// bandits_step_kernel's step body in its order (one double, then the reward; at the end of an episode with auto_reset the
// task draw, then the restart), with the action load replaced by the policy. Inside the step loop the kernel stores only
// what `rec` asks for; the env state, the carry and the five per-env results go out once, at the end.
// SAMPLED: the action is drawn from softmax(l / temperature) (inv_t [n_policies], read once per env); an exploratory draw
// still overrides it. The greedy instantiation reads no inv_t (it is passed NULL).
template <bool SAMPLED>
__global__ __launch_bounds__(BP_BLOCK) void bandits_policy_rollout_kernel(BanditsK k, int n, int T, mg_bandits_state s,
                                                                          BpPolicy pa, mg_maze_policy_carry ca, uint64_t seed,
                                                                          uint64_t step0, int episodic, BpOut po, BpRec rec,
                                                                          const float *__restrict__ inv_temperature) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int H = pa.hidden, K = k.K;
    const BpLds lds = bp_lds_layout(H, K);
    const int lane = threadIdx.x, e0 = blockIdx.x * BP_BLOCK, e = e0 + lane;
    const bool live = e < n;
    const int el = live ? e : n - 1;   // spare lanes shadow the last env's policy and carry; they step nothing and store nothing
    const float *policy_lds = reinterpret_cast<const float *>(smem + lds.policy);
    float *hc = reinterpret_cast<float *>(smem + lds.h0) + lane;           // the lane's column: h[j] at hc[j * 64]
    float *hx = reinterpret_cast<float *>(smem + lds.h1) + lane;

    // The env's policy, clamped. One id in the whole wave (a ballot: wave-uniform): stage it in LDS once.
    const int count = bp_count(H, K);
    int pid = pa.ids[el];
    pid = pid < 0 ? 0 : (pid >= pa.n_policies ? pa.n_policies - 1 : pid);
    const int pid0 = __builtin_amdgcn_readfirstlane(pid);
    const bool staged = __builtin_amdgcn_ballot_w64(pid != pid0) == 0;
    const float *__restrict__ own = pa.params + (size_t)pid * (size_t)count;
    if (staged) {
        const bp_v4f *src = reinterpret_cast<const bp_v4f *>(pa.params + (size_t)pid0 * (size_t)count);
        bp_v4f *dst = reinterpret_cast<bp_v4f *>(smem + lds.policy);
        for (int i = lane; i < count / 4; i += BP_BLOCK) dst[i] = src[i];
    }
    const uint32_t thr = pa.thr != nullptr ? pa.thr[pid] : 0u;
    const float inv_t = SAMPLED ? inv_temperature[pid] : 0.0f;

    int steps = 0, over = 1, has_gauss = 0;
    double gauss = 0.0;
    Streams g{s.mt, reinterpret_cast<uint32_t *>(smem + lds.mt), e0, lane, n, MTN};
    double *row = s.gains + (size_t)el * (size_t)K;
    double best = 0.0;
    if (live) {
        steps = s.steps[e];
        over = s.over[e];
        has_gauss = s.has_gauss[e];
        gauss = s.gauss[e];
        g.pos = (int)min(s.mt[(size_t)e * REC + MTN], (uint32_t)MTN);
        best = bp_best(row, K);
    }
    for (int j = 0; j < H; ++j) hc[j * BP_BLOCK] = ca.h[(size_t)el * H + j];
    int prev_action = ca.prev_action[el];
    float prev_reward = ca.prev_reward[el];
    int prev_done = ca.prev_done[el] != 0;
    __syncthreads();                                                       // (one wave) the staged policy is in place

    double ret_total = 0.0, ret_episode = 0.0, regret = 0.0;
    int episode_len = 0, episodes = 0;
    bool first_done = false;

    for (int t = 0; t < T; ++t) {
        const bool act = live && !over;                                    // an env that is over does nothing in this step
        const uint64_t c = step0 + (uint64_t)t;
        int a = staged ? bp_eval<SAMPLED>(policy_lds, H, K, prev_action, prev_reward, prev_done ? 1.0f : 0.0f, hc, hx, inv_t,
                                          (uint32_t)el, c, seed)
                       : bp_eval<SAMPLED>(own, H, K, prev_action, prev_reward, prev_done ? 1.0f : 0.0f, hc, hx, inv_t,
                                          (uint32_t)el, c, seed);
        if (thr != 0u) {
            uint32_t o[4];
            philox4x32_10((uint32_t)el, (uint32_t)c, (uint32_t)(c >> 32), BP_PHILOX_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), o);
            if (o[0] < thr) a = (int)(o[1] % (uint32_t)K);
        }
        if (act) { float *sw = hc; hc = hx; hx = sw; }                     // h = hn (an env that is over keeps its memory)

        const size_t at = (size_t)t * (size_t)n + (size_t)e;
        const double d = g.next_double(act);                               // every lane: the refill is collective
        bool ended = false;
        if (act) {
            const double gain = row[a];
            const int before = steps++;
            ended = steps >= k.max_steps;
            const float r = d < gain ? 1.0f : 0.0f;
            if (rec.actions) rec.actions[at] = a;
            if (rec.reward) rec.reward[at] = r;
            if (rec.done) rec.done[at] = ended;
            if (rec.info_steps) rec.info_steps[at] = before;
            if (rec.expected_gain) rec.expected_gain[at] = gain;
            if (rec.best_gain) rec.best_gain[at] = best;
            if (rec.invalid) rec.invalid[at] = 0;
            if (ended) over = 1;
            // the returns and the regret: float64 sums in step order; the episode's stops with the first done
            ret_total = ret_total + (double)r;
            if (!first_done) {
                ret_episode = ret_episode + (double)r;
                episode_len += 1;
                first_done = ended;
            }
            episodes += ended;
            regret = regret + (best - gain);
            prev_action = a;
            prev_reward = r;
            prev_done = ended;
        } else if (live) {
            if (rec.actions) rec.actions[at] = -1;
            if (rec.reward) rec.reward[at] = 0.0f;
            if (rec.done) rec.done[at] = 0;
            if (rec.info_steps) rec.info_steps[at] = steps;
            if (rec.expected_gain) rec.expected_gain[at] = 0.0;
            if (rec.best_gain) rec.best_gain[at] = 0.0;
            if (rec.invalid) rec.invalid[at] = 2;
        }
        if (k.auto_reset) {
            if (k.dist != MG_BANDITS_NONE && __ballot(ended)) {
                sample_task(k, g, ended, has_gauss, gauss, row);
                if (ended) best = bp_best(row, K);
            }
            if (ended) {
                steps = 0;
                over = 0;
                if (episodic) {                                            // the next episode starts from a fresh carry
                    for (int j = 0; j < H; ++j) hc[j * BP_BLOCK] = 0.0f;
                    prev_action = -1;
                    prev_reward = 0.0f;
                    prev_done = 0;
                }
            }
        }
    }
    if (!live) return;
    s.steps[e] = steps;
    s.over[e] = (uint8_t)over;
    s.has_gauss[e] = has_gauss;
    s.gauss[e] = gauss;
    s.mt[(size_t)e * REC + MTN] = (uint32_t)g.pos;
    for (int j = 0; j < H; ++j) ca.h[(size_t)e * H + j] = hc[j * BP_BLOCK];
    ca.prev_action[e] = prev_action;
    ca.prev_reward[e] = prev_reward;
    ca.prev_done[e] = (uint8_t)prev_done;
    po.ret_total[e] = ret_total;
    po.ret_episode[e] = ret_episode;
    po.episode_len[e] = episode_len;
    po.episodes[e] = episodes;
    po.regret[e] = regret;
}

// The two entry points: every check, then the launch of the greedy or the sampled instantiation. `name` is the entry point's.
template <bool SAMPLED>
int bandits_policy_rollout(const char *name, const mg_bandits_config *cfg, int32_t n_envs, const mg_bandits_state *state,
                           int32_t n_steps, const mg_bandits_policy *policy, const int32_t *policy_ids,
                           const mg_bandits_policy_carry *carry, const float *inv_temperature, uint64_t seed, uint64_t step0,
                           int32_t episodic, double *ret_total, double *ret_episode, int32_t *episode_len, int32_t *episodes,
                           double *regret, int32_t *actions, float *reward, uint8_t *done, int32_t *info_steps,
                           double *expected_gain, double *best_gain, uint8_t *invalid, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_STATE(state);
    MG_REQUIRE_PTR(policy);
    MG_REQUIRE_PTR(policy_ids);
    MG_REQUIRE_PTR(carry);
    if (SAMPLED) MG_REQUIRE_PTR(inv_temperature);
    MG_REQUIRE_PTR(ret_total);
    MG_REQUIRE_PTR(ret_episode);
    MG_REQUIRE_PTR(episode_len);
    MG_REQUIRE_PTR(episodes);
    MG_REQUIRE_PTR(regret);
    if (policy->params == nullptr) return mg::set_error(MG_ERR_NULL_POINTER, "mg_bandits_policy needs params");
    if (!carry->h || !carry->prev_action || !carry->prev_reward || !carry->prev_done)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_bandits_policy_carry has a NULL array");
    int rc = check_config(cfg, name);
    if (rc != MG_OK) return rc;
    if (n_envs <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "%s: n_envs = %d", name, n_envs);
    if (n_steps < 1) return mg::set_error(MG_ERR_BAD_SIZE, "%s: n_steps = %d (at least 1)", name, n_steps);
    if (policy->n_policies < 1) return mg::set_error(MG_ERR_BAD_SIZE, "n_policies=%d", policy->n_policies);
    if (policy->hidden < 1 || policy->hidden > BP_MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", policy->hidden, BP_MAX_HIDDEN);
    if (policy->arms < 2 || policy->arms > BP_MAX_ARMS)
        return mg::set_error(MG_ERR_BAD_SIZE, "arms=%d is outside [2, %d]", policy->arms, BP_MAX_ARMS);
    if (policy->arms != cfg->arms)
        return mg::set_error(MG_ERR_BAD_CONFIG, "the policy was built for arms=%d, the env has %d", policy->arms, cfg->arms);
    if (((uintptr_t)policy->params & 15u) != 0)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_bandits_policy.params must be 16-byte aligned");
    const BpLds lds = bp_lds_layout(policy->hidden, policy->arms);
    if ((size_t)lds.bytes > mg::LDS_LIMIT)
        return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d arms=%d needs %d B of LDS (> 160 KiB)", policy->hidden, policy->arms, lds.bytes);
    mg::DeviceGuard guard(mg::device_of(state->mt));
    if (int rc = mg::opt_in_dynamic_lds(bandits_policy_rollout_kernel<SAMPLED>, lds.bytes, "bandits_policy_rollout_kernel")) return rc;
    BpPolicy pa{policy->params, policy->eps_threshold, policy_ids, policy->n_policies, policy->hidden};
    BpOut po{ret_total, ret_episode, episode_len, episodes, regret};
    BpRec rec{actions, reward, done, info_steps, expected_gain, best_gain, invalid};
    hipLaunchKernelGGL(bandits_policy_rollout_kernel<SAMPLED>, dim3((unsigned)(((int64_t)n_envs + BP_BLOCK - 1) / BP_BLOCK)), dim3(BP_BLOCK),
                       (size_t)lds.bytes, static_cast<hipStream_t>(stream), fold(cfg), n_envs, n_steps, *state, pa, *carry, seed,
                       step0, episodic, po, rec, inv_temperature);
    return mg::check_launch("bandits_policy_rollout_kernel");
}

}  // namespace
