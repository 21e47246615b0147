// bandits_learner.hip — Bandits closed-loop rollouts with a classical learner inside the launch (mg_bandits_learner_*):
// greedy on a Beta prior, UCB, an index table (Gittins) and Thompson sampling, each defined exactly in include/metagym_hip.h.
//
// A translation unit of its own on bandits_core.h (Streams, sample_task, BanditsK, the host checks). Same flags
// (metagym_amd/build.py): -ffp-contract=off, which is what makes the definition hold (one rounding per operation); `/` and
// sqrtf are the correctly rounded float32 operations.
//
// Mapping: bandits_policy_rollout_kernel's — one lane per env, one wave per workgroup. The env scalars, the running argmax
// and the five results live in registers for n_steps steps; the two count arrays live in LDS lane-minor
// (cnt[(2 k + which) * 64 + lane], which = 0 pulls, 1 wins) next to the 624 words of the stream refill: 35 264 B at K = 64.
// The kind is a template parameter: greedy, UCB and the table do not pay the sampler's registers. The sampler's one loop
// over (arm, draw, attempt) has a length of its own in every lane and holds no collective. The refill inside Streams::next is a
// workgroup-collective (__syncthreads): the env half of a step is reached by all 64 lanes at every step, with act = false
// for the lanes that draw nothing. Table rows are read per lane from global memory; lanes sharing a row hit in cache.
//
// log32 and u01 live in mg_sample.h (mg::log32, mg::u01), shared with the softmax-sampled policies; their operation sequence
// is the one this unit was written with. log32's constants by their bits, as the header defines them: Lg1 0x3f2aaaaau,
// Lg2 0x3eccce13u, Lg3 0x3e91e9eeu, Lg4 0x3e789e26u, ln2_hi 0x3f317180u, ln2_lo 0x3717f7d1u, sqrt(1/2) 0x3f3504f3u.
#include "bandits_core.h"

#include "mg_philox.h"
#include "mg_sample.h"

namespace {

constexpr int BL_BLOCK = mg::WAVE;
constexpr int BL_MAX_ARMS = 64;
constexpr int BL_MAX_CAP = 1023;
constexpr int BL_MAX_ATTEMPTS = 64;
constexpr uint32_t BL_EPS_TAG = 0x4241u;         // c3 of the exploration draw: bandits_policy.hip's
constexpr uint32_t BL_GAMMA_TAG = 0x4C000000u;   // c3 of a sampler draw: tag | arm << 17 | which << 16 | attempt

struct BlLearner {
    const float *__restrict__ params;       // [n_learners][4]: a0, b0, c, 0
    const uint32_t *__restrict__ thr;       // [n_learners] or null (no exploration)
    const float *__restrict__ table;        // [n_learners][(cap + 1)(cap + 2) / 2] (MG_BANDITS_LEARNER_TABLE)
    const int32_t *__restrict__ ids;        // [n]
    int n_learners, cap, max_attempts;
};
struct BlOut {                              // [n] each
    double *ret_total, *ret_episode;
    int32_t *episode_len, *episodes;
    double *regret;
};
struct BlRec {                              // [T][n] each; each may be null
    int32_t *actions;
    float *reward;
    uint8_t *done;
    int32_t *info_steps;
    double *expected_gain, *best_gain;
    uint8_t *invalid;
};

__host__ __device__ constexpr int bl_counts_bytes(int arms) { return 2 * arms * BL_BLOCK * (int)sizeof(int32_t); }
__host__ __device__ constexpr int bl_lds_bytes(int arms) { return bl_counts_bytes(arms) + MTN * (int)sizeof(uint32_t); }
__host__ __device__ constexpr int64_t bl_cells(int cap) { return ((int64_t)cap + 1) * ((int64_t)cap + 2) / 2; }

// Thompson sampling for one env: K scores X / (X + Y) from 2 K gammas (Marsaglia-Tsang with a polar normal, a >= 1), and
// the lowest index among their maxima. ONE loop runs over the lane's own sequence of (arm, which, attempt): a lane that
// rejects tries again while its neighbours go on to their next draw, so a wave runs for its longest lane's total number of
// attempts and not for the sum over the draws of the longest lane's. Every draw's arithmetic is the definition's, so the
// bits do not depend on it. The loop's length differs between lanes: it holds no collective. `tries`: the attempts made
// per draw, max_attempts + 1 for the fallback.
__device__ __forceinline__ int bl_thompson(const int32_t *cnt, int K, float a0, float b0, int max_attempts, uint32_t e, uint64_t n,
                                           uint64_t seed, float *scores, int32_t *tries) {
    int g = 0, k = 0, i = 0;
    uint32_t which = 0;
    float best = 0.0f, X = 0.0f, d = 0.0f, c = 0.0f;
#pragma unroll 1
    while (k < K) {
        if (i == 0) {                                                      // a new draw: alpha for X, beta for Y
            const int pulls = cnt[2 * k * BL_BLOCK], wins = cnt[(2 * k + 1) * BL_BLOCK];
            const float a = which == 0 ? (float)wins + a0 : (float)(pulls - wins) + b0;
            d = a - 0.33333334f;
            c = 1.0f / sqrtf(9.0f * d);
        }
        uint32_t o[4];
        philox4x32_10(e, (uint32_t)n, (uint32_t)(n >> 32), BL_GAMMA_TAG | ((uint32_t)k << 17) | (which << 16) | (uint32_t)i,
                      (uint32_t)seed, (uint32_t)(seed >> 32), o);
        ++i;
        const float v1 = 2.0f * mg::u01(o[0]) - 1.0f;
        const float v2 = 2.0f * mg::u01(o[1]) - 1.0f;
        const float s = v1 * v1 + v2 * v2;
        bool accepted = false;
        float value = d;                                                   // the fallback
        if (s < 1.0f) {
            const float x = v1 * sqrtf((-2.0f * mg::log32(s)) / s);
            const float v = 1.0f + c * x;
            if (v > 0.0f) {
                const float v3 = (v * v) * v;
                accepted = mg::log32(mg::u01(o[2])) < (((0.5f * x) * x + d) - d * v3) + d * mg::log32(v3);
                if (accepted) value = d * v3;
            }
        }
        if (!accepted && i < max_attempts) continue;
        if (tries) tries[2 * k + (int)which] = accepted ? i : max_attempts + 1;
        i = 0;
        if (which == 0) {
            X = value;
            which = 1;
        } else {
            const float sc = X / (X + value);
            if (scores) scores[k] = sc;
            if (k == 0) best = sc;
            else if (sc > best) { g = k; best = sc; }
            which = 0;
            ++k;
        }
    }
    return g;
}

// The K scores of one env from its lane's column of the LDS counts (n = cnt[2 k * 64], w = cnt[(2 k + 1) * 64]) and the
// lowest index among their maxima. `scores` and `tries` (the probe's outputs; null in the rollout) are the env's rows.
template <int KIND>
__device__ __forceinline__ int bl_choose(const int32_t *cnt, int K, float a0, float b0, float c, const float *__restrict__ row,
                                         int cap, int max_attempts, uint32_t e, uint64_t step, uint64_t seed, float *scores,
                                         int32_t *tries) {
    if (KIND == MG_BANDITS_LEARNER_THOMPSON) return bl_thompson(cnt, K, a0, b0, max_attempts, e, step, seed, scores, tries);
    float lt = 0.0f;
    if (KIND == MG_BANDITS_LEARNER_UCB) {
        int64_t t = 0;
        int first = -1;
        for (int k = 0; k < K; ++k) {
            const int n = cnt[2 * k * BL_BLOCK];
            t += n;
            if (n == 0 && first < 0) first = k;
        }
        if (first >= 0) {                                                  // an unpulled arm first, the lowest
            if (scores)
                for (int k = 0; k < K; ++k) scores[k] = cnt[2 * k * BL_BLOCK] == 0 ? __uint_as_float(0x7f800000u) : 0.0f;
            return first;
        }
        lt = c * mg::log32((float)t);
    }
    int g = 0;
    float best = 0.0f;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const int n = cnt[2 * k * BL_BLOCK], w = cnt[(2 * k + 1) * BL_BLOCK];
        float sc;
        if (KIND == MG_BANDITS_LEARNER_GREEDY) {
            sc = ((float)w + a0) / (((float)n + a0) + b0);
        } else if (KIND == MG_BANDITS_LEARNER_UCB) {
            sc = (float)w / (float)n + sqrtf(lt / (float)n);
        } else {
            int64_t cell = n <= cap ? (int64_t)n * ((int64_t)n + 1) / 2 + w
                                    : (int64_t)cap * ((int64_t)cap + 1) / 2 + ((int64_t)w * cap) / n;
            const int64_t last = bl_cells(cap) - 1;                        // counts with w > n or n < 0: nothing is read outside
            cell = cell < 0 ? 0 : (cell > last ? last : cell);
            sc = row[cell];
        }
        if (scores) scores[k] = sc;
        if (k == 0) best = sc;
        else if (sc > best) { g = k; best = sc; }
    }
    return g;
}

// best = row[0]; for k >= 1: if row[k] > best
__device__ __forceinline__ double bl_best(const double *row, int arms) {
    double best = row[0];
    for (int i = 1; i < arms; ++i) {
        const double v = row[i];
        if (v > best) best = v;
    }
    return best;
}

// bandits_step_kernel's step body in its order (one double, then the reward; at the end of an episode with auto_reset the
// task draw, then the restart), with the action load replaced by the learner. Inside the step loop the kernel stores only
// what `rec` asks for; the env state, the counts and the five per-env results go out once, at the end.
template <int KIND>
__global__ __launch_bounds__(BL_BLOCK) void bandits_learner_rollout_kernel(BanditsK k, int n, int T, mg_bandits_state s,
                                                                           BlLearner la, mg_bandits_learner_carry ca,
                                                                           uint64_t seed, uint64_t step0, int episodic,
                                                                           BlOut po, BlRec rec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = k.K;
    const int lane = threadIdx.x, e0 = blockIdx.x * BL_BLOCK, e = e0 + lane;
    const bool live = e < n;
    const int el = live ? e : n - 1;   // spare lanes shadow the last env's learner; they step nothing and store nothing
    int32_t *cnt = reinterpret_cast<int32_t *>(smem) + lane;               // the lane's column

    int pid = la.ids[el];
    pid = pid < 0 ? 0 : (pid >= la.n_learners ? la.n_learners - 1 : pid);
    const float a0 = la.params[4 * pid], b0 = la.params[4 * pid + 1], c = la.params[4 * pid + 2];
    const float *__restrict__ trow = KIND == MG_BANDITS_LEARNER_TABLE ? la.table + (size_t)pid * (size_t)bl_cells(la.cap) : nullptr;
    const uint32_t thr = (KIND != MG_BANDITS_LEARNER_THOMPSON && la.thr != nullptr) ? la.thr[pid] : 0u;

    int steps = 0, over = 1, has_gauss = 0;
    double gauss = 0.0;
    Streams g{s.mt, reinterpret_cast<uint32_t *>(smem + bl_counts_bytes(K)), e0, lane, n, MTN};
    double *row = s.gains + (size_t)el * (size_t)K;
    double best = 0.0;
    if (live) {
        steps = s.steps[e];
        over = s.over[e];
        has_gauss = s.has_gauss[e];
        gauss = s.gauss[e];
        g.pos = (int)min(s.mt[(size_t)e * REC + MTN], (uint32_t)MTN);
        best = bl_best(row, K);
    }
    for (int j = 0; j < K; ++j) {
        cnt[2 * j * BL_BLOCK] = ca.pulls[(size_t)el * K + j];
        cnt[(2 * j + 1) * BL_BLOCK] = ca.wins[(size_t)el * K + j];
    }

    double ret_total = 0.0, ret_episode = 0.0, regret = 0.0;
    int episode_len = 0, episodes = 0;
    bool first_done = false;

    for (int t = 0; t < T; ++t) {
        const bool act = live && !over;                                    // an env that is over does nothing in this step
        int a = 0;
        if (act) {
            const uint64_t cs = step0 + (uint64_t)t;
            a = bl_choose<KIND>(cnt, K, a0, b0, c, trow, la.cap, la.max_attempts, (uint32_t)e, cs, seed, nullptr, nullptr);
            if (thr != 0u) {
                uint32_t o[4];
                philox4x32_10((uint32_t)e, (uint32_t)cs, (uint32_t)(cs >> 32), BL_EPS_TAG, (uint32_t)seed, (uint32_t)(seed >> 32), o);
                if (o[0] < thr) a = (int)(o[1] % (uint32_t)K);
            }
        }

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
            cnt[2 * a * BL_BLOCK] += 1;                                    // an exploratory pull counts too
            cnt[(2 * a + 1) * BL_BLOCK] += r == 1.0f;
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
                if (ended) best = bl_best(row, K);
            }
            if (ended) {
                steps = 0;
                over = 0;
                if (episodic)                                              // no counts are carried into a redrawn task
                    for (int j = 0; j < 2 * K; ++j) cnt[j * BL_BLOCK] = 0;
            }
        }
    }
    if (!live) return;
    s.steps[e] = steps;
    s.over[e] = (uint8_t)over;
    s.has_gauss[e] = has_gauss;
    s.gauss[e] = gauss;
    s.mt[(size_t)e * REC + MTN] = (uint32_t)g.pos;
    for (int j = 0; j < K; ++j) {
        ca.pulls[(size_t)e * K + j] = cnt[2 * j * BL_BLOCK];
        ca.wins[(size_t)e * K + j] = cnt[(2 * j + 1) * BL_BLOCK];
    }
    po.ret_total[e] = ret_total;
    po.ret_episode[e] = ret_episode;
    po.episode_len[e] = episode_len;
    po.episodes[e] = episodes;
    po.regret[e] = regret;
}

// The K scores the next step of every env would compute, by the rollout's own bl_choose on the same LDS layout; nothing
// else is written.
template <int KIND>
__global__ __launch_bounds__(BL_BLOCK) void bandits_learner_scores_kernel(int K, int n, BlLearner la, mg_bandits_learner_carry ca,
                                                                          uint64_t seed, uint64_t step0, float *scores,
                                                                          int32_t *tries) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x, e = blockIdx.x * BL_BLOCK + lane;
    if (e >= n) return;                                                    // no collective below
    int32_t *cnt = reinterpret_cast<int32_t *>(smem) + lane;
    int pid = la.ids[e];
    pid = pid < 0 ? 0 : (pid >= la.n_learners ? la.n_learners - 1 : pid);
    const float a0 = la.params[4 * pid], b0 = la.params[4 * pid + 1], c = la.params[4 * pid + 2];
    const float *__restrict__ trow = KIND == MG_BANDITS_LEARNER_TABLE ? la.table + (size_t)pid * (size_t)bl_cells(la.cap) : nullptr;
    for (int j = 0; j < K; ++j) {
        cnt[2 * j * BL_BLOCK] = ca.pulls[(size_t)e * K + j];
        cnt[(2 * j + 1) * BL_BLOCK] = ca.wins[(size_t)e * K + j];
    }
    bl_choose<KIND>(cnt, K, a0, b0, c, trow, la.cap, la.max_attempts, (uint32_t)e, step0, seed, scores + (size_t)e * K,
                    (KIND == MG_BANDITS_LEARNER_THOMPSON && tries != nullptr) ? tries + (size_t)e * 2 * K : nullptr);
}

int check_learner(const mg_bandits_learner *l, const char *fn) {
    if (l->kind < MG_BANDITS_LEARNER_GREEDY || l->kind > MG_BANDITS_LEARNER_THOMPSON)
        return mg::set_error(MG_ERR_BAD_CONFIG, "%s: kind = %d (need 0..3)", fn, l->kind);
    if (l->params == nullptr) return mg::set_error(MG_ERR_NULL_POINTER, "%s: mg_bandits_learner needs params (NULL)", fn);
    if (l->n_learners < 1) return mg::set_error(MG_ERR_BAD_SIZE, "%s: n_learners=%d", fn, l->n_learners);
    if (l->arms < 2 || l->arms > BL_MAX_ARMS)
        return mg::set_error(MG_ERR_BAD_SIZE, "%s: arms=%d is outside [2, %d]", fn, l->arms, BL_MAX_ARMS);
    if (l->kind == MG_BANDITS_LEARNER_TABLE) {
        if (l->table == nullptr) return mg::set_error(MG_ERR_NULL_POINTER, "%s: a table learner needs table (NULL)", fn);
        if (l->table_cap < 1 || l->table_cap > BL_MAX_CAP)
            return mg::set_error(MG_ERR_BAD_SIZE, "%s: table_cap=%d is outside [1, %d]", fn, l->table_cap, BL_MAX_CAP);
    }
    if (l->kind == MG_BANDITS_LEARNER_THOMPSON) {
        if (l->max_attempts < 1 || l->max_attempts > BL_MAX_ATTEMPTS)
            return mg::set_error(MG_ERR_BAD_SIZE, "%s: max_attempts=%d is outside [1, %d]", fn, l->max_attempts, BL_MAX_ATTEMPTS);
        if (l->eps_threshold != nullptr)
            return mg::set_error(MG_ERR_BAD_CONFIG, "%s: Thompson sampling takes no eps_threshold", fn);
    }
    return MG_OK;
}

}  // namespace

extern "C" int mg_bandits_learner_rollout(const mg_bandits_config *cfg, int32_t n_envs, const mg_bandits_state *state,
                                          int32_t n_steps, const mg_bandits_learner *learner, const int32_t *learner_ids,
                                          const mg_bandits_learner_carry *carry, uint64_t seed, uint64_t step0, int32_t episodic,
                                          double *ret_total, double *ret_episode, int32_t *episode_len, int32_t *episodes,
                                          double *regret, int32_t *actions, float *reward, uint8_t *done, int32_t *info_steps,
                                          double *expected_gain, double *best_gain, uint8_t *invalid, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_STATE(state);
    MG_REQUIRE_PTR(learner);
    MG_REQUIRE_PTR(learner_ids);
    MG_REQUIRE_PTR(carry);
    MG_REQUIRE_PTR(ret_total);
    MG_REQUIRE_PTR(ret_episode);
    MG_REQUIRE_PTR(episode_len);
    MG_REQUIRE_PTR(episodes);
    MG_REQUIRE_PTR(regret);
    if (!carry->pulls || !carry->wins) return mg::set_error(MG_ERR_NULL_POINTER, "mg_bandits_learner_carry has a NULL array");
    int rc = check_config(cfg, "mg_bandits_learner_rollout");
    if (rc != MG_OK) return rc;
    if (n_envs <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "mg_bandits_learner_rollout: n_envs = %d", n_envs);
    if (n_steps < 1) return mg::set_error(MG_ERR_BAD_SIZE, "mg_bandits_learner_rollout: n_steps = %d (at least 1)", n_steps);
    rc = check_learner(learner, "mg_bandits_learner_rollout");
    if (rc != MG_OK) return rc;
    if (learner->arms != cfg->arms)
        return mg::set_error(MG_ERR_BAD_CONFIG, "the learner was built for arms=%d, the env has %d", learner->arms, cfg->arms);
    mg::DeviceGuard guard(mg::device_of(state->mt));
    BlLearner la{learner->params, learner->eps_threshold, learner->table, learner_ids, learner->n_learners, learner->table_cap,
                 learner->max_attempts};
    BlOut po{ret_total, ret_episode, episode_len, episodes, regret};
    BlRec rec{actions, reward, done, info_steps, expected_gain, best_gain, invalid};
    const dim3 grid((unsigned)(((int64_t)n_envs + BL_BLOCK - 1) / BL_BLOCK)), block(BL_BLOCK);
    const size_t lds = (size_t)bl_lds_bytes(learner->arms);                // at most 35 264 B: no attribute call
    hipStream_t st = static_cast<hipStream_t>(stream);
#define BL_LAUNCH(KIND)                                                                                                        \
    hipLaunchKernelGGL(bandits_learner_rollout_kernel<KIND>, grid, block, lds, st, fold(cfg), n_envs, n_steps, *state, la, *carry, \
                       seed, step0, episodic, po, rec)
    switch (learner->kind) {
        case MG_BANDITS_LEARNER_GREEDY: BL_LAUNCH(MG_BANDITS_LEARNER_GREEDY); break;
        case MG_BANDITS_LEARNER_UCB: BL_LAUNCH(MG_BANDITS_LEARNER_UCB); break;
        case MG_BANDITS_LEARNER_TABLE: BL_LAUNCH(MG_BANDITS_LEARNER_TABLE); break;
        default: BL_LAUNCH(MG_BANDITS_LEARNER_THOMPSON); break;
    }
#undef BL_LAUNCH
    return mg::check_launch("bandits_learner_rollout_kernel");
}

extern "C" int mg_bandits_learner_scores(int32_t n_envs, const mg_bandits_learner *learner, const int32_t *learner_ids,
                                         const mg_bandits_learner_carry *carry, uint64_t seed, uint64_t step0, float *scores,
                                         int32_t *attempts, void *stream) {
    MG_REQUIRE_PTR(learner);
    MG_REQUIRE_PTR(learner_ids);
    MG_REQUIRE_PTR(carry);
    MG_REQUIRE_PTR(scores);
    if (!carry->pulls || !carry->wins) return mg::set_error(MG_ERR_NULL_POINTER, "mg_bandits_learner_carry has a NULL array");
    if (n_envs <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "mg_bandits_learner_scores: n_envs = %d", n_envs);
    int rc = check_learner(learner, "mg_bandits_learner_scores");
    if (rc != MG_OK) return rc;
    mg::DeviceGuard guard(mg::device_of(scores));
    BlLearner la{learner->params, learner->eps_threshold, learner->table, learner_ids, learner->n_learners, learner->table_cap,
                 learner->max_attempts};
    const dim3 grid((unsigned)(((int64_t)n_envs + BL_BLOCK - 1) / BL_BLOCK)), block(BL_BLOCK);
    const size_t lds = (size_t)bl_counts_bytes(learner->arms);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define BL_LAUNCH(KIND)                                                                                                        \
    hipLaunchKernelGGL(bandits_learner_scores_kernel<KIND>, grid, block, lds, st, learner->arms, n_envs, la, *carry, seed, step0, \
                       scores, attempts)
    switch (learner->kind) {
        case MG_BANDITS_LEARNER_GREEDY: BL_LAUNCH(MG_BANDITS_LEARNER_GREEDY); break;
        case MG_BANDITS_LEARNER_UCB: BL_LAUNCH(MG_BANDITS_LEARNER_UCB); break;
        case MG_BANDITS_LEARNER_TABLE: BL_LAUNCH(MG_BANDITS_LEARNER_TABLE); break;
        default: BL_LAUNCH(MG_BANDITS_LEARNER_THOMPSON); break;
    }
#undef BL_LAUNCH
    return mg::check_launch("bandits_learner_scores_kernel");
}
