// bandits.hip — K-armed Bernoulli bandits (reference metagym/bandits/bandits_env.py) for N envs at once, bit for bit.
//
// Env e owns one numpy legacy stream (numpy.random.seed(s_e)): 624 key words and pos in the record mt[e][625], the gauss
// cache beside it. Every draw of the reference's env comes from that stream, in the reference's order:
//   step        one legacy double d; reward = d < gains[a]
//   Classical   idx = bounded(K-2) (randint(0, K-1): arm K-1 is never chosen; K = 2 draws nothing); the gains are the
//               host-computed clipped lo everywhere and hi at idx
//   Uniform     K doubles d_k; gain_k = clip((d_k - 0.5) * 3.464 + mean)
//   Gaussian    K legacy gauss values (polar method, the second value of a pair cached); gain_k = clip(mean + dev * g_k)
// The one libm call is Gaussian's log (OCML here, glibc in numpy): the rejection test r2 < 1 uses basic operations only
// (-ffp-contract=off), so every draw count is exact and only the gain values may differ, by an ulp or two.
//
// Mapping: one lane per env, one wave per workgroup. steps, the episode flag, pos and the gauss cache live in registers
// for the whole launch; the key words are read from HBM where they lie (two words per step, each cache line serves 16
// steps). A refill is a wave job: the lanes whose pos reached 624 are balloted and served one after another, each block
// loaded into LDS, regenerated there by the shared three-segment refill (mg_mt19937.h) and stored back, coalesced. Task
// draws are lane-serial: when episodes end together (the usual case: every env has the same max_steps) all 64 lanes
// resample at once and the lane-serial draw keeps them all busy.
//
// This file: the four kernels it launches and the C entry points. Streams, sample_task and the host checks, which
// bandits_policy.hip and bandits_learner.hip share, are in bandits_core.h.
#include "bandits_core.h"

namespace {

__global__ __launch_bounds__(64) void bandits_seed_kernel(int n, uint32_t seed_base, const uint32_t *seeds,
                                                          mg_bandits_state s) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    uint32_t *k = s.mt + (size_t)e * REC;
    uint32_t p = seeds != nullptr ? seeds[e] : seed_base + (uint32_t)e;
    k[0] = p;
    for (int i = 1; i < MTN; ++i) {
        p = mt::seed_step(p, i);
        k[i] = p;
    }
    k[MTN] = MTN;
    s.has_gauss[e] = 0;
    s.gauss[e] = 0.0;
}

__global__ __launch_bounds__(64) void bandits_sample_kernel(BanditsK k, int n, mg_bandits_state s, const uint8_t *mask,
                                                            double *out) {
    __shared__ uint32_t lds[MTN];
    const int lane = threadIdx.x, e0 = blockIdx.x * 64, e = e0 + lane;
    const bool act = e < n && (mask == nullptr || mask[e] != 0);
    Streams g{s.mt, lds, e0, lane, n, act ? (int)min(s.mt[(size_t)e * REC + MTN], (uint32_t)MTN) : MTN};
    int has_gauss = act ? s.has_gauss[e] : 0;
    double gauss = act ? s.gauss[e] : 0.0;
    sample_task(k, g, act, has_gauss, gauss, out + (size_t)e * (size_t)k.K);
    if (act) {
        s.mt[(size_t)e * REC + MTN] = (uint32_t)g.pos;
        s.has_gauss[e] = has_gauss;
        s.gauss[e] = gauss;
    }
}

__global__ __launch_bounds__(64) void bandits_reset_kernel(int n, mg_bandits_state s, const uint8_t *mask) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n || (mask != nullptr && mask[e] == 0)) return;
    s.steps[e] = 0;
    s.over[e] = 0;
}

__global__ __launch_bounds__(64) void bandits_step_kernel(BanditsK k, int n, int T, mg_bandits_state s,
                                                          const int32_t *actions, float *reward, uint8_t *done,
                                                          int32_t *info_steps, double *expected_gain, uint8_t *invalid) {
    __shared__ uint32_t lds[MTN];
    const int lane = threadIdx.x, e0 = blockIdx.x * 64, e = e0 + lane;
    const bool live = e < n;
    const size_t K = (size_t)k.K;
    int steps = 0, over = 1, has_gauss = 0;
    double gauss = 0.0;
    Streams g{s.mt, lds, e0, lane, n, MTN};
    if (live) {
        steps = s.steps[e];
        over = s.over[e];
        has_gauss = s.has_gauss[e];
        gauss = s.gauss[e];
        g.pos = (int)min(s.mt[(size_t)e * REC + MTN], (uint32_t)MTN);
    }
    double *row = s.gains + (size_t)e * K;
    for (int t = 0; t < T; ++t) {
        const size_t o = (size_t)t * (size_t)n + (size_t)e;
        const int a = live ? actions[o] : 0;
        const int bad = over ? 2 : (a < -k.K || a >= k.K) ? 1 : 0;
        const bool act = live && bad == 0;
        const double d = g.next_double(act);
        bool ended = false;
        if (act) {
            const double gain = row[a < 0 ? a + k.K : a];
            const int before = steps++;
            ended = steps >= k.max_steps;
            reward[o] = d < gain ? 1.0f : 0.0f;
            done[o] = ended;
            info_steps[o] = before;
            expected_gain[o] = gain;
            invalid[o] = 0;
            if (ended) over = 1;
        } else if (live) {
            reward[o] = 0.0f;
            done[o] = 0;
            info_steps[o] = steps;
            expected_gain[o] = 0.0;
            invalid[o] = (uint8_t)bad;
        }
        if (k.auto_reset) {
            if (k.dist != MG_BANDITS_NONE && __ballot(ended)) sample_task(k, g, ended, has_gauss, gauss, row);
            if (ended) { steps = 0; over = 0; }
        }
    }
    if (live) {
        s.steps[e] = steps;
        s.over[e] = (uint8_t)over;
        s.has_gauss[e] = has_gauss;
        s.gauss[e] = gauss;
        s.mt[(size_t)e * REC + MTN] = (uint32_t)g.pos;
    }
}

}  // namespace

extern "C" int mg_bandits_seed(int32_t n_envs, uint32_t seed_base, const uint32_t *seeds, const mg_bandits_state *state,
                               void *stream) {
    MG_REQUIRE_PTR(state);
    MG_REQUIRE_PTR(state->mt); MG_REQUIRE_PTR(state->has_gauss); MG_REQUIRE_PTR(state->gauss);
    if (n_envs <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "mg_bandits_seed: n_envs = %d", n_envs);
    mg::DeviceGuard guard(mg::device_of(state->mt));
    hipLaunchKernelGGL(bandits_seed_kernel, dim3((unsigned)(((int64_t)n_envs + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), n_envs,
                       seed_base, seeds, *state);
    return mg::check_launch("bandits_seed_kernel");
}

extern "C" int mg_bandits_sample_task(const mg_bandits_config *cfg, int32_t n_envs, const mg_bandits_state *state,
                                      const uint8_t *mask, double *gains_out, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_STATE(state);
    MG_REQUIRE_PTR(gains_out);
    int rc = check_config(cfg, "mg_bandits_sample_task");
    if (rc != MG_OK) return rc;
    if (cfg->distribution == MG_BANDITS_NONE)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_bandits_sample_task: distribution = MG_BANDITS_NONE");
    if (n_envs <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "mg_bandits_sample_task: n_envs = %d", n_envs);
    mg::DeviceGuard guard(mg::device_of(state->mt));
    hipLaunchKernelGGL(bandits_sample_kernel, dim3((unsigned)(((int64_t)n_envs + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream),
                       fold(cfg), n_envs, *state, mask, gains_out);
    return mg::check_launch("bandits_sample_kernel");
}

extern "C" int mg_bandits_reset(const mg_bandits_config *cfg, int32_t n_envs, const mg_bandits_state *state,
                                const uint8_t *mask, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_STATE(state);
    int rc = check_config(cfg, "mg_bandits_reset");
    if (rc != MG_OK) return rc;
    if (n_envs <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "mg_bandits_reset: n_envs = %d", n_envs);
    mg::DeviceGuard guard(mg::device_of(state->steps));
    hipLaunchKernelGGL(bandits_reset_kernel, dim3((unsigned)(((int64_t)n_envs + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), n_envs,
                       *state, mask);
    return mg::check_launch("bandits_reset_kernel");
}

extern "C" int mg_bandits_step(const mg_bandits_config *cfg, int32_t n_envs, const mg_bandits_state *state, int32_t n_steps,
                               const int32_t *actions, float *reward, uint8_t *done, int32_t *info_steps,
                               double *expected_gain, uint8_t *invalid, void *stream) {
    MG_REQUIRE_PTR(cfg);
    MG_REQUIRE_STATE(state);
    MG_REQUIRE_PTR(actions); MG_REQUIRE_PTR(reward); MG_REQUIRE_PTR(done); MG_REQUIRE_PTR(info_steps);
    MG_REQUIRE_PTR(expected_gain); MG_REQUIRE_PTR(invalid);
    int rc = check_config(cfg, "mg_bandits_step");
    if (rc != MG_OK) return rc;
    if (n_envs <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "mg_bandits_step: n_envs = %d", n_envs);
    if (n_steps <= 0) return mg::set_error(MG_ERR_BAD_SIZE, "mg_bandits_step: n_steps = %d", n_steps);
    mg::DeviceGuard guard(mg::device_of(state->mt));
    hipLaunchKernelGGL(bandits_step_kernel, dim3((unsigned)(((int64_t)n_envs + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream),
                       fold(cfg), n_envs, n_steps, *state, actions, reward, done, info_steps, expected_gain, invalid);
    return mg::check_launch("bandits_step_kernel");
}
