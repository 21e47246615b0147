// walker_policy.hip — MetaLocomotion closed-loop rollouts: per-env MLP policies inside the launch (mg_walker_policy_*).
//
// A translation unit of its own, like quadrotor_policy.hip and for the same reason: it takes the wave kernel, its layout and
// wave_plan from walker_core.h, and wave_plan<WAVE_POLICY> instantiates the third form of walker_step_wave_kernel for every
// shape it can pick, and no other form. walker.hip compiles the step and the rollout forms from the same header, and the files
// build in parallel. Same flags (metagym_amd/build.py) and the same contraction pragmas: the header lets the compiler fuse
// a*b+c in the physics, which is one shared text, so the policy form's physics is the step's bit for bit; wave_policy_action
// is compiled with contraction off, which is what makes the policy definition of include/metagym_hip.h hold (one rounding
// per operation).
#include "walker_core.h"

namespace {

constexpr int WAVE_POLICY_MAX_HIDDEN = 256;     // h[hidden] sits in LDS behind x: at most four hidden units per lane

// floats of one packed policy (the layout of include/metagym_hip.h): H > 0: b1[H], w1 [D][H], b2[A], w2 [H][A]; H = 0: b[A], w [D][A]
int policy_count(int hidden, int obs_dim, int n_act) {
    return hidden > 0 ? hidden + obs_dim * hidden + n_act + hidden * n_act : n_act + obs_dim * n_act;
}

}  // namespace

extern "C" int32_t mg_walker_policy_param_count(int32_t hidden, int32_t obs_dim, int32_t n_act) {
    if (int rc = check_walker_policy_sizes(hidden, 0, WAVE_POLICY_MAX_HIDDEN, obs_dim, n_act)) return rc;
    return policy_count(hidden, obs_dim, n_act);
}

extern "C" int mg_walker_policy_rollout(const mg_walker_topology *tp, const mg_walker_models *ms, const mg_walker_params *prm,
                                        int32_t n, const mg_walker_state *st, int32_t n_steps, int32_t obs_every,
                                        const mg_walker_policy *policy, const float *obs0, float *obs, double *ret_total,
                                        double *ret_episode, int32_t *episode_len, float *actions, float *reward, float *rewards5,
                                        uint8_t *done, void *stream) {
    if (int rc = check_walker(tp, ms, prm, st, n)) return rc;
    if (int rc = check_walker_rollout("mg_walker_policy_rollout", prm, n_steps, obs_every,
                                      "the policy's output is a torque action, actuation = 0"))
        return rc;
    MG_REQUIRE_PTR(policy);
    if (policy->params_d == nullptr || policy->policy_id_d == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_walker_policy has a NULL params_d or policy_id_d");
    MG_REQUIRE_PTR(obs0);
    MG_REQUIRE_PTR(obs);
    MG_REQUIRE_PTR(ret_total);
    MG_REQUIRE_PTR(ret_episode);
    MG_REQUIRE_PTR(episode_len);
    if (policy->n_policies < 1) return mg::set_error(MG_ERR_BAD_SIZE, "mg_walker_policy: n_policies=%d", policy->n_policies);
    if (policy->hidden < 0 || policy->hidden > WAVE_POLICY_MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "mg_walker_policy: hidden=%d is outside [0, %d]", policy->hidden, WAVE_POLICY_MAX_HIDDEN);
    const int obs_dim = 8 + 2 * tp->n_joints + tp->n_feet;
    if (policy->obs_dim != obs_dim)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_walker_policy: obs_dim=%d, the topology's observation has %d entries",
                             policy->obs_dim, obs_dim);
    if (policy->n_act != tp->n_joints || tp->n_joints < 1)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_walker_policy: n_act=%d, the topology has %d joints", policy->n_act, tp->n_joints);
    WaveLaunch<WAVE_POLICY> w;
    if (int rc = wave_plan(tp, prm, st, &w, policy->hidden)) return rc;
    mg::DeviceGuard guard(mg::device_of(st->pos));
    const WavePlanArgs a = pack(w.plan);
    const WaveRoll<WAVE_POLICY> roll{n_steps, obs_every, policy->params_d, policy->policy_id_d, policy->n_policies, policy->hidden,
                                     policy_count(policy->hidden, obs_dim, tp->n_joints), obs0, actions, ret_total, ret_episode,
                                     episode_len};
    hipLaunchKernelGGL(w.kernel, dim3(n), dim3(WV), w.lds, (hipStream_t)stream, *tp, *ms, *prm, *st, n, a.rows, a.scan,
                       (const float *)nullptr, obs, reward, rewards5, done, roll);
    return mg::check_launch("walker_step_wave_kernel (policy rollout)");
}
