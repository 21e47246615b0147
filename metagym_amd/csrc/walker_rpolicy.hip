// walker_rpolicy.hip — MetaLocomotion closed-loop rollouts with recurrent policies and a carry (mg_walker_rpolicy_*).
//
// A translation unit of its own, like walker_policy.hip and for the same reason: it takes the wave kernel, its layout and
// wave_plan from walker_core.h, and wave_plan<WAVE_RPOLICY> instantiates walker_step_wave_kernel<NMAX, SH, WAVE_RPOLICY> for
// every shape it can pick, and no other form. walker.hip and walker_policy.hip compile their forms from the same header, and
// the three files build in parallel. Same flags (metagym_amd/build.py) and the same contraction pragmas: the physics is the
// one shared text, fused as in the step; wave_rpolicy_action is compiled with contraction off, which is what makes the
// definition of include/metagym_hip.h hold (one rounding per operation).
#include "walker_core.h"

namespace {

constexpr int WAVE_RPOLICY_MAX_HIDDEN = 256;    // h and hn sit in LDS behind x: at most four hidden units per lane

// floats of one packed policy (the layout of include/metagym_hip.h): b[H], wx [D][H], wa [A][H], wr[H], wd[H], wh [H][H], bo[A],
// wo [H][A]; no padding
int rpolicy_count(int hidden, int obs_dim, int n_act) {
    return hidden + (obs_dim + n_act + 2 + hidden) * hidden + n_act + hidden * n_act;
}

}  // namespace

extern "C" int32_t mg_walker_rpolicy_param_count(int32_t hidden, int32_t obs_dim, int32_t n_act) {
    if (int rc = check_walker_policy_sizes(hidden, 1, WAVE_RPOLICY_MAX_HIDDEN, obs_dim, n_act)) return rc;
    return rpolicy_count(hidden, obs_dim, n_act);
}

extern "C" int mg_walker_rpolicy_rollout(const mg_walker_topology *tp, const mg_walker_models *ms, const mg_walker_params *prm,
                                         int32_t n, const mg_walker_state *st, int32_t n_steps, int32_t obs_every,
                                         const mg_walker_policy *policy, const mg_walker_rpolicy_carry *carry, int32_t episodic,
                                         const float *obs0, float *obs, double *ret_total, double *ret_episode,
                                         int32_t *episode_len, float *actions, float *reward, float *rewards5, uint8_t *done,
                                         void *stream) {
    if (int rc = check_walker(tp, ms, prm, st, n)) return rc;
    if (int rc = check_walker_rollout("mg_walker_rpolicy_rollout", prm, n_steps, obs_every,
                                      "the policy's output is a torque action, actuation = 0"))
        return rc;
    MG_REQUIRE_PTR(policy);
    if (policy->params_d == nullptr || policy->policy_id_d == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_walker_policy has a NULL params_d or policy_id_d");
    MG_REQUIRE_PTR(carry);
    if (carry->h == nullptr || carry->prev_action == nullptr || carry->prev_reward == nullptr || carry->prev_done == nullptr)
        return mg::set_error(MG_ERR_NULL_POINTER, "mg_walker_rpolicy_carry has a NULL h, prev_action, prev_reward or prev_done");
    MG_REQUIRE_PTR(obs0);
    MG_REQUIRE_PTR(obs);
    MG_REQUIRE_PTR(ret_total);
    MG_REQUIRE_PTR(ret_episode);
    MG_REQUIRE_PTR(episode_len);
    if (policy->n_policies < 1) return mg::set_error(MG_ERR_BAD_SIZE, "mg_walker_policy: n_policies=%d", policy->n_policies);
    if (policy->hidden < 1 || policy->hidden > WAVE_RPOLICY_MAX_HIDDEN)
        return mg::set_error(MG_ERR_BAD_SIZE, "mg_walker_policy: hidden=%d is outside [1, %d] (the recurrent form)", policy->hidden,
                             WAVE_RPOLICY_MAX_HIDDEN);
    if (episodic && !prm->auto_reset)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_walker_rpolicy_rollout: episodic clears the carry at a fused reset; it needs "
                             "auto_reset");
    const int obs_dim = 8 + 2 * tp->n_joints + tp->n_feet;
    if (policy->obs_dim != obs_dim)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_walker_policy: obs_dim=%d, the topology's observation has %d entries",
                             policy->obs_dim, obs_dim);
    if (policy->n_act != tp->n_joints || tp->n_joints < 1)
        return mg::set_error(MG_ERR_BAD_CONFIG, "mg_walker_policy: n_act=%d, the topology has %d joints", policy->n_act, tp->n_joints);
    WaveLaunch<WAVE_RPOLICY> w;
    if (int rc = wave_plan(tp, prm, st, &w, policy->hidden)) return rc;
    mg::DeviceGuard guard(mg::device_of(st->pos));
    const WavePlanArgs a = pack(w.plan);
    const WaveRoll<WAVE_RPOLICY> roll{n_steps, obs_every, policy->params_d, policy->policy_id_d, policy->n_policies, policy->hidden,
                                      rpolicy_count(policy->hidden, obs_dim, tp->n_joints), obs0, actions, ret_total, ret_episode,
                                      episode_len, carry->h, carry->prev_action, carry->prev_reward, carry->prev_done,
                                      episodic != 0 ? 1 : 0};
    hipLaunchKernelGGL(w.kernel, dim3(n), dim3(WV), w.lds, (hipStream_t)stream, *tp, *ms, *prm, *st, n, a.rows, a.scan,
                       (const float *)nullptr, obs, reward, rewards5, done, roll);
    return mg::check_launch("walker_step_wave_kernel (recurrent policy rollout)");
}
