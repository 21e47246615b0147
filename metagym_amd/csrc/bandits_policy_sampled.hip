// bandits_policy_sampled.hip — Bandits closed-loop rollouts with a softmax-sampled policy (mg_bandits_policy_rollout_sampled):
// bandits_policy.hip's kernel with SAMPLED = true, the action of every step a Gumbel-max draw from softmax(l / temperature)
// (mg_sample.h). A translation unit of its own so that each policy unit emits the one instantiation it launches; everything
// but the entry point is bandits_policy_core.h. Same flags (metagym_amd/build.py): -ffp-contract=off.
#include "bandits_core.h"

#include "bandits_policy_core.h"

extern "C" int mg_bandits_policy_rollout_sampled(const mg_bandits_config *cfg, int32_t n_envs, const mg_bandits_state *state,
                                                 int32_t n_steps, const mg_bandits_policy *policy, const int32_t *policy_ids,
                                                 const mg_bandits_policy_carry *carry, const float *inv_temperature,
                                                 uint64_t seed, uint64_t step0, int32_t episodic, double *ret_total,
                                                 double *ret_episode, int32_t *episode_len, int32_t *episodes, double *regret,
                                                 int32_t *actions, float *reward, uint8_t *done, int32_t *info_steps,
                                                 double *expected_gain, double *best_gain, uint8_t *invalid, void *stream) {
    return bandits_policy_rollout<true>("mg_bandits_policy_rollout_sampled", cfg, n_envs, state, n_steps, policy, policy_ids,
                                        carry, inv_temperature, seed, step0, episodic, ret_total, ret_episode, episode_len,
                                        episodes, regret, actions, reward, done, info_steps, expected_gain, best_gain, invalid,
                                        stream);
}
