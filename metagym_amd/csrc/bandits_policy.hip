// bandits_policy.hip — Bandits closed-loop rollouts: per-env recurrent policies inside the launch (mg_bandits_policy_*).
//
// A translation unit of its own on bandits_core.h (Streams, sample_task, clip01, BanditsK, the host checks). Same flags
// (metagym_amd/build.py): -ffp-contract=off, which is what makes the policy definition of include/metagym_hip.h hold (one
// rounding per operation). The kernel keeps its own staging and exploration draw; only the host side
// takes the LDS limit and the opt-in from mg_closed_loop.h. The kernel, bp_eval and the host checks are in
// bandits_policy_core.h, a template on SAMPLED: this unit launches and emits the greedy instantiation,
// bandits_policy_sampled.hip the softmax-sampled one.
//
// Mapping: bandits_step_kernel's — one lane per env, one wave per workgroup; steps, over, the stream position, the gauss
// cache, the carry scalars, the best gain of the row in force and the five results live in registers for n_steps steps.
// The recurrent state h and its successor live in LDS lane-minor (buf[j * 64 + lane]: H is a run-time value, and the 64
// lanes of a ds_read_b32 fall on 64 consecutive dwords). The K logits are never stored: logit k is complete before logit
// k + 1 is begun, so the running argmax holds one logit and one index in registers. Weights: a wave whose lanes all hold one
// policy id stages that policy in LDS once and reads it with same-address (broadcast) 16-byte reads; a wave with mixed ids
// reads per lane from global memory. Both inline bp_eval, so the bits are equal.
//
// The refill inside Streams::next is a workgroup-collective (__syncthreads). The env half of a step is therefore reached
// by all 64 lanes at every step, with act = false for the lanes that draw nothing: the spare lanes, the envs that are over,
// and at the task draw the envs whose episode did not end.
#include "bandits_core.h"

#include "bandits_policy_core.h"

extern "C" int32_t mg_bandits_policy_param_count(int32_t hidden, int32_t arms) {
    if (hidden < 1 || hidden > BP_MAX_HIDDEN) return mg::set_error(MG_ERR_BAD_SIZE, "hidden=%d is outside [1, %d]", hidden, BP_MAX_HIDDEN);
    if (arms < 2 || arms > BP_MAX_ARMS) return mg::set_error(MG_ERR_BAD_SIZE, "arms=%d is outside [2, %d]", arms, BP_MAX_ARMS);
    return bp_count(hidden, arms);
}

extern "C" int mg_bandits_policy_rollout(const mg_bandits_config *cfg, int32_t n_envs, const mg_bandits_state *state,
                                         int32_t n_steps, const mg_bandits_policy *policy, const int32_t *policy_ids,
                                         const mg_bandits_policy_carry *carry, uint64_t seed, uint64_t step0, int32_t episodic,
                                         double *ret_total, double *ret_episode, int32_t *episode_len, int32_t *episodes,
                                         double *regret, int32_t *actions, float *reward, uint8_t *done, int32_t *info_steps,
                                         double *expected_gain, double *best_gain, uint8_t *invalid, void *stream) {
    return bandits_policy_rollout<false>("mg_bandits_policy_rollout", cfg, n_envs, state, n_steps, policy, policy_ids, carry,
                                         nullptr, seed, step0, episodic, ret_total, ret_episode, episode_len, episodes, regret,
                                         actions, reward, done, info_steps, expected_gain, best_gain, invalid, stream);
}
