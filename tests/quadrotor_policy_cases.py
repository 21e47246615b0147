"""What tests/test_quadrotor_policy.py (CPU: the oracle and the policy definition alone) and
tests/test_quadrotor_policy_gpu.py (the closed-loop launch) share: the test policies, the policy-id layouts, the priming
step that gives a loaded state its observation, and the closed loop on the CPU oracle."""
import numpy as np

import quadrotor_tasks_cases as qc

N, T = qc.N, qc.T              # 130 envs (two full waves and a 2-lane tail), 12 steps
P = 3
# A state written with load_state_dict has no observation yet. One step with this action, on the env and on the oracle
# alike, produces the row the closed loop starts from.
PRIME_ACTION = np.full((N, 4), 7.0, np.float32)


def make_policy(hidden, obs_dim=16, n_policies=P, seed=100):
    """P random policies. Voltages land inside and outside [0.1, 15], so the step's clamp runs on both sides."""
    from metagym_amd.quadrotor import QuadrotorPolicy
    rs = np.random.RandomState(seed + 17 * hidden + obs_dim)
    f = np.float32
    b2 = rs.uniform(3.0, 11.0, (n_policies, 4)).astype(f)
    if hidden == 0:
        return QuadrotorPolicy.linear(rs.uniform(-0.3, 0.3, (n_policies, 4, obs_dim)).astype(f), b2)
    return QuadrotorPolicy(rs.uniform(-0.5, 0.5, (n_policies, hidden, obs_dim)).astype(f),
                           rs.uniform(-1.0, 1.0, (n_policies, hidden)).astype(f),
                           rs.uniform(-2.0, 2.0, (n_policies, 4, hidden)).astype(f), b2)


def layout_ids(n=N):
    """One id over lanes 0..63 (the wave stages its policy in LDS), e % 3 over 64..127 (each lane reads its own), the
    2-lane tail on one id (a partial wave): one launch takes all three routes."""
    ids = np.arange(n) % P
    ids[:64] = 1
    ids[128:] = 2
    return ids


def closed_loop_oracle(og, policy, ids, steps, prime=PRIME_ACTION):
    """The closed loop on the CPU oracle: prime, then `steps` times (QuadrotorPolicy.reference, OracleGroups.step).
    Returns the actions [steps, N, 4], the per-step outputs and the first failure code of every env (priming included)."""
    obs, _, _, failed = og.step(prime)
    codes = failed.copy()
    acts, outs = [], []
    for _ in range(steps):
        a = policy.reference(obs, ids)
        out = og.step(a)
        obs = out[0]
        codes = np.where(codes == 0, out[3], codes)
        acts.append(a)
        outs.append(out)
    return np.stack(acts), outs, codes
