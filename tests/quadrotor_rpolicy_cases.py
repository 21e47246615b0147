"""What tests/test_quadrotor_rpolicy.py (CPU: the recurrent policy definition and the oracle alone) and
tests/test_quadrotor_rpolicy_gpu.py (the closed-loop launch with a carry) share: the test policies, the scalar
restatement of the definition, and the recurrent closed loop on the CPU oracle. Shapes, ids and the priming step are
those of quadrotor_policy_cases."""
import numpy as np

import quadrotor_policy_cases as pc

N, T, P = pc.N, pc.T, pc.P
HIDDEN = (1, 5, 64)            # the smallest, one that is no multiple of four (the padding skip), the largest LDS footprint
F = np.float32
# Input gain of hidden unit j of policy p: GAINS[(p + j) % 3]. Observations, voltages and rewards are of order 1 to 10, so a
# unit with gain 1 sits at +1 or -1 almost always and one with gain 0.002 never leaves (-1, 1); 0.05 does both. Every H,
# H = 1 included, therefore holds saturated and unsaturated units across the three policies
# (test_quadrotor_rpolicy.py::test_units_saturate_and_do_not_in_the_closed_loop checks it on the CPU oracle).
GAINS = (1.0, 0.002, 0.05)


def make_rpolicy(hidden, obs_dim=16, n_policies=P, seed=200):
    """P random recurrent policies. Voltages land inside and outside [0.1, 15], so the step's clamp runs on both sides:
    one output bias lies far above the range and one far below, whatever a single unit adds (|wo * h| <= 8 at H = 1)."""
    from metagym_amd.quadrotor import QuadrotorRecurrentPolicy
    rs = np.random.RandomState(seed + 17 * hidden + obs_dim)
    H = hidden
    g = np.array([[GAINS[(p + j) % 3] for j in range(H)] for p in range(n_policies)])
    u = lambda lo, hi, *shape: rs.uniform(lo, hi, shape)
    bo = u(0.0, 15.0, n_policies, 4).astype(F)
    bo[0, 0], bo[(n_policies - 1) % n_policies, 1] = 26.0, -10.0
    return QuadrotorRecurrentPolicy((u(-0.5, 0.5, n_policies, H, obs_dim) * g[:, :, None]).astype(F),
                                    (u(-0.2, 0.2, n_policies, H, 4) * g[:, :, None]).astype(F),
                                    (u(-0.3, 0.3, n_policies, H) * g).astype(F),
                                    (u(-1.0, 1.0, n_policies, H) * g).astype(F),
                                    (u(-1.0, 1.0, n_policies, H, H) * g[:, :, None]).astype(F),
                                    (u(-1.0, 1.0, n_policies, H) * g).astype(F),
                                    (u(-8.0, 8.0, n_policies, 4, H) / np.sqrt(H)).astype(F),
                                    bo)


def without_memory(policy):
    """The same policies with wh, wa, wr and wd zeroed: nothing of the carry reaches a pre-activation."""
    from metagym_amd.quadrotor import QuadrotorRecurrentPolicy
    z = np.zeros_like
    return QuadrotorRecurrentPolicy(policy.wx, z(policy.wa), z(policy.wr), z(policy.wd), z(policy.wh), policy.b, policy.wo,
                                    policy.bo)


def scalar_step(policy, pid, x, pa, pr, pd, h):
    """The definition restated with explicit Python loops over np.float32 scalars for one env: no float64, no vector
    operation, nothing shared with QuadrotorRecurrentPolicy.reference. Returns (a [4], hn [H])."""
    D, H = policy.obs_dim, policy.hidden
    one = F(1.0)
    hn = []
    for j in range(H):
        z = F(policy.b[pid, j])
        for i in range(D):
            z = F(z + F(F(policy.wx[pid, j, i]) * F(x[i])))
        for k in range(4):
            z = F(z + F(F(policy.wa[pid, j, k]) * F(pa[k])))
        z = F(z + F(F(policy.wr[pid, j]) * F(pr)))
        z = F(z + F(F(policy.wd[pid, j]) * (F(1.0) if pd else F(0.0))))
        for i in range(H):
            z = F(z + F(F(policy.wh[pid, j, i]) * F(h[i])))
        hn.append(one if z > one else (-one if z < -one else z))
    a = []
    for k in range(4):
        v = F(policy.bo[pid, k])
        for j in range(H):
            v = F(v + F(F(policy.wo[pid, k, j]) * hn[j]))
        a.append(v)
    return np.array(a, F), np.array(hn, F)


def closed_loop_oracle(og, policy, ids, steps, prime=pc.PRIME_ACTION):
    """The recurrent closed loop on the CPU oracle from a fresh carry: prime, then `steps` times
    (QuadrotorRecurrentPolicy.reference, OracleGroups.step, QuadrotorPolicyState.observed). Returns the actions
    [steps, N, 4], the memories [steps, N, H] and the end carry."""
    from metagym_amd.quadrotor import QuadrotorPolicyState
    obs = og.step(prime)[0]
    state = QuadrotorPolicyState.zeros(len(ids), policy.hidden)
    acts, mems = [], []
    for _ in range(steps):
        a, state = policy.reference(obs, ids, state)
        obs, rew, done, _ = og.step(a)
        state = state.observed(rew.astype(F), done)
        acts.append(a)
        mems.append(state.h.copy())
    return np.stack(acts), np.stack(mems), state
