"""`Bandits.rollout_policy` with a softmax-sampled policy (mg_bandits_policy_rollout_sampled, csrc/bandits_policy.hip and
csrc/mg_sample.h): the action of every env at every step is a Gumbel-max draw from softmax(l / temperature) inside the launch.
  1. the full closed-loop oracle, `BanditPolicy.reference` alternated with the reference's env on the host, bit for bit;
  2. replay identity through `rollout`; 3. splitting a rollout; 4. record=False; 5. epsilon with a temperature; 6. the cold
  limit against the greedy kernel; 7. hipGraph capture; 8. `BanditPolicyNet.replay` on the device; 10. a learning smoke.
The host helpers are those of test_bandits_policy_gpu.py. GPU box only (-m gpu)."""
import numpy as np
import pytest
import torch

from metagym_amd._policy import gumbel32, philox4x32_10
from metagym_amd.bandits import BanditPolicy, BanditPolicyNet, BanditPolicyState, Bandits, log_prob
from test_bandits_policy_gpu import (RECORDS, RESULTS, _np, check_against_host, host_rollout, make_env, make_policy, same_carry,
                                     same_results, same_sd)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
TEMPS = np.array([0.25, 1.0, 4.0], F)


def sampled(pol, temperature=TEMPS, epsilon=None):
    return BanditPolicy(pol.wa, pol.wr, pol.wd, pol.wh, pol.b, pol.wo, pol.bo, epsilon=epsilon, temperature=temperature)


def start(N, K, M, dist="Classical", auto_reset=True, seed0=300):
    """Envs at different stream positions (env e took 5 e mod 23 steps before), every seventh never reset (over)."""
    mask = np.arange(N) % 7 != 3
    pre = np.where(mask, (5 * np.arange(N)) % 23, 0)
    return make_env(N, K, M, dist, auto_reset=auto_reset, pre_steps=pre, reset_mask=mask, seed0=seed0), mask


def host_logits(pol, ids, actions, reward, done, episodic=False):
    """The float32 logits [T, N, K] of recorded steps: `reference` driven by the records (a fresh carry at step 0)."""
    T, N = actions.shape
    st = BanditPolicyState.zeros(N, pol.hidden)
    out = np.zeros((T, N, pol.arms), F)
    for t in range(T):
        _, hn, out[t] = pol.reference(ids, st, return_logits=True)
        took = actions[t] >= 0
        st.h[took], st.prev_action[took], st.prev_reward[took] = hn[took], actions[t][took], reward[t][took]
        st.prev_done[took] = done[t][took]
        if episodic:
            c = took & done[t]
            st.h[c], st.prev_action[c], st.prev_reward[c], st.prev_done[c] = 0, -1, 0, 0
    return out


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("ids_kind", ["one id per wave", "mixed ids"])
@pytest.mark.parametrize("H,K", [(1, 2), (5, 5), (32, 10), (64, 64)])
def test_full_closed_loop_oracle(H, K, ids_kind):
    """N = 130 (two full waves and a partial one), T = 40 with max_steps = 7: five or six episodes end per env, each with a
    task draw from the env's own stream. One id per wave stages the policy in LDS, mixed ids read it per lane. K = 5 reads one
    word of a second Philox block, K = 10 two of a third, K = 64 sixteen whole blocks. The counter crosses 2^32."""
    N, M, T, P = 130, 7, 40, 3
    (env, host), mask = start(N, K, M, seed0=300 + K)
    pol = sampled(make_policy(P, H, K, 10 * K + H))
    ids = (np.arange(N) // 64) % P if ids_kind == "one id per wave" else np.arange(N) % P
    state0 = BanditPolicyState.zeros(N, H, DEV)
    state0.step = (1 << 32) - 20
    before = state0.clone()
    seed = (5 << 32) | 17
    res = env.rollout_policy(pol, T, policy_ids=ids, state=state0, seed=seed, record=True)
    same_carry(state0, before, "the carry handed in is not written")
    assert res.state.step == state0.step + T and res.actions.shape == (T, N)
    rec, out, carry, explored = host_rollout(pol, ids, host, before, T, True, True, seed=seed)
    check_against_host(res, env, rec, out, carry, host, (H, K, ids_kind))
    # the case does what it is for
    acts = rec["actions"]
    assert not explored.any() and (acts[:, ~mask] == -1).all() and (acts[:, mask] >= 0).all()
    assert (rec["done"][:, mask].sum(0) >= T // M).all()
    used = np.bincount(acts[acts >= 0], minlength=K)
    print("arms used", int((used > 0).sum()), "of", K, "mean regret per step %.4f" % (out["regret"][mask].mean() / T))
    assert (used > 0).sum() >= min(K, 8)                                     # a draw, not an argmax: the arms get played


# ---------------------------------------------------------------------------------------------------------- 2, 3, 4
def test_replay_splitting_and_record_false():
    N, K, H, M, T, P = 130, 10, 5, 7, 40, 3
    (env, _), mask = start(N, K, M, dist="Uniform")
    pol = sampled(make_policy(P, H, K, 21))
    sd0 = env.state_dict()
    whole = env.rollout_policy(pol, T, seed=3, record=True)
    sd1 = env.state_dict()
    # 2. the recorded actions through `rollout` from the same state: the same records and end state (-1 is refused there as
    # it is skipped here: the env was over)
    env.load_state_dict(sd0)
    reward, done, info = env.rollout(whole.actions)
    assert torch.equal(reward.view(torch.int32), whole.reward.view(torch.int32)) and torch.equal(done, whole.done)
    assert torch.equal(info["steps"], whole.info_steps)
    assert torch.equal(info["expected_gain"].view(torch.int64), whole.expected_gain.view(torch.int64))
    same_sd(env.state_dict(), sd1, "replay")
    # 3. T1 = 13 then T2 = 27 through one carry
    env.load_state_dict(sd0)
    a = env.rollout_policy(pol, 13, seed=3, record=True)
    b = env.rollout_policy(pol, 27, state=a.state, seed=3, record=True)
    for name in RECORDS:
        assert torch.equal(torch.cat([getattr(a, name), getattr(b, name)]), getattr(whole, name)), name
    same_sd(env.state_dict(), sd1, "split")
    same_carry(b.state, whole.state, "split")
    assert (a.state.step, b.state.step) == (13, 40)
    assert torch.equal(a.episodes + b.episodes, whole.episodes) and torch.equal(a.ret_total + b.ret_total, whole.ret_total)
    # 4. record=False
    env.load_state_dict(sd0)
    lean = env.rollout_policy(pol, T, seed=3)
    assert all(getattr(lean, name) is None for name in RECORDS)
    same_results(lean, whole, "record=False", RESULTS)
    same_sd(env.state_dict(), sd1, "record=False")
    same_carry(lean.state, whole.state, "record=False")
    # another seed: other draws
    env.load_state_dict(sd0)
    assert not torch.equal(env.rollout_policy(pol, T, seed=4, record=True).actions, whole.actions)


# ---------------------------------------------------------------------------------------------------------- 5
def test_epsilon_with_a_temperature():
    N, K, H, M, T, P = 130, 10, 5, 7, 40, 3
    seed, step0 = (9 << 32) | 4, (1 << 32) - 7
    base = make_policy(P, H, K, 31)
    ids = np.arange(N) % P

    def run(epsilon):
        (env, host), _ = start(N, K, M)
        st = BanditPolicyState.zeros(N, H, DEV)
        st.step = step0
        pol = sampled(base, epsilon=epsilon)
        return env.rollout_policy(pol, T, state=st, seed=seed, record=True), env, host, pol, st
    none = run(None)[0]
    mid, env, host, pol, st = run(np.array([0.25, 0.0, 0.6]))
    rec, outs, carry, explored = host_rollout(pol, ids, host, st, T, True, True, seed=seed)
    check_against_host(mid, env, rec, outs, carry, host, "epsilon and temperature")
    n = step0 + np.arange(T, dtype=np.uint64)[:, None]
    out = philox4x32_10(np.arange(N, dtype=np.uint64)[None, :], n & np.uint64(0xFFFFFFFF), n >> np.uint64(32), 0x4241, 4, 9)
    took = _np(mid.actions) >= 0
    assert np.array_equal(explored, (out[0] < pol.thresholds[ids][None, :]) & took)
    assert not explored[:, ids == 1].any() and 0 < explored[:, ids == 0].sum() < took[:, ids == 0].sum()
    # where the draw fires the action is out[1] % K; at step 0 (one shared history) the sampled action stands elsewhere
    assert np.array_equal(_np(mid.actions)[explored], (out[1] % np.uint32(K)).astype(np.int32)[explored])
    assert np.array_equal(_np(mid.actions)[0][~explored[0]], _np(none.actions)[0][~explored[0]])
    assert (_np(mid.actions)[0][explored[0]] != _np(none.actions)[0][explored[0]]).any()
    # epsilon = 0 equals epsilon = None
    same_results(run(np.zeros(P))[0], none, "epsilon = 0")


# ---------------------------------------------------------------------------------------------------------- 6
def test_the_cold_limit_equals_the_greedy_kernel():
    """temperature 2^-20 and logit gaps of at least 2^-10: a gap times inv_t is at least 1024, the Gumbel values span less
    than 19.5, so the draw is the argmax. The policy is built so the gaps hold: every hidden unit saturates (b = +-2 and all
    other input weights multiples of 8: |z| >= 2), wo holds multiples of 2^-5 and bo[k] = k 2^-10, so the logits are distinct
    modulo 2^-5 and exact in float32."""
    N, K, H, M, T, P = 130, 10, 5, 7, 40, 2
    rs = np.random.RandomState(6)
    pm = lambda *s: rs.choice([-1.0, 1.0], s)
    w = ((8 * pm(P, H, K)).astype(F), (16 * pm(P, H)).astype(F), (32 * pm(P, H)).astype(F), (64 * pm(P, H, H)).astype(F),
         (2 * pm(P, H)).astype(F), (rs.randint(-32, 33, (P, K, H)) / 32.0).astype(F),
         np.tile(np.arange(K) * 2.0 ** -10, (P, 1)).astype(F))
    cold = BanditPolicy(*w, temperature=np.full(P, 2.0 ** -20, F))
    greedy = BanditPolicy(*w)
    assert cold.inv_temperature.tolist() == [2.0 ** 20] * P
    ids = np.arange(N) % P
    (env_c, _), mask = start(N, K, M)
    (env_g, _), _ = start(N, K, M)
    c = env_c.rollout_policy(cold, T, seed=8, record=True)
    g = env_g.rollout_policy(greedy, T, seed=8, record=True)
    same_results(c, g, "cold limit")
    same_carry(c.state, g.state, "cold limit")
    same_sd(env_c.state_dict(), env_g.state_dict(), "cold limit")
    # on the host: every gap of every recorded step, times inv_t, exceeds the whole Gumbel range
    logits = host_logits(greedy, ids, _np(c.actions), _np(c.reward), _np(c.done))
    top = np.sort(logits, axis=2)
    gap = (top[:, :, -1] - top[:, :, -2]).astype(np.float64)
    assert (gap * 2.0 ** 20 > 19.5).all() and gap.min() >= 2.0 ** -10
    words = np.array([0, 0xFFFFFFFF], np.uint32)
    assert float(gumbel32(words)[1]) - float(gumbel32(words)[0]) < 19.5
    acts = _np(c.actions)
    assert np.array_equal(acts[:, mask], logits.argmax(2).astype(np.int32)[:, mask]) and len(set(acts[acts >= 0].tolist())) >= 2


# ---------------------------------------------------------------------------------------------------------- 7
def test_graph_capture_of_one_call():
    """Captured once and replayed twice, the call equals eager calls on a twin env. step0 is an argument of the launch, so a
    replay draws with the counters of the captured call: the eager twin is handed the same step."""
    from test_graph_capture_gpu import _capture
    N, K, H, M, T, P = 130, 10, 5, 7, 25, 3
    pol = sampled(make_policy(P, H, K, 17))
    pol.to(DEV)
    pol.inv_temperature_on(DEV)
    (eager, _), _ = start(N, K, M, dist="Uniform")
    (env, _), _ = start(N, K, M, dist="Uniform")
    static = BanditPolicyState.zeros(N, H, DEV)
    names = ("h", "prev_action", "prev_reward", "prev_done")
    out = {}

    def run():
        res = env.rollout_policy(pol, T, state=static, seed=5, record=True)
        for name in names:
            getattr(static, name).copy_(getattr(res.state, name))
        out["res"] = res

    sd0 = env.state_dict()
    graph = _capture(run)
    env.load_state_dict(sd0)
    zero = BanditPolicyState.zeros(N, H, DEV)
    for name in names:
        getattr(static, name).copy_(getattr(zero, name))
    st = None
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        if st is not None:
            st.step = 0
        want = eager.rollout_policy(pol, T, state=st, seed=5, record=True)
        st = want.state
        same_results(out["res"], want, rep)
        assert torch.equal(static.h.view(torch.int32), st.h.view(torch.int32)) and torch.equal(static.prev_action, st.prev_action)
        same_sd(env.state_dict(), eager.state_dict(), rep)
    assert bool(out["res"].done.any())


# ---------------------------------------------------------------------------------------------------------- 8
def test_replay_on_the_device_is_exact_where_the_sums_are():
    """Weights that are multiples of 1/4 in [-1, 1], H = 5, K = 3, T = 5, 0 / 1 rewards: every sum of the network is exact in
    float32 (test_sampled_policy.py proves it against float64), so the device replay, whatever its order of summation,
    must return the reference's logits bit for bit."""
    N, K, H, M, T = 130, 3, 5, 3, 5
    rs = np.random.RandomState(0)
    q = lambda *s: (rs.randint(-4, 5, s) / 4.0).astype(F)
    pol = BanditPolicy(q(1, H, K), q(1, H), q(1, H), q(1, H, H), q(1, H), q(1, K, H), q(1, K), temperature=np.ones(1, F))
    ids = np.zeros(N, np.int64)
    for episodic in (False, True):
        (env, _), mask = start(N, K, M)
        res = env.rollout_policy(pol, T, seed=1, record=True, episodic=episodic)
        want = host_logits(pol, ids, _np(res.actions), _np(res.reward), _np(res.done), episodic=episodic)
        net = BanditPolicyNet.from_policy(pol).to(DEV)
        got = net.replay(res.actions, res.reward, res.done, episodic=episodic)
        assert got.is_cuda and got.requires_grad and got.shape == (T, N, K)
        assert np.array_equal(_np(got.detach()), want)
        assert bool(res.done.any()) and (_np(res.actions)[:, ~mask] == -1).all()
        lp = log_prob(got, res.actions, 1.0)
        assert lp.shape == (T, N) and not bool(lp[:, torch.as_tensor(~mask, device=DEV)].any()) and bool((lp <= 0).all())


# ---------------------------------------------------------------------------------------------------------- 10
LEARNING_ITERATIONS = 14


def test_learning_smoke():
    """REINFORCE with Adam (lr 0.1) on the fast path: N = 1024 envs, K = 2 with fixed gains (0.9, 0.1), T = 10 pulls, H = 4,
    zero initial weights, temperature 1, a per-step mean baseline over the envs. Per iteration one sampled
    `rollout_policy(record=True)` launch, one `replay`, one optimiser step, then repack. The mean reward per pull starts at
    0.5 (uniform play) and the optimum is 0.9; the last iteration must exceed 0.7, halfway between. On one MI355X run the
    mean reward per pull was 0.501 at iteration 0 and first exceeded 0.7 at iteration 6, the seventh (0.896 after 60);
    LEARNING_ITERATIONS = 14 is twice seven."""
    N, K, H, T = 1024, 2, 4, 10
    env = Bandits(num_envs=N, arms=K, max_steps=T, device=DEV, seed=0, auto_reset=True)
    env.set_task(torch.tensor([[0.9, 0.1]], dtype=torch.float64, device=DEV).repeat(N, 1))
    env.reset()
    net = BanditPolicyNet(H, K).to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=0.1)
    means = []
    for it in range(LEARNING_ITERATIONS):
        res = env.rollout_policy(net.to_policy(temperature=1.0), T, seed=it, record=True, episodic=True)
        logits = net.replay(res.actions, res.reward, res.done, episodic=True)
        ret = res.reward.flip(0).cumsum(0).flip(0)                           # the reward to go
        adv = ret - ret.mean(1, keepdim=True)
        loss = -(log_prob(logits, res.actions, 1.0) * adv).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        means.append(float(res.reward.mean()))
    first = next((i for i, m in enumerate(means) if m > 0.7), None)
    print("mean reward per pull: first %.3f, last %.3f, first above 0.7 at iteration %s" % (means[0], means[-1], first))
    assert abs(means[0] - 0.5) < 0.05
    assert means[-1] > 0.7
