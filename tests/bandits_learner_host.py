"""Host side of the classical-learner tests (tests/test_bandits_learner.py, tests/test_bandits_learner_gpu.py).

TEST INFRASTRUCTURE. `host_rollout` is the closed loop on the host: `BanditLearner.reference` for the action, the reference's
env (bandits_oracle.Env) for the step, the count update of the definition. `make_learner` and `random_counts` are the cases
both files use; `thompson_probe_case` is the one batch whose attempt counts the CPU test inspects and the GPU test compares.
"""
import numpy as np

import bandits_oracle as bo
from metagym_amd.bandits import BanditLearner, BanditLearnerState, gittins_index_table

F = np.float32
MEAN, DEVIATION = 0.45, 0.15
KINDS = ("greedy", "ucb", "table", "thompson")
_TABLES = {}


def gittins_rows(P, cap=12, discount=0.9):
    """P rows: the Gittins table (computed once per cap) and copies of it scaled a little, so the rows differ."""
    if (cap, discount) not in _TABLES:
        _TABLES[(cap, discount)] = gittins_index_table(cap, discount, depth=40, grid=200)
    row = _TABLES[(cap, discount)]
    return np.stack([(row * F(1.0 - 0.01 * p)).astype(F) for p in range(P)])


def make_learner(kind, K, P=3, epsilon=None, max_attempts=64, cap=12):
    if kind == "greedy":
        return BanditLearner.greedy(K, np.array([[1.0, 1.0], [0.5, 2.0], [3.0, 0.25]], F)[:P], epsilon)
    if kind == "ucb":
        return BanditLearner.ucb(K, np.array([2.0, 0.5, 0.0], F)[:P], epsilon)
    if kind == "table":
        return BanditLearner.table(K, gittins_rows(P, cap), epsilon)
    return BanditLearner.thompson(K, np.array([[1.0, 1.0], [2.0, 1.0], [1.0, 5.0]], F)[:P], max_attempts)


def random_counts(N, K, seed, top=5000, zero_rows=True):
    """Counts up to `top` with 0 <= wins <= pulls; small ones too (the table's triangle, UCB's unpulled arms), and rows of
    zeros."""
    rs = np.random.RandomState(seed)
    pulls = rs.randint(0, top + 1, (N, K))
    small = rs.rand(N, K) < 0.4
    pulls[small] = rs.randint(0, 16, (N, K))[small]
    pulls[rs.rand(N) < 0.5] += 1                                           # rows without an unpulled arm
    wins = (pulls * rs.rand(N, K)).astype(np.int64)
    wins[rs.rand(N, K) < 0.1] = 0
    full = rs.rand(N, K) < 0.1
    wins[full] = pulls[full]
    if zero_rows:
        pulls[::7], wins[::7] = 0, 0
    return BanditLearnerState(pulls.astype(np.int32), wins.astype(np.int32), step=(3 << 32) | 11)


def thompson_probe_case(max_attempts=64):
    """(learner, ids, state, seed) of the N = 130, K = 10 Thompson probe."""
    N, K = 130, 10
    return make_learner("thompson", K, 3, max_attempts=max_attempts), np.arange(N) % 3, random_counts(N, K, 5), (7 << 32) | 19


class Host(object):
    """The host mirror of a batch: one numpy RandomState per env, gains, steps and over."""

    def __init__(self, seeds, K, M, dist):
        self.K, self.M, self.dist = K, M, dist
        self.rss = bo.seeded(seeds)
        self.gains = np.stack([bo.sample_task(rs, K, dist, MEAN, DEVIATION) for rs in self.rss])
        self.steps = np.zeros(len(seeds), np.int64)
        self.over = np.ones(len(seeds), np.uint8)


def best_of(row):
    best = row[0]
    for v in row[1:]:
        if v > best:
            best = v
    return best


def host_rollout(learner, ids, host, state0, T, auto_reset, resample, seed=0, episodic=True):
    """Advances `host` in place; returns (records dict of [T, N] arrays, results dict of [N] arrays, end carry)."""
    N, K, M = len(host.rss), host.K, host.M
    envs = []
    for e in range(N):
        env = bo.Env(host.rss[e], K, M)
        env.exp_gains, env.steps, env.need_reset = host.gains[e], int(host.steps[e]), bool(host.over[e])
        envs.append(env)
    rec = dict(actions=np.full((T, N), -1, np.int32), reward=np.zeros((T, N), F), done=np.zeros((T, N), bool),
               info_steps=np.zeros((T, N), np.int32), expected_gain=np.zeros((T, N)), best_gain=np.zeros((T, N)),
               invalid=np.full((T, N), 2, np.uint8))
    out = dict(ret_total=np.zeros(N), ret_episode=np.zeros(N), episode_len=np.zeros(N, np.int32),
               episodes=np.zeros(N, np.int32), regret=np.zeros(N))
    first_done = np.zeros(N, bool)
    best = [best_of(env.exp_gains) for env in envs]
    st = state0.numpy()
    st = BanditLearnerState(st.pulls.copy(), st.wins.copy(), st.step)
    for t in range(T):
        acts = learner.reference(ids, st, seed=seed)
        for e, env in enumerate(envs):
            if env.need_reset:                              # over: nothing happens, the records keep their defaults
                rec["info_steps"][t, e] = env.steps
                continue
            a = int(acts[e])
            _, r, d, info = env.step(a)
            rec["actions"][t, e], rec["reward"][t, e], rec["done"][t, e] = a, r, d
            rec["info_steps"][t, e], rec["expected_gain"][t, e] = info["steps"], info["expected_gain"]
            rec["best_gain"][t, e], rec["invalid"][t, e] = best[e], 0
            out["ret_total"][e] = out["ret_total"][e] + np.float64(F(r))
            if not first_done[e]:
                out["ret_episode"][e] = out["ret_episode"][e] + np.float64(F(r))
                out["episode_len"][e] += 1
                first_done[e] = d
            out["episodes"][e] += int(d)
            out["regret"][e] = out["regret"][e] + (best[e] - info["expected_gain"])
            st.pulls[e, a] += 1
            st.wins[e, a] += int(r == 1)
            if d and auto_reset:
                if resample:
                    env.set_task(env.sample_task(host.dist, MEAN, DEVIATION))
                    best[e] = best_of(env.exp_gains)
                env.reset()
                if episodic:
                    st.pulls[e], st.wins[e] = 0, 0
        st.step += 1
    for e, env in enumerate(envs):
        host.gains[e], host.steps[e], host.over[e] = env.exp_gains, env.steps, env.need_reset
    return rec, out, st
