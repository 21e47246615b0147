"""Softmax-sampled policies on the host: the Gumbel-max draw (`_policy.gumbel32`, `sample_actions`), the sampled
`BanditPolicy.reference` / `MazePolicy.reference`, the torch modules `BanditPolicyNet` / `MazePolicyNet`, and the host half of
mg_bandits_policy_rollout_sampled / mg_maze2d_policy_rollout_sampled.
  1. the draw over all 2^23 values u01 can return; 2. the sampled reference: the order of its operations, a scalar
  restatement, what moves the draw, and temperature=None; 3. the distribution of the draw; 4. refusals and pack / unpack;
  5. `replay` is exact where every sum is exact; 6. its gradients; 7. from_policy / to_policy; 8. the declarations; 9. the
  host refusals. No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from metagym_amd import _policy
from metagym_amd._policy import SAMPLE_TAG, gumbel32, log32, philox4x32_10, sample_actions, u01
from metagym_amd.bandits import BanditPolicy, BanditPolicyNet, BanditPolicyState, log_prob
from metagym_amd.metamaze import MazePolicy, MazePolicyNet, MazePolicyState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def random_bandit_policy(P, H, K, seed, epsilon=None, temperature=None):
    rs = np.random.RandomState(seed)
    return BanditPolicy((1.5 * rs.randn(P, H, K)).astype(F), (1.5 * rs.randn(P, H)).astype(F), rs.randn(P, H).astype(F),
                        (rs.randn(P, H, H) * (2.0 / np.sqrt(H))).astype(F), (0.3 * rs.randn(P, H)).astype(F),
                        (rs.randn(P, K, H) / np.sqrt(H)).astype(F), (0.2 * rs.randn(P, K)).astype(F), epsilon, temperature)


def random_maze_policy(P, H, vg, seed, epsilon=None, temperature=None):
    rs = np.random.RandomState(seed)
    D = (2 * vg + 1) ** 2 + 6
    return MazePolicy((rs.randn(P, H, D) / np.sqrt(D)).astype(F), (rs.randn(P, H, H) / np.sqrt(H)).astype(F),
                      (0.3 * rs.randn(P, H)).astype(F), (rs.randn(P, 4, H) / np.sqrt(H)).astype(F), (0.2 * rs.randn(P, 4)).astype(F),
                      epsilon, temperature)


def random_bandit_state(N, H, K, seed, step=0):
    rs = np.random.RandomState(seed)
    return BanditPolicyState(rs.uniform(-1, 1, (N, H)).astype(F), rs.randint(-1, K, N).astype(np.int32),
                             rs.randint(0, 2, N).astype(F), rs.randint(0, 2, N).astype(np.uint8), step)


# ---------------------------------------------------------------------------------------------------------- 1
def test_the_draw_over_every_value_of_u01():
    """u01 keeps the top 23 bits of a word: 2^23 values, all visited in ascending order."""
    words = np.arange(1 << 23, dtype=np.uint32) << np.uint32(9)
    u = u01(words)
    assert u.dtype == F and (np.diff(u) > 0).all() and u[0] == F(2.0 ** -24) and u[-1] == F(1.0 - 2.0 ** -24)
    y = -log32(u)
    assert y.dtype == F and np.isfinite(y).all() and (y >= np.finfo(F).tiny).all()      # positive and normal: log32 may take it
    g = -log32(y)
    assert g.dtype == F and np.isfinite(g).all() and np.array_equal(g, gumbel32(words))
    assert (np.diff(g) >= 0).all() and g[0] < g[-1]                                      # monotone in u
    exact = -np.log(-np.log(u.astype(np.float64)))
    err = np.abs(g.astype(np.float64) - exact).max()
    print("y in [%.4g, %.4g], g in [%.4f, %.4f], max |g - float64 Gumbel| = %.3g" % (y.min(), y.max(), g.min(), g.max(), err))
    assert err <= 1e-6
    assert 5.9e-8 < y.min() and y.max() < 16.64 and -2.8117 < g.min() and g.max() < 16.6357


# ---------------------------------------------------------------------------------------------------------- 2
def test_the_order_of_the_sampled_argmax_by_hand():
    """score = (l * inv_t) + g with two roundings; the lowest index among equal maxima; a NaN score at index 0 stays, a
    later one never wins."""
    N = 4096
    rs = np.random.RandomState(3)
    logits = (3.0 * rs.randn(N, 4)).astype(F)
    inv_t = np.full(N, F(1.0) / F(0.7), F)
    e = np.arange(N, dtype=np.uint64)
    out = philox4x32_10(e, 5, 0, SAMPLE_TAG, 17, 9)
    g = np.stack([gumbel32(out[k]) for k in range(4)], 1)
    score = np.empty((N, 4), F)
    for n in range(N):
        for k in range(4):
            score[n, k] = F(F(logits[n, k] * inv_t[n]) + g[n, k])
    want = np.zeros(N, np.int32)
    for n in range(N):
        best = score[n, 0]
        for k in range(1, 4):
            if score[n, k] > best:
                want[n], best = k, score[n, k]
    got = sample_actions(logits, inv_t, e, 5, (9 << 32) | 17)
    assert got.dtype == np.int32 and np.array_equal(got, want) and sorted(set(got.tolist())) == [0, 1, 2, 3]
    # the case tells the orders apart: a fused multiply-add, or the sum scaled afterwards, gives other score bits somewhere
    fused = (logits.astype(np.float64) * inv_t[:, None].astype(np.float64) + g.astype(np.float64)).astype(F)
    assert (fused != score).any()
    # ties: equal infinite scores; the lowest index of them wins, and a finite arm 0 loses to them
    tie = np.array([[0.0, np.inf, np.inf, 1.0], [np.inf, np.inf, 0.0, 0.0], [-np.inf, -np.inf, -np.inf, -np.inf]], F)
    assert sample_actions(tie, inv_t[:3], e[:3], 0, 0).tolist() == [1, 0, 0]
    # NaN at index 0 stays (nothing is greater than it); a NaN later never wins
    nan = np.array([[np.nan, 100.0, 0.0, 0.0], [0.0, np.nan, -100.0, np.nan], [-100.0, np.nan, np.nan, 100.0]], F)
    assert sample_actions(nan, inv_t[:3], e[:3], 0, 0).tolist() == [0, 0, 3]


def scalar_bandit_step(pol, p, h, pa, pr, pd, e, n, seed):
    """The definition of bandits/policy.py for one env in Python loops over numpy float32 scalars: (action, hn, logits)."""
    H, K = pol.hidden, pol.arms
    hn = np.zeros(H, F)
    for j in range(H):
        z = pol.b[p, j]
        if pa >= 0:
            z = F(z + pol.wa[p, j, pa])
        z = F(z + F(pol.wr[p, j] * pr))
        z = F(z + F(pol.wd[p, j] * F(1.0 if pd else 0.0)))
        for i in range(H):
            z = F(z + F(pol.wh[p, j, i] * h[i]))
        hn[j] = F(1.0) if z > 1 else (F(-1.0) if z < -1 else z)
    logits = np.zeros(K, F)
    for k in range(K):
        v = pol.bo[p, k]
        for j in range(H):
            v = F(v + F(pol.wo[p, k, j] * hn[j]))
        logits[k] = v
    inv_t = F(F(1.0) / pol.temperature[p])
    action, best = 0, None
    for k in range(K):
        out = philox4x32_10(e, n & 0xFFFFFFFF, n >> 32, SAMPLE_TAG | (k >> 2), seed & 0xFFFFFFFF, seed >> 32)
        u = F(int(((int(out[k & 3]) >> 9) << 1) | 1)) * F(2.0 ** -24)
        g = -log32(-log32(np.array([u], F)))[0]
        s = F(F(logits[k] * inv_t) + g)
        if k == 0:
            best = s
        elif s > best:
            action, best = k, s
    return action, hn, logits


@pytest.mark.parametrize("H,K", [(1, 2), (5, 3), (7, 10), (64, 64), (6, 5)])
def test_the_sampled_reference_against_a_scalar_restatement(H, K):
    P, N = 3, 7
    pol = random_bandit_policy(P, H, K, 100 * H + K, temperature=np.array([0.5, 1.0, 3.0], F))
    ids = np.arange(N) % P
    st = random_bandit_state(N, H, K, 7, step=(1 << 32) + 5)
    seed = (11 << 32) | 3
    acts, hn, logits = pol.reference(ids, st, seed=seed, return_logits=True)
    assert acts.dtype == np.int32 and logits.dtype == F and logits.shape == (N, K)
    for e in range(N):
        a, h1, l1 = scalar_bandit_step(pol, ids[e], st.h[e], int(st.prev_action[e]), st.prev_reward[e], st.prev_done[e], e,
                                       st.step, seed)
        assert a == acts[e] and np.array_equal(h1.view(np.uint32), hn[e].view(np.uint32))
        assert np.array_equal(l1.view(np.uint32), logits[e].view(np.uint32))
    # return_explored and return_logits together, in that order; nothing explored without epsilon
    a4 = pol.reference(ids, st, seed=seed, return_explored=True, return_logits=True)
    assert len(a4) == 4 and not a4[2].any() and np.array_equal(a4[3], logits)


def test_five_arms_read_one_word_of_the_second_block():
    """Zero weights and zero output biases: the action is the argmax of the Gumbel values alone, and arm 4's comes from
    word 0 of the block with c3 = SAMPLE_TAG | 1."""
    N, H, K = 2000, 6, 5
    z = lambda *s: np.zeros(s, F)
    pol = BanditPolicy(z(1, H, K), z(1, H), z(1, H), z(1, H, H), z(1, H), z(1, K, H), z(1, K), temperature=np.ones(1, F))
    st = BanditPolicyState.zeros(N, H)
    st.step = 9
    acts = pol.reference(np.zeros(N, np.int64), st, seed=4)[0]
    e = np.arange(N, dtype=np.uint64)
    b0, b1 = philox4x32_10(e, 9, 0, SAMPLE_TAG, 4, 0), philox4x32_10(e, 9, 0, SAMPLE_TAG | 1, 4, 0)
    g = np.stack([gumbel32(b0[0]), gumbel32(b0[1]), gumbel32(b0[2]), gumbel32(b0[3]), gumbel32(b1[0])], 1)
    assert np.array_equal(acts, g.argmax(1)) and abs((acts == 4).mean() - 0.2) < 0.04
    assert not np.array_equal(g[:, 4], gumbel32(b0[0]))


def test_seed_step_and_env_ids_move_the_draw_and_none_is_todays_rule():
    N, H, K, P = 400, 5, 10, 3
    temp = np.array([0.5, 1.0, 3.0], F)
    eps = np.array([0.0, 0.3, 1.0])
    pol = random_bandit_policy(P, H, K, 1, epsilon=eps, temperature=temp)
    greedy = random_bandit_policy(P, H, K, 1, epsilon=eps)
    ids = np.arange(N) % P
    st = random_bandit_state(N, H, K, 2, step=40)
    acts, hn, ex, logits = pol.reference(ids, st, seed=5, return_explored=True, return_logits=True)
    acts0, hn0, ex0, logits0 = greedy.reference(ids, st, seed=5, return_explored=True, return_logits=True)
    # the network and the exploration draw do not depend on the temperature; the exploratory action overrides the sampled one
    assert np.array_equal(hn, hn0) and np.array_equal(logits, logits0) and np.array_equal(ex, ex0)
    assert np.array_equal(acts[ex], acts0[ex]) and not ex[ids == 0].any() and ex[ids == 2].all()
    sampled = sample_actions(logits, (F(1.0) / temp)[ids], np.arange(N), 40, 5)
    assert np.array_equal(acts[~ex], sampled[~ex]) and (sampled[~ex] != acts0[~ex]).any()
    # today's rule without a temperature: the running argmax of the logits
    assert greedy.temperature is None and greedy.inv_temperature is None
    assert np.array_equal(acts0[~ex0], logits0.argmax(1)[~ex0])
    st2 = st.clone()
    st2.step += 1
    keep = ids == 0
    assert not np.array_equal(pol.reference(ids, st2, seed=5)[0][keep], acts[keep])
    assert not np.array_equal(pol.reference(ids, st, seed=6)[0][keep], acts[keep])
    assert not np.array_equal(pol.reference(ids, st, seed=5 + (1 << 32))[0][keep], acts[keep])
    assert not np.array_equal(pol.reference(ids, st, seed=5, env_ids=np.arange(N) + 3)[0][keep], acts[keep])
    # the maze reference takes the same draw (one block, K = 4)
    mp = random_maze_policy(2, 5, 1, 3, temperature=np.array([0.5, 2.0], F))
    mst = MazePolicyState.zeros(N, 5)
    mst.step = 12
    win = np.random.RandomState(5).randint(-1, 2, (N, 3, 3)).astype(F)
    mids = np.arange(N) % 2
    ma, _, ml = mp.reference(win, mids, mst, seed=8, return_logits=True)
    assert np.array_equal(ma, sample_actions(ml, (F(1.0) / mp.temperature)[mids], np.arange(N), 12, 8))
    m0 = random_maze_policy(2, 5, 1, 3)
    ma0, _, ml0 = m0.reference(win, mids, mst, seed=8, return_logits=True)
    assert np.array_equal(ml, ml0) and np.array_equal(ma0, ml0.argmax(1)) and (ma != ma0).any()


# ---------------------------------------------------------------------------------------------------------- 3
def test_the_draw_follows_the_softmax():
    """Zero weights, bo = (0, 0.5, 1, 2), temperature 0.7, 2^18 envs, one step: the chi-square of the action counts against
    softmax(bo / 0.7) has 3 degrees of freedom; 21.1 is its 1e-4 upper quantile. Deterministic given the seed (0, chosen
    before looking); plain numpy uniforms in place of Philox gave 1.07."""
    N, H = 1 << 18, 1
    z = lambda *s: np.zeros(s, F)
    bo = np.array([[0.0, 0.5, 1.0, 2.0]], F)
    pol = BanditPolicy(z(1, H, 4), z(1, H), z(1, H), z(1, H, H), z(1, H), z(1, 4, H), bo, temperature=np.array([0.7], F))
    acts = pol.reference(np.zeros(N, np.int64), BanditPolicyState.zeros(N, H), seed=0)[0]
    p = np.exp(bo[0].astype(np.float64) / 0.7)
    p /= p.sum()
    counts = np.bincount(acts, minlength=4).astype(np.float64)
    chi2 = float((((counts - N * p) ** 2) / (N * p)).sum())
    print("counts", counts.astype(int).tolist(), "expected", np.round(N * p, 1).tolist(), "chi2 %.3f" % chi2)
    assert chi2 < 21.1
    mz = MazePolicy(z(1, H, 15), z(1, H, H), z(1, H), z(1, 4, H), bo, temperature=np.array([0.7], F))
    acts_m = mz.reference(z(N, 3, 3), np.zeros(N, np.int64), MazePolicyState.zeros(N, H), seed=0)[0]
    assert np.array_equal(acts_m, acts)                                   # the same logits, counters and tag: the same draw


# ---------------------------------------------------------------------------------------------------------- 4
def test_refusals_and_the_pack_round_trip():
    H, K, P = 3, 4, 2
    z = lambda *s: np.zeros(s, F)
    args = (z(P, H, K), z(P, H), z(P, H), z(P, H, H), z(P, H), z(P, K, H), z(P, K))
    margs = (z(P, H, 15), z(P, H, H), z(P, H), z(P, 4, H), z(P, 4))
    for make in (lambda t: BanditPolicy(*args, temperature=t), lambda t: MazePolicy(*margs, temperature=t),
                 lambda t: BanditPolicy.unpack(z(P, BanditPolicy(*args).param_count), H, K, temperature=t),
                 lambda t: MazePolicy.unpack(z(P, MazePolicy(*margs).param_count), H, 1, temperature=t)):
        with pytest.raises(TypeError, match="float32"):
            make(np.ones(P))
        with pytest.raises(TypeError, match="float32"):
            make([1, 2])
        for shape in ((P + 1,), (P, 1), ()):
            with pytest.raises(ValueError, match="shape"):
                make(np.ones(shape, F))
        for bad in (0.0, -0.0, -1.0, np.inf, -np.inf, np.nan):
            with pytest.raises(ValueError, match="finite and > 0"):
                make(np.array([1.0, bad], F))
        for tiny in (1e-39, 1e-45):                                        # a subnormal temperature: 1 / t overflows
            with pytest.raises(ValueError, match="1 / temperature"):
                make(np.array([tiny, 1.0], F))
        ok = make(np.array([2.0 ** -100, 3.0e38], F))                     # both inverses are finite and > 0
        assert ok.inv_temperature.dtype == F and np.array_equal(ok.inv_temperature, F(1.0) / ok.temperature)
    pol = random_bandit_policy(P, H, K, 9, epsilon=np.array([0.1, 0.2]), temperature=np.array([0.5, 2.0], F))
    back = BanditPolicy.unpack(pol.pack(), H, K, epsilon=pol.epsilon, temperature=pol.temperature)
    assert np.array_equal(back.pack(), pol.pack()) and np.array_equal(back.temperature, pol.temperature)
    assert np.array_equal(back.thresholds, pol.thresholds) and BanditPolicy.unpack(pol.pack(), H, K).temperature is None
    mp = random_maze_policy(P, H, 2, 9, temperature=np.array([0.5, 2.0], F))
    mback = MazePolicy.unpack(mp.pack(), H, 2, temperature=mp.temperature)
    assert np.array_equal(mback.pack(), mp.pack()) and np.array_equal(mback.temperature, mp.temperature)
    assert len(pol._host()) == 2 and len(mp._host()) == 2                 # `to` keeps returning (params, thresholds)


# ---------------------------------------------------------------------------------------------------------- 5
def quarters(rs, *shape):
    return (rs.randint(-4, 5, shape) / 4.0).astype(F)


def dyadic_bandit_policy(seed=0, temperature=1.0):
    rs = np.random.RandomState(seed)
    H, K = 5, 3
    return BanditPolicy(quarters(rs, 1, H, K), quarters(rs, 1, H), quarters(rs, 1, H), quarters(rs, 1, H, H), quarters(rs, 1, H),
                        quarters(rs, 1, K, H), quarters(rs, 1, K), temperature=np.array([temperature], F))


def bandit_records(pol, T, N, episodic, seed=0):
    """Records of T steps from `reference` alternated with random 0/1 rewards: env 1 is over from step 2 on (no auto_reset
    there), env 2 is over at steps 0 and 1, dones fall at steps 1 and 3 of the envs e % 3 == 0. Returns the records, the
    float32 logits of every step and the float64 logits of the same definition."""
    rs = np.random.RandomState(seed + 50)
    H, K = pol.hidden, pol.arms
    st = BanditPolicyState.zeros(N, H)
    w64 = {k: getattr(pol, k)[0].astype(np.float64) for k in ("wa", "wr", "wd", "wh", "b", "wo", "bo")}
    h64 = np.zeros((N, H))
    actions, reward, done = np.full((T, N), -1, np.int32), np.zeros((T, N), F), np.zeros((T, N), bool)
    l32, l64 = np.zeros((T, N, K), F), np.zeros((T, N, K))
    for t in range(T):
        a, hn, logits = pol.reference(np.zeros(N, np.int64), st, seed=seed, return_logits=True)
        z = w64["b"][None] + np.where(st.prev_action[:, None] >= 0, w64["wa"].T[np.maximum(st.prev_action, 0)], 0.0)
        z = z + w64["wr"][None] * st.prev_reward[:, None] + w64["wd"][None] * (st.prev_done[:, None] != 0) + h64 @ w64["wh"].T
        hn64 = np.clip(z, -1, 1)
        l32[t], l64[t] = logits, w64["bo"][None] + hn64 @ w64["wo"].T
        over = np.zeros(N, bool)
        over[1], over[2] = t >= 2, t < 2
        r, d = rs.randint(0, 2, N).astype(F), (np.arange(N) % 3 == 0) & (t in (1, 3))
        for e in np.flatnonzero(~over):
            actions[t, e], reward[t, e], done[t, e] = a[e], r[e], d[e]
            st.h[e], st.prev_action[e], st.prev_reward[e], st.prev_done[e], h64[e] = hn[e], a[e], r[e], d[e], hn64[e]
            if d[e] and episodic:
                st.h[e], st.prev_action[e], st.prev_reward[e], st.prev_done[e], h64[e] = 0, -1, 0, 0, 0
        st.step += 1
    return actions, reward, done, l32, l64


@pytest.mark.parametrize("episodic", [False, True])
def test_bandit_replay_is_exact_where_the_sums_are(episodic):
    T, N = 5, 8
    pol = dyadic_bandit_policy()
    actions, reward, done, l32, l64 = bandit_records(pol, T, N, episodic)
    assert np.array_equal(l32.astype(np.float64), l64)                     # every sum is exact: no order can matter
    assert (actions[:, 1] == -1).sum() == 3 and done.any() and len(set(actions[actions >= 0].tolist())) == 3
    net = BanditPolicyNet.from_policy(pol)
    got = net.replay(actions, reward, done, episodic=episodic)
    assert got.dtype == torch.float32 and got.shape == (T, N, 3) and got.requires_grad
    live = actions >= 0                                                    # an env that is over: its carry stood still
    assert np.array_equal(got.detach().numpy()[live], l32[live])
    assert np.array_equal(got.detach().numpy(), l32)                       # and so its logits repeat, as the reference's do
    if episodic:                                                           # the flag matters: without it the memory is kept
        other = net.replay(actions, reward, done, episodic=False).detach().numpy()
        assert not np.array_equal(other, l32)
        assert np.array_equal(net.replay(actions, reward, done, episodic=True, auto_reset=False).detach().numpy(), other)
    # a replay that starts in the middle, from the carry that stood there
    st = BanditPolicyState.zeros(N, 5)
    for t in range(2):
        a, hn, _ = pol.reference(np.zeros(N, np.int64), st, return_logits=True)
        for e in np.flatnonzero(actions[t] >= 0):
            st.h[e], st.prev_action[e], st.prev_reward[e], st.prev_done[e] = hn[e], actions[t, e], reward[t, e], done[t, e]
            if done[t, e] and episodic:
                st.h[e], st.prev_action[e], st.prev_reward[e], st.prev_done[e] = 0, -1, 0, 0
    tail = net.replay(actions[2:], reward[2:], done[2:], state0=st, episodic=episodic).detach().numpy()
    assert np.array_equal(tail, l32[2:])


def test_maze_replay_is_exact_where_the_sums_are():
    """A 5 x 5 maze by hand: closed border, one inner wall, the goal in a corner of the 3 x 3 interior. N agents walk it with
    the sampled reference; an agent that stands in the goal row after its move is done and starts again at (1, 1).
    view_grid 1."""
    T, N, H = 6, 8, 5
    rs = np.random.RandomState(1)
    D = 15
    pol = MazePolicy(quarters(rs, 1, H, D), quarters(rs, 1, H, H), quarters(rs, 1, H), quarters(rs, 1, 4, H), quarters(rs, 1, 4),
                     temperature=np.ones(1, F))
    walls = np.ones((5, 5), F)
    walls[1:4, 1:4] = 0
    walls[2, 2] = 1
    moves = ((-1, 0), (1, 0), (0, -1), (0, 1))
    pos = [(1 + e % 3, 1 + (e // 3) % 3) if (1 + e % 3, 1 + (e // 3) % 3) != (2, 2) else (1, 1) for e in range(N)]
    window = lambda p: walls[p[0] - 1:p[0] + 2, p[1] - 1:p[1] + 2].copy()
    for episodic in (False, True):
        at = list(pos)
        st = MazePolicyState.zeros(N, H)
        w64 = {k: getattr(pol, k)[0].astype(np.float64) for k in ("wx", "wh", "b", "wo", "bo")}
        h64 = np.zeros((N, H))
        obs = np.zeros((T + 1, N, 3, 3), F)
        obs[0] = np.stack([window(p) for p in at])
        actions, reward, done = np.zeros((T, N), np.int32), np.zeros((T, N), F), np.zeros((T, N), bool)
        l32, l64 = np.zeros((T, N, 4), F), np.zeros((T, N, 4))
        for t in range(T):
            a, hn, logits = pol.reference(obs[t], np.zeros(N, np.int64), st, seed=2, return_logits=True)
            x = np.concatenate([obs[t].reshape(N, 9), (st.prev_action[:, None] == np.arange(4)), st.prev_reward[:, None],
                                st.prev_done[:, None] != 0], 1).astype(np.float64)
            hn64 = np.clip(w64["b"][None] + x @ w64["wx"].T + h64 @ w64["wh"].T, -1, 1)
            l32[t], l64[t] = logits, w64["bo"][None] + hn64 @ w64["wo"].T
            for e in range(N):
                nxt = (at[e][0] + moves[a[e]][0], at[e][1] + moves[a[e]][1])
                if walls[nxt] < 1:
                    at[e] = nxt
                goal = at[e][0] == 3
                actions[t, e], reward[t, e], done[t, e] = a[e], (1.0 if goal else -0.25), goal
                if goal:
                    at[e] = (1, 1)
                st.h[e], st.prev_action[e], st.prev_reward[e], st.prev_done[e], h64[e] = hn[e], a[e], reward[t, e], goal, hn64[e]
                if goal and episodic:
                    st.h[e], st.prev_action[e], st.prev_reward[e], st.prev_done[e], h64[e] = 0, -1, 0, 0, 0
            obs[t + 1] = np.stack([window(p) for p in at])
            st.step += 1
        assert np.array_equal(l32.astype(np.float64), l64) and done.any() and not done.all()
        net = MazePolicyNet.from_policy(pol)
        got = net.replay(obs[0], obs[1:], actions, reward, done, episodic=episodic)
        assert got.shape == (T, N, 4) and got.requires_grad and np.array_equal(got.detach().numpy(), l32)
        if episodic:
            assert not np.array_equal(net.replay(obs[0], obs[1:], actions, reward, done).detach().numpy(), l32)


# ---------------------------------------------------------------------------------------------------------- 6
def test_gradients_of_replay_and_log_prob():
    """float64, H = K = T = 3, N = 2; weights of order 0.1 keep every pre-activation well inside (-1, 1), where the clamp is
    the identity and differentiable."""
    from torch.func import functional_call
    rs = np.random.RandomState(4)
    T, N = 3, 2
    actions = torch.tensor([[0, 2], [1, -1], [2, 1]])
    reward = torch.tensor(rs.randint(0, 2, (T, N)).astype(F))
    done = torch.tensor([[False, False], [True, False], [False, False]])
    net = BanditPolicyNet(3, 3).double()
    names = [k for k, _ in net.named_parameters()]
    params = [torch.tensor(0.1 * rs.randn(*p.shape), dtype=torch.float64, requires_grad=True) for p in net.parameters()]

    def f(*ps):
        logits = functional_call(net, dict(zip(names, ps)), (actions, reward, done))
        return log_prob(logits, actions, 0.7)
    out = f(*params)
    assert out.shape == (T, N) and out[1, 1] == 0 and (out[actions >= 0] < 0).all()
    assert torch.autograd.gradcheck(f, params, eps=1e-6, atol=1e-6)
    mnet = MazePolicyNet(3, 1).double()
    mnames = [k for k, _ in mnet.named_parameters()]
    mparams = [torch.tensor(0.1 * rs.randn(*p.shape), dtype=torch.float64, requires_grad=True) for p in mnet.parameters()]
    obs = torch.tensor(rs.randint(-1, 2, (T + 1, N, 3, 3)).astype(np.float64))
    mact = torch.tensor(rs.randint(0, 4, (T, N)))

    def fm(*ps):
        return log_prob(functional_call(mnet, dict(zip(mnames, ps)), (obs[0], obs[1:], mact, reward, done)), mact,
                        torch.tensor([0.5, 2.0], dtype=torch.float64))
    assert torch.autograd.gradcheck(fm, mparams, eps=1e-6, atol=1e-6)
    # log_prob is log softmax(logits / temperature) at the action
    lg = torch.tensor(rs.randn(4, 5))
    a = torch.tensor([0, 4, -1, 2])
    want = torch.log_softmax(lg / 0.3, -1)
    lp = log_prob(lg, a, 0.3)
    assert torch.equal(lp[[0, 1, 3]], want[[0, 1, 3], [0, 4, 2]]) and lp[2] == 0


# ---------------------------------------------------------------------------------------------------------- 7
def test_from_policy_to_policy_round_trip():
    pol = random_bandit_policy(3, 6, 5, 8, temperature=np.array([0.5, 1.0, 2.0], F))
    for index in range(3):
        net = BanditPolicyNet.from_policy(pol, index)
        assert isinstance(net, torch.nn.Module) and len(list(net.parameters())) == 7
        one = net.to_policy(epsilon=np.array([0.25]), temperature=pol.temperature[index:index + 1])
        assert one.num_policies == 1 and one.pack().tobytes() == pol.pack()[index:index + 1].tobytes()
        assert np.array_equal(one.temperature, pol.temperature[index:index + 1]) and one.epsilon[0] == 0.25
    assert net.to_policy().temperature is None and net.to_policy(temperature=0.5).temperature.tolist() == [0.5]
    mp = random_maze_policy(2, 7, 2, 8)
    for index in range(2):
        mnet = MazePolicyNet.from_policy(mp, index)
        assert isinstance(mnet, torch.nn.Module) and len(list(mnet.parameters())) == 5
        one = mnet.to_policy(temperature=1.5)
        assert one.view_grid == 2 and one.pack().tobytes() == mp.pack()[index:index + 1].tobytes()
        assert one.temperature.dtype == F and one.temperature.tolist() == [1.5]
    with pytest.raises(TypeError):
        BanditPolicyNet.from_policy(mp)
    with pytest.raises(TypeError):
        MazePolicyNet.from_policy(pol)


# ---------------------------------------------------------------------------------------------------------- 8
def test_entry_points_are_declared_in_the_header_and_the_binding():
    from metagym_amd import _lib
    from metagym_amd.bandits import learner
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "metagym_hip.h")).read(), flags=re.S)
    for name, greedy in (("mg_bandits_policy_rollout_sampled", "mg_bandits_policy_rollout"),
                         ("mg_maze2d_policy_rollout_sampled", "mg_maze2d_policy_rollout")):
        m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, re.S)
        assert m and re.search(r"const\s+float\s*\*\s*inv_temperature", m.group(1)), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[greedy][1]) + 1
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
    assert re.search(r"#define\s+MG_ABI_VERSION\s+10\b", text) and _lib.ABI_VERSION == 10
    # log32 and u01 exist once, in _policy.py and in csrc/mg_sample.h
    assert learner.log32 is _policy.log32 and learner.u01 is _policy.u01
    csrc = os.path.join(ROOT, "metagym_amd", "csrc")
    holders = sorted(f for f in os.listdir(csrc) if re.search(r"float\s+(\w+_)?log32\s*\(", open(os.path.join(csrc, f)).read()))
    assert holders == ["mg_sample.h"]
    for unit in ("bandits_learner.hip", "bandits_policy_core.h", "maze_policy.hip"):
        assert '#include "mg_sample.h"' in open(os.path.join(csrc, unit)).read()
    # the two bandits policy units share one header; each holds one entry point of the pair
    for unit, entry in (("bandits_policy.hip", "mg_bandits_policy_rollout"), ("bandits_policy_sampled.hip", "mg_bandits_policy_rollout_sampled")):
        src = open(os.path.join(csrc, unit)).read()
        assert '#include "bandits_policy_core.h"' in src and re.findall(r'extern "C" int (\w+)\(', src) == [entry]
    assert "0x%08X" % SAMPLE_TAG in open(os.path.join(csrc, "mg_sample.h")).read().upper().replace("0X", "0x")


# ---------------------------------------------------------------------------------------------------------- 9
def test_abi_refuses_on_the_host_before_any_device_call():
    from metagym_amd import _lib
    lib = _lib.load()
    fake = C.create_string_buffer(256)
    base = (C.addressof(fake) + 15) & ~15
    p = C.c_void_p(base)

    # the bandits
    def config(arms=10, max_steps=7, distribution=0):
        c = _lib.BanditsConfig()
        c.arms, c.max_steps, c.auto_reset, c.distribution = arms, max_steps, 1, distribution
        return c
    st = _lib.BanditsState(base, base, base, base, base, base)
    desc = lambda n=3, h=5, k=10, params=base: _lib.BanditsPolicyDesc(params, None, n, h, k)
    carry = _lib.BanditsPolicyCarry(base, base, base, base)
    order = (("cfg", config()), ("n", 4), ("state", st), ("steps", 2), ("policy", desc()), ("ids", p), ("carry", carry),
             ("inv_t", p), ("seed", 0), ("step0", 0), ("episodic", 0), ("ret_total", p), ("ret_episode", p), ("episode_len", p),
             ("episodes", p), ("regret", p), ("actions", None), ("reward", None), ("done", None), ("info_steps", None),
             ("expected_gain", None), ("best_gain", None), ("invalid", None), ("stream", None))
    call = lambda **kw: lib.mg_bandits_policy_rollout_sampled(*[kw.get(k, v) for k, v in order])
    assert call(inv_t=None) == -1001 and b"inv_temperature" in lib.mg_last_error()
    for name in ("cfg", "state", "policy", "ids", "carry", "ret_total", "ret_episode", "episode_len", "episodes", "regret"):
        assert call(**{name: None}) == -1001, name
        assert b"NULL" in lib.mg_last_error()
    assert call(policy=desc(params=None)) == -1001
    for k in range(4):
        ptrs = [base] * 4
        ptrs[k] = None
        assert call(carry=_lib.BanditsPolicyCarry(*ptrs)) == -1001
    for k in range(6):
        ptrs = [base] * 6
        ptrs[k] = None
        assert call(state=_lib.BanditsState(*ptrs)) == -1001
    assert call(n=0) == -1002 and call(n=-1) == -1002 and call(steps=0) == -1002 and call(steps=-2) == -1002
    assert b"mg_bandits_policy_rollout_sampled" in lib.mg_last_error()
    assert call(policy=desc(n=0)) == -1002 and b"n_policies" in lib.mg_last_error()
    assert call(policy=desc(h=0)) == -1002 and b"hidden" in lib.mg_last_error()
    assert call(policy=desc(h=65)) == -1002
    assert call(cfg=config(arms=65), policy=desc(k=65)) == -1002 and b"arms" in lib.mg_last_error()
    assert call(policy=desc(k=1)) == -1002
    assert call(policy=desc(k=9)) == -1003 and b"arms" in lib.mg_last_error()
    assert call(cfg=config(arms=100)) == -1003
    assert call(policy=desc(params=base + 4)) == -1003 and b"aligned" in lib.mg_last_error()
    assert call(cfg=config(arms=1), policy=desc(k=1)) == -1003
    assert call(cfg=config(max_steps=1)) == -1003 and b"max_steps" in lib.mg_last_error()
    assert call(cfg=config(distribution=4)) == -1003 and call(cfg=config(distribution=-1)) == -1003

    # the maze
    tasks = _lib.MazeTasks()
    tasks.n, tasks.n_tasks = 9, 1
    for name in ("start", "goal", "walls", "texts", "scalars"):
        setattr(tasks, name, base)
    mst = _lib.MazeState()
    mst.task_id = mst.grid = mst.steps = base
    pol = _lib.MazePolicyDesc(3, 5, 2, base, None)
    order = (("tasks", tasks), ("task_type", 0), ("max_steps", 10), ("view_grid", 2), ("auto_reset", 1), ("n", 4), ("state", mst),
             ("steps", 2), ("obs_every", 0), ("policy", pol), ("ids", p), ("carry", carry), ("inv_t", p), ("seed", 0),
             ("step0", 0), ("episodic", 0), ("obs_last", p), ("ret_total", p), ("ret_episode", p), ("episode_len", p),
             ("episodes", p), ("actions", None), ("reward", None), ("reward64", None), ("done", None), ("obs", None),
             ("stream", None))
    call = lambda **kw: lib.mg_maze2d_policy_rollout_sampled(*[kw.get(k, v) for k, v in order])
    assert call(inv_t=None) == -1001 and b"inv_temperature" in lib.mg_last_error()
    for name in ("tasks", "state", "policy", "ids", "carry", "obs_last", "ret_total", "ret_episode", "episode_len", "episodes"):
        assert call(**{name: None}) == -1001, name
        assert b"NULL" in lib.mg_last_error()
    assert call(policy=_lib.MazePolicyDesc(3, 5, 2, None, None)) == -1001
    for k in range(4):
        ptrs = [base] * 4
        ptrs[k] = None
        assert call(carry=_lib.MazePolicyCarry(*ptrs)) == -1001
    assert call(state=_lib.MazeState()) == -1001
    assert call(task_type=1) == -1001
    assert call(n=0) == -1002 and call(steps=0) == -1002 and call(obs_every=-1) == -1002
    assert b"mg_maze2d_policy_rollout_sampled" in lib.mg_last_error()
    assert call(policy=_lib.MazePolicyDesc(0, 5, 2, base, None)) == -1002 and b"n_policies" in lib.mg_last_error()
    assert call(policy=_lib.MazePolicyDesc(3, 0, 2, base, None)) == -1002 and b"hidden" in lib.mg_last_error()
    assert call(policy=_lib.MazePolicyDesc(3, 65, 2, base, None)) == -1002
    assert call(policy=_lib.MazePolicyDesc(3, 5, 1, base, None)) == -1003 and b"view_grid" in lib.mg_last_error()
    assert call(view_grid=4, policy=_lib.MazePolicyDesc(3, 5, 4, base, None)) == -1003
    assert call(view_grid=0, policy=_lib.MazePolicyDesc(3, 5, 0, base, None)) == -1003
    assert call(policy=_lib.MazePolicyDesc(3, 5, 2, base + 4, None)) == -1003 and b"aligned" in lib.mg_last_error()
    assert call(task_type=2) == -1003
