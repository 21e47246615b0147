"""`Bandits.rollout_policy` (mg_bandits_policy_rollout, csrc/bandits_policy.hip): closed-loop rollouts with per-env recurrent
policies inside the launch.
  1. the full closed-loop oracle: `BanditPolicy.reference` alternated with the reference's env (bandits_oracle.Env) on the
     host, every record, result, the end carry and the env state bit for bit; 2. replay identity through `rollout` for all
     three distributions; 3. staged and per-lane weight reads; 4. exploration; 5. splitting a rollout and record=False;
     6. episodic; 7. the over-env rule; 8. -0 and NaN in the carry; 9. hipGraph capture; 10. refused calls.
GPU box only (-m gpu)."""
import numpy as np
import pytest
import torch

import bandits_oracle as bo
from metagym_amd.bandits import BanditPolicy, BanditPolicyState
from metagym_amd.metamaze.policy import philox4x32_10

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
MEAN, DEVIATION = 0.45, 0.15
RECORDS = ("actions", "reward", "done", "info_steps", "expected_gain", "best_gain", "invalid")
RESULTS = ("ret_total", "ret_episode", "episode_len", "episodes", "regret")


def _np(t):
    return t.cpu().numpy()


def make_policy(P, H, K, seed, epsilon=None):
    """Random weights of order one: the clamp is hit on both sides and not always, the previous action, reward and done all
    move the state, and the logits are close enough for many arms to win somewhere."""
    rs = np.random.RandomState(seed)
    return BanditPolicy((1.5 * rs.randn(P, H, K)).astype(F), (1.5 * rs.randn(P, H)).astype(F), rs.randn(P, H).astype(F),
                        (rs.randn(P, H, H) * (2.0 / np.sqrt(H))).astype(F), (0.3 * rs.randn(P, H)).astype(F),
                        (rs.randn(P, K, H) / np.sqrt(H)).astype(F), (0.2 * rs.randn(P, K)).astype(F), epsilon)


class Host(object):
    """The host mirror of a batch: one numpy RandomState per env, gains, steps and over, as bandits_oracle.run keeps them."""

    def __init__(self, seeds, K, M, dist):
        self.K, self.M, self.dist = K, M, dist
        self.rss = bo.seeded(seeds)
        self.gains = np.stack([bo.sample_task(rs, K, dist, MEAN, DEVIATION) for rs in self.rss])
        self.steps = np.zeros(len(seeds), np.int64)
        self.over = np.ones(len(seeds), np.uint8)


def make_env(N, K, M, dist, auto_reset=True, resample=True, seed0=100, pre_steps=None, reset_mask=None):
    """A device batch and its host mirror in the same state: seeded, one task drawn and set, reset (the envs of `reset_mask`
    only), then advanced by pre_steps[e] valid steps each (a launch of max(pre_steps) steps in which env e's later actions
    are out of range and draw nothing), so the streams stand at different positions."""
    from metagym_amd.bandits import Bandits
    seeds = seed0 + 7 * np.arange(N)
    env = Bandits(num_envs=N, arms=K, max_steps=M, device=DEV, seeds=seeds, auto_reset=auto_reset,
                  resample_task=(dist, MEAN, DEVIATION) if resample else None)
    host = Host(seeds, K, M, dist)
    env.set_task(env.sample_task(dist, MEAN, DEVIATION))
    mask = np.ones(N, bool) if reset_mask is None else np.asarray(reset_mask, bool)
    env.reset(mask=torch.from_numpy(mask))
    host.over[mask] = 0
    if pre_steps is not None:
        pre = np.asarray(pre_steps)
        acts = np.random.RandomState(seed0 + 1).randint(0, K, size=(int(pre.max()), N)).astype(np.int32)
        acts[np.arange(acts.shape[0])[:, None] >= pre[None, :]] = K
        if acts.shape[0]:
            env.rollout(torch.from_numpy(acts))
            bo.run(host.rss, host.gains, host.steps, host.over, acts, K, M, auto_reset=auto_reset,
                   resample=dist if (auto_reset and resample) else None, mean=MEAN, dev=DEVIATION)
    return env, host


def host_rollout(pol, ids, host, state0, T, auto_reset, resample, seed=0, episodic=False):
    """The closed loop on the host: `BanditPolicy.reference` for the action, the reference's env for the step, per env.
    Advances `host` in place; returns (records dict of [T, N] arrays, results dict of [N] arrays, end carry, explored)."""
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

    def best_of(row):
        best = row[0]
        for v in row[1:]:
            if v > best:
                best = v
        return best
    best = [best_of(env.exp_gains) for env in envs]
    st = state0.numpy()
    st = BanditPolicyState(st.h.copy(), st.prev_action.copy(), st.prev_reward.copy(), st.prev_done.copy(), st.step)
    explored = np.zeros((T, N), bool)
    for t in range(T):
        acts, hn, ex = pol.reference(ids, st, seed=seed, return_explored=True)
        for e, env in enumerate(envs):
            if env.need_reset:                              # over: nothing happens, the records keep their defaults
                rec["info_steps"][t, e] = env.steps
                continue
            a = int(acts[e])
            explored[t, e] = ex[e]
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
            st.h[e], st.prev_action[e], st.prev_reward[e], st.prev_done[e] = hn[e], a, r, d
            if d and auto_reset:
                if resample:
                    env.set_task(env.sample_task(host.dist, MEAN, DEVIATION))
                    best[e] = best_of(env.exp_gains)
                env.reset()
                if episodic:
                    st.h[e], st.prev_action[e], st.prev_reward[e], st.prev_done[e] = 0, -1, 0, 0
        st.step += 1
    for e, env in enumerate(envs):
        host.gains[e], host.steps[e], host.over[e] = env.exp_gains, env.steps, env.need_reset
    return rec, out, st, explored


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    if a.dtype == np.float64:
        return a.shape == b.shape and b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


def check_against_host(res, env, rec, out, carry, host, what):
    for name in RECORDS:
        got, want = _np(getattr(res, name)), rec[name]
        assert same_bits(got, want.astype(got.dtype)), (what, name, "first difference at step %d"
                                                        % int(np.argmax((got != want).reshape(got.shape[0], -1).any(1))))
    for name in RESULTS:
        got = _np(getattr(res, name))
        assert same_bits(got, out[name].astype(got.dtype)), (what, name)
    same_carry(res.state, carry, what)
    assert same_bits(_np(env.gains), host.gains), (what, "gains")
    assert np.array_equal(_np(env.steps), host.steps) and np.array_equal(_np(env.over), host.over), (what, "steps / over")
    mt, hg, g = bo.stream_records(host.rss)
    assert np.array_equal(_np(env.mt).view(np.uint32), mt), (what, "stream")
    assert np.array_equal(_np(env.has_gauss), hg) and same_bits(_np(env.gauss), g)
    for e in sorted({0, len(host.rss) // 2, len(host.rss) - 1}):
        got, want = env.numpy_state(e), host.rss[e].get_state()
        assert np.array_equal(got[1], want[1]) and tuple(got[2:]) == tuple(want[2:]), (what, "numpy_state", e)


def same_carry(a, b, what, nan_ok=False):
    a, b = a.numpy(), b.numpy()
    if nan_ok:
        assert np.array_equal(np.isnan(a.h), np.isnan(b.h)), (what, "h NaN")
        keep = ~np.isnan(a.h)
        assert np.array_equal(a.h.view(np.uint32)[keep], b.h.view(np.uint32)[keep]), (what, "h")
    else:
        assert np.array_equal(a.h.view(np.uint32), b.h.view(np.uint32)), (what, "h")
    assert np.array_equal(a.prev_action, b.prev_action), (what, "prev_action")
    assert np.array_equal(a.prev_reward.view(np.uint32), b.prev_reward.view(np.uint32)), (what, "prev_reward")
    assert np.array_equal(a.prev_done, b.prev_done), (what, "prev_done")
    assert a.step == b.step, (what, "step")


def same_sd(sa, sb, what):
    assert sorted(sa) == sorted(sb)
    for key in sa:
        assert sa[key] == sb[key] if key == "has_task" else torch.equal(sa[key], sb[key]), (what, key)


def same_results(a, b, what, names=RECORDS + RESULTS):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        if x.dtype.is_floating_point:
            x, y = x.view(torch.int32 if x.dtype == torch.float32 else torch.int64), y.view(torch.int32 if y.dtype == torch.float32 else torch.int64)
        assert torch.equal(x, y), (what, name)


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dist", ["Classical", "Uniform"])
@pytest.mark.parametrize("K,H", [(2, 1), (3, 3), (10, 5), (64, 64)])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_full_closed_loop_oracle(N, K, H, dist):
    """max_steps = 7 and T = 330: 47 episodes end per env, each with a task draw from the env's own stream, and every
    stream crosses at least one refill (330 steps are 660 words of the 624 in a block), at a step that differs from lane to
    lane because env e took 37 e mod 300 steps before. Classical plays e mod 3 (mixed ids in a wave: per-lane weight reads),
    Uniform one id per wave (staged in LDS). Policies 0 and 2 explore."""
    M, T, P = 7, 330, 3
    pre = (37 * np.arange(N)) % 300
    env, host = make_env(N, K, M, dist, pre_steps=pre, seed0=1000 + N)
    pol = make_policy(P, H, K, 10 * K + H, epsilon=np.array([0.1, 0.0, 0.3]))
    ids = np.arange(N) % P if dist == "Classical" else (np.arange(N) // 64) % P
    pos0 = _np(env.mt).view(np.uint32)[:, 624].copy()
    state0 = BanditPolicyState.zeros(N, H, DEV)
    state0.step = (1 << 32) - 100                                            # the counter crosses 2^32 inside the rollout
    before = state0.clone()
    res = env.rollout_policy(pol, T, policy_ids=ids, state=state0, seed=(5 << 32) | 17, record=True)
    same_carry(state0, before, "the carry handed in is not written")
    assert res.state.step == state0.step + T and res.actions.shape == (T, N) and res.done.dtype == torch.bool
    rec, out, carry, explored = host_rollout(pol, ids, host, before, T, True, True, seed=(5 << 32) | 17)
    check_against_host(res, env, rec, out, carry, host, (N, K, H, dist))
    # the case does what it is for
    assert (rec["done"].sum(0) == T // M + ((pre % M + T % M) >= M)).all() and not rec["invalid"].any()
    assert len(set(pos0.tolist())) >= min(N, 20)                              # the refills fall on different steps
    assert (out["regret"] >= 0).all()
    used = np.bincount(rec["actions"].ravel(), minlength=K)
    print("arms used", int((used > 0).sum()), "of", K, "explored", int(explored.sum()), "of", explored.size,
          "mean regret per step %.4f" % (out["regret"].mean() / T))
    assert (used > 0).sum() >= 2 and (N == 1 or 0 < explored.sum() < explored.size)
    if N * H >= 300:                                                         # the clamp acts somewhere and not everywhere
        h = _np(res.state.h)
        assert (np.abs(h) == 1).any() and (np.abs(h) < 1).any()


# ---------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("dist", ["Classical", "Uniform", "Gaussian"])
def test_replay_identity_through_rollout(dist):
    """The recorded actions through `rollout` from the same state_dict give the same records and the same end state:
    the step is mg_bandits_step's. The only cover of Gaussian tasks (their gains may differ from numpy's by an ulp)."""
    N, K, H, M, T, P = 130, 10, 5, 7, 330, 4
    env, _ = make_env(N, K, M, dist, pre_steps=(53 * np.arange(N)) % 211)
    pol = make_policy(P, H, K, 21, epsilon=np.array([0.2, 0.0, 0.0, 1.0]))
    sd0 = env.state_dict()
    res = env.rollout_policy(pol, T, seed=3, record=True)
    sd1 = env.state_dict()
    env.load_state_dict(sd0)
    reward, done, info = env.rollout(res.actions)
    assert torch.equal(reward.view(torch.int32), res.reward.view(torch.int32)) and torch.equal(done, res.done)
    assert torch.equal(info["steps"], res.info_steps) and torch.equal(info["invalid"], res.invalid)
    assert torch.equal(info["expected_gain"].view(torch.int64), res.expected_gain.view(torch.int64))
    same_sd(env.state_dict(), sd1, dist)
    assert not bool(res.invalid.any()) and bool((res.episodes >= T // M).all())
    if dist == "Gaussian":
        assert len(torch.unique(res.best_gain)) > N                          # tasks were drawn in the launch
    # the results equal their definition computed from the records
    r, d = _np(res.reward).astype(np.float64), _np(res.done)
    total, epi, reg = np.zeros(N), np.zeros(N), np.zeros(N)
    length, ended = np.zeros(N, np.int32), np.zeros(N, bool)
    eg, bg = _np(res.expected_gain), _np(res.best_gain)
    for t in range(T):
        total = total + r[t]
        epi = np.where(ended, epi, epi + r[t])
        length = length + (~ended).astype(np.int32)
        ended = ended | d[t]
        reg = reg + (bg[t] - eg[t])
    assert same_bits(_np(res.ret_total), total) and same_bits(_np(res.ret_episode), epi) and same_bits(_np(res.regret), reg)
    assert np.array_equal(_np(res.episode_len), length) and np.array_equal(_np(res.episodes), d.sum(0).astype(np.int32))
    assert (bg >= eg).all()


# ---------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("K,H", [(10, 5), (64, 64)])
def test_staged_and_per_lane_weight_reads_agree(K, H):
    """The same (env stream, policy) pairs laid out one id per wave (the staged route) and interleaved (per-lane reads).
    Without exploration, whose counter holds the env's index."""
    N, T, P, M = 192, 40, 3, 7
    pol = make_policy(P, H, K, 14)
    e = np.arange(N)
    staged_ids = e // 64
    perm = (e % 3) * 64 + e // 3                       # interleaved position q holds the pair of staged position perm[q]
    mixed_ids = staged_ids[perm]
    assert all(len(set(staged_ids[w * 64:(w + 1) * 64])) == 1 for w in range(3))
    assert all(len(set(mixed_ids[w * 64:(w + 1) * 64])) == 3 for w in range(3))
    env_s, _ = make_env(N, K, M, "Uniform", pre_steps=(37 * e) % 300)
    sd = env_s.state_dict()
    p = torch.as_tensor(perm, device=DEV)
    env_m, _ = make_env(N, K, M, "Uniform")
    env_m.load_state_dict({k: (v if k == "has_task" else v[p]) for k, v in sd.items()})
    s = env_s.rollout_policy(pol, T, policy_ids=staged_ids, record=True)
    m = env_m.rollout_policy(pol, T, policy_ids=mixed_ids, record=True)
    for name in RECORDS:
        assert torch.equal(getattr(s, name)[:, p], getattr(m, name)), name
    for name in RESULTS:
        assert torch.equal(getattr(s, name)[p], getattr(m, name)), name
    assert torch.equal(s.state.h[p].view(torch.int32), m.state.h.view(torch.int32))
    assert torch.equal(s.state.prev_action[p], m.state.prev_action)
    same_sd({k: (v if k == "has_task" else v[p]) for k, v in env_s.state_dict().items()}, env_m.state_dict(), "layouts")
    assert len(set(_np(s.actions).ravel().tolist())) >= 3


# ---------------------------------------------------------------------------------------------------------- 4
def test_exploration():
    N, K, H, M, T, P = 130, 10, 5, 7, 40, 3
    seed, step0 = (9 << 32) | 4, (1 << 32) - 7
    weights = make_policy(P, H, K, 31)
    w = (weights.wa, weights.wr, weights.wd, weights.wh, weights.b, weights.wo, weights.bo)

    def run(epsilon):
        env, host = make_env(N, K, M, "Classical", pre_steps=(11 * np.arange(N)) % 50)
        st = BanditPolicyState.zeros(N, H, DEV)
        st.step = step0
        pol = BanditPolicy(*w, epsilon=epsilon)
        return env.rollout_policy(pol, T, state=st, seed=seed, record=True), env, host, pol, st
    # epsilon = 1: every action is out[1] % K (out[0] = 0xFFFFFFFF is the one value that would not explore)
    res, _, _, _, _ = run(np.ones(P))
    n = step0 + np.arange(T, dtype=np.uint64)[:, None]
    out = philox4x32_10(np.arange(N, dtype=np.uint64)[None, :], n & np.uint64(0xFFFFFFFF), n >> np.uint64(32), 0x4241, 4, 9)
    assert not (out[0] == 0xFFFFFFFF).any()
    assert np.array_equal(_np(res.actions), (out[1] % np.uint32(K)).astype(np.int32))
    assert sorted(set(_np(res.actions).ravel().tolist())) == list(range(K))
    # epsilon = 0 equals epsilon = None
    zero, env_z, _, _, _ = run(np.zeros(P))
    none, env_n, _, _, _ = run(None)
    same_results(zero, none, "epsilon = 0")
    same_carry(zero.state, none.state, "epsilon = 0")
    same_sd(env_z.state_dict(), env_n.state_dict(), "epsilon = 0")
    assert not torch.equal(zero.actions, res.actions)
    # in between: the explored mask is the reference's, and the whole loop the oracle's
    mid, env, host, pol, st = run(np.array([0.25, 0.0, 0.6]))
    ids = np.arange(N) % P
    rec, outs, carry, explored = host_rollout(pol, ids, host, st, T, True, True, seed=seed)
    check_against_host(mid, env, rec, outs, carry, host, "epsilon in between")
    assert np.array_equal(explored, out[0] < pol.thresholds[ids][None, :])
    assert not explored[:, ids == 1].any() and 0 < explored[:, ids == 0].sum() < explored[:, ids == 0].size
    differs = _np(mid.actions) != _np(none.actions)
    assert differs.any() and not differs[0, ~explored[0]].any()             # at step 0 only the explored envs differ
    other = run(np.array([0.25, 0.0, 0.6]))[0]
    same_results(other, mid, "the same seed")


# ---------------------------------------------------------------------------------------------------------- 5
def test_splitting_a_rollout_and_record_false():
    N, K, H, M, P = 65, 10, 5, 7, 3
    pol = make_policy(P, H, K, 12, epsilon=np.array([0.2, 0.0, 1.0]))
    env, _ = make_env(N, K, M, "Uniform", pre_steps=(37 * np.arange(N)) % 300)
    sd0 = env.state_dict()
    whole = env.rollout_policy(pol, 330, seed=9, record=True)
    sd_whole = env.state_dict()
    env.load_state_dict(sd0)
    a = env.rollout_policy(pol, 3, seed=9, record=True)
    b = env.rollout_policy(pol, 327, state=a.state, seed=9, record=True)
    for name in RECORDS:
        assert torch.equal(torch.cat([getattr(a, name), getattr(b, name)]), getattr(whole, name)), name
    same_sd(env.state_dict(), sd_whole, "split")
    same_carry(b.state, whole.state, "split")
    assert (a.state.step, b.state.step, whole.state.step) == (3, 330, 330)
    assert torch.equal(a.episodes + b.episodes, whole.episodes)
    assert torch.equal(a.ret_total + b.ret_total, whole.ret_total)          # sums of 0 / 1 rewards: exact in any order
    # record=False: the same results and end state, no records
    env.load_state_dict(sd0)
    lean = env.rollout_policy(pol, 330, seed=9)
    assert all(getattr(lean, name) is None for name in RECORDS)
    same_results(lean, whole, "record=False", RESULTS)
    same_sd(env.state_dict(), sd_whole, "record=False")
    same_carry(lean.state, whole.state, "record=False")


# ---------------------------------------------------------------------------------------------------------- 6
def test_episodic_clears_the_carry_at_a_done():
    N, K, H, M, T, P = 65, 10, 5, 7, 40, 3
    pol = make_policy(P, H, K, 13)
    ids = np.arange(N) % P
    env, host = make_env(N, K, M, "Classical", pre_steps=(3 * np.arange(N)) % 7)
    sd0 = env.state_dict()
    res = env.rollout_policy(pol, T, record=True, episodic=True)
    rec, out, carry, _ = host_rollout(pol, ids, host, BanditPolicyState.zeros(N, H), T, True, True, episodic=True)
    check_against_host(res, env, rec, out, carry, host, "episodic")
    assert bool((res.episodes >= 5).all())
    fresh = (_np(res.info_steps)[-1] == M - 1)                                # envs whose last step was a done: a fresh carry
    assert fresh.any() and not fresh.all()
    end = res.state.numpy()
    assert not end.h[fresh].any() and (end.prev_action[fresh] == -1).all() and not end.prev_done[fresh].any()
    assert (end.prev_action[~fresh] >= 0).all()
    # episodic=False keeps the memory: the step after a done sees prev_done = 1, and the actions part ways
    env.load_state_dict(sd0)
    env2, host2 = make_env(N, K, M, "Classical", pre_steps=(3 * np.arange(N)) % 7)
    trial = env.rollout_policy(pol, T, record=True)
    rec2, out2, carry2, _ = host_rollout(pol, ids, host2, BanditPolicyState.zeros(N, H), T, True, True)
    check_against_host(trial, env, rec2, out2, carry2, host2, "not episodic")
    assert not torch.equal(trial.actions, res.actions)
    first = int(_np(res.done).any(1).argmax())                               # up to the first done nothing differs
    assert torch.equal(trial.actions[:first + 1], res.actions[:first + 1])
    assert (trial.state.numpy().prev_done[fresh] == 1).all()
    # without auto_reset nothing restarts and the flag changes nothing
    x_env, _ = make_env(N, K, M, "Classical", auto_reset=False)
    y_env, _ = make_env(N, K, M, "Classical", auto_reset=False)
    x = x_env.rollout_policy(pol, T, record=True, episodic=True)
    y = y_env.rollout_policy(pol, T, record=True)
    same_results(x, y, "no auto_reset")
    same_carry(x.state, y.state, "no auto_reset")
    assert bool(x.done.any())


# ---------------------------------------------------------------------------------------------------------- 7
def test_envs_that_are_over_do_nothing():
    """Without auto_reset, max_steps = 7 and T = 12: every env that was reset finishes inside the launch (env e has taken
    e mod 5 steps before, so at step 6 - e mod 5) and is frozen from then on; envs 0, 3, 6, ... were never reset."""
    N, K, H, M, T, P = 130, 10, 5, 7, 12, 3
    pol = make_policy(P, H, K, 15, epsilon=np.array([0.3, 0.0, 0.3]))
    ids = np.arange(N) % P
    mask = np.arange(N) % 3 != 0
    pre = np.where(mask, np.arange(N) % 5, 0)
    env, host = make_env(N, K, M, "Uniform", auto_reset=False, pre_steps=pre, reset_mask=mask)
    rs = np.random.RandomState(1)
    st0 = BanditPolicyState(torch.as_tensor(rs.uniform(-1, 1, (N, H)).astype(F), device=DEV),
                            torch.as_tensor(rs.randint(-1, K, N).astype(np.int32), device=DEV),
                            torch.as_tensor(rs.randint(0, 2, N).astype(F), device=DEV),
                            torch.as_tensor(rs.randint(0, 2, N).astype(np.uint8), device=DEV), step=5)
    sd0 = env.state_dict()
    res = env.rollout_policy(pol, T, state=st0, seed=2, record=True)
    rec, out, carry, _ = host_rollout(pol, ids, host, st0, T, False, False, seed=2)
    check_against_host(res, env, rec, out, carry, host, "over")
    # the records of the steps an env did not take, as specified
    inv = _np(res.invalid)
    took = (np.arange(T)[:, None] < (M - pre)[None, :]) & mask[None, :]
    assert np.array_equal(inv, np.where(took, 0, 2).astype(np.uint8))
    idle = ~took
    assert (_np(res.actions)[idle] == -1).all() and not _np(res.reward)[idle].any() and not _np(res.done)[idle].any()
    assert not _np(res.expected_gain)[idle].any() and not _np(res.best_gain)[idle].any()
    assert (_np(res.info_steps)[idle] == np.broadcast_to(np.where(mask, M, 0), (T, N))[idle]).all()
    assert np.array_equal(_np(res.episodes), mask.astype(np.int32)) and np.array_equal(_np(res.episode_len), np.where(mask, M - pre, 0))
    assert np.array_equal(_np(env.over), np.ones(N, np.uint8))
    # an env that was never reset: nothing at all happened to it
    never = torch.as_tensor(~mask, device=DEV)
    sd1 = env.state_dict()
    for key in ("mt", "has_gauss", "gauss", "gains", "steps", "over"):
        assert torch.equal(sd1[key][never], sd0[key][never]), key
    end = res.state
    assert torch.equal(end.h[never].view(torch.int32), st0.h[never].view(torch.int32))
    assert torch.equal(end.prev_action[never], st0.prev_action[never]) and torch.equal(end.prev_done[never], st0.prev_done[never])
    for name in ("ret_total", "ret_episode", "regret"):
        assert not bool(getattr(res, name)[never].any()), name
    # a finished env is frozen: the launch that stops at the last done (T = 7) leaves the same carry and the same env
    env.load_state_dict(sd0)
    short = env.rollout_policy(pol, M, state=st0, seed=2, record=True)
    same_sd(env.state_dict(), sd1, "frozen")
    assert torch.equal(short.state.h.view(torch.int32), end.h.view(torch.int32))
    assert torch.equal(short.state.prev_action, end.prev_action) and torch.equal(short.state.prev_done, end.prev_done)
    assert torch.equal(short.state.prev_reward.view(torch.int32), end.prev_reward.view(torch.int32))
    same_results(short, res, "frozen", RESULTS)
    assert end.step == 5 + T and short.state.step == 5 + M                  # the counter advances whether or not an env stepped


# ---------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("H", [5, 3])
def test_negative_zero_and_nan_in_the_carry(H):
    """H = 5 (a whole quad, then v.x alone) and H = 3 (a partial quad alone, one padding float behind it).
    Policy 0 keeps a pre-activation of exactly -0 at a first step: b, wr and wd are -0, wh is +0 on a carry handed in as
    -0, and wa, all ones, is not looked up (no previous action). Policy 1 is ordinary; the envs 3 mod 4 hand it a NaN in
    h[0], which reaches every unit through wh and every logit through wo: arm 0. The NaN payload is not compared."""
    N, K, M = 130, 10, 7
    rnd = make_policy(2, H, K, 16)
    wa, wr, wd, wh, b, wo, bo = (v.copy() for v in (rnd.wa, rnd.wr, rnd.wd, rnd.wh, rnd.b, rnd.wo, rnd.bo))
    wa[0], wr[0], wd[0], wh[0], b[0] = 1.0, -0.0, -0.0, 0.0, -0.0
    pol = BanditPolicy(wa, wr, wd, wh, b, wo, bo)
    ids = (np.arange(N) % 2).astype(np.int32)
    h0 = np.random.RandomState(2).uniform(-1, 1, (N, H)).astype(F)
    h0[ids == 0] = -0.0
    nan_env = np.arange(N) % 4 == 3
    h0[nan_env, 0] = np.nan
    for T in (1, 3):
        env, host = make_env(N, K, M, "Classical", pre_steps=np.arange(N) % 3)
        st0 = BanditPolicyState.zeros(N, H, DEV)
        st0.h.copy_(torch.from_numpy(h0))
        assert bool(torch.signbit(st0.h[0]).all())
        res = env.rollout_policy(pol, T, policy_ids=ids, state=st0, record=True)
        rec, out, carry, _ = host_rollout(pol, ids, host, st0, T, True, True)
        h = _np(res.state.h)
        assert np.isnan(h[nan_env]).all() and np.isnan(carry.h[nan_env]).all()
        assert (_np(res.actions)[:, nan_env] == 0).all()
        for name in RECORDS:
            assert same_bits(_np(getattr(res, name)), rec[name].astype(_np(getattr(res, name)).dtype)), (T, name)
        same_carry(res.state, carry, T, nan_ok=True)
        if T == 1:
            assert (h[ids == 0].view(np.uint32) == 0x80000000).all()         # -0 after the step
        else:
            assert (h[ids == 0] == 1.0).all()                                # b + wa[j][prev_action] = -0 + 1


# ---------------------------------------------------------------------------------------------------------- 9
def test_graph_capture_of_one_call():
    """Captured once and replayed twice, the call equals two eager calls on a twin env (the end carry is copied back into the
    captured input inside the graph; without epsilon no argument depends on the step counter)."""
    from test_graph_capture_gpu import _capture
    N, K, H, M, T, P = 130, 10, 5, 7, 25, 3
    pol = make_policy(P, H, K, 17)
    pol.to(DEV)
    pre = (37 * np.arange(N)) % 300
    eager, _ = make_env(N, K, M, "Uniform", pre_steps=pre)
    env, _ = make_env(N, K, M, "Uniform", pre_steps=pre)
    static = BanditPolicyState.zeros(N, H, DEV)
    names = ("h", "prev_action", "prev_reward", "prev_done")
    out = {}

    def run():
        res = env.rollout_policy(pol, T, state=static, record=True)
        for name in names:
            getattr(static, name).copy_(getattr(res.state, name))
        out["res"] = res

    sd0 = env.state_dict()
    graph = _capture(run)
    env.load_state_dict(sd0)                                      # the warm-up and the capture pass advanced the state
    zero = BanditPolicyState.zeros(N, H, DEV)
    for name in names:
        getattr(static, name).copy_(getattr(zero, name))
    st = None
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        want = eager.rollout_policy(pol, T, state=st, record=True)
        st = want.state
        same_results(out["res"], want, rep)
        assert torch.equal(static.h.view(torch.int32), st.h.view(torch.int32)) and torch.equal(static.prev_action, st.prev_action)
        same_sd(env.state_dict(), eager.state_dict(), rep)
    assert bool(out["res"].done.any())


# ---------------------------------------------------------------------------------------------------------- 10
def test_refused_calls_raise_and_launch_nothing():
    N, K, H, M, P = 65, 10, 5, 7, 3
    pol = make_policy(P, H, K, 18)
    env, _ = make_env(N, K, M, "Classical")
    st = env.rollout_policy(pol, 5).state
    sd0, st0 = env.state_dict(), st.clone()
    bad_ids = np.arange(N) % P
    bad_ids[-1] = P
    neg_ids = np.arange(N) % P
    neg_ids[0] = -1
    refusals = [
        (ValueError, dict(policy_ids=bad_ids)),                                    # an id out of range
        (ValueError, dict(policy_ids=neg_ids)),
        (ValueError, dict(policy_ids=np.zeros(N - 1, int))),
        (ValueError, dict(policy_ids=np.zeros(N))),                                # not integers
        (ValueError, dict(policy=make_policy(P, H, K + 1, 18))),                   # a policy built for another K
        (ValueError, dict(state=BanditPolicyState.zeros(N - 1, H, DEV))),          # a carry of another N
        (ValueError, dict(state=BanditPolicyState.zeros(N, H + 1, DEV))),          # ... of another H
        (ValueError, dict(state=BanditPolicyState.zeros(N, H))),                   # ... on the host
        (ValueError, dict(steps=0)),
        (ValueError, dict(steps=-3)),
        (ValueError, dict(seed=-1)),
        (TypeError, dict(policy="greedy")),
        (TypeError, dict(state=(1, 2, 3))),
    ]
    for exc, kw in refusals:
        args = dict(policy=pol, steps=4, state=st)
        args.update(kw)
        with pytest.raises(exc):
            env.rollout_policy(**args)
        same_sd(env.state_dict(), sd0, kw)
        same_carry(st, st0, kw)
    # the env accepts any K; the policy's limit is its own
    from metagym_amd.bandits import Bandits
    wide = Bandits(num_envs=4, arms=65, max_steps=M, device=DEV)
    with pytest.raises(ValueError):
        wide.rollout_policy(pol, 3)
    # and the env still runs
    res = env.rollout_policy(pol, 4, state=st)
    assert res.state.step == 9


def test_a_device_policy_ids_tensor_is_kept_until_it_is_written():
    """The same device tensor, unchanged, is not read back on a repeated call and gives the same rollout; an in-place write
    is seen, validated again, and gives what a fresh env gives for that assignment as a host array."""
    N, P, H, T, K, M = 65, 2, 2, 4, 5, 7                              # one full wave and one ragged wave
    pol = make_policy(P, H, K, 31)
    env, _ = make_env(N, K, M, "Uniform")
    sd0 = env.state_dict()
    ids = torch.from_numpy((np.arange(N) % P).astype(np.int32)).to(DEV)
    first = env.rollout_policy(pol, T, policy_ids=ids, record=True)
    keep = env._policy_ids_keep
    assert keep[2] is ids and keep[3] == ids._version
    env.load_state_dict(sd0)
    again = env.rollout_policy(pol, T, policy_ids=ids, record=True)
    assert env._policy_ids_keep is keep                               # the fast path: nothing read back, nothing stored
    same_results(again, first, "the same tensor", RECORDS)
    other = ((np.arange(N) // 3 + 1) % P).astype(np.int32)
    ids.copy_(torch.from_numpy(other))
    env.load_state_dict(sd0)
    changed = env.rollout_policy(pol, T, policy_ids=ids, record=True)
    assert env._policy_ids_keep is not keep and env._policy_ids_keep[3] == ids._version
    fresh, _ = make_env(N, K, M, "Uniform")
    fresh.load_state_dict(sd0)
    want = fresh.rollout_policy(pol, T, policy_ids=other, record=True)
    same_results(changed, want, "in-place write", RECORDS)
    same_sd(env.state_dict(), fresh.state_dict(), "in-place write")
    same_carry(changed.state, want.state, "in-place write")
    assert not torch.equal(changed.actions, first.actions)            # the two assignments do play differently
