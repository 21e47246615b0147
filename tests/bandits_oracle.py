"""Host restatement of the reference's Bandits (metagym/bandits/bandits_env.py), one numpy RandomState per env.

TEST INFRASTRUCTURE. `Env` is the reference class on a private stream instead of numpy.random's global one (same draws,
same exceptions); `sample_task` adds the Uniform and Gaussian distributions as the reference's docstring intends (its own
branches raise). `run` restates one mg_bandits_step launch for a batch: per-env outputs [T, N] and the state it leaves.
"""
import numpy as np

DISTRIBUTIONS = {"Classical": 1, "Uniform": 2, "Gaussian": 3}


def classical_lo_hi(K, mean, dev):
    """The two values of a Classical task, in the reference's f64 order, clipped."""
    fac = np.sqrt(K - 1)
    lo, hi = np.clip(np.array([mean - dev / fac, mean + fac * dev]), 0.0, 1.0)
    return float(lo), float(hi)


def sample_task(rs, K, distribution="Classical", mean=0.5, dev=0.05):
    if distribution == "Classical":
        fac = np.sqrt(K - 1)
        gains = np.full((K,), mean - dev / fac)
        gains[rs.randint(0, K - 1)] = mean + fac * dev
        return np.clip(gains, 0.0, 1.0)
    if distribution == "Uniform":
        return np.clip((rs.random_sample(K) - 0.50) * 3.464 + mean, 0.0, 1.0)
    if distribution == "Gaussian":
        return np.clip(rs.normal(loc=mean, scale=dev, size=K), 0.0, 1.0)
    raise Exception("No such distribution_settings: %s", distribution)


class Env(object):
    """The reference's Bandits with its draws taken from `rs`."""

    def __init__(self, rs, arms=10, max_steps=5000):
        self.rs = rs
        self.max_steps = max_steps
        self.exp_gains = None
        self.K = arms
        self.need_reset = True
        assert self.K > 1 and self.max_steps > 1

    def sample_task(self, distribution_settings="Classical", mean=0.50, dev=0.05):
        return sample_task(self.rs, self.K, distribution_settings, mean, dev)

    def set_task(self, task_config):
        self.exp_gains = task_config
        assert np.shape(self.exp_gains) == (self.K,)
        self.need_reset = True

    def reset(self):
        if self.exp_gains is None:
            raise Exception("Must call \"set_task\" before reset")
        self.steps = 0
        self.need_reset = False

    def step(self, action):
        if self.need_reset:
            raise Exception("Must \"reset\" before doing any actions")
        exp_gain = self.exp_gains[action]
        reward = 1 if self.rs.random_sample() < exp_gain else 0
        info = {"steps": self.steps, "expected_gain": exp_gain}
        self.steps += 1
        done = self.steps >= self.max_steps
        if done:
            self.need_reset = True
        return None, reward, done, info

    def expected_upperbound(self):
        return self.max_steps * np.max(self.exp_gains)


def seeded(seeds):
    return [np.random.RandomState(int(s)) for s in seeds]


def stream_records(rss):
    """[N, 625] u32 (key, pos), has_gauss [N] i32, gauss [N] f64: what mg_bandits_state holds for these streams."""
    mt = np.empty((len(rss), 625), np.uint32)
    hg = np.empty(len(rss), np.int32)
    g = np.empty(len(rss), np.float64)
    for e, rs in enumerate(rss):
        st = rs.get_state()
        mt[e, :624] = st[1]
        mt[e, 624] = st[2]
        hg[e] = st[3]
        g[e] = st[4]
    return mt, hg, g


def run(rss, gains, steps, over, actions, K, max_steps, auto_reset=False, resample=None, mean=0.5, dev=0.05,
        replay_gain=None):
    """One mg_bandits_step launch of T = len(actions) steps on N envs, in place on rss / gains [N, K] / steps / over.
    resample: None or a distribution name (the auto-reset task draw). replay_gain [T, N] (optional): decide each reward
    against this expected gain instead of the restated one (Gaussian: the device's gains may differ by an ulp).
    Returns reward f32, done u8, info_steps i32, expected_gain f64, invalid u8, each [T, N]."""
    actions = np.asarray(actions)
    T, N = actions.shape
    out = dict(reward=np.zeros((T, N), np.float32), done=np.zeros((T, N), np.uint8),
               info_steps=np.zeros((T, N), np.int32), expected_gain=np.zeros((T, N), np.float64),
               invalid=np.zeros((T, N), np.uint8))
    for e in range(N):
        rs = rss[e]
        t = 0
        while t < T:
            if over[e]:
                out["invalid"][t, e] = 2
                out["info_steps"][t, e] = steps[e]
                t += 1
                continue
            # the steps up to the end of this episode, or to the first out-of-range action, in one vectorised chunk
            m = min(T - t, max_steps - steps[e])
            a = actions[t:t + m, e].astype(np.int64)
            bad = np.nonzero((a < -K) | (a >= K))[0]
            if len(bad):
                m = int(bad[0])
                a = a[:m]
            if m > 0:
                d = rs.random_sample(m)
                g = gains[e][a]
                ref = g if replay_gain is None else replay_gain[t:t + m, e]
                out["reward"][t:t + m, e] = (d < ref).astype(np.float32)
                out["expected_gain"][t:t + m, e] = g
                out["info_steps"][t:t + m, e] = steps[e] + np.arange(m)
                steps[e] += m
                t += m
                if steps[e] >= max_steps:
                    out["done"][t - 1, e] = 1
                    over[e] = 1
                    if auto_reset:
                        if resample is not None:
                            gains[e] = sample_task(rs, K, resample, mean, dev)
                        steps[e] = 0
                        over[e] = 0
            if len(bad):                                   # t is at the bad action, inside the episode
                out["invalid"][t, e] = 1
                out["info_steps"][t, e] = steps[e]
                t += 1
    return out
