"""bandits-v0 on the MI355X: mg_bandits_* against the reference's episodes (tests/golden/bandits.npz) and the per-env
restatement (tests/bandits_oracle.py). Exact equality everywhere except Gaussian gains (and the gauss cache), which may
differ from numpy's by 2 ulp of 1.0 and the cached gauss value by 2 ulp (the device's
log); the draw counts behind them, and so the whole stream, are exact."""
import json
import os

import numpy as np
import pytest

import bandits_oracle as bo
from test_bandits import golden_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bandits.npz")
ULP = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _np(t):
    return t.cpu().numpy()


def _make(N, K, M, **kw):
    from metagym_amd.bandits import Bandits
    return Bandits(num_envs=N, arms=K, max_steps=M, device="cuda", **kw)


def _ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


def _close(dist, a, b):
    """Gaussian gains: within 2 ulp of 1.0, the top of their range (mean + dev * g cancels towards 0, so a relative bound on
    the gain itself would not follow from one on g)."""
    if dist == "Gaussian":
        return bool((np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) <= ULP * 2.0 ** -52).all())
    return np.array_equal(a, b)


def _streams_equal(env, rss, dist):
    mt, hg, g = bo.stream_records(rss)
    assert np.array_equal(_np(env.mt).view(np.uint32), mt)
    assert np.array_equal(_np(env.has_gauss), hg)
    assert (_ulps(_np(env.gauss), g) <= ULP).all()             # the cached gauss value itself: 2 ulp


def test_goldens_as_one_batch_seeded_with_the_golden_seeds(golden):
    seeds = [int(s) for s in golden["seeds"]]
    groups = {}
    for pre, s, K, mean, dev, M, E, dist in golden_cases(golden):
        groups.setdefault((K, mean, dev, M, E, dist), []).append((pre, s))
    for (K, mean, dev, M, E, dist), runs in groups.items():
        assert [s for _p, s in runs] == seeds
        env = _make(len(seeds), K, M, seeds=seeds)
        acts = np.stack([golden[p + "_actions"] for p, _s in runs], axis=2)     # [E, M, N]
        for ep in range(E):
            g = env.sample_task(dist, mean, dev)
            env.set_task(g)
            env.reset()
            for n, (p, _s) in enumerate(runs):
                assert _close(dist, _np(g)[n], golden[p + "_gains"][ep]), (p, ep)
                assert _close(dist, _np(env.expected_upperbound())[n], golden[p + "_upperbound"][ep])
            reward, done, info = env.rollout(acts[ep])
            for n, (p, _s) in enumerate(runs):
                assert np.array_equal(_np(reward)[:, n], golden[p + "_reward"][ep]), (p, ep)
                assert np.array_equal(_np(done)[:, n], golden[p + "_done"][ep].astype(bool)), (p, ep)
                assert np.array_equal(_np(info["steps"])[:, n], golden[p + "_info_steps"][ep])
                assert _close(dist, _np(info["expected_gain"])[:, n], golden[p + "_expected_gain"][ep])
                assert not _np(info["invalid"]).any()
        for n, (p, _s) in enumerate(runs):
            st = env.numpy_state(n)
            assert np.array_equal(st[1], golden[p + "_key"]) and st[2] == int(golden[p + "_pos"]), p
            assert st[3] == int(golden[p + "_has_gauss"]) and _ulps(st[4], float(golden[p + "_gauss"])) <= ULP, p
            rs = np.random.RandomState()
            rs.set_state(st)
            assert rs.random_sample() == float(golden[p + "_next_random"])


def test_goldens_at_one_env_through_step(golden):
    for pre, s, K, mean, dev, M, E, dist in golden_cases(golden):
        if s != 7:
            continue
        env = _make(1, K, M, seed=s)
        acts = golden[pre + "_actions"]
        for ep in range(E):
            env.set_task(env.sample_task(dist, mean, dev)[0])
            env.reset()
            for t in range(M):
                _, r, d, info = env.step(int(acts[ep, t]), check=True)
                assert float(r[0]) == golden[pre + "_reward"][ep, t] and bool(d[0]) == bool(golden[pre + "_done"][ep, t])
                assert int(info["steps"][0]) == golden[pre + "_info_steps"][ep, t]
        st = env.numpy_state(0)
        assert np.array_equal(st[1], golden[pre + "_key"]) and st[2] == int(golden[pre + "_pos"]), pre


@pytest.mark.parametrize("dist", ["Classical", "Uniform", "Gaussian"])
def test_4096_envs_auto_reset_with_resampling_against_the_oracle(dist):
    import torch
    N, K, M, T, mean, dev = 4096, 11, 7, 720, 0.45, 0.15
    seeds = np.random.RandomState(5).randint(0, 2 ** 32, size=N, dtype=np.int64)
    env = _make(N, K, M, seeds=seeds, auto_reset=True, resample_task=(dist, mean, dev))
    rss = bo.seeded(seeds)
    gains = np.stack([bo.sample_task(rs, K, dist, mean, dev) for rs in rss])
    env.set_task(env.sample_task(dist, mean, dev))
    assert _close(dist, _np(env.gains), gains)
    # stagger the streams: env e has drawn e % 300 extra doubles, so refills land at scattered steps
    for e, rs in enumerate(rss):
        rs.random_sample(e % 300)
        env.set_numpy_state(e, rs.get_state())
    env.reset()
    steps, over = np.zeros(N, np.int64), np.zeros(N, np.uint8)
    acts = np.random.RandomState(6).randint(-K, K, size=(T, N)).astype(np.int32)
    for t0, t1 in ((0, 1), (1, 300), (300, T)):
        reward, done, info = env.rollout(torch.from_numpy(acts[t0:t1]))
        eg = _np(info["expected_gain"])
        out = bo.run(rss, gains, steps, over, acts[t0:t1], K, M, auto_reset=True, resample=dist, mean=mean, dev=dev,
                     replay_gain=eg if dist == "Gaussian" else None)
        assert np.array_equal(_np(reward), out["reward"]), (dist, t0)
        assert np.array_equal(_np(done), out["done"].astype(bool))
        assert np.array_equal(_np(info["steps"]), out["info_steps"])
        assert not _np(info["invalid"]).any()
        assert _close(dist, eg, out["expected_gain"])
    assert np.array_equal(_np(env.steps), steps) and not _np(env.over).any()
    assert _close(dist, _np(env.gains), gains)
    _streams_equal(env, rss, dist)
    pos = _np(env.mt).view(np.uint32)[:, 624]
    assert len(np.unique(pos)) > 100


def test_rollout_equals_step_by_step():
    import torch
    N, K, M, T = 300, 6, 5, 40
    acts = torch.from_numpy(np.random.RandomState(2).randint(-K, K, size=(T, N)).astype(np.int32))
    envs = [_make(N, K, M, seed=17, auto_reset=True, resample_task="Gaussian") for _ in range(2)]
    for env in envs:
        env.set_task(env.sample_task("Uniform"))
        env.reset()
    reward, done, info = envs[0].rollout(acts)
    for t in range(T):
        _, r, d, inf = envs[1].step(acts[t])
        assert torch.equal(r, reward[t]) and torch.equal(d, done[t])
        for k in ("steps", "expected_gain", "invalid"):
            assert torch.equal(inf[k], info[k][t]), k
    a, b = envs[0].state_dict(), envs[1].state_dict()
    for k in ("mt", "has_gauss", "gauss", "gains", "steps", "over"):
        assert torch.equal(a[k], b[k]), k


def test_invalid_actions_and_finished_envs_draw_nothing():
    import torch
    N, K, M, T = 128, 5, 3, 12
    env = _make(N, K, M, seed=40)
    rss = bo.seeded(range(40, 40 + N))
    gains = np.stack([bo.sample_task(rs, K) for rs in rss])
    env.set_task(env.sample_task())
    mask = np.arange(N) % 3 != 0                               # envs 0, 3, ... are never reset: invalid 2 throughout
    env.reset(mask=torch.from_numpy(mask))
    acts = np.random.RandomState(3).randint(-K - 2, K + 2, size=(T, N)).astype(np.int32)
    steps, over = np.zeros(N, np.int64), (~mask).astype(np.uint8)
    reward, done, info = env.rollout(torch.from_numpy(acts))
    out = bo.run(rss, gains, steps, over, acts, K, M)
    inv = _np(info["invalid"])
    assert (inv == 1).any() and (inv == 2).any()
    assert np.array_equal(inv, out["invalid"])
    assert np.array_equal(_np(reward), out["reward"]) and np.array_equal(_np(done), out["done"].astype(bool))
    assert np.array_equal(_np(info["steps"]), out["info_steps"])
    assert np.array_equal(_np(info["expected_gain"]), out["expected_gain"])
    assert np.array_equal(_np(env.steps), steps) and np.array_equal(_np(env.over), over)
    _streams_equal(env, rss, "Classical")
    with pytest.raises(Exception, match="reset"):
        env.step(torch.zeros(N, dtype=torch.int32), check=True)
    fresh = _make(2, K, M, seed=0)
    with pytest.raises(Exception, match="set_task"):
        fresh.reset()
    fresh.set_task(fresh.sample_task())
    fresh.reset()
    with pytest.raises(IndexError):
        fresh.step(torch.tensor([0, K], dtype=torch.int32), check=True)
    with pytest.raises(Exception, match="No such distribution_settings"):
        fresh.sample_task("Beta")


def test_numpy_state_round_trip_at_every_block_edge():
    import torch
    K, M = 5, 6
    base = np.random.RandomState(99).get_state()
    positions = [0, 1, 622, 623, 624]
    env = _make(len(positions), K, M, seed=0)
    rss = []
    for e, p in enumerate(positions):
        st = ("MT19937", base[1], p, 1, 0.123456789 * (e + 1))
        env.set_numpy_state(e, st)
        got = env.numpy_state(e)
        assert np.array_equal(got[1], base[1]) and got[2:] == st[2:]
        rs = np.random.RandomState()
        rs.set_state(st)
        rss.append(rs)
    gains = np.stack([bo.sample_task(rs, K, "Gaussian", 0.5, 0.2) for rs in rss])
    env.set_task(env.sample_task("Gaussian", 0.5, 0.2))
    assert _close("Gaussian", _np(env.gains), gains)
    env.reset()
    acts = np.random.RandomState(4).randint(-K, K, size=(M, len(positions))).astype(np.int32)
    steps, over = np.zeros(len(positions), np.int64), np.zeros(len(positions), np.uint8)
    reward, done, info = env.rollout(torch.from_numpy(acts))
    out = bo.run(rss, gains, steps, over, acts, K, M, replay_gain=_np(info["expected_gain"]))
    assert np.array_equal(_np(reward), out["reward"]) and np.array_equal(_np(done), out["done"].astype(bool))
    _streams_equal(env, rss, "Gaussian")
    for e, rs in enumerate(rss):          # and back into numpy: the continuation is the same stream
        probe = np.random.RandomState()
        probe.set_state(env.numpy_state(e))
        assert probe.random_sample() == rs.random_sample()


def test_two_arms_and_uniform_tasks_that_span_refills():
    import torch
    env = _make(64, 2, 9, seed=123)                      # randint(0, 1): no draw
    rss = bo.seeded(range(123, 187))
    g = _np(env.sample_task("Classical", 0.5, 0.3))
    assert np.array_equal(g, np.stack([bo.sample_task(rs, 2, "Classical", 0.5, 0.3) for rs in rss]))
    _streams_equal(env, rss, "Classical")
    K = 5000                                             # 10000 draws per task: refills inside one task draw
    env = _make(64, K, 4, seed=321, auto_reset=True, resample_task="Uniform")
    rss = bo.seeded(range(321, 385))
    for rs in rss[::2]:
        rs.random_sample(311)
        rs.randint(0, 2 ** 31)                           # one word: pos 623, the first double straddles the refill
    for e in range(0, 64, 2):
        env.set_numpy_state(e, rss[e].get_state())
    gains = np.stack([bo.sample_task(rs, K, "Uniform", 0.5, 0.05) for rs in rss])
    env.set_task(env.sample_task("Uniform"))
    assert np.array_equal(_np(env.gains), gains)
    env.reset()
    acts = np.random.RandomState(8).randint(-K, K, size=(9, 64)).astype(np.int32)
    steps, over = np.zeros(64, np.int64), np.zeros(64, np.uint8)
    reward, done, info = env.rollout(torch.from_numpy(acts))
    out = bo.run(rss, gains, steps, over, acts, K, 4, auto_reset=True, resample="Uniform")
    assert np.array_equal(_np(reward), out["reward"]) and np.array_equal(_np(info["expected_gain"]), out["expected_gain"])
    assert np.array_equal(_np(env.gains), gains)
    _streams_equal(env, rss, "Uniform")


def test_graph_captured_steps_equal_eager_steps():
    import torch
    N, K, M = 1000, 8, 4
    acts = torch.from_numpy(np.random.RandomState(9).randint(-K, K, size=(16, N)).astype(np.int32)).cuda()
    eager = _make(N, K, M, seed=1000, auto_reset=True, resample_task="Classical")
    graphed = _make(N, K, M, seed=1000, auto_reset=True, resample_task="Classical")
    for env in (eager, graphed):
        env.set_task(env.sample_task())
        env.reset()
    static_a = acts[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _, r_g, d_g, info_g = graphed.step(static_a)
    torch.cuda.current_stream().wait_stream(s)
    for t in range(16):
        static_a.copy_(acts[t])
        g.replay()
        _, r, d, info = eager.step(acts[t])
        assert torch.equal(r_g, r) and torch.equal(d_g, d), t
        assert torch.equal(info_g["steps"], info["steps"]) and torch.equal(info_g["expected_gain"], info["expected_gain"])
    a, b = eager.state_dict(), graphed.state_dict()
    for k in ("mt", "gains", "steps", "over"):
        assert torch.equal(a[k], b[k]), k


def test_state_dict_round_trip():
    import torch
    N, K, M = 200, 7, 5
    env = _make(N, K, M, seed=3, auto_reset=True, resample_task=("Gaussian", 0.4, 0.3))
    env.set_task(env.sample_task("Gaussian", 0.4, 0.3))
    env.reset()
    acts = torch.from_numpy(np.random.RandomState(1).randint(0, K, size=(30, N)).astype(np.int32))
    env.rollout(acts[:13])
    sd = env.state_dict()
    first = env.rollout(acts[13:])
    other = _make(N, K, M, seed=999, auto_reset=True, resample_task=("Gaussian", 0.4, 0.3))
    other.load_state_dict(sd)
    second = other.rollout(acts[13:])
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    for k in ("steps", "expected_gain", "invalid"):
        assert torch.equal(first[2][k], second[2][k])
    assert torch.equal(env.mt, other.mt) and torch.equal(env.gauss, other.gauss)
