"""`bench.py --dump-outputs DIR` on CPU: bench.dump_outputs writes the output buffers a caller of the timed env.step() holds
— here stand-ins with the product envs' attribute names, dtypes and shapes — as DIR/<name>.npy in float32 / float64, value for
value; beyond 64 MB in all it writes the same fixed seeded sample of env rows in every file."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _quadrotor(n, g):
    env = SimpleNamespace(_obs=torch.randn(n, 16, generator=g), _reward=torch.randn(n, generator=g),
                          reward64=torch.randn(n, generator=g, dtype=torch.float64), _done=torch.rand(n, generator=g) > 0.5,
                          _failed=(torch.rand(n, generator=g) > 0.9).to(torch.uint8), device=torch.device("cpu"))
    return SimpleNamespace(env=env, n=n)


def _maze(n, g, res=64):
    env = SimpleNamespace(_obs=torch.randint(0, 256, (n, res, res, 3), generator=g, dtype=torch.int32),
                          _reward=torch.randn(n, generator=g), reward64=torch.randn(n, generator=g, dtype=torch.float64),
                          _done=torch.rand(n, generator=g) > 0.5)
    return SimpleNamespace(env=env, n=n)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_output_whole_when_it_fits(tmp_path):
    import bench
    q = _quadrotor(65536, torch.Generator().manual_seed(1))
    rec = bench.dump_outputs(str(tmp_path), q)
    got = _load(str(tmp_path))
    assert sorted(got) == sorted(rec["files"]) == ["quadrotor_done", "quadrotor_failed", "quadrotor_obs", "quadrotor_reward",
                                                   "quadrotor_reward64"]
    assert rec["rows"] == "all"
    e = q.env
    for name, want in (("obs", e._obs), ("reward", e._reward), ("reward64", e.reward64), ("done", e._done), ("failed", e._failed)):
        a = got["quadrotor_" + name]
        assert a.dtype == (np.float64 if name == "reward64" else np.float32), name
        assert np.array_equal(a, want.numpy().astype(a.dtype)), name


def test_dump_samples_the_same_rows_everywhere_beyond_64_mb(tmp_path):
    import bench
    n = 4096                                    # 4096 maze frames of 64 x 64 x 3 float32 alone are 192 MB
    g = torch.Generator().manual_seed(2)
    q, m = _quadrotor(n, g), _maze(n, g)
    a, b = tmp_path / "a", tmp_path / "b"
    rec = bench.dump_outputs(str(a), q, m)
    assert bench.dump_outputs(str(b), q, m)["rows"] == rec["rows"]
    total = sum(os.path.getsize(os.path.join(str(a), f)) for f in os.listdir(str(a)))
    assert total <= (64 << 20) + 4096                # the .npy headers on top of the 64 MB of data
    k = rec["rows"]["sampled"]
    assert 0 < k < n
    got, again = _load(str(a)), _load(str(b))
    rows = np.sort(np.random.RandomState(rec["rows"]["seed"]).choice(n, k, replace=False))
    for name, want in (("quadrotor_obs", q.env._obs), ("quadrotor_reward64", q.env.reward64), ("quadrotor_done", q.env._done),
                       ("maze3d_obs", m.env._obs), ("maze3d_reward", m.env._reward), ("maze3d_done", m.env._done)):
        assert got[name].shape[0] == k
        assert np.array_equal(got[name], want.numpy()[rows].astype(got[name].dtype)), name
    for name in got:
        assert np.array_equal(got[name], again[name]), name
