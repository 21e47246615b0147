#!/usr/bin/env python3
"""Golden Bandits episodes run by the unmodified reference (metagym/bandits/bandits_env.py) -> tests/golden/bandits.npz.

TEST INFRASTRUCTURE; runs only where the reference tree is available (imported through oracle/refstubs, like the other
golden generators). Records, after numpy.random.seed(s) for s in SEEDS:
  - classical_<K>_<s>: E episodes of sample_task("Classical", mean, dev); set_task; reset; max_steps scripted steps
    (actions drawn from a private RandomState, negative indices included): gains, rewards, done, info, the global state
    left behind and the next numpy.random.random()
  - uniform_<s> / gaussian_<s>: the same with the task drawn by this repo's definition of the distribution (the
    reference's own branches raise), interleaved with the reference's steps; Gaussian at odd K so the cached gauss
    carries into the next task
  - errors: the exception each misuse raises in the reference
These pin tests/bandits_oracle.py (CPU) and mg_bandits_* (GPU) bit for bit.

    python scripts/gen_golden_bandits.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden  # noqa: E402  (reference import shims)

SEEDS = [0, 1, 7, 2 ** 32 - 1]
# (K, mean, dev, max_steps, episodes)
CLASSICAL = [
    (2, 0.5, 0.05, 5, 3),          # randint(0, 1) draws nothing
    (3, 0.95, 0.2, 2, 4),          # hi clips at 1
    (10, 0.02, 0.1, 400, 2),       # lo clips at 0; a refill lands mid-episode
    (50, 0.5, 0.05, 1000, 1),      # the registry's kwargs
    (1000, 0.3, 0.01, 7, 4),
]
DEFINED = {"Uniform": (10, 0.5, 0.05, 9, 5), "Gaussian": (3, 0.5, 0.2, 4, 6)}


def _actions(K, M, E, s):
    return np.random.RandomState(1000 + K + s % 97).randint(-K, K, size=(E, M)).astype(np.int32)


def _episodes(ref, K, M, E, s, draw):
    env = ref.Bandits(arms=K, max_steps=M)
    acts = _actions(K, M, E, s)
    rec = dict(gains=np.zeros((E, K)), reward=np.zeros((E, M), np.int32), done=np.zeros((E, M), np.uint8),
               info_steps=np.zeros((E, M), np.int32), expected_gain=np.zeros((E, M)), upperbound=np.zeros(E),
               actions=acts)
    for ep in range(E):
        g = draw(env)
        env.set_task(g)
        env.reset()
        rec["gains"][ep] = g
        rec["upperbound"][ep] = env.expected_upperbound()
        for t in range(M):
            _, r, d, info = env.step(int(acts[ep, t]))
            rec["reward"][ep, t] = r
            rec["done"][ep, t] = d
            rec["info_steps"][ep, t] = info["steps"]
            rec["expected_gain"][ep, t] = info["expected_gain"]
    st = np.random.get_state()
    rec.update(key=st[1], pos=np.int64(st[2]), has_gauss=np.int64(st[3]), gauss=np.float64(st[4]),
               next_random=np.float64(np.random.random()))
    return rec


def _raises(fn):
    try:
        fn()
    except BaseException as e:   # noqa: BLE001 — the class is what is recorded
        return type(e).__name__
    return "none"


def _errors(ref):
    out = {}
    np.random.seed(0)
    env = ref.Bandits(arms=4, max_steps=2)
    out["reset_before_set_task"] = _raises(env.reset)
    out["uniform"] = _raises(lambda: env.sample_task("Uniform"))
    out["gaussian_set_task"] = _raises(lambda: env.set_task(env.sample_task("Gaussian")))
    out["unknown"] = _raises(lambda: env.sample_task("Beta"))
    env.set_task(env.sample_task())
    out["step_before_reset"] = _raises(lambda: env.step(0))
    env.reset()
    out["action_k"] = _raises(lambda: env.step(4))
    out["action_minus_k_minus_1"] = _raises(lambda: env.step(-5))
    env.step(-4)
    env.step(3)
    out["step_after_done"] = _raises(lambda: env.step(0))
    out["arms_1"] = _raises(lambda: ref.Bandits(arms=1))
    out["max_steps_1"] = _raises(lambda: ref.Bandits(max_steps=1))
    return out


def main():
    gen_golden._import_reference()
    import metagym.bandits as ref
    out = {"numpy_version": np.str_(np.__version__)}
    for K, mean, dev, M, E in CLASSICAL:
        for s in SEEDS:
            np.random.seed(s)
            rec = _episodes(ref, K, M, E, s, lambda env: env.sample_task("Classical", mean, dev))
            for k, v in rec.items():
                out["classical_%d_%d_%s" % (K, s, k)] = v
    for name, (K, mean, dev, M, E) in DEFINED.items():
        if name == "Uniform":
            draw = lambda env: np.clip((np.random.random_sample(K) - 0.50) * 3.464 + mean, 0.0, 1.0)   # noqa: E731
        else:
            draw = lambda env: np.clip(np.random.normal(loc=mean, scale=dev, size=K), 0.0, 1.0)     # noqa: E731
        for s in SEEDS:
            np.random.seed(s)
            rec = _episodes(ref, K, M, E, s, draw)
            for k, v in rec.items():
                out["%s_%d_%s" % (name.lower(), s, k)] = v
    out["seeds"] = np.asarray(SEEDS, np.int64)
    out["classical"] = np.str_(json.dumps(CLASSICAL))
    out["defined"] = np.str_(json.dumps(DEFINED))
    out["errors"] = np.str_(json.dumps(_errors(ref)))
    from gym.envs.registration import _REGISTRY      # the stub keeps (entry_point, kwargs) per id
    out["registry"] = np.str_(json.dumps(_REGISTRY["bandits-v0"]))
    dst = os.path.join(ROOT, "tests", "golden", "bandits.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
