"""Times `Bandits.rollout_learner` (one launch, a classical learner inside it) per env step of the whole batch, for each kind
(greedy with epsilon, UCB1, a Gittins table, Thompson sampling), against, in the same run,
  (a) `rollout_policy` with a recurrent policy of H = 32: the learned side the baselines stand beside;
  (b) the torch loop of examples/bandits_thompson.py (a Beta draw per env and arm, argmax, `step()`, the count update), the
      host between every two steps: the one classical learner the tree had.
Shapes: N = 4 096 and 65 536, K = 10, T = 256, max_steps = 100 with auto_reset and Classical tasks drawn in the launch, one
learner id per wave and mixed ids (P = 64 parameter rows). All timings of a size run on the same commit, the same GPU and in
the same process: one warm-up call, then the median of `--repeats` regions of `--inner` calls each, between two HIP events on
the current stream with the second one synchronised. One JSON line per measurement into
profiles/bandits/bench_bandits_learner.jsonl; no time is a pass/fail gate.

    python scripts/bench_bandits_learner.py [--sizes 4096 65536] [--arms 10] [--steps 256] [--repeats 7] [--inner 4]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metagym_amd.bandits import BanditLearner, BanditPolicy, Bandits, gittins_index_table  # noqa: E402

DEV = "cuda:0"


def timed(fn, repeats, inner):
    """Median milliseconds per call over `repeats` regions of `inner` calls between HIP events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return float(np.median(ms))


def torch_thompson_loop(env, T):
    """The loop of examples/bandits_thompson.py, T steps."""
    N, K = env.num_envs, env.K
    rows = torch.arange(N, device=DEV)

    def run():
        record = torch.ones(N, K, 2, dtype=torch.float64, device=DEV)
        for _ in range(T):
            idx = torch.distributions.Beta(record[..., 0], record[..., 1]).sample().argmax(dim=1)
            _, r, done, _ = env.step(idx.to(torch.int32))
            r = r.double()
            record[rows, idx, 0] += r
            record[rows, idx, 1] += 1.0 - r
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--arms", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bandits", "bench_bandits_learner.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    T, K, H, P = args.steps, args.arms, args.hidden, 64
    rs = np.random.RandomState(K)
    f = np.float32
    prior = (1.0 + rs.rand(P, 2)).astype(f)
    gittins = gittins_index_table(100, 0.95)
    learners = {
        "greedy": BanditLearner.greedy(K, prior, epsilon=np.full(P, 0.1)),
        "ucb": BanditLearner.ucb(K, (1.0 + rs.rand(P)).astype(f)),
        "table": BanditLearner.table(K, np.stack([gittins * f(1.0 - 0.001 * p) for p in range(P)]).astype(f)),
        "thompson": BanditLearner.thompson(K, prior),
    }
    pol = BanditPolicy(rs.randn(P, H, K).astype(f), rs.randn(P, H).astype(f), rs.randn(P, H).astype(f),
                       (rs.randn(P, H, H) / np.sqrt(H)).astype(f), (0.1 * rs.randn(P, H)).astype(f),
                       (rs.randn(P, K, H) / np.sqrt(H)).astype(f), (0.1 * rs.randn(P, K)).astype(f))
    with open(args.out, "a") as out:
        def emit(**row):
            row = dict(dict(bench="bandits_learner", gpu=torch.cuda.get_device_name(0), arms=K, steps=T, repeats=args.repeats,
                            inner=args.inner), **row)
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
        for N in args.sizes:
            env = Bandits(num_envs=N, arms=K, max_steps=100, device=DEV, seed=0, auto_reset=True, resample_task="Classical")
            env.set_task(env.sample_task("Classical"))
            env.reset()
            layouts = (("one_id_per_wave", (np.arange(N) // 64) % P), ("mixed_ids", np.arange(N) % P))
            for layout, ids in layouts:
                for kind, learner in learners.items():
                    ms = timed(lambda: env.rollout_learner(learner, T, learner_ids=ids), args.repeats, args.inner)
                    emit(what="rollout_learner", kind=kind, n_envs=N, ids=layout, ms=ms, us_per_step=1e3 * ms / T)
                ms = timed(lambda: env.rollout_policy(pol, T, policy_ids=ids), args.repeats, args.inner)
                emit(what="rollout_policy", hidden=H, n_envs=N, ids=layout, ms=ms, us_per_step=1e3 * ms / T)
            ms = timed(torch_thompson_loop(env, T), max(1, args.repeats // 2), 1)
            emit(what="torch_thompson_step_loop", n_envs=N, ms=ms, us_per_step=1e3 * ms / T)
            del env
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
