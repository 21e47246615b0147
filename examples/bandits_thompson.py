#!/usr/bin/env python3
"""Thompson sampling on a batch of bandits-v0 envs (the reference's demo_thompson_sampling.py, batched).

    python examples/bandits_thompson.py [--envs 4096] [--arms 10] [--tries 10]

Every env gets its own Classical task per try; the policy keeps a Beta(successes + 1, failures + 1) posterior per env and
arm and plays the arm with the largest posterior draw (torch.distributions.Beta, on the device). The env's draws are the
reference's, bit for bit; the policy's Beta draws are torch's, so the policy is not part of that claim.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import metagym_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--arms", type=int, default=10)
    ap.add_argument("--tries", type=int, default=10)
    a = ap.parse_args()
    N, K = a.envs, a.arms
    env = metagym_amd.make("bandits-v0", num_envs=N, arms=K, seed=0)
    rows = torch.arange(N, device=env.device)
    for i in range(a.tries):
        env.set_task(env.sample_task())
        env.reset()
        record = torch.ones(N, K, 2, dtype=torch.float64, device=env.device)
        total = torch.zeros(N, dtype=torch.float64, device=env.device)
        for _ in range(env.max_steps):
            idx = torch.distributions.Beta(record[..., 0], record[..., 1]).sample().argmax(dim=1)
            _, r, done, _ = env.step(idx.to(torch.int32))
            r = r.double()
            record[rows, idx, 0] += r
            record[rows, idx, 1] += 1.0 - r
            total += r
        bound = env.expected_upperbound()
        print("%d th try, Thompson Sampling gets %.2f on average over %d envs, expected upper bound %.2f"
              % (i, total.mean().item(), N, bound.mean().item()))


if __name__ == "__main__":
    main()
