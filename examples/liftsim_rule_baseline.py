#!/usr/bin/env python3
"""The reference's rule-based baseline on liftsim-v0 (its tests/rule_benchmark: Rule_dispatcher.run_dispacher), N buildings.

    python examples/liftsim_rule_baseline.py --flow-file .../mansion_flow.npy [--envs 4096] [--launches 48] [--seed 0]

A simulated day is 172 800 steps of 0.5 s. It runs as 48 `rollout(policy="rule", steps=3600)` launches: the dispatcher and
the step both run on the device, and nothing crosses to the host inside a launch. After every 3 600 steps (half an hour
of the day) it prints what the reference logs there: the accumulated reward (here the mean over the buildings, with the
best and the worst) and the 10-minute statistics (means). Building e is the reference's LiftSim after env.seed(seed + e),
bit for bit.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import metagym_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--flow-file", required=True, help="the reference's mansion_flow.npy (its CustomDataFile)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=48, help="launches of 3 600 steps; 48 are a day")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    env = metagym_amd.make("liftsim-v0", num_envs=a.envs, seed=a.seed, flow_file=a.flow_file)
    per_launch = 3600   # the reference logs every 3 600 steps
    total = 0.0
    for launch in range(a.launches):
        out = env.rollout(policy="rule", steps=per_launch, record=())
        acc = out["return"]                                  # [N], acc_reward of these 3 600 steps per building
        stats = {k: float(v.double().mean()) for k, v in env.statistics_tensors().items()}
        total += float(acc.mean())
        print("step %7d  Accumulated Reward: %f (best %f, worst %f), Mansion Status: %s"
              % ((launch + 1) * per_launch, float(acc.mean()), float(acc.max()), float(acc.min()), stats), flush=True)
    frozen = int(env.overflow.sum()) + int(env.unsupported.sum())
    print("%d buildings, %d steps each: mean return %f; %d buildings frozen by a flag" % (a.envs, a.launches * per_launch, total,
                                                                                        frozen))


if __name__ == "__main__":
    main()
