"""Random search over recurrent bandit learners, one launch per generation.

    python examples/bandits_recurrent_search.py [--candidates 64] [--tasks 64] [--arms 10] [--pulls 100] [--generations 10]

P candidate policies x V sampled Classical tasks run a whole trial inside ONE kernel launch (`env.rollout_policy`): env e =
p * V + v plays candidate p on task v for `--pulls` pulls with the policy's memory kept (the RL^2 setting: the good arm is
hidden, and what the agent saw of its rewards decides the next pull). The fitness of a candidate is its mean regret over the
tasks, the expected reward it gave away against always pulling the best arm; it is printed next to the mean regret of
uniform-random play (epsilon = 1) on the same tasks. examples/bandits_classical_baselines.py prints the mean regret of Thompson
sampling, UCB1, epsilon-greedy and the Gittins index on these tasks and seeds."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metagym_amd.bandits import BanditPolicy, Bandits  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--tasks", type=int, default=64)
    ap.add_argument("--arms", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--pulls", type=int, default=100)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=0.3)
    ap.add_argument("--epsilon", type=float, default=0.05)
    ap.add_argument("--dev", type=float, default=0.1, help="spread of a Classical task (mean 0.5)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    P, V, H, K, T = args.candidates, args.tasks, args.hidden, args.arms, args.pulls
    n_envs = P * V
    env = Bandits(num_envs=n_envs, arms=K, max_steps=T, device="cuda:0", seed=args.seed)
    tasks = env.sample_task("Classical", 0.5, args.dev)[:V]            # V tasks; every candidate meets the same ones
    env.set_task(tasks.repeat(P, 1))
    policy_ids = np.arange(n_envs) // V                  # V = 64: every wave holds one candidate, staged in LDS once
    rs = np.random.RandomState(args.seed)
    shapes = dict(wa=(H, K), wr=(H,), wd=(H,), wh=(H, H), b=(H,), wo=(K, H), bo=(K,))
    scale = dict(wa=1.0, wr=1.0, wd=0.1, wh=1.0 / np.sqrt(H), b=0.1, wo=1.0 / np.sqrt(H), bo=0.1)
    order = ("wa", "wr", "wd", "wh", "b", "wo", "bo")
    best = {k: (scale[k] * rs.standard_normal(s)).astype(np.float32) for k, s in shapes.items()}
    env.reset()
    zeros = [np.zeros((1,) + shapes[k], np.float32) for k in order]
    uniform = env.rollout_policy(BanditPolicy(*zeros, epsilon=np.ones(1)), T, seed=args.seed).regret.mean().item()
    eps = np.full(P, args.epsilon)
    for g in range(args.generations):
        cand = {k: (best[k][None] + args.sigma * scale[k] * rs.standard_normal((P,) + shapes[k])).astype(np.float32)
                for k in shapes}
        for k in shapes:
            cand[k][0] = best[k]                         # candidate 0 is the parent
        env.reset()
        res = env.rollout_policy(BanditPolicy(*[cand[k] for k in order], epsilon=eps), T, policy_ids=policy_ids,
                                 seed=args.seed + g)
        regret = res.regret.view(P, V).mean(1).cpu().numpy()            # mean over the tasks
        k = int(np.argmin(regret))
        print("generation %2d: parent %.2f  best candidate %d: regret %.2f  (uniform-random play: %.2f, over %d pulls)"
              % (g, regret[0], k, regret[k], uniform, T))
        best = {name: cand[name][k] for name in shapes}
    print("bo =", best["bo"])


if __name__ == "__main__":
    main()
