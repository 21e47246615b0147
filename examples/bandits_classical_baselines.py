"""The classical baselines of the bandit benchmark, each one launch: Thompson sampling, UCB1, epsilon-greedy and the Gittins
index, next to uniform-random play.

    python examples/bandits_classical_baselines.py [--tasks 4096] [--arms 10] [--pulls 100] [--dev 0.1] [--seed 0]

The tasks and seeds are those of examples/bandits_recurrent_search.py (Classical tasks of mean 0.5 drawn after
Bandits(seed=seed), `--pulls` pulls per trial), so the mean regret printed here is the yardstick for the regret a searched
recurrent learner reaches there. Every learner plays every task once (`env.rollout_learner`, the learner inside the kernel);
the regret is the expected reward given away against always pulling the best arm."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metagym_amd.bandits import BanditLearner, Bandits, gittins_index_table  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=4096)
    ap.add_argument("--arms", type=int, default=10)
    ap.add_argument("--pulls", type=int, default=100)
    ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--discount", type=float, default=0.95, help="of the Gittins index")
    ap.add_argument("--dev", type=float, default=0.1, help="spread of a Classical task (mean 0.5)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    V, K, T = args.tasks, args.arms, args.pulls
    env = Bandits(num_envs=V, arms=K, max_steps=T, device="cuda:0", seed=args.seed)
    env.set_task(env.sample_task("Classical", 0.5, args.dev))
    f = np.float32
    flat = np.ones((1, 2), f)
    learners = [
        ("Thompson sampling, Beta(1, 1)", BanditLearner.thompson(K, flat)),
        ("UCB1", BanditLearner.ucb(K, np.array([2.0], f))),
        ("epsilon-greedy, epsilon = %g" % args.epsilon, BanditLearner.greedy(K, flat, epsilon=np.array([args.epsilon]))),
        ("Gittins index, discount %g" % args.discount,
         BanditLearner.table(K, gittins_index_table(min(T, 1023), args.discount)[None, :])),
        ("uniform-random play", BanditLearner.greedy(K, flat, epsilon=np.ones(1))),
    ]
    for name, learner in learners:
        env.reset()
        res = env.rollout_learner(learner, T, seed=args.seed)
        print("%-32s mean regret %6.2f  mean return %6.2f  (over %d pulls, %d tasks)"
              % (name, res.regret.mean().item(), res.ret_total.mean().item(), T, V))


if __name__ == "__main__":
    main()
