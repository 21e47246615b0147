"""(1+lambda) random search over recurrent MetaMaze policies, one launch per generation.

    python examples/maze_recurrent_search.py [--candidates 64] [--mazes 64] [--episodes 4] [--generations 10]

P candidate policies x V sampled mazes run a whole trial inside ONE kernel launch (`env.rollout_policy`): env e = p * V + v
plays candidate p on maze v for `--episodes` episodes of at most `--max-steps` steps each, with auto_reset and the policy's
memory kept across the episodes of the trial (the RL^2 setting: the maze is hidden, and what the agent learnt about it in one
episode shortens the next). The fitness of a candidate is the number of episodes it finishes inside the trial's step budget,
`episodes`, summed over the mazes: reaching the goal ends an episode early, so better policies finish more of them."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metagym_amd  # noqa: E402
from metagym_amd.metamaze import MAZE_TASK_MANAGER, MazePolicy  # noqa: E402
from metagym_amd.metamaze.policy import input_dim  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--mazes", type=int, default=64)
    ap.add_argument("--n", type=int, default=9, help="maze size")
    ap.add_argument("--view-grid", type=int, default=1)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--episodes", type=int, default=4, help="episodes per trial at the step budget")
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--epsilon", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    P, V, H, D = args.candidates, args.mazes, args.hidden, input_dim(args.view_grid)
    n_envs, steps = P * V, args.episodes * args.max_steps
    env = metagym_amd.make("meta-maze-2D-v0", num_envs=n_envs, device="cuda:0", max_steps=args.max_steps, task_type="ESCAPE",
                           view_grid=args.view_grid, auto_reset=True)
    table = MAZE_TASK_MANAGER.sample_tasks_device(V, device="cuda:0", seed=args.seed, n=args.n, allow_loops=True,
                                                  step_reward=-0.01, goal_reward=1.0)
    env.set_task(table, task_ids=np.arange(n_envs) % V)
    policy_ids = np.arange(n_envs) // V                  # V = 64: every wave holds one candidate, staged in LDS once
    rs = np.random.RandomState(args.seed)
    shapes = dict(wx=(H, D), wh=(H, H), b=(H,), wo=(4, H), bo=(4,))
    scale = dict(wx=1.0 / np.sqrt(D), wh=1.0 / np.sqrt(H), b=0.1, wo=1.0 / np.sqrt(H), bo=0.1)
    best = {k: (scale[k] * rs.standard_normal(s)).astype(np.float32) for k, s in shapes.items()}
    eps = np.full(P, args.epsilon)
    for g in range(args.generations):
        cand = {k: (best[k][None] + args.sigma * scale[k] * rs.standard_normal((P,) + shapes[k])).astype(np.float32)
                for k in shapes}
        for k in shapes:
            cand[k][0] = best[k]                         # candidate 0 is the parent: the best never gets worse
        env.reset()
        res = env.rollout_policy(MazePolicy(cand["wx"], cand["wh"], cand["b"], cand["wo"], cand["bo"], epsilon=eps), steps,
                                 policy_ids=policy_ids, seed=args.seed + g)
        score = res.episodes.view(P, V).double().mean(1).cpu().numpy()      # episodes finished per trial, mean over the mazes
        ret = res.ret_total.view(P, V).mean(1).cpu().numpy()
        k = int(np.lexsort((ret, score))[-1])            # most episodes; the trial's return breaks ties
        print("generation %2d: parent %.2f episodes  best candidate %d: %.2f episodes, return %.2f"
              % (g, score[0], k, score[k], ret[k]))
        best = {name: cand[name][k] for name in shapes}
    print("bo =", best["bo"])


if __name__ == "__main__":
    main()
