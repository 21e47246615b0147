"""Evolution-strategy search over recurrent policies that read the rendered frame of the discrete 3-D maze.

    python examples/maze3d_visual_search.py [--candidates 32] [--mazes 32] [--generations 8]

P candidate `Maze3DPolicy`s x V sampled mazes run a whole trial inside one call of `env.rollout_policy`: env e = p * V + v
plays candidate p on maze v for `--episodes` episodes of at most `--max-steps` steps each on 64 x 64 uint8 frames, with
auto_reset and the policy's memory kept across the episodes of the trial (the RL^2 setting: the maze is hidden and the view is
partial). Every step is one render and one launch that pools the frame over an 8 x 8 grid and evaluates the env's candidate;
no frame ever visits the host. The fitness of a candidate is its trial return, averaged over the mazes; each generation moves
the mean of the search distribution along the rank-weighted candidates (antithetic pairs). The result is printed beside the
expert's return on the same mazes (`env.demonstrate`, the shortest way out) and beside uniform-random play."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metagym_amd  # noqa: E402
from metagym_amd.metamaze import MAZE_TASK_MANAGER, Maze3DPolicy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=32, help="P, even: antithetic pairs")
    ap.add_argument("--mazes", type=int, default=32)
    ap.add_argument("--n", type=int, default=9, help="maze size")
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--episodes", type=int, default=2, help="episodes per trial at the step budget")
    ap.add_argument("--max-steps", type=int, default=40)
    ap.add_argument("--generations", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=0.3)
    ap.add_argument("--lr", type=float, default=0.5)
    ap.add_argument("--epsilon", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    P, V, H, grid = args.candidates, args.mazes, args.hidden, (args.grid, args.grid)
    assert P % 2 == 0, "--candidates must be even"
    D = 3 * grid[0] * grid[1] + 6
    n_envs, steps = P * V, args.episodes * args.max_steps
    env = metagym_amd.make("meta-maze-discrete-3D-v0", num_envs=n_envs, device="cuda:0", max_steps=args.max_steps,
                           task_type="ESCAPE", auto_reset=True, resolution=(args.res, args.res), obs_dtype=torch.uint8)
    table = MAZE_TASK_MANAGER.sample_tasks_device(V, device="cuda:0", seed=args.seed, n=args.n, allow_loops=True,
                                                  step_reward=-0.01, goal_reward=1.0)
    env.set_task(table, task_ids=np.arange(n_envs) % V)
    policy_ids = np.arange(n_envs) // V
    rs = np.random.RandomState(args.seed)
    shapes = dict(wx=(H, D), wh=(H, H), b=(H,), wo=(4, H), bo=(4,))
    scale = dict(wx=1.0 / np.sqrt(D), wh=1.0 / np.sqrt(H), b=0.1, wo=1.0 / np.sqrt(H), bo=0.1)
    mean = {k: (scale[k] * rs.standard_normal(s)).astype(np.float32) for k, s in shapes.items()}
    eps = np.full(P, args.epsilon)

    def trial(cand, seed):
        env.reset()
        res = env.rollout_policy(Maze3DPolicy(cand["wx"], cand["wh"], cand["b"], cand["wo"], cand["bo"], grid=grid, epsilon=eps),
                                 steps, policy_ids=policy_ids, seed=seed)
        return res.ret_total.view(P, V).mean(1).cpu().numpy(), res.episodes.view(P, V).double().mean(1).cpu().numpy()

    # the yardsticks on the same mazes: the expert, and uniform-random play (exploration rate 1)
    env.reset()
    demo = env.demonstrate(steps)
    expert = float(demo.ret_total.mean())
    zero = {k: np.zeros((P,) + s, np.float32) for k, s in shapes.items()}
    env.reset()
    rand = env.rollout_policy(Maze3DPolicy(zero["wx"], zero["wh"], zero["b"], zero["wo"], zero["bo"], grid=grid, epsilon=np.ones(P)),
                              steps, policy_ids=policy_ids, seed=args.seed)
    random_ret = float(rand.ret_total.mean())
    print("%d candidates x %d mazes of n = %d, %d steps per trial, %d x %d uint8 frames pooled %d x %d, H = %d (%d parameters)"
          % (P, V, args.n, steps, args.res, args.res, grid[0], grid[1], H, sum(int(np.prod(s)) for s in shapes.values())))
    print("expert return %.3f (%.2f episodes)   uniform-random return %.3f (%.2f episodes)"
          % (expert, float(demo.episodes.double().mean()), random_ret, float(rand.episodes.double().mean())))
    weights = np.linspace(0.5, -0.5, P)                                  # rank weights, best first; they sum to zero
    for g in range(args.generations):
        half = {k: rs.standard_normal((P // 2,) + s).astype(np.float32) for k, s in shapes.items()}
        noise = {k: np.concatenate([half[k], -half[k]]) for k in shapes}
        cand = {k: (mean[k][None] + args.sigma * scale[k] * noise[k]).astype(np.float32) for k in shapes}
        ret, episodes = trial(cand, args.seed + 1 + g)
        order = np.argsort(-ret, kind="stable")
        w = np.empty(P)
        w[order] = weights
        for k in shapes:
            step = np.tensordot(w, noise[k], axes=(0, 0)) / (P / 4.0)
            mean[k] = (mean[k] + args.lr * args.sigma * scale[k] * step).astype(np.float32)
        print("generation %2d: return mean %.3f best %.3f (%.2f episodes)" % (g, ret.mean(), ret.max(), episodes[order[0]]))
    final, episodes = trial({k: np.repeat(mean[k][None], P, 0) for k in shapes}, args.seed + 1000)
    print("searched policy: return %.3f (%.2f episodes)   expert %.3f   uniform-random %.3f"
          % (final.mean(), episodes.mean(), expert, random_ret))


if __name__ == "__main__":
    main()
