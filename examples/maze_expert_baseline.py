"""The optimum a searched MetaMaze policy can be measured against: the shortest-path expert beside uniform-random play.

    python examples/maze_expert_baseline.py [--mazes 64] [--n 9] [--episodes 4] [--max-steps 50] [--seed 0]

The V mazes are the ones `examples/maze_recurrent_search.py` samples for the same `--mazes`, `--n` and `--seed`, with the same
step budget (`--episodes` x `--max-steps` steps, auto_reset), so its printed returns and episode counts can be read against
these two lines. The expert knows the maze: `env.distance_field()` builds the goal's shortest-path field of every maze in one
launch and `env.rollout_expert()` descends it inside one more; nothing visits the host but the printed means."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metagym_amd  # noqa: E402
from metagym_amd.metamaze import MAZE_TASK_MANAGER  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mazes", type=int, default=64)
    ap.add_argument("--n", type=int, default=9, help="maze size")
    ap.add_argument("--view-grid", type=int, default=1)
    ap.add_argument("--episodes", type=int, default=4, help="episodes per trial at the step budget")
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    V, steps = args.mazes, args.episodes * args.max_steps
    env = metagym_amd.make("meta-maze-2D-v0", num_envs=V, device="cuda:0", max_steps=args.max_steps, task_type="ESCAPE",
                           view_grid=args.view_grid, auto_reset=True)
    table = MAZE_TASK_MANAGER.sample_tasks_device(V, device="cuda:0", seed=args.seed, n=args.n, allow_loops=True,
                                                  step_reward=-0.01, goal_reward=1.0)
    env.set_task(table, task_ids=np.arange(V))
    field = env.distance_field()
    start = table.tensors["start"].long()
    d = field.dist[torch.arange(V, device=field.device), 0, start[:, 0], start[:, 1]]
    print("%d mazes of n = %d: shortest path from start to goal %.1f steps on average (%d .. %d)"
          % (V, args.n, d.double().mean().item(), d.min().item(), d.max().item()))

    def line(name, res):
        print("%-8s return %7.3f per trial of %d steps, %5.2f episodes finished, first episode %5.1f steps"
              % (name, res.ret_total.mean().item(), steps, res.episodes.double().mean().item(),
                 res.episode_len.double().mean().item()))

    env.reset()
    line("expert", env.rollout_expert(steps))
    # uniform-random play: the same steps through rollout() on drawn actions
    env.reset()
    acts = torch.from_numpy(np.random.RandomState(args.seed).randint(0, 4, (steps, V)).astype(np.int32)).to("cuda:0")
    _, _, done, _ = env.rollout(acts)
    r64 = env.rollout_reward64
    ended = torch.cumsum(done.long(), 0) > 0
    first_len = torch.where(ended.any(0), ended.long().argmax(0) + 1, torch.full((V,), steps, device=done.device))
    print("%-8s return %7.3f per trial of %d steps, %5.2f episodes finished, first episode %5.1f steps"
          % ("random", r64.sum(0).mean().item(), steps, done.sum(0).double().mean().item(), first_len.double().mean().item()))


if __name__ == "__main__":
    main()
