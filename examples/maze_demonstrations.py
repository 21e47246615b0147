"""A behaviour-cloning set from the 3-D mazes: first-person uint8 frames, each with the expert's action for it.

    python examples/maze_demonstrations.py [--mazes 256] [--n 9] [--steps 400] [--every 4] [--res 64] [--seed 0]

Both 3-D envs play sampled mazes with their expert inside the launches, `env.demonstrate(T, record=True, obs_every=k)`: the
discrete maze descends the TURNS shortest-path field cell by cell, the continuous maze steers towards the next cell of the
CELLS_3D field (`steer_action`). Only every k-th step is rendered. The frame kept after step t shows the state the action of
step t + 1 was chosen on, so frame t pairs with actions[t + 1]; the last frame's label is the expert's action on the end
state, and the reset frame pairs with actions[0]. The script prints the size of the set, the success rate and the steps to the
goal beside the shortest-path length dist[start]; nothing visits the host but the printed numbers."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metagym_amd  # noqa: E402
from metagym_amd.metamaze import MAZE_TASK_MANAGER  # noqa: E402

IDS = {"discrete": "meta-maze-discrete-3D-v0", "continuous": "meta-maze-continuous-3D-v0"}


def demonstrations(name, table, steps, every, res):
    """(frames uint8 [M, H, V, 3], actions [M] or [M, 2], the rollout's results) for one env family."""
    V = table.n_tasks
    env = metagym_amd.make(IDS[name], num_envs=V, device="cuda:0", max_steps=steps + 1, task_type="ESCAPE", auto_reset=True,
                           resolution=(res, res), obs_dtype=torch.uint8)
    env.set_task(table, task_ids=np.arange(V))
    first = env.reset().clone()
    expert = env.steer_action if name == "continuous" else env.expert_action
    out = env.demonstrate(steps, record=True, obs_every=every)
    kept = torch.as_tensor(out.obs_steps, device=out.actions.device)
    labels = torch.cat([out.actions[kept[:-1] + 1], expert().clone()[None]])             # frame of step t <-> action of step t + 1
    frames = torch.cat([first[None], out.obs]).flatten(0, 1)
    actions = torch.cat([out.actions[:1], labels]).flatten(0, 1)
    return env, frames, actions, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mazes", type=int, default=256)
    ap.add_argument("--n", type=int, default=9, help="maze size")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--every", type=int, default=4, help="keep the frame of every k-th step")
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    table = MAZE_TASK_MANAGER.sample_tasks_device(args.mazes, device="cuda:0", seed=args.seed, n=args.n, allow_loops=True,
                                                  step_reward=-0.01, goal_reward=1.0)
    start = table.tensors["start"].long()
    ids = torch.arange(args.mazes, device=start.device)
    for name in ("discrete", "continuous"):
        env, frames, actions, out = demonstrations(name, table, args.steps, args.every, args.res)
        d = env.distance_field().dist[ids, 0, start[:, 0], start[:, 1]].double()             # heading 0 at reset
        ok = out.episodes > 0
        print("%-10s %d frames %s %s with actions %s %s; %d mazes of n = %d, %d steps each, every %d-th frame kept"
              % (name, frames.shape[0], tuple(frames.shape[1:]), str(frames.dtype).replace("torch.", ""), tuple(actions.shape[1:]),
                 str(actions.dtype).replace("torch.", ""), args.mazes, args.n, args.steps, args.every))
        print("%-10s reached the goal in %5.1f %% of the mazes; first episode %6.1f steps on average beside dist[start] = %5.1f "
              "(%.2f steps per cell); %.2f episodes per maze, return %.3f"
              % ("", 100.0 * ok.double().mean().item(), out.episode_len[ok].double().mean().item(), d[ok].mean().item(),
                 (out.episode_len[ok].double() / d[ok]).mean().item(), out.episodes.double().mean().item(),
                 out.ret_total.mean().item()))


if __name__ == "__main__":
    main()
