"""Random-shooting control of one ant with `rollout`: fork the robot's state into N envs, play N random H-step action
sequences in ONE launch, take the first action of the best return, step the real robot, repeat. The counterpart of
examples/maze_lookahead.py for the walkers; a use case of the call, not a controller.

    python examples/walker_shooting.py [--candidates 512] [--horizon 8] [--steps 20]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import metagym_amd.metalocomotion as ml  # noqa: E402


def fork(sd, n):
    """Env 0 of a one-env state_dict, n times."""
    out = dict(sd)
    for k, v in sd.items():
        if torch.is_tensor(v) and v.dim() >= 1 and v.shape[-1] == 1:
            out[k] = v.expand(*v.shape[:-1], n).contiguous()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=512)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    N, H = args.candidates, args.horizon
    robot = ml.MetaAntEnv(num_envs=1, device=args.device)
    planner = ml.MetaAntEnv(num_envs=N, device=args.device)        # no auto_reset: a candidate that falls keeps its penalty
    task = robot.tra_tasks[0]
    robot.set_task(task)
    planner.set_task(task)
    robot.reset(seed=0)
    planner.reset(seed=0)
    gen = torch.Generator(device=args.device).manual_seed(0)
    total, random_total = 0.0, 0.0
    for t in range(args.steps):
        planner.load_state_dict(fork(robot.state_dict(), N))
        plans = torch.rand(H, N, planner.n_joints, generator=gen, device=args.device) * 2.0 - 1.0
        _obs, reward, done, _info = planner.rollout(plans)
        # return of a candidate: its rewards up to (and including) the step that ended its episode
        alive = torch.cat([torch.ones_like(done[:1]), (done[:-1].int().cummax(0).values == 0)]).float()
        returns = (reward * alive).sum(0)
        best = int(returns.argmax())
        _o, r, d, _i = robot.step(plans[0, best:best + 1])
        total += float(r)
        random_total += float(reward[0].mean())                    # what a random first action earns on average
        print("step %2d  best of %d plans: predicted return %+.3f, reward %+.3f (random action: %+.3f)  x = %.3f"
              % (t, N, float(returns[best]), float(r), float(reward[0].mean()), float(robot.pos[0, 0])))
        if bool(d):
            break
    print("return over %d steps: %.3f with shooting, %.3f expected from random actions" % (t + 1, total, random_total))


if __name__ == "__main__":
    main()
