"""One hover controller, 256 airframes, one launch per step.

    python examples/quadrotor_domain_randomisation.py [--num-envs 4096] [--tasks 256] [--spread 0.2] [--steps 300]

`sample_tasks` draws the airframes (mass, inertia, thrust polynomial, drag and arm length within +-spread of the stock
one), `env.set_task(table)` gives env e airframe e % V, and the same PD altitude / attitude-rate controller flies all
of them. Prints the return per variant: how far one set of gains carries across the family."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metagym_amd  # noqa: E402
from metagym_amd.quadrotor import sample_tasks  # noqa: E402


def hover_controller(obs, hover_voltage=4.2):
    """Voltages [N, 4] from the observation: a common term holds altitude (z is obs[15], start height 5; vertical body
    velocity obs[2]), differential terms damp pitch / roll (obs[12], obs[13]) and the body rates (obs[9..11]).
    Propellers sit at (+,+), (-,+), (-,-), (+,-) in body x, y."""
    z_err, vz = 5.0 - obs[:, 15], obs[:, 2]
    common = hover_voltage + 1.5 * z_err - 1.0 * vz
    pitch, roll = obs[:, 12], obs[:, 13]
    tx = -2.0 * roll - 0.4 * obs[:, 9]        # torque about body x wanted
    ty = -2.0 * pitch - 0.4 * obs[:, 10]
    tz = -0.3 * obs[:, 11]
    sx = torch.tensor([1.0, -1.0, -1.0, 1.0], device=obs.device)
    sy = torch.tensor([1.0, 1.0, -1.0, -1.0], device=obs.device)
    sz = torch.tensor([-1.0, 1.0, -1.0, 1.0], device=obs.device)
    a = common[:, None] + tx[:, None] * sy[None] - ty[:, None] * sx[None] + tz[:, None] * sz[None]
    return a.clamp(0.1, 15.0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--tasks", type=int, default=256)
    ap.add_argument("--spread", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    env = metagym_amd.make("quadrotor-v0", num_envs=args.num_envs, device="cuda:0", task="hovering_control",
                           nt=args.steps, seed=args.seed)
    table = sample_tasks(args.tasks, seed=args.seed, spread=args.spread)
    env.set_task(table)
    obs = env.reset(seed=args.seed)
    ret = torch.zeros(args.num_envs, dtype=torch.float64, device=obs.device)
    alive = torch.ones(args.num_envs, dtype=torch.bool, device=obs.device)
    for _ in range(args.steps):
        obs, rew, done, info = env.step(hover_controller(obs))
        ret += torch.where(alive, env.reward64, torch.zeros_like(ret))
        alive &= ~done
    ids = env.task_ids.long()
    per_task = torch.zeros(len(table), dtype=torch.float64, device=obs.device).index_add_(0, ids, ret)
    count = torch.zeros(len(table), dtype=torch.float64, device=obs.device).index_add_(0, ids, torch.ones_like(ret))
    mean = (per_task / count.clamp(min=1)).cpu()
    order = torch.argsort(mean)
    print("return per variant over %d steps (mean of %d envs each): min %.1f  median %.1f  max %.1f"
          % (args.steps, args.num_envs // len(table), mean.min(), mean.median(), mean.max()))
    for v in list(order[:3]) + list(order[-3:]):
        c = table.configs[int(v)]
        print("  task %3d  return %9.2f  mass %.3f kg  arm %.3f m  CT0 %.3e" % (int(v), mean[int(v)], c["quality"],
                                                                                c["propeller"][0]["x"], c["thrust"]["CT"][0]))


if __name__ == "__main__":
    main()
