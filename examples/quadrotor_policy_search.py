"""(1+lambda) random search over linear hover policies, one launch per generation.

    python examples/quadrotor_policy_search.py [--candidates 64] [--tasks 16] [--steps 200] [--generations 10]

P candidate policies x V sampled airframes fly `--steps` closed-loop steps inside ONE kernel launch
(`env.rollout_policy`): env e = p * V + v flies candidate p on airframe v, and the launch hands back one return per env.
The starting point is the PD controller of examples/quadrotor_domain_randomisation.py written as a
`QuadrotorPolicy.linear`: it is linear in the observation apart from the clamp, and the step applies the clamp."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metagym_amd  # noqa: E402
from metagym_amd.quadrotor import QuadrotorPolicy, sample_tasks  # noqa: E402


def pd_hover_weights(hover_voltage=4.2):
    """(w [4, 16], b [4]) of hover_controller (quadrotor_domain_randomisation.py): a common term holds altitude
    (z is obs[15], start height 5; vertical body velocity obs[2]), differential terms damp pitch / roll (obs[12],
    obs[13]) and the body rates (obs[9..11]). Propellers sit at (+,+), (-,+), (-,-), (+,-) in body x, y."""
    sx, sy, sz = np.array([1.0, -1.0, -1.0, 1.0]), np.array([1.0, 1.0, -1.0, -1.0]), np.array([-1.0, 1.0, -1.0, 1.0])
    w = np.zeros((4, 16))
    w[:, 15], w[:, 2] = -1.5, -1.0                       # 1.5 * (5 - z) - vz
    w[:, 13], w[:, 9] = -2.0 * sy, -0.4 * sy             # torque about body x: -2 roll - 0.4 gyro_x
    w[:, 12], w[:, 10] = 2.0 * sx, 0.4 * sx              # minus the torque about body y
    w[:, 11] = -0.3 * sz
    b = np.full(4, hover_voltage + 1.5 * 5.0)
    return w.astype(np.float32), b.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--tasks", type=int, default=16)
    ap.add_argument("--spread", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    P, V = args.candidates, args.tasks
    n = P * V
    env = metagym_amd.make("quadrotor-v0", num_envs=n, device="cuda:0", task="hovering_control", nt=args.steps,
                           seed=args.seed)
    env.set_task(sample_tasks(V, seed=args.seed, spread=args.spread), np.arange(n) % V)
    policy_ids = np.arange(n) // V                       # a wave of 64 envs holds few candidates; V = 64 makes it one
    rs = np.random.RandomState(args.seed)
    # every candidate meets the same V starts (one per airframe), so scores compare policies and not start noise
    v0, w0 = np.tile(rs.uniform(-1.0, 1.0, (V, 3)), (P, 1)), np.tile(rs.uniform(-2.0, 2.0, (V, 3)), (P, 1))
    best_w, best_b = pd_hover_weights()
    scale_w, scale_b = np.abs(best_w) + 0.1, np.abs(best_b)
    for g in range(args.generations):
        w = best_w[None] + args.sigma * scale_w * rs.standard_normal((P, 4, 16)).astype(np.float32)
        b = best_b[None] + args.sigma * scale_b * rs.standard_normal((P, 4)).astype(np.float32)
        w[0], b[0] = best_w, best_b                      # candidate 0 is the parent: the best never gets worse
        env.reset(init_velocity=v0, init_angular_velocity=w0)
        res = env.rollout_policy(QuadrotorPolicy.linear(w.astype(np.float32), b.astype(np.float32)), args.steps, policy_ids)
        score = res.ret_episode.view(P, V).mean(1).cpu().numpy()     # mean over the airframes
        k = int(score.argmax())
        print("generation %2d: parent %.2f  best candidate %d: %.2f  (mean episode length %.1f)"
              % (g, score[0], k, score[k], float(res.episode_len.view(P, V)[k].double().mean())))
        best_w, best_b = w[k], b[k]
    print("b =", best_b)


if __name__ == "__main__":
    main()
