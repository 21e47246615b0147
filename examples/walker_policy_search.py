"""Random search over linear policies on the ant with `rollout_policy`: P candidate policies x V TRAIN body variants in ONE
launch per generation (env e = candidate e // V on variant e % V), each candidate ranked by its mean episode return over the
variants; the next generation is drawn around the best one. The counterpart of examples/walker_shooting.py for closed-loop
control; a use case of the call, not a learning algorithm.

    python examples/walker_policy_search.py [--candidates 64] [--variants 16] [--steps 64] [--generations 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import metagym_amd.metalocomotion as ml  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--variants", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    P, V, T = args.candidates, args.variants, args.steps
    env = ml.MetaAntEnv(num_envs=P * V, device=args.device)        # no auto_reset: ret_episode is the one episode's return
    env.set_task(env.tra_tasks[:V], task_ids=torch.arange(P * V, dtype=torch.int32) % V)
    ids = np.arange(P * V) // V
    D, A = env.obs_dim, env.n_joints
    g = np.random.RandomState(0)
    noise = g.uniform(-0.1, 0.1, size=(V, A))                      # one start pose per variant, shared by the candidates
    best_w, best_b = np.zeros((A, D), np.float32), np.zeros(A, np.float32)
    for gen in range(args.generations):
        w = (best_w + args.sigma * g.standard_normal((P, A, D))).astype(np.float32)
        b = (best_b + args.sigma * g.standard_normal((P, A))).astype(np.float32)
        w[0], b[0] = best_w, best_b                                # the incumbent stays in the race
        env.reset(joint_noise=np.tile(noise, (P, 1)))              # (the returned observation is the default obs0)
        res = env.rollout_policy(ml.WalkerPolicy.linear(w, b), T, policy_ids=ids)
        score = res.ret_episode.view(P, V).mean(1)
        k = int(score.argmax())
        best_w, best_b = w[k], b[k]
        print("generation %2d  best candidate %3d: mean episode return %+.3f over %d variants (mean length %.1f); incumbent %+.3f"
              % (gen, k, float(score[k]), V, float(res.episode_len.view(P, V)[k].float().mean()), float(score[0])))


if __name__ == "__main__":
    main()
