"""Random search over recurrent ant policies on the TRAIN body variants, one launch per generation.

    python examples/walker_recurrent_search.py [--candidates 64] [--variants 16] [--episode-steps 64] [--episodes 3]
                                               [--generations 10] [--hidden 16]

P candidate policies x V TRAIN body variants run a whole trial inside ONE kernel launch (`env.rollout_policy` with a
`WalkerRecurrentPolicy`): env e runs candidate e // V on variant e % V. A trial is `--episodes` episodes back to back with
the fused `auto_reset`, through one carry: the policy's memory survives every done and it reads its previous action, reward
and done, so what it learns about its body in the first episode is still there in the last (the RL^2 setting; the observation
does not hold the body). A candidate is ranked by `ret_total`, the return of the whole trial, averaged over the variants; the
next generation is drawn around the best one. The sibling of examples/quadrotor_recurrent_search.py and the recurrent
counterpart of examples/walker_policy_search.py; a use case of the call, not a learning algorithm."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import metagym_amd.metalocomotion as ml  # noqa: E402

F = np.float32
NAMES = ("wx", "wa", "wr", "wd", "wh", "b", "wo", "bo")


def zero_parent(H, D, A):
    """One policy (no leading P axis) as a dict of arrays: the policy that does nothing and remembers nothing."""
    return dict(wx=np.zeros((H, D), F), wa=np.zeros((H, A), F), wr=np.zeros(H, F), wd=np.zeros(H, F), wh=np.zeros((H, H), F),
                b=np.zeros(H, F), wo=np.zeros((A, H), F), bo=np.zeros(A, F))


def perturb(parent, P, sigma, rs):
    """P candidates around `parent`; candidate 0 is the parent itself, so the incumbent stays in the race."""
    out = {}
    for k, v in parent.items():
        c = v[None] + sigma * rs.standard_normal((P,) + v.shape)
        c[0] = v
        out[k] = c.astype(F)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--variants", type=int, default=16)
    ap.add_argument("--episode-steps", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    P, V, H = args.candidates, args.variants, args.hidden
    steps = args.episode_steps * args.episodes             # an episode that ends early (the ant falls) leaves room for more
    env = ml.MetaAntEnv(num_envs=P * V, device=args.device, auto_reset=True, max_steps=args.episode_steps, seed=args.seed)
    env.set_task(env.tra_tasks[:V], task_ids=torch.arange(P * V, dtype=torch.int32) % V)
    ids = np.arange(P * V) // V
    D, A = env.obs_dim, env.n_joints
    rs = np.random.RandomState(args.seed)
    noise = rs.uniform(-0.1, 0.1, size=(V, A))             # one first start pose per variant, shared by the candidates
    parent = zero_parent(H, D, A)
    for gen in range(args.generations):
        cand = perturb(parent, P, args.sigma, rs)
        env.reset(joint_noise=np.tile(noise, (P, 1)))      # (the returned observation is the default obs0)
        res = env.rollout_policy(ml.WalkerRecurrentPolicy(*[cand[k] for k in NAMES]), steps, policy_ids=ids)     # state=None: a fresh carry
        score = res.ret_total.view(P, V).mean(1)
        k = int(score.argmax())
        parent = {key: v[k] for key, v in cand.items()}
        print("generation %2d  best candidate %3d: mean trial return %+.3f over %d variants (first episode %.1f steps, memory "
              "norm %.3f); incumbent %+.3f"
              % (gen, k, float(score[k]), V, float(res.episode_len.view(P, V)[k].float().mean()),
                 float(res.state.h.view(P, V, H)[k].norm(dim=1).mean()), float(score[0])))


if __name__ == "__main__":
    main()
