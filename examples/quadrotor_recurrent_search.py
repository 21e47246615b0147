"""Random search over recurrent hover policies on a sampled family of airframes, one launch per generation.

    python examples/quadrotor_recurrent_search.py [--candidates 64] [--tasks 16] [--episode-steps 100] [--episodes 3]
                                                  [--generations 10] [--hidden 8]

P candidate policies x V airframes from `sample_tasks` fly a whole trial inside ONE kernel launch (`env.rollout_policy`
with a `QuadrotorRecurrentPolicy`): env e = p * V + v flies candidate p on airframe v. A trial is `--episodes` episodes
back to back with the fused `auto_reset`; the policy's memory survives every done and it reads its previous action, reward
and done, so what it learns about its airframe in the first episode is still there in the last (the RL^2 setting). A
candidate's score is its return per episode, averaged over the airframes.

The recurrent parent embeds the PD controller of examples/quadrotor_policy_search.py: four hidden units hold the
controller's four voltage corrections scaled into (-1, 1), the output layer scales them back, and the remaining units start
at zero and are free to become memory. Beside it the same (1+lambda) search runs over linear policies with the same number of
launches and candidates, and both best scores are printed. Which of the two wins depends on the budget, the spread of the
family and the seed; this example makes no claim about it."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metagym_amd  # noqa: E402
from metagym_amd.quadrotor import QuadrotorPolicy, QuadrotorRecurrentPolicy, sample_tasks  # noqa: E402
from quadrotor_policy_search import pd_hover_weights  # noqa: E402

F = np.float32
NAMES = ("wx", "wa", "wr", "wd", "wh", "b", "wo", "bo")
SCALE = 0.1            # a voltage correction of +-10 V maps onto a hidden unit's (-1, 1)


def recurrent_parent(hidden):
    """One policy (no leading P axis) as a dict of arrays: units 0..3 carry SCALE * (w_pd x), the rest are zero."""
    if hidden < 4:
        raise SystemExit("--hidden must be at least 4: four units carry the PD controller")
    w, b = pd_hover_weights()
    p = dict(wx=np.zeros((hidden, 16), F), wa=np.zeros((hidden, 4), F), wr=np.zeros(hidden, F), wd=np.zeros(hidden, F),
             wh=np.zeros((hidden, hidden), F), b=np.zeros(hidden, F), wo=np.zeros((4, hidden), F), bo=b.copy())
    p["wx"][:4] = SCALE * w
    p["wo"][:, :4] = np.eye(4, dtype=F) / SCALE
    return p


def perturb(parent, P, sigma, rs):
    """P candidates around `parent` (a dict of arrays); candidate 0 is the parent itself, so the best never gets worse."""
    out = {}
    for k, v in parent.items():
        scale = np.abs(v) + 0.1 * max(float(np.abs(v).max()), 0.1)
        c = v[None] + sigma * scale * rs.standard_normal((P,) + v.shape)
        c[0] = v
        out[k] = c.astype(F)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--tasks", type=int, default=16)
    ap.add_argument("--spread", type=float, default=0.3)
    ap.add_argument("--episode-steps", type=int, default=100)
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    P, V, steps = args.candidates, args.tasks, args.episode_steps * args.episodes
    n = P * V
    policy_ids = np.arange(n) // V
    rs = np.random.RandomState(args.seed)

    v0, w0 = np.tile(rs.uniform(-1.0, 1.0, (V, 3)), (P, 1)), np.tile(rs.uniform(-2.0, 2.0, (V, 3)), (P, 1))

    def make_env():
        env = metagym_amd.make("quadrotor-v0", num_envs=n, device="cuda:0", task="hovering_control", nt=args.episode_steps,
                               auto_reset=True, seed=args.seed)
        env.set_task(sample_tasks(V, seed=args.seed, spread=args.spread), np.arange(n) % V)
        return env

    def search(name, parent, build):
        env = make_env()
        score = None
        for g in range(args.generations):
            cand = perturb(parent, P, args.sigma, rs)
            # every candidate meets the same V first starts (one per airframe); the later episodes of a trial start from
            # the fused reset's own draws, which differ from env to env
            env.reset(init_velocity=v0, init_angular_velocity=w0)
            res = env.rollout_policy(build(cand), steps, policy_ids)      # recurrent: from a fresh zero carry
            score = (res.ret_total.view(P, V).mean(1) / args.episodes).cpu().numpy()
            k = int(score.argmax())
            print("%-9s generation %2d: parent %9.2f  best candidate %2d: %9.2f" % (name, g, score[0], k, score[k]))
            parent = {key: v[k] for key, v in cand.items()}
        return float(score.max())

    w, b = pd_hover_weights()
    best_lin = search("linear", dict(w=w, b=b), lambda c: QuadrotorPolicy.linear(c["w"], c["b"]))
    best_rec = search("recurrent", recurrent_parent(args.hidden), lambda c: QuadrotorRecurrentPolicy(*[c[k] for k in NAMES]))
    print("mean return per episode over %d airframes, %d episodes per trial, %d generations x %d candidates each:"
          % (V, args.episodes, args.generations, P))
    print("  best linear policy            %9.2f" % best_lin)
    print("  best recurrent policy (H=%2d)  %9.2f" % (args.hidden, best_rec))


if __name__ == "__main__":
    main()
