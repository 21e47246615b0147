#!/usr/bin/env python3
"""The evolution-strategy search of liftsim_policy_search.py over recurrent LiftSim dispatchers.

    python examples/liftsim_recurrent_search.py [--candidates 64] [--seeds 64] [--steps 600] [--generations 10] [--hidden 16]
                                                [--flow-file .../mansion_flow.npy]

P candidate networks x V seeded buildings per launch (`env.rollout_policy` with a `LiftRecurrentPolicy`): env e = p * V + v
is the building seeded with `seed + v`, dispatched by candidate p, every elevator with a memory of its own. A trial is split
into two calls that share one `LiftPolicyState`: the second continues the first, memory included, as one call of `--steps`
steps would. The fitness of a candidate is its mean return over the V buildings; the mean of the best quarter becomes the
next parent. The best candidate is printed beside the reference's rule dispatcher and, at the same H and on the same seeds,
the feed-forward search of liftsim_policy_search.py (the same parent weights where the two networks share them).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MLP_ORDER = ("ws", "we", "wt", "wr", "wu", "wd", "b", "wo", "bo")
MEMORY = ("wc", "wq", "wh")


def search(env, seeds, policy_ids, make, shapes, scale, a, label):
    """`a.generations` ES generations of the networks `make(candidates)` builds; prints one line each under `label`.
    Returns [(parent's fitness, best candidate's fitness)]."""
    from metagym_amd.liftsim import LiftPolicyState, LiftRecurrentPolicy
    P, V, T = a.candidates, a.seeds, a.steps
    rs = np.random.RandomState(a.seed)
    parent = {k: (scale[k] * rs.standard_normal(shapes[k])).astype(np.float32) for k in MLP_ORDER}
    mrs = np.random.RandomState(a.seed + 1)                         # the memory weights draw from a stream of their own
    parent.update({k: (scale[k] * mrs.standard_normal(shapes[k])).astype(np.float32) for k in shapes if k in MEMORY})
    history = []
    for g in range(a.generations):
        cand = {}
        for k in shapes:
            draw = (mrs if k in MEMORY else rs).standard_normal((P,) + shapes[k])
            cand[k] = (parent[k][None] + a.sigma * scale[k] * draw).astype(np.float32)
            cand[k][0] = parent[k]                                  # candidate 0 is the parent
        env.seed(seeds=seeds)                                       # the same buildings in every generation
        policy = make(cand)
        if isinstance(policy, LiftRecurrentPolicy):                 # one trial, two launches, one carry
            state = LiftPolicyState.zeros(env.num_envs, env.E, policy.hidden, env.device)
            first = env.rollout_policy(policy, T // 2, policy_ids=policy_ids, state=state) if T > 1 else None
            second = env.rollout_policy(policy, T - T // 2, policy_ids=policy_ids, state=state)
            ret = second["return"] if first is None else first["return"] + second["return"]
        else:
            ret = env.rollout_policy(policy, T, policy_ids=policy_ids)["return"]
        fitness = ret.view(P, V).mean(1).cpu().numpy()
        rank = np.argsort(-fitness)
        elite = rank[:max(1, P // 4)]
        frozen = int(env.overflow.sum()) + int(env.unsupported.sum())
        print("%s %2d: parent %.4f  best candidate %2d: %.4f  (%d steps, %d buildings frozen)"
              % (label, g, fitness[0], rank[0], fitness[rank[0]], T, frozen), flush=True)
        history.append((float(fitness[0]), float(fitness[rank[0]])))
        parent = {k: cand[k][elite].mean(0).astype(np.float32) for k in shapes}
    return history


def main(argv=None):
    from metagym_amd.liftsim import LiftPolicy, LiftRecurrentPolicy, LiftSim
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--seeds", type=int, default=64, help="buildings per candidate; 64 fill a wave, whose policy is staged in LDS")
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--sigma", type=float, default=0.2)
    ap.add_argument("--flow-file", default=None, help="the reference's mansion_flow.npy: CUSTOM traffic instead of UNIFORM")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    P, V, H, T = a.candidates, a.seeds, a.hidden, a.steps
    kw = dict(flow_file=a.flow_file) if a.flow_file else dict(generator="UNIFORM", dt=1.0, generation_interval=15.0)
    seeds = np.tile(a.seed + np.arange(V), P)                       # every candidate meets the same V buildings
    env = LiftSim(num_envs=P * V, seeds=seeds, device=a.device, **kw)
    F, E = env.F, env.E
    A = 2 * F + 2
    import torch
    policy_ids = torch.as_tensor(np.arange(P * V) // V, dtype=torch.int32)

    base = LiftSim(num_envs=V, seeds=seeds[:V], device=a.device, **kw)
    rule = float(base.rollout(policy="rule", steps=T, record=())["return"].mean())

    shapes = dict(ws=(H, 8), we=(H, E), wt=(H, F + 1), wr=(H, F), wu=(H, F), wd=(H, F), b=(H,), wo=(A, H), bo=(A,))
    scale = dict(ws=1.0, we=0.3, wt=0.3, wr=0.3, wu=0.3, wd=0.3, b=0.1, wo=1.0 / np.sqrt(H), bo=0.1)
    rshapes = dict(shapes, wc=(H, A), wq=(H,), wh=(H, H))
    # rewards are of the order of 1e-2 per step: wq is scaled so that the term is of the order of the others
    rscale = dict(scale, wc=0.3, wq=30.0, wh=1.0 / np.sqrt(H))
    history = search(env, seeds, policy_ids, lambda c: LiftRecurrentPolicy(**c), rshapes, rscale, a, "generation")
    mlp = search(env, seeds, policy_ids, lambda c: LiftPolicy(*[c[k] for k in MLP_ORDER]), shapes, scale, a, "MLP search, round")
    print("mean return over %d buildings and %d steps: best recurrent candidate %.4f, best MLP candidate %.4f, rule dispatcher %.4f"
          % (V, T, max(h[1] for h in history), max(h[1] for h in mlp), rule))
    return dict(rule=rule, history=history, mlp_history=mlp)


if __name__ == "__main__":
    main()
