#!/usr/bin/env python3
"""An evolution-strategy search over learned LiftSim dispatchers, one launch per generation.

    python examples/liftsim_policy_search.py [--candidates 64] [--seeds 64] [--steps 600] [--generations 10] [--hidden 16]
                                             [--flow-file .../mansion_flow.npy]

P candidate dispatcher networks x V seeded buildings run `--steps` closed-loop steps inside ONE kernel launch
(`env.rollout_policy`): env e = p * V + v is the building seeded with `seed + v`, dispatched by candidate p. The fitness of
a candidate is its mean return over the V buildings; the mean of the best quarter becomes the next parent. Traffic is the
UNIFORM generator by default (no data file needed); `--flow-file` selects the reference's CUSTOM generator on its
mansion_flow.npy. The best candidate's mean return is printed beside that of the reference's rule dispatcher
(`rollout(policy="rule")`) on the same seeds: that is the baseline a learned dispatcher has to beat. With the defaults on an
MI355X the best candidate went from -9.60 in generation 0 (its random parent: -16.21) to -6.08 in generation 9, against -5.11
for the rule dispatcher: ten generations from random weights close most of the gap and do not beat the baseline.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ORDER = ("ws", "we", "wt", "wr", "wu", "wd", "b", "wo", "bo")


def main(argv=None):
    from metagym_amd.liftsim import LiftPolicy, LiftSim
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
    rs = np.random.RandomState(a.seed)
    parent = {k: (scale[k] * rs.standard_normal(s)).astype(np.float32) for k, s in shapes.items()}
    history = []
    for g in range(a.generations):
        cand = {k: (parent[k][None] + a.sigma * scale[k] * rs.standard_normal((P,) + shapes[k])).astype(np.float32)
                for k in shapes}
        for k in shapes:
            cand[k][0] = parent[k]                                  # candidate 0 is the parent
        env.seed(seeds=seeds)                                       # the same buildings in every generation
        out = env.rollout_policy(LiftPolicy(*[cand[k] for k in ORDER]), T, policy_ids=policy_ids)
        fitness = out["return"].view(P, V).mean(1).cpu().numpy()
        rank = np.argsort(-fitness)
        elite = rank[:max(1, P // 4)]
        frozen = int(env.overflow.sum()) + int(env.unsupported.sum())
        print("generation %2d: parent %.4f  best candidate %2d: %.4f  (rule dispatcher: %.4f; %d steps, %d buildings frozen)"
              % (g, fitness[0], rank[0], fitness[rank[0]], rule, T, frozen), flush=True)
        history.append((float(fitness[0]), float(fitness[rank[0]])))
        parent = {k: cand[k][elite].mean(0).astype(np.float32) for k in shapes}
    print("mean return over %d buildings and %d steps: best candidate %.4f, rule dispatcher %.4f"
          % (V, T, max(h[1] for h in history), rule))
    return dict(rule=rule, history=history)


if __name__ == "__main__":
    main()
