"""Greedy K-step lookahead on meta-maze-2D-v0 (ESCAPE) with `rollout()`: search by forking the batched state.

The batch holds 4^K replicas of every agent, env c * A + a = candidate c of agent a, all replicas of an agent in the same
state. Per decision:
  1. `state_dict()` — the fork point;
  2. ONE `rollout()` plays all 4^K action sequences of length K for all agents at once (obs_every = 0: nobody looks at the
     K - 1 observations in between);
  3. each agent picks the sequence with the best return up to its first `done` (ties broken at random — with K = 3 the
     goal is usually out of sight, and then every wall-free sequence looks the same);
  4. `load_state_dict()` puts every replica back on the fork point, and one `step()` plays the chosen first action in all
     replicas of the agent, which keeps them identical.

    python examples/maze_lookahead.py [--agents 8] [--depth 3] [--decisions 60] [--n 9]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def candidate_sequences(depth, device):
    """[depth, 4^depth] int32: column c spells c in base 4, first action in row 0."""
    c = torch.arange(4 ** depth, device=device)
    return torch.stack([(c // 4 ** (depth - 1 - t)) % 4 for t in range(depth)]).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=8)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--decisions", type=int, default=60)
    ap.add_argument("--n", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import metagym_amd
    from metagym_amd.metamaze import MAZE_TASK_MANAGER
    dev = "cuda:0"
    A, K, C = a.agents, a.depth, 4 ** a.depth
    table = MAZE_TASK_MANAGER.sample_tasks_device(A, device=dev, seed=a.seed, n=a.n, allow_loops=True, step_reward=-0.01,
                                                  goal_reward=1.0)
    env = metagym_amd.make("meta-maze-2D-v0", num_envs=C * A, device=dev, max_steps=a.decisions + K + 1, view_grid=1,
                           task_type="ESCAPE")
    agent_of = torch.arange(C * A, device=dev) % A
    env.set_task(table, task_ids=agent_of.to(torch.int32))           # every replica of agent a plays task a
    env.reset()
    cands = candidate_sequences(K, dev)                               # [K, C]
    plans = cands.repeat_interleave(A, dim=1)                         # [K, C * A]: env c * A + a plays sequence c
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    finished = torch.zeros(A, dtype=torch.bool, device=dev)
    total = torch.zeros(A, dtype=torch.float64, device=dev)
    reached = torch.zeros(A, dtype=torch.bool, device=dev)
    goal = table.tensors["goal"][:A]
    for it in range(a.decisions):
        fork = env.state_dict()                                       # 1
        _, _, done, _ = env.rollout(plans)                            # 2: [K, C * A] records, one launch
        r = env.rollout_reward64
        alive = torch.cat([torch.ones_like(done[:1]), ~done[:-1]]).cumprod(0).bool()    # steps up to the first done
        ret = (r * alive).sum(0).view(C, A)
        ret = ret + 1.0e-6 * torch.rand(C, A, generator=gen, device=dev, dtype=torch.float64)
        best = ret.argmax(0)                                          # 3: [A]
        env.load_state_dict(fork)                                     # 4
        first = cands[0, best]                                        # the chosen sequence's first action, per agent
        _, _, d, _ = env.step(first[agent_of])
        total += torch.where(finished, torch.zeros_like(total), env.reward64[:A])
        reached |= ~finished & (env.grid[:, :A].t() == goal).all(1)
        finished |= d[:A]                                             # (a finished agent is stepped on, and ignored)
        if bool(finished.all()):
            break
    print("decisions %d, lookahead depth %d (%d sequences per agent, %d envs per rollout)" % (it + 1, K, C, C * A))
    for i in range(A):
        print("agent %d: return %+.2f, %s" % (i, float(total[i]), "reached the goal" if bool(reached[i]) else "did not reach the goal"))


if __name__ == "__main__":
    main()
