"""Times `MetaMaze2D.rollout_policy` (one launch, the recurrent policy inside it) against
  (a) `rollout(actions)` on precomputed actions: what the policy adds on top of the open loop;
  (b) the `step()` loop with the same recurrent policy in torch (a gather of the env's weights plus `bmm`, the clamp, the
      argmax), the host between every two steps.
Shapes: N = 4 096 and 2^20, 15 x 15 mazes, view_grid 2, T = 64, H = 16 and 64, one policy id per wave and mixed ids. HIP
events, one warm-up, one process. One JSON line per measurement into profiles/maze_policy/bench_maze_policy.jsonl; no time is
a pass/fail gate.

    python scripts/bench_maze_policy.py [--sizes 4096 1048576] [--hidden 16 64] [--steps 64] [--repeats 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import metagym_amd  # noqa: E402
from metagym_amd.metamaze import MAZE_TASK_MANAGER, MazePolicy  # noqa: E402
from metagym_amd.metamaze.policy import input_dim  # noqa: E402

DEV = "cuda:0"


def timed(fn, repeats):
    """Median milliseconds of `repeats` calls between HIP events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def torch_policy_loop(env, pol, ids, T):
    """The same policy with torch ops around step(): x from the returned window, a gather of each env's weights, bmm. (Not
    bit-identical to the definition: bmm chooses its own summation order. It is the baseline a user would write.)"""
    N, H = env.num_envs, pol.hidden
    idx = torch.as_tensor(ids, device=DEV).long()
    wx, wh, b = (torch.as_tensor(v, device=DEV)[idx] for v in (pol.wx, pol.wh, pol.b))
    wo, bo = torch.as_tensor(pol.wo, device=DEV)[idx], torch.as_tensor(pol.bo, device=DEV)[idx]
    eye = torch.eye(4, device=DEV)

    def run():
        h = torch.zeros(N, H, device=DEV)
        pa = torch.zeros(N, 4, device=DEV)
        pr, pd = torch.zeros(N, 1, device=DEV), torch.zeros(N, 1, device=DEV)
        obs = env._obs
        for _ in range(T):
            x = torch.cat([obs.reshape(N, -1), pa, pr, pd], 1)
            z = b + torch.bmm(wx, x.unsqueeze(2)).squeeze(2) + torch.bmm(wh, h.unsqueeze(2)).squeeze(2)
            h = z.clamp(-1.0, 1.0)
            act = (bo + torch.bmm(wo, h.unsqueeze(2)).squeeze(2)).argmax(1)
            obs, rew, done, _ = env.step(act)
            pa, pr, pd = eye[act], rew.unsqueeze(1), done.float().unsqueeze(1)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 1 << 20])
    ap.add_argument("--hidden", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--maze", type=int, default=15)
    ap.add_argument("--view-grid", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maze_policy", "bench_maze_policy.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    T, vg, P = args.steps, args.view_grid, 64
    D = input_dim(vg)
    table = MAZE_TASK_MANAGER.sample_tasks_device(64, device=DEV, seed=0, n=args.maze, allow_loops=True, step_reward=-0.01,
                                                  goal_reward=1.0)
    with open(args.out, "a") as out:
        for N in args.sizes:
            env = metagym_amd.make("meta-maze-2D-v0", num_envs=N, device=DEV, max_steps=50, task_type="ESCAPE", view_grid=vg,
                                   auto_reset=True)
            env.set_task(table)
            env.reset()
            actions = torch.randint(0, 4, (T, N), dtype=torch.int32, device=DEV)
            open_loop = timed(lambda: env.rollout(actions), args.repeats)
            for H in args.hidden:
                rs = np.random.RandomState(H)
                pol = MazePolicy((rs.randn(P, H, D) / np.sqrt(D)).astype(np.float32), (rs.randn(P, H, H) / np.sqrt(H)).astype(np.float32),
                                 (0.1 * rs.randn(P, H)).astype(np.float32), (rs.randn(P, 4, H) / np.sqrt(H)).astype(np.float32),
                                 (0.1 * rs.randn(P, 4)).astype(np.float32))
                for layout, ids in (("one_id_per_wave", (np.arange(N) // 64) % P), ("mixed_ids", np.arange(N) % P)):
                    closed = timed(lambda: env.rollout_policy(pol, T, policy_ids=ids), args.repeats)
                    loop = timed(torch_policy_loop(env, pol, ids, T), max(1, args.repeats // 2))
                    row = dict(bench="maze_policy", n_envs=N, maze=args.maze, view_grid=vg, steps=T, hidden=H, ids=layout,
                               rollout_policy_ms=closed, rollout_actions_ms=open_loop, step_loop_torch_ms=loop,
                               us_per_step_policy=1e3 * closed / T, us_per_step_actions=1e3 * open_loop / T,
                               us_per_step_loop=1e3 * loop / T)
                    print(json.dumps(row), flush=True)
                    out.write(json.dumps(row) + "\n")
            del env
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
