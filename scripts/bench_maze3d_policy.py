"""Times closed-loop rollouts of the discrete 3-D maze with the policy inside the launches (csrc/maze3d_policy.hip
mg_maze3d_policy_rollout, `env.rollout_policy`): `steps` env steps, every frame rendered and read by a `Maze3DPolicy`, beside
  (a) the `step()` loop it replaces with the same policy in torch (pooling by a reshaped sum, the P policies as one `bmm` over
      the envs sorted by policy id, clamp, argmax; float32, not bit-exact, same work), and
  (b) the open loop `env.rollout(actions, obs_every=1)` on the actions the closed loop recorded: renderer plus advance, no
      policy. That is the floor.
for N = 4 096 and 65 536 envs, 64 x 64 uint8 and int32 frames, n = 15, T = 32, grid 8 x 8, H = 32, P = 16 policies with one id
per workgroup (ids = (e // 4) % P) and mixed ids (e % P). The method is scripts/bench_maze_demo.py's: one process; every variant
is warmed up once per shape; a window is enough calls for about 0.1 s between two HIP events; the variants alternate inside
every repeat and the median of `--repeats` windows is reported with their min and max; the env is reset before every window.
One JSON line per (N, dtype, ids) into profiles/maze/bench_maze3d_policy.jsonl; no time is a pass/fail gate.

    python scripts/bench_maze3d_policy.py [--sizes 4096 65536] [--dtypes uint8 int32] [--steps 32] [--res 64] [--repeats 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import metagym_amd  # noqa: E402
from bench_maze_demo import DEV, compare  # noqa: E402
from metagym_amd.metamaze import MAZE_TASK_MANAGER, Maze3DPolicy  # noqa: E402
from metagym_amd.metamaze.policy import pool_scale  # noqa: E402


def random_policy(P, H, grid, seed):
    rs = np.random.RandomState(seed)
    D = 3 * grid[0] * grid[1] + 6
    u = lambda scale, *s: (rs.uniform(-1, 1, s) * scale).astype(np.float32)
    return Maze3DPolicy(u(3.0 / np.sqrt(D), P, H, D), u(0.5, P, H, H), u(0.3, P, H), u(1.0, P, 4, H), u(0.3, P, 4), grid=grid)


class TorchPolicy(object):
    """The same network in torch for the `step()` loop: the envs sorted by policy id, one bmm per layer."""

    def __init__(self, pol, ids, res, device):
        t = lambda a: torch.as_tensor(a, device=device)
        self.P, self.H, self.grid = pol.num_policies, pol.hidden, pol.grid
        self.bh, self.bv = res // pol.grid[0], res // pol.grid[1]
        self.scale = float(pool_scale(self.bh, self.bv))
        self.w = t(np.concatenate([pol.wx, pol.wh], axis=2).transpose(0, 2, 1).copy())      # [P, D + H, H]
        self.b, self.wo, self.bo = t(pol.b)[:, None, :], t(pol.wo.transpose(0, 2, 1).copy()), t(pol.bo)[:, None, :]
        order = np.argsort(ids, kind="stable")
        assert (np.bincount(ids, minlength=self.P) == len(ids) // self.P).all()
        self.order, self.back = t(order), t(np.argsort(order))
        N = len(ids)
        self.h = torch.zeros(N, self.H, device=device)
        self.prev = torch.zeros(N, 6, device=device)

    def act(self, frame, reward, done):
        N, (gh, gv) = frame.shape[0], self.grid
        feat = frame.view(N, gh, self.bh, gv, self.bv, 3).sum(dim=(2, 4), dtype=torch.int32).to(torch.float32).view(N, -1) * self.scale
        x = torch.cat([feat, self.prev, self.h], dim=1)[self.order].view(self.P, N // self.P, -1)
        hn = (torch.bmm(x, self.w) + self.b).clamp_(-1.0, 1.0)
        a = (torch.bmm(hn, self.wo) + self.bo).argmax(dim=2).view(N)[self.back]
        self.h = hn.view(N, self.H)[self.back]
        self.prev[:, :4] = torch.nn.functional.one_hot(a, 4).to(torch.float32)
        return a.to(torch.int32)

    def seen(self, reward, done):
        self.prev[:, 4] = reward
        self.prev[:, 5] = done.to(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--dtypes", nargs="+", default=["uint8", "int32"], choices=["uint8", "int32"])
    ap.add_argument("--ids", nargs="+", default=["workgroup", "mixed"], choices=["workgroup", "mixed"])
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--policies", type=int, default=16)
    ap.add_argument("--maze", type=int, default=15)
    ap.add_argument("--tasks", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maze", "bench_maze3d_policy.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_maze3d_policy.py measures on the GPU; there is nothing to time without one"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    T, P, grid = args.steps, args.policies, (args.grid, args.grid)
    pol = random_policy(P, args.hidden, grid, 0)
    table = MAZE_TASK_MANAGER.sample_tasks_device(args.tasks, device=DEV, seed=0, n=args.maze, allow_loops=True, step_reward=-0.01,
                                                  goal_reward=1.0)
    with open(args.out, "a") as out:
        for N in args.sizes:
            for dt in args.dtypes:
                env = metagym_amd.make("meta-maze-discrete-3D-v0", num_envs=N, device=DEV, max_steps=200, task_type="ESCAPE",
                                       auto_reset=True, resolution=(args.res, args.res), obs_dtype=getattr(torch, dt))
                env.set_task(table)
                env.reset()
                for mode in args.ids:
                    ids_h = ((np.arange(N) // 4) % P if mode == "workgroup" else np.arange(N) % P).astype(np.int32)
                    ids = torch.as_tensor(ids_h, device=DEV)
                    env.reset()
                    actions = env.rollout_policy(pol, T, policy_ids=ids, record=True).actions
                    tp = TorchPolicy(pol, ids_h, args.res, DEV)

                    def loop():
                        obs, rew, done = env._obs, env._reward, env._done
                        for _ in range(T):
                            obs, rew, done, _ = env.step(tp.act(obs, rew, done))
                            tp.seen(rew, done)

                    variants = {"rollout_policy": lambda: env.rollout_policy(pol, T, policy_ids=ids, record=True, obs_every=1),
                                "rollout_policy_last_frame": lambda: env.rollout_policy(pol, T, policy_ids=ids),
                                "rollout_actions": lambda: env.rollout(actions, obs_every=1),
                                "step_loop_torch": loop}
                    got, inner = compare(env, variants, args.repeats)
                    row = dict(bench="maze3d_rollout_policy", env="disc", n_envs=N, maze=args.maze, tasks=args.tasks, res=args.res,
                               obs_dtype=dt, steps=T, grid=args.grid, hidden=args.hidden, policies=P, ids=mode,
                               param_bytes=4 * pol.param_count, frame_read_mb_per_step=N * args.res * args.res * 3 *
                               (1 if dt == "uint8" else 4) / 1e6, repeats=args.repeats, calls_per_window=inner)
                    for name, (med, lo, hi) in got.items():
                        row[name + "_ms"], row[name + "_ms_min"], row[name + "_ms_max"] = med, lo, hi
                        row[name + "_us_per_step"] = 1e3 * med / T
                    row["speedup_over_step_loop"] = got["step_loop_torch"][0] / got["rollout_policy"][0]
                    row["rollout_policy_over_rollout_actions"] = got["rollout_policy"][0] / got["rollout_actions"][0]
                    print(json.dumps(row), flush=True)
                    out.write(json.dumps(row) + "\n")
                    out.flush()
                del env
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
