"""Times expert demonstrations of the 3-D mazes (csrc/maze_expert.hip mg_maze3d_expert_rollout, `env.demonstrate`): `steps` env
steps with the expert inside the launches, beside
  (a) the eager loop it replaces, `env.step(env.expert_action())` (discrete) / `env.step(env.steer_action())` (continuous),
      which renders a frame on every step whatever is kept, and
  (b) the open loop `env.rollout(actions, obs_every=k)` on the actions the demonstration recorded (what choosing the action
      inside the launch adds),
for N = 4 096 and 65 536 envs and obs_every = 1, 8 and 0 (every frame, every eighth, the last one only), uint8 frames.
One process; every variant is warmed up once per shape; a window is enough calls for about 0.1 s between two HIP events (ended by
an event synchronise); the variants of one (env, N, obs_every) alternate inside every repeat and the median of `--repeats` windows
is reported with their min and max. The env is reset before every window so every variant starts from the same state. One JSON
line per (env, N, obs_every) into profiles/maze/bench_maze_demo.jsonl; no time is a pass/fail gate.

    python scripts/bench_maze_demo.py [--sizes 4096 65536] [--every 1 8 0] [--steps 32] [--res 64] [--repeats 5] [--envs disc cont]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import metagym_amd  # noqa: E402
from metagym_amd.metamaze import MAZE_TASK_MANAGER  # noqa: E402

DEV = "cuda:0"
IDS = {"disc": "meta-maze-discrete-3D-v0", "cont": "meta-maze-continuous-3D-v0"}


def window_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def compare(env, variants, repeats, target_ms=100.0):
    """{name: (median, min, max) ms per call}: one warm-up call each, then `repeats` rounds in which the variants take turns."""
    inner = {}
    for name, fn in variants.items():
        env.reset()
        fn()
        torch.cuda.synchronize()
        env.reset()
        inner[name] = int(min(50, max(1, math.ceil(target_ms / max(window_ms(fn, 1), 1e-3)))))
    ms = {name: [] for name in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            env.reset()
            ms[name].append(window_ms(fn, inner[name]))
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in ms.items()}, inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--every", type=int, nargs="+", default=[1, 8, 0])
    ap.add_argument("--envs", nargs="+", default=["disc", "cont"], choices=sorted(IDS))
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--maze", type=int, default=15)
    ap.add_argument("--tasks", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maze", "bench_maze_demo.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_maze_demo.py measures on the GPU; there is nothing to time without one"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    T = args.steps
    table = MAZE_TASK_MANAGER.sample_tasks_device(args.tasks, device=DEV, seed=0, n=args.maze, allow_loops=True, step_reward=-0.01,
                                                  goal_reward=1.0)
    with open(args.out, "a") as out:
        for kind in args.envs:
            for N in args.sizes:
                env = metagym_amd.make(IDS[kind], num_envs=N, device=DEV, max_steps=200, task_type="ESCAPE", auto_reset=True,
                                       resolution=(args.res, args.res), obs_dtype=torch.uint8)
                env.set_task(table)
                env.reset()
                env.distance_field()
                expert = env.steer_action if kind == "cont" else env.expert_action
                actions = env.demonstrate(T, record=True).actions

                def loop():
                    for _ in range(T):
                        env.step(expert())

                for k in args.every:
                    variants = {"demonstrate": lambda: env.demonstrate(T, record=True, obs_every=k),
                                "demonstrate_no_records": lambda: env.demonstrate(T, obs_every=k),
                                "rollout_actions": lambda: env.rollout(actions, obs_every=k),
                                "step_loop": loop}
                    got, inner = compare(env, variants, args.repeats)
                    row = dict(bench="maze3d_demonstrate", env=kind, n_envs=N, maze=args.maze, tasks=args.tasks, res=args.res,
                               obs_dtype="uint8", steps=T, obs_every=k, frames_kept=len(env.demonstrate(T, obs_every=k).obs_steps),
                               repeats=args.repeats, calls_per_window=inner)
                    for name, (med, lo, hi) in got.items():
                        row[name + "_ms"], row[name + "_ms_min"], row[name + "_ms_max"] = med, lo, hi
                        row[name + "_us_per_step"] = 1e3 * med / T
                    row["speedup_over_step_loop"] = got["step_loop"][0] / got["demonstrate"][0]
                    row["demonstrate_over_rollout_actions"] = got["demonstrate"][0] / got["rollout_actions"][0]
                    print(json.dumps(row), flush=True)
                    out.write(json.dumps(row) + "\n")
                    out.flush()
                del env, actions
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
