"""Times the MetaMaze shortest-path fields and the expert that descends them (csrc/maze_expert.hip).
  (a) field build: `env.distance_field()` (one launch, one workgroup per task) for T = 4 096 sampled tasks at n = 15 and
      n = 63, MOVES_2D and TURNS, beside `distance_field_reference` on the host for the same tasks;
  (b) per-step time of `rollout_expert` at N = 4 096 and 65 536 over T = 256 tasks of n = 15, beside `rollout(actions)` on the
      actions it recorded (what the 4-neighbour lookup adds to the open loop) and beside the `step(expert_action())` loop.
HIP events around windows of ten calls (one pass of the step loop), one warm-up, the median of `--repeats`, one process. One JSON line per measurement into
profiles/maze/bench_maze_expert.jsonl; no time is a pass/fail gate.

    python scripts/bench_maze_expert.py [--tasks 4096] [--mazes 15 63] [--sizes 4096 65536] [--steps 64] [--repeats 5]
                                        [--host-tasks 0]     (0 = the host reference on all tasks; k = on the first k only)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import metagym_amd  # noqa: E402
from metagym_amd.metamaze import MAZE_TASK_MANAGER  # noqa: E402
from metagym_amd.metamaze import expert as ex  # noqa: E402

DEV = "cuda:0"


def timed(fn, repeats, inner=1):
    """Median milliseconds per call of `repeats` windows of `inner` calls between HIP events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return float(np.median(ms))


def sample(T, n):
    return MAZE_TASK_MANAGER.sample_tasks_device(T, device=DEV, seed=0, n=n, allow_loops=True, step_reward=-0.01, goal_reward=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=4096)
    ap.add_argument("--mazes", type=int, nargs="+", default=[15, 63])
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--rollout-tasks", type=int, default=256)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-tasks", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maze", "bench_maze_expert.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_maze_expert.py measures on the GPU; there is nothing to time without one"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        def emit(row):
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")

        # (a) the field
        for n in args.mazes:
            T = args.tasks
            table = sample(T, n)
            env = metagym_amd.make("meta-maze-2D-v0", num_envs=1, device=DEV, task_type="ESCAPE")
            env.set_task(table)
            walls = table.tensors["walls"].cpu().numpy().reshape(T, n, n)
            goal = table.tensors["goal"].cpu().numpy()
            src = np.zeros((T, n, n), np.uint8)
            src[np.arange(T), goal[:, 0], goal[:, 1]] = 1
            src_d = torch.as_tensor(src).to(DEV)
            k = T if args.host_tasks <= 0 else min(T, args.host_tasks)
            for kind in (ex.MOVES_2D, ex.TURNS):
                gpu_ms = timed(lambda: env.distance_field(src_d, kind), args.repeats, inner=10)   # (a mask: the goal field would be cached)
                t0 = time.perf_counter()
                ref = ex.distance_field_reference(walls[:k], src[:k], kind)
                host_ms = 1e3 * (time.perf_counter() - t0)
                same = bool(np.array_equal(env.distance_field(src_d, kind).numpy()[:k], ref))
                emit(dict(bench="maze_distance_field", kind=ex.KIND_NAMES[kind], n=n, tasks=T, field_ms=gpu_ms,
                          us_per_task=1e3 * gpu_ms / T, levels_max=int(ref.max()), host_reference_tasks=k,
                          host_reference_ms=host_ms, host_reference_us_per_task=1e3 * host_ms / k, equal_to_reference=same))
            del env

        # (b) the closed loop
        steps = args.steps
        table = sample(args.rollout_tasks, 15)
        for N in args.sizes:
            env = metagym_amd.make("meta-maze-2D-v0", num_envs=N, device=DEV, max_steps=50, task_type="ESCAPE", view_grid=2,
                                   auto_reset=True)
            env.set_task(table)
            env.reset()
            env.distance_field()
            actions = env.rollout_expert(steps, record=True).actions
            env.reset()
            closed = timed(lambda: env.rollout_expert(steps), args.repeats, inner=10)
            env.reset()
            open_loop = timed(lambda: env.rollout(actions), args.repeats, inner=10)
            env.reset()

            def loop():
                for _ in range(steps):
                    env.step(env.expert_action())
            step_loop = timed(loop, args.repeats)
            emit(dict(bench="maze_expert_rollout", n_envs=N, maze=15, tasks=args.rollout_tasks, view_grid=2, steps=steps,
                      rollout_expert_ms=closed, rollout_actions_ms=open_loop, step_loop_ms=step_loop,
                      us_per_step_expert=1e3 * closed / steps, us_per_step_actions=1e3 * open_loop / steps,
                      us_per_step_loop=1e3 * step_loop / steps))
            del env
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
