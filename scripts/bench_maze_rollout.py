"""MetaMaze: the same T actions from the same state_dict() snapshot as (a) `step()` in a Python loop and (b) one
`rollout()`, HIP events around the T steps, one process, one untimed pass then `--repeats` timed ones;
a line reports the median per step with the minimum and maximum over the repeats.

    python scripts/bench_maze_rollout.py [--steps 200] [--repeats 7] [--families 2d,3d] [--out FILE]

2-D: 15x15 mazes (the C1 shape: 64 tasks, view_grid 1, max_steps 200, auto_reset), ESCAPE and SURVIVAL, N = 1, 4 096 and
2^20, obs_every 0 and 1. Discrete 3-D: 9x9 mazes (the C3 shape: 64 tasks, SURVIVAL, max_steps 200, auto_reset) at 64x64 and
256x256, obs_every 0, 10 and 1; N = 16 384, or the largest power of two whose K recorded frame batches fit `--obs-gib`
(16 GiB). (a) is measured once per (case, N) and is code the rollouts do not touch: the baseline of the same run; (a) at
256x256, N = 16 384 is bench.py's C3 discrete configuration."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(env, snap, fn, T, repeats):
    import torch
    ms = []
    for r in range(repeats + 1):                       # the first pass is the warm-up
        env.load_state_dict(snap)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if r > 0:
            ms.append(t0.elapsed_time(t1) / T)
    return ms


def _line(case, way, N, T, repeats, ms, **extra):
    import torch
    med = float(np.median(ms))
    ln = dict(case=case, way=way, num_envs=N, steps=T, repeats=repeats, time_ms_per_step=med, min_ms_per_step=min(ms),
              max_ms_per_step=max(ms), env_steps_per_s=N / (med * 1e-3), device=torch.cuda.get_device_name(), **extra)
    print(json.dumps(ln), flush=True)
    return ln


def _bench_env(case, env, acts, obs_everys, T, repeats):
    """(a) once, then (b) per obs_every, all from one snapshot taken after reset + 20 steps."""
    import torch
    N = env.num_envs
    for t in range(20):
        env.step(acts[t % T])
    snap = env.state_dict()

    def loop():
        for t in range(T):
            env.step(acts[t])
    lines = [_line(case, "step_loop", N, T, repeats, _time(env, snap, loop, T, repeats))]
    for k in obs_everys:
        ms = _time(env, snap, lambda: env.rollout(acts, obs_every=k), T, repeats)
        lines.append(_line(case, "rollout", N, T, repeats, ms, obs_every=k, loop_ms_per_step=lines[0]["time_ms_per_step"],
                           speedup_vs_loop=lines[0]["time_ms_per_step"] / float(np.median(ms))))
        torch.cuda.empty_cache()
    return lines


def bench_2d(T, repeats, sizes):
    import torch
    import metagym_amd
    from metagym_amd.metamaze import MAZE_TASK_MANAGER
    table = MAZE_TASK_MANAGER.sample_tasks_device(64, device="cuda:0", seed=0, n=15, allow_loops=True, crowd_ratio=0.35,
                                                  step_reward=-0.01, goal_reward=1.0)
    lines = []
    for task_type in ("ESCAPE", "SURVIVAL"):
        for N in sizes:
            env = metagym_amd.make("meta-maze-2D-v0", num_envs=N, device="cuda:0", max_steps=200, view_grid=1,
                                   task_type=task_type, auto_reset=True)
            env.set_task(table)
            env.reset()
            acts = torch.randint(0, 4, (T, N), device="cuda:0", dtype=torch.int32)
            lines += _bench_env("maze2d_15x15_%s" % task_type.lower(), env, acts, (0, 1), T, repeats)
            del env, acts
            torch.cuda.empty_cache()
    return lines


def bench_3d(T, repeats, n_max, obs_gib):
    import torch
    import metagym_amd
    from metagym_amd.metamaze import MAZE_TASK_MANAGER
    from metagym_amd.metamaze.maze_env import rollout_obs_steps
    table = MAZE_TASK_MANAGER.sample_tasks_device(64, device="cuda:0", seed=0, n=9, allow_loops=False, step_reward=-0.01,
                                                  goal_reward=1.0, food_density=0.06, food_interval=20)
    lines = []
    for res in (64, 256):
        by_n = {}
        for k in (0, 10, 1):
            N = n_max
            while N > 1 and len(rollout_obs_steps(T, k)) * N * res * res * 12 > obs_gib * 2 ** 30:
                N //= 2
            by_n.setdefault(N, []).append(k)
        for N, ks in sorted(by_n.items(), reverse=True):
            env = metagym_amd.make("meta-maze-discrete-3D-v0", num_envs=N, device="cuda:0", max_steps=200,
                                   resolution=(res, res), task_type="SURVIVAL", auto_reset=True)
            env.set_task(table)
            env.reset()
            acts = torch.randint(0, 4, (T, N), device="cuda:0", dtype=torch.int32)
            lines += _bench_env("maze3d_discrete_9x9_%dx%d_survival" % (res, res), env, acts, ks, T, repeats)
            del env, acts
            torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--families", default="2d,3d")
    ap.add_argument("--sizes-2d", default="1,4096,1048576")
    ap.add_argument("--envs-3d", type=int, default=16384)
    ap.add_argument("--obs-gib", type=float, default=16.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    if "2d" in a.families.split(","):
        lines += bench_2d(a.steps, a.repeats, [int(n) for n in a.sizes_2d.split(",")])
    if "3d" in a.families.split(","):
        lines += bench_3d(a.steps, a.repeats, a.envs_3d, a.obs_gib)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
