"""Time the quadrotor task-table step against the uniform steps, in one process, with HIP events.

    python scripts/bench_quadrotor_tasks.py [--steps 200] [--warmup 20] [--out profiles/quadrotor/bench_quadrotor_tasks.jsonl]

Per batch size (4 096 and 65 536 envs): the table path with V = 1, 16 and 256 sampled airframes, the uniform generic
form (MG_QUAD_GENERIC=1, read when the env is built) and the uniform default step. One JSON line per case. No time here
is a pass/fail gate."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metagym_amd  # noqa: E402
from metagym_amd.quadrotor import sample_tasks  # noqa: E402


def make_env(n, generic=False):
    if generic:
        os.environ["MG_QUAD_GENERIC"] = "1"
    try:
        return metagym_amd.make("quadrotor-v0", num_envs=n, device="cuda:0", task="hovering_control", nt=1000,
                                auto_reset=True, seed=0)
    finally:
        os.environ.pop("MG_QUAD_GENERIC", None)


def time_steps(env, steps, warmup):
    n = env.num_envs
    a = torch.rand(n, 4, device="cuda:0") * 10.0 + 2.0
    env.reset(seed=0)
    for _ in range(warmup):
        env.step(a)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        env.step(a)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / steps
    return us, n / us * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "quadrotor", "bench_quadrotor_tasks.jsonl"))
    args = ap.parse_args()
    rows = []
    for n in (4096, 65536):
        cases = [("uniform_default", make_env(n)), ("uniform_generic", make_env(n, generic=True))]
        for v in (1, 16, 256):
            env = make_env(n)
            env.set_task(sample_tasks(v, seed=0, spread=0.0 if v == 1 else 0.2))
            cases.append(("table_V%d" % v, env))
        for name, env in cases:
            us, rate = time_steps(env, args.steps, args.warmup)
            rows.append(dict(case=name, num_envs=n, steps=args.steps, us_per_step=round(us, 3), env_steps_per_s=round(rate),
                             device=torch.cuda.get_device_name(0)))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
