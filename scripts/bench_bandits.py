#!/usr/bin/env python3
"""bandits-v0 throughput on one GPU: one JSON line per workload.

    python scripts/bench_bandits.py [--reps 5] [--warmup 2]

Workloads (K = 50 unless named): eager `step` at N = 65 536 and 2^20; `rollout` of T = 1000 at the same sizes; a
resample-heavy rollout (max_steps = 2, auto-reset with every distribution, K = 50 and 1000, T = 100, N = 65 536); and the
host baseline, the reference's Bandits restated on one numpy stream (tests/bandits_oracle.py Env, one env, one CPU core).
Times come from HIP events on the launching stream around `reps` back-to-back calls.

Byte model per env-step (what must cross HBM at least once): rollout = action 4 + outputs 18 (reward 4, done 1, steps 4,
expected gain 8, invalid 1) + the gathered gain 8 + two key words 8 + the refill's read and write of a 2496-byte block
every 312 steps (16.0) = 54.0 B; a T = 1 step adds the per-env state read and written around the launch (steps, episode
flag, pos, gauss cache: 34 B). `copy_fraction` is the modelled rate over the 6.3 TB/s measured copy ceiling."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_CEILING = 6.3e12
ROLLOUT_B = 4 + 18 + 8 + 8 + 2 * 2496 / 312
STEP_B = ROLLOUT_B + 34


def _env(N, K, M, auto_reset=False, resample=None):
    from metagym_amd.bandits import Bandits
    env = Bandits(num_envs=N, arms=K, max_steps=M, device="cuda", seed=0, auto_reset=auto_reset, resample_task=resample)
    env.set_task(env.sample_task())
    env.reset()
    return env


def _time(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(st)
    for _ in range(reps):
        fn()
    t1.record(st)
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3 / reps


def _line(name, N, K, T, sec, bytes_per_step, **extra):
    import torch
    rate = N * T / sec
    d = {"workload": name, "num_envs": N, "arms": K, "steps_per_call": T, "time_ms": sec * 1e3, "env_steps_per_s": rate,
         "model_bytes_per_env_step": bytes_per_step, "model_bytes_per_s": rate * bytes_per_step,
         "copy_fraction": rate * bytes_per_step / COPY_CEILING, "device": torch.cuda.get_device_name(0)}
    d.update(extra)
    return d


def gpu_lines(reps, warmup):
    import torch
    K = 50
    for N in (65536, 1 << 20):
        env = _env(N, K, 1000, auto_reset=True)
        a = torch.randint(-K, K, (N,), dtype=torch.int32, device="cuda")
        yield _line("step_N%d" % N, N, K, 1, _time(lambda: env.step(a), reps * 20, warmup), STEP_B, max_steps=1000)
        T = 1000
        acts = torch.randint(-K, K, (T, N), dtype=torch.int32, device="cuda")
        yield _line("rollout_T%d_N%d" % (T, N), N, K, T, _time(lambda: env.rollout(acts), reps, warmup), ROLLOUT_B,
                    max_steps=1000)
        del env, acts
        torch.cuda.empty_cache()
    N, T = 65536, 100
    for K in (50, 1000):
        acts = torch.randint(-K, K, (T, N), dtype=torch.int32, device="cuda")
        for dist in ("Classical", "Uniform", "Gaussian"):
            env = _env(N, K, 2, auto_reset=True, resample=dist)
            sec = _time(lambda: env.rollout(acts), reps, warmup)
            yield _line("resample_%s_K%d" % (dist, K), N, K, T, sec, ROLLOUT_B, max_steps=2,
                        tasks_per_s=N * T / 2 / sec)


def host_line(steps=200000):
    import numpy as np
    import bandits_oracle as bo
    env = bo.Env(np.random.RandomState(0), arms=50, max_steps=1000)
    acts = np.random.RandomState(1).randint(0, 50, size=steps).tolist()
    t0 = time.perf_counter()
    for a in acts:
        if env.need_reset:
            env.set_task(env.sample_task())
            env.reset()
        env.step(a)
    sec = time.perf_counter() - t0
    return {"workload": "host_reference_restatement", "num_envs": 1, "arms": 50, "env_steps": steps,
            "time_ms": sec * 1e3, "env_steps_per_s": steps / sec, "threads": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    for line in gpu_lines(a.reps, a.warmup):
        print(json.dumps(line), flush=True)
    if not a.no_host:
        print(json.dumps(host_line()), flush=True)


if __name__ == "__main__":
    main()
