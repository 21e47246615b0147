#!/usr/bin/env python3
"""liftsim-v0 throughput on one GPU: one JSON line per workload.

    python scripts/bench_liftsim.py [--reps 200] [--warmup 50] [--out FILE]
    python scripts/bench_liftsim.py --rollout 500 [--policy both] [--repeats 7] [--out FILE]

Workloads: the default config (CUSTOM, F = 10, E = 4, dt = 0.5; the flow table is tests/golden/liftsim_flow.npy, the
reference's mansion_flow.npy) at N = 4096 and 65 536, `step` with uniformly random actions drawn on the device before the
timed region (one [reps, N, 8] tensor); and the host baseline, the reference restated in tests/liftsim_oracle.py (one env,
one CPU core, the same kind of random actions). Every env starts at 07:30 (the morning rush, where queues are longest:
warm-up steps first run the envs from midnight). Times come from HIP events on the launching stream around `reps`
back-to-back step() calls.

--rollout T compares, per size and in one process, four ways to run the same T steps from the same 07:30 state (the arena
is put back from a snapshot before every timed repeat): (a) `step_loop`, step() in a Python loop over pre-drawn random
actions; (b) `rollout_actions`, one rollout(actions) launch over the same actions; (c) `rollout_rule`, one
rollout(policy="rule") launch; (d) `step_rule_loop`, step(rule_policy()) in a Python loop. --policy random runs (a) and
(b), rule (c) and (d), both all four. Each is timed `--repeats` times after one untimed pass, by HIP events around the
whole T steps; a line reports the median per step with the minimum and maximum over the repeats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FLOW = os.path.join(ROOT, "tests", "golden", "liftsim_flow.npy")


def _actions(reps, N, F, E, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.empty(reps, N, 2 * E, dtype=torch.int32, device="cuda")
    a[:, :, 0::2] = torch.randint(-1, F + 1, (reps, N, E), generator=g, device="cuda", dtype=torch.int32)
    a[:, :, 1::2] = torch.randint(-1, 2, (reps, N, E), generator=g, device="cuda", dtype=torch.int32)
    return a


def bench_gpu(N, reps, warmup, start_steps):
    import torch
    from metagym_amd.liftsim import LiftSim
    env = LiftSim(num_envs=N, seed=0, flow=np.load(FLOW))
    pre = _actions(256, N, env.F, env.E, 1)
    for k in range(start_steps):                       # run the day up to the rush
        env.step(pre[k % 256])
    acts = _actions(reps + warmup, N, env.F, env.E, 2)
    for k in range(warmup):
        env.step(acts[k])
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(reps):
        env.step(acts[warmup + k])
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / reps
    flags = int(env.overflow.sum().item()) + int(env.unsupported.sum().item()) + int(env.invalid.sum().item())
    return dict(workload="step_N%d" % N, num_envs=N, time_ms=ms, env_steps_per_s=N / (ms * 1e-3),
                start_step=start_steps + warmup, flagged_envs=flags, arena_bytes_per_env=env.arena.numel() / N,
                device=torch.cuda.get_device_name())


def bench_rollout(N, T, repeats, start_steps, policies):
    import torch
    from metagym_amd.liftsim import LiftSim
    env = LiftSim(num_envs=N, seed=0, flow=np.load(FLOW))
    pre = _actions(256, N, env.F, env.E, 1)
    for k in range(0, start_steps, 256):               # run the day up to the rush, 256 steps a launch
        env.rollout(pre[:min(256, start_steps - k)], record=())
    acts = _actions(T, N, env.F, env.E, 2)
    snap = env.arena.clone()

    def step_loop():
        for k in range(T):
            env.step(acts[k])

    def step_rule_loop():
        for k in range(T):
            env.step(env.rule_policy())
    ways = []
    if "random" in policies:
        ways += [("step_loop", step_loop), ("rollout_actions", lambda: env.rollout(acts, record=()))]
    if "rule" in policies:
        ways += [("rollout_rule", lambda: env.rollout(policy="rule", steps=T, record=())),
                 ("step_rule_loop", step_rule_loop)]
    lines = []
    for name, fn in ways:
        ms = []
        for r in range(repeats + 1):                   # the first pass is the warm-up
            env.arena.copy_(snap)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if r > 0:
                ms.append(t0.elapsed_time(t1) / T)
        flags = int(env.overflow.sum().item()) + int(env.unsupported.sum().item()) + int(env.invalid.sum().item())
        med = float(np.median(ms))
        lines.append(dict(workload="%s_N%d" % (name, N), num_envs=N, steps_per_launch=T, repeats=repeats,
                          time_ms_per_step=med, min_ms_per_step=min(ms), max_ms_per_step=max(ms),
                          env_steps_per_s=N / (med * 1e-3), start_step=start_steps, flagged_envs=flags,
                          device=torch.cuda.get_device_name()))
        print(json.dumps(lines[-1]), flush=True)
    return lines


def bench_host(steps, start_steps):
    import liftsim_oracle as O
    env = O.Env(O.Config(flow=np.load(FLOW)), 0)
    rs = np.random.RandomState(0)
    acts = np.empty((steps + start_steps, 8), np.int32)
    acts[:, 0::2] = rs.randint(-1, 11, size=(steps + start_steps, 4))
    acts[:, 1::2] = rs.randint(-1, 2, size=(steps + start_steps, 4))
    for k in range(start_steps):
        env.step(acts[k].tolist())
    t = time.perf_counter()
    for k in range(steps):
        env.step(acts[start_steps + k].tolist())
    s = time.perf_counter() - t
    return dict(workload="host_restatement_1core", num_envs=1, time_ms=s * 1e3 / steps, env_steps_per_s=steps / s,
                start_step=start_steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--start", type=int, default=54000)    # 07:30 at dt = 0.5
    ap.add_argument("--host-steps", type=int, default=5000)
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rollout", type=int, default=0, metavar="T", help="compare T steps as a loop and as one launch")
    ap.add_argument("--policy", choices=("random", "rule", "both"), default="both")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if a.rollout > 0:
        pol = ("random", "rule") if a.policy == "both" else (a.policy,)
        lines = [ln for n in a.sizes.split(",") for ln in bench_rollout(int(n), a.rollout, a.repeats, a.start, pol)]
    else:
        lines = [bench_gpu(int(n), a.reps, a.warmup, a.start) for n in a.sizes.split(",")]
        lines.append(bench_host(a.host_steps, a.start))
        for ln in lines:
            print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
