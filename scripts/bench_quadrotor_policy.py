"""Time quadrotor closed-loop rollouts against the step() loop and the open-loop rollout, in one process, with HIP events.

    python scripts/bench_quadrotor_policy.py [--repeats 5] [--out profiles/quadrotor/bench_quadrotor_policy.jsonl]

Per batch size (4 096 and 65 536 envs), T = 64 steps per launch, H in {0, 32, 128} with 64 policies:
  rollout_policy   policies wave-uniform (id = e // 64 % P) and fully mixed (id = e % P), records off and on
  step_loop        T x (the same policy in torch, then env.step)
  rollout_actions  env.rollout on precomputed actions (no policy at all)
One JSON line per case, time per env step. No time here is a pass/fail gate."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metagym_amd  # noqa: E402
from metagym_amd.quadrotor import QuadrotorPolicy  # noqa: E402

T, P = 64, 64


def make_policy(hidden, rs):
    f = np.float32
    b2 = rs.uniform(3.0, 8.0, (P, 4)).astype(f)
    if hidden == 0:
        return QuadrotorPolicy.linear(rs.uniform(-0.1, 0.1, (P, 4, 16)).astype(f), b2)
    return QuadrotorPolicy(rs.uniform(-0.3, 0.3, (P, hidden, 16)).astype(f), rs.uniform(-1, 1, (P, hidden)).astype(f),
                           rs.uniform(-0.2, 0.2, (P, 4, hidden)).astype(f), b2)


def torch_policy(pol, ids, dev):
    """the same policy as batched torch operations (not the defined association: this is the timing baseline)"""
    ids = torch.as_tensor(ids, device=dev).long()
    b2 = torch.as_tensor(pol.b2, device=dev)[ids]
    w2 = torch.as_tensor(pol.w2, device=dev)[ids]
    if pol.hidden == 0:
        return lambda x: (b2 + torch.bmm(w2, x[:, :, None])[:, :, 0]).contiguous()
    w1, b1 = torch.as_tensor(pol.w1, device=dev)[ids], torch.as_tensor(pol.b1, device=dev)[ids]
    return lambda x: (b2 + torch.bmm(w2, torch.relu(b1 + torch.bmm(w1, x[:, :, None])[:, :, 0])[:, :, None])[:, :, 0]).contiguous()


def timed(fn, repeats):
    fn()                                                   # warm-up
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(repeats):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / repeats             # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "quadrotor", "bench_quadrotor_policy.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    rs = np.random.RandomState(0)
    rows = []

    def emit(**kw):
        kw["us_per_env_step"] = round(kw.pop("us") / T, 3)
        kw["device"] = torch.cuda.get_device_name(0)
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for n in (4096, 65536):
        env = metagym_amd.make("quadrotor-v0", num_envs=n, device=dev, task="hovering_control", nt=1000, auto_reset=True,
                               seed=0)
        obs = env.reset(seed=0)
        acts = torch.rand(T, n, 4, device=dev) * 10.0 + 2.0
        emit(case="rollout_actions", num_envs=n, steps=T, us=timed(lambda: env.rollout(acts), args.repeats))
        layouts = {"wave_uniform": np.arange(n) // 64 % P, "mixed": np.arange(n) % P}
        for hidden in (0, 32, 128):
            pol = make_policy(hidden, rs)
            for name, ids in layouts.items():
                for record in (False, True):
                    us = timed(lambda: env.rollout_policy(pol, T, ids, record=record), args.repeats)
                    emit(case="rollout_policy", hidden=hidden, layout=name, record=record, num_envs=n, steps=T, us=us)
            f = torch_policy(pol, layouts["mixed"], dev)

            def loop():
                o = obs
                for _ in range(T):
                    o = env.step(f(o))[0]
            emit(case="step_loop", hidden=hidden, layout="mixed", num_envs=n, steps=T, us=timed(loop, args.repeats))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
