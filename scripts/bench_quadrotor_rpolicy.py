"""Time quadrotor closed-loop rollouts with recurrent policies against the MLP form of the same width and against a step()
loop with the same recurrent policy in torch, in one process, with HIP events.

    python scripts/bench_quadrotor_rpolicy.py [--regions 7] [--out profiles/quadrotor/bench_quadrotor_rpolicy.jsonl]

Per batch size (4 096 and 65 536 envs), T = 64 steps per launch, H in {32, 64} with 64 policies, fused auto-reset,
records off:
  rollout_rpolicy  the recurrent form, policies wave-uniform (id = e // 64 % P) and fully mixed (id = e % P), the carry
                   kept from call to call
  rollout_policy   the MLP form (QuadrotorPolicy) with the same H, the same two layouts
  step_loop        T x (the same recurrent policy in torch with a per-env weight gather, then env.step), mixed ids
Every case: one warm-up call, then `regions` timed regions of one call each (T = 64 env steps: 0.6 to 110 ms of device work
per region), each between two HIP events; the median region is reported, with the fastest and the slowest beside it. One JSON
line per case, time per env step of the whole batch. No time here is a pass/fail gate; the script fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metagym_amd  # noqa: E402
from metagym_amd.quadrotor import QuadrotorPolicy, QuadrotorPolicyState, QuadrotorRecurrentPolicy  # noqa: E402

T, P, D = 64, 64, 16


def make_policies(hidden, rs):
    """(recurrent, MLP) of the same width. Gains small enough that most units stay inside (-1, 1)."""
    f = np.float32
    u = lambda lo, hi, *shape: rs.uniform(lo, hi, shape).astype(f)
    bo = u(3.0, 8.0, P, 4)
    rec = QuadrotorRecurrentPolicy(u(-0.1, 0.1, P, hidden, D), u(-0.02, 0.02, P, hidden, 4), u(-0.02, 0.02, P, hidden),
                                   u(-0.1, 0.1, P, hidden), u(-0.1, 0.1, P, hidden, hidden), u(-0.5, 0.5, P, hidden),
                                   u(-0.2, 0.2, P, 4, hidden), bo)
    mlp = QuadrotorPolicy(u(-0.3, 0.3, P, hidden, D), u(-1, 1, P, hidden), u(-0.2, 0.2, P, 4, hidden), bo)
    return rec, mlp


def torch_recurrent(pol, ids, n, dev):
    """The same recurrent policy as batched torch operations on gathered per-env weights (not the defined association:
    this is the timing baseline, what a user of per-env recurrent policies writes without the launch). Returns
    step(x, reward, done) -> actions; the carry lives in the closure."""
    ids = torch.as_tensor(ids, device=dev).long()
    g = lambda a: torch.as_tensor(a, device=dev)[ids].contiguous()
    win = torch.cat([g(pol.wx), g(pol.wa), g(pol.wr)[:, :, None], g(pol.wd)[:, :, None], g(pol.wh)], dim=2)   # [N, H, D + 6 + H]
    b, wo, bo = g(pol.b), g(pol.wo), g(pol.bo)
    h = torch.zeros(n, pol.hidden, device=dev)
    pa = torch.zeros(n, 4, device=dev)

    def step(x, reward, done):
        nonlocal h, pa
        inp = torch.cat([x, pa, reward[:, None], done[:, None].to(torch.float32), h], dim=1)
        h = torch.clamp(b + torch.bmm(win, inp[:, :, None])[:, :, 0], -1.0, 1.0)
        pa = (bo + torch.bmm(wo, h[:, :, None])[:, :, 0]).contiguous()
        return pa
    return step


def timed(fn, regions):
    """one warm-up, then `regions` regions of one call each; (median, min, max) in us per call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3)
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--hidden", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--out", default=os.path.join("profiles", "quadrotor", "bench_quadrotor_rpolicy.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_quadrotor_rpolicy.py measures on a GPU; none is visible")
    dev = "cuda:0"
    rs = np.random.RandomState(0)
    rows = []

    def emit(us, **kw):
        med, lo, hi = us
        kw.update(us_per_env_step=round(med / T, 3), us_per_env_step_min=round(lo / T, 3), us_per_env_step_max=round(hi / T, 3),
                  regions=args.regions, steps=T, device=torch.cuda.get_device_name(0))
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for n in args.sizes:
        env = metagym_amd.make("quadrotor-v0", num_envs=n, device=dev, task="hovering_control", nt=1000, auto_reset=True,
                               seed=0)
        env.reset(seed=0)
        layouts = {"wave_uniform": np.arange(n) // 64 % P, "mixed": np.arange(n) % P}
        for hidden in args.hidden:
            rec, mlp = make_policies(hidden, rs)
            for name, ids in layouts.items():
                carry = QuadrotorPolicyState.zeros(n, hidden, dev)
                emit(timed(lambda: env.rollout_policy(rec, T, ids, state=carry), args.regions),
                     case="rollout_rpolicy", hidden=hidden, layout=name, num_envs=n)
                emit(timed(lambda: env.rollout_policy(mlp, T, ids), args.regions),
                     case="rollout_policy", hidden=hidden, layout=name, num_envs=n)
            f = torch_recurrent(rec, layouts["mixed"], n, dev)

            def loop():
                o, r, d = env._obs, env._reward, env._done
                for _ in range(T):
                    o, r, d, _ = env.step(f(o, r, d))
            emit(timed(loop, args.regions), case="step_loop", hidden=hidden, layout="mixed", num_envs=n)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
