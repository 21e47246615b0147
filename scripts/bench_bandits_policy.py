"""Times `Bandits.rollout_policy` (one launch, the recurrent policy inside it) per env step against
  (a) `rollout(actions)` on pre-drawn actions: what the policy adds on top of the open loop;
  (b) the `step()` loop with the same recurrent policy in torch (a gather of the env's weights, `bmm`, the clamp, the argmax),
      the host between every two steps.
Shapes: N = 4 096 and 65 536, K = 10, H = 32, T = 256, max_steps = 100 with auto_reset and Classical tasks drawn in the launch,
one policy id per wave and mixed ids. The three timings of a row run on the same commit, the same GPU and in the same process:
one warm-up call, then the median of `--repeats` regions, each between two HIP events on the current stream with the second
one synchronised. One JSON line per measurement into profiles/bandits/bench_bandits_policy.jsonl; no time is a pass/fail gate.

    python scripts/bench_bandits_policy.py [--sizes 4096 65536] [--hidden 32] [--arms 10] [--steps 256] [--repeats 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metagym_amd.bandits import BanditPolicy, Bandits  # noqa: E402

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
    """The same policy with torch ops around step(): a gather of each env's weights, the looked-up column of wa, bmm. (Not
    bit-identical to the definition: bmm chooses its own summation order. It is the baseline a user would write.)"""
    N, H = env.num_envs, pol.hidden
    idx = torch.as_tensor(ids, device=DEV).long()
    wa, wr, wd, wh, b, wo, bo = (torch.as_tensor(v, device=DEV)[idx] for v in (pol.wa, pol.wr, pol.wd, pol.wh, pol.b, pol.wo, pol.bo))

    def run():
        h = torch.zeros(N, H, device=DEV)
        z = b
        pr, pd = torch.zeros(N, 1, device=DEV), torch.zeros(N, 1, device=DEV)
        for _ in range(T):
            z = z + wr * pr + wd * pd + torch.bmm(wh, h.unsqueeze(2)).squeeze(2)
            h = z.clamp(-1.0, 1.0)
            act = (bo + torch.bmm(wo, h.unsqueeze(2)).squeeze(2)).argmax(1)
            _, rew, done, _ = env.step(act)
            z = b + torch.gather(wa, 2, act.view(N, 1, 1).expand(N, H, 1)).squeeze(2)
            pr, pd = rew.unsqueeze(1), done.float().unsqueeze(1)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--arms", type=int, default=10)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bandits", "bench_bandits_policy.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    T, K, H, P = args.steps, args.arms, args.hidden, 64
    rs = np.random.RandomState(H)
    f = np.float32
    pol = BanditPolicy(rs.randn(P, H, K).astype(f), rs.randn(P, H).astype(f), rs.randn(P, H).astype(f),
                       (rs.randn(P, H, H) / np.sqrt(H)).astype(f), (0.1 * rs.randn(P, H)).astype(f),
                       (rs.randn(P, K, H) / np.sqrt(H)).astype(f), (0.1 * rs.randn(P, K)).astype(f))
    with open(args.out, "a") as out:
        for N in args.sizes:
            env = Bandits(num_envs=N, arms=K, max_steps=100, device=DEV, seed=0, auto_reset=True, resample_task="Classical")
            env.set_task(env.sample_task("Classical"))
            env.reset()
            actions = torch.randint(0, K, (T, N), dtype=torch.int32, device=DEV)
            open_loop = timed(lambda: env.rollout(actions), args.repeats)
            for layout, ids in (("one_id_per_wave", (np.arange(N) // 64) % P), ("mixed_ids", np.arange(N) % P)):
                closed = timed(lambda: env.rollout_policy(pol, T, policy_ids=ids), args.repeats)
                loop = timed(torch_policy_loop(env, pol, ids, T), max(1, args.repeats // 2))
                row = dict(bench="bandits_policy", gpu=torch.cuda.get_device_name(0), n_envs=N, arms=K, hidden=H, steps=T,
                           ids=layout, repeats=args.repeats, rollout_policy_ms=closed, rollout_actions_ms=open_loop,
                           step_loop_torch_ms=loop, us_per_step_policy=1e3 * closed / T, us_per_step_actions=1e3 * open_loop / T,
                           us_per_step_loop=1e3 * loop / T)
                print(json.dumps(row), flush=True)
                out.write(json.dumps(row) + "\n")
            del env
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
