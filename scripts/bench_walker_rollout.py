"""Per-env-step time of WalkerBatchEnv.rollout(actions[T]) against the step() loop, eager and replayed from a captured hipGraph.

    python scripts/bench_walker_rollout.py [--out profiles/walker/bench_walker_rollout.jsonl] [--sizes 64,512,8192] [--T 32]

Humanoid and ant, default preset, auto_reset on, from a steady-state batch (WARM_STEPS random steps after reset, so episodes
end and restart at different times). Every variant is warmed up, then timed in `--rounds` alternating rounds (loop, graph,
rollout, loop, ...) of `--reps` calls of T steps each, with device events around each round's calls; the result is the median
round. One JSON line per (robot, N): microseconds per env step (one step of the whole batch) for the three variants.
A run without a GPU fails: there is nothing to measure."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import metagym_amd.metalocomotion as ml  # noqa: E402

WARM_STEPS = 40


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def bench(robot, n, T, reps, rounds, device):
    cls = {"humanoid": ml.MetaHumanoidEnv, "ant": ml.MetaAntEnv}[robot]
    env = cls(num_envs=n, device=device, auto_reset=True, max_steps=200, seed=1)
    env.set_task(env.tra_tasks[:8])
    env.reset(seed=0)
    gen = torch.Generator(device=device).manual_seed(0)
    acts = torch.rand(T, n, env.n_joints, generator=gen, device=device) * 2.0 - 1.0
    for t in range(WARM_STEPS):
        env.step(acts[t % T])

    def loop():
        for t in range(T):
            env.step(acts[t])

    def rollout():
        env.rollout(acts)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loop()
        rollout()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loop()
    variants = {"loop_eager": loop, "loop_graph": graph.replay, "rollout": rollout}
    for fn in variants.values():
        timed(fn, 2)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, reps) / (reps * T) * 1e6)
    row = {"robot": robot, "num_envs": n, "T": T, "reps": reps, "rounds": rounds, "preset": env.preset, "auto_reset": True,
           "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        row["us_per_step_" + k] = round(statistics.median(v), 3)
        row["us_per_step_" + k + "_min_max"] = [round(min(v), 3), round(max(v), 3)]
    row["rollout_vs_loop_eager"] = round(row["us_per_step_loop_eager"] / row["us_per_step_rollout"], 3)
    row["rollout_vs_loop_graph"] = round(row["us_per_step_loop_graph"] / row["us_per_step_rollout"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "walker", "bench_walker_rollout.jsonl"))
    ap.add_argument("--sizes", default="64,512,8192")
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--reps", type=int, default=0, help="calls per timed round (0: sized so that a round is >= ~0.3 s)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_walker_rollout.py measures on the GPU; there is nothing to time without one"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for robot in ("humanoid", "ant"):
            for n in [int(x) for x in args.sizes.split(",")]:
                reps = args.reps or max(3, min(40, 65536 // max(n, 1)))
                row = bench(robot, n, args.T, reps, args.rounds, args.device)
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
                f.flush()


if __name__ == "__main__":
    main()
