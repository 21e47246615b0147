"""Per-env-step time of WalkerBatchEnv.rollout_policy with a recurrent policy (WalkerRecurrentPolicy, the carry kept from call
to call) against the MLP policy of the same width in the launch and against the step() loop with the recurrent policy in torch.

    python scripts/bench_walker_rpolicy.py [--out profiles/walker/bench_walker_rpolicy.jsonl] [--sizes 64,512,8192] [--T 32]
                                           [--hidden 32,64,256]

Humanoid and ant, default preset, auto_reset on, from a steady-state batch (WARM_STEPS closed-loop steps after reset, so
episodes end and restart at different times), 16 policies dealt round-robin. Cases, per (robot, N, H):
    rpolicy        env.rollout_policy(rpol, T, state=carry)    one launch per T steps, nothing recorded, one carry throughout
    mlp            env.rollout_policy(pol, T)                  the feed-forward policy of the same H: what the memory adds
    loop_torch     for t: step(policy(obs, carry)) with the recurrent policy in torch: the weights gathered once per call,
                   one baddbmm per layer and step, the carry updated from step()'s reward and done
Every case is warmed up, then timed in 7 regions of `--reps` calls of T steps each between HIP events, the cases alternating;
the result is the median region. One JSON line per (robot, N, H): microseconds per env step (one step of the whole batch). The
torch policy is the same network, not the same bits (bmm picks its own summation order): it is a timing baseline, the
bit-exact reference is WalkerRecurrentPolicy.reference. No time is a pass/fail gate. A run without a GPU fails: there is nothing
to measure."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import metagym_amd.metalocomotion as ml  # noqa: E402

WARM_STEPS, N_POLICIES, REGIONS = 40, 16, 7


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def make_policies(H, D, A, P, seed=0):
    g = np.random.RandomState(seed)
    u = lambda s, *shape: g.uniform(-s, s, size=shape).astype(np.float32)
    rpol = ml.WalkerRecurrentPolicy(u(0.05, P, H, D), u(0.05, P, H, A), u(0.05, P, H), u(0.05, P, H), u(0.05, P, H, H), u(0.1, P, H),
                                    u(0.05, P, A, H), u(0.1, P, A))
    return rpol, ml.WalkerPolicy(rpol.wx, rpol.b, rpol.wo, rpol.bo)


def bench(robot, n, T, H, reps, device):
    cls = {"humanoid": ml.MetaHumanoidEnv, "ant": ml.MetaAntEnv}[robot]
    env = cls(num_envs=n, device=device, auto_reset=True, max_steps=200, seed=1)
    env.set_task(env.tra_tasks[:8])
    env.reset(seed=0)
    rpol, pol = make_policies(H, env.obs_dim, env.n_joints, N_POLICIES)
    ids = torch.arange(n, device=device) % N_POLICIES
    carry = env.rollout_policy(rpol, WARM_STEPS).state
    # the torch policy: one [H, D + A + 2 + H] matrix per env over the concatenated input, gathered once per call of T steps
    t = lambda a: torch.from_numpy(a).to(device)
    w_in = torch.cat([t(rpol.wx), t(rpol.wa), t(rpol.wr)[:, :, None], t(rpol.wd)[:, :, None], t(rpol.wh)], dim=2)
    b, wo, bo = t(rpol.b), t(rpol.wo), t(rpol.bo)
    loop = {"h": carry.h.clone(), "pa": carry.prev_action.clone(), "pr": carry.prev_reward.clone(),
            "pd": carry.prev_done.float()}

    def loop_torch():
        W, B, WO, BO = w_in[ids], b[ids], wo[ids], bo[ids]
        obs, h, pa, pr, pd = env._obs, loop["h"], loop["pa"], loop["pr"], loop["pd"]
        for _ in range(T):
            x = torch.cat([obs, pa, pr[:, None], pd[:, None], h], dim=1).unsqueeze(2)
            h = torch.baddbmm(B.unsqueeze(2), W, x).clamp_(-1.0, 1.0)
            pa = torch.baddbmm(BO.unsqueeze(2), WO, h).squeeze(2)
            h = h.squeeze(2)
            obs, pr, done, _info = env.step(pa)
            pd = done.float()
        loop["h"], loop["pa"], loop["pr"], loop["pd"] = h, pa, pr.clone(), pd

    cases = {"rpolicy": lambda: env.rollout_policy(rpol, T, state=carry), "mlp": lambda: env.rollout_policy(pol, T),
             "loop_torch": loop_torch}
    for fn in cases.values():
        timed(fn, 2)
    times = {k: [] for k in cases}
    for _ in range(REGIONS):
        for k, fn in cases.items():
            times[k].append(timed(fn, reps) / (reps * T) * 1e6)
    row = {"robot": robot, "num_envs": n, "T": T, "hidden": H, "n_policies": N_POLICIES, "reps": reps, "regions": REGIONS,
           "preset": env.preset, "auto_reset": True, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        row["us_per_step_" + k] = round(statistics.median(v), 3)
        row["us_per_step_" + k + "_min_max"] = [round(min(v), 3), round(max(v), 3)]
    row["rpolicy_vs_mlp"] = round(row["us_per_step_rpolicy"] / row["us_per_step_mlp"], 3)
    row["loop_torch_vs_rpolicy"] = round(row["us_per_step_loop_torch"] / row["us_per_step_rpolicy"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "walker", "bench_walker_rpolicy.jsonl"))
    ap.add_argument("--sizes", default="64,512,8192")
    ap.add_argument("--hidden", default="32,64,256")
    ap.add_argument("--robots", default="humanoid,ant")
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--reps", type=int, default=0, help="calls per timed region (0: sized by the batch)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_walker_rpolicy.py measures on the GPU; there is nothing to time without one"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for robot in args.robots.split(","):
            for n in [int(x) for x in args.sizes.split(",")]:
                for H in [int(x) for x in args.hidden.split(",")]:
                    reps = args.reps or max(2, min(10, 8192 // max(n, 1)))
                    row = bench(robot, n, args.T, H, reps, args.device)
                    print(json.dumps(row), flush=True)
                    f.write(json.dumps(row) + "\n")
                    f.flush()


if __name__ == "__main__":
    main()
