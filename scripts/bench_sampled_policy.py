"""Times the softmax-sampled closed-loop launches (`rollout_policy` with a policy that has a temperature) per env step, for
the bandits and the 2-D maze, against
  (a) the greedy launch of the same weights: what the Gumbel-max draw adds;
  (b) one training iteration: the sampled launch with record=True, the torch `replay` of its records, `log_prob` and the
      backward pass (no optimiser step);
  (c) the `step()` loop with the same recurrent policy in torch and `torch.distributions.Categorical` sampling, the host
      between every two steps: the baseline a user would write.
Shapes: N = 4 096 and 65 536; bandits K = 10, H = 32, T = 256, max_steps = 100 with auto_reset and Classical tasks drawn in
the launch; maze 15 x 15, view_grid 2, H = 32, T = 64, max_steps = 50 with auto_reset. One policy for all envs (what a policy
gradient trains), temperature 1. The timings of a row run on the same commit, the same GPU and in the same process: one
warm-up call, then the median of `--repeats` regions, each between two HIP events on the current stream with the second one
synchronised. One JSON line per measurement into profiles/bandits/bench_bandits_sampled.jsonl and
profiles/maze/bench_maze_sampled.jsonl; no time is a pass/fail gate.

    python scripts/bench_sampled_policy.py [--sizes 4096 65536] [--hidden 32] [--repeats 7] [--out-dir profiles]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import metagym_amd  # noqa: E402
from metagym_amd.bandits import BanditPolicy, BanditPolicyNet, Bandits, log_prob  # noqa: E402
from metagym_amd.metamaze import MAZE_TASK_MANAGER, MazePolicy, MazePolicyNet  # noqa: E402
from metagym_amd.metamaze.policy import input_dim  # noqa: E402

DEV = "cuda:0"
F = np.float32


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


def bandit_categorical_loop(env, net, T):
    """The net's policy with torch ops around step(), the action drawn by Categorical."""
    N, H = env.num_envs, net.hidden
    wa, wr, wd, wh, b, wo, bo = (p.detach() for p in (net.wa, net.wr, net.wd, net.wh, net.b, net.wo, net.bo))

    def run():
        h = torch.zeros(N, H, device=DEV)
        z = b.expand(N, H)
        pr, pd = torch.zeros(N, 1, device=DEV), torch.zeros(N, 1, device=DEV)
        for _ in range(T):
            h = (z + wr * pr + wd * pd + h @ wh.t()).clamp(-1.0, 1.0)
            act = torch.distributions.Categorical(logits=bo + h @ wo.t()).sample().int()
            _, rew, done, _ = env.step(act)
            z = b + wa.t()[act.long()]
            pr, pd = rew.unsqueeze(1), done.float().unsqueeze(1)
    return run


def maze_categorical_loop(env, net, T):
    N, H = env.num_envs, net.hidden
    wx, wh, b, wo, bo = (p.detach() for p in (net.wx, net.wh, net.b, net.wo, net.bo))
    eye = torch.eye(4, device=DEV)

    def run():
        h = torch.zeros(N, H, device=DEV)
        pa = torch.zeros(N, 4, device=DEV)
        pr, pd = torch.zeros(N, 1, device=DEV), torch.zeros(N, 1, device=DEV)
        obs = env._obs
        for _ in range(T):
            x = torch.cat([obs.reshape(N, -1), pa, pr, pd], 1)
            h = (b + x @ wx.t() + h @ wh.t()).clamp(-1.0, 1.0)
            act = torch.distributions.Categorical(logits=bo + h @ wo.t()).sample().int()
            obs, rew, done, _ = env.step(act)
            pa, pr, pd = eye[act.long()], rew.unsqueeze(1), done.float().unsqueeze(1)
    return run


def bandit_rows(args, out):
    T, K, H = 256, 10, args.hidden
    rs = np.random.RandomState(H)
    w = (rs.randn(1, H, K).astype(F), rs.randn(1, H).astype(F), rs.randn(1, H).astype(F), (rs.randn(1, H, H) / np.sqrt(H)).astype(F),
         (0.1 * rs.randn(1, H)).astype(F), (rs.randn(1, K, H) / np.sqrt(H)).astype(F), (0.1 * rs.randn(1, K)).astype(F))
    greedy, sampled = BanditPolicy(*w), BanditPolicy(*w, temperature=np.ones(1, F))
    net = BanditPolicyNet.from_policy(sampled).to(DEV)
    for N in args.sizes:
        env = Bandits(num_envs=N, arms=K, max_steps=100, device=DEV, seed=0, auto_reset=True, resample_task="Classical")
        env.set_task(env.sample_task("Classical"))
        env.reset()

        def train():
            res = env.rollout_policy(sampled, T, record=True)
            logits = net.replay(res.actions, res.reward, res.done)
            net.zero_grad()
            (-(log_prob(logits, res.actions, 1.0) * res.reward).mean()).backward()
        t_greedy = timed(lambda: env.rollout_policy(greedy, T), args.repeats)
        t_sampled = timed(lambda: env.rollout_policy(sampled, T), args.repeats)
        t_record = timed(lambda: env.rollout_policy(sampled, T, record=True), args.repeats)
        t_train = timed(train, max(1, args.repeats // 2))
        t_loop = timed(bandit_categorical_loop(env, net, T), max(1, args.repeats // 2))
        row = dict(bench="bandits_sampled", gpu=torch.cuda.get_device_name(0), n_envs=N, arms=K, hidden=H, steps=T,
                   repeats=args.repeats, greedy_ms=t_greedy, sampled_ms=t_sampled, sampled_record_ms=t_record,
                   train_iteration_ms=t_train, step_loop_categorical_ms=t_loop, us_per_step_greedy=1e3 * t_greedy / T,
                   us_per_step_sampled=1e3 * t_sampled / T, us_per_step_train=1e3 * t_train / T, us_per_step_loop=1e3 * t_loop / T)
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")
        del env
        torch.cuda.empty_cache()


def maze_rows(args, out):
    T, vg, H, n = 64, 2, args.hidden, 15
    D = input_dim(vg)
    rs = np.random.RandomState(H)
    w = ((rs.randn(1, H, D) / np.sqrt(D)).astype(F), (rs.randn(1, H, H) / np.sqrt(H)).astype(F), (0.1 * rs.randn(1, H)).astype(F),
         (rs.randn(1, 4, H) / np.sqrt(H)).astype(F), (0.1 * rs.randn(1, 4)).astype(F))
    greedy, sampled = MazePolicy(*w), MazePolicy(*w, temperature=np.ones(1, F))
    net = MazePolicyNet.from_policy(sampled).to(DEV)
    table = MAZE_TASK_MANAGER.sample_tasks_device(64, device=DEV, seed=0, n=n, allow_loops=True, step_reward=-0.01, goal_reward=1.0)
    for N in args.sizes:
        env = metagym_amd.make("meta-maze-2D-v0", num_envs=N, device=DEV, max_steps=50, task_type="ESCAPE", view_grid=vg,
                               auto_reset=True)
        env.set_task(table)
        env.reset()

        def train():
            obs0 = env._obs.clone()
            res = env.rollout_policy(sampled, T, record=True, obs_every=1)
            logits = net.replay(obs0, res.obs, res.actions, res.reward, res.done)
            net.zero_grad()
            (-(log_prob(logits, res.actions, 1.0) * res.reward).mean()).backward()
        t_greedy = timed(lambda: env.rollout_policy(greedy, T), args.repeats)
        t_sampled = timed(lambda: env.rollout_policy(sampled, T), args.repeats)
        t_record = timed(lambda: env.rollout_policy(sampled, T, record=True, obs_every=1), args.repeats)
        t_train = timed(train, max(1, args.repeats // 2))
        t_loop = timed(maze_categorical_loop(env, net, T), max(1, args.repeats // 2))
        row = dict(bench="maze_sampled", gpu=torch.cuda.get_device_name(0), n_envs=N, maze=n, view_grid=vg, hidden=H, steps=T,
                   repeats=args.repeats, greedy_ms=t_greedy, sampled_ms=t_sampled, sampled_record_ms=t_record,
                   train_iteration_ms=t_train, step_loop_categorical_ms=t_loop, us_per_step_greedy=1e3 * t_greedy / T,
                   us_per_step_sampled=1e3 * t_sampled / T, us_per_step_train=1e3 * t_train / T, us_per_step_loop=1e3 * t_loop / T)
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")
        del env
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    for sub, name, rows in (("bandits", "bench_bandits_sampled.jsonl", bandit_rows), ("maze", "bench_maze_sampled.jsonl", maze_rows)):
        os.makedirs(os.path.join(args.out_dir, sub), exist_ok=True)
        with open(os.path.join(args.out_dir, sub, name), "a") as out:
            rows(args, out)


if __name__ == "__main__":
    main()
