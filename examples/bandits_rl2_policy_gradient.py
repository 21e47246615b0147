"""RL^2 on bandits-v0 with a policy gradient: REINFORCE with Adam on the fast path.

    python examples/bandits_rl2_policy_gradient.py [--tasks 4096] [--arms 10] [--pulls 100] [--hidden 32] [--iterations 200]

One recurrent policy is trained to explore and exploit inside a trial of `--pulls` pulls on a hidden Classical task (Duan et
al. 2016, "RL^2"; the benchmark of SNAIL). Per iteration:

  1. one `env.rollout_policy(record=True)` launch plays a whole trial of N = `--tasks` freshly drawn tasks, the action of
     every pull SAMPLED from the policy's softmax inside the kernel (the policy has a temperature), the memory kept;
  2. one `BanditPolicyNet.replay` of the records gives the logits of every pull with autograd, `log_prob` the log-likelihood;
  3. REINFORCE: the reward to go minus its per-step mean over the envs (the baseline), divided by its per-step standard
     deviation over the envs; one Adam step; then `to_policy` repacks the weights.

The mean regret of the sampled trials is printed per iteration, after the regret of Thompson sampling, the Gittins index and
uniform-random play on tasks drawn the same way (`rollout_learner`, the learner inside the kernel)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metagym_amd.bandits import BanditLearner, BanditPolicyNet, Bandits, gittins_index_table, log_prob  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=4096)
    ap.add_argument("--arms", type=int, default=10)
    ap.add_argument("--pulls", type=int, default=100)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--dev", type=float, default=0.1, help="spread of a Classical task (mean 0.5)")
    ap.add_argument("--discount", type=float, default=0.95, help="of the Gittins index")
    ap.add_argument("--every", type=int, default=10, help="print every so many iterations")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    N, K, T, H, temp = args.tasks, args.arms, args.pulls, args.hidden, args.temperature
    dev = "cuda:0"
    env = Bandits(num_envs=N, arms=K, max_steps=T, device=dev, seed=args.seed)

    def new_trial():
        env.set_task(env.sample_task("Classical", 0.5, args.dev))
        env.reset()

    f = np.float32
    flat = np.ones((1, 2), f)
    for name, learner in (("Thompson sampling, Beta(1, 1)", BanditLearner.thompson(K, flat)),
                          ("Gittins index, discount %g" % args.discount,
                           BanditLearner.table(K, gittins_index_table(min(T, 1023), args.discount)[None, :])),
                          ("uniform-random play", BanditLearner.greedy(K, flat, epsilon=np.ones(1)))):
        new_trial()
        res = env.rollout_learner(learner, T, seed=args.seed)
        print("%-32s mean regret %6.2f  (over %d pulls, %d tasks)" % (name, res.regret.mean().item(), T, N))

    torch.manual_seed(args.seed)
    net = BanditPolicyNet(H, K).to(dev)
    with torch.no_grad():
        for name, scale in (("wa", 0.5), ("wr", 0.5), ("wh", 0.5 / np.sqrt(H)), ("wo", 0.5 / np.sqrt(H))):
            getattr(net, name).normal_(0.0, scale)
    opt = torch.optim.Adam(net.parameters(), lr=args.lr)
    for it in range(args.iterations):
        new_trial()
        res = env.rollout_policy(net.to_policy(temperature=temp), T, seed=args.seed + it, record=True)
        logits = net.replay(res.actions, res.reward, res.done)
        to_go = res.reward.flip(0).cumsum(0).flip(0)
        advantage = to_go - to_go.mean(1, keepdim=True)                     # the per-step mean over the envs as the baseline
        advantage = advantage / (advantage.std(1, keepdim=True) + 1e-6)
        loss = -(log_prob(logits, res.actions, temp) * advantage).sum(0).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        if it % args.every == 0 or it == args.iterations - 1:
            print("iteration %4d: mean regret of the sampled trials %6.2f  mean return %6.2f"
                  % (it, res.regret.mean().item(), res.ret_total.mean().item()))


if __name__ == "__main__":
    main()
