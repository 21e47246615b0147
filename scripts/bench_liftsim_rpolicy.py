#!/usr/bin/env python3
"""liftsim-v0 closed-loop rollouts with a recurrent dispatcher on one GPU: one JSON line per workload.

    python scripts/bench_liftsim_rpolicy.py [--steps 200] [--hidden 32] [--sizes 4096,65536] [--repeats 7] [--out FILE]

The protocol of bench_liftsim_policy.py: the default config (CUSTOM, F = 10, E = 4, dt = 0.5; the flow table is
tests/golden/liftsim_flow.npy) from one arena snapshot taken at 07:30 (warm-up steps under random actions first run the
envs from midnight; the arena is put back from the snapshot, and the carry zeroed, before every pass). The same T steps
three ways: (a) `rollout_rpolicy`, one launch with the recurrent network inside the kernel; (b) `rollout_policy`, one
launch with the feed-forward network at the same H (LiftPolicy on the weights the two share); (c)
`step_torch_rpolicy_loop`, step() in a Python loop with the same recurrent network in torch between the launches (the
dense form: one-hot inputs and two matrix products; it is timed, not bit-compared, since its sums associate differently).
Each runs with one policy id for all envs (every wave stages it in LDS) and with ids mixed inside every wave (per-lane
reads from global memory). Each way makes one untimed pass and then `--repeats` timed ones, by HIP events around the whole
T steps; a line reports the median per step with the minimum and maximum over the repeats."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_liftsim_policy as B                                   # noqa: E402  (_actions, FLOW, the shared protocol)

NAMES = ("ws", "we", "wt", "wr", "wu", "wd", "wc", "wq", "wh", "b", "wo", "bo")


def random_policy(P, H, F, E, seed):
    from metagym_amd.liftsim import LiftRecurrentPolicy
    rs = np.random.RandomState(seed)
    A = 2 * F + 2
    shapes = dict(ws=(P, H, 8), we=(P, H, E), wt=(P, H, F + 1), wr=(P, H, F), wu=(P, H, F), wd=(P, H, F), wc=(P, H, A),
                  wq=(P, H), wh=(P, H, H), b=(P, H), wo=(P, A, H), bo=(P, A))
    sigma = dict(wh=0.5 / np.sqrt(H))
    return LiftRecurrentPolicy(**{k: (sigma.get(k, 0.5) * rs.standard_normal(shapes[k])).astype(np.float32) for k in NAMES})


class TorchRecurrentPolicy(object):
    """The network of a LiftRecurrentPolicy in torch, dense: per (env, elevator) the input vector [8 scalars | elevator
    one-hot | dispatch-target one-hot | reserved bits | up calls | down calls | previous-choice one-hot | previous reward |
    memory], then clamp(W1 x + b, -1, 1) and W2 h + bo. With one id a plain matrix product, with mixed ids a batched one
    over per-env weights gathered before the timed region. The carry (h, prev_choice, prev_reward) lives in torch tensors."""

    def __init__(self, pol, ids, device, N):
        import torch
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.F, self.E, self.H, self.A = pol.floors, pol.elevators, pol.hidden, pol.choices
        w1 = t(np.concatenate([pol.ws, pol.we, pol.wt, pol.wr, pol.wu, pol.wd, pol.wc, pol.wq[:, :, None], pol.wh], axis=2))
        b, w2, bo = t(pol.b), t(pol.wo), t(pol.bo)
        ids = torch.as_tensor(ids, device=device).long()
        self.one = bool((ids == ids[0]).all())
        if self.one:
            q = int(ids[0])
            self.w1, self.b, self.w2, self.bo = w1[q].t().contiguous(), b[q], w2[q].t().contiguous(), bo[q]
        else:
            self.w1, self.b = w1[ids].transpose(1, 2).contiguous(), b[ids][:, None, :]
            self.w2, self.bo = w2[ids].transpose(1, 2).contiguous(), bo[ids][:, None, :]
        self.scale = t(pol.scale)
        self.eye = torch.eye(self.E, device=device)
        self.h = torch.zeros(N, self.E, self.H, device=device)
        self.pc = torch.full((N, self.E), -1, dtype=torch.long, device=device)
        self.pr = torch.zeros(N, device=device)

    def reset(self):
        self.h.zero_()
        self.pc.fill_(-1)
        self.pr.zero_()

    def __call__(self, env):
        import torch
        F, E, A, N = self.F, self.E, self.A, env.num_envs
        f32 = torch.float32
        x = torch.stack([env.floor.to(f32), env.velocity.to(f32), env.direction.to(f32), env.door_state.to(f32),
                         env.load_weight.to(f32), env.overloaded_alarm.to(f32), env.door_is_opening.to(f32),
                         env.door_is_closing.to(f32)], dim=2) * self.scale
        d = env.dispatch_target.long()
        ok = (d >= 0) & (d <= F)
        target = torch.nn.functional.one_hot(d.clamp(0, F), F + 1).to(f32) * ok[:, :, None]
        listed = torch.arange(F, device=d.device)[None, None, :] < env.reserved_count[:, :, None]
        member = torch.zeros(N, E, F + 1, device=d.device)
        member.scatter_(2, torch.where(listed, env.reserved_target_floors, 0).long(), 1.0)
        up = env.requiring_upward.to(f32)[:, None, :].expand(N, E, F)
        down = env.requiring_downward.to(f32)[:, None, :].expand(N, E, F)
        chosen = torch.nn.functional.one_hot(self.pc.clamp(0, A - 1), A).to(f32) * (self.pc >= 0)[:, :, None]
        pr = self.pr[:, None, None].expand(N, E, 1)
        v = torch.cat([x, self.eye[None].expand(N, E, E), target, member[:, :, 1:], up, down, chosen, pr, self.h], dim=2)
        if self.one:
            self.h = (v @ self.w1 + self.b).clamp(-1.0, 1.0)
            c = (self.h @ self.w2 + self.bo).argmax(2)
        else:
            self.h = (torch.bmm(v, self.w1) + self.b).clamp(-1.0, 1.0)
            c = (torch.bmm(self.h, self.w2) + self.bo).argmax(2)
        self.pc = c
        tf = torch.where(c < F, c + 1, torch.where(c < 2 * F, c - F + 1, torch.where(c == 2 * F, 0, -1)))
        dr = torch.where((c >= F) & (c < 2 * F), -1, 1)
        return torch.stack([tf, dr], dim=2).reshape(N, 2 * E).to(torch.int32)

    def observed(self, env):
        self.pr = env.reward.to(self.pr.dtype)


def bench(N, T, H, repeats, start_steps):
    import torch
    from metagym_amd.liftsim import LiftPolicy, LiftPolicyState, LiftSim
    env = LiftSim(num_envs=N, seed=0, flow=np.load(B.FLOW))
    pre = B._actions(256, N, env.F, env.E, 1)
    for k in range(0, start_steps, 256):               # run the day up to the rush, 256 steps a launch
        env.rollout(pre[:min(256, start_steps - k)], record=())
    snap = env.arena.clone()
    P = 8
    pol = random_policy(P, H, env.F, env.E, 3)
    mlp = LiftPolicy(pol.ws, pol.we, pol.wt, pol.wr, pol.wu, pol.wd, pol.b, pol.wo, pol.bo)
    pol.to(env.device)
    mlp.to(env.device)
    state = LiftPolicyState.zeros(N, env.E, H, env.device)
    id_sets = {"one_id": torch.zeros(N, dtype=torch.int32, device=env.device),
               "mixed_ids": (torch.arange(N, device=env.device) % P).to(torch.int32)}
    ways = []
    for kind, ids in id_sets.items():
        tp = TorchRecurrentPolicy(pol, ids, env.device, N)

        def recurrent_launch(ids=ids):
            env.rollout_policy(pol, T, policy_ids=ids, state=state)

        def mlp_launch(ids=ids):
            env.rollout_policy(mlp, T, policy_ids=ids)

        def torch_loop(tp=tp):
            for _ in range(T):
                env.step(tp(env))
                tp.observed(env)
        ways += [("rollout_rpolicy_%s" % kind, recurrent_launch, None), ("rollout_policy_%s" % kind, mlp_launch, None),
                 ("step_torch_rpolicy_loop_%s" % kind, torch_loop, tp)]
    lines = []
    for name, fn, tp in ways:
        ms = []
        for r in range(repeats + 1):                   # the first pass is the warm-up
            env.arena.copy_(snap)
            state.h.zero_()
            state.prev_choice.fill_(-1)
            state.prev_reward.zero_()
            if tp is not None:
                tp.reset()
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
        lines.append(dict(workload="%s_N%d" % (name, N), num_envs=N, hidden=H, n_policies=P, steps_per_launch=T,
                          repeats=repeats, time_ms_per_step=med, min_ms_per_step=min(ms), max_ms_per_step=max(ms),
                          env_steps_per_s=N / (med * 1e-3), start_step=start_steps, flagged_envs=flags,
                          device=torch.cuda.get_device_name()))
        print(json.dumps(lines[-1]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--start", type=int, default=54000)    # 07:30 at dt = 0.5
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [ln for n in a.sizes.split(",") for ln in bench(int(n), a.steps, a.hidden, a.repeats, a.start)]
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
