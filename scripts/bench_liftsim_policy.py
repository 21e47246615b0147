#!/usr/bin/env python3
"""liftsim-v0 closed-loop rollouts with a learned dispatcher on one GPU: one JSON line per workload.

    python scripts/bench_liftsim_policy.py [--steps 200] [--hidden 32] [--sizes 4096,65536] [--repeats 7] [--out FILE]

The default config (CUSTOM, F = 10, E = 4, dt = 0.5; the flow table is tests/golden/liftsim_flow.npy) from one arena
snapshot taken at 07:30 (warm-up steps under random actions first run the envs from midnight; the arena is put back from
the snapshot before every pass). The same T steps three ways: (a) `rollout_policy`, one launch with the network inside
the kernel; (b) `step_torch_policy_loop`, step() in a Python loop with the same network in torch between the launches
(the dense form: one-hot inputs and two matrix products; it is timed, not bit-compared, since its sums associate
differently); (c) `rollout_rule`, one rollout(policy="rule") launch, the reference's baseline dispatcher. (a) and (b) run
with one policy id for all envs (every wave stages it in LDS) and with ids mixed inside every wave (per-lane reads from
global memory). Each way makes one untimed pass and then `--repeats` timed ones, by HIP events around the whole T steps; a
line reports the median per step with the minimum and maximum over the repeats."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLOW = os.path.join(ROOT, "tests", "golden", "liftsim_flow.npy")
ORDER = ("ws", "we", "wt", "wr", "wu", "wd", "b", "wo", "bo")


def _actions(reps, N, F, E, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.empty(reps, N, 2 * E, dtype=torch.int32, device="cuda")
    a[:, :, 0::2] = torch.randint(-1, F + 1, (reps, N, E), generator=g, device="cuda", dtype=torch.int32)
    a[:, :, 1::2] = torch.randint(-1, 2, (reps, N, E), generator=g, device="cuda", dtype=torch.int32)
    return a


def random_policy(P, H, F, E, seed):
    from metagym_amd.liftsim import LiftPolicy
    rs = np.random.RandomState(seed)
    A = 2 * F + 2
    shapes = dict(ws=(P, H, 8), we=(P, H, E), wt=(P, H, F + 1), wr=(P, H, F), wu=(P, H, F), wd=(P, H, F), b=(P, H), wo=(P, A, H),
                  bo=(P, A))
    return LiftPolicy(*[(0.5 * rs.standard_normal(shapes[k])).astype(np.float32) for k in ORDER])


class TorchPolicy(object):
    """The network of a LiftPolicy in torch, dense: per (env, elevator) the input vector [8 scalars | elevator one-hot |
    dispatch-target one-hot | reserved bits | up calls | down calls], then relu(W1 x + b) and W2 h + bo. With one id a plain
    matrix product, with mixed ids a batched one over per-env weights gathered before the timed region."""

    def __init__(self, pol, ids, device):
        import torch
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.F, self.E = pol.floors, pol.elevators
        w1 = t(np.concatenate([pol.ws, pol.we, pol.wt, pol.wr, pol.wu, pol.wd], axis=2))       # [P, H, D]
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

    def __call__(self, env):
        import torch
        F, E, N = self.F, self.E, env.num_envs
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
        v = torch.cat([x, self.eye[None].expand(N, E, E), target, member[:, :, 1:], up, down], dim=2)
        if self.one:
            c = (torch.relu(v @ self.w1 + self.b) @ self.w2 + self.bo).argmax(2)
        else:
            c = (torch.bmm(torch.relu(torch.bmm(v, self.w1) + self.b), self.w2) + self.bo).argmax(2)
        tf = torch.where(c < F, c + 1, torch.where(c < 2 * F, c - F + 1, torch.where(c == 2 * F, 0, -1)))
        dr = torch.where((c >= F) & (c < 2 * F), -1, 1)
        return torch.stack([tf, dr], dim=2).reshape(N, 2 * E).to(torch.int32)


def bench(N, T, H, repeats, start_steps):
    import torch
    from metagym_amd.liftsim import LiftSim
    env = LiftSim(num_envs=N, seed=0, flow=np.load(FLOW))
    pre = _actions(256, N, env.F, env.E, 1)
    for k in range(0, start_steps, 256):               # run the day up to the rush, 256 steps a launch
        env.rollout(pre[:min(256, start_steps - k)], record=())
    snap = env.arena.clone()
    P = 8
    pol = random_policy(P, H, env.F, env.E, 3)
    pol.to(env.device)
    id_sets = {"one_id": torch.zeros(N, dtype=torch.int32, device=env.device),
               "mixed_ids": (torch.arange(N, device=env.device) % P).to(torch.int32)}
    ways = []
    for kind, ids in id_sets.items():
        tp = TorchPolicy(pol, ids, env.device)

        def one_launch(ids=ids):
            env.rollout_policy(pol, T, policy_ids=ids)

        def torch_loop(tp=tp):
            for _ in range(T):
                env.step(tp(env))
        ways += [("rollout_policy_%s" % kind, one_launch), ("step_torch_policy_loop_%s" % kind, torch_loop)]
    ways.append(("rollout_rule", lambda: env.rollout(policy="rule", steps=T, record=())))
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
