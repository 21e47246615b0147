"""Quadrotor one-wave step (STEP_STOCK_SHADOW): what the whole-step fallback costs a batch that sits at a folded failure
edge, against the headline batch.

    METAGYM_HIP_LIB=<lib> python scripts/quad_lean_threshold.py

Two batches of 65 536 envs, hovering_control with fused auto-reset, each timed over STEPS eager steps:
  headline  the stock config after PREROLL steps, U(0.1, 15) actions (bench.py's workload)
  parked    every env hovers at rest at p = (pos_safe32 + 1, 0, 0.5) on the voltage that holds its rotor speed: no env
            fails, and every wave redoes every step with the full failure tests (the documented worst case)
Prints one JSON line: microseconds per step for each batch, and how many envs of the parked batch ended an episode.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import metagym_amd  # noqa: E402
from metagym_amd import _lib  # noqa: E402

N = int(os.environ.get("QN", "65536"))
PREROLL = int(os.environ.get("PREROLL", "1000"))
STEPS = int(os.environ.get("STEPS", "400"))
HOVER_W, HOVER_V = 282.2, 4.982   # rotor speed with 4 * ct0 * w^2 = quality * 9.8, and the voltage that keeps it


def timed(env, actions):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(STEPS):
        env.step(actions[i % len(actions)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS * 1e3


def main():
    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    rand = [a for a in torch.rand(8, N, 4, device="cuda", generator=g) * 14.9 + 0.1]
    env = metagym_amd.make("quadrotor-v0", num_envs=N, task="hovering_control", nt=1000, auto_reset=True, seed=1)
    env.reset(seed=0)
    for i in range(PREROLL):
        env.step(rand[i % len(rand)])
    headline = timed(env, rand)

    fold = _lib.QuadrotorFold()
    _lib.check(_lib.load().mg_quadrotor_plan_fold(env._plan, fold), "mg_quadrotor_plan_fold")
    sd = env.state_dict()
    episodes_before = sd["episode"].clone()
    parked = dict(sd)
    parked["pos"] = torch.zeros_like(sd["pos"])
    parked["pos"][0] = fold.pos_safe32 + 1.0
    parked["pos"][2] = 0.5
    parked["vel"] = torch.zeros_like(sd["vel"])
    parked["omega"] = torch.zeros_like(sd["omega"])
    parked["propw"] = torch.full_like(sd["propw"], HOVER_W)
    rot = torch.zeros_like(sd["rot"])
    rot[0] = rot[4] = rot[8] = 1.0
    parked["rot"] = rot
    parked["ct"] = torch.zeros_like(sd["ct"])
    env.load_state_dict({k: v for k, v in parked.items() if torch.is_tensor(v)})
    parked_us = timed(env, [torch.full((N, 4), HOVER_V, device="cuda")])
    ended = int((env.state_dict()["episode"] != episodes_before).sum())
    print(json.dumps({"lib": os.path.basename(_lib.lib_path()), "n": N, "steps": STEPS, "one_wave_form": fold.one_wave_form,
                      "pos_safe32": fold.pos_safe32, "headline_us": headline, "parked_us": parked_us,
                      "parked_envs_that_ended": ended}), flush=True)


if __name__ == "__main__":
    main()
