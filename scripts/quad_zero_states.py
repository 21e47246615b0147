"""Quadrotor one-wave step (STEP_STOCK_SHADOW) on batches whose states hold exact zeros, against the headline batch.

    METAGYM_HIP_LIB=<lib> python scripts/quad_zero_states.py

Three batches of 65 536 envs, hovering_control with fused auto-reset, each timed over STEPS eager steps after PREROLL:
  headline     the stock config, U(0.1, 15) actions (bench.py's workload)
  still_reset  init_velocity and init_angular_velocity noisy = 0: every reset state has v = w = 0 exactly
  equilibrium  the same config, and every rotor gets the same constant voltage: w stays exactly 0 for ever
Prints one JSON line: microseconds per step for each batch.
"""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import metagym_amd  # noqa: E402
from metagym_amd import _lib  # noqa: E402
from metagym_amd.quadrotor.env import DEFAULT_SIM_CONFIG  # noqa: E402

N = int(os.environ.get("QN", "65536"))
PREROLL = int(os.environ.get("PREROLL", "1000"))
STEPS = int(os.environ.get("STEPS", "1000"))


def time_batch(still, actions):
    kw = {}
    if still:
        cfg = json.loads(json.dumps(DEFAULT_SIM_CONFIG))
        cfg["init_velocity"]["noisy"] = 0.0
        cfg["init_angular_velocity"]["noisy"] = 0.0
        f = tempfile.NamedTemporaryFile("w", suffix=".json", delete=False)
        json.dump(cfg, f)
        f.close()
        kw["simulator_conf"] = f.name
    env = metagym_amd.make("quadrotor-v0", num_envs=N, task="hovering_control", nt=1000, auto_reset=True, seed=1, **kw)
    env.reset(seed=0)
    for i in range(PREROLL):
        env.step(actions[i % len(actions)])
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
    equal = [torch.full((N, 4), 7.5, device="cuda")]
    out = {"lib": os.path.basename(_lib.lib_path()), "n": N,
           "headline_us": time_batch(False, rand),
           "still_reset_us": time_batch(True, rand),
           "equilibrium_us": time_batch(True, equal)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
