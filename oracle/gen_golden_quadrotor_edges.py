#!/usr/bin/env python3
"""Golden vectors for the quadrotor's clamp and failure edges, recorded from the UNMODIFIED reference.

TEST INFRASTRUCTURE; runs only in the build container (needs the reference tree):

    python oracle/gen_golden_quadrotor_edges.py

One `env.step` (task='hovering_control', 10 sub-steps) per case, from a state set on the simulator as
`_quadrotor_fail` in gen_golden.py does, under a simulator config that differs from config.json only in
`fail.*` and `electric.*`:
  * actions at the clamp (quadrotorsim.py:130-134): exactly min_voltage / max_voltage as f32, one f32 ulp on
    each side, 0, -0.0, negative values, +-FLT_MAX, +-inf, and a config with min_voltage == max_voltage;
  * fail.range of -1, -0.0, 0, inf and 1e39 (rounds to inf as f32); fail.velocity and fail.w of -1, 0 and inf,
    each from a calm state and from one that fails under config.json's thresholds.
Recorded: the failure code (1 range, 2 velocity, 3 body rate: which message `_check_failure`, quadrotorsim.py:212-221,
raised; 0 none), the simulator state after the step (at the raise for a failure), and obs / reward / done of a step
that did not raise. NaN actions are not recorded: `_check_collision` raises ValueError on them (int(floor(nan))).
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "quadrotor_edges.npz")
sys.path.insert(0, HERE)

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
INF = float("inf")


def _up(x):
    return float(np.nextafter(F32(x), F32(INF)))


def _down(x):
    return float(np.nextafter(F32(x), F32(-INF)))


# the action values of the clamp cases (all exactly representable as f32)
CLAMP_VALUES = [float(F32(0.1)), _down(0.1), _up(0.1), 15.0, _down(15.0), _up(15.0), 0.0, -0.0, -1.0, -15.0,
                FLT_MAX, -FLT_MAX, INF, -INF]

CALM = ([1.5, -2.0, 0.75], [0.5, -0.25, 0.3], [0.2, -0.1, 0.3])      # pos, vel, omega: fails nothing by default
FAR = ([600.0, 800.0, 0.5], [3.0, 4.0, 0.0], [0.1, 0.0, 0.0])        # |pos| = 1000.0001: range at sub-step 1
FAST = ([0.0, 0.0, 0.0], [150.0, 0.0, 0.0], [0.0, 0.0, 0.0])         # velocity
SPIN = ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1500.0, 0.0, 0.0])        # body rate
PROPW = [300.0, 310.0, 290.0, 305.0]


def cases():
    """(fail_range, fail_velocity, fail_w, min_voltage, max_voltage, (pos, vel, omega), action[4])"""
    d = (1000.0, 100.0, 1000.0, 0.10, 15.0)
    out = []
    for v in CLAMP_VALUES:
        out.append(d + (CALM, [v, v, v, v]))
    out.append(d + (CALM, [float(F32(0.1)), 15.0, -INF, INF]))
    out.append(d + (CALM, [_down(0.1), _up(15.0), -0.0, FLT_MAX]))
    for a in ([0.5, 2.0, 10.0, INF], [-INF, 2.0, _up(2.0), _down(2.0)]):
        out.append((1000.0, 100.0, 1000.0, 2.0, 2.0, CALM, a))
    for r in (-1.0, -0.0, 0.0, INF, 1e39):
        for st in (CALM, FAR):
            out.append((r, 100.0, 1000.0, 0.10, 15.0, st, [3.0] * 4))
    for v in (-1.0, 0.0, INF):
        for st in (CALM, FAST):
            out.append((1000.0, v, 1000.0, 0.10, 15.0, st, [3.0] * 4))
    for w in (-1.0, 0.0, INF):
        for st in (CALM, SPIN):
            out.append((1000.0, 100.0, w, 0.10, 15.0, st, [3.0] * 4))
    return out


def sim_config(base, fail_range, fail_velocity, fail_w, min_v, max_v):
    cfg = json.loads(json.dumps(base))
    cfg["fail"] = {"velocity": fail_velocity, "w": fail_w, "range": fail_range}
    cfg["electric"] = {"min_voltage": min_v, "max_voltage": max_v}
    return cfg


CODES = [("exists the valid zone", 1), ("too large velocity to recover", 2), ("too large angular velocity", 3)]


def failure_code(e):
    msg = str(e)
    for text, code in CODES:
        if text in msg:
            return code
    raise e


def main():
    from gen_golden import REF, _import_reference, _sim_state
    gym = _import_reference()
    with open(os.path.join(REF, "metagym", "quadrotor", "config.json")) as f:
        base = json.load(f)
    keys = ("pos", "vel", "omega", "propw", "R")
    rec = {k: [] for k in ["fail_range", "fail_velocity", "fail_w", "min_voltage", "max_voltage", "actions", "code",
                           "obs", "reward", "done"] + ["in_" + k for k in keys] + ["out_" + k for k in keys]}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (fr, fv, fw, lo, hi, (pos, vel, om), act) in enumerate(cases()):
            path = os.path.join(tmp, "c%d.json" % i)
            with open(path, "w") as f:
                json.dump(sim_config(base, fr, fv, fw, lo, hi), f)
            env = gym.make("quadrotor-v0", task="hovering_control", simulator_conf=path)
            env.reset()
            sim = env.simulator
            sim._zero_state()
            sim.global_position = np.array(pos, dtype=np.float32)
            sim.global_velocity = np.array(vel, dtype=np.float64)
            sim.body_angular_velocity = np.array(om, dtype=np.float64)
            sim.propeller_angular_velocity = np.array(PROPW, dtype=np.float32)
            sim._coordination_converter_to_world = sim.rotation_matrix
            sim._coordination_converter_to_body = np.linalg.inv(sim.rotation_matrix)
            env.ct = 0
            st = _sim_state(sim)
            a = np.array(act, dtype=np.float32)
            code, obs, reward, done = 0, np.zeros(16, np.float32), np.nan, True
            with np.errstate(over="ignore"):      # 1e39 as the f32 comparand of `norm > fail_range` is inf
                try:
                    o, reward, done, _info = env.step(a)
                    obs = np.asarray(o, np.float32)
                except Exception as e:            # quadrotorsim.py:212-221 raises a bare Exception
                    code = failure_code(e)
            so = _sim_state(sim)
            for k in keys:
                rec["in_" + k].append(st[k])
                rec["out_" + k].append(so[k])
            for k, v in zip(("fail_range", "fail_velocity", "fail_w", "min_voltage", "max_voltage"), (fr, fv, fw, lo, hi)):
                rec[k].append(float(v))
            rec["actions"].append(a)
            rec["code"].append(code)
            rec["obs"].append(obs)
            rec["reward"].append(np.float64(reward))
            rec["done"].append(bool(done))
    out = {k: np.asarray(v) for k, v in rec.items()}
    out["code"] = out["code"].astype(np.int32)
    out["numpy_version"] = np.str_(np.__version__)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "cases", len(out["code"]), "codes", out["code"].tolist())


if __name__ == "__main__":
    main()
