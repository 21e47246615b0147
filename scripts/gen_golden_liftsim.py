#!/usr/bin/env python3
"""Golden LiftSim runs of the unmodified reference (metagym/liftsim/environment/env.py) -> tests/golden/liftsim.npz, and
its flow table -> tests/golden/liftsim_flow.npy.

TEST INFRASTRUCTURE; runs only where the reference tree is available (imported through oracle/refstubs like the other
golden generators; pyglet, which the reference's renderer imports, is replaced by a stand-in here). Every run is
env.seed(s); env.reset(); then scripted actions (tests/liftsim_oracle.scripted_actions), with one reset() in mid-run:
  - custom_<s>: the default config (CUSTOM, mansion_flow.npy) over a whole simulated day (172 800 steps);
  - uniform<i>_<s>: the reference's test configs conf/config<i>.ini (UNIFORM), 6000 steps.
Per run: per-step reward / info for the windows, the full state every CHECK steps, a SHA-256 of the whole per-step
stream (reward, info, buttons), the statistics and both streams at the end. Also: the CUSTOM tables the reference builds,
and the config refusals.
Each run also counts its events (rush-hour queue length, overload alarms, give-ups, target -1, direction 0, and mid-deque
deletes: a person boarding after an older one in the same pass was refused for overload); every kind must occur.
These pin tests/liftsim_oracle.py (CPU) and mg_liftsim_* (GPU) bit for bit.

    python scripts/gen_golden_liftsim.py
"""
import hashlib
import json
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden  # noqa: E402  (reference import shims)
import liftsim_oracle as O  # noqa: E402

CUSTOM_SEEDS = [0, 1]
DAY = 172800
WINDOWS = [(0, 2000), (57600, 59600)]   # the first 2000 steps and 08:00-08:16:40, the morning rush
UNIFORM_STEPS = 6000
CHECK = 10000


def _pyglet_stand_in():
    pg = types.ModuleType("pyglet")
    pg.resource = types.ModuleType("pyglet.resource")
    pg.resource.reindex = lambda: None
    pg.window = types.ModuleType("pyglet.window")
    pg.window.Window = type("Window", (object,), {})
    sys.modules.update({"pyglet": pg, "pyglet.resource": pg.resource, "pyglet.window": pg.window})


class _Boarding(object):
    """Records, without changing them, the reference's boarding calls (Elevator.person_request_in) of one step, to count
    mid-deque deletes: a person who boards after an older one in the same pass was refused for overload."""

    def __init__(self, elevator_cls):
        self.calls = {}
        orig = elevator_cls.person_request_in
        rec = self

        def wrapped(el, person):
            entering = len(el._entering_person)
            ok = orig(el, person)
            overload = not ok and entering < el._mpee_number and el._is_overloaded_alarm == 2.0
            rec.calls.setdefault(id(el), []).append("A" if ok else ("R" if overload else "O"))
            return ok
        elevator_cls.person_request_in = wrapped

    def mid_deque_deletes(self):
        n = sum(1 for seq in self.calls.values() if "R" in seq and "A" in seq[seq.index("R"):])
        self.calls = {}
        return n


def _run(env, seed, steps, windows, check, reset_at, boarding):
    F, E = env.attribute.NumberOfFloor, env.attribute.ElevatorNumber
    acts = O.scripted_actions(seed, steps, F, E)
    env.seed(seed)
    env.reset()
    h = hashlib.sha256()
    rec = {}
    win = [(a, min(b, steps)) for a, b in windows if a < steps]
    for w, (a, b) in enumerate(win):
        rec["w%d_reward" % w] = np.zeros(b - a)
        rec["w%d_info" % w] = np.zeros((b - a, 3))
    states, ev = [], dict(max_queue=0, alarm=0, give_up=0, target_minus1=0, direction0=0, mid_deque_delete=0)
    for k in range(steps):
        if k == reset_at:
            env.reset()
        a = [int(x) for x in acts[k]]
        boarding.calls = {}
        s, r, _, info = env.step(a)
        ev["mid_deque_delete"] += boarding.mid_deque_deletes()
        O.step_digest(h, r, info, s)
        for w, (lo, hi) in enumerate(win):
            if lo <= k < hi:
                rec["w%d_reward" % w][k - lo] = r
                rec["w%d_info" % w][k - lo] = [info["time_consume"], info["energy_consume"], info["given_up_persons"]]
        if (k + 1) % check == 0 or k + 1 == steps:
            st, up, down = O.state_array(s)
            states.append((k + 1, st, up, down))
        q = env._mansion.waiting_queue
        ev["max_queue"] = max(ev["max_queue"], max(len(x) for side in q for x in side))
        ev["alarm"] += any(e.OverloadedAlarm > 0 for e in s.ElevatorStates)
        ev["give_up"] += info["given_up_persons"] > 0
        ev["target_minus1"] += int((acts[k, 0::2] == -1).any())
        ev["direction0"] += int((acts[k, 1::2] == 0).any())
    rec["windows"] = np.asarray(win, np.int64)
    rec["check_steps"] = np.asarray([x[0] for x in states], np.int64)
    rec["check_state"] = np.stack([x[1] for x in states])
    rec["check_up"] = np.stack([x[2] for x in states])
    rec["check_down"] = np.stack([x[3] for x in states])
    rec["digest"] = np.str_(h.hexdigest())
    rec["statistics"] = np.str_(json.dumps(env.statistics))
    py = random.getstate()
    rec["py_key"] = np.asarray(py[1][:624], np.uint32)
    rec["py_pos"] = np.int64(py[1][624])
    st = np.random.get_state()
    rec["np_key"] = st[1]
    rec["np_pos"] = np.int64(st[2])
    rec["steps"] = np.int64(steps)
    rec["reset_at"] = np.int64(reset_at)
    rec["events"] = np.str_(json.dumps(ev))
    return rec, ev


def _raises(fn):
    try:
        fn()
    except BaseException as e:   # noqa: BLE001 — the class is what is recorded
        return type(e).__name__
    return "none"


def main():
    gen_golden._import_reference()
    _pyglet_stand_in()
    from metagym.liftsim.environment.env import LiftSim
    from metagym.liftsim.environment.mansion.elevator import Elevator
    boarding = _Boarding(Elevator)
    ref_dir = os.path.join(gen_golden.REF, "metagym", "liftsim")
    flow_path = os.path.join(ref_dir, "environment", "mansion", "person_generators", "mansion_flow.npy")
    out = {"numpy_version": np.str_(np.__version__)}
    runs = {}
    for s in CUSTOM_SEEDS:
        env = LiftSim()
        rec, ev = _run(env, s, DAY, WINDOWS, CHECK, 100000 if s == 1 else -1, boarding)
        runs["custom_%d" % s] = (rec, ev)
        if s == 0:
            g = env._mansion._person_generator
            out["ref_in_density"] = g._in_density
            out["ref_out_prob"] = g._out_prob
    for i in (1, 2, 3, 4):
        env = LiftSim(config_file=os.path.join(ref_dir, "tests", "conf", "config%d.ini" % i))
        rec, ev = _run(env, 3, UNIFORM_STEPS, [(0, UNIFORM_STEPS)], 1000, UNIFORM_STEPS // 2, boarding)
        runs["uniform%d_3" % i] = (rec, ev)
    total = {k: sum(ev[k] for _, ev in runs.values())
             for k in ("alarm", "give_up", "target_minus1", "direction0", "mid_deque_delete")}
    assert all(v > 0 for v in total.values()), total
    assert max(ev["max_queue"] for _, ev in runs.values()) >= 10
    for name, (rec, ev) in runs.items():
        for k, v in rec.items():
            out["%s_%s" % (name, k)] = v
        print(name, ev)
    out["runs"] = np.str_(json.dumps(sorted(runs)))
    out["refusals"] = np.str_(json.dumps({
        "time_step_more_than_1": _raises(lambda: LiftSim(config_file=os.path.join(
            ref_dir, "tests", "conf", "config_time_step_more_than_1.ini")))}))
    dst = os.path.join(ROOT, "tests", "golden", "liftsim.npz")
    np.savez_compressed(dst, **out)
    np.save(os.path.join(ROOT, "tests", "golden", "liftsim_flow.npy"), np.load(flow_path))
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
