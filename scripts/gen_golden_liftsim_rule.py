#!/usr/bin/env python3
"""Golden runs of the reference's rule-based dispatcher driving the reference's LiftSim -> tests/golden/liftsim_rule.npz.

TEST INFRASTRUCTURE; runs only where the reference tree is available (imported through oracle/refstubs, pyglet replaced
by a stand-in, like scripts/gen_golden_liftsim.py). The unmodified Rule_dispatcher.policy
(metagym/liftsim/tests/rule_benchmark/dispatcher.py) picks every action of the unmodified LiftSim, as run_dispacher does:
  - custom_<s>: the default config (CUSTOM, mansion_flow.npy), env.seed(s), a whole day (172 800 steps), s = 0, 1;
  - uniform<i>_3: the reference's tests/conf/config<i>.ini (UNIFORM), env.seed(3), 6 000 steps, i = 1..4.
Per run: a SHA-256 over every step's actions, reward, info and hall buttons (`digest`), and one over the actions, reward
and info alone (`digest_records`: what a rollout launch records per step; it has no per-step buttons); actions, reward and info of the windows
liftsim.npz uses; the full state every CHECK steps (14 400 of the day, 1 000 of a UNIFORM run); the accumulated reward
(acc = 0.0; acc += reward) per 3 600 steps, and per 1 000 for the UNIFORM runs; the final statistics and both streams; and
event counts.

The events are counted by watching, not by editing the dispatcher: a trace function sees which lines of `policy` run
(EVENT_LINES names them by number; nothing of the file's text is kept), and the dispatcher's queue is counted through a
stand-in `queue` module that forwards to the real one. The same events are counted by the restatement in
tests/liftsim_rule_oracle.py, which is run on every state next to the reference: its actions and its counts must equal
the reference's at every step, or the generator stops.

    python scripts/gen_golden_liftsim_rule.py
"""
import hashlib
import json
import multiprocessing
import os
import queue as real_queue
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden  # noqa: E402  (reference import shims)
import gen_golden_liftsim as G  # noqa: E402  (the pyglet stand-in)
import liftsim_oracle as O  # noqa: E402
import liftsim_rule_oracle as R  # noqa: E402

DAY = 172800
WINDOWS = [(0, 2000), (57600, 59600)]
UNIFORM_STEPS = 6000
HOUR = 3600
# line of Rule_dispatcher.policy -> the event its execution means
EVENT_LINES = {74: "dequeue", 85: "reserved_bonus", 130: "reserved_bonus", 93: "assign_up", 97: "displace_up",
               113: "fallback_up", 138: "assign_down", 142: "displace_down", 158: "fallback_down", 188: "assign_zero",
               192: "displace_zero_up", 198: "displace_zero_down"}
MUST_OCCUR = ("assign_up", "assign_down", "assign_zero", "fallback_up", "fallback_down", "calls_with_displacement",
              "displace_zero", "reserved_bonus")


class _Watch(object):
    """Counts the lines of EVENT_LINES as `code` runs them. A statement that spans several lines reports its first line
    again when its last one is done, so a line counts only when the line before it was not one of the next three."""

    def __init__(self, code):
        self.code, self.ev, self.prev = code, {}, -1

    def glob(self, frame, event, arg):
        if frame.f_code is self.code:
            self.prev = -1
            return self.local
        return None

    def local(self, frame, event, arg):
        if event == "line":
            ln = frame.f_lineno
            name = EVENT_LINES.get(ln)
            if name is not None and not ln <= self.prev <= ln + 3:
                self.ev[name] = self.ev.get(name, 0) + 1
            self.prev = ln
        return self.local


class _CountingQueue(real_queue.Queue):
    puts = gets = 0

    def put(self, *a, **kw):
        _CountingQueue.puts += 1
        return real_queue.Queue.put(self, *a, **kw)

    def get(self, *a, **kw):
        _CountingQueue.gets += 1
        return real_queue.Queue.get(self, *a, **kw)


def records_digest(h, actions, reward, time_consume, energy_consume, given_up):
    """Feed one step's records into a hashlib object."""
    h.update(np.asarray(actions, np.int32).tobytes())
    h.update(np.array([reward, time_consume, energy_consume], np.float64).tobytes())
    h.update(np.array([given_up], np.int64).tobytes())


def _run(job):
    name, config_file, seed, steps, windows, check, acc_every = job
    gen_golden._import_reference()
    G._pyglet_stand_in()
    from metagym.liftsim.environment.env import LiftSim
    from metagym.liftsim.tests.rule_benchmark import dispatcher as D
    q = types.ModuleType("queue")
    q.Queue = _CountingQueue
    D.queue = q
    env = LiftSim() if config_file is None else LiftSim(config_file=config_file)
    E = env.attribute.ElevatorNumber
    env.seed(seed)
    env.reset()
    disp = D.Rule_dispatcher(env, steps)
    watch = _Watch(D.Rule_dispatcher.policy.__code__)
    ours = {}
    h, h_rec = hashlib.sha256(), hashlib.sha256()
    rec = {}
    win = [(a, min(b, steps)) for a, b in windows if a < steps]
    for w, (a, b) in enumerate(win):
        rec["w%d_reward" % w] = np.zeros(b - a)
        rec["w%d_info" % w] = np.zeros((b - a, 3))
        rec["w%d_actions" % w] = np.zeros((b - a, 2 * E), np.int16)
    states, accs = [], {n: [] for n in acc_every}
    acc = {n: 0.0 for n in acc_every}
    ev = dict(max_queue=0, max_dequeues=0, calls_with_displacement=0, idle=0, down_indicator=0)
    for k in range(steps):
        state = env.state
        g0 = _CountingQueue.gets
        sys.settrace(watch.glob)
        try:
            action = disp.policy(state)
        finally:
            sys.settrace(None)
        taken = _CountingQueue.gets - g0
        flat = [int(x) for a in action for x in (a.TargetFloor, a.DirectionIndicator)]
        assert flat == R.policy(state, ours), (name, k)
        ev["max_dequeues"] = max(ev["max_dequeues"], taken)
        ev["calls_with_displacement"] += taken > E
        ev["idle"] += sum(1 for a in action if a.TargetFloor == 0)
        ev["down_indicator"] += sum(1 for a in action if a.DirectionIndicator == -1)
        s, r, _, info = env.step(flat)   # env.step takes the flat list (the benchmark's wrapper flattens it)
        h.update(np.asarray(flat, np.int32).tobytes())
        O.step_digest(h, r, info, s)
        records_digest(h_rec, flat, r, info["time_consume"], info["energy_consume"], info["given_up_persons"])
        for n in acc_every:
            acc[n] += r
            if (k + 1) % n == 0:
                accs[n].append(acc[n])
                acc[n] = 0.0
        for w, (lo, hi) in enumerate(win):
            if lo <= k < hi:
                rec["w%d_reward" % w][k - lo] = r
                rec["w%d_info" % w][k - lo] = [info["time_consume"], info["energy_consume"], info["given_up_persons"]]
                rec["w%d_actions" % w][k - lo] = flat
        if (k + 1) % check == 0 or k + 1 == steps:
            st, up, down = O.state_array(s)
            states.append((k + 1, st, up, down))
        wq = env._mansion.waiting_queue
        ev["max_queue"] = max(ev["max_queue"], max(len(x) for side in wq for x in side))
    # what the trace saw is what the queue stand-in and the restatement counted
    t = watch.ev
    assert t.get("dequeue", 0) == _CountingQueue.gets == _CountingQueue.puts, (t, _CountingQueue.gets)
    displaced = sum(t.get(n, 0) for n in ("displace_up", "displace_down", "displace_zero_up", "displace_zero_down"))
    assert _CountingQueue.puts == E * steps + displaced
    for n in set(EVENT_LINES.values()) - {"dequeue"}:
        assert t.get(n, 0) == ours.get(n, 0), (name, n, t, ours)
        ev[n] = t.get(n, 0)
    assert ours["max_taken"] == ev["max_dequeues"] and ours.get("calls_with_displacement", 0) == ev["calls_with_displacement"]
    assert ours["max_line"] <= E   # the bound the device's ring is sized by
    ev["displace_zero"] = ev["displace_zero_up"] + ev["displace_zero_down"]
    ev["dequeues"] = t.get("dequeue", 0)
    ev["max_line"] = ours["max_line"]
    rec["windows"] = np.asarray(win, np.int64)
    rec["check_steps"] = np.asarray([x[0] for x in states], np.int64)
    rec["check_state"] = np.stack([x[1] for x in states])
    rec["check_up"] = np.stack([x[2] for x in states])
    rec["check_down"] = np.stack([x[3] for x in states])
    for n in acc_every:
        rec["acc%d" % n] = np.asarray(accs[n], np.float64)
    rec["digest"] = np.str_(h.hexdigest())
    rec["digest_records"] = np.str_(h_rec.hexdigest())
    rec["statistics"] = np.str_(json.dumps(env.statistics))
    py = random.getstate()
    rec["py_key"] = np.asarray(py[1][:624], np.uint32)
    rec["py_pos"] = np.int64(py[1][624])
    st = np.random.get_state()
    rec["np_key"] = st[1]
    rec["np_pos"] = np.int64(st[2])
    rec["steps"] = np.int64(steps)
    rec["seed"] = np.int64(seed)
    rec["events"] = np.str_(json.dumps({k: int(v) for k, v in ev.items()}))
    return name, rec, ev


def main():
    ref_dir = os.path.join(gen_golden.REF, "metagym", "liftsim")
    jobs = [("custom_%d" % s, None, s, DAY, WINDOWS, 14400, (HOUR,)) for s in (0, 1)]
    jobs += [("uniform%d_3" % i, os.path.join(ref_dir, "tests", "conf", "config%d.ini" % i), 3, UNIFORM_STEPS,
              [(0, UNIFORM_STEPS)], 1000, (HOUR, 1000)) for i in (1, 2, 3, 4)]
    with multiprocessing.Pool(len(jobs)) as pool:   # one process per run: the reference's streams are module globals
        done = pool.map(_run, jobs, chunksize=1)
    out = {"numpy_version": np.str_(np.__version__), "runs": np.str_(json.dumps(sorted(n for n, _, _ in done)))}
    total = {}
    for name, rec, ev in done:
        print(name, ev)
        for k, v in rec.items():
            out["%s_%s" % (name, k)] = v
        for k, v in ev.items():
            total[k] = total.get(k, 0) + v
    missing = [k for k in MUST_OCCUR if not total.get(k, 0) > 0]
    assert not missing, "the runs do not cover: %s" % missing
    dst = os.path.join(ROOT, "tests", "golden", "liftsim_rule.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
