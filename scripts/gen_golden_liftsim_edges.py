#!/usr/bin/env python3
"""Golden runs of the unmodified reference LiftSim at the edges of tests/liftsim_cases.py -> tests/golden/liftsim_edges.npz.

TEST INFRASTRUCTURE; runs only where the reference tree is available (imported through oracle/refstubs with the pyglet
stand-in of scripts/gen_golden_liftsim.py). Each run writes its own temporary config.ini (and, for CUSTOM, a flow .npy made
by liftsim_cases.synth_flow) and hands it to the reference's LiftSim(config_file=...):
  - custom<F>_<s>, F = 2, 9, 16, s = 0, 1: the three-row synthetic table liftsim_cases.edge_flow(F), env.seed(s), scripted actions
    (liftsim_oracle.scripted_actions) up to the step that enters the table's third row, whose rates numpy draws with PTRS.
    Per run: reward and info of every step, the state after the last one, the statistics and both streams. Per F: the
    reference's _in_density and _out_prob. Under these actions and in so few steps no run delivers anybody: the runs
    pin generation, queueing, boarding and the overload alarms at these tables, not delivery.
  - big_<s>, s = 0, 1: F = 128, E = 32, UNIFORM, under the reference's own Rule_dispatcher (the run loop of
    scripts/gen_golden_liftsim_rule.py, which also holds tests/liftsim_rule_oracle.py to the reference at every step):
    actions, reward and info of every step, the final state, statistics and streams.
A config the reference refuses is recorded in `refusals` by its exception class and has no run.

    python scripts/gen_golden_liftsim_edges.py
"""
import json
import multiprocessing
import os
import random
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden  # noqa: E402  (reference import shims)
import gen_golden_liftsim as G  # noqa: E402  (the pyglet stand-in)
import gen_golden_liftsim_rule as GR  # noqa: E402  (the dispatcher run loop)
import liftsim_cases as LC  # noqa: E402
import liftsim_oracle as O  # noqa: E402

INI = """[Configuration]
RunningTimeStep = %r
LogLevel = Notice

[MansionInfo]
Name = EdgeMansion
NumberOfFloors = %d
FloorHeight = 4.0
ElevatorNumber = %d

[PersonGenerator]
%s
"""


def write_config(tmp, name, F, E, dt, generator):
    path = os.path.join(tmp, name + ".ini")
    with open(path, "w") as f:
        f.write(INI % (dt, F, E, generator))
    return path


def _streams(rec):
    py = random.getstate()
    rec["py_key"] = np.asarray(py[1][:624], np.uint32)
    rec["py_pos"] = np.int64(py[1][624])
    st = np.random.get_state()
    rec["np_key"] = st[1]
    rec["np_pos"] = np.int64(st[2])


def _run_custom(job):
    name, config_file, F, seed, steps = job
    gen_golden._import_reference()
    G._pyglet_stand_in()
    from metagym.liftsim.environment.env import LiftSim
    try:
        env = LiftSim(config_file=config_file)
    except Exception as e:   # noqa: BLE001 -- the class is what is recorded
        return name, None, type(e).__name__
    E = env.attribute.ElevatorNumber
    acts = O.scripted_actions(seed, steps, F, E)
    env.seed(seed)
    env.reset()
    g = env._mansion._person_generator
    rec = dict(in_density=g._in_density.copy(), out_prob=g._out_prob.copy(), reward=np.zeros(steps),
               info=np.zeros((steps, 3)))
    longest = 0
    for k in range(steps):
        s, r, _, info = env.step([int(x) for x in acts[k]])
        rec["reward"][k] = r
        rec["info"][k] = [info["time_consume"], info["energy_consume"], info["given_up_persons"]]
        longest = max(longest, max(len(x) for side in env._mansion.waiting_queue for x in side))
    assert g._cur_time_index == 1, "the run must end in the table's second row"
    rec["state"], rec["up"], rec["down"] = O.state_array(s)
    rec["statistics"] = np.str_(json.dumps(env.statistics))
    rec["steps"], rec["seed"], rec["max_queue"] = np.int64(steps), np.int64(seed), np.int64(longest)
    _streams(rec)
    return name, rec, "none"


def _run_big(job):
    name, config_file, seed, steps = job
    _, rec, ev = GR._run((name, config_file, seed, steps, [(0, steps)], steps, ()))
    keep = dict(actions=rec["w0_actions"], reward=rec["w0_reward"], info=rec["w0_info"], state=rec["check_state"][-1],
                up=rec["check_up"][-1], down=rec["check_down"][-1])
    for k in ("statistics", "py_key", "py_pos", "np_key", "np_pos", "steps", "seed", "events"):
        keep[k] = rec[k]
    return name, keep, "none"


def main():
    out = {"numpy_version": np.str_(np.__version__)}
    refusals, runs = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        custom_jobs, big_jobs = [], []
        for F in (2, 9, 16):
            E, dt = LC.CUSTOM[F]
            flow_path = os.path.join(tmp, "flow%d.npy" % F)
            np.save(flow_path, LC.edge_flow(F))
            # the reference joins CustomDataFile to its own directory; an absolute path stands on its own
            ini = write_config(tmp, "custom%d" % F, F, E, dt, "PersonGeneratorType = CUSTOM\nCustomDataFile = %s" % flow_path)
            custom_jobs += [("custom%d_%d" % (F, s), ini, F, s, LC.steps_to_row2(dt)) for s in (0, 1)]
        F, E = 128, 32
        ini = write_config(tmp, "big", F, E, LC.BIG_KW["dt"], "PersonGeneratorType = UNIFORM\nParticleNumber = %d\n"
                           "GenerationInterval = %r" % (LC.BIG_KW["particle_number"], LC.BIG_KW["generation_interval"]))
        big_jobs = [("big_%d" % s, ini, s, LC.BIG[(F, E)]) for s in (0, 1)]
        with multiprocessing.Pool(8) as pool:   # one process per run: the reference's streams are module globals
            a = pool.map_async(_run_custom, custom_jobs, chunksize=1)
            b = pool.map_async(_run_big, big_jobs, chunksize=1)
            done = a.get() + b.get()
    for name, rec, refused in done:
        refusals[name] = refused
        if rec is None:
            continue
        runs.append(name)
        if name.startswith("custom"):
            table = name.split("_")[0]
            for k in ("in_density", "out_prob"):      # the same for both seeds of a table
                v = rec.pop(k)
                assert ("%s_%s" % (table, k)) not in out or np.array_equal(out["%s_%s" % (table, k)], v)
                out["%s_%s" % (table, k)] = v
        for k, v in rec.items():
            out["%s_%s" % (name, k)] = v
        print(name, {k: v for k, v in rec.items() if np.ndim(v) == 0})
    out["runs"] = np.str_(json.dumps(sorted(runs)))
    out["refusals"] = np.str_(json.dumps(refusals))
    dst = os.path.join(ROOT, "tests", "golden", "liftsim_edges.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
