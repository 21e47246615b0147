"""The rule-based dispatcher and the rollout without a GPU: the restatement (tests/liftsim_rule_oracle.py) driving the
host LiftSim (tests/liftsim_oracle.py) reproduces the golden runs of the unmodified reference dispatcher on the
unmodified reference LiftSim (tests/golden/liftsim_rule.npz), and the new entry points check their arguments."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import liftsim_oracle as O
import liftsim_rule_oracle as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CONF = {  # the reference's tests/conf/config<i>.ini
    1: dict(dt=0.5, floors=2, elevators=1, particle_number=12, generation_interval=150.0),
    2: dict(dt=0.3, floors=100, elevators=20, particle_number=12, generation_interval=150.0),
    3: dict(dt=1.0, floors=10, elevators=4, particle_number=12, generation_interval=15.0),
    4: dict(dt=0.1, floors=10, elevators=4, particle_number=11, generation_interval=150.0),
}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "liftsim_rule.npz"))


@pytest.fixture(scope="module")
def flow():
    return np.load(os.path.join(GOLD, "liftsim_flow.npy"))


def records_digest(h, actions, reward, time_consume, energy_consume, given_up):
    """One step of the fixture's `digest_records`."""
    h.update(np.asarray(actions, np.int32).tobytes())
    h.update(np.array([reward, time_consume, energy_consume], np.float64).tobytes())
    h.update(np.array([given_up], np.int64).tobytes())


def _replay(golden, name, cfg):
    steps, seed = int(golden[name + "_steps"]), int(golden[name + "_seed"])
    env = O.Env(cfg, seed)
    wins = [(int(a), int(b)) for a, b in golden[name + "_windows"]]
    checks = [int(k) for k in golden[name + "_check_steps"]]
    every = [n for n in (3600, 1000) if "%s_acc%d" % (name, n) in golden.files]
    acc, accs = {n: 0.0 for n in every}, {n: [] for n in every}
    h, h_rec = hashlib.sha256(), hashlib.sha256()
    stats = {}
    for k in range(steps):
        a = R.policy(env.mansion_state(), stats)
        r, info = env.step(a)
        s = env.mansion_state()
        h.update(np.asarray(a, np.int32).tobytes())
        O.step_digest(h, r, info, s)
        records_digest(h_rec, a, r, info["time_consume"], info["energy_consume"], info["given_up_persons"])
        for n in every:
            acc[n] += r
            if (k + 1) % n == 0:
                accs[n].append(acc[n])
                acc[n] = 0.0
        for w, (lo, hi) in enumerate(wins):
            if lo <= k < hi:
                assert a == golden["%s_w%d_actions" % (name, w)][k - lo].tolist(), k
                assert r == golden["%s_w%d_reward" % (name, w)][k - lo], k
                assert [info["time_consume"], info["energy_consume"], info["given_up_persons"]] == \
                    golden["%s_w%d_info" % (name, w)][k - lo].tolist(), k
        if k + 1 in checks:
            j = checks.index(k + 1)
            st, up, down = O.state_array(s)
            np.testing.assert_array_equal(st, golden[name + "_check_state"][j])
            np.testing.assert_array_equal(up, golden[name + "_check_up"][j])
            np.testing.assert_array_equal(down, golden[name + "_check_down"][j])
    assert h.hexdigest() == str(golden[name + "_digest"])
    assert h_rec.hexdigest() == str(golden[name + "_digest_records"])
    for n in every:
        assert accs[n] == golden["%s_acc%d" % (name, n)].tolist()
    assert env.statistics() == json.loads(str(golden[name + "_statistics"]))
    py = env.py.getstate()
    assert list(py[1][:624]) == golden[name + "_py_key"].tolist() and py[1][624] == int(golden[name + "_py_pos"])
    st = env.np.get_state()
    np.testing.assert_array_equal(st[1], golden[name + "_np_key"])
    assert st[2] == int(golden[name + "_np_pos"])
    # the restatement saw what the trace of the reference saw
    ev = json.loads(str(golden[name + "_events"]))
    for n in ("assign_up", "assign_down", "assign_zero", "fallback_up", "fallback_down", "displace_up", "displace_down",
              "displace_zero_up", "displace_zero_down", "reserved_bonus", "calls_with_displacement"):
        assert stats.get(n, 0) == ev[n], n
    assert stats["max_taken"] == ev["max_dequeues"] and stats["max_line"] == ev["max_line"] <= cfg.E
    return env


@pytest.mark.parametrize("seed", [0, 1])
def test_rule_oracle_reproduces_the_custom_day(golden, flow, seed):
    env = _replay(golden, "custom_%d" % seed, O.Config(flow=flow))
    assert env.max_queue <= 128   # the default queue_capacity holds the day under this dispatcher too
    assert len(golden["custom_%d_acc3600" % seed]) == 48


@pytest.mark.parametrize("i", [1, 2, 3, 4])
def test_rule_oracle_reproduces_the_uniform_configs(golden, i):
    env = _replay(golden, "uniform%d_3" % i, O.Config(generator="UNIFORM", **CONF[i]))
    assert env.max_queue <= 128


def test_golden_runs_cover_the_policy(golden):
    runs = json.loads(str(golden["runs"]))
    assert runs == ["custom_0", "custom_1", "uniform1_3", "uniform2_3", "uniform3_3", "uniform4_3"]
    ev = [json.loads(str(golden[n + "_events"])) for n in runs]

    def total(k):
        return sum(e[k] for e in ev)
    # each Direction branch takes a call; both fallbacks; a displacement (more dequeues than elevators in one call), one of
    # them in the Direction == 0 branch, on either side; the already-reserved bonus
    for k in ("assign_up", "assign_down", "assign_zero", "fallback_up", "fallback_down", "calls_with_displacement",
              "displace_up", "displace_down", "displace_zero_up", "displace_zero_down", "reserved_bonus"):
        assert total(k) > 0, k
    assert total("idle") > 0 and total("down_indicator") > 0
    assert max(e["max_queue"] for e in ev) >= 40
    assert all(e["max_queue"] <= 128 for e in ev)
    # the FIFO never held more entries than there are elevators (the device's ring is sized by that)
    assert all(e["max_line"] <= E for e, E in zip(ev, (4, 4, 1, 20, 4, 4)))
    assert max(e["max_dequeues"] for e in ev) == 32


def test_rule_oracle_quirks():
    S, Ev = O.MansionState, O.ElevatorState

    def el(floor, vel, direction, reserved=()):
        return Ev(floor, 10, vel, 2.0, direction, 0.0, 0, 1, 0.0, 1600, list(reserved), 0.0, False, False)
    # the down branch answers with indicator +1; nothing to do is (0, 1)
    assert R.policy(S([el(5.0, 0.0, -1), el(1.0, 0.0, 1)], [], [3])) == [3, 1, 0, 1]
    # a fallback: moving up with only a down call below takes it with indicator -1
    assert R.policy(S([el(5.0, 0.0, 1)], [], [3])) == [3, -1]
    # Direction 0: the displaced elevator keeps its stale action when its next bid finds nothing.
    # Elevator 0 (idle at 1) takes the up call at 3; elevator 1 (idle at 2.5) is nearer, takes it and elevator 0 bids
    # again: nothing it can beat, so its (3, 1) stays
    assert R.policy(S([el(1.0, 0.0, 0), el(2.5, 0.0, 0)], [3], [])) == [3, 1, 3, 1]
    # in the up branch the loser goes back to (0, 1)
    assert R.policy(S([el(1.0, 1.0, 1), el(2.5, 1.0, 1)], [3], [])) == [0, 1, 3, 1]


def test_new_entry_points_check_their_arguments():
    from metagym_amd import _lib as L
    lib = L.load()
    assert lib.mg_abi_version() == 10 == L.ABI_VERSION

    def cfg(**kw):
        c = L.LiftsimConfig()
        c.floors, c.elevators, c.queue_capacity, c.window, c.dt, c.floor_height = 10, 4, 128, 1200, 0.5, 4.0
        c.generator, c.particle_number, c.generation_interval = 1, 12, 150.0
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    p = C.c_void_p(8)   # never dereferenced: every call below is refused before a launch
    assert lib.mg_liftsim_rule_policy(None, 64, p, p, None) == -1001
    assert lib.mg_liftsim_rule_policy(cfg(), 64, None, p, None) == -1001
    assert lib.mg_liftsim_rule_policy(cfg(), 64, p, None, None) == -1001
    assert lib.mg_liftsim_rule_policy(cfg(), 0, p, p, None) == -1002
    assert lib.mg_liftsim_rule_policy(cfg(elevators=33), 64, p, p, None) == -1003
    A, RULE = L.LIFTSIM_POLICY_ACTIONS, L.LIFTSIM_POLICY_RULE
    none = (None,) * 5
    assert lib.mg_liftsim_rollout(None, 64, p, RULE, None, 10, p, *none, None) == -1001
    assert lib.mg_liftsim_rollout(cfg(), 64, None, RULE, None, 10, p, *none, None) == -1001
    assert lib.mg_liftsim_rollout(cfg(), 64, p, RULE, None, 10, None, *none, None) == -1001        # ret
    assert lib.mg_liftsim_rollout(cfg(), 64, p, A, None, 10, p, *none, None) == -1001              # ACTIONS needs actions
    assert lib.mg_liftsim_rollout(cfg(), 64, p, RULE, None, 0, p, *none, None) == -1002            # n_steps < 1
    assert lib.mg_liftsim_rollout(cfg(), 64, p, A, p, -3, p, *none, None) == -1002
    assert lib.mg_liftsim_rollout(cfg(), 0, p, RULE, None, 10, p, *none, None) == -1002
    assert lib.mg_liftsim_rollout(cfg(floors=1), 64, p, RULE, None, 10, p, *none, None) == -1003
    assert lib.mg_liftsim_rollout(cfg(), 64, p, 7, None, 10, p, *none, None) == -1003              # unknown policy
    assert lib.mg_liftsim_rollout(cfg(), 64, p, A, p, 10, p, None, None, None, None, p, None) == -1003
    assert b"rec_actions" in lib.mg_last_error()


def test_layout_appends_the_dispatcher_workspace():
    from metagym_amd import _lib as L
    lib = L.load()
    assert L.LIFTSIM_FIELDS[-2:] == ["rp_holder", "rp_priority"] and L.LIFTSIM_FIELDS[-3] == "st_w"
    c = L.LiftsimConfig()
    c.floors, c.elevators, c.queue_capacity, c.window, c.dt, c.floor_height = 100, 20, 128, 2000, 0.3, 4.0
    c.generator, c.particle_number, c.generation_interval = 1, 12, 150.0
    offs = (C.c_int64 * len(L.LIFTSIM_FIELDS))()
    total = C.c_int64()
    assert lib.mg_liftsim_layout(c, 100, offs, total) == 0
    o = dict(zip(L.LIFTSIM_FIELDS, offs))
    assert list(offs) == sorted(offs) and all(x % 256 == 0 for x in offs)
    assert o["rp_priority"] - o["rp_holder"] == (2 * 100 * 100 + 255) // 256 * 256           # i8 [2][F][N]
    assert total.value - o["rp_priority"] == (8 * 2 * 100 * 100 + 255) // 256 * 256            # f64 [2][F][N]
