"""The quadrotor's clamp and failure edges on the CPU: the oracle against the reference's own answers
(tests/golden/quadrotor_edges.npz, oracle/gen_golden_quadrotor_edges.py), and the library's config folding for
failure thresholds the range search of `fold_config` could not reach (negative, +inf as f32).

Cases: actions exactly at min_voltage / max_voltage as f32, one f32 ulp on each side, 0, -0.0, negative values,
+-FLT_MAX and +-inf; a config with min_voltage == max_voltage; fail.range of -1, -0.0, 0, inf and 1e39; fail.velocity
and fail.w of -1, 0 and inf. NaN actions are out of scope: the reference raises ValueError on them (`int(floor(nan))`
in `_check_collision`, env.py:248-260), so it defines no result to match. The GPU side of the same edges is
tests/test_quadrotor_edges_gpu.py."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import quadrotor as qo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "quadrotor_edges.npz")
THRESHOLDS = ("fail_range", "fail_velocity", "fail_w", "min_voltage", "max_voltage")
_F32 = np.float32
# the action values at the clamp (quadrotorsim.py:130-134; all exact in f32)
CLAMP = [float(_F32(0.1)), float(np.nextafter(_F32(0.1), _F32(-np.inf))), float(np.nextafter(_F32(0.1), _F32(np.inf))),
         15.0, float(np.nextafter(_F32(15.0), _F32(-np.inf))), float(np.nextafter(_F32(15.0), _F32(np.inf))),
         0.0, -0.0, -1.0, -15.0, float(np.finfo(_F32).max), -float(np.finfo(_F32).max), float("inf"), float("-inf")]


def test_golden_covers_the_edges():
    g = np.load(GOLDEN)
    acts = g["actions"]
    for v in CLAMP:
        assert (acts == _F32(v)).any(), v
    assert (np.signbit(acts) & (acts == 0)).any()                       # -0.0
    assert (g["min_voltage"] == g["max_voltage"]).any()
    for r in (-1.0, 0.0, np.inf, 1e39):
        assert (g["fail_range"] == r).any(), r
    assert (np.signbit(g["fail_range"]) & (g["fail_range"] == 0)).any()
    for k in ("fail_velocity", "fail_w"):
        for v in (-1.0, 0.0, np.inf):
            assert (g[k] == v).any(), (k, v)
    assert set(np.unique(g["code"]).tolist()) == {0, 1, 2, 3}


def test_oracle_reproduces_the_reference_at_the_edges():
    """Failure code, the state after the step (at the raise for a failure, quadrotorsim.py:210-212), and obs, reward
    and done of the steps that did not raise: bit for bit, the atan2 entries obs[12:15] within 4 ulp."""
    g = np.load(GOLDEN)
    n = len(g["code"])
    for i in range(n):
        c = case_consts(**{k: float(g[k][i]) for k in THRESHOLDS})
        st = qo.make_states(g["in_pos"][i:i + 1], g["in_vel"][i:i + 1], g["in_omega"][i:i + 1],
                            g["in_propw"][i:i + 1], g["in_R"][i:i + 1])
        ct = np.zeros(1, np.int32)
        obs, rew, done, failed = qo.batch_env_step(c, st, ct, g["actions"][i:i + 1])
        assert failed[0] == g["code"][i], i
        s = qo.states_to_arrays(st)
        for k in ("pos", "vel", "omega", "propw", "R"):
            assert np.array_equal(s[k][0], g["out_" + k][i]), (i, k)
        if failed[0]:
            assert done[0] == 1 and rew[0] == 0.0 and ct[0] == 0
            continue
        assert bool(done[0]) == bool(g["done"][i]) and rew[0] == g["reward"][i], i
        nonang = [j for j in range(16) if j not in (12, 13, 14)]
        assert np.array_equal(obs[0, nonang], g["obs"][i, nonang]), i
        assert np.max(np.abs(obs[0, 12:15] - g["obs"][i, 12:15])) <= 4 * np.spacing(np.float32(np.pi)), i


# Run in a child so that a search that never ends fails the test on its timeout instead of hanging the suite.
_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from metagym_amd import _lib
lib = _lib.load()
cfg = _lib.QuadrotorConfig()
assert lib.mg_quadrotor_default_config(cfg) == 0
cfg.fail_range, cfg.fail_velocity, cfg.fail_w = (float(x) for x in sys.argv[2:5])
fake = C.create_string_buffer(64)
st = _lib.QuadrotorState(*[C.addressof(fake)] * 7)
plan = _lib.QuadrotorPlan()
ar = _lib.QuadrotorAutoReset()
print(lib.mg_quadrotor_plan_init(plan, cfg, None, 4, st), lib.mg_quadrotor_plan_init(plan, cfg, ar, 4, st))
"""

SPECIAL = [(r, 100.0, 1000.0) for r in (-1.0, -0.0, 0.0, 1e-30, 3e38, float("inf"), 1e39, float("-inf"), float("nan"))]
SPECIAL += [(1000.0, v, 1000.0) for v in (-1.0, 0.0, float("inf"), float("nan"))]
SPECIAL += [(1000.0, 100.0, w) for w in (-1.0, 0.0, float("inf"), float("nan"))]


def test_plan_init_folds_special_thresholds_without_hanging():
    """mg_quadrotor_plan_init is host-only with fake buffers (tests/test_abi.py): it folds the config and launches
    nothing. Every threshold the reference accepts must fold and return 0, with and without auto-reset."""
    def run(t):
        try:
            p = subprocess.run([sys.executable, "-c", _CHILD, ROOT] + [repr(x) for x in t], capture_output=True,
                               text=True, timeout=60)
        except subprocess.TimeoutExpired:
            return t, "timed out after 60 s (the threshold search in fold_config does not end)"
        return t, p.stdout.strip() if p.returncode == 0 else "exit %d: %s" % (p.returncode, p.stderr[-400:])

    with ThreadPoolExecutor(4) as pool:
        results = list(pool.map(run, SPECIAL))
    bad = [(t, r) for t, r in results if r != "0 0"]
    assert not bad, bad


# ---- threshold boundaries, found with the oracle alone (tests/test_quadrotor_edges_gpu.py runs every step form on them)
#
# Failing is monotone in each threshold, so a bisection over the threshold's bit patterns finds the largest value at
# which the oracle still reports the failure: the range over f32 values (the kernel and the reference compare against
# the config's double cast to f32), velocity and body rate over doubles. Each env's norm peaks at a known sub-step:
# the first (moving inward, decelerating) or the tenth (moving outward, accelerating), which is the stock forms' peeled
# sub-step. The two-threshold cases fail both tests in the same sub-step, so the reference's precedence decides the code.

DEFAULT_THRESHOLDS = dict(fail_range=1000.0, fail_velocity=100.0, fail_w=1000.0)
NORM_OF = {"fail_range": "pos", "fail_velocity": "vel", "fail_w": "omega"}
CODE_OF = {"fail_range": 1, "fail_velocity": 2, "fail_w": 3}

# name: (thresholds at their boundary, expected code, sub-step of the peak, pos, vel, omega, propw, action)
BOUNDARY = {
    "range_inward": (("fail_range",), 1, 1, [300, 400, 2], [-12, -16, 0], [0, 0, 0], [400] * 4, [3.0] * 4),
    "range_outward": (("fail_range",), 1, 10, [300, 400, 2], [12, 16, 0], [0, 0, 0], [400] * 4, [3.0] * 4),
    "velocity_decelerating": (("fail_velocity",), 2, 1, [1, 2, 0.5], [60, 0, 0], [0, 0, 0], [400] * 4, [3.0] * 4),
    "velocity_accelerating": (("fail_velocity",), 2, 10, [1, 2, 0.5], [2, 0, -3], [0, 0, 0], [0] * 4, [0.1] * 4),
    "body_rate_decelerating": (("fail_w",), 3, 1, [1, 2, 0.5], [0.5, 0, 0], [40, 0, 0], [400] * 4, [3.0] * 4),
    "body_rate_accelerating": (("fail_w",), 3, 10, [1, 2, 0.5], [0.5, 0, 0], [0, 0, -2], [0] * 4, [15, 0.1, 15, 0.1]),
    "range_and_velocity_sub1": (("fail_range", "fail_velocity"), 1, 1, [300, 400, 2], [-36, -48, 0], [0, 0, 0],
                                [400] * 4, [3.0] * 4),
    "range_and_velocity_sub10": (("fail_range", "fail_velocity"), 1, 10, [0, 0, -500], [0, 0, -3], [0, 0, 0],
                                 [0] * 4, [0.1] * 4),
    "velocity_and_body_rate_sub1": (("fail_velocity", "fail_w"), 2, 1, [1, 2, 0.5], [60, 0, 0], [40, 0, 0],
                                    [400] * 4, [3.0] * 4),
    "velocity_and_body_rate_sub10": (("fail_velocity", "fail_w"), 2, 10, [1, 2, 0.5], [2, 0, -3], [0, 0, -2],
                                     [0] * 4, [15, 0.1, 15, 0.1]),
}


def boundary_env(name):
    """(state arrays of one env, f32 action [1, 4]) of a BOUNDARY case"""
    _t, _c, _p, pos, vel, om, propw, act = BOUNDARY[name]
    x = dict(pos=np.array([pos], np.float32), vel=np.array([vel], np.float64), omega=np.array([om], np.float64),
             propw=np.array([propw], np.float32), R=np.eye(3, dtype=np.float32).reshape(1, 9))
    return x, np.array([act], np.float32)


def case_consts(cfg=None, **thresholds):
    """Oracle constants of a simulator config (None: config.json) with DEFAULT_THRESHOLDS overridden by `thresholds`."""
    c = qo.default_consts() if cfg is None else qo.consts_from_config(cfg)
    for k, v in dict(DEFAULT_THRESHOLDS, **thresholds).items():
        setattr(c, k, v)
    return c


def _oracle_code(name, cfg=None, **thresholds):
    x, a = boundary_env(name)
    c = case_consts(cfg, **thresholds)
    st = qo.make_states(x["pos"], x["vel"], x["omega"], x["propw"], x["R"])
    return int(qo.batch_env_step(c, st, np.zeros(1, np.int32), a)[3][0]), st


def _next_up(name, v):
    if name == "fail_range":
        return float(np.nextafter(np.float32(v), np.float32(np.inf)))
    return float(np.nextafter(v, np.inf))


def _bisect(name, threshold, cfg):
    """Largest threshold value (f32 for the range, f64 otherwise) at which the oracle reports CODE_OF[threshold]."""
    want = CODE_OF[threshold]
    if threshold == "fail_range":
        t, u = np.float32, np.uint32
    else:
        t, u = np.float64, np.uint64
    lo, hi = 0, int(np.array(np.inf, t).view(u))               # fails at +0, not at +inf
    assert _oracle_code(name, cfg, **{threshold: 0.0})[0] == want
    while hi - lo > 1:
        mid = (lo + hi) // 2
        v = float(np.array(mid, u).view(t))
        if _oracle_code(name, cfg, **{threshold: v})[0] == want:
            lo = mid
        else:
            hi = mid
    return float(np.array(lo, u).view(t))


def substep_trace(name, cfg=None, **thresholds):
    """Step the oracle one sub-step per call (dt = precision). Returns the pos / vel / omega norms after each of
    the ten sub-steps and the sub-step at which it first reports a failure (0: none)."""
    x, a = boundary_env(name)
    c = case_consts(cfg, **thresholds)
    c.dt = c.precision
    st = qo.make_states(x["pos"], x["vel"], x["omega"], x["propw"], x["R"])
    ct = np.zeros(1, np.int32)
    norms, first = {k: [] for k in ("pos", "vel", "omega")}, 0
    for i in range(10):
        f = qo.batch_env_step(c, st, ct, a)[3][0]
        s = qo.states_to_arrays(st)
        for k in norms:
            norms[k].append(float(np.linalg.norm(s[k][0].astype(np.float64))))
        if f:
            first = i + 1
            break
    return norms, first, st


_BOUNDS = {}


def boundary_thresholds(name, cfg=None):
    """{threshold: largest failing value} of a BOUNDARY case under a simulator config (memoised)."""
    key = (name, json.dumps(cfg, sort_keys=True))
    if key not in _BOUNDS:
        _BOUNDS[key] = {t: _bisect(name, t, cfg) for t in BOUNDARY[name][0]}
    return _BOUNDS[key]


def boundary_sides(name, cfg=None):
    """The two configs of a case: every threshold at its boundary (fails), and every one a value above (does not)."""
    b = boundary_thresholds(name, cfg)
    return [dict(DEFAULT_THRESHOLDS, **b), dict(DEFAULT_THRESHOLDS, **{k: _next_up(k, v) for k, v in b.items()})]


def test_substep_stepping_equals_the_ten_substep_step():
    """The peak search steps the oracle with dt = precision; ten such calls give the state of one env.step."""
    inf = dict(fail_range=np.inf, fail_velocity=np.inf, fail_w=np.inf)
    for name in BOUNDARY:
        _norms, first, one = substep_trace(name, **inf)
        _code, ten = _oracle_code(name, **inf)
        assert first == 0
        a, b = qo.states_to_arrays(one), qo.states_to_arrays(ten)
        for k in ("pos", "vel", "omega", "propw", "R"):
            assert np.array_equal(a[k], b[k]), (name, k)


@pytest.mark.parametrize("name", sorted(BOUNDARY))
def test_boundary_thresholds_split_fail_from_pass(name):
    """At the bisected value the oracle fails with the expected code at the sub-step where the norm peaks; one value
    above, it does not fail. For two thresholds, both tests fail alone at that same sub-step."""
    thresholds, code, peak, *_ = BOUNDARY[name]
    b = boundary_thresholds(name)
    inf = dict(fail_range=np.inf, fail_velocity=np.inf, fail_w=np.inf)
    norms, _f, _s = substep_trace(name, **inf)
    for t in thresholds:
        n = norms[NORM_OF[t]]
        assert int(np.argmax(n)) + 1 == peak and n.count(max(n)) == 1, (t, n)
        # alone (every other test off), this threshold fails at the peak and nowhere else
        assert substep_trace(name, **dict(inf, **{t: b[t]}))[1] == peak, t
        print("%s: %s = %r (next %r), norm peaks at sub-step %d" % (name, t, b[t], _next_up(t, b[t]), peak))
    fail, ok = boundary_sides(name)
    assert _oracle_code(name, **fail)[0] == code
    assert substep_trace(name, **fail)[1] == peak
    assert _oracle_code(name, **ok)[0] == 0
