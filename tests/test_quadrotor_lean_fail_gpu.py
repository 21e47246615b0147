"""The one-wave stock step without failure tests in its sub-steps (fold_lean, csrc/quadrotor.hip): lanes placed at the
edges of the folded window, against the generic form (MG_QUAD_GENERIC=1) and the CPU oracle, bit for bit: obs (the atan2
entries within 4 ulp, as everywhere), reward, reward64, done, failed and the full state after each of three steps, with
auto-reset.

A wave redoes its whole step with the full tests as soon as ONE of its lanes clears the fast path's flag, so two special
lanes in one wave would hide each other: a broken fold of one test would go unseen behind a working fold of another.
Each case therefore holds ONE kind of special lane, one such lane per wave, every other lane ordinary (far from every
edge, so only the special lane can send its wave through the fallback). Then a lane that fails must clear the flag by
its own folded condition alone, or the main path stores failed = 0 for it and the comparison fails; and a lane just
inside the window is stepped by the main path.

Special lanes (the edge, the threshold and pos_safe32 come from mg_quadrotor_plan_fold):
  * |v|^2 after sub-step 1, where a fast decelerating env has its peak, one high-word unit below the edge (main path, no
    failure), between the edge and the threshold (fallback, no failure), just over the threshold (code 2). The initial
    speed comes from a bisection with the oracle stepped one sub-step, |v|^2 restated with the kernel's fma chain;
  * the same three for |w|^2 after sub-step 1 (code 3 for the third), twice. Under the stock threshold of 1000 rad/s the
    stock drag makes the next explicit Euler sub-step overshoot, so the first two fail with code 3 at sub-step 2: they pass
    the first update's window and leave a later one. Under a plan with fail_w = 40 rad/s, where the body rate decays after
    its peak at sub-step 1, they are the analogues of the |v| lanes: main path and no failure, fallback and no failure;
  * max-norm of the position one float below pos_safe32 on all ten samples (hovering on equal voltages keeps p_x and
    p_y), at pos_safe32, between pos_safe32 and the range, and beyond the range (code 1);
  * one lane that meets code 3 at sub-step 1 and code 1 later in the same step: the reference's precedence is per
    sub-step, so the first code, 3, is the result.
n = 256 (one block, four waves: the special lane sits in waves 0 and 2, waves 1 and 3 are ordinary) and n = 200 (waves 0
and the partial wave 3). Runs on the GPU box only (-m gpu)."""
import fractions

import numpy as np
import pytest
import torch

from oracle import quadrotor as qo
from test_quadrotor_edges_gpu import _plan_form, _sim_config
from test_quadrotor_fastpath_gpu import _same, _same_obs
from test_quadrotor_lean_fail import _fold as _host_fold
from test_quadrotor_straightline_gpu import SEED, _generic, _load

pytestmark = pytest.mark.gpu
F32 = np.float32
STEPS = 3
STATE_KEYS = ("pos", "vel", "omega", "propw", "R", "ct", "episode")


PLANS = {"stock": {}, "low_w": dict(fail_w=40.0)}    # threshold overrides of the stock simulator config


def _fold(env):
    from metagym_amd import _lib
    out = _lib.QuadrotorFold()
    assert _lib.load().mg_quadrotor_plan_fold(env._plan, out) == 0
    return out


def _hi(x):
    return int(np.float64(x).view(np.uint64)) >> 32


def _double(hi, lo=0):
    return float(np.uint64((hi << 32) | lo).view(np.float64))


def _sumsq3(x):
    """sumsq3(const double *) of csrc/quadrotor.hip: fma(x2, x2, fma(x1, x1, x0 * x0)), each step correctly rounded."""
    Fr = fractions.Fraction
    t = float(x[0]) * float(x[0])
    t = float(Fr(float(x[1])) * Fr(float(x[1])) + Fr(t))
    return float(Fr(float(x[2])) * Fr(float(x[2])) + Fr(t))


def _lane(**kw):
    """One env hovering on equal rotor speeds and voltages (no propeller torque), fields overridden by kw."""
    x = dict(pos=np.array([1.0, 2.0, 0.5], F32), vel=np.zeros(3), omega=np.zeros(3), propw=np.full(4, 400.0, F32),
             R=np.eye(3, dtype=F32).reshape(9), act=np.full(4, 3.0, F32))
    for k, v in kw.items():
        x[k] = np.asarray(v, x[k].dtype)
    return x


def _after_substep_1(lane):
    """The oracle's state of `lane` after one sub-step, no failure test in the way."""
    c = qo.default_consts()
    c.fail_range = c.fail_velocity = c.fail_w = float("inf")
    c.dt = c.precision
    st = qo.make_states(lane["pos"][None], lane["vel"][None], lane["omega"][None], lane["propw"][None], lane["R"][None])
    qo.batch_env_step(c, st, np.zeros(1, np.int32), lane["act"][None])
    return {k: v[0] for k, v in qo.states_to_arrays(st).items()}


def _speed_for(key, direction, target, lo, hi):
    """Initial speed s in [lo, hi] along `direction` (key: "vel" or "omega") whose squared norm after sub-step 1 is the
    least one >= target; the squared norm after sub-step 1 grows with s on the bracket."""
    direction = np.asarray(direction, np.float64)

    def sq(s):
        return _sumsq3(_after_substep_1(_lane(**{key: s * direction}))[key])

    assert sq(lo) < target <= sq(hi)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        lo, hi = (lo, mid) if sq(mid) >= target else (mid, hi)
    return hi, sq(hi)


def _norm_lanes(out, prefix, key, edge, thr, code, lo, hi, later):
    """The three lanes around one folded norm test: below the edge, between edge and threshold, over the threshold."""
    d = np.array([1.0, 0.0, 0.0])
    below, x = _speed_for(key, d, _double(edge - 1, 0x80000000), lo, hi)
    assert _hi(x) == edge - 1                                  # one high-word unit below the edge
    between, y = _speed_for(key, d, thr * thr * (1.0 - 2.0 ** -20), lo, hi)
    assert _hi(y) >= edge and np.sqrt(y) <= thr                # outside the window, not failing
    over, z = _speed_for(key, d, thr * thr * (1.0 + 2.0 ** -20), lo, hi)
    assert np.sqrt(z) > thr
    out[prefix + "_below_edge"] = (_lane(**{key: below * d}), later, True)
    out[prefix + "_edge_to_threshold"] = (_lane(**{key: between * d}), later, False)
    out[prefix + "_over_threshold"] = (_lane(**{key: over * d}), code, False)


_SPECIALS = {}


def _special_lanes(plan):
    """name -> (lane, expected failure code of step 1, sub-step 1's update lies inside the window) for PLANS[plan]"""
    if plan in _SPECIALS:
        return _SPECIALS[plan]
    f = _host_fold(**PLANS[plan])
    assert f.one_wave_form == 2
    out = {}
    if plan == "low_w":       # a body rate that decays after sub-step 1: w1 = w0 * (1 - 5.48e-3 * w0) grows with w0 below 91
        _norm_lanes(out, "omega", "omega", f.edge_w, f.fail_w, 3, 45.0, 70.0, 0)
    else:
        _norm_lanes(out, "vel", "vel", f.edge_v, f.fail_velocity, 2, 95.0, 110.0, 0)
        _norm_lanes(out, "omega", "omega", f.edge_w, f.fail_w, 3, 480.0, 560.0, 3)   # overshoots at sub-step 2: code 3
        P = F32(f.pos_safe32)
        m = np.nextafter(P, F32(0))
        out["pos_below_safe"] = (_lane(pos=[m, -m, 0.5]), 0, True)
        out["pos_at_safe"] = (_lane(pos=[P, 3.0, 0.5]), 0, False)
        out["pos_safe_to_range"] = (_lane(pos=[-800.0, 3.0, 0.5]), 0, False)
        out["pos_beyond_range"] = (_lane(pos=[1000.5, 3.0, 0.5]), 1, False)
        w3 = out["omega_over_threshold"][0]["omega"]
        out["code3_then_code1"] = (_lane(pos=[999.8, 0.0, 0.5], vel=[50.0, 0.0, 0.0], omega=w3), 3, False)
    _SPECIALS[plan] = out
    return out


CASES = [("stock", n) for n in ("vel_below_edge", "vel_edge_to_threshold", "vel_over_threshold", "omega_below_edge",
                                "omega_edge_to_threshold", "omega_over_threshold", "pos_below_safe", "pos_at_safe",
                                "pos_safe_to_range", "pos_beyond_range", "code3_then_code1")]
CASES += [("low_w", n) for n in ("omega_below_edge", "omega_edge_to_threshold", "omega_over_threshold")]


def _batch(n, specials, placements):
    rs = np.random.RandomState(n)
    x = dict(pos=(rs.uniform(-30, 30, (n, 3)) * [1, 1, 0.15]).astype(F32), vel=rs.uniform(-4, 4, (n, 3)),
             omega=rs.uniform(-5, 5, (n, 3)), propw=rs.uniform(0, 600, (n, 4)).astype(F32),
             R=np.tile(np.eye(3, dtype=F32).reshape(9), (n, 1)) + rs.uniform(-0.05, 0.05, (n, 9)).astype(F32),
             ct=rs.randint(0, 900, n).astype(np.int32), episode=rs.randint(0, 1 << 20, n).astype(np.uint32))
    acts = [rs.uniform(0.1, 15.0, (n, 4)).astype(F32) for _ in range(STEPS)]
    for lane_id, name in placements.items():
        lane = specials[name][0]
        for k in ("pos", "vel", "omega", "propw", "R"):
            x[k][lane_id] = lane[k]
        for a in acts:
            a[lane_id] = lane["act"]
    return x, acts


def _env(n, generic, conf):
    import metagym_amd
    with _generic(generic):
        return metagym_amd.make("quadrotor-v0", num_envs=n, device="cuda:0", task="hovering_control", nt=1000,
                                auto_reset=True, seed=SEED, env_id_base=3, simulator_conf=conf)


def _step(env, a):
    obs, rew, done, info = env.step(torch.as_tensor(a))
    sd = env.state_dict()
    return dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), reward64=env.reward64.cpu().numpy(),
                done=done.cpu().numpy(), failed=info["failed"].cpu().numpy(), pos=sd["pos"].T.cpu().numpy(),
                vel=sd["vel"].T.cpu().numpy(), omega=sd["omega"].T.cpu().numpy(), propw=sd["propw"].T.cpu().numpy(),
                R=sd["rot"].T.cpu().numpy(), ct=sd["ct"].cpu().numpy(),
                episode=sd["episode"].cpu().numpy().view(np.uint32))


def _inside(f, s):
    """all_in_range and the max-norm test for the oracle state `s` of one env"""
    return (_hi(_sumsq3(s["vel"])) < f.edge_v and _hi(_sumsq3(s["omega"])) < f.edge_w
            and bool(np.max(np.abs(s["pos"])) < F32(f.pos_safe32)))


@pytest.mark.parametrize("n", [256, 200])
@pytest.mark.parametrize("plan,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_lean_failure_fold(tmp_path, plan, name, n):
    import json
    cfg = _sim_config("stock", **PLANS[plan])
    conf = tmp_path / "sim.json"
    conf.write_text(json.dumps(cfg))
    env, gen = _env(n, False, str(conf)), _env(n, True, str(conf))
    assert _plan_form(env, 1) == (1, 1, 1, 1) and _plan_form(gen, 1) == (1, 0, 0, 0)
    f, host = _fold(env), _host_fold(**PLANS[plan])
    assert f.one_wave_form == 2 and _fold(gen).one_wave_form == 0
    assert (f.edge_v, f.edge_w, f.pos_safe32, f.fail_w) == (host.edge_v, host.edge_w, host.pos_safe32, host.fail_w)
    specials = _special_lanes(plan)
    lane, code, inside = specials[name]
    assert _inside(f, _after_substep_1(lane)) == inside
    placements = {37: name, (165 if n == 256 else 195): name}      # one special lane per wave; waves 1 and 3 / 2 ordinary
    x, acts = _batch(n, specials, placements)
    consts, ar = qo.consts_from_config(cfg), qo.default_autoreset(seed=SEED, env_id_base=3)
    for i in range(n):                                              # ordinary lanes start far inside every window
        if i not in placements:
            assert _inside(f, {k: x[k][i] for k in ("pos", "vel", "omega")})
    _load(env, x)
    _load(gen, x)
    st = qo.make_states(x["pos"], x["vel"], x["omega"], x["propw"], x["R"])
    ct, ep = x["ct"].copy(), x["episode"].copy()
    for t, a in enumerate(acts):
        g, h = _step(env, a), _step(gen, a)
        for k in ("reward", "reward64", "done", "failed") + STATE_KEYS:
            _same(g[k], h[k], "%s against the generic form, step %d" % (k, t))
        _same_obs(g["obs"], h["obs"])
        obs, rew, done, failed = qo.batch_env_step_autoreset(consts, ar, st, ct, ep, a)
        _same(g["failed"], failed.astype(np.uint8), "failed, step %d" % t)
        _same(g["done"], done.astype(bool), "done, step %d" % t)
        _same(g["reward64"], rew, "reward64, step %d" % t)
        _same(g["reward"], rew.astype(F32), "reward, step %d" % t)
        _same_obs(g["obs"], obs)
        o = qo.states_to_arrays(st)
        for k in ("pos", "vel", "omega", "propw", "R"):
            _same(g[k], o[k], "state %s, step %d" % (k, t))
        _same(g["ct"], ct, "ct")
        _same(g["episode"], ep, "episode")
        if t == 0:
            for lane_id in placements:
                assert g["failed"][lane_id] == code, (name, lane_id, g["failed"][lane_id])
            ordinary = [i for i in range(n) if i not in placements]
            assert not g["failed"][ordinary].any()
