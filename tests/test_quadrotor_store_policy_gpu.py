"""Store policy of the quadrotor step kernels (csrc/quadrotor.hip: MG_QUAD_ST_*, MG_QUAD_STP_*, MG_QUAD_LD_STATE).

A store policy (plain, nt, write-through) cannot alter a value. It can alter which bytes a store touches and when they
become visible to the next reader, so that is what these tests look at, for whichever policy the library was built with:

  * masked tails: every state and output array sits between two 256-byte guards filled with a pattern; three steps with
    auto-reset, one lane per wave at the last step of its episode (the rare `episode` store and reset_apply), at n with a
    partial last wave (200, 65, 1) and with full waves (256, 64); guards intact, every array bit-equal to the CPU oracle
    (NaN only required to be NaN). For the one-wave form, STEP_STOCK (a plan that cannot fold: fail_velocity below sqrt 2)
    and the generic form (MG_QUAD_GENERIC=1);
  * byte-wide neighbours: at n = 200 the done / failed bytes of envs 192-199 share a 64-byte segment with bytes past n.
    The whole allocation is preset to 0xA5; only the first n bytes may change;
  * visibility without a host synchronisation: step on stream A, event, stream B waits and copies obs, reward, done and
    the state with a torch kernel; the copy equals one taken after torch.cuda.synchronize(). The same with the step
    captured in a hipGraph and replayed twice: the second replay reads the state the first one wrote;
  * step after step: 12 step()s at n = 320 against one rollout() of 12 steps, which keeps the state in registers and never
    reads back its own stores; records and final state_dict() equal.
Shapes are the smallest that hold a full wave, a partial wave and more than one block. Runs on the GPU box only (-m gpu)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from oracle import quadrotor as qo
from test_quadrotor_edges_gpu import _plan_form, _sim_config
from test_quadrotor_fastpath_gpu import _same, _same_obs
from test_quadrotor_straightline_gpu import SEED, _generic

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD, PATTERN = 256, 0xA5
NT = 1000
STATE = ("pos", "vel", "omega", "propw", "rot", "ct", "episode")
OUTPUTS = ("_obs", "_reward", "_reward64", "_done", "_failed")
# form -> (MG_QUAD_GENERIC, threshold overrides, mg_quadrotor_fold.one_wave_form); fail_velocity = 1.41 cannot fold
FORMS = {"one_wave": (False, {}, 2), "stock": (False, dict(fail_velocity=1.41), 1), "generic": (True, {}, 0)}


def _framed(t):
    """A copy of `t` between two guards: (whole allocation as bytes, the body as a tensor like t)."""
    nbytes = t.numel() * t.element_size()
    buf = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=t.device)
    body = buf[GUARD:GUARD + nbytes].view(t.dtype).view(t.shape)
    body.copy_(t)
    return buf, body


def _make(n, form, tmp_path, framed=True):
    """The env in the given form; with `framed`, every array the kernels write moved between guards (the plan is folded
    again for the new addresses). Returns (env, {array name: whole allocation}, config dict)."""
    import metagym_amd
    from metagym_amd import _lib
    generic, over, one_wave_form = FORMS[form]
    cfg = _sim_config("stock", **over)
    conf = tmp_path / ("sim_%s.json" % form)
    conf.write_text(json.dumps(cfg))
    frames = {}
    with _generic(generic):
        env = metagym_amd.make("quadrotor-v0", num_envs=n, device="cuda:0", task="hovering_control", nt=NT,
                               auto_reset=True, seed=SEED, env_id_base=3, simulator_conf=str(conf))
        if framed:
            for k in STATE + OUTPUTS:
                frames[k], body = _framed(getattr(env, k))
                setattr(env, k, body)
            env._state = _lib.QuadrotorState(*[_lib.ptr(getattr(env, k)) for k in STATE])
            env._out_ptrs = [_lib.ptr(getattr(env, k)) for k in OUTPUTS]
            env._info_obj = type(env._info_obj)(env._obs, env._failed)
            env._plan = _lib.QuadrotorPlan()
            _lib.check(env._lib.mg_quadrotor_plan_init(env._plan, env._cfg, env._ar, n, env._state), "mg_quadrotor_plan_init")
            env._plan_ref = C.byref(env._plan)
    fold = _lib.QuadrotorFold()
    assert env._lib.mg_quadrotor_plan_fold(env._plan, fold) == 0
    assert fold.one_wave_form == one_wave_form
    simple, stock, xframe, shadow = _plan_form(env, 1)
    assert (stock, shadow and one_wave_form == 2) == ((1, True) if form == "one_wave" else (1, False) if form == "stock" else (0, False))
    return env, frames, cfg


def _batch(n, steps):
    """Slow envs (|v| stays below the `stock` form's 1.41 m/s for most lanes), lane 5 of every wave one step before the end
    of its episode."""
    rs = np.random.RandomState(1000 + n)
    x = dict(pos=(rs.uniform(-30, 30, (n, 3)) * [1, 1, 0.15]).astype(F32), vel=rs.uniform(-0.2, 0.2, (n, 3)),
             omega=rs.uniform(-5, 5, (n, 3)), propw=rs.uniform(0, 600, (n, 4)).astype(F32),
             R=np.tile(np.eye(3, dtype=F32).reshape(9), (n, 1)) + rs.uniform(-0.05, 0.05, (n, 9)).astype(F32),
             ct=rs.randint(0, 900, n).astype(np.int32), episode=rs.randint(0, 1 << 20, n).astype(np.uint32))
    enders = [e for e in range(n) if e % 64 == min(5, n - 1)]
    x["ct"][enders] = NT - 1
    acts = [rs.uniform(0.1, 15.0, (n, 4)).astype(F32) for _ in range(steps)]
    return x, acts, enders


def _load(env, x):
    """In place: the arrays keep their (framed) addresses."""
    for k, v in (("pos", x["pos"].T), ("vel", x["vel"].T), ("omega", x["omega"].T), ("propw", x["propw"].T),
                 ("rot", x["R"].T), ("ct", x["ct"]), ("episode", x["episode"].view(np.int32))):
        getattr(env, k).copy_(torch.as_tensor(np.ascontiguousarray(v)))


def _guards_intact(frames):
    for k, buf in frames.items():
        b = buf.cpu().numpy()
        assert (b[:GUARD] == PATTERN).all(), "guard in front of %s" % k
        assert (b[-GUARD:] == PATTERN).all(), "guard behind %s" % k


def _against_oracle(env, cfg, x, acts, enders, frames):
    n = len(x["ct"])
    consts, ar = qo.consts_from_config(cfg, nt=NT), qo.default_autoreset(seed=SEED, env_id_base=3)
    st = qo.make_states(x["pos"], x["vel"], x["omega"], x["propw"], x["R"])
    ct, ep = x["ct"].copy(), x["episode"].copy()
    for t, a in enumerate(acts):
        obs, rew, done, info = env.step(torch.as_tensor(a))
        o_obs, o_rew, o_done, o_failed = qo.batch_env_step_autoreset(consts, ar, st, ct, ep, a)
        _same(info["failed"].cpu().numpy(), o_failed.astype(np.uint8), "failed, step %d" % t)
        _same(done.cpu().numpy(), o_done.astype(bool), "done, step %d" % t)
        _same(env.reward64.cpu().numpy(), o_rew, "reward64, step %d" % t)
        _same(rew.cpu().numpy(), o_rew.astype(F32), "reward, step %d" % t)
        _same_obs(obs.cpu().numpy(), o_obs)
        o = qo.states_to_arrays(st)
        for k, kk in (("pos", "pos"), ("vel", "vel"), ("omega", "omega"), ("propw", "propw"), ("rot", "R")):
            _same(getattr(env, k).T.cpu().numpy(), o[kk], "state %s, step %d" % (k, t))
        _same(env.ct.cpu().numpy(), ct, "ct, step %d" % t)
        _same(env.episode.cpu().numpy().view(np.uint32), ep, "episode, step %d" % t)
        if t == 0:
            assert o_done[enders].all() and (ep[enders] == x["episode"][enders] + 1).all()   # the forced episode ends
        _guards_intact(frames)


@pytest.mark.parametrize("n", [200, 65, 1, 256, 64])
@pytest.mark.parametrize("form", list(FORMS))
def test_masked_tails(tmp_path, form, n):
    env, frames, cfg = _make(n, form, tmp_path)
    x, acts, enders = _batch(n, 3)
    _load(env, x)
    _against_oracle(env, cfg, x, acts, enders, frames)


@pytest.mark.parametrize("form", list(FORMS))
def test_byte_wide_neighbours(tmp_path, form):
    n = 200
    env, frames, cfg = _make(n, form, tmp_path)
    x, acts, enders = _batch(n, 1)
    _load(env, x)
    for k in ("_done", "_failed"):
        frames[k].fill_(PATTERN)                     # the n bytes of the array as well
    _against_oracle(env, cfg, x, acts, enders, frames)
    for k in ("_done", "_failed"):
        b = frames[k].cpu().numpy()
        assert (b[GUARD:GUARD + n] <= 3).all(), k      # every one of the n bytes was written (0 / 1, or a failure code)
        assert (b[GUARD + n:] == PATTERN).all() and (b[:GUARD] == PATTERN).all(), k


def _snapshot(env):
    return [t.clone() for t in (env._obs, env._reward, env._reward64, env._done, env._failed)] + \
           [getattr(env, k).clone() for k in STATE]


def _equal(a, b, what):
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p.view(torch.uint8), q.view(torch.uint8)), "%s, array %d" % (what, i)


@pytest.mark.parametrize("n", [256, 200])
def test_next_reader_sees_the_step_without_a_host_sync(tmp_path, n):
    env, _, _ = _make(n, "one_wave", tmp_path, framed=False)
    ref, _, _ = _make(n, "one_wave", tmp_path, framed=False)
    x, acts, _ = _batch(n, 4)
    for e in (env, ref):
        _load(e, x)
    acts_d = [torch.as_tensor(a).cuda() for a in acts]
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    # eager: the reader on stream B is ordered behind the step by an event only
    for a in acts_d[:2]:
        with torch.cuda.stream(sa):
            env.step(a)
            ev = torch.cuda.Event()
            ev.record(sa)
        with torch.cuda.stream(sb):
            sb.wait_event(ev)
            early = _snapshot(env)
        torch.cuda.synchronize()
        _equal(early, _snapshot(env), "copy behind the event against the copy behind a synchronize")
        ref.step(a)
        torch.cuda.synchronize()
        _equal(early, _snapshot(ref), "against an env stepped with a synchronize after every step")
    # the step in a hipGraph, replayed twice: replay 2 loads the state replay 1 stored
    static_a = acts_d[2].clone()
    sd0 = env.state_dict()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.step(static_a)                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(static_a)
    env.load_state_dict(sd0)                         # the warm-up and the capture pass advanced the state
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        g.replay()
        g.replay()
        ev = torch.cuda.Event()
        ev.record(sa)
    with torch.cuda.stream(sb):
        sb.wait_event(ev)
        early = _snapshot(env)
    torch.cuda.synchronize()
    _equal(early, _snapshot(env), "replays: copy behind the event against the copy behind a synchronize")
    for _ in range(2):
        ref.step(static_a)
        torch.cuda.synchronize()
    _equal(early, _snapshot(ref), "replays against eager steps")


def test_steps_equal_one_rollout(tmp_path):
    n, T = 320, 12
    stepped, rolled = _make(n, "one_wave", tmp_path, framed=False)[0], _make(n, "one_wave", tmp_path, framed=False)[0]
    x, acts, _ = _batch(n, T)
    for e in (stepped, rolled):
        _load(e, x)
    a = torch.as_tensor(np.stack(acts)).cuda()
    rec = []
    for t in range(T):                               # no host synchronisation between the steps
        obs, rew, done, info = stepped.step(a[t])
        rec.append((obs.clone(), rew.clone(), stepped.reward64.clone(), done.clone(), info["failed"].clone()))
    obs, rew, done, failed = rolled.rollout(a)
    rew64 = rolled._last_rollout_reward64
    torch.cuda.synchronize()
    assert bool(done.any())                          # the forced episode ends are part of the comparison
    for t in range(T):
        _equal(rec[t], (obs[t], rew[t], rew64[t], done[t], failed[t]), "step %d against the rollout's record" % t)
    ss, sr = stepped.state_dict(), rolled.state_dict()
    for k in STATE:
        assert torch.equal(ss[k].view(torch.uint8), sr[k].view(torch.uint8)), k
