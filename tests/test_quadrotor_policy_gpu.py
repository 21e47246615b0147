"""Quadrotor closed-loop rollouts on the GPU (Quadrotor.rollout_policy). The central check is a replay identity that
rests only on code already pinned to the reference: the recorded actions are QuadrotorPolicy.reference of the recorded
observations bit for bit (policy half), and the existing rollout(recorded actions) from the same state reproduces every
record and the final state bit for bit (environment half)."""
import numpy as np
import pytest
import torch

import quadrotor_policy_cases as pc
import quadrotor_tasks_cases as qc
from oracle import quadrotor as qo
from test_quadrotor_gpu import _get_state, _load_state

pytestmark = pytest.mark.gpu
N, T = pc.N, pc.T
RECORDS = ("actions", "obs", "reward", "reward64", "done", "failed")


def _env(n=N, **kw):
    import metagym_amd
    kw.setdefault("task", "hovering_control")
    return metagym_amd.make("quadrotor-v0", num_envs=n, device="cuda:0", **kw)


def _table():
    from metagym_amd.quadrotor import QuadrotorTaskTable
    return QuadrotorTaskTable(qc.mixed_configs())


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa) == sorted(sb)
    for k in sa:
        if torch.is_tensor(sa[k]):
            assert torch.equal(sa[k], sb[k]), k
        else:                                              # np_random: (name, keys, pos, has_gauss, cached)
            assert all(np.array_equal(u, v) for u, v in zip(sa[k], sb[k])), k


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _returns(reward64, done):
    """ret_total, ret_episode, episode_len as sequential float64 sums over the records, on the host"""
    steps, n = reward64.shape
    total, ep, length, ended = np.zeros(n), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, bool)
    for t in range(steps):
        total = total + reward64[t]
        ep = np.where(ended, ep, ep + reward64[t])
        length = np.where(ended, length, length + 1).astype(np.int32)
        ended = ended | done[t].astype(bool)
    return total, ep, length


def _check_returns(res):
    total, ep, length = _returns(res.reward64.cpu().numpy(), res.done.cpu().numpy())
    assert np.array_equal(res.ret_total.cpu().numpy().view(np.uint64), total.view(np.uint64))
    assert np.array_equal(res.ret_episode.cpu().numpy().view(np.uint64), ep.view(np.uint64))
    assert res.episode_len.dtype == torch.int32 and np.array_equal(res.episode_len.cpu().numpy(), length)


def _replay_identity(make, prepare, policy, ids, steps=T):
    """make(): a fresh env; prepare(env): brings it to the start state and returns the observation it then holds."""
    a = make()
    x0 = prepare(a).clone()
    sd = a.state_dict()
    res = a.rollout_policy(policy, steps, ids, record=True)
    n, D = a.num_envs, a.obs_dim
    assert res.actions.shape == (steps, n, 4) and res.obs.shape == (steps, n, D)
    # policy half
    obs_h, act_h = res.obs.cpu().numpy(), res.actions.cpu().numpy()
    x = x0.cpu().numpy()
    for t in range(steps):
        assert np.array_equal(_bits(policy.reference(x, ids)), _bits(act_h[t])), t
        x = obs_h[t]
    # environment half: the existing open-loop rollout on the recorded actions
    b = make()
    prepare(b)
    b.load_state_dict(sd)
    obs, rew, done, failed = b.rollout(res.actions)
    assert torch.equal(obs, res.obs) and torch.equal(rew, res.reward) and torch.equal(done, res.done)
    assert torch.equal(failed, res.failed) and torch.equal(b._last_rollout_reward64, res.reward64)
    _same_state(a, b)
    # the persistent output buffers hold the last step
    assert torch.equal(a._obs, res.obs[-1]) and torch.equal(a._reward, res.reward[-1]) and torch.equal(a._done, res.done[-1])
    assert torch.equal(a._failed, res.failed[-1]) and torch.equal(a.reward64, res.reward64[-1])
    _check_returns(res)
    return a, res


def _reset(seed=3):
    return lambda env: env.reset(seed=seed)


@pytest.mark.parametrize("hidden", [0, 1, 5, 32])
def test_replay_identity_hovering(hidden):
    _replay_identity(lambda: _env(), _reset(), pc.make_policy(hidden), pc.layout_ids())


def test_replay_identity_velocity_control():
    env, res = _replay_identity(lambda: _env(task="velocity_control", nt=40, seed=6), _reset(), pc.make_policy(5, 19),
                                pc.layout_ids())
    assert res.obs.shape[2] == 19 and torch.equal(res.obs[0, :, 16:], env.velocity_targets[1].expand(N, 3))


def test_replay_identity_no_collision_with_a_map(tmp_path):
    p = tmp_path / "map.txt"
    p.write_text(qc.map_text(qc.small_map()))
    _replay_identity(lambda: _env(task="no_collision", map_file=str(p)), _reset(), pc.make_policy(5), pc.layout_ids())


def test_replay_identity_with_fused_auto_reset():
    env, res = _replay_identity(lambda: _env(nt=4, auto_reset=True, seed=11), _reset(), pc.make_policy(5), pc.layout_ids())
    assert int(env.episode.min()) >= 2                     # every env restarted inside the launch at least twice
    never_failed = (res.failed[:4] == 0).all(0)
    assert bool(never_failed.any()) and bool((res.episode_len[never_failed] == 4).all())
    assert bool((res.episode_len <= 4).all())


@pytest.fixture(scope="module")
def mixed_run():
    """auto_reset=False with the mixed task table, from random states: the tight row freezes some envs next to live ones."""
    ids_t, ids_p, pol = qc.mixed_ids(), pc.layout_ids(), pc.make_policy(5)
    state = qc.random_batch(N, qc.STATE_SEED)
    table = _table()

    def make():
        env = _env()
        env.set_task(table, ids_t)
        return env

    def prepare(env):
        _load_state(env, *state)
        return env.step(torch.as_tensor(pc.PRIME_ACTION))[0]

    env, res = _replay_identity(make, prepare, pol, ids_p)
    return dict(make=make, prepare=prepare, env=env, res=res, ids_t=ids_t, ids_p=ids_p, pol=pol, state=state)


def test_mixed_table_freezes_failed_lanes_next_to_live_ones(mixed_run):
    res, ids_t = mixed_run["res"], mixed_run["ids_t"]
    failed_any = (res.failed != 0).any(0).cpu().numpy()
    tight = failed_any[ids_t == 4]
    assert tight.any() and (~tight).any()
    assert not failed_any[ids_t != 4].any()


def test_mixed_table_equals_the_step_loop(mixed_run):
    """frozen envs keep being stepped exactly as the step() loop steps them"""
    res = mixed_run["res"]
    c = mixed_run["make"]()
    mixed_run["prepare"](c)
    for t in range(T):
        obs, rew, done, info = c.step(res.actions[t])
        assert torch.equal(obs, res.obs[t]) and torch.equal(rew, res.reward[t]) and torch.equal(done, res.done[t]), t
        assert torch.equal(info["failed"], res.failed[t]) and torch.equal(c.reward64, res.reward64[t]), t
    _same_state(c, mixed_run["env"])


def test_mixed_table_recorded_actions_on_the_oracle(mixed_run):
    res, ids_t = mixed_run["res"], mixed_run["ids_t"]
    og = qc.OracleGroups(qc.mixed_configs(), ids_t, mixed_run["state"], task=qo.TASK_HOVERING)
    og.step(pc.PRIME_ACTION)
    acts = res.actions.cpu().numpy()
    g_obs, g_rew, g_done, g_failed = (getattr(res, k).cpu().numpy() for k in ("obs", "reward64", "done", "failed"))
    nonang = [i for i in range(16) if i not in (12, 13, 14)]
    for t in range(T):
        o, r, d, f = og.step(acts[t])
        assert np.array_equal(g_failed[t], f.astype(np.uint8)) and np.array_equal(g_done[t], d.astype(bool)), t
        assert np.array_equal(g_rew[t], r), t
        assert np.array_equal(g_obs[t][:, nonang], o[:, nonang]), t
        assert np.max(np.abs(g_obs[t][:, 12:15] - o[:, 12:15])) <= 4 * np.spacing(np.float32(np.pi)), t
    gs, os_ = _get_state(mixed_run["env"]), og.state()
    for k in ("pos", "vel", "omega", "propw", "R", "ct"):
        assert np.array_equal(gs[k], os_[k]), k


def test_staged_and_per_lane_policy_reads_give_the_same_bits():
    """The same (env, policy) pairs laid out so that every wave holds one id (LDS route) and so that every wave holds
    several (each lane reads global memory): each env gets the same bits."""
    pol = pc.make_policy(32)
    n = 192
    ids_u = np.repeat(np.arange(3), 64)                    # wave w flies policy w
    perm = (np.arange(n) % 3) * 64 + np.arange(n) // 3     # position i holds the pair perm[i]: ids 0, 1, 2, 0, 1, 2, ...
    assert sorted(perm.tolist()) == list(range(n))
    ids_m = ids_u[perm]
    assert all(len(set(ids_u[w * 64:(w + 1) * 64])) == 1 and len(set(ids_m[w * 64:(w + 1) * 64])) == 3 for w in range(3))
    rs = np.random.RandomState(21)
    v, w = rs.uniform(-2, 2, (n, 3)), rs.uniform(-5, 5, (n, 3))
    out = []
    for ids, order in ((ids_u, np.arange(n)), (ids_m, perm)):
        env = _env(n)
        env.reset(init_velocity=v[order], init_angular_velocity=w[order])
        out.append((env.rollout_policy(pol, T, ids, record=True), env.state_dict()))
    (ru, su), (rm, sm) = out
    p = torch.as_tensor(perm).cuda()
    for k in RECORDS:
        assert torch.equal(getattr(ru, k)[:, p], getattr(rm, k)), k
    for k in ("ret_total", "ret_episode", "episode_len"):
        assert torch.equal(getattr(ru, k)[p], getattr(rm, k)), k
    for k in ("pos", "vel", "omega", "propw", "rot"):
        assert torch.equal(su[k][:, p], sm[k]), k
    assert torch.equal(su["ct"][p], sm["ct"])


def test_record_off_and_splitting():
    pol, ids = pc.make_policy(5), pc.layout_ids()
    mk = lambda: _env(nt=4, auto_reset=True, seed=13)
    full, quiet, split = mk(), mk(), mk()
    for env in (full, quiet, split):
        env.reset(seed=2)
    rf = full.rollout_policy(pol, T, ids, record=True)
    rq = quiet.rollout_policy(pol, T, ids)
    assert all(getattr(rq, k) is None for k in RECORDS)
    for k in ("ret_total", "ret_episode", "episode_len"):
        assert torch.equal(getattr(rf, k), getattr(rq, k)), k
    _same_state(full, quiet)
    assert torch.equal(full._obs, quiet._obs) and torch.equal(full.reward64, quiet.reward64)
    # 12 = 5 + 7
    r5 = split.rollout_policy(pol, 5, ids, record=True)
    r7 = split.rollout_policy(pol, 7, ids, record=True)
    _same_state(full, split)
    assert torch.equal(torch.cat([r5.obs, r7.obs]), rf.obs) and torch.equal(torch.cat([r5.actions, r7.actions]), rf.actions)
    assert torch.equal(torch.cat([r5.reward64, r7.reward64]), rf.reward64)
    _check_returns(r5)
    _check_returns(r7)


def test_negative_zero_pre_activation_on_the_device():
    """test_quadrotor_policy.py::test_relu_of_negative_zero_and_nan_is_plus_zero, the signed-zero half, in the kernel:
    with b1 = -0.0 and zero weights signed against x every product is -0.0, so z = -0.0; h must be +0.0, and
    b2 + 1 * h with b2 = -0.0 is then +0.0 (an h of -0.0 would leave -0.0)."""
    from metagym_amd.quadrotor import QuadrotorPolicy
    f = np.float32
    env = _env(70)
    x0 = env.reset(init_velocity=np.zeros((70, 3)), init_angular_velocity=np.zeros((70, 3))).cpu().numpy()
    assert np.array_equal(_bits(x0), np.tile(_bits(x0[:1]), (70, 1)))        # one state, one sign pattern
    neg = np.signbit(x0[0])
    w1 = np.where(neg, f(0.0), f(-0.0)).astype(f).reshape(1, 1, 16)
    with np.errstate(all="ignore"):
        assert np.signbit(w1[0, 0] * x0[0]).all() and not (w1[0, 0] * x0[0]).any()
    pol = QuadrotorPolicy(w1, np.array([[-0.0]], f), np.ones((1, 4, 1), f), np.full((1, 4), -0.0, f))
    res = env.rollout_policy(pol, 1, record=True)
    assert np.array_equal(_bits(res.actions.cpu().numpy()), np.zeros((1, 70, 4), np.uint32))
    assert np.array_equal(_bits(pol.reference(x0, np.zeros(70, int))), np.zeros((70, 4), np.uint32))


def test_graph_capture_of_a_policy_rollout():
    pol, ids = pc.make_policy(5), pc.layout_ids()
    mk = lambda: _env(nt=4, auto_reset=True, seed=8)
    eager, graphed = mk(), mk()
    for env in (eager, graphed):
        env.reset(seed=5)
    sd0 = graphed.state_dict()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm-up outside capture: module load, parameter and id upload
        graphed.rollout_policy(pol, 6, ids)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                              # one stream, one launch: no parallel branches
        res = graphed.rollout_policy(pol, 6, ids)
    graphed.load_state_dict(sd0)                           # the warm-up and the capture pass advanced the state
    for i in range(2):
        g.replay()
        want = eager.rollout_policy(pol, 6, ids)
        for k in ("ret_total", "ret_episode", "episode_len"):
            assert torch.equal(getattr(res, k), getattr(want, k)), (k, i)
        assert torch.equal(graphed._obs, eager._obs) and torch.equal(graphed.reward64, eager.reward64), i
    _same_state(eager, graphed)


def test_refused_calls_leave_the_env_untouched():
    from metagym_amd.quadrotor import QuadrotorPolicy
    env = _env(70)
    env.reset(seed=9)
    env.step(torch.full((70, 4), 6.0))
    sd = env.state_dict()
    outs = [t.clone() for t in (env._obs, env._reward, env._reward64, env._done, env._failed)]
    pol = pc.make_policy(5)
    for bad in (np.full(70, 3), np.full(70, -1), np.zeros(69, int), np.zeros((70, 1), int), np.zeros(70)):
        with pytest.raises(ValueError):
            env.rollout_policy(pol, 4, bad)
    with pytest.raises(ValueError):
        env.rollout_policy(pc.make_policy(5, 19), 4)       # a policy for velocity_control's 19 entries
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 0)
    with pytest.raises(TypeError):
        env.rollout_policy(object(), 4)
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(ValueError):
        QuadrotorPolicy(z(1, 257, 16), z(1, 257), z(1, 4, 257), z(1, 4))     # H too large never becomes a policy
    torch.cuda.synchronize()
    after = env.state_dict()
    for k in sd:
        if torch.is_tensor(sd[k]):
            assert torch.equal(sd[k], after[k]), k
    for u, v in zip(outs, (env._obs, env._reward, env._reward64, env._done, env._failed)):
        assert torch.equal(u, v)
    # and the env still runs: default ids are e % P
    res = env.rollout_policy(pol, 3, record=True)
    x = outs[0].cpu().numpy()
    assert np.array_equal(_bits(pol.reference(x, np.arange(70) % pc.P)), _bits(res.actions[0].cpu().numpy()))
