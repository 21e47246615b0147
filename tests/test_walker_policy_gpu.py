"""WalkerBatchEnv.rollout_policy / mg_walker_policy_rollout against what it is defined as: the policy's float32 definition
(`WalkerPolicy.reference`, numpy) applied to the observation each step produced, and `rollout(actions)` on the actions that
gives. Every comparison is torch.equal / np.array_equal: the policy form shares its device code with the rollout, the library
is built without contraction and the reference keeps the kernel's association, so there is no tolerance to choose.
Agreement with the step loop and the physics oracle is inherited through tests/test_walker_rollout_gpu.py. Argument errors
that need no device: tests/test_walker_policy.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_MAX, MAX_STEPS = 12, 5            # every env ends an episode inside the rollout, at steps 4 and 9
IDS = [0, 2, 1, 1, 0]               # P = 3 policies over N = 5 envs


def _cls(robot):
    import metagym_amd.metalocomotion as ml
    return {"humanoid": ml.MetaHumanoidEnv, "ant": ml.MetaAntEnv}[robot]


_MODELS = {}


def _make(robot, n, preset=None, auto_reset=True, **kw):
    env = _cls(robot)(num_envs=n, device=DEV, max_steps=MAX_STEPS, auto_reset=auto_reset, seed=11, env_id_base=7,
                      preset=preset, **kw)
    key = (robot, env.preset)
    if key not in _MODELS:              # two body variants, parsed once per robot and preset
        _MODELS[key] = [env._to_model(t) for t in env.tra_tasks[:2]]
    env.set_task(_MODELS[key])
    env.reset(seed=3)
    return env


def _policy(env, H, P=3, seed=17):
    """Weights uniform in +-0.05, biases in +-0.1, from a fixed generator."""
    from metagym_amd.metalocomotion import WalkerPolicy
    g = np.random.RandomState(seed)
    u = lambda s, *shape: g.uniform(-s, s, size=shape).astype(np.float32)
    D, A = env.obs_dim, env.n_joints
    if H == 0:
        return WalkerPolicy.linear(u(0.05, P, A, D), u(0.1, P, A))
    return WalkerPolicy(u(0.05, P, H, D), u(0.1, P, H), u(0.05, P, A, H), u(0.1, P, A))


def _assert_same_state(a, b):
    for k in a._STATE_KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    if a.foot_force is not None:
        assert torch.equal(a.foot_force, b.foot_force), "foot_force"
    assert a.global_step == b.global_step


def _assert_recorded_run_means_something(res, ids):
    """Conditions on a recorded run, so that a pass of the comparisons means something."""
    for name in ("actions", "reward", "rewards5", "obs", "ret_total", "ret_episode"):
        assert torch.isfinite(getattr(res, name)).all(), name
    a = res.actions
    inside = ((a > -1.0) & (a < 1.0)).float().mean().item()
    assert inside > 0.5, "the clamp hides the policy: only %.2f of the actions lie inside (-1, 1)" % inside
    ids = list(ids)
    for i in range(len(ids)):
        for j in range(i + 1, len(ids)):
            if ids[i] != ids[j]:
                assert not torch.equal(a[0, i], a[0, j]), (i, j)


def _assert_actions_are_the_definition(pol, ids, x0, res):
    """(a) actions[t] = reference(x_t), x_0 the observation before the call, x_t = obs[t - 1] (res recorded with obs_every = 1)."""
    T = res.actions.shape[0]
    assert res.obs.shape[0] == T and res.obs_steps == list(range(T))
    obs, act = res.obs.cpu().numpy(), res.actions.cpu().numpy()
    x = x0.cpu().numpy()
    for t in range(T):
        assert np.array_equal(pol.reference(x, np.asarray(ids)), act[t]), "action of step %d" % t
        x = obs[t]


def _assert_twin_rollout_reproduces(twin, env, res):
    """(b) a twin env in the same start state running rollout(actions) reproduces everything."""
    obs, rew, done, info = twin.rollout(res.actions, obs_every=1, rewards5=True)
    assert torch.equal(obs, res.obs), "obs"
    assert torch.equal(rew, res.reward), "reward"
    assert done.dtype == torch.bool and res.done.dtype == torch.bool and torch.equal(done, res.done), "done"
    assert torch.equal(info["rewards"], res.rewards5), "rewards5"
    assert torch.equal(twin.steps, env.steps)
    _assert_same_state(twin, env)


def _returns(reward, done):
    """ret_total, ret_episode, episode_len by their definitions, in float64 from the recorded float32 reward and done."""
    r, d = reward.cpu().numpy().astype(np.float64), done.cpu().numpy()
    T, N = r.shape
    tot, ep, ln, over = np.zeros(N), np.zeros(N), np.zeros(N, np.int32), np.zeros(N, bool)
    for t in range(T):
        tot = tot + r[t]
        ep = np.where(over, ep, ep + r[t])
        ln = np.where(over, ln, ln + 1).astype(np.int32)
        over = over | d[t]
    return tot, ep, ln


def _assert_returns_are_their_definitions(res):
    tot, ep, ln = _returns(res.reward, res.done)
    assert res.ret_total.dtype == torch.float64 and res.ret_episode.dtype == torch.float64 and res.episode_len.dtype == torch.int32
    assert np.array_equal(res.ret_total.cpu().numpy(), tot), "ret_total"
    assert np.array_equal(res.ret_episode.cpu().numpy(), ep), "ret_episode"
    assert np.array_equal(res.episode_len.cpu().numpy(), ln), "episode_len"


_CASES = [(robot, H, "bullet", ar) for robot in ("humanoid", "ant") for H in (0, 1, 70, 256) for ar in (True, False)] + \
         [(robot, 70, "mujoco", ar) for robot in ("humanoid", "ant") for ar in (True, False)]


@pytest.mark.parametrize("robot,H,preset,auto_reset", _CASES)
def test_closed_loop_is_the_definition(robot, H, preset, auto_reset):
    env, twin = _make(robot, 5, preset, auto_reset), _make(robot, 5, preset, auto_reset)
    pol = _policy(env, H)
    x0 = env._obs.clone()
    gs = env.global_step
    res = env.rollout_policy(pol, T_MAX, IDS, record=True, obs_every=1)
    assert env.global_step == gs + T_MAX
    assert res.actions.shape == (T_MAX, 5, env.n_joints) and res.reward.shape == (T_MAX, 5) and res.rewards5.shape == (T_MAX, 5, 5)
    _assert_recorded_run_means_something(res, IDS)
    if auto_reset:      # both episode ends happened, each followed by a fresh episode
        assert res.done[4].all() and res.done[9].all() and not res.done[5].any() and int(env.steps.max()) == 2
        assert (res.episode_len == 5).all()
    else:               # stepped past done: the envs went on, done stays set
        assert res.done[4:].all() and int(env.steps.min()) == T_MAX
    _assert_actions_are_the_definition(pol, IDS, x0, res)
    _assert_twin_rollout_reproduces(twin, env, res)
    _assert_returns_are_their_definitions(res)
    assert not torch.equal(res.ret_total, res.ret_episode)       # (the episode's return stops at step 4, the total does not)


def test_records_off_gives_the_same_returns_state_and_observation():
    env = _make("ant", 5)
    pol = _policy(env, 70)
    sd0, x0 = env.state_dict(), env._obs.clone()
    rec = env.rollout_policy(pol, T_MAX, IDS, record=True, obs_every=1, obs0=x0)
    end = {k: getattr(env, k).clone() for k in env._STATE_KEYS}
    env.load_state_dict(sd0)
    env._reward.fill_(123.0)
    env._done.fill_(True)
    off = env.rollout_policy(pol, T_MAX, IDS, record=False, obs_every=0, obs0=x0)
    assert off.actions is None and off.reward is None and off.done is None and off.rewards5 is None
    assert torch.equal(off.ret_total, rec.ret_total) and torch.equal(off.ret_episode, rec.ret_episode)
    assert torch.equal(off.episode_len, rec.episode_len)
    for k in env._STATE_KEYS:
        assert torch.equal(getattr(env, k), end[k]), k
    assert off.obs is env._obs and off.obs_steps == [T_MAX - 1] and torch.equal(env._obs, rec.obs[-1])
    assert bool((env._reward == 123.0).all()) and bool(env._done.all())      # the persistent reward / done buffers are step()'s


@pytest.mark.parametrize("robot", ["humanoid", "ant"])
def test_one_env_one_step(robot):
    env, twin = _make(robot, 1), _make(robot, 1)
    pol = _policy(env, 70)
    x0 = env._obs.clone()
    res = env.rollout_policy(pol, 1, [2], record=True, obs_every=1)
    assert torch.isfinite(res.actions).all() and torch.isfinite(res.reward).all()
    _assert_actions_are_the_definition(pol, [2], x0, res)
    _assert_twin_rollout_reproduces(twin, env, res)
    _assert_returns_are_their_definitions(res)
    assert int(res.episode_len[0]) == 1


def test_relu_of_minus_zero_is_plus_zero_on_the_device():
    """A hidden unit whose pre-activation is exactly -0.0 at step 0: b1 = -0.0 and every product w1 * x is -0.0 (a zero weight of
    the sign opposite to x's). h must be +0.0: then a = b2 + w2 * h = -0.0 + (-1 * +0.0) = -0.0, where an h of -0.0 gives +0.0."""
    from metagym_amd.metalocomotion import WalkerPolicy
    env = _make("ant", 1)
    x0 = env._obs.clone()
    x = x0.cpu().numpy()
    w1 = np.where(np.signbit(x[0]), np.float32(0.0), np.float32(-0.0)).astype(np.float32)[None, None, :]
    pol = WalkerPolicy(w1, np.full((1, 1), -0.0, np.float32), np.full((1, env.n_joints, 1), -1.0, np.float32),
                       np.full((1, env.n_joints), -0.0, np.float32))
    z = np.float32(-0.0)
    for i in range(env.obs_dim):
        z = np.float32(z + np.float32(w1[0, 0, i] * x[0, i]))
    assert z == 0 and np.signbit(z)                       # the premise: the pre-activation is -0.0
    res = env.rollout_policy(pol, 1, record=True, obs_every=1)
    a = res.actions.cpu().numpy()[0]
    assert np.array_equal(a, np.zeros_like(a)) and np.signbit(a).all()
    assert np.array_equal(np.signbit(pol.reference(x, np.array([0]))), np.signbit(a))


def test_chunked_calls_and_a_following_step_continue_like_one_call():
    whole, parts, mixed = _make("ant", 5), _make("ant", 5), _make("ant", 5)
    pol = _policy(whole, 70)
    ids = np.asarray(IDS)
    w = whole.rollout_policy(pol, T_MAX, IDS, record=True)
    p1 = parts.rollout_policy(pol, 7, IDS, record=True)
    p2 = parts.rollout_policy(pol, 5, IDS, record=True)
    assert torch.equal(torch.cat([p1.reward, p2.reward]), w.reward) and torch.equal(torch.cat([p1.done, p2.done]), w.done)
    assert torch.equal(torch.cat([p1.actions, p2.actions]), w.actions)
    assert torch.equal(parts._obs, whole._obs)
    _assert_same_state(parts, whole)
    # ret_total of the chunks adds up in float64 order: the second chunk's rewards one by one onto the first chunk's sum
    tot = p1.ret_total.cpu().numpy().copy()
    r2 = p2.reward.cpu().numpy().astype(np.float64)
    for t in range(5):
        tot = tot + r2[t]
    assert np.array_equal(tot, w.ret_total.cpu().numpy())
    m1 = mixed.rollout_policy(pol, 11, IDS, record=True)
    a = pol.reference(mixed._obs.cpu().numpy(), ids)
    o, r, d, _info = mixed.step(torch.from_numpy(a).to(DEV))
    assert torch.equal(torch.cat([m1.reward, r[None]]), w.reward) and torch.equal(torch.cat([m1.done, d[None]]), w.done)
    assert torch.equal(o, whole._obs)
    _assert_same_state(mixed, whole)


def test_obs0_carries_the_observation_of_a_checkpoint():
    env = _make("ant", 5)
    pol = _policy(env, 70)
    env.rollout_policy(pol, 3, IDS)                       # a state whose observation carries feet flags
    sd, saved = env.state_dict(), env._obs.clone()
    first = env.rollout_policy(pol, T_MAX, IDS, record=True)
    end = {k: getattr(env, k).clone() for k in env._STATE_KEYS}
    assert not torch.equal(env._obs, saved)               # the buffer now holds another observation
    env.load_state_dict(sd)                               # ... and load_state_dict does not restore it
    again = env.rollout_policy(pol, T_MAX, IDS, record=True, obs0=saved)
    assert torch.equal(again.actions, first.actions) and torch.equal(again.reward, first.reward)
    assert torch.equal(again.ret_total, first.ret_total) and torch.equal(again.ret_episode, first.ret_episode)
    for k in env._STATE_KEYS:
        assert torch.equal(getattr(env, k), end[k]), k
    env.load_state_dict(sd)
    other = env.rollout_policy(pol, T_MAX, IDS, record=True)      # the default: whatever the buffer holds
    assert not torch.equal(other.actions[0], first.actions[0])


def test_a_shape_generic_robot():
    """The shape-generic instantiation (<14 slots, 8 joints>): terrain boxes, a push, per-proxy friction, foot forces."""
    def mk():
        env = _make("ant", 5, per_proxy_friction=True, foot_force=True)
        env.set_terrain([((0.6, 0.6, 0.04), (0.2, 0.0, 0.04), (0, 0, 0, 1), 0.9),
                         ((0.3, 0.3, 0.08), (-0.4, 0.3, 0.08), (0, 0, 0.3, 1), 0.5)])
        w = torch.zeros(6, 5, dtype=torch.float64, device=DEV)
        w[0], w[2], w[4] = 40.0, 15.0, 0.1
        env.set_external_wrench(w)
        return env
    env, twin = mk(), mk()
    pol = _policy(env, 70)
    x0 = env._obs.clone()
    res = env.rollout_policy(pol, T_MAX, IDS, record=True, obs_every=1)
    _assert_recorded_run_means_something(res, IDS)
    _assert_actions_are_the_definition(pol, IDS, x0, res)
    _assert_twin_rollout_reproduces(twin, env, res)       # bad_contacts and foot_force after the last step included
    assert float(env.foot_force.abs().sum()) > 0.0


def test_graph_replay_is_bit_identical():
    eager, graphed = _make("ant", 5), _make("ant", 5)
    pol = _policy(eager, 70)
    sd0, x0 = graphed.state_dict(), graphed._obs.clone()
    outs = []

    def one_call():
        outs.clear()
        outs.append(graphed.rollout_policy(pol, T_MAX, IDS))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):             # warm-up outside capture (lazy module load, the uploads of the policy and the ids)
        one_call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphed.load_state_dict(sd0)              # global_step too: the Philox step index is a launch argument, frozen by the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        one_call()
    graphed.load_state_dict(sd0)
    graphed._obs.copy_(x0)                    # the default obs0 is the persistent buffer: the replay reads what it holds now
    g.replay()
    want = eager.rollout_policy(pol, T_MAX, IDS)
    got = outs[0]
    assert torch.equal(got.ret_total, want.ret_total) and torch.equal(got.ret_episode, want.ret_episode)
    assert torch.equal(got.episode_len, want.episode_len)
    assert torch.equal(graphed._obs, eager._obs)
    for k in eager._STATE_KEYS:
        assert torch.equal(getattr(graphed, k), getattr(eager, k)), k


def test_envs_in_one_state_share_one_policy():
    env = _make("ant", 5, auto_reset=False)
    pol = _policy(env, 70, P=1)
    sd0 = env.state_dict()
    fork = dict(sd0)                          # env 0's state and task in every env
    for k in env._STATE_KEYS + ("task_id",):
        fork[k] = sd0[k][..., :1].expand_as(sd0[k]).contiguous()
    env.load_state_dict(fork)
    x0 = env._obs[:1].expand_as(env._obs).contiguous()
    res = env.rollout_policy(pol, T_MAX, record=True, obs0=x0)
    assert torch.isfinite(res.actions).all() and torch.isfinite(res.ret_total).all()
    assert torch.equal(res.actions, res.actions[:, :1].expand_as(res.actions))
    assert torch.equal(res.reward, res.reward[:, :1].expand_as(res.reward))
    for name in ("ret_total", "ret_episode", "episode_len"):
        v = getattr(res, name)
        assert torch.equal(v, v[:1].expand_as(v)), name


def test_refused_calls_leave_the_env_alone():
    from metagym_amd._lib import MetaGymHipError
    from metagym_amd.metalocomotion import WalkerPolicy
    env = _make("ant", 3, mapping="lane")
    pol = _policy(env, 4)
    before = {k: getattr(env, k).clone() for k in env._STATE_KEYS}
    gs = env.global_step
    with pytest.raises(MetaGymHipError, match="mapping"):
        env.rollout_policy(pol, 4)
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 4, policy_ids=[0, 3, 1])              # P = 3: ids 0..2
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 0)
    with pytest.raises(ValueError):
        env.rollout_policy(WalkerPolicy.linear(np.zeros((1, 17, 44), np.float32), np.zeros((1, 17), np.float32)), 4)   # a humanoid's
    assert env.global_step == gs
    for k in env._STATE_KEYS:
        assert torch.equal(getattr(env, k), before[k]), k
