"""WalkerBatchEnv.rollout_policy with a WalkerRecurrentPolicy / mg_walker_rpolicy_rollout against what it is defined as: the
policy's float32 definition (`WalkerRecurrentPolicy.reference`, numpy) fed the recorded observations, rewards and dones step by
step from the start carry, and `rollout(actions)` on the actions that gives. Every comparison is torch.equal / np.array_equal,
for the reasons in tests/test_walker_policy_gpu.py's docstring: shared device code, no contraction in the policy, a reference
that keeps the kernel's order of operations. Shapes are that file's smallest: N = 5, P = 3, T = 12, max_steps = 5, two body
variants. H = 1, 64, 65, 256: one unit, a full wave, a second unit on lane 0, four units per lane.
Argument errors that need no device: tests/test_walker_rpolicy.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_MAX, MAX_STEPS = 12, 5            # every env ends an episode inside the rollout, at steps 4 and 9
IDS = [0, 2, 1, 1, 0]               # P = 3 policies over N = 5 envs
CARRY = ("h", "prev_action", "prev_reward", "prev_done")


def _cls(robot):
    import metagym_amd.metalocomotion as ml
    return {"humanoid": ml.MetaHumanoidEnv, "ant": ml.MetaAntEnv}[robot]


_MODELS = {}


def _make(robot, n, auto_reset=True, **kw):
    env = _cls(robot)(num_envs=n, device=DEV, max_steps=MAX_STEPS, auto_reset=auto_reset, seed=11, env_id_base=7, **kw)
    key = (robot, env.preset)
    if key not in _MODELS:              # two body variants, parsed once per robot and preset
        _MODELS[key] = [env._to_model(t) for t in env.tra_tasks[:2]]
    env.set_task(_MODELS[key])
    env.reset(seed=3)
    return env


_POLICIES = {}


def _policy(env, H, P=3, seed=17, wh=True):
    """Weights uniform in +-0.05, biases in +-0.1, from a fixed generator. wh=False: the same policy with wh zeroed."""
    from metagym_amd.metalocomotion import WalkerRecurrentPolicy
    D, A = env.obs_dim, env.n_joints
    key = (D, A, H, P, seed)
    if key not in _POLICIES:
        g = np.random.RandomState(seed)
        u = lambda s, *shape: g.uniform(-s, s, size=shape).astype(np.float32)
        _POLICIES[key] = WalkerRecurrentPolicy(u(0.05, P, H, D), u(0.05, P, H, A), u(0.05, P, H), u(0.05, P, H), u(0.05, P, H, H),
                                               u(0.1, P, H), u(0.05, P, A, H), u(0.1, P, A))
    pol = _POLICIES[key]
    if wh:
        return pol
    return WalkerRecurrentPolicy(pol.wx, pol.wa, pol.wr, pol.wd, np.zeros_like(pol.wh), pol.b, pol.wo, pol.bo)


def _fresh(env, H):
    from metagym_amd.metalocomotion import WalkerPolicyState
    return WalkerPolicyState(env.num_envs, H, env.n_joints, DEV)


def _assert_same_state(a, b, global_step=True):
    for k in a._STATE_KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    if a.foot_force is not None:
        assert torch.equal(a.foot_force, b.foot_force), "foot_force"
    if global_step:
        assert a.global_step == b.global_step


def _assert_same_carry(a, b):
    for k in CARRY:
        x, y = getattr(a, k), getattr(b, k)
        x = x.cpu().numpy() if hasattr(x, "cpu") else x
        y = y.cpu().numpy() if hasattr(y, "cpu") else y
        assert x.dtype == y.dtype and np.array_equal(x, y), k
        if x.dtype == np.float32:
            assert np.array_equal(np.signbit(x), np.signbit(y)), k


def _assert_recorded_run_means_something(res, ids):
    """Conditions on a recorded run, so that a pass of the comparisons means something."""
    for name in ("actions", "reward", "rewards5", "obs", "ret_total", "ret_episode"):
        assert torch.isfinite(getattr(res, name)).all(), name
    assert torch.isfinite(res.state.h).all()
    a = res.actions
    inside = ((a > -1.0) & (a < 1.0)).float().mean().item()
    assert inside > 0.5, "the clamp hides the policy: only %.2f of the actions lie inside (-1, 1)" % inside
    ids = list(ids)
    for i in range(len(ids)):
        for j in range(i + 1, len(ids)):
            if ids[i] != ids[j]:
                assert not torch.equal(a[0, i], a[0, j]), (i, j)


def _assert_actions_and_carry_are_the_definition(pol, ids, x0, start, res, episodic):
    """(a) `reference`, fed x_0 = the observation before the call and then the recorded observations, rewards and dones (res
    recorded with obs_every = 1), from the start carry, gives every recorded action and the end carry."""
    T = res.actions.shape[0]
    assert res.obs.shape[0] == T and res.obs_steps == list(range(T))
    obs, act = res.obs.cpu().numpy(), res.actions.cpu().numpy()
    rew, done = res.reward.cpu().numpy(), res.done.cpu().numpy()
    x, st = x0.cpu().numpy(), start.numpy()
    for t in range(T):
        a, st = pol.reference(x, np.asarray(ids), st)
        assert np.array_equal(a, act[t]), "action of step %d" % t
        st = st.observed(rew[t], done[t], clear=done[t] if episodic else None)
        x = obs[t]
    _assert_same_carry(st, res.state)


def _assert_twin_rollout_reproduces(twin, env, res):
    """(b) a twin env in the same start state running rollout(actions) reproduces everything."""
    obs, rew, done, info = twin.rollout(res.actions, obs_every=1, rewards5=True)
    assert torch.equal(obs, res.obs), "obs"
    assert torch.equal(rew, res.reward), "reward"
    assert done.dtype == torch.bool and res.done.dtype == torch.bool and torch.equal(done, res.done), "done"
    assert torch.equal(info["rewards"], res.rewards5), "rewards5"
    assert torch.equal(twin.steps, env.steps)
    _assert_same_state(twin, env)


def _assert_returns_are_their_definitions(res):
    """ret_total, ret_episode, episode_len by their definitions, in float64 from the recorded float32 reward and done."""
    r, d = res.reward.cpu().numpy().astype(np.float64), res.done.cpu().numpy()
    T, N = r.shape
    tot, ep, ln, over = np.zeros(N), np.zeros(N), np.zeros(N, np.int32), np.zeros(N, bool)
    for t in range(T):
        tot = tot + r[t]
        ep = np.where(over, ep, ep + r[t])
        ln = np.where(over, ln, ln + 1).astype(np.int32)
        over = over | d[t]
    assert res.ret_total.dtype == torch.float64 and res.ret_episode.dtype == torch.float64 and res.episode_len.dtype == torch.int32
    assert np.array_equal(res.ret_total.cpu().numpy(), tot), "ret_total"
    assert np.array_equal(res.ret_episode.cpu().numpy(), ep), "ret_episode"
    assert np.array_equal(res.episode_len.cpu().numpy(), ln), "episode_len"


_MODES = [(True, False), (True, True), (False, False)]          # (auto_reset, episodic): episodic on where auto_reset is


@pytest.mark.parametrize("auto_reset,episodic", _MODES)
@pytest.mark.parametrize("H", [1, 64, 65, 256])
@pytest.mark.parametrize("robot", ["humanoid", "ant"])
def test_closed_loop_is_the_definition(robot, H, auto_reset, episodic):
    env, twin = _make(robot, 5, auto_reset), _make(robot, 5, auto_reset)
    pol = _policy(env, H)
    x0 = env._obs.clone()
    gs = env.global_step
    start = _fresh(env, H)
    start.h.uniform_(-1.0, 1.0, generator=torch.Generator(device=DEV).manual_seed(5))      # a carry that is not the fresh one
    start.prev_action.fill_(0.25)
    start.prev_reward.fill_(-0.5)
    start.prev_done[1] = 1
    st = start.clone()
    res = env.rollout_policy(pol, T_MAX, IDS, record=True, obs_every=1, state=st, episodic=episodic)
    assert res.state is st and env.global_step == gs + T_MAX
    assert res.actions.shape == (T_MAX, 5, env.n_joints) and res.reward.shape == (T_MAX, 5) and res.rewards5.shape == (T_MAX, 5, 5)
    _assert_recorded_run_means_something(res, IDS)
    if auto_reset:      # both episode ends happened, each followed by a fresh episode
        assert res.done[4].all() and res.done[9].all() and not res.done[5].any() and int(env.steps.max()) == 2
        assert (res.episode_len == 5).all()
    else:               # stepped past done: the envs went on, done stays set
        assert res.done[4:].all() and int(env.steps.min()) == T_MAX
    _assert_actions_and_carry_are_the_definition(pol, IDS, x0, start, res, episodic)
    assert torch.equal(st.prev_action, res.actions[-1]) and torch.equal(st.prev_reward, res.reward[-1])
    assert torch.equal(st.prev_done.bool(), res.done[-1])
    _assert_twin_rollout_reproduces(twin, env, res)
    _assert_returns_are_their_definitions(res)
    assert not torch.equal(res.ret_total, res.ret_episode)       # (the episode's return stops at step 4, the total does not)


@pytest.mark.parametrize("robot", ["humanoid", "ant"])
def test_the_memory_is_used(robot):
    H = 65
    runs = {}
    for name, wh, episodic in (("plain", True, False), ("no_wh", False, False), ("episodic", True, True)):
        env = _make(robot, 5)
        pol = _policy(env, H, wh=wh)
        runs[name] = env.rollout_policy(pol, T_MAX, IDS, record=True, obs_every=1, episodic=episodic)
    plain, no_wh, epi = runs["plain"], runs["no_wh"], runs["episodic"]
    # h = 0 at step 0: wh multiplies zeros. From step 1 on the memory is not zero and wh matters.
    assert torch.equal(plain.actions[0], no_wh.actions[0])
    for t in range(1, T_MAX):
        assert not torch.equal(plain.actions[t], no_wh.actions[t]), t
    # up to the first done the two agree; the step after it sees the kept carry or the zeroed one
    assert torch.equal(plain.actions[:5], epi.actions[:5]) and torch.equal(plain.obs[:5], epi.obs[:5])
    assert plain.done[4].all()
    for e in range(5):
        assert not torch.equal(plain.actions[5, e], epi.actions[5, e]), e
    env = _make(robot, 5)
    pol = _policy(env, H)
    from metagym_amd.metalocomotion import WalkerPolicyState
    a, _ = pol.reference(epi.obs[4].cpu().numpy(), np.asarray(IDS), WalkerPolicyState(5, H, env.n_joints))
    assert np.array_equal(a, epi.actions[5].cpu().numpy())       # episodic: step 5 starts from the zero carry


@pytest.mark.parametrize("episodic", [False, True])
def test_chunks_through_one_state_object_are_one_call(episodic):
    whole, parts = _make("ant", 5), _make("ant", 5)
    pol = _policy(whole, 65)
    w = whole.rollout_policy(pol, T_MAX, IDS, record=True, state=None, episodic=episodic)      # state=None: a fresh zero carry
    st = _fresh(parts, 65)
    p1 = parts.rollout_policy(pol, 5, IDS, record=True, state=st, episodic=episodic)           # the cut falls right after a done
    assert p1.done[4].all() and p1.state is st
    assert bool(st.prev_done.all()) != episodic                  # kept: pd = 1; episodic: the done cleared the carry
    if episodic:
        for k in CARRY:
            assert not getattr(st, k).any(), k
    p2 = parts.rollout_policy(pol, 7, IDS, record=True, state=st, episodic=episodic)
    assert p2.state is st
    for name in ("actions", "reward", "done", "rewards5"):
        assert torch.equal(torch.cat([getattr(p1, name), getattr(p2, name)]), getattr(w, name)), name
    assert torch.equal(parts._obs, whole._obs)
    _assert_same_state(parts, whole)
    _assert_same_carry(st, w.state)
    fresh = _make("ant", 5)
    f = fresh.rollout_policy(pol, T_MAX, IDS, record=True, state=_fresh(fresh, 65), episodic=episodic)
    assert torch.equal(f.actions, w.actions) and torch.equal(f.ret_total, w.ret_total)
    _assert_same_carry(f.state, w.state)
    _assert_same_state(fresh, whole)


def test_clamp_edges_on_the_device():
    """Pre-activations exactly 1, nextafter(1, 2), -1, nextafter(-1, -2) and -0.0 at step 0 of a fresh carry: every weight is
    a zero whose sign makes its product -0.0 (x by its own sign; pa, pr, pd, h are +0.0), so z is the bias, bit for bit. The
    output layer is zero: the action is 0 and the physics sees nothing unusual. (NaN: tests/test_walker_rpolicy.py.)"""
    from metagym_amd.metalocomotion import WalkerRecurrentPolicy
    env = _make("ant", 1)
    D, A = env.obs_dim, env.n_joints
    x = env._obs.cpu().numpy()
    f32 = np.float32
    up, dn = np.nextafter(f32(1), f32(2)), np.nextafter(f32(-1), f32(-2))
    b = np.array([[1.0, up, -1.0, dn, -0.0]], f32)
    H = b.shape[1]
    neg = lambda *s: np.full(s, -0.0, f32)
    wx = np.broadcast_to(np.where(np.signbit(x[0]), f32(0.0), f32(-0.0)).astype(f32)[None, None, :], (1, H, D)).copy()
    pol = WalkerRecurrentPolicy(wx, neg(1, H, A), neg(1, H), neg(1, H), neg(1, H, H), b, np.zeros((1, A, H), f32), np.zeros((1, A), f32))
    res = env.rollout_policy(pol, 1, record=True, obs_every=1)
    h = res.state.h.cpu().numpy()[0]
    assert np.array_equal(h, np.array([1.0, 1.0, -1.0, -1.0, 0.0], f32))
    assert np.array_equal(np.signbit(h), [False, False, True, True, True])       # -0 stays -0
    _, want = pol.reference(x, np.array([0]), _fresh(env, H))
    assert np.array_equal(want.h[0], h) and np.array_equal(np.signbit(want.h[0]), np.signbit(h))
    assert not res.actions.any()


@pytest.mark.parametrize("robot", ["humanoid", "ant"])
def test_one_env_one_step(robot):
    env, twin = _make(robot, 1), _make(robot, 1)
    pol = _policy(env, 65)
    x0 = env._obs.clone()
    start = _fresh(env, 65)
    res = env.rollout_policy(pol, 1, [2], record=True, obs_every=1)
    assert torch.isfinite(res.actions).all() and torch.isfinite(res.reward).all()
    _assert_actions_and_carry_are_the_definition(pol, [2], x0, start, res, False)
    _assert_twin_rollout_reproduces(twin, env, res)
    _assert_returns_are_their_definitions(res)
    assert int(res.episode_len[0]) == 1


def test_records_off_gives_the_same_returns_state_observation_and_carry():
    env = _make("ant", 5)
    pol = _policy(env, 65)
    sd0, x0 = env.state_dict(), env._obs.clone()
    rec = env.rollout_policy(pol, T_MAX, IDS, record=True, obs_every=1, obs0=x0)
    end = {k: getattr(env, k).clone() for k in env._STATE_KEYS}
    env.load_state_dict(sd0)
    off = env.rollout_policy(pol, T_MAX, IDS, record=False, obs_every=0, obs0=x0)
    assert off.actions is None and off.reward is None and off.done is None and off.rewards5 is None
    assert torch.equal(off.ret_total, rec.ret_total) and torch.equal(off.ret_episode, rec.ret_episode)
    assert torch.equal(off.episode_len, rec.episode_len)
    for k in env._STATE_KEYS:
        assert torch.equal(getattr(env, k), end[k]), k
    assert off.obs is env._obs and off.obs_steps == [T_MAX - 1] and torch.equal(env._obs, rec.obs[-1])
    assert off.state is not rec.state
    _assert_same_carry(off.state, rec.state)


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
    pol = _policy(env, 65)
    x0 = env._obs.clone()
    start = _fresh(env, 65)
    res = env.rollout_policy(pol, T_MAX, IDS, record=True, obs_every=1)
    _assert_recorded_run_means_something(res, IDS)
    _assert_actions_and_carry_are_the_definition(pol, IDS, x0, start, res, False)
    _assert_twin_rollout_reproduces(twin, env, res)       # bad_contacts and foot_force after the last step included
    assert float(env.foot_force.abs().sum()) > 0.0


def test_graph_replays_with_a_carry_are_eager_calls():
    """One capture of a call with a carry; two replays equal two eager calls through one carry. (The Philox step index is a
    launch argument, frozen by the capture: the eager twin's second call is given the same one.)"""
    eager, graphed = _make("ant", 5), _make("ant", 5)
    pol = _policy(eager, 65)
    sd0, x0 = graphed.state_dict(), graphed._obs.clone()
    st_g, st_e = _fresh(graphed, 65), _fresh(eager, 65)
    outs = []

    def one_call():
        outs.clear()
        outs.append(graphed.rollout_policy(pol, T_MAX, IDS, state=st_g))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):             # warm-up outside capture (lazy module load, the uploads of the policy and the ids)
        one_call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphed.load_state_dict(sd0)              # global_step too
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        one_call()
    graphed.load_state_dict(sd0)
    graphed._obs.copy_(x0)                    # the default obs0 is the persistent buffer: the replay reads what it holds now
    for k in CARRY:
        getattr(st_g, k).zero_()              # ... and the carry the warm-up left
    gs0 = eager.global_step
    for call in range(2):
        g.replay()
        eager.global_step = gs0
        want = eager.rollout_policy(pol, T_MAX, IDS, state=st_e)
        got = outs[0]
        assert got.state is st_g and want.state is st_e
        assert torch.equal(got.ret_total, want.ret_total) and torch.equal(got.ret_episode, want.ret_episode), call
        assert torch.equal(got.episode_len, want.episode_len)
        assert torch.equal(graphed._obs, eager._obs)
        _assert_same_state(graphed, eager, global_step=False)
        _assert_same_carry(st_g, st_e)
    assert bool(st_g.h.any())


def test_refused_calls_leave_the_env_and_the_carry_alone():
    from metagym_amd._lib import MetaGymHipError
    from metagym_amd.metalocomotion import WalkerPolicy, WalkerPolicyState, WalkerRecurrentPolicy
    z = lambda *s: np.zeros(s, np.float32)

    def check(env, st, calls):
        st.h.fill_(0.5)
        st.prev_action.fill_(-0.25)
        st.prev_reward.fill_(2.0)
        st.prev_done.fill_(1)
        keep = st.clone()
        before = {k: getattr(env, k).clone() for k in env._STATE_KEYS}
        gs, obs = env.global_step, env._obs.clone()
        for exc, match, call in calls:
            with pytest.raises(exc, match=match):
                call()
        assert env.global_step == gs and torch.equal(env._obs, obs)
        for k in env._STATE_KEYS:
            assert torch.equal(getattr(env, k), before[k]), k
        _assert_same_carry(st, keep)

    env = _make("ant", 3, auto_reset=False)
    D, A, H = env.obs_dim, env.n_joints, 4
    pol = _policy(env, H)
    st = _fresh(env, H)
    humanoid = WalkerRecurrentPolicy(z(1, H, 44), z(1, H, 17), z(1, H), z(1, H), z(1, H, H), z(1, H), z(1, 17, H), z(1, 17))
    wrong_a = WalkerRecurrentPolicy(z(1, H, D), z(1, H, A + 1), z(1, H), z(1, H), z(1, H, H), z(1, H), z(1, A + 1, H), z(1, A + 1))
    mlp = WalkerPolicy(z(1, H, D), z(1, H), z(1, A, H), z(1, A))
    check(env, st, [
        (ValueError, "observation", lambda: env.rollout_policy(humanoid, 4, state=st)),              # wrong D
        (ValueError, "actions", lambda: env.rollout_policy(wrong_a, 4)),                             # wrong A
        (ValueError, "state.h", lambda: env.rollout_policy(pol, 4, state=WalkerPolicyState(4, H, A, DEV))),           # another N
        (ValueError, "state.h", lambda: env.rollout_policy(pol, 4, state=WalkerPolicyState(3, H + 1, A, DEV))),       # another H
        (ValueError, "state.prev_action", lambda: env.rollout_policy(pol, 4, state=WalkerPolicyState(3, H, A + 1, DEV))),   # another A
        (ValueError, "lives on", lambda: env.rollout_policy(pol, 4, state=WalkerPolicyState(3, H, A, "cpu"))),        # another device
        (ValueError, "torch tensors", lambda: env.rollout_policy(pol, 4, state=WalkerPolicyState(3, H, A))),          # a numpy carry
        (TypeError, "WalkerPolicyState", lambda: env.rollout_policy(pol, 4, state=object())),
        (ValueError, "policy_ids", lambda: env.rollout_policy(pol, 4, policy_ids=[0, 3, 1], state=st)),               # P = 3: ids 0..2
        (ValueError, "steps", lambda: env.rollout_policy(pol, 0, state=st)),
        (ValueError, "auto_reset", lambda: env.rollout_policy(pol, 4, state=st, episodic=True)),     # episodic without auto_reset
        (TypeError, "WalkerRecurrentPolicy", lambda: env.rollout_policy(mlp, 4, state=st)),
        (TypeError, "WalkerRecurrentPolicy", lambda: env.rollout_policy(mlp, 4, episodic=True)),
    ])
    lane = _make("ant", 3, mapping="lane")
    check(lane, st, [(MetaGymHipError, "mapping", lambda: lane.rollout_policy(pol, 4, state=st))])
