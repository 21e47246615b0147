"""CPU-side checks of the recurrent walker policies (metagym_amd/metalocomotion/policy.py: WalkerRecurrentPolicy,
WalkerPolicyState) and of mg_walker_rpolicy_rollout's argument errors (include/metagym_hip.h): the packed layout round-trips,
the float32 definition keeps its order and its clamp edges, the carry bookkeeping does what `episodic` does, and every wrong
argument is a code with a message, decided on the host before any launch (so no GPU is needed). The kernel itself:
tests/test_walker_rpolicy_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from metagym_amd.metalocomotion.policy import (MAX_HIDDEN, WalkerPolicy, WalkerPolicyState, WalkerRecurrentPolicy,
                                                recurrent_param_count)

NULL_POINTER, BAD_SIZE, BAD_CONFIG, UNSUPPORTED = -1001, -1002, -1003, -1004
D, A = 28, 8                                  # the ant's observation and action widths
f32 = np.float32


def _policy(P, H, d=D, a=A, seed=0, scale=1.0):
    g = np.random.RandomState(seed)
    u = lambda *s: g.uniform(-scale, scale, size=s).astype(f32)
    return WalkerRecurrentPolicy(u(P, H, d), u(P, H, a), u(P, H), u(P, H), u(P, H, H), u(P, H), u(P, a, H), u(P, a))


def _state(N, H, a=A, seed=1):
    g = np.random.RandomState(seed)
    return WalkerPolicyState.of(g.uniform(-1, 1, size=(N, H)).astype(f32), g.uniform(-2, 2, size=(N, a)).astype(f32),
                                g.uniform(-3, 3, size=N).astype(f32), (g.uniform(size=N) < 0.5).astype(np.uint8))


@pytest.mark.parametrize("H", [1, 64, 65, 256, 31, 32, 33, 129, 193])
def test_pack_unpack_round_trip_and_layout(H):
    pol = _policy(3, H)
    packed = pol.pack()
    assert packed.dtype == f32 and packed.shape == (3, pol.param_count) and len(pol) == 3
    assert pol.param_count == recurrent_param_count(H, D, A) == H + (D + A + 2 + H) * H + A + H * A
    back = WalkerRecurrentPolicy.unpack(packed, H, D, A)
    assert (back.hidden, back.obs_dim, back.n_act, back.num_policies) == (H, D, A, 3)
    for name in ("wx", "wa", "wr", "wd", "wh", "b", "wo", "bo"):
        assert np.array_equal(getattr(back, name), getattr(pol, name)), name
    # the documented places: b[H], wx [D][H], wa [A][H], wr[H], wd[H], wh [H_in][H_out], bo[A], wo [H][A], no padding
    p, j, i, k, hi = 2, H - 1, 5, 3, H // 2
    assert packed[p, j] == pol.b[p, j]
    assert packed[p, H + i * H + j] == pol.wx[p, j, i]
    assert packed[p, H + (D + k) * H + j] == pol.wa[p, j, k]
    assert packed[p, H + (D + A) * H + j] == pol.wr[p, j]
    assert packed[p, H + (D + A + 1) * H + j] == pol.wd[p, j]
    assert packed[p, H + (D + A + 2 + hi) * H + j] == pol.wh[p, j, hi]
    at = H + (D + A + 2 + H) * H
    assert packed[p, at + k] == pol.bo[p, k]
    assert packed[p, at + A + j * A + k] == pol.wo[p, k, j]
    with pytest.raises(ValueError):
        WalkerRecurrentPolicy.unpack(packed[:, :-1], H, D, A)


def test_param_count_is_the_librarys():
    from metagym_amd import _lib
    lib = _lib.load()
    for H in (1, 64, 65, 256):
        for d, a in ((28, 8), (44, 17), (33, 12)):
            assert lib.mg_walker_rpolicy_param_count(H, d, a) == recurrent_param_count(H, d, a), (H, d, a)
    assert lib.mg_walker_rpolicy_param_count(257, 28, 8) == BAD_SIZE and b"hidden" in lib.mg_last_error()
    assert lib.mg_walker_rpolicy_param_count(0, 28, 8) == BAD_SIZE and b"hidden" in lib.mg_last_error()
    assert lib.mg_walker_rpolicy_param_count(4, 28, 0) == BAD_SIZE and b"n_act" in lib.mg_last_error()
    assert lib.mg_walker_rpolicy_param_count(4, 0, 8) == BAD_SIZE and b"obs_dim" in lib.mg_last_error()
    for bad in (0, MAX_HIDDEN + 1):
        with pytest.raises(ValueError):
            recurrent_param_count(bad, 28, 8)


def test_constructor_refuses_what_is_not_a_policy():
    z = lambda *s: np.zeros(s, f32)
    ok = lambda H=4, P=2: [z(P, H, D), z(P, H, A), z(P, H), z(P, H), z(P, H, H), z(P, H), z(P, A, H), z(P, A)]
    WalkerRecurrentPolicy(*ok())
    WalkerRecurrentPolicy(*ok(MAX_HIDDEN, 1))
    with pytest.raises(ValueError):
        WalkerRecurrentPolicy(*ok(MAX_HIDDEN + 1, 1))
    with pytest.raises(ValueError):
        WalkerRecurrentPolicy(*ok(0))
    for at, bad in ((1, z(2, 4, A + 1)), (2, z(2, 5)), (3, z(3, 4)), (4, z(2, 4, 5)), (5, z(2, 5)), (6, z(2, A, 5)),
                    (7, z(2, A + 1)), (0, z(4, D)), (2, z(2, 4, 1))):
        args = ok()
        args[at] = bad
        with pytest.raises(ValueError):
            WalkerRecurrentPolicy(*args)
    args = ok()
    args[4] = np.zeros((2, 4, 4), np.float64)
    with pytest.raises(TypeError):
        WalkerRecurrentPolicy(*args)
    for bad in (np.nan, np.inf, -np.inf):
        args = ok()
        args[4][1, 2, 3] = bad
        with pytest.raises(ValueError):
            WalkerRecurrentPolicy(*args)


def _scalar_reference(pol, x, ids, st):
    """The definition, one float32 operation at a time."""
    N, H = x.shape[0], pol.hidden
    act, hn = np.zeros((N, pol.n_act), f32), np.zeros((N, H), f32)
    with np.errstate(all="ignore"):
        for n in range(N):
            p = int(ids[n])
            for j in range(H):
                z = f32(pol.b[p, j])
                for i in range(pol.obs_dim):
                    z = f32(z + f32(pol.wx[p, j, i] * x[n, i]))
                for k in range(pol.n_act):
                    z = f32(z + f32(pol.wa[p, j, k] * st.prev_action[n, k]))
                z = f32(z + f32(pol.wr[p, j] * st.prev_reward[n]))
                z = f32(z + f32(pol.wd[p, j] * f32(1.0 if st.prev_done[n] else 0.0)))
                for i in range(H):
                    z = f32(z + f32(pol.wh[p, j, i] * st.h[n, i]))
                hn[n, j] = f32(1.0) if z > 1 else (f32(-1.0) if z < -1 else z)
            for k in range(pol.n_act):
                a = f32(pol.bo[p, k])
                for j in range(H):
                    a = f32(a + f32(pol.wo[p, k, j] * hn[n, j]))
                act[n, k] = a
    return act, hn


def test_reference_is_the_scalar_loop():
    g = np.random.RandomState(3)
    pid = np.array([0, 2, 1, 1, 0, 2])
    for H, scale in ((1, 1.0), (5, 0.2), (70, 0.05)):
        pol = _policy(3, H, seed=H + 1, scale=scale)
        xs = (g.uniform(-5, 5, size=(6, D)) * g.choice([1.0, 1e2, 1e-4], size=(6, D))).astype(f32)
        st = _state(6, H, seed=H)
        keep = st.clone()
        a, new = pol.reference(xs, pid, st)
        want_a, want_h = _scalar_reference(pol, xs, pid, st)
        assert a.dtype == f32 and np.array_equal(a, want_a), H
        assert new.h.dtype == f32 and np.array_equal(new.h, want_h), H
        assert np.array_equal(new.prev_action, a) and np.array_equal(new.prev_reward, st.prev_reward)
        assert np.array_equal(new.prev_done, st.prev_done)
        for name in WalkerPolicyState.__slots__:             # the state is read, never written
            assert np.array_equal(getattr(st, name), getattr(keep, name)), name
        if H > 1:
            assert (np.abs(want_h) < 1).any()                # (not everything sits on the clamp)


def test_reference_keeps_the_stated_order():
    # b + wx x0 + wa pa0 + wr pr + wd pd + wh h0 = ((((1e8 + 1) - 1e8) + 1) - 1e8 ... chosen so that any other order shows:
    # z = 0; + 1e8 (x); + 1 (pa) -> 1e8; - 1e8 (pr) -> 0; + 0.25 (pd) -> 0.25; + 0.5 (h) -> 0.75. Right to left gives 0.
    one = lambda v, *s: np.full(s, v, f32)
    pol = WalkerRecurrentPolicy(one(1.0, 1, 1, 1), one(1.0, 1, 1, 1), one(1.0, 1, 1), one(0.25, 1, 1), one(1.0, 1, 1, 1),
                                one(0.0, 1, 1), one(2.0, 1, 1, 1), one(0.5, 1, 1))
    st = WalkerPolicyState.of(one(0.5, 1, 1), one(1.0, 1, 1), one(-1e8, 1), np.array([7], np.uint8))     # (any non-zero done is 1)
    a, new = pol.reference(one(1e8, 1, 1), np.array([0]), st)
    assert np.array_equal(new.h, one(0.75, 1, 1)) and np.array_equal(a, one(2.0, 1, 1))
    with pytest.raises(ValueError):
        pol.reference(np.ones((1, 1), np.float64), np.array([0]), st)
    with pytest.raises(ValueError):
        pol.reference(one(1.0, 1, 1), np.array([1]), st)                         # only policy 0 exists
    with pytest.raises(ValueError):
        pol.reference(one(1.0, 1, 1), np.array([0]), WalkerPolicyState(1, 2, 1))  # another H


def test_clamp_edges_in_reference():
    """Pre-activations exactly 1, nextafter(1, 2), -1, nextafter(-1, -2), -0.0 and NaN. Units 0-4: every product is -0.0 (a zero
    weight of the sign that makes it so), so z is the bias. Unit 5: finite parameters and inputs whose sum is inf + -inf."""
    up, dn = np.nextafter(f32(1), f32(2)), np.nextafter(f32(-1), f32(-2))
    assert up > 1 and dn < -1
    b = np.array([[1.0, up, -1.0, dn, -0.0, 0.0]], f32)
    H = b.shape[1]
    z = lambda *s: np.zeros(s, f32)
    wx = np.full((1, H, 2), -0.0, f32)           # x = (5, 5): -0.0 * 5 = -0.0
    wx[0, 5] = (3e38, -3e38)                     # 3e38 * 5 = inf, then inf + -inf = NaN
    wd = np.full((1, H), -0.0, f32)              # pd = 0 enters as +0.0: -0.0 * +0.0 = -0.0
    wo = np.eye(H, dtype=f32)[None]              # a[k] = h[k] + ...: the action shows h
    pol = WalkerRecurrentPolicy(wx, z(1, H, H), z(1, H), wd, z(1, H, H), b, wo, z(1, H))
    # pa, pr, h = -0.0 under weights +0.0: those products are -0.0 as well (one +0.0 term would turn unit 4's -0.0 into +0.0)
    st = WalkerPolicyState.of(np.full((1, H), -0.0, f32), np.full((1, H), -0.0, f32), np.full(1, -0.0, f32), np.zeros(1, np.uint8))
    x = np.array([[5.0, 5.0]], f32)
    a, new = pol.reference(x, np.array([0]), st)
    h = new.h[0]
    assert np.array_equal(h[:4], np.array([1.0, 1.0, -1.0, -1.0], f32))
    assert h[4] == 0 and np.signbit(h[4])                                        # -0 stays -0
    assert np.isnan(h[5])                                                        # a NaN pre-activation stays NaN
    want_a, want_h = _scalar_reference(pol, x, np.array([0]), st)
    assert np.array_equal(h, want_h[0], equal_nan=True) and np.array_equal(np.signbit(h[:5]), np.signbit(want_h[0, :5]))
    assert np.array_equal(a, want_a, equal_nan=True) and np.isnan(a).all()       # 0 * NaN: the NaN reaches every output


def test_state_is_zero_when_fresh_and_observed_does_the_bookkeeping():
    st = WalkerPolicyState(4, 3, 2)
    assert (st.num_envs, st.hidden, st.n_act, st.device) == (4, 3, 2, None)
    assert st.h.shape == (4, 3) and st.prev_action.shape == (4, 2) and st.prev_reward.shape == (4,) and st.prev_done.shape == (4,)
    assert st.h.dtype == f32 and st.prev_action.dtype == f32 and st.prev_reward.dtype == f32 and st.prev_done.dtype == np.uint8
    for name in WalkerPolicyState.__slots__:
        assert not getattr(st, name).any(), name
    with pytest.raises(ValueError):
        WalkerPolicyState(0, 3, 2)
    with pytest.raises(ValueError):
        WalkerPolicyState(4, MAX_HIDDEN + 1, 2)
    st = _state(4, 3, a=2)
    c = st.clone()
    c.h[0, 0] = 9.0
    assert st.h[0, 0] != 9.0                                                     # a clone owns its arrays
    rew, done = np.array([0.5, -1.5, 2.0, 0.0]), np.array([0, 1, 1, 0], bool)    # (float64 rewards are narrowed)
    out = st.observed(rew, done)
    assert np.array_equal(out.h, st.h) and np.array_equal(out.prev_action, st.prev_action)
    assert out.prev_reward.dtype == f32 and np.array_equal(out.prev_reward, rew.astype(f32))
    assert out.prev_done.dtype == np.uint8 and np.array_equal(out.prev_done, [0, 1, 1, 0])
    out = st.observed(rew, done, clear=done)
    for n in range(4):
        if done[n]:
            assert not out.h[n].any() and not out.prev_action[n].any() and out.prev_reward[n] == 0 and out.prev_done[n] == 0
        else:
            assert np.array_equal(out.h[n], st.h[n]) and np.array_equal(out.prev_action[n], st.prev_action[n])
            assert out.prev_reward[n] == f32(rew[n]) and out.prev_done[n] == 0
    with pytest.raises(ValueError):
        st.observed(rew[:3], done[:3])


# ---- mg_walker_rpolicy_rollout refusals (the helper is that of tests/test_walker_policy.py) ----------------------------
def _fake_call():
    """An ant-shaped call whose every required pointer is a (host) dummy: it passes each check, so one wrong argument at a time
    can be shown to be THE reason for a refusal. Nothing here may reach a launch."""
    from metagym_amd import _lib
    fake = C.create_string_buffer(256)
    addr = C.addressof(fake)
    tp = _lib.WalkerTopology()
    tp.n_bodies, tp.n_joints, tp.n_spheres, tp.n_feet, tp.n_geoms, tp.n_pairs = 5, 4, 5, 4, 5, 0
    for b in range(5):                       # a torso and four one-hinge legs, one proxy per body, the legs are the feet
        tp.body_parent[b] = -1 if b == 0 else 0
        tp.sphere_body[b], tp.geom_body[b] = b, b
        tp.sphere_foot[b] = b - 1
    for j in range(4):
        tp.joint_body[j], tp.foot_body[j] = j + 1, j + 1
    ms = _lib.WalkerModels()
    ms.table, ms.n_tasks, ms.model_stride = addr, 1, 25 * 5 + 12 * 4 + 4 * 5 + 7 * 5
    prm = _lib.WalkerParams()
    prm.time_step, prm.frame_skip, prm.solver_iterations, prm.mapping, prm.max_steps = 0.005, 4, 5, 1, 10
    st = _lib.WalkerState()
    for k in ("task_id", "pos", "rot", "vel", "omega", "q", "qd", "potential", "feet_contact", "steps"):
        setattr(st, k, addr)
    return _lib.load(), tp, ms, prm, st, C.c_void_p(addr), fake


def _policy_desc(p, **kw):
    from metagym_amd import _lib
    d = dict(params_d=p.value, policy_id_d=p.value, n_policies=3, hidden=70, obs_dim=8 + 2 * 4 + 4, n_act=4)
    d.update(kw)
    return _lib.WalkerPolicyDesc(d["params_d"], d["policy_id_d"], d["n_policies"], d["hidden"], d["obs_dim"], d["n_act"])


def _carry(p, **kw):
    from metagym_amd import _lib
    d = dict(h=p.value, prev_action=p.value, prev_reward=p.value, prev_done=p.value)
    d.update(kw)
    return _lib.WalkerRPolicyCarry(d["h"], d["prev_action"], d["prev_reward"], d["prev_done"])


def _caller(lib, tp, ms, prm, st, p):
    ok = dict(topo=tp, models=ms, prm=prm, n_envs=3, state=st, n_steps=4, obs_every=0, policy=_policy_desc(p), carry=_carry(p),
              episodic=0, obs0=p, obs=p, ret_total=p, ret_episode=p, episode_len=p, actions=None, reward=None, rewards5=None,
              done=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mg_walker_rpolicy_rollout(*[a[k] for k in ok])
    return call


def test_walker_rpolicy_rollout_null_pointers_and_sizes_are_codes_not_crashes():
    lib, tp, ms, prm, st, p, _keep = _fake_call()
    call = _caller(lib, tp, ms, prm, st, p)
    for name in ("topo", "models", "prm", "state", "policy", "carry", "obs0", "obs", "ret_total", "ret_episode", "episode_len"):
        assert call(**{name: None}) == NULL_POINTER, name
        assert b"NULL" in lib.mg_last_error(), name
    for name in ("params_d", "policy_id_d"):
        assert call(policy=_policy_desc(p, **{name: None})) == NULL_POINTER, name
        assert b"NULL" in lib.mg_last_error() and b"mg_walker_policy" in lib.mg_last_error(), name
    for name in ("h", "prev_action", "prev_reward", "prev_done"):
        assert call(carry=_carry(p, **{name: None})) == NULL_POINTER, name
        assert b"NULL" in lib.mg_last_error() and b"mg_walker_rpolicy_carry" in lib.mg_last_error(), name
    assert call(n_steps=0) == BAD_SIZE and b"n_steps" in lib.mg_last_error()
    assert call(n_steps=-5) == BAD_SIZE and b"n_steps" in lib.mg_last_error()
    assert call(obs_every=-1) == BAD_SIZE and b"obs_every" in lib.mg_last_error()
    assert call(n_envs=0) == BAD_SIZE and b"n_envs" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, hidden=257)) == BAD_SIZE and b"hidden" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, hidden=0)) == BAD_SIZE and b"hidden" in lib.mg_last_error()      # (the MLP's linear form)
    assert call(policy=_policy_desc(p, hidden=-1)) == BAD_SIZE and b"hidden" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, n_policies=0)) == BAD_SIZE and b"n_policies" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, obs_dim=21)) == BAD_CONFIG and b"obs_dim" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, n_act=5)) == BAD_CONFIG and b"n_act" in lib.mg_last_error()
    prm.auto_reset = 0
    assert call(episodic=1) == BAD_CONFIG and b"auto_reset" in lib.mg_last_error()
    st.q = None                                                   # an array of the state
    assert call() == NULL_POINTER and b"NULL" in lib.mg_last_error()


def test_walker_rpolicy_rollout_refuses_what_the_rollout_refuses():
    lib, tp, ms, prm, st, p, _keep = _fake_call()
    call = _caller(lib, tp, ms, prm, st, p)
    prm.mapping = 0
    assert call() == UNSUPPORTED and b"mapping" in lib.mg_last_error()
    prm.mapping = 1
    prm.actuation, prm.pd_command = 1, p.value
    assert call() == UNSUPPORTED and b"actuation" in lib.mg_last_error()
    prm.actuation, prm.pd_command = 0, None
    prm.substep_log = p.value
    assert call() == BAD_CONFIG and b"substep_log" in lib.mg_last_error()
    prm.substep_log = None
    tp.body_parent[2] = 3                                         # parents come first (wave_plan)
    assert call() == BAD_CONFIG and b"parent" in lib.mg_last_error()
    tp.body_parent[2] = 0
    prm.n_terrain_boxes = -1
    assert call() == BAD_SIZE and b"terrain" in lib.mg_last_error()


def test_env_rollout_policy_refuses_wrong_arguments_before_any_device_work():
    import metagym_amd.metalocomotion as ml
    assert ml.WalkerRecurrentPolicy is WalkerRecurrentPolicy and ml.WalkerPolicyState is WalkerPolicyState
    env = ml.MetaAntEnv(num_envs=3, device="cuda:0")              # (no task set: nothing is allocated on a device yet)
    mlp = WalkerPolicy.linear(np.zeros((2, A, D), f32), np.zeros((2, A), f32))
    with pytest.raises(TypeError, match="WalkerRecurrentPolicy"):
        env.rollout_policy(mlp, 4, state=WalkerPolicyState(3, 4, A))             # state= and episodic= are the recurrent form's
    with pytest.raises(TypeError, match="WalkerRecurrentPolicy"):
        env.rollout_policy(mlp, 4, episodic=True)
    with pytest.raises(TypeError):
        env.rollout_policy(object(), 4, state=None)
    with pytest.raises(Exception, match="set_robot"):
        env.rollout_policy(_policy(2, 4), 4)
    assert env.global_step == 0
