"""CPU-side checks of the walker policies (metagym_amd/metalocomotion/policy.py) and of mg_walker_policy_rollout's argument
errors (include/metagym_hip.h): the packed layout round-trips, the float32 definition keeps its association, and every wrong
argument is a code with a message, decided on the host before any launch (so no GPU is needed). The kernel itself:
tests/test_walker_policy_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from metagym_amd.metalocomotion.policy import MAX_HIDDEN, WalkerPolicy, param_count

NULL_POINTER, BAD_SIZE, BAD_CONFIG, UNSUPPORTED = -1001, -1002, -1003, -1004
D, A = 28, 8                                  # the ant's observation and action widths


def _policy(P, H, d=D, a=A, seed=0):
    g = np.random.RandomState(seed)
    u = lambda *s: g.uniform(-1.0, 1.0, size=s).astype(np.float32)
    if H == 0:
        return WalkerPolicy.linear(u(P, a, d), u(P, a))
    return WalkerPolicy(u(P, H, d), u(P, H), u(P, a, H), u(P, a))


@pytest.mark.parametrize("H", [0, 1, 70, 256, 64, 129])
def test_pack_unpack_round_trip_and_layout(H):
    pol = _policy(3, H)
    packed = pol.pack()
    assert packed.dtype == np.float32 and packed.shape == (3, pol.param_count) and len(pol) == 3
    assert pol.param_count == param_count(H, D, A) == (H + D * H + A + H * A if H else A + D * A)
    back = WalkerPolicy.unpack(packed, H, D, A)
    assert (back.hidden, back.obs_dim, back.n_act, back.num_policies) == (H, D, A, 3)
    assert np.array_equal(back.w2, pol.w2) and np.array_equal(back.b2, pol.b2)
    if H:
        assert np.array_equal(back.w1, pol.w1) and np.array_equal(back.b1, pol.b1)
        # the documented places: b1[H], w1 input-major [D][H], b2[A], w2 hidden-major [H][A]
        p, j, i, k = 2, H - 1, 5, 3
        assert packed[p, j] == pol.b1[p, j]
        assert packed[p, H + i * H + j] == pol.w1[p, j, i]
        assert packed[p, H + D * H + k] == pol.b2[p, k]
        assert packed[p, H + D * H + A + j * A + k] == pol.w2[p, k, j]
    else:
        assert back.w1 is None and back.b1 is None
        p, i, k = 1, 27, 7
        assert packed[p, k] == pol.b2[p, k] and packed[p, A + i * A + k] == pol.w2[p, k, i]
    with pytest.raises(ValueError):
        WalkerPolicy.unpack(packed[:, :-1], H, D, A)


def test_param_count_is_the_librarys():
    from metagym_amd import _lib
    lib = _lib.load()
    for H in (0, 1, 64, 70, 256):
        for d, a in ((28, 8), (44, 17), (33, 12)):
            assert lib.mg_walker_policy_param_count(H, d, a) == param_count(H, d, a), (H, d, a)
    assert lib.mg_walker_policy_param_count(257, 28, 8) == BAD_SIZE and b"hidden" in lib.mg_last_error()
    assert lib.mg_walker_policy_param_count(-1, 28, 8) == BAD_SIZE
    assert lib.mg_walker_policy_param_count(4, 28, 0) == BAD_SIZE and b"n_act" in lib.mg_last_error()
    assert lib.mg_walker_policy_param_count(4, 0, 8) == BAD_SIZE and b"obs_dim" in lib.mg_last_error()


def test_constructor_refuses_what_is_not_a_policy():
    f = lambda *s: np.zeros(s, np.float32)
    WalkerPolicy(f(2, 4, D), f(2, 4), f(2, A, 4), f(2, A))                       # the well-formed one
    with pytest.raises(TypeError):
        WalkerPolicy(np.zeros((2, 4, D), np.float64), f(2, 4), f(2, A, 4), f(2, A))
    with pytest.raises(TypeError):
        WalkerPolicy.linear(np.zeros((2, A, D), np.float64), f(2, A))
    with pytest.raises(ValueError):
        WalkerPolicy(f(4, D), f(2, 4), f(2, A, 4), f(2, A))                      # ranks
    with pytest.raises(ValueError):
        WalkerPolicy(f(2, 4, D), f(2, 4, 1), f(2, A, 4), f(2, A))
    with pytest.raises(ValueError):
        WalkerPolicy.linear(f(A, D), f(A))
    with pytest.raises(ValueError):
        WalkerPolicy(f(2, 4, D), f(2, 5), f(2, A, 4), f(2, A))                   # shapes that do not belong together
    with pytest.raises(ValueError):
        WalkerPolicy(f(2, 4, D), f(2, 4), f(2, A, 5), f(2, A))
    with pytest.raises(ValueError):
        WalkerPolicy(f(2, 4, D), f(2, 4), f(2, A, 4), f(3, A))
    with pytest.raises(ValueError):
        WalkerPolicy.linear(f(2, A, D), f(2, A + 1))
    for bad in (np.nan, np.inf, -np.inf):
        w = f(2, 4, D)
        w[1, 2, 3] = bad
        with pytest.raises(ValueError):
            WalkerPolicy(w, f(2, 4), f(2, A, 4), f(2, A))
        b = f(2, A)
        b[0, 0] = bad
        with pytest.raises(ValueError):
            WalkerPolicy.linear(f(2, A, D), b)
    with pytest.raises(ValueError):
        WalkerPolicy(f(2, 0, D), f(2, 0), f(2, A, 0), f(2, A))                   # H = 0 goes through linear()
    with pytest.raises(ValueError):
        WalkerPolicy(f(1, MAX_HIDDEN + 1, D), f(1, MAX_HIDDEN + 1), f(1, A, MAX_HIDDEN + 1), f(1, A))
    WalkerPolicy(f(1, MAX_HIDDEN, D), f(1, MAX_HIDDEN), f(1, A, MAX_HIDDEN), f(1, A))


def _scalar_reference(pol, x, ids):
    """The definition, one float32 operation at a time."""
    f32 = np.float32
    out = np.zeros((x.shape[0], pol.n_act), f32)
    for n in range(x.shape[0]):
        p = int(ids[n])
        if pol.hidden == 0:
            src = x[n]
        else:
            src = np.zeros(pol.hidden, f32)
            for j in range(pol.hidden):
                z = f32(pol.b1[p, j])
                for i in range(pol.obs_dim):
                    z = f32(z + f32(pol.w1[p, j, i] * x[n, i]))
                src[j] = z if z > 0 else f32(0.0)
        for k in range(pol.n_act):
            a = f32(pol.b2[p, k])
            for j in range(src.shape[0]):
                a = f32(a + f32(pol.w2[p, k, j] * src[j]))
            out[n, k] = a
    return out


def test_reference_keeps_the_stated_association():
    # (1e8 + 1) - 1e8 + 1 in float32, left to right: 1e8 + 1 = 1e8, - 1e8 = 0, + 1 = 1. A pairwise, reversed or float64 sum
    # gives 2 or 0.
    f32 = np.float32
    x = np.array([[1e8, 1.0, -1e8, 1.0]], f32)
    ids = np.array([0])
    lin = WalkerPolicy.linear(np.ones((1, 2, 4), f32), np.zeros((1, 2), f32))
    assert np.array_equal(lin.reference(x, ids), np.array([[1.0, 1.0]], f32))
    assert float(np.ones(4) @ x[0].astype(np.float64)) == 2.0                    # (what the other orders give)
    # the same cancellation inside a hidden sum (unit 1) and again inside an output sum (output 0, over h = (1e8, 1, 1e8, 1))
    w1 = np.zeros((1, 4, 4), f32)
    w1[0, 0] = (1.0, 0.0, 0.0, 0.0)          # h0 = 1e8
    w1[0, 1] = (1.0, 1.0, 1.0, 1.0)          # h1 = 1 by the order above (2 or 0 by any other)
    w1[0, 2] = (1.0, 0.0, 0.0, 0.0)          # h2 = 1e8
    w1[0, 3] = (0.0, 0.0, 0.0, 1.0)          # h3 = 1
    w2 = np.array([[[1.0, 1.0, -1.0, 1.0],   # a0 = ((1e8 + 1) - 1e8) + 1 = 1
                    [0.0, 1.0, 0.0, 0.0]]], f32)      # a1 = h1
    mlp = WalkerPolicy(w1, np.zeros((1, 4), f32), w2, np.zeros((1, 2), f32))
    got = mlp.reference(x, ids)
    assert got.dtype == f32 and np.array_equal(got, _scalar_reference(mlp, x, ids))
    assert np.array_equal(got, np.array([[1.0, 1.0]], f32))
    # random policies, every form: the vectorised reference is the scalar loop, bit for bit
    g = np.random.RandomState(3)
    for H in (0, 1, 70):
        pol = _policy(3, H, seed=H + 1)
        xs = (g.uniform(-5, 5, size=(6, D)) * g.choice([1.0, 1e4, 1e-4], size=(6, D))).astype(f32)
        pid = np.array([0, 2, 1, 1, 0, 2])
        assert np.array_equal(pol.reference(xs, pid), _scalar_reference(pol, xs, pid)), H
    with pytest.raises(ValueError):
        lin.reference(x.astype(np.float64), ids)
    with pytest.raises(ValueError):
        lin.reference(x, np.array([1]))                                          # only policy 0 exists


def test_relu_of_minus_zero_and_of_a_negative_is_plus_zero():
    f32 = np.float32
    # unit 0: z = -0.0 (b1 = -0.0 plus the product -0.0 * 1); unit 1: z = -3. Both must give h = +0.0. Then every term of
    # a = b2 + sum w2 * h is -0.0 (b2 = -0.0, w2 = -1) and a = -0.0; an h of -0.0 would add a +0.0 and flip a to +0.0.
    w1 = np.array([[[-0.0], [-3.0]]], f32)
    b1 = np.array([[-0.0, 0.0]], f32)
    x = np.array([[1.0]], f32)               # z0 = -0.0 + (-0.0 * 1) = -0.0, z1 = 0 + (-3 * 1) = -3
    w2 = np.array([[[-1.0, -1.0], [-1.0, -1.0]]], f32)  # every product is -0.0 when h is +0.0
    b2 = np.array([[-0.0, -0.0]], f32)
    pol = WalkerPolicy(w1, b1, w2, b2)
    z0 = f32(b1[0, 0] + w1[0, 0, 0] * x[0, 0])
    assert z0 == 0 and np.signbit(z0)        # the test's premise: the pre-activation really is -0.0
    a = pol.reference(x, np.array([0]))
    assert np.array_equal(a, np.zeros((1, 2), f32)) and np.signbit(a).all()
    assert np.array_equal(a, _scalar_reference(pol, x, np.array([0])))
    assert np.array_equal(np.signbit(a), np.signbit(_scalar_reference(pol, x, np.array([0]))))


# ---- mg_walker_policy_rollout refusals (the helper is that of tests/test_walker_rollout.py) ----------------------------
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


def _caller(lib, tp, ms, prm, st, p):
    ok = dict(topo=tp, models=ms, prm=prm, n_envs=3, state=st, n_steps=4, obs_every=0, policy=_policy_desc(p), obs0=p, obs=p,
              ret_total=p, ret_episode=p, episode_len=p, actions=None, reward=None, rewards5=None, done=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mg_walker_policy_rollout(*[a[k] for k in ok])
    return call


def test_walker_policy_rollout_null_pointers_and_sizes_are_codes_not_crashes():
    lib, tp, ms, prm, st, p, _keep = _fake_call()
    call = _caller(lib, tp, ms, prm, st, p)
    for name in ("topo", "models", "prm", "state", "policy", "obs0", "obs", "ret_total", "ret_episode", "episode_len"):
        assert call(**{name: None}) == NULL_POINTER, name
        assert b"NULL" in lib.mg_last_error(), name
    for name in ("params_d", "policy_id_d"):
        assert call(policy=_policy_desc(p, **{name: None})) == NULL_POINTER, name
        assert b"NULL" in lib.mg_last_error() and b"mg_walker_policy" in lib.mg_last_error(), name
    assert call(n_steps=0) == BAD_SIZE and b"n_steps" in lib.mg_last_error()
    assert call(n_steps=-5) == BAD_SIZE and b"n_steps" in lib.mg_last_error()
    assert call(obs_every=-1) == BAD_SIZE and b"obs_every" in lib.mg_last_error()
    assert call(n_envs=0) == BAD_SIZE and b"n_envs" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, hidden=257)) == BAD_SIZE and b"hidden" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, hidden=-1)) == BAD_SIZE and b"hidden" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, n_policies=0)) == BAD_SIZE and b"n_policies" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, obs_dim=21)) == BAD_CONFIG and b"obs_dim" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, obs_dim=28)) == BAD_CONFIG and b"obs_dim" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, n_act=5)) == BAD_CONFIG and b"n_act" in lib.mg_last_error()
    assert call(policy=_policy_desc(p, n_act=8)) == BAD_CONFIG and b"n_act" in lib.mg_last_error()
    st.q = None                                                   # an array of the state
    assert call() == NULL_POINTER and b"NULL" in lib.mg_last_error()


def test_walker_policy_rollout_refuses_what_the_rollout_refuses():
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
    assert ml.WalkerPolicy is WalkerPolicy
    env = ml.MetaAntEnv(num_envs=3, device="cuda:0")              # (no task set: nothing is allocated on a device yet)
    with pytest.raises(TypeError):
        env.rollout_policy(object(), 4)
    with pytest.raises(Exception, match="set_robot"):
        env.rollout_policy(_policy(2, 0), 4)
    assert env.global_step == 0
