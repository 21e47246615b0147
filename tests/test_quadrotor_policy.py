"""Quadrotor closed-loop policies, host side (no GPU): the exact policy definition (QuadrotorPolicy.reference), the packed
layout, the ABI's host-side refusals, and the oracle-only precondition of the GPU test's mixed-table case."""
import ctypes as C

import numpy as np
import pytest

import quadrotor_policy_cases as pc
import quadrotor_tasks_cases as qc

F = np.float32


def _loops(policy, x, pid):
    """The definition restated with explicit Python loops over np.float32 scalars: no float64, no vector operation."""
    D, H = policy.obs_dim, policy.hidden
    a = [F(0)] * 4
    if H == 0:
        for k in range(4):
            a[k] = F(policy.b2[pid, k])
            for i in range(D):
                a[k] = F(a[k] + F(F(policy.w2[pid, k, i]) * F(x[i])))
        return np.array(a, F)
    h = []
    for j in range(H):
        z = F(policy.b1[pid, j])
        for i in range(D):
            z = F(z + F(F(policy.w1[pid, j, i]) * F(x[i])))
        h.append(z if z > 0 else F(0))
    for k in range(4):
        a[k] = F(policy.b2[pid, k])
        for j in range(H):
            a[k] = F(a[k] + F(F(policy.w2[pid, k, j]) * h[j]))
    return np.array(a, F)


@pytest.mark.parametrize("hidden", [0, 1, 5, 33, 256])
@pytest.mark.parametrize("obs_dim", [16, 19])
def test_reference_equals_the_scalar_restatement(hidden, obs_dim):
    pol = pc.make_policy(hidden, obs_dim)
    n = 23
    rs = np.random.RandomState(5)
    x = (rs.uniform(-30, 30, (n, obs_dim)) * rs.choice([1.0, 0.01], (n, obs_dim))).astype(F)
    ids = rs.randint(0, pc.P, n)
    got = pol.reference(x, ids)
    assert got.dtype == F and got.shape == (n, 4)
    want = np.stack([_loops(pol, x[e], int(ids[e])) for e in range(n)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_reference_is_the_unfused_value():
    """b * c = 1 + 2^-11 + 2^-24 exactly, which float32 rounds (a tie, to even) to 1 + 2^-11. With a = -(1 + 2^-11) the
    defined value a + fl(b * c) is 0.0; a fused multiply-add would give 2^-24."""
    from metagym_amd.quadrotor import QuadrotorPolicy
    a, b = F(-(1.0 + 2.0 ** -11)), F(1.0 + 2.0 ** -12)
    assert float(b) * float(b) == 1.0 + 2.0 ** -11 + 2.0 ** -24 and F(b * b) == F(1.0 + 2.0 ** -11)
    assert float(a) + float(b) * float(b) == 2.0 ** -24                      # what an fma would return, exactly
    x = np.zeros((1, 16), F)
    x[0, 0] = b
    w = np.zeros((1, 4, 16), F)
    w[0, :, 0] = b
    lin = QuadrotorPolicy.linear(w, np.full((1, 4), a, F))
    out = lin.reference(x, np.zeros(1, int))
    assert np.array_equal(out.view(np.uint32), np.zeros((1, 4), np.uint32))
    # the same through a hidden unit: z = a + b * b = 0 -> h = 0; and through the output layer: b2 + w2 * h with h = b
    w1 = np.zeros((1, 2, 16), F)
    w1[0, 0, 0] = b                                                          # unit 0: z = a + b * b
    w1[0, 1, 0] = F(1.0)                                                     # unit 1: z = 0 + 1 * b = b
    w2 = np.zeros((1, 4, 2), F)
    w2[0, :, 0] = F(1.0)
    w2[0, :, 1] = b
    mlp = QuadrotorPolicy(w1, np.array([[a, 0.0]], F), w2, np.full((1, 4), a, F))
    out = mlp.reference(x, np.zeros(1, int))
    assert np.array_equal(out.view(np.uint32), np.zeros((1, 4), np.uint32))


def test_relu_of_negative_zero_and_nan_is_plus_zero():
    """Unit 0 sees a negative pre-activation, unit 1 a negative zero, unit 2 a NaN: each h is +0.0, so the outputs are
    b2 + w2 * (+0.0). With b2 = -0.0 and w2 = 1 that is +0.0; an h of -0.0 would leave -0.0 and a NaN would spread."""
    from metagym_amd.quadrotor import QuadrotorPolicy
    x = np.zeros((3, 16), F)
    x[0, 0], x[1, 0], x[2, 0] = -2.0, -1.0, np.nan
    w1 = np.zeros((3, 1, 16), F)
    w1[0, 0, 0], w1[1, 0, 0], w1[2, 0, 0] = 1.0, 0.0, 1.0                   # z = -2; z = -0.0 + 0 * -1 = -0.0; z = NaN
    w1[1, 0, 1:] = -0.0                                                      # ... and stays -0.0: every product is -0.0
    b1 = np.array([[0.0], [-0.0], [0.0]], F)
    pol = QuadrotorPolicy(w1, b1, np.ones((3, 4, 1), F), np.full((3, 4), -0.0, F))
    z1 = F(-0.0)
    for i in range(16):
        z1 = F(z1 + F(w1[1, 0, i] * x[1, i]))
    assert z1 == 0 and np.signbit(z1)
    out = pol.reference(x, np.arange(3))
    assert np.array_equal(out.view(np.uint32), np.zeros((3, 4), np.uint32))


@pytest.mark.parametrize("hidden", [0, 1, 256, 33])
@pytest.mark.parametrize("obs_dim", [16, 19])
def test_packing_round_trips_and_matches_the_library_count(hidden, obs_dim):
    from metagym_amd import _lib
    from metagym_amd.quadrotor import QuadrotorPolicy
    lib = _lib.load()
    pol = pc.make_policy(hidden, obs_dim, n_policies=2)
    packed = pol.pack()
    assert packed.dtype == F and packed.shape == (2, pol.param_count)
    assert lib.mg_quadrotor_policy_param_count(hidden, obs_dim) == pol.param_count == packed.shape[1]
    assert pol.param_count % 4 == 0                                          # 16-byte rows: policy p starts aligned
    back = QuadrotorPolicy.unpack(packed, hidden, obs_dim)
    assert back.hidden == hidden and back.obs_dim == obs_dim and back.num_policies == 2
    for name in ("w1", "b1", "w2", "b2"):
        u, v = getattr(pol, name), getattr(back, name)
        assert (u is None and v is None) or np.array_equal(u.view(np.uint32), v.view(np.uint32)), name
    assert np.array_equal(back.pack().view(np.uint32), packed.view(np.uint32))
    # the documented places
    if hidden:
        j = hidden - 1
        rec = packed[1, 4 + 24 * j: 4 + 24 * (j + 1)]
        assert np.array_equal(rec[:obs_dim], pol.w1[1, j]) and rec[obs_dim] == pol.b1[1, j]
        assert np.array_equal(rec[20:], pol.w2[1, :, j]) and not rec[obs_dim + 1:20].any()
    else:
        assert packed[1, 4 + 4 * 7 + 2] == pol.w2[1, 2, 7]
    assert np.array_equal(packed[:, :4], pol.b2)


def test_policy_constructor_refusals():
    from metagym_amd.quadrotor import QuadrotorPolicy
    f = lambda *s: np.zeros(s, F)
    with pytest.raises(ValueError):
        QuadrotorPolicy(f(1, 257, 16), f(1, 257), f(1, 4, 257), f(1, 4))      # H too large
    with pytest.raises(ValueError):
        QuadrotorPolicy(f(1, 5, 17), f(1, 5), f(1, 4, 5), f(1, 4))            # no such observation
    with pytest.raises(ValueError):
        QuadrotorPolicy(f(1, 5, 16), f(1, 4), f(1, 4, 5), f(1, 4))            # b1 does not fit
    with pytest.raises(ValueError):
        QuadrotorPolicy(f(0, 5, 16), f(0, 5), f(0, 4, 5), f(0, 4))            # P = 0
    with pytest.raises(TypeError):
        QuadrotorPolicy.linear(np.zeros((1, 4, 16)), f(1, 4))                  # float64
    bad = f(1, 4, 16)
    bad[0, 0, 0] = np.inf
    with pytest.raises(ValueError):
        QuadrotorPolicy.linear(bad, f(1, 4))
    with pytest.raises(ValueError):
        QuadrotorPolicy.linear(f(1, 3, 16), f(1, 4))
    pol = QuadrotorPolicy.linear(f(2, 4, 16), f(2, 4))
    with pytest.raises(ValueError):
        pol.reference(f(3, 16), np.array([0, 1, 2]))                           # id out of range
    with pytest.raises(ValueError):
        pol.reference(f(3, 19), np.zeros(3, int))


def test_abi_refuses_on_the_host_before_any_device_call():
    from metagym_amd import _lib
    lib = _lib.load()
    cfg = _lib.QuadrotorConfig()
    lib.mg_quadrotor_default_config(cfg)
    cfg.task = 2
    fake = C.create_string_buffer(256)
    base = (C.addressof(fake) + 15) & ~15
    p = C.c_void_p(base)
    st = _lib.QuadrotorState()
    for name, _ in _lib.QuadrotorState._fields_:
        setattr(st, name, base)
    pol = _lib.QuadrotorPolicyDesc(base, base, 3, 5, 16)
    last = _lib.QuadrotorPolicyLast(base, None, None, base, None)
    call = lambda **kw: lib.mg_quadrotor_policy_rollout(*[kw.get(k, v) for k, v in (
        ("cfg", cfg), ("tasks", None), ("n", 4), ("steps", 2), ("state", st), ("ar", None), ("policy", pol), ("ret_total", p),
        ("ret_episode", p), ("episode_len", p), ("records", None), ("last", last), ("stream", None))])
    # null required pointers
    for name in ("cfg", "state", "policy", "ret_total", "ret_episode", "episode_len", "last"):
        assert call(**{name: None}) == -1001, name
        assert b"NULL" in lib.mg_last_error()
    assert call(last=_lib.QuadrotorPolicyLast(None, None, None, base, None)) == -1001
    assert call(last=_lib.QuadrotorPolicyLast(base, None, None, None, None)) == -1001
    assert call(policy=_lib.QuadrotorPolicyDesc(None, base, 3, 5, 16)) == -1001
    assert call(policy=_lib.QuadrotorPolicyDesc(base, None, 3, 5, 16)) == -1001
    empty = _lib.QuadrotorState()
    assert call(state=empty) == -1001
    # sizes
    assert call(policy=_lib.QuadrotorPolicyDesc(base, base, 3, 257, 16)) == -1002 and b"hidden" in lib.mg_last_error()
    assert call(policy=_lib.QuadrotorPolicyDesc(base, base, 3, -1, 16)) == -1002
    assert call(policy=_lib.QuadrotorPolicyDesc(base, base, 0, 5, 16)) == -1002 and b"n_policies" in lib.mg_last_error()
    assert call(n=0) == -1002 and call(steps=0) == -1002
    # the observation width is the task's
    assert call(policy=_lib.QuadrotorPolicyDesc(base, base, 3, 5, 19)) == -1003 and b"obs_dim" in lib.mg_last_error()
    assert call(policy=_lib.QuadrotorPolicyDesc(base + 4, base, 3, 5, 16)) == -1003 and b"aligned" in lib.mg_last_error()
    cfg.task = 1
    assert call() == -1003                                                     # velocity_control reads 19 entries
    cfg.task = 2
    # a fused reset needs the episode counters; a table needs its rows
    st.episode = None
    assert call(ar=_lib.QuadrotorAutoReset()) == -1001 and b"episode" in lib.mg_last_error()
    tk = _lib.QuadrotorTasks()
    assert call(tasks=tk) == -1002                                             # n_tasks = 0
    tk.n_tasks = 2
    assert call(tasks=tk) == -1001
    cfg.precision = 1.0
    assert call() == -1003                                                     # what every entry point refuses about cfg
    # the count refuses the same sizes
    assert lib.mg_quadrotor_policy_param_count(257, 16) == -1002
    assert lib.mg_quadrotor_policy_param_count(5, 17) == -1003
    assert lib.mg_quadrotor_policy_param_count(0, 19) == 4 + 4 * 19 and lib.mg_quadrotor_policy_param_count(256, 16) == 4 + 24 * 256


def test_tight_row_fails_some_envs_and_not_others_in_the_closed_loop():
    """The precondition of the GPU test's mixed-table case, from the oracle and the policy definition alone: with the
    test's policy in the loop, the tight-threshold row holds envs that fail and envs that do not inside the T steps."""
    from oracle import quadrotor as qo
    ids = qc.mixed_ids()
    og = qc.OracleGroups(qc.mixed_configs(), ids, qc.random_batch(qc.N, qc.STATE_SEED), task=qo.TASK_HOVERING)
    pol = pc.make_policy(5)
    acts, outs, codes = pc.closed_loop_oracle(og, pol, pc.layout_ids(), pc.T)
    assert acts.shape == (pc.T, pc.N, 4) and acts.dtype == F
    tight = codes[ids == 4]
    assert (tight != 0).any() and (tight == 0).any()
    assert (codes[ids != 4] == 0).all()
    # the policy's voltages leave the range on both sides, so the step's clamp is part of the loop
    assert (acts > 15.0).any() and (acts < 0.1).any()
