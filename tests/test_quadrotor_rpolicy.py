"""Quadrotor recurrent closed-loop policies, host side (no GPU): the exact definition (QuadrotorRecurrentPolicy.reference
against a scalar restatement), the packed layout, the carry, the refusals of the constructor and of the ABI, and the
oracle-only preconditions of the GPU tests."""
import ctypes as C
import importlib

import numpy as np
import pytest

import quadrotor_policy_cases as pc
import quadrotor_rpolicy_cases as rc
import quadrotor_tasks_cases as qc

F = np.float32
NEG0 = np.uint32(0x80000000)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _pad4(v):
    return (v + 3) // 4 * 4


@pytest.mark.parametrize("hidden", rc.HIDDEN + (2, 3, 4, 32, 33, 35, 36, 39, 63))      # policy_size_cases.QUADROTOR_RECURRENT_ADDED
@pytest.mark.parametrize("obs_dim", [16, 19])
def test_packing_round_trips_and_matches_the_layout_formula(hidden, obs_dim):
    from metagym_amd import _lib
    from metagym_amd.quadrotor import QuadrotorRecurrentPolicy
    from metagym_amd.quadrotor.policy import recurrent_param_count
    lib = _lib.load()
    pol = rc.make_rpolicy(hidden, obs_dim, n_policies=2)
    DP, HP = _pad4(obs_dim), _pad4(hidden)
    R = DP + HP + 12
    assert DP == (16 if obs_dim == 16 else 20)
    assert pol.param_count == recurrent_param_count(hidden, obs_dim) == 4 + hidden * R
    assert lib.mg_quadrotor_rpolicy_param_count(hidden, obs_dim) == pol.param_count
    packed = pol.pack()
    assert packed.dtype == F and packed.shape == (2, pol.param_count) and pol.param_count % 4 == 0
    back = QuadrotorRecurrentPolicy.unpack(packed, hidden, obs_dim)
    assert back.hidden == hidden and back.obs_dim == obs_dim and back.num_policies == 2
    for name in ("wx", "wa", "wr", "wd", "wh", "b", "wo", "bo"):
        assert np.array_equal(_bits(getattr(pol, name)), _bits(getattr(back, name))), name
    assert np.array_equal(_bits(back.pack()), _bits(packed))
    # the documented places, and zeros in every padding entry
    assert np.array_equal(packed[:, :4], pol.bo)
    j = hidden - 1
    rec = packed[1, 4 + R * j: 4 + R * (j + 1)]
    assert np.array_equal(rec[:obs_dim], pol.wx[1, j]) and not rec[obs_dim:DP].any()
    assert rec[DP] == pol.b[1, j] and rec[DP + 1] == pol.wr[1, j] and rec[DP + 2] == pol.wd[1, j] and rec[DP + 3] == 0
    assert np.array_equal(rec[DP + 4:DP + 8], pol.wa[1, j])
    assert np.array_equal(rec[DP + 8:DP + 8 + hidden], pol.wh[1, j]) and not rec[DP + 8 + hidden:DP + 8 + HP].any()
    assert np.array_equal(rec[DP + 8 + HP:], pol.wo[1, :, j]) and len(rec[DP + 8 + HP:]) == 4


def test_param_count_and_lds_budget_of_the_largest_policy():
    """H = 64, D = 19: 24 592 bytes of staged policy; with h and hn (32 768) and the static tile (4 352) under 64 KiB."""
    from metagym_amd import _lib
    from metagym_amd.quadrotor.policy import recurrent_param_count
    lib = _lib.load()
    assert recurrent_param_count(64, 19) * 4 == 24592
    assert recurrent_param_count(64, 19) * 4 + 2 * 64 * 64 * 4 + 64 * 17 * 4 == 61712 < 64 * 1024
    assert lib.mg_quadrotor_rpolicy_param_count(0, 16) == -1002 and lib.mg_quadrotor_rpolicy_param_count(65, 16) == -1002
    assert lib.mg_quadrotor_rpolicy_param_count(5, 17) == -1003
    for bad in ((0, 16), (65, 16), (5, 17)):
        with pytest.raises(ValueError):
            recurrent_param_count(*bad)


def _zeros(P=1, H=5, D=16):
    f = lambda *s: np.zeros(s, F)
    return dict(wx=f(P, H, D), wa=f(P, H, 4), wr=f(P, H), wd=f(P, H), wh=f(P, H, H), b=f(P, H), wo=f(P, 4, H), bo=f(P, 4))


def _build(kw):
    from metagym_amd.quadrotor import QuadrotorRecurrentPolicy
    return QuadrotorRecurrentPolicy(*[kw[k] for k in ("wx", "wa", "wr", "wd", "wh", "b", "wo", "bo")])


def test_constructor_refusals():
    from metagym_amd.quadrotor import QuadrotorPolicyState
    _build(_zeros())
    for name, shape in (("wa", (1, 5, 3)), ("wr", (1, 4)), ("wd", (2, 5)), ("wh", (1, 5, 4)), ("b", (1, 6)), ("wo", (1, 5, 4)),
                        ("bo", (1, 3)), ("wx", (1, 4, 16))):
        kw = _zeros()
        kw[name] = np.zeros(shape, F)
        with pytest.raises(ValueError):
            _build(kw)
    kw = _zeros()
    kw["wr"] = np.zeros(5, F)                                                  # wrong rank
    with pytest.raises(ValueError):
        _build(kw)
    for name in ("wx", "wa", "wr", "wd", "wh", "b", "wo", "bo"):
        kw = _zeros()
        kw[name] = kw[name].astype(np.float64)
        with pytest.raises(TypeError):
            _build(kw)
        for bad in (np.inf, np.nan):
            kw = _zeros()
            kw[name].flat[0] = bad
            with pytest.raises(ValueError):
                _build(kw)
    with pytest.raises(ValueError):
        _build(_zeros(H=0))
    with pytest.raises(ValueError):
        _build(_zeros(H=65))
    _build(_zeros(H=64, D=19))
    with pytest.raises(ValueError):
        _build(_zeros(D=17))
    with pytest.raises(ValueError):
        _build(_zeros(P=0))
    pol = _build(_zeros(P=2))
    st = QuadrotorPolicyState.zeros(3, 5)
    with pytest.raises(ValueError):
        pol.reference(np.zeros((3, 16), F), np.array([0, 1, 2]), st)           # id out of range
    with pytest.raises(ValueError):
        pol.reference(np.zeros((3, 19), F), np.zeros(3, int), st)
    with pytest.raises(ValueError):
        pol.reference(np.zeros((3, 16), F), np.zeros(3, int), QuadrotorPolicyState.zeros(3, 4))
    with pytest.raises(ValueError):
        pol.reference(np.zeros((3, 16), F), np.zeros(3, int), QuadrotorPolicyState.zeros(2, 5))
    with pytest.raises(ValueError):
        QuadrotorPolicyState.zeros(3, 65)


def edge_policy():
    """One policy, H = 5 (three padding entries behind wh), D = 16, and inputs for one env such that unit 0's
    pre-activation is exactly -0 (b = -0 and every weight a zero signed against its input, so every product is -0), unit 1
    is clamped at +1, unit 2 at -1, units 3 and 4 stay inside. Returns (policy, x, pa, pr, pd, h)."""
    rs = np.random.RandomState(77)
    x = rs.uniform(-3, 3, 16).astype(F)
    pa = np.array([7.5, -2.0, 16.0, 0.25], F)
    pr, pd = F(-3.25), 1
    h = np.array([0.5, -1.0, 1.0, -0.125, 0.75], F)
    kw = _zeros()
    against = lambda v: np.where(np.signbit(v), F(0.0), F(-0.0)).astype(F)    # w * v = -0.0
    kw["wx"][0, 0], kw["wa"][0, 0], kw["wh"][0, 0] = against(x), against(pa), against(h)
    kw["wr"][0, 0], kw["wd"][0, 0], kw["b"][0, 0] = against(pr), F(-0.0), F(-0.0)
    for j, gain in ((1, 1.0), (2, 1.0), (3, 0.01), (4, 0.01)):
        kw["wx"][0, j] = rs.uniform(-0.5, 0.5, 16) * gain
        kw["wa"][0, j] = rs.uniform(-0.2, 0.2, 4) * gain
        kw["wh"][0, j] = rs.uniform(-1, 1, 5) * gain
        kw["wr"][0, j], kw["wd"][0, j] = rs.uniform(-0.3, 0.3) * gain, rs.uniform(-1, 1) * gain
    kw["b"][0, 1], kw["b"][0, 2], kw["b"][0, 3], kw["b"][0, 4] = 40.0, -40.0, 0.3, -0.3
    kw["wo"][0] = rs.uniform(-2, 2, (4, 5))
    kw["bo"][0] = rs.uniform(3, 11, 4)
    return _build(kw), x, pa, pr, pd, h


def _state_of(pa, pr, pd, h):
    from metagym_amd.quadrotor import QuadrotorPolicyState
    return QuadrotorPolicyState(h[None].copy(), pa[None].copy(), np.array([pr], F), np.array([pd], np.uint8))


def test_reference_equals_the_scalar_restatement_at_the_edges():
    pol, x, pa, pr, pd, h = edge_policy()
    want_a, want_h = rc.scalar_step(pol, 0, x, pa, pr, pd, h)
    # the inputs do what they were chosen for
    assert _bits(want_h)[0] == NEG0 and want_h[1] == 1.0 and want_h[2] == -1.0
    assert 0 < abs(want_h[3]) < 1 and 0 < abs(want_h[4]) < 1
    st = _state_of(pa, pr, pd, h)
    before = [v.copy() for v in (st.h, st.prev_action, st.prev_reward, st.prev_done)]
    a, new = pol.reference(x[None], np.zeros(1, int), st)
    assert a.dtype == F and a.shape == (1, 4) and new.h.dtype == F and new.h.shape == (1, 5)
    assert np.array_equal(_bits(a[0]), _bits(want_a)) and np.array_equal(_bits(new.h[0]), _bits(want_h))
    assert np.array_equal(_bits(new.prev_action), _bits(a))
    for u, v in zip(before, (st.h, st.prev_action, st.prev_reward, st.prev_done)):      # the state is read, never written
        assert np.array_equal(u, v)
    # -0 stays -0 only if the padding behind wh is skipped: one more term 0 * h turns it into +0
    assert _bits(F(want_h[0] + F(F(0.0) * h[0])))[()] == 0
    # with pd = 0 the wd term is wd * 0
    a0, new0 = pol.reference(x[None], np.zeros(1, int), _state_of(pa, pr, 0, h))
    w0 = rc.scalar_step(pol, 0, x, pa, pr, 0, h)
    assert np.array_equal(_bits(a0[0]), _bits(w0[0])) and np.array_equal(_bits(new0.h[0]), _bits(w0[1]))
    assert _bits(new0.h[0])[0] == NEG0


def test_a_nan_observation_entry_reaches_every_unit():
    pol, x, pa, pr, pd, h = edge_policy()
    x = x.copy()
    x[7] = np.nan
    want_a, want_h = rc.scalar_step(pol, 0, x, pa, pr, pd, h)
    assert np.isnan(want_h).all() and np.isnan(want_a).all()               # unit 0 included: its zero weight times NaN is NaN
    a, new = pol.reference(x[None], np.zeros(1, int), _state_of(pa, pr, pd, h))
    assert np.isnan(new.h).all() and np.isnan(a).all()                     # neither the clamp nor the sums drop it


@pytest.mark.parametrize("hidden", rc.HIDDEN + (2, 3, 4, 32, 33, 35, 36, 39, 63))      # policy_size_cases.QUADROTOR_RECURRENT_ADDED
@pytest.mark.parametrize("obs_dim", [16, 19])
def test_two_calls_through_the_state_equal_one_scalar_pass(hidden, obs_dim):
    from metagym_amd.quadrotor import QuadrotorPolicyState
    pol = rc.make_rpolicy(hidden, obs_dim)
    n = 7
    rs = np.random.RandomState(9)
    xs = (rs.uniform(-30, 30, (2, n, obs_dim)) * rs.choice([1.0, 0.01], (2, n, obs_dim))).astype(F)
    rew = rs.uniform(-20, 11, (2, n)).astype(F)
    done = rs.randint(0, 2, (2, n))
    ids = rs.randint(0, rc.P, n)
    st = QuadrotorPolicyState.zeros(n, hidden)
    got = []
    for t in range(2):
        a, st = pol.reference(xs[t], ids, st)
        st = st.observed(rew[t], done[t])
        got.append(a)
    for e in range(n):
        pa, pr, pd, h = np.zeros(4, F), F(0), 0, np.zeros(hidden, F)
        for t in range(2):
            a, h = rc.scalar_step(pol, int(ids[e]), xs[t, e], pa, pr, pd, h)
            assert np.array_equal(_bits(a), _bits(got[t][e])), (e, t)
            pa, pr, pd = a, rew[t, e], int(done[t, e])
        assert np.array_equal(_bits(h), _bits(st.h[e])) and np.array_equal(_bits(pa), _bits(st.prev_action[e]))
        assert st.prev_reward[e] == pr and st.prev_done[e] == pd
    # `observed` with a clear mask is what episodic does: the four fields of those envs are zero, the others kept
    c = st.observed(rew[1], done[1], clear=done[1] != 0)
    m = done[1] != 0
    assert m.any() and (~m).any()
    assert not c.h[m].any() and not c.prev_action[m].any() and not c.prev_reward[m].any() and not c.prev_done[m].any()
    assert np.array_equal(_bits(c.h[~m]), _bits(st.h[~m])) and np.array_equal(c.prev_reward[~m], st.prev_reward[~m])


def test_carry_construction_clone_and_numpy():
    from metagym_amd.quadrotor import QuadrotorPolicyState
    st = QuadrotorPolicyState.zeros(6, 5)
    assert st.num_envs == 6 and st.hidden == 5 and st.device is None
    assert (st.h.shape, st.prev_action.shape, st.prev_reward.shape, st.prev_done.shape) == ((6, 5), (6, 4), (6,), (6,))
    assert (st.h.dtype, st.prev_action.dtype, st.prev_reward.dtype, st.prev_done.dtype) == (F, F, F, np.uint8)
    assert not any(v.any() for v in (st.h, st.prev_action, st.prev_reward, st.prev_done))
    c = st.clone()
    c.h[0, 0] = 1
    c.prev_done[1] = 1
    assert not st.h.any() and not st.prev_done.any()
    h = c.numpy()
    assert h.h is not c.h and np.array_equal(h.h, c.h) and np.array_equal(h.prev_done, c.prev_done)


def test_the_policy_module_needs_no_gpu():
    import torch
    mod = importlib.import_module("metagym_amd.quadrotor.policy")
    pol = rc.make_rpolicy(5)
    pol.reference(np.zeros((2, 16), F), np.zeros(2, int), mod.QuadrotorPolicyState.zeros(2, 5))
    assert not torch.cuda.is_initialized()
    from metagym_amd.quadrotor import QuadrotorPolicyState, QuadrotorRecurrentPolicy
    assert mod.QuadrotorRecurrentPolicy is QuadrotorRecurrentPolicy and mod.QuadrotorPolicyState is QuadrotorPolicyState


@pytest.mark.parametrize("hidden", rc.HIDDEN)
def test_units_saturate_and_do_not_in_the_closed_loop(hidden):
    """The precondition of the GPU tests, from the oracle and the definition alone: over the T steps of the mixed-table
    closed loop some memories sit at +1, some at -1 and some strictly inside, the voltages leave [0.1, 15] on both sides,
    and with memory the actions differ from the memoryless form's from the second step on."""
    from oracle import quadrotor as qo
    ids_t = qc.mixed_ids()
    mk = lambda: qc.OracleGroups(qc.mixed_configs(), ids_t, qc.random_batch(qc.N, qc.STATE_SEED), task=qo.TASK_HOVERING)
    pol = rc.make_rpolicy(hidden)
    acts, mems, end = rc.closed_loop_oracle(mk(), pol, pc.layout_ids(), rc.T)
    assert acts.shape == (rc.T, rc.N, 4) and acts.dtype == F and mems.shape == (rc.T, rc.N, hidden)
    assert (mems == 1).any() and (mems == -1).any() and (np.abs(mems) < 1).any()
    assert (acts > 15.0).any() and (acts < 0.1).any()
    flat, _, _ = rc.closed_loop_oracle(mk(), rc.without_memory(pol), pc.layout_ids(), rc.T)
    assert np.array_equal(_bits(flat[0]), _bits(acts[0]))                  # a fresh carry is all zero: step 1 is the same
    assert all((_bits(flat[t]) != _bits(acts[t])).any() for t in range(1, rc.T))


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
    carry = _lib.QuadrotorRPolicyCarry(base, base, base, base)
    call = lambda **kw: lib.mg_quadrotor_rpolicy_rollout(*[kw.get(k, v) for k, v in (
        ("cfg", cfg), ("tasks", None), ("n", 4), ("steps", 2), ("state", st), ("ar", None), ("policy", pol), ("carry", carry),
        ("episodic", 0), ("ret_total", p), ("ret_episode", p), ("episode_len", p), ("records", None), ("last", last),
        ("stream", None))])
    for name in ("cfg", "state", "policy", "carry", "ret_total", "ret_episode", "episode_len", "last"):
        assert call(**{name: None}) == -1001, name
        assert b"NULL" in lib.mg_last_error()
    assert call(last=_lib.QuadrotorPolicyLast(None, None, None, base, None)) == -1001
    assert call(last=_lib.QuadrotorPolicyLast(base, None, None, None, None)) == -1001
    assert call(policy=_lib.QuadrotorPolicyDesc(None, base, 3, 5, 16)) == -1001
    assert call(policy=_lib.QuadrotorPolicyDesc(base, None, 3, 5, 16)) == -1001
    for i in range(4):
        ptrs = [base] * 4
        ptrs[i] = None
        assert call(carry=_lib.QuadrotorRPolicyCarry(*ptrs)) == -1001 and b"carry" in lib.mg_last_error()
    assert call(state=_lib.QuadrotorState()) == -1001
    assert call(policy=_lib.QuadrotorPolicyDesc(base, base, 3, 65, 16)) == -1002 and b"hidden" in lib.mg_last_error()
    assert call(policy=_lib.QuadrotorPolicyDesc(base, base, 3, 0, 16)) == -1002
    assert call(policy=_lib.QuadrotorPolicyDesc(base, base, 0, 5, 16)) == -1002 and b"n_policies" in lib.mg_last_error()
    assert call(n=0) == -1002 and call(steps=0) == -1002
    assert call(policy=_lib.QuadrotorPolicyDesc(base, base, 3, 5, 19)) == -1003 and b"obs_dim" in lib.mg_last_error()
    assert call(policy=_lib.QuadrotorPolicyDesc(base + 4, base, 3, 5, 16)) == -1003 and b"aligned" in lib.mg_last_error()
    assert call(carry=_lib.QuadrotorRPolicyCarry(base, base + 4, base, base)) == -1003 and b"aligned" in lib.mg_last_error()
    assert call(episodic=1) == -1003 and b"episodic" in lib.mg_last_error()  # no fused reset to clear at
    cfg.task = 1
    assert call() == -1003                                                     # velocity_control reads 19 entries
    cfg.task = 2
    st.episode = None
    assert call(ar=_lib.QuadrotorAutoReset()) == -1001 and b"episode" in lib.mg_last_error()
    tk = _lib.QuadrotorTasks()
    assert call(tasks=tk) == -1002                                             # n_tasks = 0
    tk.n_tasks = 2
    assert call(tasks=tk) == -1001
    cfg.precision = 1.0
    assert call() == -1003                                                     # what every entry point refuses about cfg
