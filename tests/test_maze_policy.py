"""MetaMaze recurrent policies, host side (no GPU): the exact definition (MazePolicy.reference), the packed layout, the
constructor's refusals, the clamp, the argmax, the exploration threshold, and the ABI's declarations and host-side refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from metagym_amd.metamaze.policy import (MAX_HIDDEN, MazePolicy, MazePolicyState, eps_threshold, input_dim, param_count,
                                         philox4x32_10)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_policy(P, H, vg, seed, epsilon=None):
    rs = np.random.RandomState(seed)
    D = input_dim(vg)
    return MazePolicy((rs.randn(P, H, D) / np.sqrt(D)).astype(F), (rs.randn(P, H, H) / np.sqrt(H)).astype(F),
                      (0.1 * rs.randn(P, H)).astype(F), (rs.randn(P, 4, H) / np.sqrt(H)).astype(F), (0.1 * rs.randn(P, 4)).astype(F),
                      epsilon)


def _state(h, prev_action, prev_reward, prev_done, step=0):
    return MazePolicyState(np.asarray(h, F), np.asarray(prev_action, np.int32), np.asarray(prev_reward, F),
                           np.asarray(prev_done, np.uint8), step)


def _loops(pol, pid, win, h, pa, pr, pd):
    """The definition restated with explicit Python loops over np.float32 scalars: no float64, no vector operation."""
    D, H = pol.input_dim, pol.hidden
    ww = D - 6
    x = [F(v) for v in win.ravel()] + [F(1.0) if pa == k else F(0.0) for k in range(4)] + [F(pr), F(1.0) if pd else F(0.0)]
    hn = []
    with np.errstate(all="ignore"):
        for j in range(H):
            z = F(pol.b[pid, j])
            for i in range(D):
                z = F(z + F(F(pol.wx[pid, j, i]) * x[i]))
            for i in range(H):
                z = F(z + F(F(pol.wh[pid, j, i]) * F(h[i])))
            hn.append(F(1.0) if z > 1 else (F(-1.0) if z < -1 else z))
        logits = []
        for k in range(4):
            v = F(pol.bo[pid, k])
            for j in range(H):
                v = F(v + F(F(pol.wo[pid, k, j]) * hn[j]))
            logits.append(v)
    g = 0
    for k in range(1, 4):
        if logits[k] > logits[g]:
            g = k
    assert len(x) == D and ww == win.size
    return g, np.array(hn, F)


@pytest.mark.parametrize("hidden", [1, 5, 64, 2, 3, 4, 6, 7, 63])       # the last six: policy_size_cases.MAZE_ADDED
@pytest.mark.parametrize("view_grid", [1, 2, 3])
def test_pack_round_trips_and_matches_the_library_count(hidden, view_grid):
    from metagym_amd import _lib
    lib = _lib.load()
    pol = _random_policy(2, hidden, view_grid, 3, epsilon=np.array([0.0, 0.5]))
    D = input_dim(view_grid)
    packed = pol.pack()
    assert packed.dtype == F and packed.shape == (2, pol.param_count)
    assert lib.mg_maze2d_policy_param_count(hidden, view_grid) == pol.param_count == param_count(hidden, view_grid)
    assert pol.param_count % 4 == 0 and (D + 1) % 4 == 0                     # 16-byte reads: every piece starts aligned
    back = MazePolicy.unpack(packed, hidden, view_grid, pol.epsilon)
    assert (back.hidden, back.view_grid, back.input_dim, back.num_policies) == (hidden, view_grid, D, 2)
    for name in ("wx", "wh", "b", "wo", "bo"):
        assert np.array_equal(getattr(pol, name).view(np.uint32), getattr(back, name).view(np.uint32)), name
    assert np.array_equal(back.pack().view(np.uint32), packed.view(np.uint32))
    # the documented places
    hp = (hidden + 3) & ~3
    R = D + 1 + hp + 4
    assert pol.param_count == 4 + hidden * R
    j = hidden - 1
    rec = packed[1, 4 + R * j: 4 + R * (j + 1)]
    assert np.array_equal(packed[:, :4], pol.bo)
    assert np.array_equal(rec[:D], pol.wx[1, j]) and rec[D] == pol.b[1, j]
    assert np.array_equal(rec[D + 1:D + 1 + hidden], pol.wh[1, j]) and not rec[D + 1 + hidden:D + 1 + hp].any()
    assert np.array_equal(rec[R - 4:], pol.wo[1, :, j])


def test_param_count_refusals():
    from metagym_amd import _lib
    lib = _lib.load()
    assert [input_dim(v) for v in (1, 2, 3)] == [15, 31, 55]
    for bad in (0, 65):
        with pytest.raises(ValueError):
            param_count(bad, 1)
        assert lib.mg_maze2d_policy_param_count(bad, 1) == -1002 and b"hidden" in lib.mg_last_error()
    for bad in (0, 4):
        with pytest.raises(ValueError):
            param_count(5, bad)
        assert lib.mg_maze2d_policy_param_count(5, bad) == -1003 and b"view_grid" in lib.mg_last_error()


def test_policy_constructor_refusals():
    f = lambda *s: np.zeros(s, F)
    ok = lambda P=1, H=5, D=15: [f(P, H, D), f(P, H, H), f(P, H), f(P, 4, H), f(P, 4)]
    MazePolicy(*ok())
    MazePolicy(*ok(H=1, D=55))
    MazePolicy(*ok(H=MAX_HIDDEN, D=31))
    with pytest.raises(ValueError):
        MazePolicy(*ok(H=65))                                                  # H too large
    with pytest.raises(ValueError):
        MazePolicy(*ok(H=0))                                                   # H = 0
    with pytest.raises(ValueError):
        MazePolicy(*ok(P=0))                                                   # P = 0
    for D in (9, 16, 87):                                                      # view_grid 0 and 4, and no window at all
        with pytest.raises(ValueError):
            MazePolicy(*ok(D=D))
    for k, shape in ((1, (1, 5, 4)), (2, (1, 4)), (3, (1, 3, 5)), (3, (1, 4, 4)), (4, (1, 3)), (4, (2, 4))):
        a = ok()
        a[k] = f(*shape)
        with pytest.raises(ValueError):
            MazePolicy(*a)
    for k in range(5):
        a = ok()
        a[k] = a[k][0]                                                         # one dimension short
        with pytest.raises(ValueError):
            MazePolicy(*a)
        a = ok()
        a[k] = a[k].astype(np.float64)
        with pytest.raises(TypeError):
            MazePolicy(*a)
        for v in (np.inf, np.nan):
            a = ok()
            a[k].flat[0] = v
            with pytest.raises(ValueError):
                MazePolicy(*a)
    with pytest.raises(TypeError):
        MazePolicy(*ok(), epsilon=np.zeros(1, F))                              # epsilon is float64
    for eps in (np.zeros(2), np.array([-1e-9]), np.array([1.0 + 1e-9]), np.array([np.nan])):
        with pytest.raises(ValueError):
            MazePolicy(*ok(), epsilon=eps)
    MazePolicy(*ok(P=2), epsilon=np.array([0.0, 1.0]))
    pol = MazePolicy(*ok(P=2))
    st = MazePolicyState.zeros(3, 5)
    with pytest.raises(ValueError):
        pol.reference(f(3, 3, 3), np.array([0, 1, 2]), st)                     # id out of range
    with pytest.raises(ValueError):
        pol.reference(f(3, 5, 5), np.zeros(3, int), st)                        # another window
    with pytest.raises(ValueError):
        pol.reference(f(3, 3, 3), np.zeros(3, int), MazePolicyState.zeros(3, 4))   # another H
    with pytest.raises(ValueError):
        pol.reference(f(3, 3, 3), np.zeros(3, int), MazePolicyState.zeros(2, 5))   # another N
    with pytest.raises(ValueError):
        MazePolicy.unpack(f(1, 7), 5, 1)


def test_fresh_state():
    st = MazePolicyState.zeros(3, 2)
    assert st.h.shape == (3, 2) and st.h.dtype == F and not st.h.any()
    assert st.prev_action.dtype == np.int32 and (st.prev_action == -1).all()
    assert st.prev_reward.dtype == F and not st.prev_reward.any()
    assert st.prev_done.dtype == np.uint8 and not st.prev_done.any() and st.step == 0
    assert (st.num_envs, st.hidden) == (3, 2)
    c = st.clone()
    c.h[0, 0] = 1
    assert st.h[0, 0] == 0


@pytest.mark.parametrize("hidden,view_grid", [(1, 1), (5, 2), (7, 3), (2, 1), (3, 2), (6, 3), (7, 1), (4, 2), (63, 3)])
def test_reference_equals_the_scalar_restatement(hidden, view_grid):
    P, n = 3, 11
    pol = _random_policy(P, hidden, view_grid, 5)
    w = 2 * view_grid + 1
    rs = np.random.RandomState(6)
    win = rs.choice([-1.0, 0.0, 1.0, 0.37], (n, w, w)).astype(F)
    ids = rs.randint(0, P, n)
    st = _state(rs.uniform(-1, 1, (n, hidden)), rs.randint(-1, 4, n), rs.uniform(-1, 1, n), rs.randint(0, 2, n))
    acts, hn = pol.reference(win, ids, st)
    assert acts.dtype == np.int32 and acts.shape == (n,) and hn.dtype == F and hn.shape == (n, hidden)
    for e in range(n):
        g, h1 = _loops(pol, int(ids[e]), win[e], st.h[e], int(st.prev_action[e]), st.prev_reward[e], int(st.prev_done[e]))
        assert g == acts[e] and np.array_equal(h1.view(np.uint32), hn[e].view(np.uint32)), e
    # the flat window is the same input, and the state was only read
    acts2, hn2 = pol.reference(win.reshape(n, w * w), ids, st)
    assert np.array_equal(acts, acts2) and np.array_equal(hn.view(np.uint32), hn2.view(np.uint32))


def test_reference_pins_the_order_on_a_hand_written_case():
    """H = 2, view_grid = 1. Unit 0: b = 1, the window entry 0 contributes 2^-24 and the entry 1 another 2^-24, then h[0]
    contributes -1 through wh. In float32, in the defined order: 1 + 2^-24 = 1 (a tie, to even), again 1, then 1 - 1 = 0. In
    float64 the result is 2^-23; summing the two small terms first (re-associated) also gives 1 + 2^-23 - 1 = 2^-23. Unit 1
    reads h[1] through wh after x: (0.5 + 2^-25) rounds to 0.5 in float32, minus 0.5 = 0; float64 keeps 2^-25."""
    t = F(2.0 ** -24)
    assert F(F(1.0) + t) == F(1.0) and F(F(1.0) + F(t + t)) != F(1.0) and 1.0 + 2.0 ** -24 + 2.0 ** -24 - 1.0 == 2.0 ** -23
    wx = np.zeros((1, 2, 15), F)
    wx[0, 0, 0] = wx[0, 0, 1] = 1.0
    wx[0, 1, 8] = 1.0
    wh = np.array([[[1.0, 0.0], [0.0, 1.0]]], F)
    b = np.array([[1.0, 0.5]], F)
    wo = np.zeros((1, 4, 2), F)
    wo[0, 1, 0] = 1.0                       # logit 1 = hn[0], logit 2 = hn[1]: any positive rest would move the argmax
    wo[0, 2, 1] = 1.0
    pol = MazePolicy(wx, wh, b, wo, np.zeros((1, 4), F))
    win = np.zeros((1, 3, 3), F)
    win[0, 0, 0] = win[0, 0, 1] = t
    win[0, 2, 2] = F(2.0 ** -25)
    st = _state([[-1.0, -0.5]], [-1], [0.0], [0])
    acts, hn = pol.reference(win, np.zeros(1, int), st)
    assert np.array_equal(hn.view(np.uint32), np.zeros((1, 2), np.uint32)) and acts[0] == 0
    # what float64 arithmetic, or float32 with the small terms added first, would have given: a positive h and action 1
    z64 = 1.0 + float(t) + float(t) - 1.0
    z_re = F(F(F(1.0) + F(t + t)) - F(1.0))
    assert z64 == 2.0 ** -23 and z_re == F(2.0 ** -23) and 0.5 + 2.0 ** -25 - 0.5 == 2.0 ** -25
    g, h1 = _loops(pol, 0, win[0], st.h[0], -1, F(0), 0)
    assert g == 0 and not h1.any()


def test_clamp_on_plus_minus_one_negative_zero_and_nan():
    """hn = z > 1 ? 1 : (z < -1 ? -1 : z): exactly +-1 pass through the third branch, the next float above 1 and below -1
    clamp, and a NaN stays a NaN. z is b alone (zero weights, zero window) except for the NaN, which is inf - inf: weights
    of 3e38 and -3e38 on two window entries of 2. -0 stays -0 (bit pattern 0x80000000): the second policy, whose weights
    carry the sign (with zero weights the first product, +0, would turn a bias of -0 into +0)."""
    up, dn = np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))
    bs = [F(1.0), F(-1.0), up, dn, F(0.75), F(3.0), F(-3.0)]
    H = len(bs) + 1
    wx = np.zeros((1, H, 15), F)
    wx[0, H - 1, 0], wx[0, H - 1, 1] = 3e38, -3e38
    pol = MazePolicy(wx, np.zeros((1, H, H), F), np.array([bs + [F(0)]], F), np.zeros((1, 4, H), F), np.zeros((1, 4), F))
    win = np.zeros((1, 3, 3), F)
    win[0, 0, 0] = win[0, 0, 1] = 2.0
    acts, hn = pol.reference(win, np.zeros(1, int), MazePolicyState.zeros(1, H))
    want = np.array([1.0, -1.0, 1.0, -1.0, 0.75, 1.0, -1.0], F)
    assert np.array_equal(hn[0, :-1].view(np.uint32), want.view(np.uint32))
    assert np.isnan(hn[0, -1])
    assert acts[0] == 0                                                        # 0 * NaN = NaN in every logit: the lowest index
    # -0 survives the x and h loops: every weight is -0 and every input >= 0, so every product is -0 and -0 + -0 = -0
    wx2 = np.full((1, 1, 15), -0.0, F)
    pol2 = MazePolicy(wx2, np.full((1, 1, 1), -0.0, F), np.array([[-0.0]], F), np.ones((1, 4, 1), F), np.full((1, 4), -0.0, F))
    acts2, hn2 = pol2.reference(np.ones((1, 3, 3), F), np.zeros(1, int), _state([[1.0]], [2], [1.0], [1]))
    assert hn2[0, 0] == 0 and np.signbit(hn2[0, 0]) and acts2[0] == 0


def test_argmax_on_ties_and_nan():
    """greedy = 0; for k in 1..3: if l[k] > l[greedy]: greedy = k. The logits are bo alone (wo = 0), except where a NaN is
    wanted: hn[0] is NaN (inf - inf) and wo routes it into chosen logits."""
    def greedy(bo, nan_into=()):
        wx = np.zeros((1, 1, 15), F)
        wo = np.zeros((1, 4, 1), F)
        win = np.zeros((1, 3, 3), F)
        if nan_into:
            wx[0, 0, 0], wx[0, 0, 1] = 3e38, -3e38
            win[0, 0, 0] = win[0, 0, 1] = 2.0
            for k in nan_into:
                wo[0, k, 0] = 1.0
        pol = MazePolicy(wx, np.zeros((1, 1, 1), F), np.zeros((1, 1), F), wo, np.array([bo], F))
        acts, hn = pol.reference(win, np.zeros(1, int), MazePolicyState.zeros(1, 1))
        assert bool(nan_into) == bool(np.isnan(hn[0, 0]))
        return int(acts[0])
    assert greedy([0, 0, 0, 0]) == 0                       # all tied: the lowest
    assert greedy([1, 2, 2, 1]) == 1                       # a tie of the two largest: the lower
    assert greedy([1, 2, 3, 3]) == 2
    assert greedy([0, 0, 0, 1]) == 3
    assert greedy([-0.0, 0.0, 0.0, 0.0]) == 0              # +0 > -0 is false
    assert greedy([3, 2, 1, 0]) == 0
    # a NaN h reaches every logit (0 * NaN is NaN, and with |h| <= 1 and finite weights no logit is NaN on its own): all four
    # are NaN whatever wo holds, nothing compares greater than l[0], and the action is 0
    assert greedy([1, 2, 3, 4], nan_into=(0, 1, 2, 3)) == 0
    assert greedy([1, 2, 3, 4], nan_into=(3,)) == 0
    assert greedy([4, 3, 2, 1], nan_into=(0,)) == 0


def test_threshold_rule_and_exploration():
    """thr = min(floor(epsilon * 2^32), 2^32 - 1): 0 never explores, 1 explores unless out[0] is 0xFFFFFFFF, 2^-32 only when
    out[0] is 0. The draw is out[1] & 3 with the counter and key of the definition."""
    eps = np.array([0.0, 1.0, 2.0 ** -32, 0.25, 0.5, 1.0 - 2.0 ** -33, 2.0 ** -33])
    assert eps_threshold(eps).dtype == np.uint32
    assert [int(v) for v in eps_threshold(eps)] == [0, 0xFFFFFFFF, 1, 1 << 30, 1 << 31, 0xFFFFFFFF, 0]
    # the published Random123 known answers, and a 64-bit step and seed split as defined
    assert [int(v) for v in philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(v) for v in philox4x32_10(*[0xffffffff] * 6)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert [int(v) for v in philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    n = 4096
    P = 3
    pol = _random_policy(P, 2, 1, 9, epsilon=np.array([0.0, 1.0, 0.25]))
    assert [int(v) for v in pol.thresholds] == [0, 0xFFFFFFFF, 1 << 30]
    ids = np.arange(n) % P
    win = np.zeros((n, 3, 3), F)
    st = MazePolicyState.zeros(n, 2)
    st.step = (7 << 32) | 5
    seed = (11 << 32) | 13
    acts, hn, ex = pol.reference(win, ids, st, seed=seed, return_explored=True)
    greedy, hn0 = MazePolicy(pol.wx, pol.wh, pol.b, pol.wo, pol.bo).reference(win, ids, st, seed=seed)
    out = philox4x32_10(np.arange(n), 5, 7, 0x4D5A, 13, 11)
    assert np.array_equal(ex, out[0] < pol.thresholds[ids])
    assert not ex[ids == 0].any() and ex[ids == 1].all() and 0 < ex[ids == 2].sum() < (ids == 2).sum()
    assert abs(ex[ids == 2].mean() - 0.25) < 0.05
    assert np.array_equal(acts, np.where(ex, out[1] & 3, greedy)) and np.array_equal(hn.view(np.uint32), hn0.view(np.uint32))
    assert sorted(set(acts[ids == 1].tolist())) == [0, 1, 2, 3]
    # another step, another seed, other env ids: other draws
    st2 = st.clone()
    st2.step += 1
    assert not np.array_equal(pol.reference(win, ids, st2, seed=seed)[0], acts)
    assert not np.array_equal(pol.reference(win, ids, st, seed=seed + 1)[0], acts)
    shifted = pol.reference(win, ids, st, seed=seed, env_ids=np.arange(n) + 3)[0]
    assert np.array_equal(shifted[ids == 1][:-1], acts[ids == 1][1:])           # env e + 3 holds policy 1 again: the same draw


def _header():
    text = open(os.path.join(ROOT, "include", "metagym_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_entry_points_are_declared_in_the_header_and_the_binding():
    from metagym_amd import _lib
    lib = _lib.load()
    text = _header()
    for name in ("mg_maze2d_policy_rollout", "mg_maze2d_policy_param_count"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    for name in ("mg_maze_policy", "mg_maze_policy_carry"):
        assert re.search(r"\}\s*%s\s*;" % name, text), name
    assert re.search(r"#define\s+MG_ABI_VERSION\s+10\b", text) and _lib.ABI_VERSION == 10
    # the structs of the binding have the header's fields in the header's order
    m = re.search(r"typedef struct mg_maze_policy \{(.*?)\} mg_maze_policy;", text, re.S)
    assert re.findall(r"(\w+)\s*[;,]", m.group(1)) == [f[0] for f in _lib.MazePolicyDesc._fields_]
    m = re.search(r"typedef struct mg_maze_policy_carry \{(.*?)\} mg_maze_policy_carry;", text, re.S)
    assert re.findall(r"(\w+)\s*[;,]", m.group(1)) == [f[0] for f in _lib.MazePolicyCarry._fields_]
    assert len(_lib.SIGNATURES["mg_maze2d_policy_rollout"][1]) == 26


def test_abi_refuses_on_the_host_before_any_device_call():
    from metagym_amd import _lib
    lib = _lib.load()
    fake = C.create_string_buffer(256)
    base = (C.addressof(fake) + 15) & ~15
    p = C.c_void_p(base)
    tasks = _lib.MazeTasks()
    tasks.n, tasks.n_tasks = 9, 1
    for name in ("start", "goal", "walls", "texts", "scalars"):
        setattr(tasks, name, base)
    st = _lib.MazeState()
    st.task_id = st.grid = st.steps = base
    pol = _lib.MazePolicyDesc(3, 5, 2, base, None)
    carry = _lib.MazePolicyCarry(base, base, base, base)
    order = (("tasks", tasks), ("task_type", 0), ("max_steps", 10), ("view_grid", 2), ("auto_reset", 1), ("n", 4), ("state", st),
             ("steps", 2), ("obs_every", 0), ("policy", pol), ("ids", p), ("carry", carry), ("seed", 0), ("step0", 0),
             ("episodic", 0), ("obs_last", p), ("ret_total", p), ("ret_episode", p), ("episode_len", p), ("episodes", p),
             ("actions", None), ("reward", None), ("reward64", None), ("done", None), ("obs", None), ("stream", None))
    call = lambda **kw: lib.mg_maze2d_policy_rollout(*[kw.get(k, v) for k, v in order])
    for name in ("tasks", "state", "policy", "ids", "carry", "obs_last", "ret_total", "ret_episode", "episode_len", "episodes"):
        assert call(**{name: None}) == -1001, name
        assert b"NULL" in lib.mg_last_error()
    assert call(policy=_lib.MazePolicyDesc(3, 5, 2, None, None)) == -1001
    for k in range(4):
        ptrs = [base] * 4
        ptrs[k] = None
        assert call(carry=_lib.MazePolicyCarry(*ptrs)) == -1001
    assert call(state=_lib.MazeState()) == -1001
    assert call(task_type=1) == -1001                                          # SURVIVAL needs the food arrays
    assert call(n=0) == -1002 and call(steps=0) == -1002 and call(obs_every=-1) == -1002
    assert call(policy=_lib.MazePolicyDesc(0, 5, 2, base, None)) == -1002 and b"n_policies" in lib.mg_last_error()
    assert call(policy=_lib.MazePolicyDesc(3, 0, 2, base, None)) == -1002 and b"hidden" in lib.mg_last_error()
    assert call(policy=_lib.MazePolicyDesc(3, 65, 2, base, None)) == -1002
    assert call(policy=_lib.MazePolicyDesc(3, 5, 1, base, None)) == -1003 and b"view_grid" in lib.mg_last_error()
    assert call(view_grid=4, policy=_lib.MazePolicyDesc(3, 5, 4, base, None)) == -1003
    assert call(view_grid=0, policy=_lib.MazePolicyDesc(3, 5, 0, base, None)) == -1003
    assert call(policy=_lib.MazePolicyDesc(3, 5, 2, base + 4, None)) == -1003 and b"aligned" in lib.mg_last_error()
    assert call(task_type=2) == -1003


def test_only_the_2d_env_has_the_method():
    from metagym_amd.metamaze import MetaMaze2D, MetaMazeContinuous3D, MetaMazeDiscrete3D
    assert hasattr(MetaMaze2D, "rollout_policy")
    assert not hasattr(MetaMazeDiscrete3D, "rollout_policy") and not hasattr(MetaMazeContinuous3D, "rollout_policy")
