"""Recurrent bandit policies, host side (no GPU): the exact definition (BanditPolicy.reference), the packed layout, the
constructor's refusals, the order of the additions, the clamp, the argmax, the exploration threshold, and the ABI's
declarations and host-side refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from metagym_amd.bandits import BanditPolicy, BanditPolicyState
from metagym_amd.bandits.policy import MAX_ARMS, MAX_HIDDEN, PHILOX_TAG, param_count
from metagym_amd.metamaze.policy import MazePolicyState, eps_threshold, philox4x32_10

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_policy(P, H, K, seed, epsilon=None):
    rs = np.random.RandomState(seed)
    return BanditPolicy(rs.randn(P, H, K).astype(F), rs.randn(P, H).astype(F), rs.randn(P, H).astype(F),
                        (rs.randn(P, H, H) / np.sqrt(H)).astype(F), (0.1 * rs.randn(P, H)).astype(F),
                        (rs.randn(P, K, H) / np.sqrt(H)).astype(F), (0.1 * rs.randn(P, K)).astype(F), epsilon)


def _state(h, prev_action, prev_reward, prev_done, step=0):
    return BanditPolicyState(np.asarray(h, F), np.asarray(prev_action, np.int32), np.asarray(prev_reward, F),
                             np.asarray(prev_done, np.uint8), step)


def _zero_policy(H, K, **kw):
    """One policy, every weight +0, but for the arrays given."""
    a = dict(wa=np.zeros((1, H, K), F), wr=np.zeros((1, H), F), wd=np.zeros((1, H), F), wh=np.zeros((1, H, H), F),
             b=np.zeros((1, H), F), wo=np.zeros((1, K, H), F), bo=np.zeros((1, K), F))
    for name, v in kw.items():
        a[name] = np.asarray(v, F).reshape(a[name].shape)
    return BanditPolicy(a["wa"], a["wr"], a["wd"], a["wh"], a["b"], a["wo"], a["bo"])


def _loops(pol, pid, h, pa, pr, pd):
    """The definition restated with explicit Python loops over np.float32 scalars: no float64, no vector operation."""
    H, K = pol.hidden, pol.arms
    hn = []
    with np.errstate(all="ignore"):
        for j in range(H):
            z = F(pol.b[pid, j])
            if pa >= 0:
                z = F(z + F(pol.wa[pid, j, pa]))
            z = F(z + F(F(pol.wr[pid, j]) * F(pr)))
            z = F(z + F(F(pol.wd[pid, j]) * (F(1.0) if pd else F(0.0))))
            for i in range(H):
                z = F(z + F(F(pol.wh[pid, j, i]) * F(h[i])))
            hn.append(F(1.0) if z > 1 else (F(-1.0) if z < -1 else z))
        logits = []
        for k in range(K):
            v = F(pol.bo[pid, k])
            for j in range(H):
                v = F(v + F(F(pol.wo[pid, k, j]) * hn[j]))
            logits.append(v)
    g = 0
    for k in range(1, K):
        if logits[k] > logits[g]:
            g = k
    return g, np.array(hn, F)


@pytest.mark.parametrize("arms", [2, 3, 10, 64, 4, 5, 6, 7, 63])          # the sizes of policy_size_cases.BANDITS_ADDED too
@pytest.mark.parametrize("hidden", [1, 3, 4, 5, 64, 2, 6, 7, 63])
def test_pack_round_trips_and_matches_the_library_count(hidden, arms):
    from metagym_amd import _lib
    lib = _lib.load()
    H, K = hidden, arms
    pol = _random_policy(2, H, K, 3, epsilon=np.array([0.0, 0.5]))
    packed = pol.pack()
    assert packed.dtype == F and packed.shape == (2, pol.param_count)
    assert lib.mg_bandits_policy_param_count(H, K) == pol.param_count == param_count(H, K)
    back = BanditPolicy.unpack(packed, H, K, pol.epsilon)
    assert (back.hidden, back.arms, back.num_policies) == (H, K, 2)
    for name in ("wa", "wr", "wd", "wh", "b", "wo", "bo"):
        assert np.array_equal(getattr(pol, name).view(np.uint32), getattr(back, name).view(np.uint32)), name
    assert np.array_equal(back.pack().view(np.uint32), packed.view(np.uint32))
    # the documented places; every record starts on a multiple of four floats (16-byte reads are aligned)
    hp, kp = (H + 3) & ~3, (K + 3) & ~3
    ru, ra = 4 + kp + hp, 4 + hp
    assert pol.param_count == H * ru + K * ra and ru % 4 == 0 and ra % 4 == 0 and pol.param_count % 4 == 0
    j, k = H - 1, K - 1
    rec = packed[1, ru * j: ru * (j + 1)]
    assert rec[0] == pol.b[1, j] and rec[1] == pol.wr[1, j] and rec[2] == pol.wd[1, j] and rec[3] == 0
    assert np.array_equal(rec[4:4 + K], pol.wa[1, j]) and not rec[4 + K:4 + kp].any()
    assert np.array_equal(rec[4 + kp:4 + kp + H], pol.wh[1, j]) and not rec[4 + kp + H:].any()
    rec = packed[1, H * ru + ra * k: H * ru + ra * (k + 1)]
    assert rec[0] == pol.bo[1, k] and not rec[1:4].any()
    assert np.array_equal(rec[4:4 + H], pol.wo[1, k]) and not rec[4 + H:].any()


def test_param_count_refusals():
    from metagym_amd import _lib
    lib = _lib.load()
    for bad in (0, MAX_HIDDEN + 1):
        with pytest.raises(ValueError):
            param_count(bad, 10)
        assert lib.mg_bandits_policy_param_count(bad, 10) == -1002 and b"hidden" in lib.mg_last_error()
    for bad in (0, 1, MAX_ARMS + 1):
        with pytest.raises(ValueError):
            param_count(5, bad)
        assert lib.mg_bandits_policy_param_count(5, bad) == -1002 and b"arms" in lib.mg_last_error()
    assert lib.mg_bandits_policy_param_count(64, 64) == 64 * 132 + 64 * 68


def test_policy_constructor_refusals():
    f = lambda *s: np.zeros(s, F)
    ok = lambda P=1, H=5, K=10: [f(P, H, K), f(P, H), f(P, H), f(P, H, H), f(P, H), f(P, K, H), f(P, K)]
    BanditPolicy(*ok())
    BanditPolicy(*ok(H=1, K=2))
    BanditPolicy(*ok(H=MAX_HIDDEN, K=MAX_ARMS))
    for kw in (dict(H=65), dict(H=0), dict(P=0), dict(K=1), dict(K=65)):
        with pytest.raises(ValueError):
            BanditPolicy(*ok(**kw))
    for k, shape in ((1, (1, 4)), (2, (2, 5)), (3, (1, 5, 4)), (3, (1, 4, 5)), (4, (1, 6)), (5, (1, 5, 10)), (5, (1, 9, 5)),
                     (6, (1, 9)), (6, (2, 10))):
        a = ok()
        a[k] = f(*shape)
        with pytest.raises(ValueError):
            BanditPolicy(*a)
    for k in range(7):
        a = ok()
        a[k] = a[k][0]                                                         # one dimension short
        with pytest.raises(ValueError):
            BanditPolicy(*a)
        a = ok()
        a[k] = a[k].astype(np.float64)
        with pytest.raises(TypeError):
            BanditPolicy(*a)
        for v in (np.inf, np.nan):
            a = ok()
            a[k].flat[0] = v
            with pytest.raises(ValueError):
                BanditPolicy(*a)
    with pytest.raises(TypeError):
        BanditPolicy(*ok(), epsilon=np.zeros(1, F))                            # epsilon is float64
    for eps in (np.zeros(2), np.array([-1e-9]), np.array([1.0 + 1e-9]), np.array([np.nan])):
        with pytest.raises(ValueError):
            BanditPolicy(*ok(), epsilon=eps)
    BanditPolicy(*ok(P=2), epsilon=np.array([0.0, 1.0]))
    pol = BanditPolicy(*ok(P=2))
    st = BanditPolicyState.zeros(3, 5)
    with pytest.raises(ValueError):
        pol.reference(np.array([0, 1, 2]), st)                                 # id out of range
    with pytest.raises(ValueError):
        pol.reference(np.zeros(3, int), BanditPolicyState.zeros(3, 4))         # another H
    with pytest.raises(ValueError):
        pol.reference(np.zeros(3, int), BanditPolicyState.zeros(2, 5))         # another N
    bad = BanditPolicyState.zeros(3, 5)
    bad.prev_action[1] = 10
    with pytest.raises(ValueError):
        pol.reference(np.zeros(3, int), bad)                                   # a previous action that is no arm
    with pytest.raises(ValueError):
        BanditPolicy.unpack(f(1, 7), 5, 10)


def test_the_carry_is_the_maze_policies_carry():
    assert BanditPolicyState is MazePolicyState
    st = BanditPolicyState.zeros(3, 2)
    assert st.h.shape == (3, 2) and (st.prev_action == -1).all() and not st.prev_reward.any() and not st.prev_done.any()
    assert st.step == 0 and PHILOX_TAG == 0x4241


@pytest.mark.parametrize("hidden,arms", [(1, 2), (5, 3), (7, 10), (64, 64), (2, 5), (4, 4), (6, 7), (7, 63), (63, 6)])
def test_reference_equals_the_scalar_restatement(hidden, arms):
    P, n = 3, 11 if hidden < 64 else 4
    pol = _random_policy(P, hidden, arms, 5)
    rs = np.random.RandomState(6)
    ids = rs.randint(0, P, n)
    st = _state(rs.uniform(-1, 1, (n, hidden)), rs.randint(-1, arms, n), rs.randint(0, 2, n), rs.randint(0, 2, n))
    st.prev_action[0] = -1
    st.prev_action[1] = arms - 1
    before = st.clone()
    acts, hn = pol.reference(ids, st)
    assert acts.dtype == np.int32 and acts.shape == (n,) and hn.dtype == F and hn.shape == (n, hidden)
    for e in range(n):
        g, h1 = _loops(pol, int(ids[e]), st.h[e], int(st.prev_action[e]), st.prev_reward[e], int(st.prev_done[e]))
        assert g == acts[e] and np.array_equal(h1.view(np.uint32), hn[e].view(np.uint32)), e
    assert np.array_equal(st.h, before.h) and np.array_equal(st.prev_action, before.prev_action)   # the state was only read
    if arms > 2:
        assert len(set(acts.tolist())) > 1


def test_reference_pins_the_order_on_a_hand_written_case():
    """H = 2, K = 3, t = 2^-24. Unit 0: b = 1, wa[0][prev_action] = t, wr * prev_reward = t, wd * 1 = 0, wh[0][0] * h[0] =
    -1. In float32, in the defined order: 1 + t = 1 (a tie, to even), again 1, 1 + 0, then 1 - 1 = 0. In float64 the result
    is 2^-23, and float32 with the two small terms added first gives 2^-23 too. Unit 1: b = t, the lookup adds 1 (1 + t = 1),
    the reward term adds -1: 0; with the lookup after the reward term it would be (t - 1) + 1 = t. The logits are hn[0] and
    hn[1] on arms 1 and 2 against 0 on arm 0: any positive rest moves the argmax."""
    t = F(2.0 ** -24)
    assert F(F(1.0) + t) == F(1.0) and F(F(1.0) + F(t + t)) != F(1.0) and 1.0 + 2.0 ** -24 + 2.0 ** -24 - 1.0 == 2.0 ** -23
    assert F(F(t - F(1.0)) + F(1.0)) != 0
    pol = _zero_policy(2, 3, wa=[[0, t, 0], [0, 1, 0]], wr=[t, -1], wh=[[1, 0], [0, 0]], b=[1, t],
                       wo=[[0, 0], [1, 0], [0, 1]])
    st = _state([[-1.0, 0.25]], [1], [1.0], [1])
    acts, hn = pol.reference(np.zeros(1, int), st)
    assert np.array_equal(hn.view(np.uint32), np.zeros((1, 2), np.uint32)) and acts[0] == 0
    g, h1 = _loops(pol, 0, st.h[0], 1, F(1), 1)
    assert g == 0 and not h1.any()
    # the done term comes after the reward term and before the recurrent sum: b = 1, wr * 1 = t, wd * 1 = t, wh * h = -1
    pol = _zero_policy(1, 2, wr=[t], wd=[t], wh=[[1]], b=[1], wo=[[0], [1]])
    acts, hn = pol.reference(np.zeros(1, int), _state([[-1.0]], [-1], [1.0], [1]))
    assert hn[0, 0] == 0 and acts[0] == 0
    # and prev_done = 0 leaves the term out as wd * 0
    pol = _zero_policy(1, 2, wd=[0.5], b=[0.25], wo=[[0], [1]])
    acts, hn = pol.reference(np.zeros(2, int), _state([[0.0], [0.0]], [-1, -1], [0.0, 0.0], [0, 1]))
    assert hn[:, 0].tolist() == [0.25, 0.75] and acts.tolist() == [1, 1]


def test_clamp_on_plus_minus_one_negative_zero_and_nan():
    """hn = z > 1 ? 1 : (z < -1 ? -1 : z): exactly +-1 pass through the third branch, the next float above 1 and below -1
    clamp, and a NaN stays a NaN. z is b alone (zero weights) except for the NaN, which is inf - inf: recurrent weights of
    3e38 and -3e38 on two units of the carry that hold 2."""
    up, dn = np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))
    bs = [F(1.0), F(-1.0), up, dn, F(0.75), F(3.0), F(-3.0)]
    H = len(bs) + 1
    wh = np.zeros((1, H, H), F)
    wh[0, H - 1, 0], wh[0, H - 1, 1] = 3e38, -3e38
    pol = _zero_policy(H, 3, wh=wh, b=bs + [F(0)])
    h0 = np.zeros((1, H), F)
    h0[0, :2] = 2.0
    acts, hn = pol.reference(np.zeros(1, int), _state(h0, [-1], [0.0], [0]))
    want = np.array([1.0, -1.0, 1.0, -1.0, 0.75, 1.0, -1.0], F)
    assert np.array_equal(hn[0, :-1].view(np.uint32), want.view(np.uint32))
    assert np.isnan(hn[0, -1])
    assert acts[0] == 0                                                        # 0 * NaN = NaN in every logit: the lowest index
    g, h1 = _loops(pol, 0, h0[0], -1, F(0), 0)
    assert g == 0 and np.isnan(h1[-1]) and np.array_equal(h1[:-1], want)


def test_negative_zero_survives_because_the_one_hot_is_a_lookup():
    """b = -0, wr = wd = -0 (times a reward and a done >= 0: -0), wh = +0 on a carry of -0 (+0 * -0 = -0): every addend is
    -0 and so is the sum (bit pattern 0x80000000). wa is all ones and there is no previous action: the lookup adds nothing. A
    K-wide one-hot multiply-add would add wa[j][k] * 0 = +0, and -0 + +0 = +0."""
    neg = np.full((1, 1), -0.0, F)
    pol = _zero_policy(1, 3, wa=np.ones((1, 1, 3), F), wr=neg, wd=neg, b=neg, wo=np.ones((1, 3, 1), F),
                       bo=np.full((1, 3), -0.0, F))
    for pr, pd in ((0.0, 0), (1.0, 1)):
        acts, hn = pol.reference(np.zeros(1, int), _state([[-0.0]], [-1], [pr], [pd]))
        assert hn.view(np.uint32)[0, 0] == 0x80000000 and acts[0] == 0
        g, h1 = _loops(pol, 0, np.array([-0.0], F), -1, F(pr), pd)
        assert h1.view(np.uint32)[0] == 0x80000000 and g == 0
    assert F(F(-0.0) + F(F(1.0) * F(0.0))).view(np.uint32) == 0                 # what the multiply-add form would give
    # with a previous action the lookup is one add of wa[j][prev_action] alone
    acts, hn = pol.reference(np.zeros(1, int), _state([[-0.0]], [2], [0.0], [0]))
    assert hn[0, 0] == 1.0


def test_argmax_on_ties_and_nan():
    """greedy = 0; for k in 1..K-1: if l[k] > l[greedy]: greedy = k. The logits are bo alone (wo = 0), except where a NaN is
    wanted: hn[0] is NaN (inf - inf through wh on a carry of 2, 2) and wo routes it into chosen logits."""
    def greedy(bo, nan_into=()):
        K = len(bo)
        wh = np.zeros((1, 2, 2), F)
        wo = np.zeros((1, K, 2), F)
        h0 = np.zeros((1, 2), F)
        if nan_into:
            wh[0, 0, 0], wh[0, 0, 1] = 3e38, -3e38
            h0[:] = 2.0
            for k in nan_into:
                wo[0, k, 0] = 1.0
        pol = _zero_policy(2, K, wh=wh, wo=wo, bo=bo)
        acts, hn = pol.reference(np.zeros(1, int), _state(h0, [-1], [0.0], [0]))
        assert bool(nan_into) == bool(np.isnan(hn[0, 0]))
        return int(acts[0])
    assert greedy([0, 0, 0, 0, 0]) == 0                    # all tied: the lowest
    assert greedy([1, 2, 2, 1, 0]) == 1                    # a tie of the two largest: the lower
    assert greedy([1, 2, 3, 3, 3]) == 2
    assert greedy([0, 0, 0, 0, 1]) == 4
    assert greedy([-0.0, 0.0, 0.0]) == 0                   # +0 > -0 is false
    assert greedy([3, 2, 1]) == 0 and greedy([1, 2]) == 1 and greedy([2, 2]) == 0
    # a NaN h reaches every logit (0 * NaN is NaN): all are NaN whatever wo holds, nothing compares greater than l[0]
    assert greedy([1, 2, 3, 4, 5], nan_into=(0, 1, 2, 3, 4)) == 0
    assert greedy([1, 2, 3, 4, 5], nan_into=(4,)) == 0
    assert greedy([5, 4, 3], nan_into=(0,)) == 0


def test_threshold_rule_and_exploration():
    """thr = min(floor(epsilon * 2^32), 2^32 - 1): 0 never explores, 1 explores unless out[0] is 0xFFFFFFFF, 2^-32 only when
    out[0] is 0. The draw is out[1] % K, an unsigned modulo, with the counter and key of the definition; K = 10 and 3 are no
    powers of two, so the modulo is not a mask."""
    eps = np.array([0.0, 1.0, 2.0 ** -32, 0.25, 0.5, 1.0 - 2.0 ** -33, 2.0 ** -33])
    assert [int(v) for v in eps_threshold(eps)] == [0, 0xFFFFFFFF, 1, 1 << 30, 1 << 31, 0xFFFFFFFF, 0]
    n, P = 4096, 3
    for K in (10, 3):
        pol = _random_policy(P, 2, K, 9, epsilon=np.array([0.0, 1.0, 0.25]))
        assert [int(v) for v in pol.thresholds] == [0, 0xFFFFFFFF, 1 << 30]
        ids = np.arange(n) % P
        st = BanditPolicyState.zeros(n, 2)
        st.step = (7 << 32) | 5
        seed = (11 << 32) | 13
        acts, hn, ex = pol.reference(ids, st, seed=seed, return_explored=True)
        plain = BanditPolicy(pol.wa, pol.wr, pol.wd, pol.wh, pol.b, pol.wo, pol.bo)
        greedy, hn0 = plain.reference(ids, st, seed=seed)
        out = philox4x32_10(np.arange(n), 5, 7, 0x4241, 13, 11)
        assert np.array_equal(ex, out[0] < pol.thresholds[ids])
        assert not ex[ids == 0].any() and ex[ids == 1].all() and 0 < ex[ids == 2].sum() < (ids == 2).sum()
        assert abs(ex[ids == 2].mean() - 0.25) < 0.05
        draw = np.array([int(v) % K for v in out[1]], np.int32)               # Python integers: no sign, no wrap
        assert np.array_equal(acts, np.where(ex, draw, greedy)) and np.array_equal(hn.view(np.uint32), hn0.view(np.uint32))
        assert (out[1] >= 2 ** 31).any() and not np.array_equal(draw, (out[1] & np.uint32(K - 1)).astype(np.int32))
        assert sorted(set(acts[ids == 1].tolist())) == list(range(K))
        # another step, another seed, other env ids: other draws
        st2 = st.clone()
        st2.step += 1
        assert not np.array_equal(pol.reference(ids, st2, seed=seed)[0], acts)
        assert not np.array_equal(pol.reference(ids, st, seed=seed + 1)[0], acts)
        shifted = pol.reference(ids, st, seed=seed, env_ids=np.arange(n) + 3)[0]
        assert np.array_equal(shifted[ids == 1][:-1], acts[ids == 1][1:])       # env e + 3 holds policy 1 again: the same draw


def _header():
    text = open(os.path.join(ROOT, "include", "metagym_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_entry_points_are_declared_in_the_header_and_the_binding():
    from metagym_amd import _lib
    lib = _lib.load()
    text = _header()
    for name in ("mg_bandits_policy_rollout", "mg_bandits_policy_param_count"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"#define\s+MG_ABI_VERSION\s+10\b", text) and _lib.ABI_VERSION == 10
    # the struct of the binding has the header's fields in the header's order; the carry is the maze policies' struct
    m = re.search(r"typedef struct mg_bandits_policy \{(.*?)\} mg_bandits_policy;", text, re.S)
    assert re.findall(r"(\w+)\s*[;,]", m.group(1)) == [f[0] for f in _lib.BanditsPolicyDesc._fields_]
    assert [f[0] for f in _lib.BanditsPolicyDesc._fields_] == ["params", "eps_threshold", "n_policies", "hidden", "arms"]
    assert re.search(r"typedef\s+mg_maze_policy_carry\s+mg_bandits_policy_carry\s*;", text)
    assert _lib.BanditsPolicyCarry is _lib.MazePolicyCarry
    assert len(_lib.SIGNATURES["mg_bandits_policy_rollout"][1]) == 23
    from csrc_structure import assert_unit_sits_on_the_bandits_core
    assert_unit_sits_on_the_bandits_core("bandits_policy.hip")


def test_abi_refuses_on_the_host_before_any_device_call():
    from metagym_amd import _lib
    lib = _lib.load()
    fake = C.create_string_buffer(256)
    base = (C.addressof(fake) + 15) & ~15
    p = C.c_void_p(base)

    def config(arms=10, max_steps=7, distribution=0):
        c = _lib.BanditsConfig()
        c.arms, c.max_steps, c.auto_reset, c.distribution = arms, max_steps, 1, distribution
        return c
    st = _lib.BanditsState(base, base, base, base, base, base)
    desc = lambda n=3, h=5, k=10, params=base: _lib.BanditsPolicyDesc(params, None, n, h, k)
    carry = _lib.BanditsPolicyCarry(base, base, base, base)
    order = (("cfg", config()), ("n", 4), ("state", st), ("steps", 2), ("policy", desc()), ("ids", p), ("carry", carry),
             ("seed", 0), ("step0", 0), ("episodic", 0), ("ret_total", p), ("ret_episode", p), ("episode_len", p),
             ("episodes", p), ("regret", p), ("actions", None), ("reward", None), ("done", None), ("info_steps", None),
             ("expected_gain", None), ("best_gain", None), ("invalid", None), ("stream", None))
    call = lambda **kw: lib.mg_bandits_policy_rollout(*[kw.get(k, v) for k, v in order])
    for name in ("cfg", "state", "policy", "ids", "carry", "ret_total", "ret_episode", "episode_len", "episodes", "regret"):
        assert call(**{name: None}) == -1001, name
        assert b"NULL" in lib.mg_last_error()
    assert call(policy=desc(params=None)) == -1001
    for k in range(4):
        ptrs = [base] * 4
        ptrs[k] = None
        assert call(carry=_lib.BanditsPolicyCarry(*ptrs)) == -1001
    for k in range(6):
        ptrs = [base] * 6
        ptrs[k] = None
        assert call(state=_lib.BanditsState(*ptrs)) == -1001
    assert call(n=0) == -1002 and call(n=-1) == -1002 and call(steps=0) == -1002 and call(steps=-2) == -1002
    assert call(policy=desc(n=0)) == -1002 and b"n_policies" in lib.mg_last_error()
    assert call(policy=desc(h=0)) == -1002 and b"hidden" in lib.mg_last_error()
    assert call(policy=desc(h=65)) == -1002
    assert call(cfg=config(arms=65), policy=desc(k=65)) == -1002 and b"arms" in lib.mg_last_error()
    assert call(policy=desc(k=1)) == -1002
    assert call(policy=desc(k=9)) == -1003 and b"arms" in lib.mg_last_error()      # not the env's K
    assert call(cfg=config(arms=100)) == -1003                                      # the env accepts K = 100, the policy is for 10
    assert call(policy=desc(params=base + 4)) == -1003 and b"aligned" in lib.mg_last_error()
    # the config checks of mg_bandits_step
    assert call(cfg=config(arms=1), policy=desc(k=1)) == -1003
    assert call(cfg=config(max_steps=1)) == -1003 and b"max_steps" in lib.mg_last_error()
    assert call(cfg=config(distribution=4)) == -1003 and call(cfg=config(distribution=-1)) == -1003


def test_the_env_has_the_method_and_the_package_exports_the_classes():
    import inspect
    import metagym_amd.bandits as mb
    assert {"BanditPolicy", "BanditPolicyState", "BanditsPolicyRollout"} <= set(mb.__all__)
    sig = inspect.signature(mb.Bandits.rollout_policy)
    assert list(sig.parameters) == ["self", "policy", "steps", "policy_ids", "state", "seed", "record", "episodic"]
    assert [sig.parameters[k].default for k in ("policy_ids", "state", "seed", "record", "episodic")] == [None, None, 0, False, False]
    assert set(mb.BanditsPolicyRollout.__slots__) == {"ret_total", "ret_episode", "episode_len", "episodes", "regret", "state",
                                                      "actions", "reward", "done", "info_steps", "expected_gain", "best_gain",
                                                      "invalid"}
