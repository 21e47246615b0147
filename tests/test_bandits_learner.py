"""Classical bandit learners, host side (no GPU): log32 and the sampler of the definition, the four rules, the Gittins table,
the ABI's declarations and host-side refusals, and `BanditLearner.reference` closed loop against the reference's env."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import bandits_learner_host as blh
from metagym_amd.bandits import BanditLearner, BanditLearnerState, BanditPolicy, BanditPolicyState, gittins_index_table, log32
from metagym_amd.bandits import learner as L
from metagym_amd.metamaze.policy import philox4x32_10

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(1, 1), (1, 2), (3, 1), (10, 40), (2500, 2500), (1, 4999)]


def _bits(v):
    return int(np.array([v], F).view(np.uint32)[0])


def _f(bits):
    return np.array([bits], np.uint32).view(F)[0]


# ---------------------------------------------------------------------------------------------------- scalar restatement
def _log32_scalar(x):
    """log32 one np.float32 operation at a time, on one value."""
    i = (_bits(x) + 0x3f800000 - 0x3f3504f3) & 0xFFFFFFFF
    k = (i >> 23) - 127
    m = _f((i & 0x007fffff) + 0x3f3504f3)
    f = F(m - F(1))
    s = F(f / F(F(2) + f))
    z = F(s * s)
    w = F(z * z)
    t1 = F(w * F(_f(0x3eccce13) + F(w * _f(0x3e789e26))))
    t2 = F(z * F(_f(0x3f2aaaaa) + F(w * _f(0x3e91e9ee))))
    R = F(t2 + t1)
    hfsq = F(F(F(0.5) * f) * f)
    dk = F(k)
    return F(F(F(F(F(s * F(hfsq + R)) + F(dk * _f(0x3717f7d1))) - hfsq) + f) + F(dk * _f(0x3f317180)))


def _u01_scalar(word):
    return F(F(((int(word) >> 9) << 1) | 1) * F(2.0 ** -24))


def _gamma_scalar(a, e, n, k, which, seed, max_attempts):
    d = F(F(a) - F(0.33333334))
    c = F(F(1) / np.sqrt(F(F(9) * d)))
    for i in range(max_attempts):
        o = [int(v) for v in philox4x32_10(e, n & 0xFFFFFFFF, n >> 32, 0x4C000000 | k << 17 | which << 16 | i,
                                           seed & 0xFFFFFFFF, seed >> 32)]
        v1 = F(F(F(2) * _u01_scalar(o[0])) - F(1))
        v2 = F(F(F(2) * _u01_scalar(o[1])) - F(1))
        s = F(F(v1 * v1) + F(v2 * v2))
        if s >= 1:
            continue
        x = F(v1 * np.sqrt(F(F(F(-2) * _log32_scalar(s)) / s)))
        v = F(F(1) + F(c * x))
        if v <= 0:
            continue
        v3 = F(F(v * v) * v)
        if _log32_scalar(_u01_scalar(o[2])) < F(F(F(F(F(F(0.5) * x) * x) + d) - F(d * v3)) + F(d * _log32_scalar(v3))):
            return F(d * v3), i + 1
    return d, max_attempts + 1


def _scores_scalar(learner, pid, pulls, wins, e, n, seed):
    """The K scores of one env, loop by loop over np.float32 scalars and Python integers."""
    K = learner.arms
    a0, b0, c = (F(v) for v in learner.params[pid, :3])
    if learner.kind == "ucb":
        if any(int(p) == 0 for p in pulls):
            return [F(np.inf) if int(p) == 0 else F(0) for p in pulls]
        lt = F(c * _log32_scalar(F(sum(int(p) for p in pulls))))
    out = []
    for k in range(K):
        nk, w = int(pulls[k]), int(wins[k])
        if learner.kind == "greedy":
            out.append(F(F(F(w) + a0) / F(F(F(nk) + a0) + b0)))
        elif learner.kind == "ucb":
            out.append(F(F(F(w) / F(nk)) + np.sqrt(F(lt / F(nk)))))
        elif learner.kind == "table":
            cap = learner.table_cap
            cell = nk * (nk + 1) // 2 + w if nk <= cap else cap * (cap + 1) // 2 + (w * cap) // nk
            out.append(learner.index[pid, cell])
        else:
            X, _ = _gamma_scalar(F(F(w) + a0), e, n, k, 0, seed, learner.max_attempts)
            Y, _ = _gamma_scalar(F(F(nk - w) + b0), e, n, k, 1, seed, learner.max_attempts)
            out.append(F(X / F(X + Y)))
    return out


def _argmax_scalar(scores):
    g = 0
    for k in range(1, len(scores)):
        if scores[k] > scores[g]:
            g = k
    return g


# ---------------------------------------------------------------------------------------------------------------- log32
def test_log32_is_within_one_ulp_of_the_float64_log():
    rs = np.random.RandomState(0)
    x = np.concatenate([rs.uniform(0, 1, 150000), np.exp(rs.uniform(-50, 50, 150000)), np.linspace(0.5, 2, 100001),
                        [2.0 ** -72, 2.0 ** -45, 2.0 ** -24, 1 - 2.0 ** -24]]).astype(F)
    x = x[x > 0]
    assert x.size > 400000 and (x >= np.finfo(F).tiny).all()
    got = log32(x)
    assert got.dtype == F and got.shape == x.shape
    want = np.log(x.astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(F)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want) / ulp
    print("log32: max error %.3f ulp over %d inputs" % (err.max(), x.size))
    assert err.max() < 1.0
    assert log32(np.array([1.0], F))[0] == 0 and log32(np.ones((2, 3), F)).shape == (2, 3)
    with pytest.raises(TypeError):
        log32(np.ones(3))


def test_log32_constants_by_their_bits():
    for name, bits in (("LG1", 0x3f2aaaaa), ("LG2", 0x3eccce13), ("LG3", 0x3e91e9ee), ("LG4", 0x3e789e26),
                       ("LN2_HI", 0x3f317180), ("LN2_LO", 0x3717f7d1)):
        v = getattr(L, name)
        assert v.dtype == F and _bits(v) == bits, name
    src = open(os.path.join(ROOT, "metagym_amd", "csrc", "bandits_learner.hip")).read()
    for bits in ("0x3f2aaaaau", "0x3eccce13u", "0x3e91e9eeu", "0x3e789e26u", "0x3f317180u", "0x3717f7d1u", "0x3f3504f3u"):
        assert bits in src, bits
    assert "0.33333334f" in src and _bits(F(0.33333334)) == 0x3eaaaaab


def test_log32_equals_its_scalar_restatement():
    rs = np.random.RandomState(1)
    x = np.concatenate([rs.uniform(0, 2, 300), np.exp(rs.uniform(-50, 50, 300)), [2.0 ** -72, 2.0 ** -45, 1 - 2.0 ** -24]]).astype(F)
    x = x[x > 0]
    got = log32(x)
    for v, g in zip(x, got):
        assert _bits(_log32_scalar(v)) == _bits(g), v


# ----------------------------------------------------------------------------------- reference against the restatement
@pytest.mark.parametrize("kind", blh.KINDS)
def test_reference_equals_the_scalar_restatement(kind):
    N, K, P = 12, 5, 3
    learner = blh.make_learner(kind, K, P)
    st = blh.random_counts(N, K, 3, top=300)
    ids = np.arange(N) % P
    seed = (5 << 32) | 9
    acts, scores = learner.reference(ids, st, seed=seed, return_scores=True)
    assert acts.dtype == np.int32 and scores.dtype == F and scores.shape == (N, K)
    for e in range(N):
        want = _scores_scalar(learner, int(ids[e]), st.pulls[e], st.wins[e], e, st.step, seed)
        assert [_bits(v) for v in want] == [_bits(v) for v in scores[e]], (kind, e)
        assert _argmax_scalar(want) == acts[e]


def test_reference_pins_the_order_on_a_hand_written_case():
    """t = 2^-24. Greedy with a0 = b0 = t, n = w = 1: (1 + t) = 1 (a tie, to even) and again (1 + t) = 1, so the score is
    1 / 1 = 1 exactly; with a0 + b0 added first the denominator is 1 + 2^-23 and the score below 1. Arm 1 holds n = w = 2
    with score (2 + t) / ((2 + t) + t) = 1 too: the tie goes to arm 0. UCB with c = 1 and pulls 1, 1: t = 2,
    score = w / n + sqrt((1 * log32(2)) / 1), and log32(2) is ln2_hi + ln2_lo rounded once."""
    t = F(2.0 ** -24)
    assert F(F(1) + t) == F(1) and F(F(1) + F(t + t)) != F(1)
    g = BanditLearner.greedy(2, np.array([[t, t]], F))
    st = BanditLearnerState(np.array([[1, 2]], np.int32), np.array([[1, 2]], np.int32))
    acts, scores = g.reference(np.zeros(1, int), st, return_scores=True)
    assert scores[0].tolist() == [1.0, 1.0] and acts[0] == 0
    assert F(F(1) + t) / F(F(1) + F(t + t)) < 1
    u = BanditLearner.ucb(2, np.array([1.0], F))
    st = BanditLearnerState(np.array([[1, 1]], np.int32), np.array([[0, 1]], np.int32))
    acts, scores = u.reference(np.zeros(1, int), st, return_scores=True)
    l2 = log32(np.array([2.0], F))[0]
    assert _bits(l2) == _bits(F(_f(0x3717f7d1) + _f(0x3f317180))) == _bits(F(math.log(2.0)))
    assert _bits(scores[0, 0]) == _bits(np.sqrt(l2)) and _bits(scores[0, 1]) == _bits(F(F(1) + np.sqrt(l2))) and acts[0] == 1


# -------------------------------------------------------------------------------------------------------------- sampler
def _beta(a, b, n, seed, max_attempts=64):
    learner = BanditLearner.thompson(2, np.array([[a, b]], F), max_attempts)
    st = BanditLearnerState.zeros(n, 2)
    st.step = 77
    _, scores, tries = learner.reference(np.zeros(n, int), st, seed=seed, return_scores=True, return_attempts=True)
    return scores, tries


@pytest.mark.parametrize("a,b", PAIRS)
def test_sampler_mean_and_range(a, b):
    """400 000 draws of X / (X + Y) (200 000 envs, two arms) against the Beta mean, 4 standard errors from the Beta variance."""
    scores, tries = _beta(a, b, 200000, seed=1234)
    s = scores.astype(np.float64).ravel()
    assert s.size == 400000 and (s > 0).all() and (s <= 1).all()
    se = math.sqrt(a * b / ((a + b) ** 2 * (a + b + 1.0)) / s.size)
    z = (s.mean() - a / (a + b)) / se
    print("Beta(%g, %g): mean off by %.2f standard errors, at most %d attempts" % (a, b, z, tries.max()))
    assert abs(z) < 4.0
    assert tries.min() >= 1 and tries.max() <= 64                            # no fallback with 64 attempts


def test_sampler_fallback_and_attempt_counts():
    scores, tries = _beta(1, 1, 5000, seed=5, max_attempts=1)
    fell = tries == 2
    assert fell.any() and (tries[~fell] == 1).all() and 0.1 < fell.mean() < 0.5
    both = fell.all(axis=2)                                                  # X = Y = d: the score is d / (d + d)
    assert both.any() and (scores[both] == 0.5).all()
    assert (scores > 0).all() and (scores <= 1).all()
    # the batch the GPU test compares: some draws need three attempts or more, none falls back
    learner, ids, st, seed = blh.thompson_probe_case()
    _, scores, tries = learner.reference(ids, st, seed=seed, return_scores=True, return_attempts=True)
    assert tries.max() >= 3 and tries.max() <= 64 and tries.min() == 1
    assert (scores > 0).all() and (scores <= 1).all()
    learner1, _, _, _ = blh.thompson_probe_case(max_attempts=1)
    assert (learner1.reference(ids, st, seed=seed, return_attempts=True)[1] == 2).any()


# ---------------------------------------------------------------------------------------------------------------- rules
def test_ucb_plays_the_unpulled_arms_first_in_index_order():
    K = 6
    u = BanditLearner.ucb(K, np.array([2.0], F))
    st = BanditLearnerState.zeros(1, K)
    for k in range(K):
        a, scores = u.reference(np.zeros(1, int), st, return_scores=True)
        assert a[0] == k and np.isinf(scores[0, k:]).all() and not scores[0, :k].any()
        st.pulls[0, a[0]] += 1
        st.wins[0, a[0]] += k % 2
    a, scores = u.reference(np.zeros(1, int), st, return_scores=True)
    assert np.isfinite(scores).all() and a[0] == 1                           # all pulled once: the first arm with a win
    st.pulls[0, 2] = 0
    assert u.reference(np.zeros(1, int), st)[0] == 2


def test_ties_go_to_the_lowest_index():
    for kind in ("greedy", "ucb", "table"):
        learner = blh.make_learner(kind, 4, 1)
        st = BanditLearnerState(np.full((1, 4), 3, np.int32), np.full((1, 4), 1, np.int32))
        a, scores = learner.reference(np.zeros(1, int), st, return_scores=True)
        assert len(set(scores[0].tolist())) == 1 and a[0] == 0, kind
        st.wins[0, 2:] = 2
        assert learner.reference(np.zeros(1, int), st)[0] == 2, kind


def test_table_saturation_against_the_integer_formula():
    C = 3
    cells = (C + 1) * (C + 2) // 2
    index = np.arange(cells, dtype=F)[None, :] + F(0.5)                      # a cell's score names the cell
    learner = BanditLearner.table(2, index)
    assert learner.table_cap == C
    for n in range(11):
        for w in range(n + 1):
            st = BanditLearnerState(np.array([[n, 0]], np.int32), np.array([[w, 0]], np.int32))
            _, scores = learner.reference(np.zeros(1, int), st, return_scores=True)
            cell = n * (n + 1) // 2 + w if n <= C else C * (C + 1) // 2 + (w * C) // n
            assert scores[0, 0] == cell + 0.5 and scores[0, 1] == 0.5, (n, w)
    for bad in (2, 4, 7, cells + 1):
        with pytest.raises(ValueError):
            BanditLearner.table(2, np.zeros((1, bad), F))
    assert BanditLearner.table(2, np.zeros((1, 3), F)).table_cap == 1
    assert BanditLearner.table(2, np.zeros((1, 1024 * 1025 // 2), F)).table_cap == 1023
    with pytest.raises(ValueError):
        BanditLearner.table(2, np.zeros((1, 1025 * 1026 // 2), F))


def test_greedy_prior_and_epsilon_is_the_policys_draw():
    K, N = 10, 512
    g = BanditLearner.greedy(K, np.array([[1.0, 1.0], [2.0, 6.0]], F))
    st = BanditLearnerState.zeros(2, K)
    _, scores = g.reference(np.arange(2), st, return_scores=True)
    assert (scores[0] == 0.5).all() and (scores[1] == 0.25).all()
    st.pulls[:, 3], st.wins[:, 3] = 2, 2
    a, scores = g.reference(np.arange(2), st, return_scores=True)
    assert scores[0, 3] == F(3) / F(4) and scores[1, 3] == F(4) / F(10) and a.tolist() == [3, 3]
    # epsilon: the same (e, n, seed) explore, and to the same arm, as a BanditPolicy with the same epsilon
    eps = np.array([0.3, 0.0, 1.0])
    learner = BanditLearner.greedy(K, np.ones((3, 2), F), eps)
    z = lambda *s: np.zeros(s, F)
    pol = BanditPolicy(z(3, 1, K), z(3, 1), z(3, 1), z(3, 1, 1), z(3, 1), z(3, K, 1), z(3, K), eps)
    ids = np.arange(N) % 3
    step, seed = (2 << 32) | 5, (9 << 32) | 1
    ps = BanditPolicyState.zeros(N, 1)
    ps.step = step
    pa, _, explored = pol.reference(ids, ps, seed=seed, return_explored=True)
    ls = BanditLearnerState.zeros(N, K)
    ls.step = step
    la = learner.reference(ids, ls, seed=seed)
    assert np.array_equal(la, pa) and explored[ids == 2].all() and not explored[ids == 1].any()   # both are greedy at arm 0
    assert 0 < explored[ids == 0].sum() < (ids == 0).sum() and len(set(la.tolist())) == K
    assert np.array_equal(learner.thresholds, pol.thresholds)
    with pytest.raises(ValueError):
        BanditLearner("thompson", K, np.ones((1, 4), F), epsilon=np.array([0.1]))


def test_constructor_refusals():
    one = np.ones((1, 2), F)
    for bad in (np.zeros((1, 2), F), np.array([[1.0, -1.0]], F), np.ones((1, 3), F), np.ones(2, F), np.array([[np.inf, 1]], F)):
        with pytest.raises(ValueError):
            BanditLearner.greedy(5, bad)
    with pytest.raises(TypeError):
        BanditLearner.greedy(5, np.ones((1, 2)))
    for bad in (np.array([[0.5, 1.0]], F), np.array([[1.0, 0.99]], F)):
        with pytest.raises(ValueError):
            BanditLearner.thompson(5, bad)
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError):
            BanditLearner.thompson(5, one, max_attempts=bad)
    for arms in (1, 65):
        with pytest.raises(ValueError):
            BanditLearner.greedy(arms, one)
    with pytest.raises(ValueError):
        BanditLearner.ucb(5, np.array([-1.0], F))
    with pytest.raises(TypeError):
        BanditLearner.ucb(5, np.array([2.0], F), epsilon=np.array([0.1], F))
    for eps in (np.zeros(2), np.array([1.5]), np.array([np.nan])):
        with pytest.raises(ValueError):
            BanditLearner.ucb(5, np.array([2.0], F), epsilon=eps)
    g = BanditLearner.greedy(5, one)
    with pytest.raises(ValueError):
        g.reference(np.ones(3, int), BanditLearnerState.zeros(3, 5))          # id out of range
    with pytest.raises(ValueError):
        g.reference(np.zeros(3, int), BanditLearnerState.zeros(3, 4))         # another K
    bad = BanditLearnerState.zeros(3, 5)
    bad.wins[1, 1] = 1
    with pytest.raises(ValueError):
        g.reference(np.zeros(3, int), bad)                                    # wins > pulls
    with pytest.raises(ValueError):
        bad.validate()


# -------------------------------------------------------------------------------------------------------------- Gittins
def _gittins_by_bisection(n0, s0, discount, depth, tol):
    """An independent route to one cell: bisection on lam over a DP of its own, cut `depth` pulls below the cell with the
    value max(retire, pull for ever). Error: tol from the bisection plus discount^depth / (1 - discount) from the cut."""
    def advantage(lam):
        M = lam / (1.0 - discount)
        top = n0 + depth
        V = [max(M, ((s + 1.0) / (top + 2.0)) / (1.0 - discount)) for s in range(s0, s0 + depth + 1)]
        for n in range(top - 1, n0 - 1, -1):
            nxt = []
            for j, s in enumerate(range(s0, s0 + (n - n0) + 1)):
                p = (s + 1.0) / (n + 2.0)
                cont = p + discount * (p * V[j + 1] + (1.0 - p) * V[j])
                nxt.append(cont if n == n0 else max(M, cont))
            V = nxt
        return V[0] - M
    lo, hi = 0.0, 1.0
    while hi - lo > tol:
        mid = 0.5 * (lo + hi)
        if advantage(mid) > 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def test_gittins_table():
    cap, discount, depth, grid = 7, 0.8, 40, 400
    table = gittins_index_table(cap, discount, depth=depth, grid=grid)
    assert table.dtype == F and table.shape == ((cap + 1) * (cap + 2) // 2,)
    for n in range(cap + 1):
        row = table[n * (n + 1) // 2: n * (n + 1) // 2 + n + 1]
        mean = ((np.arange(n + 1) + 1.0) / (n + 2.0)).astype(F)
        assert (row >= mean).all() and (row < 1).all(), n                    # never below the posterior mean
        assert (np.diff(row) >= 0).all(), n                                  # non-decreasing in s
    bound = L.gittins_error_bound(discount, depth, grid)
    assert bound == 1.0 / grid + discount ** depth / (1 - discount)
    deep, tol = 60, 1e-6
    other_bound = tol + discount ** deep / (1 - discount)
    for n, s in ((0, 0), (2, 1), (2, 2), (7, 2)):
        want = _gittins_by_bisection(n, s, discount, deep, tol)
        got = float(table[n * (n + 1) // 2 + s])
        print("Gittins (%d, %d): table %.6f, bisection %.6f, bound %.2g" % (n, s, got, want, bound + other_bound))
        assert abs(got - want) <= bound + other_bound + 2.0 ** -24
        assert got > (s + 1.0) / (n + 2.0) + 1e-3                            # an index, not the mean
    # the default depth makes the cut's term no larger than the grid's
    assert np.abs(gittins_index_table(3, discount, grid=grid) - table[:10]).max() <= 2 * bound
    for bad in (dict(cap=0), dict(cap=1024), dict(discount=1.0), dict(discount=0.0), dict(grid=1), dict(depth=0)):
        kw = dict(cap=3, discount=0.9)
        kw.update(bad)
        with pytest.raises(ValueError):
            gittins_index_table(**kw)


# --------------------------------------------------------------------------------------------------- header and binding
def _header():
    text = open(os.path.join(ROOT, "include", "metagym_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_entry_points_are_declared_in_the_header_and_the_binding():
    from metagym_amd import _lib
    lib = _lib.load()
    text = _header()
    for name in ("mg_bandits_learner_rollout", "mg_bandits_learner_scores"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"#define\s+MG_ABI_VERSION\s+10\b", text) and _lib.ABI_VERSION == 10
    m = re.search(r"typedef struct mg_bandits_learner \{(.*?)\} mg_bandits_learner;", text, re.S)
    assert re.findall(r"(\w+)\s*;", m.group(1)) == [f[0] for f in _lib.BanditsLearnerDesc._fields_]
    assert [f[0] for f in _lib.BanditsLearnerDesc._fields_] == ["kind", "n_learners", "arms", "params", "eps_threshold", "table",
                                                                "table_cap", "max_attempts"]
    m = re.search(r"typedef struct mg_bandits_learner_carry \{(.*?)\} mg_bandits_learner_carry;", text, re.S)
    assert re.findall(r"(\w+)\s*;", m.group(1)) == [f[0] for f in _lib.BanditsLearnerCarry._fields_] == ["pulls", "wins"]
    for name, code in L.KINDS.items():
        assert re.search(r"#define\s+MG_BANDITS_LEARNER_%s\s+%d\b" % (name.upper(), code), text), name
    assert len(_lib.SIGNATURES["mg_bandits_learner_rollout"][1]) == 23 and len(_lib.SIGNATURES["mg_bandits_learner_scores"][1]) == 9
    from csrc_structure import assert_unit_sits_on_the_bandits_core
    assert_unit_sits_on_the_bandits_core("bandits_learner.hip")


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

    def desc(kind=0, n=3, k=10, params=base, thr=None, table=None, cap=0, attempts=64):
        return _lib.BanditsLearnerDesc(kind, n, k, params, thr, table, cap, attempts)
    carry = _lib.BanditsLearnerCarry(base, base)
    order = (("cfg", config()), ("n", 4), ("state", st), ("steps", 2), ("learner", desc()), ("ids", p), ("carry", carry),
             ("seed", 0), ("step0", 0), ("episodic", 1), ("ret_total", p), ("ret_episode", p), ("episode_len", p),
             ("episodes", p), ("regret", p), ("actions", None), ("reward", None), ("done", None), ("info_steps", None),
             ("expected_gain", None), ("best_gain", None), ("invalid", None), ("stream", None))
    rollout = lambda **kw: lib.mg_bandits_learner_rollout(*[kw.get(k, v) for k, v in order])
    sorder = (("n", 4), ("learner", desc()), ("ids", p), ("carry", carry), ("seed", 0), ("step0", 0), ("scores", p),
              ("attempts", None), ("stream", None))
    scores = lambda **kw: lib.mg_bandits_learner_scores(*[kw.get(k, v) for k, v in sorder])
    for name in ("cfg", "state", "learner", "ids", "carry", "ret_total", "ret_episode", "episode_len", "episodes", "regret"):
        assert rollout(**{name: None}) == -1001, name
        assert b"NULL" in lib.mg_last_error()
    for name in ("learner", "ids", "carry", "scores"):
        assert scores(**{name: None}) == -1001, name
    for k in range(6):
        ptrs = [base] * 6
        ptrs[k] = None
        assert rollout(state=_lib.BanditsState(*ptrs)) == -1001
    for call in (rollout, scores):
        assert call(learner=desc(params=None)) == -1001
        assert call(carry=_lib.BanditsLearnerCarry(None, base)) == -1001 and call(carry=_lib.BanditsLearnerCarry(base, None)) == -1001
        assert call(n=0) == -1002 and call(n=-1) == -1002
        assert call(learner=desc(n=0)) == -1002 and b"n_learners" in lib.mg_last_error()
        assert call(learner=desc(k=1)) == -1002 and b"arms" in lib.mg_last_error()
        assert call(learner=desc(kind=4)) == -1003 and call(learner=desc(kind=-1)) == -1003
        assert call(learner=desc(kind=2, cap=3)) == -1001                              # a table learner without a table
        for cap in (0, 1024, -1):
            assert call(learner=desc(kind=2, table=base, cap=cap)) == -1002 and b"table_cap" in lib.mg_last_error()
        for attempts in (0, 65, -1):
            assert call(learner=desc(kind=3, attempts=attempts)) == -1002 and b"max_attempts" in lib.mg_last_error()
        assert call(learner=desc(kind=3, thr=base)) == -1003 and b"Thompson" in lib.mg_last_error()
    assert scores(learner=desc(k=65)) == -1002
    assert rollout(steps=0) == -1002 and rollout(steps=-2) == -1002
    assert rollout(cfg=config(arms=65), learner=desc(k=65)) == -1002
    assert rollout(learner=desc(k=9)) == -1003 and b"arms" in lib.mg_last_error()      # not the env's K
    assert rollout(cfg=config(arms=100)) == -1003
    assert rollout(cfg=config(max_steps=1)) == -1003 and b"max_steps" in lib.mg_last_error()
    assert rollout(cfg=config(distribution=4)) == -1003


def test_the_env_has_the_methods_and_the_package_exports_the_classes():
    import inspect
    import metagym_amd.bandits as mb
    assert {"BanditLearner", "BanditLearnerState", "BanditsLearnerRollout", "gittins_index_table", "log32"} <= set(mb.__all__)
    sig = inspect.signature(mb.Bandits.rollout_learner)
    assert list(sig.parameters) == ["self", "learner", "steps", "learner_ids", "state", "seed", "record", "episodic"]
    assert [sig.parameters[k].default for k in ("learner_ids", "state", "seed", "record", "episodic")] == [None, None, 0, False, True]
    sig = inspect.signature(mb.Bandits.learner_scores)
    assert list(sig.parameters)[:5] == ["self", "learner", "state", "learner_ids", "seed"]
    sig = inspect.signature(mb.BanditLearner.reference)
    assert list(sig.parameters) == ["self", "learner_ids", "state", "seed", "env_ids", "return_scores", "return_attempts"]
    st = mb.BanditLearnerState.zeros(3, 4)
    assert st.pulls.shape == (3, 4) and st.pulls.dtype == np.int32 and not st.wins.any() and st.step == 0
    assert mb.BanditsLearnerRollout.__slots__ == mb.BanditsPolicyRollout.__slots__


# ---------------------------------------------------------------------------------------------------------- closed loop
@pytest.mark.parametrize("kind", blh.KINDS)
def test_reference_closed_loop_splits_exactly(kind):
    """`reference` + the reference's env for T1 and then T2 steps through one state equal T1 + T2 steps in one go; the done
    with a task redraw falls inside (max_steps = 7)."""
    N, K, M, T1, T2 = 9, 4, 7, 5, 11
    learner = blh.make_learner(kind, K, 3, epsilon=None if kind == "thompson" else np.array([0.2, 0.0, 0.5]))
    ids = np.arange(N) % 3
    seeds = 50 + 3 * np.arange(N)

    def fresh():
        host = blh.Host(seeds, K, M, "Uniform")
        host.over[:] = 0
        return host
    st0 = BanditLearnerState.zeros(N, K)
    st0.step = (1 << 32) - 3
    whole_host = fresh()
    rec, out, carry = blh.host_rollout(learner, ids, whole_host, st0, T1 + T2, True, True, seed=4)
    assert not st0.pulls.any() and st0.step == (1 << 32) - 3                 # the state handed in was only read
    host = fresh()
    rec_a, out_a, carry_a = blh.host_rollout(learner, ids, host, st0, T1, True, True, seed=4)
    rec_b, out_b, carry_b = blh.host_rollout(learner, ids, host, carry_a, T2, True, True, seed=4)
    for name in rec:
        assert np.array_equal(np.concatenate([rec_a[name], rec_b[name]]), rec[name]), name
    assert np.array_equal(carry_b.pulls, carry.pulls) and np.array_equal(carry_b.wins, carry.wins)
    assert carry_a.step == st0.step + T1 and carry_b.step == carry.step == st0.step + T1 + T2
    assert np.array_equal(host.gains, whole_host.gains) and np.array_equal(host.steps, whole_host.steps)
    assert np.array_equal(out_a["episodes"] + out_b["episodes"], out["episodes"]) and (out["episodes"] == 2).all()
    assert np.array_equal(out_a["ret_total"] + out_b["ret_total"], out["ret_total"])
    # episodic: the counts are those of the running episode alone (16 steps = two episodes of 7 and 2 steps)
    assert (carry.pulls.sum(1) == (T1 + T2) % M).all() and (carry.wins <= carry.pulls).all()
    keep = blh.host_rollout(learner, ids, fresh(), st0, T1 + T2, True, True, seed=4, episodic=False)[2]
    assert (keep.pulls.sum(1) == T1 + T2).all()
    assert len(set(rec["actions"].ravel().tolist())) >= 2
