"""Classical bandit learners for `Bandits.rollout_learner`: greedy on a Beta prior, UCB, an index table (Gittins) and Thompson
sampling, evaluated inside the rollout launch (include/metagym_hip.h, mg_bandits_learner_rollout). They are the baselines a
learned bandit policy is reported against (RL^2, SNAIL).

The arithmetic is defined exactly, in float32 operations that are rounded once and never fused, plus integers, so
`BanditLearner.reference` in numpy reproduces every action bit for bit. K arms (2 <= K <= 64); a learner object has one kind
and P parameter rows, env e uses row learner_ids[e]. Its memory is two counts per arm, n = pulls[k] and w = wins[k]. Every
kind computes K scores and plays the lowest index among the maxima (best = score[0]; for k >= 1: if score[k] > best). With
(float) the conversion int32 -> float32, and `/` and sqrt the correctly rounded float32 operations:

    greedy     a0, b0 > 0:  score = ((float)w + a0) / (((float)n + a0) + b0)
    ucb        c >= 0 (UCB1 is c = 2). An arm with n = 0: the lowest such arm is played (as scores: +inf for the unpulled
               arms, 0 for the others). Otherwise t = the int64 sum of the pulls, converted to float32, and
               score = (float)w / (float)n + sqrt((c * log32(t)) / (float)n)
    table      an index read from a caller's float32 table [P, (C + 1)(C + 2) / 2], 1 <= C <= 1023; the cell of (n, s) with
               0 <= s <= n <= C is n (n + 1) / 2 + s. n <= C: score = cell (n, w); otherwise cell (C, floor(w C / n)), in
               64-bit integers. `gittins_index_table` makes the table of the Gittins index.
    thompson   a0, b0 >= 1:  alpha = (float)w + a0, beta = (float)(n - w) + b0, X = gamma(alpha; which = 0),
               Y = gamma(beta; which = 1), score = X / (X + Y)

Exploration (`epsilon`, all kinds but Thompson) is `BanditPolicy`'s rule as it stands: the threshold, the tag 0x4241 and
out[1] % K are those of bandits/policy.py (the threshold rule itself lives in _policy.py), not restated.

log32(x), for positive normal x, is fdlibm's single-precision log, one operation at a time. With i the bits of x:

    i += 0x3f800000 - 0x3f3504f3;  k = (i >> 23) - 127;  m = the float with bits (i & 0x007fffff) + 0x3f3504f3
    f = m - 1;  s = f / (2 + f);  z = s*s;  w = z*z;  t1 = w * (Lg2 + w*Lg4);  t2 = z * (Lg1 + w*Lg3);  R = t2 + t1
    hfsq = (0.5*f)*f;  dk = (float)k;  result = (((s*(hfsq + R) + dk*ln2_lo) - hfsq) + f) + dk*ln2_hi

gamma(a; which) for env e, arm k at carry step n is Marsaglia-Tsang with a polar normal:

    d = a - 0.33333334f;  c = 1 / sqrt(9*d);  u01(word) = (float)(((word >> 9) << 1) | 1) * 2^-24   (exact, never 0 or 1)
    attempt i = 0 .. max_attempts - 1:
        o = philox4x32_10(c0 = e, c1 = n lo, c2 = n hi, c3 = 0x4C000000 | k << 17 | which << 16 | i, key = seed)
        v1 = 2*u01(o[0]) - 1;  v2 = 2*u01(o[1]) - 1;  s = v1*v1 + v2*v2;  if s >= 1: next attempt
        x = v1 * sqrt((-2*log32(s)) / s);  v = 1 + c*x;  if v <= 0: next attempt
        v3 = (v*v)*v;  accept if log32(u01(o[2])) < (((0.5*x)*x + d) - d*v3) + d*log32(v3): the result is d*v3
    all attempts exhausted: the result is d

Nothing here needs a GPU to import.

    ts = BanditLearner.thompson(10, np.ones((1, 2), np.float32))
    res = env.rollout_learner(ts, steps=256)                      # res.regret is the per-env regret
    res = env.rollout_learner(ts, steps=256, state=res.state)     # and goes on, counts kept
"""
import numpy as np

from .._policy import (LG1, LG2, LG3, LG4, LN2_HI, LN2_LO, PackedPolicySet, check_epsilon, f32_array, log32,  # noqa: F401
                       philox4x32_10, to_numpy, u01)
from .policy import MAX_ARMS, PHILOX_TAG, BanditsPolicyRollout

F = np.float32
KINDS = {"greedy": 0, "ucb": 1, "table": 2, "thompson": 3}       # MG_BANDITS_LEARNER_*
MAX_CAP = 1023
MAX_ATTEMPTS = 64
GAMMA_TAG = 0x4C000000       # c3 of a sampler draw: tag | arm << 17 | which << 16 | attempt

BanditsLearnerRollout = BanditsPolicyRollout   # the same fields; .state is a BanditLearnerState


def table_cells(cap):
    """Cells of one table row: (C + 1)(C + 2) / 2."""
    return (int(cap) + 1) * (int(cap) + 2) // 2


def gamma32(a, e, n, arm, which, seed, max_attempts=MAX_ATTEMPTS):
    """gamma(a; which) of the module docstring, elementwise: a float32, e (env), arm integers of a's shape (or broadcast to
    it), n the carry step, `which` 0 or 1. Returns (value float32, attempts int32: the attempts made, max_attempts + 1 where
    the fallback d was taken)."""
    a = np.asarray(a)
    if a.dtype != F:
        raise TypeError("gamma32 takes float32, got %s" % a.dtype)
    shape = a.shape
    e = np.broadcast_to(np.asarray(e, np.uint64), shape).reshape(-1)
    arm = np.broadcast_to(np.asarray(arm, np.uint64), shape).reshape(-1)
    a = a.reshape(-1)
    n, seed, which = int(n), int(seed), int(which)
    one, two, half = F(1.0), F(2.0), F(0.5)
    with np.errstate(all="ignore"):
        d = a - F(0.33333334)
        c = one / np.sqrt(F(9.0) * d)
    value = d.copy()
    tries = np.full(a.shape, int(max_attempts) + 1, np.int32)
    pend = np.arange(a.size)
    for i in range(int(max_attempts)):
        if pend.size == 0:
            break
        c3 = np.uint64(GAMMA_TAG | which << 16 | i) | (arm[pend] << np.uint64(17))
        o = philox4x32_10(e[pend], n & 0xFFFFFFFF, (n >> 32) & 0xFFFFFFFF, c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        dp, cp = d[pend], c[pend]
        with np.errstate(all="ignore"):
            v1 = two * u01(o[0]) - one
            v2 = two * u01(o[1]) - one
            s = v1 * v1 + v2 * v2
            ok = ~(s >= one)
            x = v1 * np.sqrt((F(-2.0) * log32(s)) / s)
            v = one + cp * x
            ok &= ~(v <= F(0.0))
            v3 = (v * v) * v
            v3s = np.where(ok, v3, one)                        # the rejected lanes compute nothing that is used
            ok &= log32(u01(o[2])) < (((half * x) * x + dp) - dp * v3) + dp * log32(v3s)
            res = dp * v3
        assert res.dtype == F
        value[pend[ok]] = res[ok]
        tries[pend[ok]] = i + 1
        pend = pend[~ok]
    return value.reshape(shape), tries.reshape(shape)


class BanditLearnerState(object):
    """The carry of `Bandits.rollout_learner`, the learner's memory of each env: pulls int32 [N, K], wins int32 [N, K]
    (0 <= wins <= pulls) and `step`, the Python int n of the Philox step counter, which advances by `steps` per call as in
    `BanditPolicyState`. The arrays are torch tensors on the env's device (or numpy arrays, for `reference`)."""
    __slots__ = ("pulls", "wins", "step")

    def __init__(self, pulls, wins, step=0):
        self.pulls, self.wins, self.step = pulls, wins, int(step)

    @classmethod
    def zeros(cls, num_envs, arms, device=None):
        """The fresh carry: no pulls, step = 0. device None: numpy arrays."""
        N, K = int(num_envs), int(arms)
        if device is None:
            return cls(np.zeros((N, K), np.int32), np.zeros((N, K), np.int32))
        import torch
        return cls(torch.zeros(N, K, dtype=torch.int32, device=device), torch.zeros(N, K, dtype=torch.int32, device=device))

    @property
    def num_envs(self):
        return int(self.pulls.shape[0])

    @property
    def arms(self):
        return int(self.pulls.shape[1])

    def clone(self):
        c = (lambda v: v.clone()) if hasattr(self.pulls, "clone") else (lambda v: v.copy())
        return BanditLearnerState(c(self.pulls), c(self.wins), self.step)

    def numpy(self):
        """The same carry on the host, as numpy arrays."""
        return BanditLearnerState(to_numpy(self.pulls).astype(np.int32), to_numpy(self.wins).astype(np.int32), self.step)

    def validate(self):
        """Raises unless 0 <= wins <= pulls everywhere (reads the arrays back: not for a captured region)."""
        p, w = to_numpy(self.pulls), to_numpy(self.wins)
        if p.shape != w.shape or p.ndim != 2 or not ((w >= 0) & (w <= p)).all():
            raise ValueError("a BanditLearnerState needs pulls and wins of one shape [N, K] with 0 <= wins <= pulls")
        return self


class BanditLearner(PackedPolicySet):
    """P parameter rows of one kind of classical learner for K arms; build one with `greedy`, `ucb`, `table` or `thompson`."""

    def __init__(self, kind, arms, params, epsilon=None, table=None, table_cap=0, max_attempts=MAX_ATTEMPTS):
        if kind not in KINDS:
            raise ValueError("kind must be one of %s, got %r" % (sorted(KINDS), kind))
        K = int(arms)
        if not (2 <= K <= MAX_ARMS):
            raise ValueError("arms must be in [2, %d], got %r" % (MAX_ARMS, arms))
        P = params.shape[0]
        if P < 1:
            raise ValueError("a learner needs at least one parameter row")
        if epsilon is not None:
            if kind == "thompson":
                raise ValueError("Thompson sampling takes no epsilon")
            epsilon = check_epsilon(epsilon, P)
        self.kind, self.arms, self.num_learners = kind, K, P
        self.params, self.epsilon, self.index, self.table_cap = params, epsilon, table, int(table_cap)
        self.max_attempts = int(max_attempts)

    # ------------------------------------------------------------------ the four kinds
    @staticmethod
    def _rows(values, width):
        rows = np.zeros((values[0].shape[0], 4), F)
        for j, v in enumerate(values):
            rows[:, width[j]] = v
        return rows

    @classmethod
    def greedy(cls, arms, prior, epsilon=None):
        """score = posterior mean under the prior Beta(a0, b0): prior float32 [P, 2], both > 0."""
        prior = f32_array("prior", prior, 2)
        if prior.shape[1] != 2 or not (prior > 0).all():
            raise ValueError("prior must be [P, 2] with a0, b0 > 0")
        return cls("greedy", arms, cls._rows([prior[:, 0], prior[:, 1]], [0, 1]), epsilon)

    @classmethod
    def ucb(cls, arms, c, epsilon=None):
        """score = mean + sqrt(c log(t) / n), every arm once first: c float32 [P], >= 0 (UCB1 is c = 2)."""
        c = f32_array("c", c, 1)
        if not (c >= 0).all():
            raise ValueError("c must be >= 0")
        return cls("ucb", arms, cls._rows([c], [2]), epsilon)

    @classmethod
    def table(cls, arms, index, epsilon=None):
        """score = index[cell of (n, w)]: index float32 [P, (C + 1)(C + 2) / 2] with 1 <= C <= 1023 (C is found from the
        row length)."""
        index = f32_array("index", index, 2)
        cells = index.shape[1]
        cap = int((np.sqrt(8.0 * cells + 1.0) - 3.0) / 2.0 + 0.5)
        if cap < 1 or cap > MAX_CAP or table_cells(cap) != cells:
            raise ValueError("index rows must hold (C + 1)(C + 2) / 2 cells with 1 <= C <= %d, got %d" % (MAX_CAP, cells))
        return cls("table", arms, np.zeros((index.shape[0], 4), F), epsilon, table=index, table_cap=cap)

    @classmethod
    def thompson(cls, arms, prior, max_attempts=MAX_ATTEMPTS):
        """score = a draw from the posterior Beta(a0 + w, b0 + n - w): prior float32 [P, 2], both >= 1."""
        prior = f32_array("prior", prior, 2)
        if prior.shape[1] != 2 or not (prior >= 1).all():
            raise ValueError("prior must be [P, 2] with a0, b0 >= 1")
        if int(max_attempts) != max_attempts or not (1 <= int(max_attempts) <= MAX_ATTEMPTS):
            raise ValueError("max_attempts must be in [1, %d], got %r" % (MAX_ATTEMPTS, max_attempts))
        return cls("thompson", arms, cls._rows([prior[:, 0], prior[:, 1]], [0, 1]), None, max_attempts=max_attempts)

    def __len__(self):
        return self.num_learners

    def _host(self):
        """`to(device)` gives (params [P, 4], thresholds or None, table or None); the thresholds travel as the int32 tensor
        with the uint32's bits."""
        return self.params, self._threshold_bits(), self.index

    # ------------------------------------------------------------------ the definition in numpy
    def reference(self, learner_ids, state, seed=0, env_ids=None, return_scores=False, return_attempts=False):
        """One step of the definition in numpy float32 and numpy integers. learner_ids [N]; state: a `BanditLearnerState`
        (pulls, wins and step are read; nothing is written); env e draws with counter c0 = env_ids[e] (default e). Returns
        the actions int32 [N]; with `return_scores` also the scores float32 [N, K]; with `return_attempts` also int32
        [N, K, 2], the attempts of gamma(.; which) (zeros unless Thompson). The caller applies the count update."""
        P, K = self.num_learners, self.arms
        ids = to_numpy(learner_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("learner_ids must be a vector of integers")
        N = ids.shape[0]
        if N and (int(ids.min()) < 0 or int(ids.max()) >= P):
            raise ValueError("learner_ids must be in [0, %d)" % P)
        pulls, wins = to_numpy(state.pulls), to_numpy(state.wins)
        if pulls.shape != (N, K) or wins.shape != (N, K) or pulls.dtype != np.int32 or wins.dtype != np.int32:
            raise ValueError("state.pulls and state.wins must be int32 [%d, %d]" % (N, K))
        if not ((wins >= 0) & (wins <= pulls)).all():
            raise ValueError("the counts must satisfy 0 <= wins <= pulls")
        e = np.arange(N, dtype=np.uint64) if env_ids is None else to_numpy(env_ids).astype(np.uint64)
        n, s = int(state.step), int(seed)
        a0, b0, c = (self.params[ids, j][:, None] for j in range(3))
        nf, wf = pulls.astype(F), wins.astype(F)
        attempts = np.zeros((N, K, 2), np.int32)
        with np.errstate(all="ignore"):
            if self.kind == "greedy":
                scores = (wf + a0) / ((nf + a0) + b0)
            elif self.kind == "ucb":
                unpulled = pulls == 0
                fresh = unpulled.any(axis=1)
                t = pulls.astype(np.int64).sum(axis=1).astype(F)[:, None]
                t = np.where(fresh[:, None], F(2.0), t)                    # (those rows are replaced below)
                nz = np.where(unpulled, F(1.0), nf)
                scores = wf / nz + np.sqrt((c * log32(t)) / nz)
                scores = np.where(fresh[:, None], np.where(unpulled, F(np.inf), F(0.0)), scores).astype(F)
            elif self.kind == "table":
                C = self.table_cap
                n64, w64 = pulls.astype(np.int64), wins.astype(np.int64)
                inside = n64 <= C
                cell = np.where(inside, n64 * (n64 + 1) // 2 + w64, C * (C + 1) // 2 + (w64 * C) // np.maximum(n64, 1))
                scores = self.index[ids[:, None], cell]
            else:
                arm = np.broadcast_to(np.arange(K, dtype=np.uint64)[None, :], (N, K))
                env = np.broadcast_to(e[:, None], (N, K))
                X, attempts[:, :, 0] = gamma32(wf + a0, env, n, arm, 0, s, self.max_attempts)
                Y, attempts[:, :, 1] = gamma32((pulls - wins).astype(F) + b0, env, n, arm, 1, s, self.max_attempts)
                scores = X / (X + Y)
        assert scores.dtype == F and scores.shape == (N, K)
        actions = np.zeros(N, np.int32)
        best = scores[:, 0].copy()
        for k in range(1, K):
            better = scores[:, k] > best
            actions = np.where(better, np.int32(k), actions)
            best = np.where(better, scores[:, k], best)
        if self.epsilon is not None:
            thr = self.thresholds[ids]
            out = philox4x32_10(e, n & 0xFFFFFFFF, (n >> 32) & 0xFFFFFFFF, PHILOX_TAG, s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF)
            actions = np.where(out[0] < thr, (out[1] % np.uint32(K)).astype(np.int32), actions)
        res = (actions.astype(np.int32),)
        if return_scores:
            res += (scores,)
        if return_attempts:
            res += (attempts,)
        return res[0] if len(res) == 1 else res


def gittins_error_bound(discount, depth, grid):
    """The bound on |table - Gittins index| that `gittins_index_table(cap, discount, depth, grid)` documents (before the
    rounding to float32): 1 / grid + discount^depth / (1 - discount)."""
    return 1.0 / int(grid) + float(discount) ** int(depth) / (1.0 - float(discount))


def gittins_index_table(cap, discount, depth=None, grid=2000):
    """The Gittins index (in reward-per-step units, so in (0, 1)) of a Bernoulli arm with posterior Beta(1 + s, 1 + n - s)
    under `discount`, for every cell 0 <= s <= n <= cap, as the float32 [(cap + 1)(cap + 2) / 2] row `BanditLearner.table`
    takes (cell n (n + 1) / 2 + s). Host numpy, float64.

    Method: calibration against a retirement value. For a safe arm paying lam per step, M = lam / (1 - discount), the value
    of the state is V(n, s) = max(M, p + discount (p V(n + 1, s + 1) + (1 - p) V(n + 1, s))) with p = (s + 1) / (n + 2); the
    index is the lam at which the two branches are equal. The recursion is cut at the level n = cap + depth, where
    V = max(M, p / (1 - discount)) (retire or pull that arm for ever), and run for the grid lam = j / grid, j = 0..grid, all
    at once; the index is the root of the chord through the two neighbouring grid points between which
    continue - retire changes its sign.

    Error bound. The cut-off value errs by at most 1 / (1 - discount) and sits at least `depth` pulls below every cell, so
    continue(M) errs by at most discount^depth / (1 - discount); continue(M) - M has a slope of at most discount - 1 in M
    (a continuing arm retires one pull later at the earliest), so the root in M moves by at most that over (1 - discount)
    and the root in lam = (1 - discount) M by at most discount^depth / (1 - discount). The chord's root lies in the same
    grid interval as the true root: at most 1 / grid away. Together |table - index| <= 1 / grid + discount^depth /
    (1 - discount) (`gittins_error_bound`), plus half a float32 ulp. depth=None takes the smallest depth for which the
    second term is below 1 / grid. The index is never below the posterior mean p, and the table keeps that."""
    C, g, G = int(cap), float(discount), int(grid)
    if not (1 <= C <= MAX_CAP):
        raise ValueError("cap must be in [1, %d], got %r" % (MAX_CAP, cap))
    if not (0.0 < g < 1.0):
        raise ValueError("discount must be in (0, 1), got %r" % (discount,))
    if G < 2:
        raise ValueError("grid must be at least 2, got %r" % (grid,))
    if depth is None:
        depth = int(np.ceil(np.log((1.0 - g) / G) / np.log(g)))
    D = int(depth)
    if D < 1:
        raise ValueError("depth must be at least 1, got %r" % (depth,))
    lam = np.arange(G + 1, dtype=np.float64) / G
    M = lam / (1.0 - g)                                                   # [G + 1]
    top = C + D
    p = (np.arange(top + 1) + 1.0) / (top + 2.0)
    V = np.maximum(M[None, :], p[:, None] / (1.0 - g))                     # level `top`: [top + 1, G + 1]
    out = np.zeros(table_cells(C), np.float64)
    for n in range(top - 1, -1, -1):
        p = ((np.arange(n + 1) + 1.0) / (n + 2.0))[:, None]
        cont = p + g * (p * V[1:n + 2] + (1.0 - p) * V[:n + 1])
        if n <= C:
            diff = cont - M[None, :]                                       # decreasing in lam: > 0 at lam = 0, < 0 at lam = 1
            j = np.argmax(diff < 0.0, axis=1)                              # the first grid point where retiring wins
            rows = np.arange(n + 1)
            hi, lo = diff[rows, j], diff[rows, j - 1]
            root = (lam[j - 1] * (-hi) + lam[j] * lo) / (lo - hi)
            out[n * (n + 1) // 2: n * (n + 1) // 2 + n + 1] = np.maximum(root, p[:, 0])
        V = np.maximum(M[None, :], cont)
    return out.astype(F)
