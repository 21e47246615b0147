"""Host restatements of the MetaLM sequence generator (reference metagym/metalm/metalm.py), in two forms.

* `draw_level_row` / `draw_level_batch` work on raw 32-bit MT19937 outputs (`MTStream`) and spell out every draw the reference
  makes: this is the accounting metagym_amd/csrc/metalm.hip implements, written as plainly as possible.
* `fast_row` / `fast_batch` drive a private `numpy.random.RandomState` through NumPy's own `poisson`, `randint` and `random`:
  fast enough for thousands of rows, and independent of the draw-level form.

Both are pinned by tests/golden/metalm.npz (recorded from the unmodified reference); the device kernel is then compared with
them. Everything here is exact integer equality.
"""
import math

import numpy as np

MASK_RATIO = 0.30
_N, _M = 624, 397


class MTStream(object):
    """NumPy's legacy MT19937 (`RandomState`): 624-word key, read position `pos` (624 = regenerate before the next draw)."""

    def __init__(self, key, pos):
        self.key = np.array(key, dtype=np.uint32)
        assert self.key.shape == (_N,)
        self.pos = int(pos)
        self.phase = None        # set by draw_level_row: which part of the row is drawing
        self.refills = []        # the phase of every refill, "<phase>/straddle" where a double's two draws span it

    @classmethod
    def seeded(cls, seed):
        """numpy.random.seed(seed) for an integer seed < 2^32: init_genrand."""
        key = np.empty(_N, np.uint32)
        p = int(seed) & 0xFFFFFFFF
        key[0] = p
        for i in range(1, _N):
            p = (1812433253 * (p ^ (p >> 30)) + i) & 0xFFFFFFFF
            key[i] = p
        return cls(key, _N)

    @classmethod
    def from_numpy_state(cls, st):
        assert st[0] == "MT19937"
        return cls(st[1], st[2])

    def regenerate(self):
        """The refill in three segments, each independent inside itself: [0,227) reads only old words, [227,454) reads
        the new words of the first segment at i-227, [454,624) the new words of the second (and word 623 the new word 0)."""
        k = self.key.astype(np.uint64)
        new = k.copy()
        for lo, hi in ((0, _N - _M), (_N - _M, 2 * (_N - _M)), (2 * (_N - _M), _N)):
            i = np.arange(lo, hi)
            nxt = np.where(i + 1 < _N, k[(i + 1) % _N], new[0])
            y = (k[i] & np.uint64(0x80000000)) | (nxt & np.uint64(0x7FFFFFFF))
            src = np.where(i + _M < _N, k[(i + _M) % _N], new[(i + _M - _N) % _N])
            new[i] = src ^ (y >> np.uint64(1)) ^ np.where(y & np.uint64(1), np.uint64(0x9908B0DF), np.uint64(0))
        self.key = new.astype(np.uint32)
        self.pos = 0
        self.refills.append(self.phase)

    def next_u32(self):
        if self.pos >= _N:
            self.regenerate()
        y = int(self.key[self.pos])
        self.pos += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y

    def next_double(self):
        if self.pos == _N - 1:
            phase, self.phase = self.phase, "%s/straddle" % self.phase
            a = self.next_u32() >> 5
            b = self.next_u32() >> 6
            self.phase = phase
            return (a * 67108864.0 + b) / 9007199254740992.0
        a, b = self.next_u32() >> 5, self.next_u32() >> 6
        return (a * 67108864.0 + b) / 9007199254740992.0

    def bounded(self, r):
        """Masked rejection on 32-bit draws: 0..r inclusive. r == 0 consumes nothing."""
        if r == 0:
            return 0
        mask = r
        for s in (1, 2, 4, 8, 16):
            mask |= mask >> s
        while True:
            d = self.next_u32() & mask
            if d <= r:
                return d

    def numpy_state(self):
        return ("MT19937", self.key.copy(), self.pos)


def _loggam(x):
    """NumPy's random_loggam (a Stirling series after shifting x up to >= 7)."""
    a = (8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04,
         8.417508417508418e-04, -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02,
         1.796443723688307e-01, -1.39243221690590e+00)
    if x == 1.0 or x == 2.0:
        return 0.0
    n = int(7 - x) if x < 7.0 else 0
    x0 = x + n
    x2 = (1.0 / x0) * (1.0 / x0)
    gl0 = a[9]
    for k in range(8, -1, -1):
        gl0 *= x2
        gl0 += a[k]
    gl = gl0 / x0 + 0.5 * 1.8378770664093453e+00 + (x0 - 0.5) * math.log(x0) - x0      # 0.5 * log(2 pi)
    if x < 7.0:
        for _ in range(n):
            gl -= math.log(x0 - 1.0)
            x0 -= 1.0
    return gl


def poisson(g, lam):
    """NumPy's legacy Poisson: PTRS (transformed rejection) for lam >= 10, multiplication below."""
    if lam >= 10:
        slam, loglam = math.sqrt(lam), math.log(lam)
        b = 0.931 + 2.53 * slam
        a = -0.059 + 0.02483 * b
        invalpha = 1.1239 + 1.1328 / (b - 3.4)
        vr = 0.9277 - 3.6224 / (b - 2)
        while True:
            U = g.next_double() - 0.5
            V = g.next_double()
            us = 0.5 - abs(U)
            k = int(math.floor((2 * a / us + b) * U + lam + 0.43))
            if us >= 0.07 and V <= vr:
                return k
            if k < 0 or (us < 0.013 and V > us):
                continue
            lv = math.log(V) if V > 0 else -math.inf
            if lv + math.log(invalpha) - math.log(a / (us * us) + b) <= -lam + k * loglam - _loggam(k + 1):
                return k
    if lam == 0:
        return 0
    enlam, x, prod = math.exp(-lam), 0, 1.0
    while True:
        prod *= g.next_double()
        if prod > enlam:
            x += 1
        else:
            return x


def draw_level_row(g, V, n, l, e, L, mask_ratio=MASK_RATIO):
    """One data_generator() row from the raw stream `g` (advanced in place). Returns int32 (features[L], labels[L])."""
    elements = []
    for _ in range(n):                                   # elements_generator
        g.phase = "poisson"
        m = max(3, poisson(g, l))
        g.phase = "elements"
        elements.append([1 + g.bounded(V - 2) for _ in range(m)])
    feat, lab = [], []
    while len(feat) < L + 1:                             # cur_l == len(feat)
        g.phase = "choice"
        seq = elements[g.bounded(n - 2)]                 # randint(0, n-1): the last element is never picked
        m = len(seq)
        g.phase = "values"
        value = [1 + g.bounded(V - 2) for _ in range(m)]     # add_noise: all noise values first,
        g.phase = "noise"
        noise = [g.next_double() < e for _ in range(m)]      # then the noise flags,
        g.phase = "mask"
        mask = [g.next_double() < mask_ratio for _ in range(m)]  # then the mask flags
        for k in range(m):
            f = value[k] if noise[k] else seq[k]
            feat.append(0 if (noise[k] and mask[k]) else f)
        lab.extend(seq)
        feat.append(V + 1)
        lab.append(V + 1)
    g.phase = None
    return np.asarray(feat[:L], np.int32), np.asarray(lab[1:L + 1], np.int32)


def draw_level_batch(g, B, V, n, l, e, L, mask_ratio=MASK_RATIO):
    rows = [draw_level_row(g, V, n, l, e, L, mask_ratio) for _ in range(B)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def fast_row(rs, V, n, l, e, L, mask_ratio=MASK_RATIO):
    """The same row from a numpy RandomState `rs` through NumPy's own samplers (vectorised per element / chunk)."""
    elements = [rs.randint(1, V, size=max(3, rs.poisson(l)), dtype=np.int32) for _ in range(n)]
    feats, labs, cur = [], [], 0
    sep = np.array([V + 1], np.int32)
    while cur < L + 1:
        seq = elements[rs.randint(0, n - 1)]
        value = rs.randint(1, V, size=seq.shape, dtype=np.int32)
        noise = rs.random_sample(seq.shape) < e
        mask = rs.random_sample(seq.shape) < mask_ratio
        f = np.where(noise, value, seq)
        f[noise & mask] = 0
        feats += [f, sep]
        labs += [seq, sep]
        cur += len(seq) + 1
    return np.concatenate(feats)[:L].astype(np.int32), np.concatenate(labs)[1:L + 1].astype(np.int32)


def fast_batch(rs, B, V, n, l, e, L, mask_ratio=MASK_RATIO):
    rows = [fast_row(rs, V, n, l, e, L, mask_ratio) for _ in range(B)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def fast_seeded(seeds, V, n, l, e, L, mask_ratio=MASK_RATIO):
    """Seeded mode: row t from its own stream numpy.random.seed(seeds[t])."""
    rows = [fast_row(np.random.RandomState(int(s)), V, n, l, e, L, mask_ratio) for s in seeds]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def to_text(features, labels):
    """generate_to_file's format: one line per row, tab-separated "feature,label" pairs."""
    return "".join("\t".join("%d,%d" % (a, b) for a, b in zip(f.tolist(), lb.tolist())) + "\n"
                   for f, lb in zip(features, labels))
