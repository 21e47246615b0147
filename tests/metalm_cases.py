"""MetaLM edge fixtures shared by tests/test_metalm_edges.py (CPU), tests/test_metalm_edges_gpu.py and
scripts/gen_golden_metalm.py: the table of configurations and seeds recorded in tests/golden/metalm_edges.npz, and a draw
tracker that replays a row of `metalm_oracle.draw_level_row` and tells where each of the kernel's draw batches (bulk_tokens,
doubles in metagym_amd/csrc/metalm.hip) falls inside the generator's 624-word block."""
import numpy as np

import metalm_oracle as mo

_N = 624
WAVE = 64                      # draws per bulk_tokens step, doubles per doubles() step

E0 = dict(V=34, n=3, l=3.5, e=0.3, L=60)
# chained-mode sweeps over the start position: a PTRS configuration, and E0 for the multiplication method
CHAIN_PTRS = dict(E0, l=12.5)
CHAIN_MULT = E0
OVERFLOW_CAP = 44              # an element_capacity about one standard deviation above CHAIN_PTRS's mean total of 37.5

# (name, configuration, seeds). A configuration is MetaLM's (V, n, l, e, L), plus `mask_ratio` where it is not the default.
# The seeds after the first few of a case were picked so that every event of EVENTS occurs in some row of the table
# (test_metalm_edges.py asserts it); 2^32 - 1 is the largest seed there is.
CASES = [
    # V - 2 = 2^k: the mask is 2^(k+1) - 1 and about half of every batch of draws is rejected
    ("reject_half_v34", E0, [0, 1, 2, 3, 2 ** 32 - 1, 23, 52, 24, 31, 6, 20]),
    ("reject_half_v66", dict(V=66, n=4, l=10.0, e=0.5, L=200), [0, 1, 2, 3, 2 ** 32 - 1]),
    ("reject_half_v1026", dict(V=1026, n=3, l=12.5, e=0.1, L=300), [0, 1, 2, 3, 2 ** 32 - 1]),
    # V - 2 = 2^k - 1: nothing is rejected
    ("reject_none_v65", dict(V=65, n=5, l=40.0, e=0.2, L=250), [0, 1, 2, 3, 63]),
    # the smallest token ranges: bounded(1) (one bit, nothing rejected) and bounded(2) (two bits, a quarter rejected)
    ("v3", dict(V=3, n=4, l=6.0, e=0.3, L=100), [0, 1, 2, 3]),
    ("v4", dict(V=4, n=3, l=15.0, e=0.3, L=120), [0, 1, 2, 3, 41]),
    # element-index ranges: n = 3 (bounded(1)), n = 4 (bounded(2), mask 3), n = 6 (bounded(4), mask 7); their elements are
    # long enough for a rejection-heavy batch of 64 draws to leave the quota open
    ("n3", dict(V=66, n=3, l=50.0, e=0.25, L=250), [0, 1, 2, 3, 27]),
    ("n4", dict(V=34, n=4, l=80.0, e=0.2, L=300), [0, 1, 2, 3]),
    ("n6", dict(V=130, n=6, l=30.0, e=0.15, L=250), [0, 1, 2, 3]),
    # the Poisson switch: l = 10.0 exactly is PTRS (reject_half_v66 too); just above the floor l > 1 every element is 3 long
    ("ptrs_at_10", dict(V=50, n=5, l=10.0, e=0.2, L=150), [0, 1, 2, 3]),
    ("l_floor", dict(V=4, n=5, l=1.0000001, e=0.2, L=50), [0, 1, 2, 3, 2 ** 32 - 1]),
    # the largest V the ABI accepts: tokens reach 2^31 - 3, the separator is 2^31 - 1, bit 31 stays the kernel's noise flag
    ("v_int32_limit", dict(V=2 ** 31 - 2, n=3, l=20.0, e=0.4, L=150), [0, 1, 2, 3, 2 ** 32 - 1]),
    # long elements: about 78 batches of 64 per element, default capacity 11148 = 92 KB of LDS
    ("long_elements", dict(V=64, n=2, l=5000.0, e=0.1, L=300), [0, 1, 2]),
    # mask_ratio at and outside [0, 1], and a noise ratio no double is below
    ("mask_0", dict(E0, mask_ratio=0.0), [0, 1, 2, 3]),
    ("mask_1", dict(E0, mask_ratio=1.0), [0, 1, 2, 3]),
    ("mask_negative", dict(E0, mask_ratio=-1.0), [0, 1, 2, 3]),
    ("mask_2", dict(E0, mask_ratio=2.0), [0, 1, 2, 3]),
    ("mask_inf", dict(E0, mask_ratio=float("inf")), [0, 1, 2, 3]),
    ("e_1e-300", dict(E0, e=1e-300), [0, 1, 2, 3]),
]


def cfg_args(cfg):
    return cfg["V"], cfg["n"], cfg["l"], cfg["e"], cfg["L"]


def mask_ratio(cfg):
    return cfg.get("mask_ratio", mo.MASK_RATIO)


def ctor_kwargs(cfg):
    """MetaLM's constructor arguments (mask_ratio is an attribute set afterwards, in the reference too)."""
    return {k: v for k, v in cfg.items() if k != "mask_ratio"}


def table_rows():
    """(case index, name, configuration, seed) of every row of the table, in fixture order."""
    return [(ci, name, cfg, s) for ci, (name, cfg, seeds) in enumerate(CASES) for s in seeds]


class DrawTracker(mo.MTStream):
    """An MTStream that records, for every sampler call of draw_level_row (each assignment to `phase` opens one), the read
    position of every 32-bit draw (0 where the draw refills first) and, for bounded draws, whether it was accepted."""
    _straddling = False

    def __init__(self, key, pos):
        self.calls = []
        super(DrawTracker, self).__init__(key, pos)

    @property
    def phase(self):
        return self._phase

    @phase.setter
    def phase(self, value):
        # MTStream.next_double renames the phase to "<phase>/straddle" around a straddling pair and back: the same call
        straddle = isinstance(value, str) and value.endswith("/straddle")
        if not straddle and not self._straddling:
            self.calls.append(dict(phase=value, pos=[], accepted=[]))
        self._straddling = straddle
        self._phase = value

    def next_u32(self):
        self.calls[-1]["pos"].append(self.pos % _N)
        return super(DrawTracker, self).next_u32()

    def bounded(self, r):
        call = self.calls[-1]
        n0 = len(call["pos"])
        d = super(DrawTracker, self).bounded(r)
        drawn = len(call["pos"]) - n0
        if drawn:                                        # masked rejection: every draw but the last was rejected
            call["accepted"] += [False] * (drawn - 1) + [True]
        return d


def token_batches(call):
    """One "elements" or "values" call as bulk_tokens runs it: batches of up to 64 draws that stop at the end of the block
    (`take`) and at the draw that fills the quota (`used`). Per batch: the read position at its start, take, used (the
    draws it consumed), how many of those were accepted and rejected, the quota still open at its start, whether it fills."""
    pos, acc = call["pos"], call["accepted"]
    assert len(pos) == len(acc)
    out, i, need = [], 0, sum(acc)
    while i < len(pos):
        p = pos[i]
        take = min(WAVE, _N - p)
        filled = len(pos) - i <= take                    # the record of a call ends at the draw that fills its quota
        used = len(pos) - i if filled else take
        assert pos[i:i + used] == list(range(p, p + used))
        a = sum(acc[i:i + used])
        out.append(dict(pos=p, take=take, used=used, accepted=a, rejected=used - a, need=need, filled=filled))
        need -= a
        i += used
    return out


def double_batches(call):
    """One "noise" or "mask" call as doubles() runs it: batches of up to 64 pairs that stop at the end of the block; a pair
    that starts on the block's last word is drawn alone. Per batch: the read position at its start, the words left in the
    block, the doubles drawn (two draws each), whether it is the lone straddling pair."""
    pos = call["pos"]
    assert len(pos) % 2 == 0
    out, i = [], 0
    while i < len(pos):
        p = pos[i]
        avail = _N - p
        if avail == 1:
            assert pos[i + 1] == 0
            out.append(dict(pos=p, avail=1, count=1, straddle=True))
            i += 2
            continue
        cnt = min((len(pos) - i) // 2, WAVE, avail >> 1)
        assert pos[i:i + 2 * cnt] == list(range(p, p + 2 * cnt))
        out.append(dict(pos=p, avail=avail, count=cnt, straddle=False))
        i += 2 * cnt
    return out


EVENTS = (
    "tokens_start_under_64_left",             # (a) take < 64
    "tokens_quota_fills_inside_window",       # (b) used < take: the draws behind the filling one belong to the next sampler
    "tokens_24_of_64_rejected_quota_open",    # (c) a full batch of 64, >= 24 rejected, the quota needs another batch
    "doubles_odd_left_then_straddle",         # (d) a batch takes all pairs of an odd remainder, then the lone pair
    "doubles_start_one_left",                 # (e) a batch starts with exactly 1 word left
    "row_end_plus_0", "row_end_plus_1", "row_end_plus_2", "row_end_plus_3_or_more",   # (f) cur - (L + 1) after the last chunk
    # beyond the required ones
    "tokens_cut_at_block_end_quota_open",     # take < 64 and the quota goes on behind the refill
    "tokens_quota_fills_on_last_word",        # the filling draw is word 623
    "doubles_call_opens_on_straddle",         # the first double of a chunk's noise or mask flags straddles
)


def row_end_excess(tracker, L):
    """cur - (L + 1) after the row's last chunk. The stream of a row is cur long and the outputs are its [0, L) and [1, L+1):
    0 puts the last separator at labels[L-1] (and nowhere in features); x > 0 drops it and the last x - 1 tokens, and the
    token before those is labels[L-1] alone."""
    cur = sum(len(c["pos"]) // 2 + 1 for c in tracker.calls if c["phase"] == "noise")
    assert cur >= L + 1
    return cur - (L + 1)


def row_events(tracker, L):
    seen = set()
    for call in tracker.calls:
        if call["phase"] in ("elements", "values"):
            for b in token_batches(call):
                if b["take"] < WAVE:
                    seen.add("tokens_start_under_64_left")
                    if not b["filled"]:
                        seen.add("tokens_cut_at_block_end_quota_open")
                if b["filled"] and b["used"] < b["take"]:
                    seen.add("tokens_quota_fills_inside_window")
                if b["filled"] and b["pos"] + b["used"] == _N:
                    seen.add("tokens_quota_fills_on_last_word")
                if b["take"] == WAVE and b["rejected"] >= 24 and not b["filled"]:
                    seen.add("tokens_24_of_64_rejected_quota_open")
        elif call["phase"] in ("noise", "mask"):
            bs = double_batches(call)
            for k, b in enumerate(bs):
                if b["straddle"]:
                    seen.add("doubles_start_one_left")
                    if k == 0:
                        seen.add("doubles_call_opens_on_straddle")
                elif b["avail"] % 2 == 1 and b["count"] == b["avail"] >> 1 and k + 1 < len(bs) and bs[k + 1]["straddle"]:
                    seen.add("doubles_odd_left_then_straddle")
    x = row_end_excess(tracker, L)
    seen.add("row_end_plus_%d" % x if x < 3 else "row_end_plus_3_or_more")
    return seen


def tracked_row(cfg, seed):
    """(features, labels, tracker) of draw_level_row on numpy.random.seed(seed)'s stream."""
    g = DrawTracker.seeded(seed)
    f, lb = mo.draw_level_row(g, *cfg_args(cfg), mask_ratio=mask_ratio(cfg))
    return f, lb, g


def element_total(rs, V, n, l):
    """Advance the RandomState through one row's elements; their total length (what element_capacity bounds)."""
    t = 0
    for _ in range(n):
        m = max(3, rs.poisson(l))
        rs.randint(1, V, size=m, dtype=np.int32)
        t += m
    return t


def chained_overflow_seed(cfg, cap, row, seeds=range(4096)):
    """The first s for which, from numpy.random.seed(s), rows 0..row-1 of a chained batch fit `cap` element tokens and row
    `row` does not."""
    V, n, l, e, L = cfg_args(cfg)
    for s in seeds:
        rs = np.random.RandomState(s)
        fits = True
        for _ in range(row):
            st = rs.get_state()
            fits = element_total(rs, V, n, l) <= cap
            if not fits:
                break
            rs.set_state(st)
            mo.fast_row(rs, V, n, l, e, L, mask_ratio(cfg))
        if fits and element_total(rs, V, n, l) > cap:
            return s
    raise AssertionError("no start state found")
