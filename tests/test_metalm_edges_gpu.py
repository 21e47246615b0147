"""meta-lm-v0 on the MI355X at its edges: mg_metalm_generate on the configurations of tests/metalm_cases.py (whose rows put
bulk_tokens, doubles and the row end on every edge of the 624-word block; test_metalm_edges.py asserts that), chained mode
from every start position, the launches that need more than 64 KiB of LDS, overflow in the middle of a batch, and batch
sizes around the wave width. Every comparison is exact integer equality with tests/metalm_oracle.py's fast_* restatement
(NumPy's own RandomState) or the reference's recorded rows (tests/golden/metalm_edges.npz)."""
import os

import numpy as np
import pytest

import metalm_cases as mc
import metalm_oracle as mo

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metalm_edges.npz")
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _gen(cfg, **kw):
    from metagym_amd.metalm import MetaLM
    gen = MetaLM(device="cuda", **dict(mc.ctor_kwargs(cfg), **kw))
    gen.mask_ratio = mc.mask_ratio(cfg)
    return gen


def _np(t):
    return t.cpu().numpy()


def _ref_seeded(seeds, cfg):
    return mo.fast_seeded(seeds, *mc.cfg_args(cfg), mask_ratio=mc.mask_ratio(cfg))


def _lds_bytes(gen):
    return 2496 + 8 * (int(gen.n) + gen.element_capacity)


# ------------------------------------------------------------------------------------------------ 1. the table, seeded
def test_every_table_row_in_seeded_mode(golden):
    for ci, (name, cfg, seeds) in enumerate(mc.CASES):
        gen = _gen(cfg)
        fo, lo = _ref_seeded(seeds, cfg)
        f, lb = gen.batch_generator(len(seeds), seeds=seeds)
        f, lb = _np(f), _np(lb)
        assert np.array_equal(f, fo) and np.array_equal(lb, lo), name
        for r, s in enumerate(seeds):
            assert np.array_equal(f[r], golden["row_%d_%d_features" % (ci, s)]), (name, s)
            assert np.array_equal(lb[r], golden["row_%d_%d_labels" % (ci, s)]), (name, s)
            f1, lb1 = gen.batch_generator(1, seed=s)
            assert np.array_equal(_np(f1)[0], fo[r]) and np.array_equal(_np(lb1)[0], lo[r]), (name, s)


def test_seed_at_the_top_of_its_range():
    B = 5
    for cfg in (mc.E0, mc.CHAIN_PTRS):
        gen = _gen(cfg)
        top = list(range(2 ** 32 - B, 2 ** 32))
        f, lb = gen.batch_generator(B, seed=2 ** 32 - B)
        fs, ls = gen.batch_generator(B, seeds=top)
        fo, lo = _ref_seeded(top, cfg)
        assert np.array_equal(_np(f), _np(fs)) and np.array_equal(_np(lb), _np(ls))
        assert np.array_equal(_np(f), fo) and np.array_equal(_np(lb), lo)
        with pytest.raises(ValueError):
            gen.batch_generator(B, seed=2 ** 32 - B + 1)


# ------------------------------------------------------------------------------------ 2. chained, every start position
def _chained_sweep(cfg, positions, B=2):
    """From the key of numpy.random.seed(7) read at `pos`: the batch, the stream handed back and the next global draw."""
    key = mo.MTStream.seeded(7).key
    gen = _gen(cfg)
    state = np.random.get_state()
    try:
        for pos in positions:
            start = ("MT19937", key, pos, 0, 0.0)
            rs = np.random.RandomState()
            rs.set_state(start)
            fo, lo = mo.fast_batch(rs, B, *mc.cfg_args(cfg), mask_ratio=mc.mask_ratio(cfg))
            np.random.set_state(start)
            f, lb = gen.batch_generator(B)
            assert np.array_equal(_np(f), fo) and np.array_equal(_np(lb), lo), pos
            after, want = np.random.get_state(), rs.get_state()
            assert np.array_equal(after[1], want[1]), pos
            assert after[2] == want[2], (pos, after[2], want[2])
            assert np.random.random() == rs.random_sample(), pos
    finally:
        np.random.set_state(state)


def test_chained_mode_from_every_start_position_ptrs():
    _chained_sweep(mc.CHAIN_PTRS, range(625))


def test_chained_mode_from_the_block_ends_multiplication_poisson():
    _chained_sweep(mc.CHAIN_MULT, [0, 1, 2, 3] + list(range(560, 625)))


# ----------------------------------------------------------------------------------------- 3. more than 64 KiB of LDS
WIDE = dict(V=64, n=100, l=64, e=0.1, L=600)        # default capacity 13600: 112 KB
WIDE_SEEDS = [0, 1, 2, 3, 4, 5, 6, 2 ** 32 - 1]


@pytest.fixture(scope="module")
def wide_rows():
    return _ref_seeded(WIDE_SEEDS, WIDE)


def test_large_lds_seeded_launch_and_a_default_size_launch_after_it(wide_rows):
    gen = _gen(WIDE)
    assert _lds_bytes(gen) == 112096 > 64 * 1024
    f, lb = gen.batch_generator(len(WIDE_SEEDS), seeds=WIDE_SEEDS)
    assert np.array_equal(_np(f), wide_rows[0]) and np.array_equal(_np(lb), wide_rows[1])
    small = _gen(mc.CHAIN_PTRS)                                            # straight after the large one
    assert _lds_bytes(small) < 64 * 1024
    f, lb = small.batch_generator(4, seed=10)
    fo, lo = _ref_seeded(range(10, 14), mc.CHAIN_PTRS)
    assert np.array_equal(_np(f), fo) and np.array_equal(_np(lb), lo)
    f, lb = gen.batch_generator(len(WIDE_SEEDS), seeds=WIDE_SEEDS)         # and the large one again
    assert np.array_equal(_np(f), wide_rows[0]) and np.array_equal(_np(lb), wide_rows[1])


def test_large_lds_long_elements():
    name, cfg, seeds = [c for c in mc.CASES if c[0] == "long_elements"][0]
    gen = _gen(cfg)
    assert gen.element_capacity == 11148 and _lds_bytes(gen) > 64 * 1024
    f, lb = gen.batch_generator(len(seeds), seeds=seeds)
    fo, lo = _ref_seeded(seeds, cfg)
    assert np.array_equal(_np(f), fo) and np.array_equal(_np(lb), lo)


def test_element_capacity_of_exactly_160_kib():
    cfg = dict(V=64, n=10, l=64, e=0.1, L=600)
    seeds = [0, 1, 2, 2 ** 32 - 1]
    full = _gen(cfg, element_capacity=20158)
    assert _lds_bytes(full) == 160 * 1024
    f, lb = full.batch_generator(len(seeds), seeds=seeds)
    fd, ld = _gen(cfg).batch_generator(len(seeds), seeds=seeds)
    fo, lo = _ref_seeded(seeds, cfg)
    assert np.array_equal(_np(f), _np(fd)) and np.array_equal(_np(lb), _np(ld))
    assert np.array_equal(_np(f), fo) and np.array_equal(_np(lb), lo)
    from metagym_amd._lib import MetaGymHipError
    with pytest.raises(MetaGymHipError, match="160 KiB"):
        _gen(cfg, element_capacity=20159).batch_generator(1, seed=0)


def test_large_lds_chained_launch():
    gen = _gen(WIDE)
    state = np.random.get_state()
    try:
        np.random.seed(11)
        np.random.randint(0, 10, size=333)                                 # start part-way through the block
        rs = np.random.RandomState()
        rs.set_state(np.random.get_state())
        f, lb = gen.batch_generator(3)
        fo, lo = mo.fast_batch(rs, 3, *mc.cfg_args(WIDE))
        assert np.array_equal(_np(f), fo) and np.array_equal(_np(lb), lo)
        after, want = np.random.get_state(), rs.get_state()
        assert np.array_equal(after[1], want[1]) and after[2] == want[2]
        assert np.random.random() == rs.random_sample()
    finally:
        np.random.set_state(state)


# --------------------------------------------------------------------------------- 4. overflow in the middle of a batch
def test_seeded_overflow_mid_batch_leaves_the_fitting_rows_complete():
    import torch
    cfg, cap = mc.CHAIN_PTRS, mc.OVERFLOW_CAP
    V, n, l, e, L = mc.cfg_args(cfg)
    pool = list(range(300, 364))
    totals = np.asarray([mc.element_total(np.random.RandomState(s), V, n, l) for s in pool])
    under = [s for s, t in zip(pool, totals) if t <= cap]
    over = [s for s, t in zip(pool, totals) if t > cap]
    assert len(under) >= 10 and len(over) >= 3
    seeds = under[:5] + over[:1] + under[5:10] + over[1:] + under[10:]     # rows 5 and 11.. overflow
    B = len(seeds)
    fits = np.asarray([s in under for s in seeds])
    gen = _gen(cfg, element_capacity=cap)
    feat = torch.full((B, L), -7, dtype=torch.int32, device="cuda")
    lab = torch.full((B, L), -7, dtype=torch.int32, device="cuda")
    gen.batch_generator(B, seeds=seeds, out=(feat, lab), check=False)
    assert int(gen.last_overflow.item()) == 5
    fo, lo = _ref_seeded(seeds, cfg)
    f, lb = _np(feat), _np(lab)
    assert np.array_equal(f[fits], fo[fits]) and np.array_equal(lb[fits], lo[fits])
    assert (f[~fits] == -7).all() and (lb[~fits] == -7).all()             # an overflowing row writes nothing
    from metagym_amd._lib import MetaGymHipError
    with pytest.raises(MetaGymHipError, match="row 5 "):
        gen.batch_generator(B, seeds=seeds)
    # the lowest overflowing row, not the first to finish: the same rows with the overflowing ones last but one
    seeds2 = under[:12] + over[:2] + under[12:13]
    gen.batch_generator(len(seeds2), seeds=seeds2, check=False)
    assert int(gen.last_overflow.item()) == 12
    gen.batch_generator(12, seeds=under[:12], check=False)
    assert int(gen.last_overflow.item()) == INT32_MAX


def test_chained_overflow_at_row_2_names_it_and_leaves_the_global_state():
    from metagym_amd._lib import MetaGymHipError
    cfg, cap = mc.CHAIN_PTRS, mc.OVERFLOW_CAP
    s = mc.chained_overflow_seed(cfg, cap, 2)
    gen = _gen(cfg, element_capacity=cap)
    state = np.random.get_state()
    try:
        np.random.seed(s)
        before = np.random.get_state()
        with pytest.raises(MetaGymHipError, match="row 2 "):
            gen.batch_generator(4)
        after = np.random.get_state()
        assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
        # the two rows that fit are there for the asking, from the untouched state
        rs = np.random.RandomState(s)
        f, lb = gen.batch_generator(2)
        fo, lo = mo.fast_batch(rs, 2, *mc.cfg_args(cfg))
        assert np.array_equal(_np(f), fo) and np.array_equal(_np(lb), lo)
        assert np.random.random() == rs.random_sample()
    finally:
        np.random.set_state(state)


# --------------------------------------------------------------------------------------------------- 5. batch shape
def test_batch_sizes_around_the_wave_width():
    gen = _gen(mc.E0)
    fo, lo = _ref_seeded(range(100, 357), mc.E0)
    for B in (1, 63, 64, 65, 257):
        f, lb = gen.batch_generator(B, seed=100)
        assert f.shape == (B, mc.E0["L"])
        assert np.array_equal(_np(f), fo[:B]) and np.array_equal(_np(lb), lo[:B]), B
    for t in (0, 1, 62, 63, 64, 65, 255, 256):                             # f, lb: the batch of 257
        f1, lb1 = gen.batch_generator(1, seed=100 + t)
        assert np.array_equal(_np(f1)[0], _np(f)[t]) and np.array_equal(_np(lb1)[0], _np(lb)[t]), t
