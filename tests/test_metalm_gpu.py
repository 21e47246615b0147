"""meta-lm-v0 on the MI355X: mg_metalm_generate against the reference's rows (tests/golden/metalm.npz) and the host
restatements (tests/metalm_oracle.py). Every comparison is exact integer equality."""
import io
import json
import os

import numpy as np
import pytest

import metalm_oracle as mo

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metalm.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _gen(cfg, **kw):
    from metagym_amd.metalm import MetaLM
    return MetaLM(device="cuda", **dict(cfg, **kw))


def _np(t):
    return t.cpu().numpy()


def test_every_golden_row_in_seeded_mode(golden):
    cases = json.loads(str(golden["cases"]))
    by_case = {}
    for ci, s in golden["rows"]:
        by_case.setdefault(int(ci), []).append(int(s))
    for ci, seeds in by_case.items():
        gen = _gen(cases[ci])
        f, lb = gen.batch_generator(len(seeds), seeds=seeds)
        f, lb = _np(f), _np(lb)
        for r, s in enumerate(seeds):
            assert np.array_equal(f[r], golden["row_%d_%d_features" % (ci, s)]), (cases[ci], s)
            assert np.array_equal(lb[r], golden["row_%d_%d_labels" % (ci, s)]), (cases[ci], s)
        f1, lb1 = gen.data_generator(seed=seeds[-1])
        assert f1.shape == (cases[ci]["L"],)
        assert np.array_equal(_np(f1), golden["row_%d_%d_features" % (ci, seeds[-1])])
        assert np.array_equal(_np(lb1), golden["row_%d_%d_labels" % (ci, seeds[-1])])


def test_chained_mode_is_the_reference_batch_generator_and_leaves_its_global_state(golden):
    state = np.random.get_state()
    try:
        for bi, (cfg, s, B) in enumerate(json.loads(str(golden["batches"]))):
            np.random.seed(s)
            f, lb = _gen(cfg).batch_generator(B)
            assert np.array_equal(_np(f), golden["batch_%d_features" % bi])
            assert np.array_equal(_np(lb), golden["batch_%d_labels" % bi])
            st = np.random.get_state()
            assert np.array_equal(st[1], golden["batch_%d_key" % bi]) and st[2] == int(golden["batch_%d_pos" % bi])
            assert np.random.random() == float(golden["batch_%d_next_random" % bi])
        # data_generator() without a seed continues the global stream too: the 65536-token row
        cases = json.loads(str(golden["cases"]))
        ci = [i for i, c in enumerate(cases) if c["L"] == 65536][0]
        np.random.seed(3)
        f, lb = _gen(cases[ci]).data_generator()
        assert np.array_equal(_np(f), golden["row_%d_3_features" % ci])
        assert np.array_equal(_np(lb), golden["row_%d_3_labels" % ci])
        rs = np.random.RandomState(3)
        mo.fast_row(rs, 64, 10, 64, 0.10, 65536)
        assert np.random.random() == rs.random_sample()
        # a stream already part-way through its 624-word block, with a cached gaussian that must survive
        np.random.seed(12)
        np.random.standard_normal()
        np.random.randint(0, 10, size=101)
        before = np.random.get_state()
        rs = np.random.RandomState()
        rs.set_state(before)
        f, lb = _gen(dict(V=17, n=4, l=20.5, e=0.2, L=900)).batch_generator(6)
        fo, lo = mo.fast_batch(rs, 6, 17, 4, 20.5, 0.2, 900)
        assert np.array_equal(_np(f), fo) and np.array_equal(_np(lb), lo)
        after = np.random.get_state()
        assert after[3] == before[3] == 1 and after[4] == before[4]
        assert np.array_equal(after[1], rs.get_state()[1]) and after[2] == rs.get_state()[2]
    finally:
        np.random.set_state(state)


def test_4096_seeded_rows_at_the_defaults_against_the_fast_restatement():
    import torch
    import metagym_amd
    gen = metagym_amd.make("meta-lm-v0", device="cuda")
    f, lb = gen.batch_generator(4096, seed=0)
    assert f.shape == (4096, 2048) and lb.shape == (4096, 2048)
    assert f.dtype == torch.int32 and lb.dtype == torch.int32 and f.is_cuda and lb.is_cuda
    fo, lo = mo.fast_seeded(range(4096), 64, 10, 64, 0.10, 2048)
    assert np.array_equal(_np(f), fo)
    assert np.array_equal(_np(lb), lo)


def test_rows_are_independent_streams_and_seeds_equal_seed():
    gen = _gen(dict(V=64, n=10, l=64, e=0.1, L=1500))
    f, lb = gen.batch_generator(37, seed=1000)
    f, lb = _np(f), _np(lb)
    for t in (0, 1, 17, 36):
        f1, lb1 = gen.batch_generator(1, seed=1000 + t)
        assert np.array_equal(_np(f1)[0], f[t]) and np.array_equal(_np(lb1)[0], lb[t])
    fs, ls = gen.batch_generator(37, seeds=np.arange(1000, 1037))
    assert np.array_equal(_np(fs), f) and np.array_equal(_np(ls), lb)
    top = [2 ** 32 - 1, 0, 123456789, 2 ** 31]
    fs, ls = gen.batch_generator(4, seeds=top)
    fo, lo = mo.fast_seeded(top, 64, 10, 64, 0.1, 1500)
    assert np.array_equal(_np(fs), fo) and np.array_equal(_np(ls), lo)
    gen.mask_ratio = 0.55                                                  # the attribute is read at every call
    fs, ls = gen.batch_generator(4, seeds=top)
    fo, lo = mo.fast_seeded(top, 64, 10, 64, 0.1, 1500, mask_ratio=0.55)
    assert np.array_equal(_np(fs), fo) and np.array_equal(_np(ls), lo)


def test_out_buffers_and_a_non_default_stream():
    import torch
    gen = _gen(dict(V=30, n=6, l=25.0, e=0.15, L=800))
    fo, lo = mo.fast_seeded(range(50, 70), 30, 6, 25.0, 0.15, 800)
    feat = torch.full((20, 800), -7, dtype=torch.int32, device="cuda")
    lab = torch.full((20, 800), -7, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rf, rl = gen.batch_generator(20, seed=50, out=(feat, lab), check=False)
    s.synchronize()
    assert rf is feat and rl is lab
    assert np.array_equal(_np(feat), fo) and np.array_equal(_np(lab), lo)
    assert int(gen.last_overflow.item()) == 2 ** 31 - 1
    with pytest.raises(ValueError):
        gen.batch_generator(20, seed=50, out=(feat[:, :10], lab))


def _element_totals(seeds, V, n, l):
    totals = []
    for s in seeds:
        rs = np.random.RandomState(s)
        t = 0
        for _ in range(n):
            m = max(3, rs.poisson(l))
            rs.randint(1, V, size=m, dtype=np.int32)
            t += m
        totals.append(t)
    return np.asarray(totals)


def test_too_small_element_capacity_raises_and_names_the_row():
    from metagym_amd._lib import MetaGymHipError
    V, n, l = 64, 10, 64.0
    pool = np.arange(200, 264)
    totals = _element_totals(pool, V, n, l)
    cap = int(np.sort(totals)[-5])                        # four seeds of the pool need more than this
    under, over = pool[totals <= cap].tolist(), pool[totals > cap].tolist()
    seeds = under[:5] + over[:1] + under[5:10] + over[1:]  # rows 5 and 11.. overflow
    gen = _gen(dict(V=V, n=n, l=l, e=0.1, L=600), element_capacity=cap)
    with pytest.raises(MetaGymHipError, match="row 5 "):
        gen.batch_generator(len(seeds), seeds=seeds)
    # rows that fit are complete
    f, lb = gen.batch_generator(5, seeds=under[:5])
    fo, lo = mo.fast_seeded(under[:5], V, n, l, 0.1, 600)
    assert np.array_equal(_np(f), fo) and np.array_equal(_np(lb), lo)
    # chained: the error names the row and numpy.random's state is left as it was
    state = np.random.get_state()
    try:
        np.random.seed(over[0])
        before = np.random.get_state()
        with pytest.raises(MetaGymHipError, match="row 0 "):
            gen.batch_generator(3)
        after = np.random.get_state()
        assert np.array_equal(before[1], after[1]) and before[2] == after[2]
    finally:
        np.random.set_state(state)


def test_generate_to_file_text_equals_the_reference(golden, tmp_path):
    cfg, s, B = json.loads(str(golden["text_case"]))
    state = np.random.get_state()
    try:
        np.random.seed(s)
        buf = io.StringIO()
        _gen(cfg).generate_to_file(B, buf)
        assert buf.getvalue() == str(golden["text"])
        np.random.seed(s)
        path = str(tmp_path / "metalm.txt")
        _gen(cfg).generate_to_file(B, path)
        assert open(path).read() == str(golden["text"])
    finally:
        np.random.set_state(state)
    f, lb = mo.fast_seeded(range(9, 9 + B), cfg["V"], cfg["n"], cfg["l"], cfg["e"], cfg["L"])
    buf = io.StringIO()
    _gen(cfg).generate_to_file(B, buf, seed=9)
    assert buf.getvalue() == mo.to_text(f, lb)
