"""meta-lm-v0 at its edges, without a GPU: on the configurations of tests/metalm_cases.py the two host restatements agree with
each other and with the reference's own rows (tests/golden/metalm_edges.npz), and those rows put the kernel's draw batches on
every edge of the 624-word block that test_metalm_edges_gpu.py then relies on. The LDS limit of the C ABI, to the byte."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import metalm_cases as mc
import metalm_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metalm_edges.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def tracked():
    """Every table row through the draw-level restatement, once: {(case index, seed): (features, labels, tracker)}."""
    return {(ci, s): mc.tracked_row(cfg, s) for ci, _, cfg, s in mc.table_rows()}


def test_the_fixture_holds_the_table(golden):
    assert json.loads(str(golden["cases"])) == [[name, cfg] for name, cfg, _ in mc.CASES]
    assert golden["rows"].tolist() == [[ci, s] for ci, _, _, s in mc.table_rows()]
    assert os.path.getsize(GOLDEN) < 1 << 20
    for _, cfg, _ in mc.CASES:
        assert cfg["L"] <= 300


def test_draw_level_row_equals_fast_row_on_every_table_row(tracked):
    for ci, name, cfg, s in mc.table_rows():
        f, lb, _ = tracked[ci, s]
        fo, lo = mo.fast_row(np.random.RandomState(s), *mc.cfg_args(cfg), mask_ratio=mc.mask_ratio(cfg))
        assert f.shape == (cfg["L"],) and f.dtype == np.int32
        assert np.array_equal(f, fo) and np.array_equal(lb, lo), (name, s)


def test_both_restatements_reproduce_the_reference_rows(golden, tracked):
    for ci, name, cfg, s in mc.table_rows():
        gf, gl = golden["row_%d_%d_features" % (ci, s)], golden["row_%d_%d_labels" % (ci, s)]
        f, lb, _ = tracked[ci, s]
        assert np.array_equal(f, gf) and np.array_equal(lb, gl), (name, s)
        fo, lo = mo.fast_seeded([s], *mc.cfg_args(cfg), mask_ratio=mc.mask_ratio(cfg))
        assert np.array_equal(fo[0], gf) and np.array_equal(lo[0], gl), (name, s)


def test_tracker_leaves_the_stream_as_a_plain_mtstream_does():
    cfg = mc.CASES[1][1]
    f, lb, g = mc.tracked_row(cfg, 2)
    p = mo.MTStream.seeded(2)
    fp, lp = mo.draw_level_row(p, *mc.cfg_args(cfg))
    assert np.array_equal(f, fp) and np.array_equal(lb, lp)
    assert np.array_equal(g.key, p.key) and g.pos == p.pos and g.refills == p.refills
    # every draw of the row is in the record, in stream order
    pos = [q for c in g.calls for q in c["pos"]]
    assert pos == [i % 624 for i in range(len(pos))] and (len(pos) - 1) // 624 + 1 == len(p.refills)
    # and the batches of every call account for exactly its draws
    for c in g.calls:
        if c["phase"] in ("elements", "values"):
            bs = mc.token_batches(c)
            assert sum(b["used"] for b in bs) == len(c["pos"]) and sum(b["accepted"] for b in bs) == sum(c["accepted"])
            assert all(b["filled"] == (k == len(bs) - 1) for k, b in enumerate(bs))
        elif c["phase"] in ("noise", "mask"):
            assert 2 * sum(b["count"] for b in mc.double_batches(c)) == len(c["pos"])


def test_table_rows_put_the_draw_batches_on_every_edge(tracked):
    """A condition on the inputs of the GPU test: each edge of bulk_tokens, doubles and the row end occurs in some row."""
    where = {}
    for ci, name, cfg, s in mc.table_rows():
        for ev in mc.row_events(tracked[ci, s][2], cfg["L"]):
            where.setdefault(ev, []).append("%s/%d" % (name, s))
    for ev in mc.EVENTS:
        print("%-40s %3d rows, first %s" % (ev, len(where.get(ev, [])), where.get(ev, ["-"])[0]))
    missing = [ev for ev in mc.EVENTS if ev not in where]
    assert not missing, missing
    # the first configuration alone ends its rows in all four ways
    first = {ev for (ci, s), (_, _, g) in tracked.items() if ci == 0 for ev in mc.row_events(g, mc.E0["L"])}
    assert {"row_end_plus_0", "row_end_plus_1", "row_end_plus_2", "row_end_plus_3_or_more"} <= first
    # the ranges are what the table says they are: share of rejected token draws per case
    share = {}
    for ci, name, cfg, s in mc.table_rows():
        acc = [a for c in tracked[ci, s][2].calls if c["phase"] in ("elements", "values") for a in c["accepted"]]
        tot = share.setdefault(name, [0, 0])
        tot[0] += len(acc) - sum(acc)
        tot[1] += len(acc)
    for name in ("reject_half_v34", "reject_half_v66", "reject_half_v1026"):
        assert 0.40 < share[name][0] / share[name][1] < 0.55, (name, share[name])
    for name in ("reject_none_v65", "v3"):
        assert share[name][0] == 0
    assert share["long_elements"][1] > 3 * 2 * 4000                # thousands of draws per element


def test_row_end_events_are_where_the_separator_lands(tracked):
    """row_end_plus_0 is exactly the rows whose labels end on a separator: the one store `p <= L` allows and `p < L` does
    not. In the other classes the last chunk's separator falls outside both outputs and one of its tokens is labels[L-1]."""
    for ci, name, cfg, s in mc.table_rows():
        f, lb, g = tracked[ci, s]
        L, sep = cfg["L"], cfg["V"] + 1
        assert (lb[L - 1] == sep) == (mc.row_end_excess(g, L) == 0), (name, s)


def test_value_ranges_at_the_int32_limit(golden):
    """V = 2^31 - 2: tokens and noise values stay below bit 31, the separator is INT32_MAX, and some noise value has bit 30
    set (a flag kept in bit 31 would be told apart from it)."""
    ci = [i for i, (name, _, _) in enumerate(mc.CASES) if name == "v_int32_limit"][0]
    V = mc.CASES[ci][1]["V"]
    top = 0
    for s in mc.CASES[ci][2]:
        f, lb = golden["row_%d_%d_features" % (ci, s)], golden["row_%d_%d_labels" % (ci, s)]
        assert f.min() >= 0 and lb.min() >= 1 and f.max() == lb.max() == V + 1 == 2 ** 31 - 1
        top = max(top, int(f[f <= V].max()))
        assert (f == 0).any() and (f[1:] != lb[:-1]).any()      # masked and noised tokens occur
    assert top >= 2 ** 30 and top <= V - 1


def test_the_overflow_searches_find_their_rows():
    """The start state the GPU overflow test uses exists, and is what it is meant to be."""
    cfg = mc.CHAIN_PTRS
    s = mc.chained_overflow_seed(cfg, mc.OVERFLOW_CAP, 2)
    rs = np.random.RandomState(s)
    V, n, l, e, L = mc.cfg_args(cfg)
    totals = []
    for _ in range(3):
        st = rs.get_state()
        totals.append(mc.element_total(rs, V, n, l))
        rs.set_state(st)
        mo.fast_row(rs, V, n, l, e, L)
    assert totals[0] <= mc.OVERFLOW_CAP and totals[1] <= mc.OVERFLOW_CAP < totals[2]
    assert mc.OVERFLOW_CAP >= 3 * n


def _params(**kw):
    from metagym_amd import _lib
    p = _lib.MetaLMParams()
    p.V, p.n, p.L, p.l, p.e, p.mask_ratio = 64, 10, 2048, 64.0, 0.1, 0.3
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_abi_lds_limit_to_the_byte():
    """2496 + 8 (n + element_capacity) == 160 KiB passes the size check (the call then stops at the next argument check, here
    seeds together with mt_state, so nothing is launched); one more token is MG_ERR_UNSUPPORTED. The accepted size is
    launched in test_metalm_edges_gpu.py."""
    from metagym_amd import _lib
    lib = _lib.load()
    fake = C.create_string_buffer(64)
    q = C.c_void_p(C.addressof(fake))
    gen = lib.mg_metalm_generate
    for n, cap in ((10, 20158), (2, 20166), (100, 20068)):
        assert 2496 + 8 * (n + cap) == 160 * 1024
        p = _params(n=n)
        assert gen(p, 4, 0, q, q, cap, q, q, q, None) == -1003 and b"exclusive" in lib.mg_last_error()
        assert gen(p, 4, 0, q, q, cap + 1, q, q, q, None) == -1004 and b"160 KiB" in lib.mg_last_error()
        assert gen(p, 4, 0, None, None, cap + 1, q, q, q, None) == -1004
    assert gen(_params(n=10), 4, 0, None, None, 2 ** 31 - 1, q, q, q, None) == -1004
