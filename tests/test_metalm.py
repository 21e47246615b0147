"""meta-lm-v0 without a GPU: both host restatements (tests/metalm_oracle.py) against the reference's own rows
(tests/golden/metalm.npz), the refill boundary crossed in every phase of a row, the C ABI's argument checks, the registry
entry and the refusal of a CPU device. The device kernel is compared with the same goldens in test_metalm_gpu.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import metalm_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metalm.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _cfg_args(cfg):
    return cfg["V"], cfg["n"], cfg["l"], cfg["e"], cfg["L"]


def test_draw_level_restatement_reproduces_every_golden_row(golden):
    cases = json.loads(str(golden["cases"]))
    for ci, s in golden["rows"]:
        g = mo.MTStream.seeded(s)
        f, lb = mo.draw_level_row(g, *_cfg_args(cases[ci]))
        assert np.array_equal(f, golden["row_%d_%d_features" % (ci, s)]), (cases[ci], s)
        assert np.array_equal(lb, golden["row_%d_%d_labels" % (ci, s)]), (cases[ci], s)


def test_fast_restatement_reproduces_every_golden_row(golden):
    cases = json.loads(str(golden["cases"]))
    for ci, s in golden["rows"]:
        f, lb = mo.fast_row(np.random.RandomState(s), *_cfg_args(cases[ci]))
        assert np.array_equal(f, golden["row_%d_%d_features" % (ci, s)]), (cases[ci], s)
        assert np.array_equal(lb, golden["row_%d_%d_labels" % (ci, s)]), (cases[ci], s)


def test_both_restatements_reproduce_the_reference_batches_and_final_state(golden):
    for bi, (cfg, s, B) in enumerate(json.loads(str(golden["batches"]))):
        g = mo.MTStream.seeded(s)
        f, lb = mo.draw_level_batch(g, B, *_cfg_args(cfg))
        assert np.array_equal(f, golden["batch_%d_features" % bi]) and np.array_equal(lb, golden["batch_%d_labels" % bi])
        assert np.array_equal(g.key, golden["batch_%d_key" % bi]) and g.pos == int(golden["batch_%d_pos" % bi])
        rs = np.random.RandomState(s)
        f, lb = mo.fast_batch(rs, B, *_cfg_args(cfg))
        assert np.array_equal(f, golden["batch_%d_features" % bi]) and np.array_equal(lb, golden["batch_%d_labels" % bi])
        st = rs.get_state()
        assert np.array_equal(st[1], golden["batch_%d_key" % bi]) and st[2] == int(golden["batch_%d_pos" % bi])
        assert rs.random_sample() == float(golden["batch_%d_next_random" % bi])


def test_text_format_matches_the_reference(golden):
    cfg, s, B = json.loads(str(golden["text_case"]))
    f, lb = mo.fast_batch(np.random.RandomState(s), B, *_cfg_args(cfg))
    assert mo.to_text(f, lb) == str(golden["text"])


def test_golden_rows_cross_the_refill_in_every_phase(golden):
    """The rows the GPU test compares cross a 624-word refill inside every part of the row program, including a double
    whose two draws straddle it, so the kernel's boundary handling is exercised in each."""
    cases = json.loads(str(golden["cases"]))
    seen = set()
    for ci, s in golden["rows"]:
        g = mo.MTStream.seeded(s)
        mo.draw_level_row(g, *_cfg_args(cases[ci]))
        seen.update(g.refills)
    for phase in ("poisson", "elements", "choice", "values", "noise", "mask", "noise/straddle", "mask/straddle",
                  "poisson/straddle"):
        assert phase in seen, (phase, sorted(map(str, seen)))


def _params(**kw):
    from metagym_amd import _lib
    p = _lib.MetaLMParams()
    p.V, p.n, p.L, p.l, p.e, p.mask_ratio = 64, 10, 2048, 64.0, 0.1, 0.3
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_abi_argument_errors_are_codes():
    from metagym_amd import _lib
    lib = _lib.load()
    fake = C.create_string_buffer(64)
    q = C.c_void_p(C.addressof(fake))
    ok = _params()
    gen = lib.mg_metalm_generate
    assert gen(None, 4, 0, None, None, 1360, q, q, q, None) == -1001
    for i in range(3):
        args = [q, q, q]
        args[i] = None
        assert gen(ok, 4, 0, None, None, 1360, *args, None) == -1001 and b"NULL" in lib.mg_last_error()
    assert gen(ok, 0, 0, None, None, 1360, q, q, q, None) == -1002
    # the reference's assert: n > 1 and V > 1 and l > 1 and e > 0 and e < 1 and L > 1
    for bad in (dict(n=1), dict(V=1), dict(l=1.0), dict(l=float("nan")), dict(l=float("inf")), dict(e=0.0), dict(e=1.0),
                dict(L=1), dict(V=2 ** 31 - 1)):
        assert gen(_params(**bad), 4, 0, None, None, 1360, q, q, q, None) == -1003, bad
    assert b"V + 1 < 2^31" in lib.mg_last_error()
    assert gen(ok, 4, 0, None, None, 29, q, q, q, None) == -1002 and b"3 n" in lib.mg_last_error()
    assert gen(ok, 4, 0, None, None, 21000, q, q, q, None) == -1004 and b"160 KiB" in lib.mg_last_error()
    assert gen(ok, 4, 0, q, q, 1360, q, q, q, None) == -1003 and b"exclusive" in lib.mg_last_error()


def test_default_capacity_fits_the_lds_budget_for_the_reference_defaults():
    from metagym_amd.metalm import default_element_capacity
    cap = default_element_capacity(10, 64)
    assert cap == 10 * 136
    assert 2496 + 8 * (10 + cap) <= 160 * 1024


def test_registry_entry_has_the_reference_kwargs():
    import metagym_amd
    entry_point, kwargs = metagym_amd.registry["meta-lm-v0"]
    assert entry_point == "metagym_amd.metalm:MetaLM"
    assert kwargs == {"V": 64, "n": 10, "l": 64, "e": 0.10, "L": 2048}


def test_cpu_device_is_refused():
    import metagym_amd
    from metagym_amd._lib import MetaGymHipError
    with pytest.raises(MetaGymHipError):
        metagym_amd.make("meta-lm-v0", device="cpu")
    from metagym_amd.metalm import MetaLM
    with pytest.raises(AssertionError):
        MetaLM(e=1.0)
