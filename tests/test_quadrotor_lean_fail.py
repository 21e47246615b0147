"""The failure tests that the one-wave stock step folds into its range window (fold_lean, csrc/quadrotor.hip), checked
on the host through mg_quadrotor_plan_fold, which needs no GPU.

The one-wave form holds no failure test in its sub-steps. A lane stays on its main path, which reports failed = 0, only
while the high word of |v|^2 and of |w|^2 is below the plan's edge and no |p_c| reaches pos_safe32. So for every plan
that folds:
  * for doubles x just below an edge, in both words, sqrt(x) <= threshold: such a lane does not fail that test;
  * the edge is not above threshold^2 * (1 - 2^-19) nor 2^233, and base = edge - span is not below 2^-767;
  * for float32 triples with max-norm just below pos_safe32 (all three equal included), the kernel's sum of squares
    (f32 products, two f64 adds, one f32 rounding) is at most fail_range_sq32: such a lane does not fail the range test;
  * the largest m below pos_safe32 has 3 * m^2 * (1 + 2^-20) <= fail_range_sq32 in double, and pos_safe32 is close to
    range / sqrt(3), so that the fold does not send ordinary states through the fallback.
Thresholds that cannot be folded report the straight-line stock form, which keeps the tests in its sub-steps."""
import ctypes as C
import struct

import numpy as np
import pytest

F32 = np.float32
STOCK = dict(fail_velocity=100.0, fail_w=1000.0, fail_range=1000.0)
HI_2M767, HI_2P233, HI_2P1 = 256 << 20, (1023 + 233) << 20, 1024 << 20


def _fold(ct0=None, arm=None, **thresholds):
    """mg_quadrotor_fold of a plan for the stock configuration with fused auto-reset and the given thresholds."""
    from metagym_amd import _lib
    lib = _lib.load()
    cfg = _lib.QuadrotorConfig()
    assert lib.mg_quadrotor_default_config(cfg) == 0
    for k, v in dict(STOCK, **thresholds).items():
        setattr(cfg, k, v)
    if ct0 is not None:
        cfg.ct0 = ct0
    if arm is not None:                          # the stock X frame with another arm coordinate c
        for i, (sx, sy) in enumerate(((1, 1), (-1, 1), (-1, -1), (1, -1))):
            cfg.prop_coord[3 * i], cfg.prop_coord[3 * i + 1] = sx * arm, sy * arm
    st = _lib.QuadrotorState()
    fake = C.create_string_buffer(64)           # host-only: the plan records the pointers and launches nothing
    for name, _ in _lib.QuadrotorState._fields_:
        setattr(st, name, C.addressof(fake))
    plan, ar, out = _lib.QuadrotorPlan(), _lib.QuadrotorAutoReset(), _lib.QuadrotorFold()
    assert lib.mg_quadrotor_plan_init(plan, cfg, ar, 256, st) == 0
    assert lib.mg_quadrotor_plan_fold(plan, out) == 0
    return out


def _double(hi, lo):
    return struct.unpack("<d", struct.pack("<Q", (hi << 32) | lo))[0]


def _sumsq3(p):
    """sumsq3(const float *) of csrc/quadrotor.hip: np.linalg.norm(f32[3])^2 as OpenBLAS sdot computes it."""
    p = np.asarray(p, F32)
    q = p * p
    return F32((np.float64(q[0]) + np.float64(q[1])) + np.float64(q[2]))


NORM_THRESHOLDS = [100.0, 1000.0, 1.5, 2.0, 3.0, 7.25, 12.345678, 99.99999, 4096.0, 1e5, 3.3e7, 1e12, 1e30, 1.1e35,
                   1.2e35, 1e100, 1e150, 1e200, 1.7e308, float("inf")]   # 2^233 is the square of 1.17e35


@pytest.mark.parametrize("thr", NORM_THRESHOLDS)
@pytest.mark.parametrize("key", ["fail_velocity", "fail_w"])
def test_norm_edges(key, thr):
    f = _fold(**{key: thr})
    assert f.one_wave_form == 2
    edge, base = (f.edge_v, f.base_v) if key == "fail_velocity" else (f.edge_w, f.base_w)
    assert f.span == 768 << 20 and base == edge - f.span
    assert HI_2M767 <= base and HI_2P1 <= edge <= HI_2P233
    assert _double(edge, 0) <= np.square(np.float64(min(thr, 1e150))) * (1.0 - 2.0 ** -19)
    # doubles just below the edge: the last high words with low words at both ends and in between
    for hi in (edge - 1, edge - 2, edge - 1000):
        for lo in (0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 1, 0):
            assert np.sqrt(np.float64(_double(hi, lo))) <= thr, (hi, lo)
    assert np.sqrt(np.float64(_double(edge, 0))) <= thr
    if thr < 1.1e35:   # below the 2^233 clamp the edge wastes little: within 2^-18 of the threshold's square
        assert _double(edge + 1, 0) > thr * thr * (1.0 - 2.0 ** -18)
    stock = _fold()                                      # the other test keeps its own edge
    assert (f.edge_w == stock.edge_w) if key == "fail_velocity" else (f.edge_v == stock.edge_v)


def test_stock_edges():
    f = _fold()
    assert f.one_wave_form == 2
    assert (f.fail_velocity, f.fail_w) == (100.0, 1000.0)
    assert f.edge_v == struct.unpack("<Q", struct.pack("<d", 1e4 * (1 - 2.0 ** -19)))[0] >> 32
    assert f.edge_w == struct.unpack("<Q", struct.pack("<d", 1e6 * (1 - 2.0 ** -19)))[0] >> 32
    assert abs(float(f.pos_safe32) - 1000.0 / np.sqrt(3.0)) < 1e-2


RANGES = [1000.0, 1.0, 0.75, 3.0, 1e-3, 1e-12, 2.0 ** -49, 17.5, 123456.789, 1e10, 1e18, 1.8e19]


@pytest.mark.parametrize("rng", RANGES)
def test_pos_safe(rng):
    f = _fold(fail_range=rng)
    assert f.one_wave_form == 2
    S, P = F32(f.fail_range_sq32), F32(f.pos_safe32)
    assert np.sqrt(S) <= F32(rng) < np.sqrt(np.nextafter(S, F32(np.inf)))      # S is the range test's own threshold
    assert P > 0 and P >= np.finfo(F32).tiny
    below = [P]
    for _ in range(4):
        below.append(np.nextafter(below[-1], F32(0)))
    below = below[1:]                                    # the four floats just below pos_safe32
    m = below[0]
    assert 3.0 * (float(m) * float(m)) * (1.0 + 2.0 ** -20) <= float(S)
    assert float(P) > float(F32(rng)) / np.sqrt(3.0) * (1.0 - 1e-5)             # and not needlessly small
    rs = np.random.RandomState(5)
    with np.errstate(over="raise"):
        for m in below:
            triples = [(m, m, m), (-m, m, -m), (m, 0, 0), (0, -m, 0), (m, m, 0), (m, np.nextafter(m, F32(0)), m)]
            triples += [tuple(m * s * F32(u) for s, u in zip(rs.choice([-1, 1], 3), (1, rs.uniform(), rs.uniform())))
                        for _ in range(50)]
            for t in triples:
                assert max(abs(F32(c)) for c in t) <= m
                assert _sumsq3(t) <= S, (t, S)
    # and the fold is tight to a few parts in 10^5: a little above pos_safe32 the equal triple does fail
    over = F32(float(P) * (1.0 + 1e-4))
    assert _sumsq3((over, over, over)) > S


UNFOLDABLE = [dict(fail_velocity=v) for v in (-1.0, -0.0, 0.0, float("nan"), 1e-200, 1.0, 1.41)]
UNFOLDABLE += [dict(fail_w=v) for v in (-1.0, -0.0, 0.0, float("nan"), 1e-200, 1.0, 1.41)]
UNFOLDABLE += [dict(fail_range=v) for v in (-1.0, -0.0, 0.0, float("nan"), float("inf"), 1e39, 1e-16, 1e-30)]


@pytest.mark.parametrize("over", UNFOLDABLE, ids=lambda d: "%s=%r" % next(iter(d.items())))
def test_unfoldable_thresholds_keep_the_full_tests(over):
    f = _fold(**over)
    assert f.one_wave_form == 1
    assert (f.base_v, f.base_w, f.edge_v, f.edge_w, f.pos_safe32) == (0, 0, 0, 0, 0.0)


def test_thrust_coefficient_condition():
    """substep<FAST> reuses products on the strength of ct0_32 > 0 (thrust is never -0.0)."""
    assert _fold(ct0=0.0).one_wave_form == 1
    assert _fold(ct0=-1.538e-5).one_wave_form == 1
    assert _fold(ct0=1.538e-5).one_wave_form == 2


def test_arm_length_condition():
    """substep<XF, FAST> states lm > 0; an X frame whose c * c underflows in float32 has lm = 0 and keeps the full tests."""
    assert _fold(arm=0.25).one_wave_form == 2
    assert _fold(arm=1e-30).one_wave_form == 1


def test_flt_max_range_folds():
    f = _fold(fail_range=float(np.finfo(F32).max))
    # sqrt(FLT_MAX)^2 overflows float32, so fold_config's search ends at S = FLT_MAX: finite, and it folds
    assert f.one_wave_form == 2 and np.isfinite(f.fail_range_sq32) and f.pos_safe32 > 1e18


def test_generic_plan_reports_generic(monkeypatch):
    monkeypatch.setenv("MG_QUAD_GENERIC", "1")
    assert _fold().one_wave_form == 0
