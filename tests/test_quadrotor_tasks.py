"""Quadrotor task table, host side (no GPU): mg_quadrotor_tasks_fold against the oracle's constants, its rejections, the
host randomiser, and the oracle-only precondition of the GPU test's tight-failure row."""
import ctypes as C
import json

import numpy as np
import pytest

import quadrotor_tasks_cases as qc
from oracle import quadrotor as qo


def _fold(cfg, ar=None):
    from metagym_amd import _lib
    lib = _lib.load()
    row = np.zeros(int(lib.mg_quadrotor_tasks_row_bytes()), np.uint8)
    rc = lib.mg_quadrotor_tasks_fold(cfg, ar, row.ctypes.data_as(C.c_void_p))
    if rc != 0:
        return rc, None
    out = _lib.QuadrotorTaskFold()
    assert lib.mg_quadrotor_tasks_describe(row.ctypes.data_as(C.c_void_p), out) == 0
    return 0, out


def _config(sim, dt=0.01):
    from metagym_amd import _lib
    from metagym_amd.quadrotor.env import _fill_config
    cfg = _lib.QuadrotorConfig()
    _fill_config(cfg, sim, dt, 1000, "hovering_control", 1.0)
    return cfg


def _sdot_norm(p):
    """np.linalg.norm of a float32 3-vector as OpenBLAS computes it: float32 products, double sum, float32 sqrt"""
    p = np.asarray(p, np.float32)
    q = p * p
    return np.sqrt(np.float32((np.float64(q[0]) + np.float64(q[1])) + np.float64(q[2])))


@pytest.mark.parametrize("name,times", [("stock", 10), ("custom", 5)])
def test_fold_matches_the_oracle_constants(name, times):
    from metagym_amd import _lib
    sim = qc.stock() if name == "stock" else json.load(open(qc.CUSTOM_CONF))
    ar = _lib.QuadrotorAutoReset()
    for i, ax in enumerate("xyz"):
        ar.init_velocity[i] = float(sim["init_velocity"][ax])
        ar.init_angular_velocity[i] = float(sim["init_angular_velocity"][ax])
    ar.init_velocity_noisy = float(sim["init_velocity"]["noisy"])
    ar.init_angular_velocity_noisy = float(sim["init_angular_velocity"]["noisy"])
    rc, d = _fold(_config(sim), ar)
    assert rc == 0
    i = sim["inertia"]
    inertia = np.array([[i["xx"], i["xy"], i["xz"]], [i["xy"], i["yy"], i["yz"]], [i["xz"], i["yz"], i["zz"]]], np.float32)
    want = qo.inv3(inertia).reshape(9)
    assert np.array_equal(np.array(d.inertia_inv[:], np.float32).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want, np.array(qo.consts_from_config(sim).inertia_inv[:], np.float32))
    assert d.times == times
    lm = [_sdot_norm([sim["propeller"][p][ax] for ax in "xyz"]) for p in range(4)]
    assert np.array_equal(np.array(d.lm[:], np.float32), np.array(lm, np.float32))
    p = float(sim["precision"])
    assert d.precision == p and d.half_dt2 == 0.5 * p * p and d.prec32 == np.float32(p) and d.dt == 0.01
    assert d.simple == (1 if name == "stock" else 0)
    T = np.float32(sim["fail"]["range"])
    S = np.float32(d.fail_range_sq32)
    assert np.sqrt(S) <= T and np.sqrt(np.nextafter(S, np.float32(np.inf))) > T
    # the init-noise block is carried through
    assert list(d.init_velocity) == [np.float32(sim["init_velocity"][ax]) for ax in "xyz"]
    assert list(d.init_angular_velocity) == [np.float32(sim["init_angular_velocity"][ax]) for ax in "xyz"]
    assert d.init_velocity_noisy == float(sim["init_velocity"]["noisy"])
    assert d.init_angular_velocity_noisy == float(sim["init_angular_velocity"]["noisy"])
    # no block: zeros
    rc, d0 = _fold(_config(sim), None)
    assert rc == 0 and list(d0.init_velocity) == [0.0] * 3 and d0.init_angular_velocity_noisy == 0.0


def test_fold_rejects_what_the_uniform_path_rejects():
    from metagym_amd import _lib
    lib = _lib.load()
    cfg = _config(qc.stock())
    cfg.precision = 0.02                                   # above dt (quadrotorsim.py:299-300)
    assert _fold(cfg)[0] == -1003 and b"precision" in lib.mg_last_error()
    cfg.precision = float("nan")
    assert _fold(cfg)[0] == -1003
    cfg.precision = 1e-9
    assert _fold(cfg)[0] == -1003
    cfg.precision = 0.001
    assert _fold(cfg)[0] == 0
    row = np.zeros(int(lib.mg_quadrotor_tasks_row_bytes()), np.uint8)
    assert lib.mg_quadrotor_tasks_fold(None, None, row.ctypes.data_as(C.c_void_p)) == -1001
    assert lib.mg_quadrotor_tasks_fold(cfg, None, None) == -1001
    assert lib.mg_quadrotor_tasks_describe(row.ctypes.data_as(C.c_void_p), _lib.QuadrotorTaskFold()) == -1003   # not a row
    # the launch validates on the host before it touches the device
    st, tk = _lib.QuadrotorState(), _lib.QuadrotorTasks()
    p = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert lib.mg_quadrotor_tasks_step(cfg, tk, 4, 1, st, None, p, p, None, None, p, None, None) == -1002   # n_tasks = 0
    tk.n_tasks = 2
    assert lib.mg_quadrotor_tasks_step(cfg, tk, 4, 1, st, None, p, p, None, None, p, None, None) == -1001   # no rows
    with pytest.raises(_lib.MetaGymHipError):
        from metagym_amd.quadrotor import QuadrotorTaskTable
        bad = qc.stock()
        bad["precision"] = 0.5
        QuadrotorTaskTable([qc.stock(), bad])


def test_sample_tasks_is_deterministic_and_spread_zero_is_the_base():
    from metagym_amd.quadrotor import QuadrotorTaskTable, sample_tasks
    a, b, c = sample_tasks(16, seed=3, spread=0.2), sample_tasks(16, seed=3, spread=0.2), sample_tasks(16, seed=4, spread=0.2)
    assert np.array_equal(a.rows, b.rows) and a.configs == b.configs
    assert not np.array_equal(a.rows, c.rows)
    assert len(set(r.tobytes() for r in a.rows)) == 16                     # sixteen different airframes
    base = QuadrotorTaskTable([qc.stock()])
    z = sample_tasks(7, seed=3, spread=0.0)
    assert z.rows.shape == (7, base.rows.shape[1]) and all(np.array_equal(r, base.rows[0]) for r in z.rows)
    zc = sample_tasks(3, seed=9, base=qc.CUSTOM_CONF, spread=0.0)
    assert all(np.array_equal(r, QuadrotorTaskTable([qc.CUSTOM_CONF]).rows[0]) for r in zc.rows)
    # the varied quantities stay inside the spread
    for cfg in a.configs:
        assert abs(cfg["quality"] / 0.5 - 1.0) <= 0.2 + 1e-12
        assert abs(cfg["propeller"][0]["x"] / 0.18 - 1.0) <= 0.2 + 1e-12


def test_table_accepts_dicts_and_json_paths(tmp_path):
    from metagym_amd.quadrotor import QuadrotorTaskTable
    p = tmp_path / "stock.json"
    p.write_text(json.dumps(qc.stock()))
    t = QuadrotorTaskTable([qc.stock(), str(p), qc.CUSTOM_CONF, json.load(open(qc.CUSTOM_CONF))])
    assert len(t) == 4 and t.num_tasks == 4
    assert np.array_equal(t.rows[0], t.rows[1]) and np.array_equal(t.rows[2], t.rows[3])
    assert not np.array_equal(t.rows[0], t.rows[2])
    assert [t.describe(v).times for v in range(4)] == [10, 10, 5, 5]
    assert [t.describe(v, dt=0.02).times for v in range(4)] == [20, 20, 10, 10]    # another env step: folded again
    assert t.init_velocity_noisy.tolist() == [2.0, 2.0, 1.5, 1.5]
    with pytest.raises(ValueError):
        QuadrotorTaskTable([])


def test_tight_row_fails_some_envs_and_not_others():
    """The precondition of the GPU test's mixed table, from the oracle alone: inside the T steps the tight-threshold row
    holds envs that fail (with every failure code) and envs that do not, on both tasks it is run on."""
    ids = qc.mixed_ids()
    acts = qc.mixed_actions()
    for task, kw in ((qo.TASK_HOVERING, {}), (qo.TASK_NO_COLLISION, dict(map_matrix=_cleared(qc.small_map()), offsets=(5, 5)))):
        og = qc.OracleGroups(qc.mixed_configs(), ids, qc.random_batch(qc.N, qc.STATE_SEED), task=task, **kw)
        codes = np.zeros(qc.N, int)
        for t in range(qc.T):
            f = og.step(acts[t])[3]
            codes = np.where(codes == 0, f, codes)
        tight = codes[ids == 4]
        assert (tight != 0).any() and (tight == 0).any()
        assert set(tight.tolist()) == {0, 1, 2, 3}
        assert (codes[ids != 4] == 0).all()                # the stock thresholds are far away


def _cleared(grid):
    g = grid.copy()
    g[g == -1] = 0
    return g
