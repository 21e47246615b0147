"""Quadrotor task tables: one simulator config (the reference's config.json schema) per task, folded into the rows that
`mg_quadrotor_tasks_step` reads (include/metagym_hip.h). `Quadrotor.set_task(table, task_ids)` then steps a batch in
which every env flies its own airframe, in one launch.

    table = sample_tasks(256, seed=0, spread=0.2)          # 256 airframes around the stock one
    env.set_task(table)                                    # env e flies task e % 256
"""
import copy
import ctypes as C
import json

import numpy as np

from .. import _lib
from .env import DEFAULT_SIM_CONFIG, _fill_config


def _load_config(c):
    if isinstance(c, dict):
        return copy.deepcopy(c)
    with open(c, "r") as f:
        return json.load(f)


def _init_block(sim):
    """The init-noise block of one config, with the reference's guard (quadrotorsim.py:241-254: both blocks sit behind
    `init_velocity`): (velocity base[3], velocity noisy, body-rate base[3], body-rate noisy)."""
    cv = sim.get("init_velocity")
    cw = sim.get("init_angular_velocity") if cv is not None else None
    vb = [float(cv[ax]) for ax in "xyz"] if cv else [0.0] * 3
    wb = [float(cw[ax]) for ax in "xyz"] if cw else [0.0] * 3
    return vb, (float(cv["noisy"]) if cv else 0.0), wb, (float(cw["noisy"]) if cw else 0.0)


class QuadrotorTaskTable(object):
    """V simulator configs, folded on the host (no GPU is touched until `.to(device)`).

    Args:
        configs: list of dicts or JSON paths in the config.json schema (see `DEFAULT_SIM_CONFIG`).
        dt: the env step the rows are folded for (sub-steps per step = int(dt / precision), per task). An env with
            another dt folds the configs again when the table is set.
    A config the library rejects (precision outside [1e-8, dt], ...) raises `MetaGymHipError`.
    """

    def __init__(self, configs, dt=0.01):
        configs = list(configs)
        if len(configs) == 0:
            raise ValueError("a task table needs at least one config")
        self.configs = [_load_config(c) for c in configs]
        self.dt = float(dt)
        self._folded = {}      # dt -> (rows uint8 [V, row_bytes], all_simple)
        self._device = {}      # (device, dt) -> torch uint8 [V, row_bytes]
        blocks = [_init_block(c) for c in self.configs]
        self.init_velocity = np.array([b[0] for b in blocks], np.float32)            # [V, 3]
        self.init_velocity_noisy = np.array([b[1] for b in blocks], np.float64)      # [V]
        self.init_angular_velocity = np.array([b[2] for b in blocks], np.float32)
        self.init_angular_velocity_noisy = np.array([b[3] for b in blocks], np.float64)
        self.fold(self.dt)

    def __len__(self):
        return len(self.configs)

    @property
    def num_tasks(self):
        return len(self.configs)

    def config_struct(self, v, dt, nt=1000, task="hovering_control", healthy_reward=1.0):
        """mg_quadrotor_config of task v (per-task fields from its config, the rest from the arguments)."""
        cfg = _lib.QuadrotorConfig()
        _fill_config(cfg, self.configs[v], dt, nt, task, healthy_reward)
        return cfg

    def fold(self, dt):
        """(rows, all_simple) for an env step of `dt`: uint8 [V, row_bytes] host array, folded once per dt."""
        dt = float(dt)
        if dt not in self._folded:
            lib = _lib.load()
            nb = int(lib.mg_quadrotor_tasks_row_bytes())
            rows = np.zeros((len(self.configs), nb), np.uint8)
            simple = True
            for v in range(len(self.configs)):
                ar = _lib.QuadrotorAutoReset()
                for i in range(3):
                    ar.init_velocity[i] = float(self.init_velocity[v, i])
                    ar.init_angular_velocity[i] = float(self.init_angular_velocity[v, i])
                ar.init_velocity_noisy = float(self.init_velocity_noisy[v])
                ar.init_angular_velocity_noisy = float(self.init_angular_velocity_noisy[v])
                rc = lib.mg_quadrotor_tasks_fold(self.config_struct(v, dt), ar, rows[v].ctypes.data_as(C.c_void_p))
                _lib.check(rc, "mg_quadrotor_tasks_fold (task %d)" % v)
                simple = simple and bool(self.describe(v, rows=rows).simple)
            self._folded[dt] = (rows, simple)
        return self._folded[dt]

    @property
    def rows(self):
        return self.fold(self.dt)[0]

    def describe(self, v, dt=None, rows=None):
        """mg_quadrotor_task_fold of row v."""
        if rows is None:
            rows = self.fold(self.dt if dt is None else dt)[0]
        out = _lib.QuadrotorTaskFold()
        rc = _lib.load().mg_quadrotor_tasks_describe(rows[v].ctypes.data_as(C.c_void_p), out)
        _lib.check(rc, "mg_quadrotor_tasks_describe")
        return out

    def to(self, device, dt=None):
        """Upload the rows (once per device and dt). Returns self."""
        self.device_rows(device, self.dt if dt is None else dt)
        return self

    def device_rows(self, device, dt):
        import torch
        device = _lib.canonical_device(device)
        key = (str(device), float(dt))
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.fold(dt)[0]).to(device).contiguous()
        return self._device[key]


def _scaled(x, f):
    return float(x) * f


def sample_tasks(num_tasks, seed, base=None, spread=0.1, dt=0.01):
    """`num_tasks` airframes around `base` (a dict or JSON path; None = the stock config), drawn on the host from
    `RandomState(seed)`: mass, the three diagonal inertias, the thrust polynomial CT, the drag coefficients and the arm
    length are each multiplied by 1 + spread * U(-1, 1) (seven draws per task). The same arguments give the same table;
    `spread=0` gives `num_tasks` rows that equal the base bit for bit."""
    if not (0.0 <= float(spread) < 1.0):
        raise ValueError("spread must be in [0, 1)")
    base = _load_config(DEFAULT_SIM_CONFIG if base is None else base)
    u = np.random.RandomState(seed).uniform(-1.0, 1.0, (int(num_tasks), 7))
    f = 1.0 + float(spread) * u
    configs = []
    for v in range(int(num_tasks)):
        c = copy.deepcopy(base)
        c["quality"] = _scaled(c["quality"], f[v, 0])
        for j, key in enumerate(("xx", "yy", "zz")):
            c["inertia"][key] = _scaled(c["inertia"][key], f[v, 1 + j])
        c["thrust"]["CT"] = [_scaled(x, f[v, 4]) for x in c["thrust"]["CT"]]
        for key in ("m_xx", "m_yy", "m_zz", "f_xx", "f_yy", "f_zz"):
            c["drag"][key] = _scaled(c["drag"][key], f[v, 5])
        c["propeller"] = [{ax: _scaled(p[ax], f[v, 6]) for ax in "xyz"} for p in c["propeller"]]
        configs.append(c)
    return QuadrotorTaskTable(configs, dt=dt)
