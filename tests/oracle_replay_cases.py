"""Case writer of tests/test_oracle_replay.py: serialises the inputs the ctypes front ends of the C oracles take
(oracle/quadrotor.py, oracle/maze.py, oracle/walker_c.py) into the case file oracle/replay_main.c reads, and computes
what the front ends return for the same inputs, in the layout of the replay's result file. A helper module, no test.

A `Call` is one call of the replay program: its op, its input blobs, and `expect()`, which runs the same inputs through
the ctypes front end and returns the output blobs in the replay's order. Structs travel as the raw bytes of the ctypes
structures with their pointer members cleared; the replay sets them again (file format: top of oracle/replay_main.c).
No file of cases is committed: everything is built from tests/golden/ and the case modules the GPU edge tests use
(test_quadrotor_edges, quadrotor_tasks_cases, maze_cont_cases, maze_large_cases, walker_cases, walker_fixtures)."""
import ctypes as C
import glob
import json
import os
import struct

import numpy as np

from oracle import maze as mo
from oracle import quadrotor as qo
from oracle import walker_c as wc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Q_STEP, Q_VEL_STEP, Q_VEL_TARGETS, Q_DEFAULTS, Q_INV3, Q_PHILOX, Q_RESET_NOISE, Q_OBSERVE, Q_BATCH_RUN = range(1, 10)
M_EPISODE, M_VIEW = 16, 17
W_EPISODE, W_SUBSTEP, W_RUN = 32, 33, 34
NAN, INF = float("nan"), float("inf")


class Call(object):
    def __init__(self, name, op, blobs, expect, nan=False, int_tail=None):
        """nan: the inputs hold a NaN or an infinity, so outputs can hold a NaN (its sign and payload are the compiler's choice
        of operand order). int_tail(k, n_blobs) -> how many trailing bytes of output blob k are integers (-1: all of it), for
        the calls with `nan`: a comparison that forgives the bits of a NaN must not forgive an integer that looks like one."""
        self.name, self.op, self.blobs, self.expect, self.nan = name, op, [bytes(b) for b in blobs], expect, nan
        self.int_tail = int_tail

    def __repr__(self):
        return self.name


def _pad(b):
    return b + b"\0" * (-len(b) % 8)


def write_cases(path, calls):
    with open(path, "wb") as f:
        f.write(b"MGRPLY01" + struct.pack("<II", len(calls), 0))
        for c in calls:
            f.write(struct.pack("<II", c.op, len(c.blobs)))
            for b in c.blobs:
                f.write(struct.pack("<Q", len(b)) + _pad(b))


def read_results(path):
    """-> [(op, [blob bytes, ...]) per call]"""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:8] == b"MGRRES01", data[:8]
    n_calls, _ = struct.unpack_from("<II", data, 8)
    at, out = 16, []
    for _ in range(n_calls):
        op, nb = struct.unpack_from("<II", data, at)
        at += 8
        blobs = []
        for _ in range(nb):
            n, = struct.unpack_from("<Q", data, at)
            blobs.append(data[at + 8:at + 8 + n])
            at += 8 + n + (-n % 8)
        out.append((op, blobs))
    assert at == len(data)
    return out


def _ints(*v):
    return np.asarray(v, np.int64).tobytes()


def _raw(s, clear=()):
    """The bytes of a ctypes structure (or array of them) with the named pointer members cleared."""
    c = type(s).from_buffer_copy(s)
    for f in clear:
        setattr(c, f, None)
    return bytes(c)


def _clone(s):
    return type(s).from_buffer_copy(s)


def _non_finite(*arrays):
    return any(not np.isfinite(np.asarray(a, np.float64)).all() for a in arrays)


def _b(a, dtype):
    return b"" if a is None else np.ascontiguousarray(a, dtype).tobytes()


# ---- quadrotor ------------------------------------------------------------------------------------------------------------

_Q_PTRS = ("map", "velocity_targets")


def _q_consts(c, grid, vt):
    """A copy of `c` whose pointers name `grid` / `vt` (returned too: they have to stay alive)."""
    c = _clone(c)
    grid = None if grid is None else np.ascontiguousarray(grid, np.int32)
    vt = None if vt is None else np.ascontiguousarray(vt, np.float32)
    c.map = None if grid is None else grid.ctypes.data_as(C.POINTER(C.c_int32))
    c.velocity_targets = None if vt is None else vt.ctypes.data_as(C.POINTER(C.c_float))
    if grid is not None:
        c.map_h, c.map_w = grid.shape
    return c, grid, vt


def q_step(name, consts, states, ct, actions, legacy=0, ar=None, episode=None, grid=None, vt=None):
    """T x qo.batch_env_step (ar None) or qo.batch_env_step_autoreset on n envs; actions [T, n, 4]."""
    consts, grid, vt = _q_consts(consts, grid, vt)
    actions = np.ascontiguousarray(actions, np.float32)
    T, n = actions.shape[:2]
    ct = np.ascontiguousarray(ct, np.int32)
    episode = None if ar is None else np.ascontiguousarray(episode, np.uint32)
    states = _clone(states)
    blobs = [_ints(n, T, legacy, int(ar is not None)), _raw(consts, _Q_PTRS), _b(grid, np.int32), _b(vt, np.float32), bytes(states),
             ct.tobytes(), actions.tobytes(), b"" if ar is None else bytes(ar), _b(episode, np.uint32)]

    def expect(keep=(grid, vt)):
        st, c, ep, out = _clone(states), ct.copy(), None if episode is None else episode.copy(), []
        qo.lib().qo_set_legacy_promotion(legacy)
        try:
            for a in actions:
                r = qo.batch_env_step(consts, st, c, a) if ar is None else qo.batch_env_step_autoreset(consts, ar, st, c, ep, a)
                out += [x.tobytes() for x in r]
        finally:
            qo.lib().qo_set_legacy_promotion(0)
        return out + [bytes(st), c.tobytes(), b"" if ep is None else ep.tobytes()]

    def int_tail(k, n_blobs):            # per step obs, reward, done (i32), failed (i32); then the states, ct (i32), episode (u32)
        return -1 if (k % 4 >= 2 if k < 4 * T else k > 4 * T) else 0
    return Call(name, Q_STEP, blobs, expect, nan=bool(np.isnan(actions).any()) or _non_finite(*qo.states_to_arrays(states).values()),
                int_tail=int_tail)


def _golden_states(g, prefix="init_", one=True):
    f = (lambda k: g[prefix + k][None]) if one else (lambda k: g[prefix + k])
    return qo.make_states(f("pos"), f("vel"), f("omega"), f("propw"), f("R"))


def _custom_config():
    with open(os.path.join(GOLDEN, "quadrotor_custom_config.json")) as f:
        return json.load(f)


def _special_states(n, seed):
    """quadrotor_tasks_cases.random_batch with NaN, +-inf and huge values written into one field of every second env."""
    import quadrotor_tasks_cases as qt
    pos, vel, omega, propw, R = qt.random_batch(n, seed)
    specials = (NAN, INF, -INF, 1e30, -1e30, 3e38)
    fields = (pos, vel, omega, propw, R)
    for e in range(0, n, 2):
        f = fields[(e // 2) % 5]
        f[e, (e // 10) % f.shape[1]] = specials[(e // 2) % len(specials)]
    return pos, vel, omega, propw, R


def quadrotor_calls():
    import quadrotor_tasks_cases as qt
    import test_quadrotor_edges as qe
    calls = []
    # the committed goldens: rollouts (one of them, and the custom config, in the numpy 1.22 reading too), single steps, failures
    for path in sorted(glob.glob(os.path.join(GOLDEN, "quadrotor_traj_*.npz"))):
        g = np.load(path)
        base = os.path.basename(path)[:-4]
        c = qo.consts_from_config(_custom_config(), nt=int(g["nt"])) if "_custom_" in base else qo.default_consts(nt=int(g["nt"]))
        for legacy in ((0, 1) if ("short" in base or "custom" in base) else (0,)):
            calls.append(q_step("%s legacy=%d" % (base, legacy), c, _golden_states(g), np.zeros(1, np.int32), g["actions"][:, None],
                                legacy=legacy))
    for name in ("quadrotor_onestep", "quadrotor_fail"):
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        st = _golden_states(g, "in_", one=False)
        calls.append(q_step(name, qo.default_consts(), st, np.zeros(len(st), np.int32), g["actions"][None]))
    g = np.load(os.path.join(GOLDEN, "quadrotor_edges.npz"))
    for i in range(len(g["code"])):
        c = qe.case_consts(**{k: float(g[k][i]) for k in qe.THRESHOLDS})
        st = qo.make_states(*[g["in_" + k][i:i + 1] for k in ("pos", "vel", "omega", "propw", "R")])
        calls.append(q_step("quadrotor_edges[%d]" % i, c, st, np.zeros(1, np.int32), g["actions"][i:i + 1][None]))
    g = np.load(os.path.join(GOLDEN, "quadrotor_no_collision_map.npz"))
    grid = np.array(g["map"], np.int32)
    ys, xs = np.where(grid == -1)
    grid[ys[0], xs[0]] = 0
    for k in range(3):
        c = qo.default_consts(nt=int(g["nt"]), task=qo.TASK_NO_COLLISION)
        c.x_offset, c.y_offset = int(xs[0]), int(ys[0])
        st = qo.make_states(np.zeros((1, 3), np.float32), g["init_vel_%d" % k][None], g["init_omega_%d" % k][None],
                            np.zeros((1, 4), np.float32), np.eye(3, dtype=np.float32).reshape(1, 9))
        calls.append(q_step("no_collision_map[%d]" % k, c, st, np.zeros(1, np.int32), g["actions_%d" % k][:, None], grid=grid))
    # velocity_control: the target trajectory, then the golden rollout across ct == nt
    g = np.load(os.path.join(GOLDEN, "quadrotor_velocity_control.npz"))
    nt = int(g["nt"])
    c = qo.default_consts(nt=nt, task=qo.TASK_VELOCITY)
    c.x_offset = c.y_offset = 0
    c.z_offset = 0.0
    tacts = qo.velocity_target_actions(int(g["seed"]), nt)
    calls.append(Call("velocity_targets", Q_VEL_TARGETS, [_ints(nt), _raw(c, _Q_PTRS), tacts.tobytes()],
                      lambda c=c, tacts=tacts: [qo.velocity_targets(c, tacts).tobytes()]))
    targets = qo.velocity_targets(c, tacts)
    cv, _, targets = _q_consts(c, None, targets)
    st = qo.make_states(np.zeros((1, 3), np.float32), g["init_vel"][None], g["init_omega"][None], np.zeros((1, 4), np.float32),
                        np.eye(3, dtype=np.float32).reshape(1, 9))
    vacts = np.ascontiguousarray(g["actions"], np.float32)

    def expect_velocity(cv=cv, st=st, vacts=vacts, keep=targets):
        s, ct, out = _clone(st), C.c_int(0), []
        for a in vacts:
            obs, r, d, f = qo.env_step_velocity(cv, s[0], ct, a)
            out += [obs.tobytes(), struct.pack("<d", r), struct.pack("<i", int(d)), struct.pack("<i", f)]
        return out + [bytes(s), struct.pack("<i", ct.value)]
    calls.append(Call("velocity_control rollout", Q_VEL_STEP, [_ints(len(vacts)), _raw(cv, _Q_PTRS), b"", targets.tobytes(), bytes(st),
                                                               struct.pack("<i", 0), vacts.tobytes()], expect_velocity))
    # the threshold boundaries of tests/test_quadrotor_edges.py (both sides), its special thresholds and clamp actions
    for name in sorted(qe.BOUNDARY):
        x, a = qe.boundary_env(name)
        for side, over in zip(("fails", "passes"), qe.boundary_sides(name)):
            st = qo.make_states(x["pos"], x["vel"], x["omega"], x["propw"], x["R"])
            calls.append(q_step("boundary %s %s" % (name, side), qe.case_consts(**over), st, np.zeros(1, np.int32), a[None]))
    n = 24
    ar = qo.default_autoreset(seed=5, env_id_base=3)
    for r, v, w in qe.SPECIAL:
        st = qo.make_states(*qt.random_batch(n, 202))
        acts = np.random.RandomState(203).uniform(0.1, 15.0, (3, n, 4)).astype(np.float32)
        calls.append(q_step("thresholds %r %r %r" % (r, v, w), qe.case_consts(fail_range=r, fail_velocity=v, fail_w=w), st,
                            np.zeros(n, np.int32), acts, ar=ar, episode=np.zeros(n, np.uint32)))
    clamp = np.asarray(qe.CLAMP, np.float32)
    acts = clamp[(np.arange(2 * n * 4).reshape(2, n, 4) * 5) % len(clamp)]
    for lo, hi in ((0.10, 15.0), (2.0, 2.0)):
        c = qo.default_consts()
        c.min_voltage, c.max_voltage = lo, hi
        calls.append(q_step("clamp actions %r..%r" % (lo, hi), c, qo.make_states(*qt.random_batch(n, 303)), np.zeros(n, np.int32), acts))
    # the mixed task table of tests/quadrotor_tasks_cases.py, row by row; the last row once more on the small map with offsets
    # that put half the batch at negative map indices (python's slices wrap there), task no_collision
    state, ids, macts = qt.random_batch(qt.N, qt.STATE_SEED), qt.mixed_ids(), qt.mixed_actions()
    for v, cfg in enumerate(qt.mixed_configs()):
        idx = np.nonzero(ids == v)[0]
        st = qo.make_states(*[a[idx] for a in state])
        calls.append(q_step("task table row %d" % v, qo.consts_from_config(cfg), st, np.zeros(len(idx), np.int32), macts[:, idx]))
    grid = np.array(qt.small_map(), np.int32)
    grid[5, 5] = 0
    c = qo.consts_from_config(qt.stock(), task=qo.TASK_NO_COLLISION)
    c.x_offset, c.y_offset = 5, 5
    pos, vel, omega, propw, R = qt.random_batch(48, 77)
    pos[:, :2] *= 0.4
    calls.append(q_step("small map, negative slices", c, qo.make_states(pos, vel, omega, propw, R), np.zeros(48, np.int32),
                        macts[:4, :48], grid=grid))
    # NaN, +-inf and huge values in states and actions, with and without the fused reset
    n = 40
    acts = np.random.RandomState(9).uniform(0.1, 15.0, (3, n, 4)).astype(np.float32)
    acts[0, 1::8, 0], acts[0, 3::8, 1], acts[1, 5::8, 2], acts[1, 7::8, 3] = NAN, INF, -INF, NAN
    for task in (qo.TASK_HOVERING, qo.TASK_NO_COLLISION):
        c = qo.default_consts(task=task)
        calls.append(q_step("special values task=%d" % task, c, qo.make_states(*_special_states(n, 41)), np.zeros(n, np.int32), acts))
        calls.append(q_step("special values task=%d auto-reset" % task, c, qo.make_states(*_special_states(n, 42)), np.zeros(n, np.int32),
                            acts, ar=qo.default_autoreset(seed=1, env_id_base=0), episode=np.zeros(n, np.uint32)))
    # the fused reset with Philox counters crossing 2^32: the global env id (counter words 0 / 1) and the episode (word 2)
    n = 6
    c = qo.default_consts(nt=2)
    acts = np.random.RandomState(10).uniform(0.1, 15.0, (7, n, 4)).astype(np.float32)
    ar = qo.default_autoreset(seed=(0xABCD << 32) | 17, env_id_base=2 ** 32 - 3)
    ar.init_velocity[:] = [0.5, -0.25, 0.125]
    ar.init_angular_velocity[:] = [1.0, 2.0, -3.0]
    calls.append(q_step("auto-reset counters cross 2^32", c, qo.make_states(*qt.random_batch(n, 5)), np.zeros(n, np.int32), acts, ar=ar,
                        episode=np.full(n, 2 ** 32 - 2, np.uint32)))
    # the small entry points
    def expect_defaults():
        c = qo.Consts()
        qo.lib().qo_default_consts(C.byref(c))
        return [bytes(c), struct.pack("<QQ", qo.lib().qo_sizeof_state(), qo.lib().qo_sizeof_consts())]
    calls.append(Call("default consts", Q_DEFAULTS, [_ints()], expect_defaults))
    rs = np.random.RandomState(0)
    for k in range(4):
        A = (np.eye(3) + rs.uniform(-0.3, 0.3, (3, 3))).astype(np.float32)
        calls.append(Call("inv3[%d]" % k, Q_INV3, [_ints(), A.tobytes()], lambda A=A: [qo.inv3(A).tobytes()]))
    for ctr, key in (([0] * 4, [0] * 2), ([0xffffffff] * 4, [0xffffffff] * 2),
                     ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])):
        calls.append(Call("philox %x" % ctr[0], Q_PHILOX, [_ints(), np.asarray(ctr, np.uint32).tobytes(), np.asarray(key, np.uint32).tobytes()],
                          lambda ctr=ctr, key=key: [np.asarray(qo.philox4x32_10(ctr, key), np.uint32).tobytes()]))
    for gid, ep in ((0, 0), (2 ** 32 - 1, 2 ** 32 - 1), ((1 << 40) + 9, 70000)):
        calls.append(Call("reset noise %d %d" % (gid, ep), Q_RESET_NOISE, [_ints(gid, ep), bytes(ar)],
                          lambda gid=gid, ep=ep: [x.tobytes() for x in qo.reset_noise(ar, gid, ep)]))
    st = qo.make_states(*_special_states(20, 43))

    def expect_observe(st=st):
        s = _clone(st)
        for e in range(len(s)):
            qo.lib().qo_refresh_inverse(C.byref(s[e]))
        return [qo.observe(qo.default_consts(), s).tobytes(), bytes(s)]
    calls.append(Call("observe", Q_OBSERVE, [_ints(len(st), 1), _raw(qo.default_consts(), _Q_PTRS), bytes(st)], expect_observe))
    n = 8
    st, init = qo.make_states(*qt.random_batch(n, 6)), qo.make_states(*qt.random_batch(n, 7))
    acts = np.random.RandomState(8).uniform(0.1, 15.0, (3, n, 4)).astype(np.float32)
    c = qo.default_consts(nt=5)

    def expect_run(st=st, init=init, acts=acts, c=c):
        s, ct = _clone(st), np.zeros(len(st), np.int32)
        count = qo.batch_run(c, s, init, ct, acts, 17)
        return [struct.pack("<q", count), bytes(s), ct.tobytes()]
    calls.append(Call("batch_run", Q_BATCH_RUN, [_ints(n, 3, 17), _raw(c, _Q_PTRS), b"", b"", bytes(st), bytes(init),
                                                 np.zeros(n, np.int32).tobytes(), acts.tobytes()], expect_run))
    return calls


# ---- maze -----------------------------------------------------------------------------------------------------------------

_T_PTRS = ("walls", "texts", "food_rewards", "food_interval")
_S_PTRS = ("cur_food", "wait_refresh", "revival")
_V_PTRS = ("textures", "ceil_tex")
_TEX = {}


def maze_view(H, V, **kw):
    if not _TEX:
        _TEX.update(np.load(os.path.join(GOLDEN, "maze_textures.npz")))
    return mo.View(_TEX["grounds"], _TEX["ceil"], H, V, **kw)


def _task_blobs(task):
    return [_raw(task.c, _T_PTRS), task.walls.tobytes(), task.texts.tobytes(), task.food_rewards.tobytes(), task.food_interval.tobytes()]


def _view_blobs(view):
    if view is None:
        return [b"", b"", b"", b"", b""]
    return [_raw(view.c, _V_PTRS), view.tex.tobytes(), view.ceil.tobytes(), view.sin4.tobytes(), view.cos4.tobytes()]


def _plain_state(st):
    return _raw(st.c, _S_PTRS)


def m_episode(name, task, task_type, mode, actions, max_steps=1000, view_grid=1, view=None, observe=True, start=None, col_dist=0.20):
    """mo.reset, optionally `start` = dict(grid, ori_idx, ori, loc, ...) written into the state, then one step per action
    (mode 0: step_2d with an int action, 1: step_disc3d, 2: step_cont3d with (turn, walk)) and the observation after each."""
    actions = np.ascontiguousarray(np.asarray(actions, np.float64).reshape(-1, 1 if mode < 2 else 2))
    if mode < 2:
        actions = np.concatenate([actions, np.zeros_like(actions)], 1)
    sb = b""
    if start is not None:                # the whole state as the front end leaves it: reset, then the placed members
        s0 = mo.State(task)
        mo.reset(task, task_type, s0)
        _place(s0.c, start)
        sb = _plain_state(s0)
    blobs = ([_ints(task_type, max_steps, mode, view_grid, len(actions), int(observe)), struct.pack("<d", col_dist)] + _task_blobs(task)
             + [sb, actions.tobytes()] + _view_blobs(view))

    def observation(st):
        if mode == 0:
            return mo.observe_2d(task, task_type, st, view_grid).tobytes()
        return mo.observe_3d(task, task_type, view, st, int(mode == 2)).tobytes()

    def expect():
        st = mo.State(task)
        mo.reset(task, task_type, st)
        if start is not None:
            _place(st.c, start)
        out = [observation(st)] if observe else []
        for a in actions:
            if mode == 0:
                r, d = mo.step_2d(task, task_type, max_steps, st, int(a[0]))
            elif mode == 1:
                r, d = mo.step_disc3d(task, task_type, max_steps, st, int(a[0]))
            else:
                r, d = mo.step_cont3d(task, task_type, max_steps, st, a[0], a[1], col_dist)
            out += [struct.pack("<d", r), struct.pack("<i", int(d)), _plain_state(st)]
            if observe:
                out.append(observation(st))
        return out + [st.cur_food.tobytes(), st.wait.tobytes(), st.revival.tobytes()]
    return Call(name, M_EPISODE, blobs, expect)


def _place(s, start):
    for k, v in start.items():
        if k in ("grid", "loc"):
            getattr(s, k)[0], getattr(s, k)[1] = v
        else:
            setattr(s, k, v)


def _otask(t):
    return mo.Task(**(t._asdict() if hasattr(t, "_asdict") else t))


def m_view(name, task, view, pos, s_ori, c_ori, transp):
    transp = np.ascontiguousarray(transp, np.float64)
    D = np.asarray([pos[0], pos[1], s_ori, c_ori], np.float64)

    def expect():
        rgb = np.zeros((view.H, view.V, 3), np.int32)
        mo.lib().mo_maze_view(C.byref(task.c), C.byref(view.c), D[:2].ctypes.data_as(C.c_void_p), C.c_double(D[2]), C.c_double(D[3]),
                              transp.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p))
        return [rgb.tobytes()]
    blobs = [_ints(), D.tobytes()] + _task_blobs(task)[:3] + _view_blobs(view)[:3] + [transp.tobytes()]
    return Call(name, M_VIEW, blobs, expect)


def _segments(g):
    """The action stream of a golden episode file cut where the recorder reset the env: [(first step, actions)]."""
    cuts = [0] + [t for t in range(1, len(g["actions"])) if g["reset_before"][t]] + [len(g["actions"])]
    return [(a, g["actions"][a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def maze_calls():
    import maze_cont_cases as mc
    import maze_large_cases as ml
    calls = []
    # the committed goldens, each episode of the recording; the 3-D ones render their first 3 steps at the recorded resolution
    for path in sorted(glob.glob(os.path.join(GOLDEN, "maze2d_*.npz")) + glob.glob(os.path.join(GOLDEN, "maze3d_*.npz"))):
        g = np.load(path)
        base = os.path.basename(path)[:-4]
        tt = mo.SURVIVAL if "survival" in base else mo.ESCAPE
        task = mo.Task.from_golden(g)
        mode = 0 if base.startswith("maze2d") else (2 if "_cont_" in base else 1)
        view = None
        if mode:
            H, V = (int(x) for x in g["resolution"])
            kw = dict(max_vision=float(g["max_vision"]), fov=float(g["fol_angle"])) if "max_vision" in g.files else {}
            view = maze_view(H, V, **kw)
        for first, acts in _segments(g):
            if mode == 0:
                calls.append(m_episode("%s@%d" % (base, first), task, tt, 0, acts, int(g["max_steps"]), int(g["view_grid"])))
            else:
                calls.append(m_episode("%s@%d frames" % (base, first), task, tt, mode, acts[:3], int(g["max_steps"]), view=view))
                calls.append(m_episode("%s@%d" % (base, first), task, tt, mode, acts, int(g["max_steps"]), view=view, observe=False))
    # every size class: 2-D windows that leave the map, the four discrete headings, a continuous walk, 32 x 32 frames
    rs = np.random.RandomState(3)
    view32 = maze_view(32, 32)
    for n in (7, 9, 15, 63, 255):
        task = _otask(ml.synthetic_task(n, 100 + n))
        for tt in (mo.ESCAPE, mo.SURVIVAL):
            for vg in (1, 2):
                # on the border wall itself only moves that stay inside the map: index n is an IndexError in the reference
                # (index -1 wraps there, and here)
                for cell, acts in (((0, 0), [0, 1, 2, 3]), ((1, 1), [0, 1, 2, 3, 3, 1]), ((n - 1, n - 1), [0, 2, 0]),
                                   ((n - 2, 1), [1, 2, 3, 0]), ((0, n // 2), [0, 2, 3, 1]), ((n - 2, n - 2), [1, 3, 0, 2])):
                    calls.append(m_episode("2d n=%d tt=%d vg=%d at %r" % (n, tt, vg, cell), task, tt, 0, acts, 5, vg,
                                           start=dict(grid=cell)))
            calls.append(m_episode("2d n=%d tt=%d walk" % (n, tt), task, tt, 0, rs.randint(0, 4, 40), 30, 2))
            calls.append(m_episode("disc3d n=%d tt=%d" % (n, tt), task, tt, 1, [0, 3, 0, 3, 0, 2, 0, 3, 1, 3, 1, 1, 1, 2], 12, view=view32))
            acts = np.stack([rs.uniform(-1.3, 1.3, 12), rs.uniform(-1.3, 1.3, 12)], 1)
            calls.append(m_episode("cont3d n=%d tt=%d" % (n, tt), task, tt, 2, acts, 10, view=view32))
        for k in range(3):
            ang = rs.uniform(0, 6.3)
            pos = (rs.uniform(1.0, n - 1.0) * task.c.cell_size, rs.uniform(1.0, n - 1.0) * task.c.cell_size)
            calls.append(m_view("maze_view n=%d [%d]" % (n, k), task, view32, pos, np.sin(ang), np.cos(ang), task.food_rewards))
    # every collision branch of the continuous move (tests/maze_cont_cases.py): the placed cases, ESCAPE; every 8th in SURVIVAL too
    built = mc.build_cases()
    otasks = {n: [mo.Task(**t) for t in ts] for n, ts in built.tab.items()}
    for k, c in enumerate(list(built.exact) + list(built.general)):
        task = otasks[c.n][c.task]
        cs32 = np.float32(task.c.cell_size)
        start = dict(loc=(float(c.loc[0]), float(c.loc[1])), ori=float(c.ori),
                     grid=(int(np.float32(c.loc[0]) / cs32), int(np.float32(c.loc[1]) / cs32)))
        for tt in ((mo.ESCAPE, mo.SURVIVAL) if k % 8 == 0 else (mo.ESCAPE,)):
            calls.append(m_episode("cont case %d tt=%d" % (k, tt), task, tt, 2, [(float(a), float(b)) for a, b in c.actions], mc.MAX_STEPS,
                                   observe=False, start=start, col_dist=c.col_dist))
    # 256-wide frames: next to the outer wall of the largest maze, and the open field whose long rays cross more translucent
    # cells than the oracle's per-ray list holds (MAX_TRANSP 256: cell 0.04 gives up to 2 * 300 + 4 crossings, the map 511)
    view256 = maze_view(256, 24)
    task = _otask(ml.synthetic_task(255, 355))
    for cell, ori in (((1, 1), 0), ((253, 253), 2), ((1, 253), 3), ((253, 1), 1)):
        calls.append(m_episode("wall cell %r 256 wide" % (cell,), task, mo.SURVIVAL, 1, [], view=view256, start=dict(grid=cell, ori_idx=ori)))
    for n, cs in ((81, 0.1), (255, 0.04)):
        task = _otask(ml.open_field_task(n, cs))
        for tt in (mo.SURVIVAL, mo.ESCAPE):
            calls.append(m_episode("open field n=%d cell %g tt=%d" % (n, cs, tt), task, tt, 1, [], view=view256))
        calls.append(m_episode("open field n=%d cell %g diagonal" % (n, cs), task, mo.SURVIVAL, 2, [(0.25, 1.0)], view=view256))
    return calls


# ---- walker ---------------------------------------------------------------------------------------------------------------

def _w_model(m, power):
    cm, table = wc.make_model(m, power)
    margin_off = len(table) - len(m.sph_body)
    return cm, table, margin_off


def walker_setup(name):
    """(mjcf model, wo_model, table, margin_off, wo_params) of a model of walker_fixtures.load_models() or of the 24-hinge
    centipede of tests/walker_cases.py ("centipede" / "centipede@mujoco"), with the constants the tests run them with."""
    import walker_cases as wk
    from oracle import abd
    if name.startswith("centipede"):
        m = wk.model("centipede", "mujoco" if name.endswith("@mujoco") else "bullet")
        cm, table, off = _w_model(m, np.full(len(m.joint_lo), 100.0) * wk.CENTIPEDE_POWER)
        r = wk.ROBOT["centipede"]
        prm = wc.ant_params(m, alive_z=r["alive_z"], alive_bonus=r["alive_bonus"], self_collision=0)
    else:
        from walker_fixtures import load_models
        m = _MODELS.setdefault("all", load_models())[name]
        ant = name.startswith("ant")
        cm, table, off = _w_model(m, np.full(len(m.joint_lo), 100.0) * 2.5 if ant else abd.HUMANOID_MOTOR_POWER * 0.41)
        prm = wc.ant_params(m) if ant else wc.humanoid_params(m)
    return m, cm, table, off, prm


_MODELS = {}


def w_episode(name, setup, actions, noise=None, env=None, **over):
    """wo_env_reset with `noise` (None: NULL) when `env` is None, else the loaded `env`; then one wo_env_step per action row."""
    m, cm, table, off, prm = setup
    prm = _clone(prm)
    for k, v in over.items():
        setattr(prm, k, v)
    nj, nobs = cm.nj, 8 + 2 * cm.nj + cm.nf
    actions = np.ascontiguousarray(np.asarray(actions, np.float32).reshape(-1, nj))
    noise = None if noise is None else np.ascontiguousarray(noise, np.float64)
    env0 = wc.Env() if env is None else _clone(env)
    blobs = [_ints(len(actions), int(env is None), off), _raw(cm, ("table", "sph_margin")), table.tobytes(), bytes(prm), bytes(env0),
             _b(noise, np.float64), actions.tobytes()]

    def expect(keep=table):
        lib, e, out = wc.load(), _clone(env0), []
        obs = np.zeros(nobs, np.float32)
        po = obs.ctypes.data_as(C.POINTER(C.c_float))
        if env is None:
            lib.wo_env_reset(C.byref(cm), C.byref(prm), C.byref(e), None if noise is None else noise.ctypes.data_as(C.POINTER(C.c_double)), po)
            out += [obs.tobytes(), bytes(e)]
        r = (C.c_double * 6)()
        for a in actions:
            d = lib.wo_env_step(C.byref(cm), C.byref(prm), C.byref(e), a.ctypes.data_as(C.POINTER(C.c_float)), po, r,
                                C.cast(C.byref(r, 8), C.POINTER(C.c_double)))
            out += [obs.tobytes(), bytes(r), struct.pack("<i", d), bytes(e)]
        return out

    def int_tail(k, n_blobs):            # [obs, env] of a reset; per step obs, the six reward terms, done (i32), env
        k -= 2 if env is None else 0
        if k >= 0 and k % 4 == 2:
            return -1
        is_env = k == -1 or (k >= 0 and k % 4 == 3)
        return C.sizeof(wc.Env) - wc.Env.steps.offset if is_env else 0      # steps, floor_known, initial_z_unset
    return Call(name, W_EPISODE, blobs, expect, int_tail=int_tail,
                nan=bool(np.isnan(actions).any()) or _non_finite(*[getattr(env0.s, f)[:] for f in ("pos", "rot", "vel", "omega", "q", "qd")]))


def reset_env(setup, noise=None, **over):
    """The wo_env a reset leaves (through the ctypes front end), for cases that edit it before stepping."""
    m, cm, table, off, prm = setup
    prm = _clone(prm)
    for k, v in over.items():
        setattr(prm, k, v)
    e = wc.Env()
    noise = None if noise is None else np.ascontiguousarray(noise, np.float64)
    wc.load().wo_env_reset(C.byref(cm), C.byref(prm), C.byref(e), None if noise is None else noise.ctypes.data_as(C.POINTER(C.c_double)), None)
    return e


SIDE = (1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0)       # rolled a quarter turn about x: lying on its side
BACK = (0.0, 0.0, -1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0)       # pitched a quarter turn about y: lying on its back


def posed_env(setup, rot=None, z=None, q=None, edits=(), **over):
    e = reset_env(setup, **over)
    if rot is not None:
        e.s.rot[:] = list(rot)
    if z is not None:
        e.s.pos[2] = z
    if q is not None:
        e.s.q[:len(q)] = list(q)
    for field, i, v in edits:
        getattr(e.s, {"q": "q", "qd": "qd", "pos": "pos", "vel": "vel"}[field])[i] = v
    return e


def standing_env(setup):
    """The reset pose (no joint noise), at rest, lowered until the lowest collision proxy touches the ground."""
    from oracle import abd
    m = setup[0]
    e = reset_env(setup)
    s = abd.State(m)
    s.pos, s.rot = np.array(e.s.pos[:], float), np.array(e.s.rot[:], float).reshape(3, 3)
    s.q = np.array(e.s.q[:len(s.q)], float)
    kin = abd.kinematics(m, s)
    low = min(float((kin["o"][m.sph_body[g]] + kin["R"][m.sph_body[g]] @ m.sph_pos[g])[2] - m.sph_radius[g]) for g in range(len(m.sph_body)))
    e.s.pos[2] = e.s.pos[2] - low
    return e


def w_substep(name, setup, state, tau, n_sub=4, **over):
    m, cm, table, off, prm = setup
    prm = _clone(prm)
    for k, v in over.items():
        setattr(prm, k, v)
    tau = np.ascontiguousarray(tau, np.float64)
    blobs = [_ints(n_sub, off), _raw(cm, ("table", "sph_margin")), table.tobytes(), bytes(prm), bytes(state), tau.tobytes()]

    def expect(keep=table):
        s, out = _clone(state), []
        for _ in range(n_sub):
            touch = (C.c_ulonglong * 2)()
            nr = wc.load().wo_substep(C.byref(cm), C.byref(prm), C.byref(s), tau.ctypes.data_as(C.POINTER(C.c_double)), touch)
            out += [struct.pack("<i", nr), bytes(touch), bytes(s)]
        return out
    return Call(name, W_SUBSTEP, blobs, expect)


def w_run(name, setups, task_id, n_steps, actions):
    prm = setups[0][4]
    task_id = np.ascontiguousarray(task_id, np.int32)
    n = len(task_id)
    models = (wc.Model * len(setups))(*[s[1] for s in setups])
    envs = (wc.Env * n)()
    for i in range(n):
        envs[i] = reset_env(setups[task_id[i]])
    actions = np.ascontiguousarray(actions, np.float32)
    cleared = (wc.Model * len(setups))(*[type(s[1]).from_buffer_copy(_raw(s[1], ("table", "sph_margin"))) for s in setups])
    blobs = ([_ints(len(setups), n, n_steps, len(actions), *[s[3] for s in setups]), bytes(cleared), task_id.tobytes(), bytes(prm), bytes(envs),
              actions.tobytes()] + [s[2].tobytes() for s in setups])

    def expect(keep=setups):
        e = _clone(envs)
        count = wc.load().wo_run(models, task_id.ctypes.data_as(C.POINTER(C.c_int)), C.byref(prm), e, n, n_steps,
                                 actions.ctypes.data_as(C.POINTER(C.c_float)), len(actions))
        flops = (C.c_ulonglong * 9)()
        return [struct.pack("<q", count), bytes(e), struct.pack("<i", wc.load().wo_flops_read(flops, 0))]
    return Call(name, W_RUN, blobs, expect)


def walker_names():
    from walker_fixtures import load_models
    return sorted(_MODELS.setdefault("all", load_models())) + ["centipede", "centipede@mujoco"]


def walker_calls():
    import walker_cases as wk
    calls = []
    rs = np.random.RandomState(17)
    for name in walker_names():
        setup = walker_setup(name)
        m, cm = setup[0], setup[1]
        nj = cm.nj
        kind = name.split("@")[0].split("_")[0]
        preset = "mujoco" if name.endswith("@mujoco") else "bullet"
        rand = lambda T: rs.uniform(-1.3, 1.3, (T, nj)).astype(np.float32)
        sat = np.where(rs.rand(6, nj) < 0.5, -3.0, 3.0).astype(np.float32)
        z0 = float(m.body_pos[0][2])
        # reset (with and without joint noise) and the landing; standing: the reset pose set on the ground (lowered until the
        # lowest collision proxy touches it), at rest, zero actions: the humanoids stand on both feet (both flags come on), the
        # ants and the centipede rest on whatever is lowest in that pose; free flight
        calls.append(w_episode("%s reset + random" % name, setup, rand(24), noise=rs.uniform(-0.1, 0.1, nj)))
        calls.append(w_episode("%s reset, no noise, saturated" % name, setup, sat))
        calls.append(w_episode("%s standing" % name, setup, np.zeros((8, nj), np.float32), env=standing_env(setup)))
        calls.append(w_episode("%s free flight" % name, setup, rand(4), env=posed_env(setup, z=z0 + 3.0)))
        # lying on the side and on the back at z = 0.25, self-collision on and off
        for pose, rot in (("side", SIDE), ("back", BACK)):
            for sc in (1, 0):
                calls.append(w_episode("%s lying on its %s self_collision=%d" % (name, pose, sc), setup, rand(12),
                                       env=posed_env(setup, rot=rot, z=0.25), self_collision=sc))
        calls.append(w_episode("%s lying, saturated" % name, setup, np.tile(sat, (2, 1)), env=posed_env(setup, rot=SIDE, z=0.25),
                               self_collision=1))
        # NaN actions and states, the float32-overflowing joint angles of walker_cases.OVERFLOW
        bad = rand(3)
        bad[0, 0], bad[1, nj - 1], bad[2, nj // 2] = NAN, NAN, INF
        calls.append(w_episode("%s NaN actions" % name, setup, bad))
        if kind in wk.ROBOT and "_" not in name.split("@")[0]:
            for row in wk.loaded_rows(kind, preset):
                if row.kind != "plain":
                    calls.append(w_episode("%s %s" % (name, row.name), setup, np.zeros((2, nj), np.float32),
                                           env=posed_env(setup, edits=row.edits)))
            # the joint-limit batch, upside down in free flight
            for r, scaled in enumerate(wk.limit_batch(kind, preset)):
                calls.append(w_episode("%s limit row %d" % (name, r), setup, np.zeros((1, nj), np.float32),
                                       env=posed_env(setup, rot=wk.FLIP, z=wk.LIMIT_Z, q=wk.limit_q(kind, preset, scaled))))
        # one sub-step at a time from a lying state, with the torques of a saturated action
        e = posed_env(setup, rot=BACK, z=0.2)
        calls.append(w_substep("%s sub-steps" % name, setup, e.s, rs.uniform(-40, 40, nj), n_sub=8, self_collision=1))
    # the fixed-size tables: a lying, folded centipede with self-collision fills WO_MAX_CONTACTS and overruns WO_MAX_CANDIDATES
    for name in ("centipede", "centipede@mujoco"):
        setup = walker_setup(name)
        nj = setup[1].nj
        for pose, rot in (("side", SIDE), ("back", BACK), ("upright", None)):
            for z in (0.05, 0.25):
                q = np.where(np.arange(nj) % 2 == 0, 1.2, -1.2)
                calls.append(w_episode("%s folded on its %s z=%g" % (name, pose, z), setup, rs.uniform(-1, 1, (6, nj)).astype(np.float32),
                                       env=posed_env(setup, rot=rot, z=z, q=q), self_collision=1))
    # ... and overruns WO_MAX_CANDIDATES (48): every joint of the standing centipede bent 1.6 or 2 rad one way or the other, the
    # body just above the ground. The sign patterns were found by search (48 seeds tried, these leave 1 to 19 of the 48
    # self-collision pairs untested once the table is full); tests/test_oracle_replay.py counts with -DWO_COUNT_CAPS that they do.
    # Ground candidates alone cannot overrun the table: no robot here has more than 29 collision proxies.
    setup = walker_setup("centipede")
    nj = setup[1].nj
    for seed, amp in ((1005, 2.0), (1020, 2.0), (1035, 1.6), (1036, 1.6), (1043, 2.0)):
        q = np.random.RandomState(seed).choice([-1.0, 1.0], nj) * amp
        calls.append(w_episode("centipede knotted %d %g" % (seed, amp), setup, rs.uniform(-1, 1, (3, nj)).astype(np.float32),
                               env=posed_env(setup, z=0.02, q=q), self_collision=1))
    # wo_run: the bench baseline's loop over a mixed batch (restarts included: max_steps 3)
    setups = [walker_setup("humanoid"), walker_setup("humanoid_tra_137")]
    setups[0][4].max_steps = 3
    calls.append(w_run("wo_run humanoids", setups, [0, 1, 1, 0, 1], 7, rs.uniform(-1.3, 1.3, (11, 17)).astype(np.float32)))
    return calls


def all_calls():
    return {"quadrotor": quadrotor_calls(), "maze": maze_calls(), "walker": walker_calls()}
