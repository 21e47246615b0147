"""Case tables and helpers shared by tests/test_walker_edges.py (CPU: the restatement of the auto-reset noise stream and the
numpy oracle's verdict on every table row) and tests/test_walker_edges_gpu.py (the HIP kernels on the same rows). Nothing here
needs a GPU.

The fused auto-reset draws the joint angles of a restarted env from Philox4x32-10 (csrc/walker_core.h, reset_joint_noise):
    counter  c0 = gid lo, c1 = step lo, c2 = step hi ^ (gid hi << 8), c3 = 0x57414c4b + j / 4      (gid = env_id_base + e)
    key      seed lo, seed hi
    value    -0.1 + 0.2 * (word[j & 3] * 2^-32)        in float64
`reset_noise` restates that with the Philox of metagym_amd.metamaze.policy (Random123 known answers: tests/test_maze_policy.py).
A device that fuses the multiply-add differs from the restatement by at most NOISE_BOUND = 2^-55: the rounding of 0.2 * x (< 0.2)
is at most 2^-56 and the two roundings of results below 0.1 at most 2^-57 each. Neighbouring values are 0.2 * 2^-32 = 4.7e-11
apart."""
import functools

import numpy as np

from metagym_amd.metamaze.policy import philox4x32_10

NOISE_BOUND = 2.0 ** -55
SEEDS = (11, 0x9E3779B97F4A7C15)
ENV_ID_BASES = (7, 2 ** 32 - 2, (5 << 32) + 3)      # 2^32 - 2: the batch crosses the word boundary of the global env id
GLOBAL_STEPS = (0, 2 ** 32 - 3)                     # 2^32 - 3: a rollout of 6 steps crosses the word boundary of the step
_M64 = (1 << 64) - 1


def reset_noise(seed, env_id_base, e, step, nj):
    """Joint noise the fused auto-reset gives env `e` (an index or an array of them) at Philox step `step` (one int, or one
    per env): float64 [len(e), nj]."""
    e = np.atleast_1d(np.asarray(e)).ravel()
    gid = np.array([(int(env_id_base) + int(x)) & _M64 for x in e], dtype=np.uint64)
    st = [int(s) & _M64 for s in np.atleast_1d(np.asarray(step, dtype=object)).ravel()]
    step = np.broadcast_to(np.array(st, dtype=np.uint64), gid.shape)
    seed = int(seed) & _M64
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    j = np.arange(int(nj))
    c0, c1 = (gid & m32)[:, None], (step & m32)[:, None]
    c2 = ((step >> s32) ^ (((gid >> s32) << np.uint64(8)) & m32))[:, None]
    c3 = ((0x57414c4b + j // 4) & 0xFFFFFFFF).astype(np.uint64)[None, :]
    words = np.stack(philox4x32_10(c0, c1, c2, c3, seed & 0xFFFFFFFF, seed >> 32), -1)            # [n, nj, 4]
    word = np.take_along_axis(words, np.broadcast_to((j & 3)[None, :, None], words.shape[:2] + (1,)), -1)[:, :, 0]
    return -0.1 + 0.2 * (word.astype(np.float64) * 2.0 ** -32)


# ---- the robots -------------------------------------------------------------------------------------------------------

CENTIPEDE = "24 hinges (30 dof, every slot of <30, any>)"      # tests/test_walker_generic_gpu.ROBOTS: every joint slot, j / 4 up to 5
# alive_z of the test's own 24-hinge robot: above the reach of its legs, so that a body at the threshold is in free flight
ROBOT = {"humanoid": dict(nj=17, alive_z=0.50, alive_bonus=2.0, initial_z=0.8, f32_sum=True),
         "ant": dict(nj=8, alive_z=0.26, alive_bonus=1.0, initial_z=0.75, f32_sum=False),
         "centipede": dict(nj=24, alive_z=0.45, alive_bonus=1.0, initial_z=0.6, f32_sum=False)}
CENTIPEDE_POWER = 0.4


@functools.lru_cache(maxsize=None)
def model(kind, preset):
    """The parsed robot: the recorded humanoid / ant of tests/golden/walker_models.npz, or the 24-hinge centipede."""
    if kind == "centipede":
        from metagym_amd.metalocomotion.mjcf import load_mjcf
        from test_walker_generic_gpu import ROBOTS, _centipede
        text, feet = _centipede(ROBOTS[CENTIPEDE])
        return load_mjcf(text, foot_names=feet, preset=preset)
    from walker_fixtures import load_models
    return load_models()[kind if preset == "bullet" else kind + "@" + preset]


def centipede_feet():
    from test_walker_generic_gpu import ROBOTS, _centipede
    return _centipede(ROBOTS[CENTIPEDE])[1]


def oracle_env(kind, preset, **kw):
    """oracle/abd.WalkerEnv with the robot's constants (tests/test_walker_gpu._oracle_env; the centipede as in
    tests/test_walker_generic_gpu.py, self-collision off, with this file's alive_z)."""
    from oracle import abd
    from walker_fixtures import world_kw
    m = model(kind, preset)
    if kind == "centipede":
        return abd.WalkerEnv(m, prm=abd.Params(friction=0.8 * float(m.geom_friction), power=CENTIPEDE_POWER, self_collision=False,
                                               self_friction=float(m.geom_friction) ** 2, **world_kw(m)),
                             motor_power=np.full(len(m.joint_lo), 100.0), alive_z=ROBOT[kind]["alive_z"], alive_bonus=1.0,
                             initial_z=None, torque_f32=False, **kw)
    from test_walker_gpu import _oracle_env
    return _oracle_env(m, kind == "ant", **kw)


# ---- B: loaded states ---------------------------------------------------------------------------------------------------
# An edit is (field, index, value): field one of q / qd / pos / vel, written into the state a zero-noise reset leaves.

# float32 overflow, float64 finite ("bullet" world: the +-100 clamp keeps every velocity finite): a joint angle of +-1e39
OVERFLOW = {"humanoid": ((0, 1e39), (4, 1e39), (0, -1e39), (3, -1e39), (5, -1e39), (7, -1e39), (9, -1e39), (13, -1e39), (16, -1e39)),
            "ant": ((1, 1e39), (3, 1e39), (5, 1e39), (7, 1e39), (1, -1e39), (3, -1e39), (5, -1e39), (7, -1e39))}
# The same overflow with the base LIFT metres higher. A joint 1e39 rad past its limit is pulled back by an impulse of that size, every
# generalized velocity ends each sub-step AT the +-100 clamp and its sign is a matter of round-off (the numpy oracle and
# oracle/walker_oracle.c already disagree on them): the base moves by 0 ... 2 m per env step in either direction, so whether a row
# above is alive differs between implementations of the same engine. 3 m up the robot is alive whatever the signs are
# (4 sub-steps x 5 ms x 100 m/s = 2 m), and `done` is decided by the finite rule alone.
LIFT = 3.0
OVERFLOW_LIFTED = {"humanoid": OVERFLOW["humanoid"][:4], "ant": OVERFLOW["ant"][2:6], "centipede": ((0, 1e39), (10, 1e39), (23, -1e39), (5, -1e39))}
NAN = float("nan")
V100 = float(np.nextafter(100.0, np.inf))


class Row(object):
    """name, edits, done (True / False: what the reference's rule gives, asserted against the oracle on the CPU), pinned
    {obs index: value}, kind: 'overflow' | 'lifted' | 'head' | 'nan' | 'clamp' | 'plain'."""
    def __init__(self, name, edits, done, pinned, kind):
        self.name, self.edits, self.done, self.pinned, self.kind = name, tuple(edits), done, dict(pinned), kind

    def __repr__(self):
        return self.name


def loaded_rows(kind, preset):
    """The rows of section B for one robot and preset. The overflow rows are the "bullet" world's (without its velocity clamp
    the state itself overflows and nothing is defined)."""
    rows = [Row("plain", (), False, {}, "plain")]
    if preset == "bullet":
        for j, v in OVERFLOW.get(kind, ()):
            rows.append(Row("q[%d]=%g" % (j, v), [("q", j, v)], False, {8 + 2 * j: 5.0 if v > 0 else -5.0}, "overflow"))
        z = float(model(kind, preset).body_pos[0][2]) + LIFT
        for j, v in OVERFLOW_LIFTED[kind]:
            rows.append(Row("q[%d]=%g,z+%g" % (j, v, LIFT), [("q", j, v), ("pos", 2, z)], False, {8 + 2 * j: 5.0 if v > 0 else -5.0},
                            "lifted"))
    rows.append(Row("z=1e39", [("pos", 2, 1e39)], False, {0: 5.0}, "head"))
    rows.append(Row("vx=1e3", [("vel", 0, 1e3)], False, {3: 5.0}, "head"))
    rows.append(Row("q[2]=nan", [("q", 2, NAN)], True, {}, "nan"))
    rows.append(Row("qd[1]=nan", [("qd", 1, NAN)], True, {}, "nan"))
    rows.append(Row("z=nan", [("pos", 2, NAN)], True, {}, "nan"))
    rows.append(Row("vy=nan", [("vel", 1, NAN)], True, {}, "nan"))
    if preset == "bullet":          # the velocity clamp: joint rates beyond, at and one ulp over +-100 on two joints
        for v in (150.0, 100.0, V100):
            rows.append(Row("qd[1]=%r,qd[5]=%r" % (v, -v), [("qd", 1, v), ("qd", 5, -v)], False, {}, "clamp"))
            rows.append(Row("qd[1]=%r,qd[5]=%r" % (-v, v), [("qd", 1, -v), ("qd", 5, v)], False, {}, "clamp"))
    return rows


def apply_edits(o, edits):
    """Write a row's edits into an abd.WalkerEnv that was just reset."""
    for field, i, v in edits:
        {"q": o.s.q, "qd": o.s.qd, "pos": o.s.pos, "vel": o.s.v}[field][i] = v


class Outcome(object):
    __slots__ = ("obs", "done", "rewards", "q", "qd", "pos", "vel", "z")


def oracle_step(kind, preset, edits=(), q=None, rot=None, action=None, max_steps=2000):
    """Zero-noise reset, the edits (and optionally all joint angles `q` and the base rotation `rot`), ONE step: what the
    numpy oracle returns and the state it leaves."""
    o = oracle_env(kind, preset, max_steps=max_steps)
    nj = len(o.m.joint_lo)
    o.reset(np.zeros(nj))
    if q is not None:
        o.s.q[:] = q
    if rot is not None:
        o.s.rot = np.array(rot, float).reshape(3, 3).copy()
    apply_edits(o, edits)
    with np.errstate(all="ignore"):
        obs, rew, done, info = o.step(np.zeros(nj, np.float32) if action is None else np.asarray(action, np.float32))
    out = Outcome()
    out.obs, out.done, out.rewards = np.asarray(obs, np.float32), bool(done), np.asarray(info["rewards"], float)
    out.q, out.qd, out.pos, out.vel, out.z = o.s.q.copy(), o.s.qd.copy(), o.s.pos.copy(), o.s.v.copy(), float(o.s.pos[2])
    return out


@functools.lru_cache(maxsize=None)
def loaded_outcomes(kind, preset):
    """The oracle's outcome of every row of `loaded_rows`, computed once and shared by the tests (one oracle step per row)."""
    return tuple(oracle_step(kind, preset, r.edits) for r in loaded_rows(kind, preset))


# ---- C: thresholds --------------------------------------------------------------------------------------------------------
# The alive sweep runs in free flight, so that the step moves the base by a constant and nothing else: the robot upside down
# (legs up), every joint in the middle of its range (no limit row), the base a little above the threshold. One env step of
# 4 x 5 ms then lowers the base by DROP, the same for every height: the figures are the numpy oracle's, and
# tests/test_walker_edges.py holds them against it to 1e-12.
FLIP = (1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, -1.0)
DROP = {("humanoid", "bullet"): 0.0024494620457363, ("ant", "bullet"): 0.0024494620457363, ("centipede", "bullet"): 0.0024494620457363,
        ("humanoid", "mujoco"): 0.0026209125526362, ("ant", "mujoco"): 0.00245, ("centipede", "mujoco"): 0.00245}
SWEEP_N = 64


def mid_q(kind, preset):
    m = model(kind, preset)
    return 0.5 * (np.asarray(m.joint_lo, float) + np.asarray(m.joint_hi, float))


def alive_threshold_obs(kind):
    """obs[0] = float32(z - initial_z) of a base exactly at the alive threshold."""
    r = ROBOT[kind]
    return np.float32(r["alive_z"] - r["initial_z"])


def alive_sweep(kind, preset, n=SWEEP_N):
    """Base heights to load, ascending: after the step, obs[0] runs through the threshold in half-ulp steps of obs[0], n / 2 envs
    on either side (n = 64: +-16 float32 ulps)."""
    r = ROBOT[kind]
    ulp = float(np.spacing(np.abs(alive_threshold_obs(kind))))
    return r["alive_z"] + DROP[(kind, preset)] + 0.5 * ulp * (np.arange(n) - n // 2 + 0.5)


def alive_rule(kind, obs0):
    """walker_base_env.py:47-48 on the returned float32 obs[:, 0]: (alive bonus float64 [N], alive bool [N]). The humanoid's
    initial_z is a python float, so its sum stays float32; the ant's (and the centipede's) comes out of calc_state as a float64."""
    r = ROBOT[kind]
    obs0 = np.asarray(obs0, np.float32)
    if r["f32_sum"]:
        h = (obs0 + np.float32(r["initial_z"])).astype(np.float64)
    else:
        h = obs0.astype(np.float64) + float(r["initial_z"])
    alive = h > r["alive_z"]
    return np.where(alive, r["alive_bonus"], -1.0), alive


def ulps_from(obs0, ref):
    """Distance of float32 values of one sign from `ref` in units in the last place."""
    a = np.asarray(obs0, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - int(np.float32(ref).view(np.int32)))


# joints-at-limit: rows of the batch (in free flight, upside down, LIMIT_Z up): which joints sit past 0.99 of their half range, and
# on which side. In free flight nothing moves a joint that is inside its range, so the scaled positions are 0.995 for "at the
# limit" and 0.98 for "not", either side of 0.99 by half a percent. The humanoid of the "mujoco" reading has joint springs that do:
# there the rows start 10 % outside the range on the low side (the limit row pulls a fifth of the excess back per sub-step) and
# at half range. tests/test_walker_edges.py holds the counts against the oracle.
LIMIT_Z = 3.0


def limit_batch(kind, preset):
    """[rows, nj] scaled joint positions: counts 0, 1, nj - 1, nj in rows 0-3, then all on the high side, alternating sides, the
    last joint alone on the low side, the first half on the low side."""
    nj = ROBOT[kind]["nj"]
    P, A = (0.5, 1.1) if (kind, preset) == ("humanoid", "mujoco") else (0.98, 0.995)
    rows = [np.full(nj, P), np.full(nj, P), np.full(nj, -A), np.full(nj, -A), np.full(nj, A), np.full(nj, -A), np.full(nj, P),
            np.full(nj, P)]
    rows[1][0] = A
    rows[2][nj - 1] = P
    rows[5][1::2] = A
    rows[6][nj - 1] = -A
    rows[7][:nj // 2] = -A
    return np.stack(rows)


def limit_q(kind, preset, scaled):
    m = model(kind, preset)
    lo, hi = np.asarray(m.joint_lo, float), np.asarray(m.joint_hi, float)
    return 0.5 * (lo + hi) + 0.5 * (hi - lo) * np.asarray(scaled, float)


def limit_count(obs, nj):
    """The reference's count (walker_base.py:57, robot_bases.py:317-323) on returned float32 observations [N, obs_dim]."""
    return (np.abs(np.asarray(obs, np.float32)[:, 8:8 + 2 * nj:2]) > np.float32(0.99)).sum(1)


# action clamp: np.clip(a, -1, +1) (walker_base.py:27). Groups of values that must give the same state, and pairs that must not.
ONE_UP, ONE_DOWN = float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(1), np.float32(0)))
CLAMP_ACTIONS = np.array([1.0, ONE_UP, 1.3, 3e38, np.inf, -1.0, -ONE_UP, -1.3, -3e38, -np.inf, ONE_DOWN, -ONE_DOWN, 0.0, -0.0],
                         np.float32)
CLAMP_SAME = ((0, 1, 2, 3, 4), (5, 6, 7, 8, 9), (12, 13))
CLAMP_DIFFERENT = ((0, 10), (5, 11), (0, 12), (5, 12))
