"""GPU: the A1 control kernels (metagym_amd/csrc/a1.hip: ETG action path, sensor stack, action filter, reward shaping, info)
on HETEROGENEOUS batches, robot by robot against one CPU oracle instance per robot (oracle/a1.py, pinned to the reference's
goldens by test_oracle_a1_control.py / test_oracle_a1_env.py / test_oracle_a1_info.py). Every robot has its own inputs, its own
per-robot state and its own place in the masks (resets at different steps), so a kernel that reads another robot's entry, walks
a history ring with the wrong stride or takes a mask from the wrong robot fails here. Batch sizes 1, 63 / 64 / 65 (one wave,
its partial and its second block) and 1000 (ragged, 16 blocks); at 1000 the compared robots are 0, 63, 64, N - 1, both sides of
every block boundary and 256 seeded random ones. Tolerances as in test_a1_control_gpu.py: 1e-12 where device transcendentals
enter, exact for the filter, flags and counts."""
import ctypes as C

import numpy as np
import pytest
import torch

from metagym_amd import _lib
from metagym_amd.quadrupedal import ActionFilter, EtgActionPath, RewardShaping, SensorStack
from metagym_amd.quadrupedal.a1_actuators import A1Actuators
from metagym_amd.quadrupedal.terrain import task_terrain
from oracle import a1 as oa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rtol=1e-12, atol=1e-12)
SIZES = [1, 63, 64, 65, 1000]
TERMS = ("torso", "up", "feet", "tau", "badfoot", "footcontact")


def compared_robots(n, seed=0):
    """Every robot up to 65; beyond, robots 0, 63, 64, N - 1, both sides of every block boundary and 256 seeded random ones."""
    if n <= 65:
        return np.arange(n)
    edges = np.arange(64, n, 64)
    pick = {0, 63, 64, n - 1} | set(edges.tolist()) | set((edges - 1).tolist())
    pick |= set(np.random.RandomState(1000 + seed).choice(n, 256, replace=False).tolist())
    return np.array(sorted(pick))


def dev(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def etg_weights(H, scale):
    """ETG_w / ETG_b for which the traj-mode leg IK has to retry (shrink the foot offset) at some phases and not at others."""
    pat = np.sin(np.linspace(0, 2 * np.pi, H)) if H > 1 else np.ones(1)
    return scale * np.array([[0.5], [0.2], [-1.0]]) * pat, np.array([0.0, 0.0, -0.06])


# (act_mode, task_mode, action_space, ETG, H, w scale)
ETG_CASES = [("traj", "normal", 0, 1, 20, 0.04), ("traj", "gallop", 2, 1, 32, 0.04), ("pose", "normal", 3, 1, 1, 0.5),
             ("pose", "gallop", 1, 1, 20, 0.3), ("traj", "normal", 2, 0, 20, 0.0)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", range(len(ETG_CASES)))
def test_etg_action_path_robot_by_robot(case, n):
    act_mode, task_mode, space, etg, H, scale = ETG_CASES[case]
    w, b = etg_weights(H, scale)
    rs = np.random.RandomState(10 * case + n)
    p = EtgActionPath(n, DEV, ETG=etg, ETG_H=H, ETG_w=w, ETG_b=b, act_mode=act_mode, task_mode=task_mode, action_space=space)
    idx = compared_robots(n, case)
    cpu = {e: oa.EtgActionPath(w, b, enabled=bool(etg), H=H, pose_mode=act_mode == "pose", gallop=task_mode == "gallop",
                               action_space=space) for e in idx}
    t = rs.uniform(0.0, 1.0, n)                                  # each robot's own time since reset
    obs = p.reset(dev(t))
    mixed = 0                                                    # steps at which the IK retried for some robots and not for others
    for e in idx:
        want = cpu[e].reset(t[e])
        if etg:
            assert np.allclose(obs[e].cpu().numpy(), want, **TOL), "reset ETG_obs, robot %d" % e
    for k in range(6):
        if k == 3:                                               # a masked reset of some robots at their own new time
            m = rs.rand(n) < 0.4
            t = np.where(m, rs.uniform(0.0, 0.5, n), t)
            obs = p.reset(dev(t), mask=dev(m, torch.bool))
            for e in idx:
                if m[e]:
                    want = cpu[e].reset(t[e])
                    if etg:
                        assert np.allclose(obs[e].cpu().numpy(), want, **TOL), "masked reset ETG_obs, robot %d" % e
        a = rs.uniform(-0.2, 0.2, (n, 12))
        cmd, obs = p.step(dev(a), dev(t))
        cmd = cmd.cpu().numpy()
        last = p.last_ETG_act.t().cpu().numpy()
        o = None if obs is None else obs.cpu().numpy()
        before = np.array([cpu[e].retries for e in idx])
        for e in idx:
            want_cmd, want_obs = cpu[e].step(a[e], t[e])
            assert np.allclose(cmd[e], want_cmd, **TOL), "command, robot %d step %d" % (e, k)
            if etg:
                assert np.allclose(o[e], want_obs, **TOL), "ETG_obs, robot %d step %d" % (e, k)
                assert np.allclose(last[e], cpu[e].last_etg_act, **TOL), "last_ETG_act, robot %d step %d" % (e, k)
        retried = np.array([cpu[e].retries for e in idx]) > before
        mixed += int(retried.any() and not retried.all())
        t = t + 0.026
    if etg and act_mode == "traj" and n >= 63:                   # in one launch, the IK retry loop ran for some robots and not for others
        assert mixed > 0


def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("normal", [0, 1])
def test_sensor_stack_robot_by_robot(normal, n):
    """Staggered resets: reset_mask 0 (step), 1 (reset) and 2 (not this robot's call: state and row untouched) mixed per robot
    and per step; yaws that cross +-pi between steps; the noise of every observation replayed as distinct [33, N] draws."""
    rs = np.random.RandomState(20 + 7 * normal + n)
    sigma = np.array(SensorStack.NOISE_SIGMA).reshape(33, 1)
    draws = []
    st = SensorStack(n, DEV, normal=normal, noise=True, noise_source=lambda: draws[-1])
    idx = compared_robots(n, normal)
    cpu = {e: oa.SensorStack(normal) for e in idx}
    base = rs.uniform(-1, 1, (n, 3))
    yaw0, dyaw = rs.uniform(-np.pi, np.pi, n), rs.uniform(-0.5, 0.5, n)
    yaw0[::3] = np.pi - 0.2 * rs.rand(n)[::3]                     # (a third start just below +pi and turn through it)
    dyaw[::3] = 0.15
    angles = np.tile([0, 0.9, -1.8], (n, 4)) + rs.uniform(-0.3, 0.3, (n, 12))
    crossed = 0
    for k in range(8):
        rm = np.ones(n, np.uint8) if k == 0 else rs.choice(np.array([0, 1, 2], np.uint8), n, p=[0.6, 0.2, 0.2])
        base = base + rs.uniform(-0.02, 0.03, (n, 3))
        yaw = wrap(yaw0 + k * dyaw)
        if k:
            crossed += int(np.sum(np.abs(yaw - prev_yaw) > np.pi))
        prev_yaw = yaw
        rpy = np.stack([rs.uniform(-0.3, 0.3, n), rs.uniform(-0.3, 0.3, n), yaw], 1)
        drpy = rs.uniform(-2, 2, (n, 3))
        angles = angles + rs.uniform(-0.05, 0.05, (n, 12))
        contact = (rs.rand(n, 4) < 0.7).astype(np.float64)
        draws.append(rs.normal(size=(33, n)) * sigma)
        before = {key: t.clone() for key, t in st._t.items()}
        obs = st.observe(dev(base), dev(rpy), dev(drpy), dev(angles), dev(contact), reset_mask=dev(rm, torch.uint8)).cpu().numpy()
        for key, t in st._t.items():       # value 2: this robot's sensor state is left untouched
            col = t.t() if t.dim() == 2 else t
            old = before[key].t() if t.dim() == 2 else before[key]
            assert torch.equal(col[dev(rm == 2, torch.bool)], old[dev(rm == 2, torch.bool)]), key
        for e in idx:
            if rm[e] == 2:
                continue
            want = cpu[e].observe(base[e], rpy[e], drpy[e], angles[e], contact[e], bool(rm[e] == 1), noise=draws[-1][:, e])
            assert np.allclose(obs[e], want, **TOL), "observation, robot %d step %d (reset_mask %d)" % (e, k, rm[e])
    assert crossed > 0 or n == 1


def filter_coefficients(kind):
    """[12, H + 1] a, b per joint, every joint its own: Butterworth low-pass (H = 2), band-pass (H = 4), exponential (H = 1)."""
    from scipy.signal import butter
    rate = 1 / (0.002 * 13)
    nyq = 0.5 * rate
    a, b = [], []
    for j in range(12):
        if kind == "low":
            bb, aa = butter(2, [(3.0 + 0.25 * j) / nyq], btype="low")
        elif kind == "band":
            bb, aa = butter(2, [(0.5 + 0.1 * j) / nyq, (4.0 + 0.3 * j) / nyq], btype="band")
        else:
            alpha = 0.1 + 0.07 * j
            aa, bb = np.array([1.0, alpha - 1.0]), np.array([alpha, 0.0])
        a.append(aa); b.append(bb)
    return np.stack(a), np.stack(b)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["low", "band", "exp"])
def test_action_filter_robot_by_robot(kind, n):
    """Partial reset(mask), init_history(x, mask) and filter(x, init_mask) at every step; bit-exact."""
    a, b = filter_coefficients(kind)
    rs = np.random.RandomState(30 + n + len(kind))
    f = ActionFilter(n, a, b, DEV)
    idx = compared_robots(n, len(kind))
    an, bn = a / a[:, :1], b / a[:, :1]                           # action_filter.py:55-57, as the wrapper does
    cpu = {e: oa.ActionFilter(an, bn) for e in idx}
    for k in range(14):
        m_reset, m_hist, m_init = (rs.rand(n) < 0.2), (rs.rand(n) < 0.2), (rs.rand(n) < 0.25)
        if k == 0:
            m_init[:] = True
        xh = rs.uniform(-1, 1, (n, 12))
        x = rs.uniform(-1, 1, (n, 12))
        f.reset(dev(m_reset, torch.bool))
        f.init_history(dev(xh), dev(m_hist, torch.bool))
        y = f.filter(dev(x), init_mask=dev(m_init, torch.bool)).cpu().numpy()
        for e in idx:
            if m_reset[e]:
                cpu[e].reset()
            if m_hist[e]:
                cpu[e].init_history(xh[e])
            if m_init[e]:
                cpu[e].init_history(x[e])
            assert np.array_equal(y[e], cpu[e].filter(x[e])), "filter output, robot %d step %d" % (e, k)


COURSES = ("slopeslope", "stairslope", "plane")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("vel_mode", ["max", "equal"])
def test_reward_shaping_robot_by_robot(vel_mode, n):
    """Staggered reset(mask=) steps, > 10 steps after every robot's reset; still robots (the stillness rule of last_base10
    fires 10 steps after THEIR reset), moving robots, and robots on both sides of the attitude, foot-height and yaw limits;
    three courses through the terrain table; a per-robot d_yaw; reward_p 1.7."""
    rs = np.random.RandomState(40 + n + len(vel_mode))
    pm = dict(torso=1.0, up=0.3, feet=0.2, tau=0.1, badfoot=0.1, footcontact=0.1)
    gpu = RewardShaping(n, DEV, param=pm, reward_p=1.7, vel_d=0.6, vel_mode=vel_mode)
    rows, counts, segs = [], [], []
    for task in COURSES:
        _, env_info, _ = task_terrain(task)
        r, c = RewardShaping.pack_env_info(env_info)
        rows.append(r); counts.append(c)
        segs.append([(s[0], s[1], s[2][0], s[2][1], s[2][4]) for s in env_info])
    course = rs.randint(0, len(COURSES), n)
    table, cnt, tid = dev(np.stack(rows)), dev(np.array(counts), torch.int32), dev(course, torch.int32)
    gpu.set_terrain_table(table, cnt, tid)
    idx = compared_robots(n, len(vel_mode))
    cpu = {e: oa.RewardShaping([pm[t] for t in TERMS], reward_p=1.7, vel_d=0.6, segments=segs[course[e]], vel_mode=vel_mode) for e in idx}
    d_yaw = rs.uniform(-0.4, 0.4, n)
    # kinds: 0 still, 1 moving, 2 attitude probe, 3 foot-height probe, 4 yaw probe
    kind = rs.randint(0, 5, n)
    kind[0], kind[min(1, n - 1)] = 0, 1
    start = np.stack([rs.uniform(-1.4, 8.0, n), rs.uniform(-0.2, 0.2, n), rs.uniform(0.25, 0.35, n)], 1)
    feet0 = np.tile([0.18, -0.13, -0.27, 0.18, 0.13, -0.27, -0.18, -0.13, -0.27, -0.18, 0.13, -0.27], (n, 1))
    second_reset = rs.randint(2, 13, n)                            # every robot's second reset, after step second_reset - 1
    n_steps = 12 + 12

    def inputs(k, base):
        moving = kind != 0
        step = np.stack([rs.uniform(-0.005, 0.03, n), rs.uniform(-0.004, 0.004, n), rs.uniform(-0.01, 0.01, n)], 1)
        base = np.where(moving[:, None], base + step, base)
        pose = rs.uniform(-0.3, 0.3, (n, 3))
        pose[:, 2] = np.where(kind == 4, rs.uniform(-0.9, 0.9, n), rs.uniform(-0.5, 0.5, n))
        rot = np.tile(np.eye(3).reshape(-1), (n, 1)) + rs.uniform(-0.05, 0.05, (n, 9))
        rot[:, 8] = np.where(kind == 2, rs.uniform(0.3, 0.7, n), rot[:, 8])
        foot = feet0 + rs.uniform(-0.03, 0.03, (n, 12))
        probe = kind == 3
        foot[probe, 2::3] = rs.uniform(-0.2, 0.03, (int(probe.sum()), 4))      # mean around -0.1, some feet above 0
        contact = (rs.rand(n, 4) < 0.7).astype(np.float64)
        return base, pose, rot, foot, contact, rs.uniform(0, 3, n), rs.randint(0, 3, n)

    base = start.copy()
    _, _, rot, foot, *_ = inputs(0, base)
    base = start.copy()
    gpu.reset(dev(base), dev(rot), dev(foot))
    for e in idx:
        cpu[e].reset(base[e], rot[e], foot[e].reshape(4, 3))
    still_fired, dones = set(), []
    for k in range(n_steps):
        base, pose, rot, foot, contact, energy, bad = inputs(k, base)
        reward, done, terms = gpu.step(dev(base), dev(pose), dev(rot), dev(foot), dev(contact), dev(energy), dev(bad, torch.int32),
                                       dev(d_yaw))
        reward, done = reward.cpu().numpy(), done.cpu().numpy()
        got = np.stack([terms[t].cpu().numpy() for t in TERMS], 1)
        for e in idx:
            w_terms, w_reward, w_done = cpu[e].step(base[e], pose[e], rot[e], foot[e].reshape(4, 3), contact[e], energy[e], int(bad[e]), d_yaw[e])
            assert np.allclose(got[e], w_terms, **TOL), "terms, robot %d step %d" % (e, k)
            assert np.allclose(reward[e], w_reward, **TOL), "reward, robot %d step %d" % (e, k)
            assert bool(done[e]) == w_done, "done, robot %d step %d (kind %d)" % (e, k, kind[e])
            dones.append(w_done)
            if kind[e] == 0 and w_done:       # (a still robot meets no other rule: only the stillness rule ends it)
                assert cpu[e].steps >= 10
                still_fired.add(k)
        m = second_reset == k + 1
        if m.any():
            base = np.where(m[:, None], start, base)
            gpu.reset(dev(base), dev(rot), dev(foot), mask=dev(m, torch.bool))
            for e in idx:
                if m[e]:
                    cpu[e].reset(base[e], rot[e], foot[e].reshape(4, 3))
    if n >= 63:
        assert any(dones) and not all(dones)     # the stillness rule fired 10 steps after each still robot's own reset, i.e. at different steps
        assert len(still_fired) >= 2, still_fired


def info_via_kernel(n, co):
    """mg_a1_info on control observations co [n, 43] written straight into an actuator state."""
    robot = A1Actuators(n, DEV)
    robot._control_obs.copy_(dev(co).t())
    f64 = dict(dtype=torch.float64, device=DEV)
    o = dict(pose=torch.empty(3, n, **f64), rot_mat=torch.empty(9, n, **f64), footposition=torch.empty(12, n, **f64),
             joint_angle=torch.empty(12, n, **f64), drpy=torch.empty(3, n, **f64), energy=torch.empty(n, **f64))
    lib = _lib.load()
    with torch.cuda.device(robot.device):
        rc = lib.mg_a1_info(C.byref(robot._cfg), n, C.byref(robot._st), _lib.ptr(o["pose"]), _lib.ptr(o["rot_mat"]),
                            _lib.ptr(o["footposition"]), _lib.ptr(o["joint_angle"]), _lib.ptr(o["drpy"]), _lib.ptr(o["energy"]),
                            _lib.current_stream(robot.device))
    _lib.check(rc, "mg_a1_info")
    return {k: (v if v.dim() == 1 else v.t()).cpu().numpy() for k, v in o.items()}


def stressed_control_obs(n, rs):
    """Control observations whose attitude and joint angles sit where the info conversions are delicate: yaw near +-pi, pitch
    near +-pi/2 (the asin argument rounding past +-1, decided by the clamp), quaternions off unit length (taken as they come:
    the present formula, which the PyBullet stand-in does not share — DESIGN.md), joint angles exactly +-pi, just either side
    of +-pi and large multiples of 2 pi."""
    co = np.zeros((n, 43))
    ang = rs.uniform(-4, 4, (n, 12))
    special = np.array([np.pi, -np.pi, np.nextafter(np.pi, 0), np.nextafter(np.pi, 4), np.nextafter(-np.pi, 0), np.nextafter(-np.pi, -4),
                        2 * np.pi * 1000 + 0.3, -2 * np.pi * 12345 - 1.1, 2 * np.pi, 3 * np.pi, 0.0, -0.0])
    pick = rs.rand(n, 12) < 0.5
    ang[pick] = rs.choice(special, int(pick.sum()))
    co[:, :12] = ang
    co[:, 12:36] = rs.uniform(-20, 20, (n, 24))
    rpy = np.stack([rs.uniform(-np.pi, np.pi, n), rs.uniform(-1.5, 1.5, n), rs.uniform(-np.pi, np.pi, n)], 1)
    c = rs.randint(0, 4, n)
    rpy[c == 1, 2] = rs.choice([np.pi, -np.pi, np.nextafter(np.pi, 0), np.nextafter(-np.pi, 0), np.pi - 1e-9], int((c == 1).sum()))
    rpy[c == 2, 1] = rs.choice([0.5 * np.pi, -0.5 * np.pi, 0.5 * np.pi - 1e-9, -0.5 * np.pi + 1e-8, 0.5 * np.pi - 1e-3], int((c == 2).sum()))
    for e in range(n):
        r, p, y = rpy[e] / 2
        cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
        co[e, 36:40] = (sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy)
    scaled = c == 3
    co[scaled, 36:40] *= rs.uniform(0.98, 1.02, (int(scaled.sum()), 1))
    co[:, 40:43] = rs.uniform(-3, 3, (n, 3))
    return co


@pytest.mark.parametrize("n", SIZES)
def test_info_entries_robot_by_robot(n):
    rs = np.random.RandomState(50 + n)
    co = stressed_control_obs(n, rs)
    got = info_via_kernel(n, co)
    clamped = 0
    for e in compared_robots(n):
        want = oa.info_from_control_obs(co[e])
        for key in ("pose", "rot_mat", "footposition", "joint_angle", "drpy"):
            assert np.allclose(got[key][e], want[key], **TOL), "%s, robot %d" % (key, e)
        assert np.allclose(got["energy"][e], want["energy"], **TOL), "energy, robot %d" % e
        x, y, z, w = co[e, 36:40]
        clamped += int(abs(2 * (w * y - z * x)) > 1.0)
    assert clamped > 0 or n < 63                                     # the clamp decided some pitches
