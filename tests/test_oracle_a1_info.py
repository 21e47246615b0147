"""CPU: the oracle's restatement of what mg_a1_info computes from a robot's delayed control observation
(oracle/a1.py: info_from_control_obs — pose, rot_mat, foot FK, wrapped angles, drpy, energy) against the `info` entries the
unmodified `A1GymEnv` reported on the scripted Bullet client (tests/golden/a1_env.npz). The GPU batch tests use it as the
per-robot reference of the info kernel and to give each oracle robot its own pose and rot_mat."""
import os

import numpy as np
import pytest

from oracle import a1 as oa
from test_oracle_a1_env import make_env, world

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "a1_env.npz")


@pytest.mark.parametrize("idx", range(11))
def test_info_restatement_matches_the_reference_env(idx):
    g = np.load(GOLDEN)
    name = str(g["cases"][idx])
    env, d_yaw = make_env(g, name)
    env.reset(g[name + "/reset_true_obs"][0], world(g, name, 0), g[name + "/true_obs"][0], world(g, name, 1), d_yaw)
    for k in range(len(g[name + "/action"])):
        env.step(g[name + "/action"][k], g[name + "/true_obs"][k + 1], world(g, name, k + 2), d_yaw)
        inf = oa.info_from_control_obs(env.act.control_obs[0])
        assert np.array_equal(inf["pose"], g[name + "/info_pose"][k]), "%s pose, step %d" % (name, k)
        assert np.array_equal(inf["rot_mat"], g[name + "/info_rot_mat"][k]), "%s rot_mat, step %d" % (name, k)
        assert np.array_equal(inf["footposition"], g[name + "/info_footposition"][k].reshape(-1)), "%s footposition, step %d" % (name, k)
        assert np.array_equal(inf["joint_angle"], g[name + "/info_joint_angle"][k])
        assert np.array_equal(inf["drpy"], g[name + "/info_drpy"][k])
        assert inf["energy"] == pytest.approx(g[name + "/info_energy"][k], rel=1e-14, abs=1e-300)


def test_info_restatement_differs_from_the_pybullet_stand_in_near_gimbal_lock():
    """The one known open point: the PyBullet stand-in normalises the quaternion and snaps to roll 0, pitch
    +-pi/2 once |sin(pitch)| >= 0.99999; the scripted client (and mg_a1_info) do neither. Away from there they agree."""
    from oracle.refstubs import pybullet as pb
    q_lock = pb.getQuaternionFromEuler((0.3, 0.5 * np.pi - 1e-3, -0.4))          # |sin(pitch)| > 0.99999
    q_far = pb.getQuaternionFromEuler((0.3, 0.7, -0.4))
    assert not np.allclose(oa.euler_from_quaternion(q_lock), pb.getEulerFromQuaternion(q_lock), rtol=0, atol=1e-6)
    assert np.allclose(oa.euler_from_quaternion(q_far), pb.getEulerFromQuaternion(q_far), rtol=0, atol=1e-12)
    q_scaled = 1.001 * np.asarray(q_far)                                          # not normalised: only the stand-in rescales
    assert not np.allclose(oa.euler_from_quaternion(q_scaled), pb.getEulerFromQuaternion(q_scaled), rtol=0, atol=1e-6)
