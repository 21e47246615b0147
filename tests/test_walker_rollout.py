"""CPU-side checks of the walker rollout (include/metagym_hip.h mg_walker_rollout): wrong arguments are error codes with a
message, decided on the host before any launch (so no GPU is needed), and WalkerBatchEnv.rollout refuses a wrong action shape
before it touches a device. The kernel itself: tests/test_walker_rollout_gpu.py."""
import ctypes as C

import pytest

NULL_POINTER, BAD_SIZE, BAD_CONFIG, UNSUPPORTED = -1001, -1002, -1003, -1004


def _fake_call():
    """An ant-shaped call whose every required pointer is a (host) dummy: it passes each check, so one wrong argument at a time
    can be shown to be THE reason for a refusal. Nothing here may reach a launch."""
    from metagym_amd import _lib
    fake = C.create_string_buffer(256)
    addr = C.addressof(fake)
    tp = _lib.WalkerTopology()
    tp.n_bodies, tp.n_joints, tp.n_spheres, tp.n_feet, tp.n_geoms, tp.n_pairs = 5, 4, 5, 4, 5, 0
    for b in range(5):                       # a torso and four one-hinge legs, one proxy per body, the legs are the feet
        tp.body_parent[b] = -1 if b == 0 else 0
        tp.sphere_body[b], tp.geom_body[b] = b, b
        tp.sphere_foot[b] = b - 1
    for j in range(4):
        tp.joint_body[j], tp.foot_body[j] = j + 1, j + 1
    ms = _lib.WalkerModels()
    ms.table, ms.n_tasks, ms.model_stride = addr, 1, 25 * 5 + 12 * 4 + 4 * 5 + 7 * 5
    prm = _lib.WalkerParams()
    prm.time_step, prm.frame_skip, prm.solver_iterations, prm.mapping, prm.max_steps = 0.005, 4, 5, 1, 10
    st = _lib.WalkerState()
    for k in ("task_id", "pos", "rot", "vel", "omega", "q", "qd", "potential", "feet_contact", "steps"):
        setattr(st, k, addr)
    return _lib.load(), tp, ms, prm, st, C.c_void_p(addr), fake


def _caller(lib, tp, ms, prm, st, p):
    ok = dict(topo=tp, models=ms, prm=prm, n_envs=3, state=st, n_steps=4, obs_every=0, actions=p, obs=p, reward=p,
              rewards5=None, done=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mg_walker_rollout(*[a[k] for k in ok])
    return call


def test_walker_rollout_null_pointers_and_sizes_are_codes_not_crashes():
    lib, tp, ms, prm, st, p, _keep = _fake_call()
    call = _caller(lib, tp, ms, prm, st, p)
    for name in ("topo", "models", "prm", "state", "actions", "obs", "reward", "done"):
        assert call(**{name: None}) == NULL_POINTER, name
        assert b"NULL" in lib.mg_last_error(), name
    assert call(n_steps=0) == BAD_SIZE and b"n_steps" in lib.mg_last_error()
    assert call(n_steps=-5) == BAD_SIZE and b"n_steps" in lib.mg_last_error()
    assert call(obs_every=-1) == BAD_SIZE and b"obs_every" in lib.mg_last_error()
    assert call(n_envs=0) == BAD_SIZE and b"n_envs" in lib.mg_last_error()
    st.q = None                                                   # an array of the state
    assert call() == NULL_POINTER and b"NULL" in lib.mg_last_error()


def test_walker_rollout_refuses_what_stays_single_step():
    lib, tp, ms, prm, st, p, _keep = _fake_call()
    call = _caller(lib, tp, ms, prm, st, p)
    prm.mapping = 0
    assert call() == UNSUPPORTED and b"mapping" in lib.mg_last_error()
    prm.mapping = 1
    prm.actuation, prm.pd_command = 1, p.value
    assert call() == UNSUPPORTED and b"actuation" in lib.mg_last_error()
    prm.actuation, prm.pd_command = 0, None
    prm.substep_log = p.value
    assert call() == BAD_CONFIG and b"substep_log" in lib.mg_last_error()


def test_walker_rollout_refuses_what_the_step_refuses():
    lib, tp, ms, prm, st, p, _keep = _fake_call()
    call = _caller(lib, tp, ms, prm, st, p)
    tp.body_parent[2] = 3                                         # parents come first
    assert call() == BAD_CONFIG and b"parent" in lib.mg_last_error()
    tp.body_parent[2] = 0
    tp.sphere_foot[1] = 4                                         # n_feet = 4: feet 0..3
    assert call() == BAD_CONFIG and b"sphere_foot" in lib.mg_last_error()
    tp.sphere_foot[1] = 0
    ms.model_stride -= 1
    assert call() == BAD_SIZE and b"stride" in lib.mg_last_error()
    ms.model_stride += 1
    prm.n_terrain_boxes = -1
    assert call() == BAD_SIZE and b"terrain" in lib.mg_last_error()
    prm.n_terrain_boxes = 2                                       # boxes without a box array
    assert call() == NULL_POINTER
    prm.n_terrain_boxes = 0
    prm.frame_skip = 0
    assert call() == BAD_CONFIG
    prm.frame_skip = 4
    tp.n_joints = 60                                              # beyond the ABI's joint count
    assert call() == BAD_SIZE


def test_env_rollout_refuses_a_wrong_action_shape_before_any_device_work():
    import torch
    import metagym_amd.metalocomotion as ml
    env = ml.MetaAntEnv(num_envs=3, device="cuda:0")              # (no task set: nothing is allocated on a device yet)
    with pytest.raises(ValueError):
        env.rollout(torch.zeros(3, 8))                            # 2-D: a step's action, not a rollout's
    with pytest.raises(ValueError):
        env.rollout(torch.zeros(0, 3, 8))                         # T = 0
    assert env.global_step == 0
