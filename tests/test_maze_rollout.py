"""CPU-side checks of the maze rollouts (include/metagym_hip.h mg_maze2d_rollout / mg_maze3d_rollout): wrong arguments are
error codes with a message, decided on the host before any launch (so no GPU is needed), and the rule that maps `obs_every`
to the recorded step indices, as a pure function. The kernels themselves: tests/test_maze_rollout_gpu.py."""
import ctypes as C

import pytest

NULL_POINTER, BAD_SIZE, BAD_CONFIG, UNSUPPORTED = -1001, -1002, -1003, -1004


def _fake_call():
    """Structs whose every required pointer is a (host) dummy: they pass each check, so one wrong argument at a time can be
    shown to be THE reason for a refusal. Nothing here may reach a launch."""
    from metagym_amd import _lib
    fake = C.create_string_buffer(256)
    addr = C.addressof(fake)
    t = _lib.MazeTasks()
    t.n, t.n_tasks = 9, 1
    for k in ("start", "goal", "walls", "texts", "food_rewards", "food_interval", "scalars"):
        setattr(t, k, addr)
    st = _lib.MazeState()
    for k in ("task_id", "grid", "steps", "ori_idx", "ori", "loc", "life", "cur_food", "wait_refresh", "revival"):
        setattr(st, k, addr)
    st.food_env_stride, st.food_cell_stride, st.food_by_slot = 81, 1, 0
    v = _lib.MazeView()
    v.res_h, v.res_v, v.max_vision, v.l_focal, v.text_size, v.tan_half_fov, v.collision_dist = 64, 64, 12.0, 0.2, 1.0, 1.37, 0.2
    for k in ("col_cos", "col_sin", "textures", "ceil_texture"):
        setattr(v, k, addr)
    v.n_textures, v.tex_size, v.max_ray_records, v.obs_format, v.uniform_cell_size = 2, 64, 17, 0, 0.0
    return _lib.load(), t, st, v, C.c_void_p(addr), fake


def test_maze2d_rollout_argument_errors_are_codes_not_crashes():
    lib, t, st, _v, p, _keep = _fake_call()
    # (tasks, task_type, max_steps, view_grid, auto_reset, n_envs, state, n_steps, obs_every, actions, obs, reward, reward64, done, stream)
    ok = dict(tasks=t, task_type=0, max_steps=10, view_grid=1, auto_reset=0, n_envs=4, state=st, n_steps=3, obs_every=0,
              actions=p, obs=p, reward=None, reward64=None, done=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mg_maze2d_rollout(*[a[k] for k in ok])

    for name in ("tasks", "state", "actions", "obs", "done"):
        assert call(**{name: None}) == NULL_POINTER, name
        assert b"NULL" in lib.mg_last_error(), name
    assert call(n_steps=0) == BAD_SIZE and b"n_steps" in lib.mg_last_error()
    assert call(n_steps=-5) == BAD_SIZE
    assert call(obs_every=-1) == BAD_SIZE and b"obs_every" in lib.mg_last_error()
    assert call(n_envs=0) == BAD_SIZE
    assert call(view_grid=-1) == BAD_SIZE
    assert call(task_type=7) == BAD_CONFIG
    # what mg_maze2d_step refuses about the tables is refused here too
    t.n = 2
    assert call() == BAD_SIZE
    t.n = 9
    st.life = None
    assert call(task_type=1) == NULL_POINTER and b"SURVIVAL" in lib.mg_last_error()
    st.life = p.value
    st.food_by_slot = 1                                          # slot layout without the task's slot tables
    assert call(task_type=1) == NULL_POINTER and b"food_by_slot" in lib.mg_last_error()


def test_maze3d_rollout_argument_errors_are_codes_not_crashes():
    lib, t, st, v, p, _keep = _fake_call()
    ok = dict(tasks=t, view=v, task_type=0, max_steps=10, continuous=0, auto_reset=0, n_envs=4, state=st, n_steps=3,
              obs_every=0, actions=p, obs=p, reward=None, reward64=None, done=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mg_maze3d_rollout(*[a[k] for k in ok])

    for name in ("tasks", "view", "state", "actions", "obs", "done"):
        assert call(**{name: None}) == NULL_POINTER, name
        assert b"NULL" in lib.mg_last_error(), name
    assert call(n_steps=0) == BAD_SIZE and b"n_steps" in lib.mg_last_error()
    assert call(obs_every=-2) == BAD_SIZE and b"obs_every" in lib.mg_last_error()
    assert call(n_envs=0) == BAD_SIZE
    assert call(task_type=5) == BAD_CONFIG
    # everything mg_maze3d_step refuses, refused before the first launch
    st.food_by_slot = 1
    assert call(task_type=1) == UNSUPPORTED and b"food_by_slot" in lib.mg_last_error()
    st.food_by_slot = 0
    st.ori = None
    assert call(continuous=1) == NULL_POINTER and b"continuous" in lib.mg_last_error()
    st.ori = p.value
    st.ori_idx = None
    assert call() == NULL_POINTER and b"discrete" in lib.mg_last_error()
    st.ori_idx = p.value
    v.res_v = 5000
    assert call() == BAD_SIZE and b"resolution" in lib.mg_last_error()
    v.res_v = 64
    v.textures = None
    assert call() == NULL_POINTER
    v.textures = p.value
    v.tex_size = 0
    assert call() == BAD_SIZE
    v.tex_size = 64
    t.n, v.max_ray_records = 100, 0                               # 2n + 1 = 201 translucent cells per ray
    assert call() == UNSUPPORTED and b"127" in lib.mg_last_error()


def _expected_steps(T, k):
    """The rule of the header, spelled out independently: every k-th step, and the last one."""
    if k == 0:
        return [T - 1]
    steps = list(range(k - 1, T, k))
    if not steps or steps[-1] != T - 1:
        steps.append(T - 1)
    return steps


@pytest.mark.parametrize("T", [1, 2, 7, 64])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 64, 100])
def test_obs_every_selects_every_kth_step_and_always_the_last(T, k):
    from metagym_amd.metamaze.maze_env import rollout_obs_steps
    got = rollout_obs_steps(T, k)
    assert got == _expected_steps(T, k)
    assert got[-1] == T - 1 and len(set(got)) == len(got) and got == sorted(got)
    K = len(got)
    if k == 0:
        assert K == 1
    elif k == 1:
        assert K == T and got == list(range(T))
    else:
        assert K == T // k + (1 if T % k else 0)
    for t in got[:-1]:
        assert (t + 1) % k == 0


def test_obs_every_and_step_count_are_validated():
    from metagym_amd.metamaze.maze_env import rollout_obs_steps
    with pytest.raises(ValueError):
        rollout_obs_steps(0, 1)
    with pytest.raises(ValueError):
        rollout_obs_steps(5, -1)
