"""MetaMaze shortest-path fields and the expert on the GPU (csrc/maze_expert.hip: mg_maze_distance_field,
mg_maze_expert_action, mg_maze2d_expert_rollout):
  1. field == `distance_field_reference`, exactly, for every kind: hand-built tables, sampled tables, n = 3, one n = 255
     serpentine for TURNS (the deepest search, the field outside LDS), levels wider than the kernel's queue;
  2. `expert_action` == `expert_action_reference` on scattered states;
  3. the 2-D closed loop: actions, the step of the first done, the replay identity through rollout() and step(), auto_reset,
     record=False, SURVIVAL;
  4. the discrete 3-D step(expert_action()) loop, and hipGraph captures;
  5. refused calls.
GPU box only (-m gpu)."""
import os

import numpy as np
import pytest
import torch

import maze_expert_oracle as mx
from metagym_amd.metamaze import expert as ex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
KINDS = [ex.MOVES_2D, ex.CELLS_3D, ex.TURNS]
KIND_IDS = ["moves2d", "cells3d", "turns"]
IDS = {"2d": "meta-maze-2D-v0", "disc": "meta-maze-discrete-3D-v0", "cont": "meta-maze-continuous-3D-v0"}


@pytest.fixture(scope="module", autouse=True)
def reference_textures():
    from metagym_amd.metamaze import MAZE_TASK_MANAGER
    tex = np.load(os.path.join(GOLDEN, "maze_textures.npz"))
    MAZE_TASK_MANAGER.set_textures(tex["grounds"], tex["ceil"])
    yield


def make(kind, n_envs, task_type="ESCAPE", auto_reset=False, max_steps=1000, view_grid=2):
    import metagym_amd
    kw = dict(num_envs=n_envs, device=DEV, max_steps=max_steps, task_type=task_type, auto_reset=auto_reset)
    if kind == "2d":
        kw["view_grid"] = view_grid
    else:
        kw["resolution"] = (1, 1)                  # the smallest frame the renderer accepts: these tests never look at it
    return metagym_amd.make(IDS[kind], **kw)


def hand_env(walls, n_envs=1):
    """A 2-D env over hand-built walls (start and goal: any two cells, the field tests pass their own sources)."""
    env = make("2d", n_envs)
    env.set_task([mx.task_of(w, (1, 1), (w.shape[0] - 2, w.shape[0] - 2)) for w in walls])
    return env


def sample_table(T, n, seed, **kw):
    from metagym_amd.metamaze import MAZE_TASK_MANAGER
    args = dict(n=n, allow_loops=True, step_reward=-0.01, goal_reward=1.0)
    args.update(kw)
    return MAZE_TASK_MANAGER.sample_tasks_device(T, device=DEV, seed=seed, **args)


def table_arrays(table):
    """walls [T, n, n], start [T, 2], goal [T, 2] of a device table, on the host."""
    T, n = table.n_tasks, table.n
    t = table.tensors
    return t["walls"].cpu().numpy().reshape(T, n, n).astype(np.int32), t["start"].cpu().numpy(), t["goal"].cpu().numpy()


def goal_masks(n, goals):
    return np.stack([mx.mask(n, [tuple(g)]) for g in goals])


def assert_field(env, walls, sources, kind, what):
    """env.distance_field(sources, kind) == the reference, exactly; returns the reference."""
    want = ex.distance_field_reference(walls, sources, kind)
    field = env.distance_field(torch.as_tensor(sources), kind)
    assert isinstance(field, ex.MazeDistanceField) and (field.kind, field.n) == (kind, walls.shape[1])
    got = field.numpy()
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "first difference at [t, k, x, y] = %s: got %d, want %d"
                           % (bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))
    return want


# ------------------------------------------------------------------------------------------------ 1. the field
def _tables_n9():
    c = 4
    return [("room", mx.room(9), mx.mask(9, [(1, 1)])),
            ("serpentine", mx.serpentine(9), mx.mask(9, [(7, 7)])),
            ("enclosed", mx.enclosed(9), mx.mask(9, [(c, c)])),
            ("free_border", mx.free_border(9), mx.mask(9, [(0, 8)])),
            ("minus_one", mx.with_minus_one(9), mx.mask(9, [(1, 1)])),
            ("multi_source", mx.room(9), mx.mask(9, [(1, 1), (7, 7), (1, 7), (0, 0)])),
            ("no_source", mx.room(9), mx.mask(9, []))]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_field_on_hand_built_tables(kind):
    """One T = 7 table of different n = 9 mazes (open room, serpentine, enclosed goal, free border cells, a -1 cell, several
    sources, none), and the n = 15 serpentine."""
    tables = _tables_n9()
    walls, src = np.stack([w for _, w, _ in tables]), np.stack([s for _, _, s in tables])
    env = hand_env(walls)
    want = assert_field(env, walls, src, kind, "n = 9")
    by_name = {name: want[i] for i, (name, _, _) in enumerate(tables)}
    # the properties the tables stand for hold in what was just compared
    x, y = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    inside = mx.room(9) == 0
    if kind != ex.TURNS:
        assert np.array_equal(by_name["room"][0][inside], (np.abs(x - 1) + np.abs(y - 1))[inside])      # Manhattan
        assert (by_name["minus_one"][0, 7, 7] > 0) == (kind == ex.MOVES_2D)                          # -1: a door in 2-D only
    assert (by_name["enclosed"][:, 1, 1] == -1).all() and (by_name["enclosed"][:, 4, 4] == 0).all()
    assert by_name["free_border"][0, 8, 8] > 1                                                       # one step if moves wrapped
    assert (by_name["no_source"] == -1).all()
    s15 = mx.serpentine(15)[None]
    w15 = assert_field(hand_env(s15), s15, mx.mask(15, [(1, 1)])[None], kind, "serpentine 15")
    assert w15[0, 0, 13, 13] >= 6 * 12 + 12 + 12                                                    # the corridor's length


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("n", [9, 15, 21])
def test_field_on_sampled_tables(n, kind):
    """Device-sampled tables: the default (goal) sources, and a mask of the starts and goals together."""
    table = sample_table(8, n, 100 + n)
    walls, start, goal = table_arrays(table)
    env = make("2d", 1)
    env.set_task(table)
    want = ex.distance_field_reference(walls, goal_masks(n, goal), kind)
    assert np.array_equal(env.distance_field(kind=kind).numpy(), want)
    for t in range(8):
        assert want[t, 0][tuple(start[t])] > 0                          # a sampled maze is connected
    assert_field(env, walls, goal_masks(n, goal) | goal_masks(n, start), kind, ("sampled, two sources", n))


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_field_at_the_smallest_size(kind):
    walls = np.stack([mx.room(3), np.zeros((3, 3), np.int32), np.ones((3, 3), np.int32)])
    src = np.stack([mx.mask(3, [(1, 1)]), mx.mask(3, [(0, 2)]), mx.mask(3, [(1, 1), (2, 2)])])
    assert_field(hand_env(walls), walls, src, kind, "n = 3")


def test_field_at_the_largest_size_with_the_deepest_search():
    """n = 255, TURNS: 260 100 states, more than fit in LDS, so the field is built in `dist` itself; the serpentine makes the
    search as deep as a maze of that size allows."""
    walls = mx.serpentine(255)[None]
    src = mx.mask(255, [(1, 1)])[None]
    want = assert_field(hand_env(walls), walls, src, ex.TURNS, "n = 255")
    assert want.max() > 127 * 253


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_field_with_levels_wider_than_the_queue(kind):
    """Sources on every third cell of an open room sized from the queue's capacity: the sources fit the queue (for K = 1),
    the next levels, four times as wide, do not, the last one (the border) fits again. For TURNS every level overflows."""
    from metagym_amd import _lib
    cap = _lib.load().mg_maze_distance_queue_capacity()
    m = int(np.sqrt(cap))
    n = 3 * m + 2
    assert 0 < cap and n <= 255, "the case is built from the capacity and needs an open room of n = %d" % n
    walls = mx.room(n)[None]
    src = np.zeros((1, n, n), np.uint8)
    src[0, 2:n - 1:3, 2:n - 1:3] = 1
    want = assert_field(hand_env(walls), walls, src, kind, ("wide levels", n))
    sizes = np.bincount(want[want >= 0].ravel())
    assert sizes.max() > cap, (sizes, cap)                              # the reference's widest level exceeds the capacity
    assert mx.widest_level(want)[0] == sizes.max()
    if kind != ex.TURNS:
        assert sizes[0] == m * m <= cap and sizes[1] > cap and sizes[-1] <= cap      # queue, scan, ..., queue again


def test_default_kinds_and_the_cache():
    """The class's own kind is the default; the default goal field is built once per set_task and dropped by the next."""
    table, other = sample_table(4, 9, 31), sample_table(4, 9, 32)
    walls, _, goal = table_arrays(table)
    for name, kind in (("2d", ex.MOVES_2D), ("disc", ex.TURNS), ("cont", ex.CELLS_3D)):
        env = make(name, 3)
        env.set_task(table)
        f = env.distance_field()
        assert f.kind == kind and f.dist.shape == (4, ex.orientations(kind), 9, 9) and f.dist.device == torch.device(DEV)
        assert np.array_equal(f.numpy(), ex.distance_field_reference(walls, goal_masks(9, goal), kind))
        assert env.distance_field() is f and env.distance_field(kind=kind) is f
        assert env.distance_field(kind=ex.KIND_NAMES[kind]) is f
        assert env.distance_field(sources=torch.as_tensor(goal_masks(9, goal))) is not f            # only the default is kept
        env.set_task(other)
        g = env.distance_field()
        w2, _, g2 = table_arrays(other)
        assert g is not f and np.array_equal(g.numpy(), ex.distance_field_reference(w2, goal_masks(9, g2), kind))


# ------------------------------------------------------------------------------------------------ 2. expert_action
def _scatter(env, rs, n, N):
    """Random cells (walls, sources and unreachable cells among them) and headings, through load_state_dict."""
    sd = env.state_dict()
    sd["grid"] = torch.as_tensor(rs.randint(0, n, (2, N)).astype(np.int32))
    sd["ori_idx"] = torch.as_tensor(rs.randint(0, 4, N).astype(np.int32))
    env.load_state_dict(sd)
    return sd["grid"].numpy(), sd["ori_idx"].numpy()


def _reference_actions(field, walls, task_id, grid, ori):
    return np.array([ex.expert_action_reference(field[task_id[e]], walls[task_id[e]], grid[:, e], ori[e])
                     for e in range(len(task_id))], np.int32)


@pytest.mark.parametrize("name", ["2d", "disc"])
def test_expert_action_on_scattered_states(name):
    kind = ex.MOVES_2D if name == "2d" else ex.TURNS
    tables = _tables_n9()
    walls, src = np.stack([w for _, w, _ in tables]), np.stack([s for _, _, s in tables])
    N, T = 448, len(tables)
    env = make(name, N)
    env.set_task([mx.task_of(w, (1, 1), (7, 7)) for w in walls])
    env.reset()
    field = env.distance_field(torch.as_tensor(src), kind)
    ref = field.numpy()
    rs = np.random.RandomState(5)
    task_id = env.task_id.cpu().numpy()
    seen = set()
    for rep in range(3):
        grid, ori = _scatter(env, rs, 9, N)
        if name == "2d":
            ori = np.zeros(N, np.int32)
        keep = env.state_dict()
        got = env.expert_action(field)
        assert got.dtype == torch.int32 and got.shape == (N,)
        want = _reference_actions(ref, walls, task_id, grid, ori)
        assert np.array_equal(got.cpu().numpy(), want), rep
        for key, v in env.state_dict().items():                         # nothing but the action buffer is written
            assert torch.equal(v, keep[key]), key
        d = ref[task_id, ori, grid[0], grid[1]]
        seen |= {"source"} if (d == 0).any() else set()
        seen |= {"unreachable"} if (d < 0).any() else set()
        seen |= {"heading %d" % o for o in np.unique(ori)}
        seen |= {"action %d" % a for a in np.unique(want)}
    # (with turns the expert never needs action 1: turning the other way and walking backward is as short, and 0 is lower)
    need = {"source", "unreachable", "action 0", "action 2", "action 3"}
    need |= {"heading %d" % o for o in range(4)} if name == "disc" else {"heading 0", "action 1"}
    assert need <= seen, need - seen
    # the default field is the goal's
    grid, ori = _scatter(env, rs, 9, N)
    goal = ex.distance_field_reference(walls, goal_masks(9, [(7, 7)] * T), kind)
    want = _reference_actions(goal, walls, task_id, grid, ori if name == "disc" else np.zeros(N, np.int32))
    assert np.array_equal(env.expert_action().cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 3. the 2-D closed loop
def _same_sd(sa, sb, what):
    assert sorted(sa) == sorted(sb)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), (what, key)


def _results_from_records(res):
    """ret_total: the T float64 rewards added in step order; ret_episode / episode_len: up to and including the first done;
    episodes: the number of steps with done."""
    r64, dn = res.reward64.cpu().numpy(), res.done.cpu().numpy().astype(bool)
    T, N = r64.shape
    total, epi = np.zeros(N), np.zeros(N)
    length, ended = np.zeros(N, np.int32), np.zeros(N, bool)
    for t in range(T):
        total = total + r64[t]
        epi = np.where(ended, epi, epi + r64[t])
        length = length + (~ended).astype(np.int32)
        ended = ended | dn[t]
    assert np.array_equal(res.ret_total.cpu().numpy(), total)
    assert np.array_equal(res.ret_episode.cpu().numpy(), epi)
    assert np.array_equal(res.episode_len.cpu().numpy(), length)
    assert np.array_equal(res.episodes.cpu().numpy(), dn.sum(0).astype(np.int32))
    assert np.array_equal(res.reward.cpu().numpy(), r64.astype(np.float32))


def _closed_loop(n, task_type, auto_reset, seed=0):
    """A fresh env over 8 sampled tasks, N = 64, and what the checks need: (env, walls, start distance per env, the field)."""
    table = sample_table(8, n, 200 + n + seed, food_density=0.1, food_interval=4, initial_life=1.0)
    walls, start, goal = table_arrays(table)
    env = make("2d", 64, task_type=task_type, auto_reset=auto_reset)
    env.set_task(table)
    env.reset()
    ref = ex.distance_field_reference(walls, goal_masks(n, goal), ex.MOVES_2D)
    task_id = env.task_id.cpu().numpy()
    d = np.array([ref[t, 0][tuple(start[t])] for t in task_id])
    return env, walls, d, ref, task_id


def _check_replay(env, res, sd0, what, walls=None, ref=None, task_id=None):
    """The recorded actions through rollout() and through step() from the same snapshot: reward64, done, the results and the
    end state bit for bit. With `ref`: every recorded action is `expert_action_reference` on the state before its step."""
    T = res.actions.shape[0]
    sd1, obs1 = env.state_dict(), env._obs.clone()
    env.load_state_dict(sd0)
    obs, rew, done, info = env.rollout(res.actions)
    assert torch.equal(env.rollout_reward64, res.reward64) and torch.equal(rew, res.reward) and torch.equal(done, res.done), what
    assert torch.equal(obs, obs1), what
    _same_sd(env.state_dict(), sd1, (what, "rollout"))
    env.load_state_dict(sd0)
    acts = res.actions.cpu().numpy()
    for t in range(T):
        if ref is not None:
            grid = env.grid.cpu().numpy()
            want = _reference_actions(ref, walls, task_id, grid, np.zeros(len(task_id), np.int32))
            assert np.array_equal(acts[t], want), (what, "action of step %d" % t)
        o, r, d, _ = env.step(res.actions[t])
        assert torch.equal(env.reward64, res.reward64[t]) and torch.equal(d, res.done[t]), (what, t)
    assert torch.equal(o, obs1), what
    _same_sd(env.state_dict(), sd1, (what, "step"))
    _results_from_records(res)


@pytest.mark.parametrize("n", [9, 15])
def test_closed_loop_escape_reaches_the_goal_at_dist_of_start(n):
    env, walls, d, ref, task_id = _closed_loop(n, "ESCAPE", False)
    T = int(d.max()) + 3
    sd0 = env.state_dict()
    res = env.rollout_expert(T, record=True)
    assert res.state is None and res.actions.shape == (T, 64) and res.actions.dtype == torch.int32 and res.done.dtype == torch.bool
    assert res.obs.data_ptr() == env._obs.data_ptr() and res.obs_steps == [T - 1]
    done = res.done.cpu().numpy()
    first = done.argmax(0) + 1
    assert done.any(0).all() and np.array_equal(first, d), (first, d)   # the first done of env e is at step dist[task, start]
    assert np.array_equal(res.episode_len.cpu().numpy(), d)
    step_r, goal_r = -0.01, 1.0
    assert np.allclose(res.ret_episode.cpu().numpy(), d * step_r + goal_r, rtol=0, atol=1e-12)
    _check_replay(env, res, sd0, ("escape", n), walls, ref, task_id)
    # record=False: the same results and end state, nothing per step
    sd1 = env.state_dict()
    env.load_state_dict(sd0)
    lean = env.rollout_expert(T)
    assert lean.actions is None and lean.reward is None and lean.reward64 is None and lean.done is None
    for name in ("ret_total", "ret_episode", "episode_len", "episodes"):
        assert torch.equal(getattr(lean, name), getattr(res, name)), name
    _same_sd(env.state_dict(), sd1, "record=False")


@pytest.mark.parametrize("n", [9, 15])
def test_closed_loop_escape_with_auto_reset(n):
    env, walls, d, ref, task_id = _closed_loop(n, "ESCAPE", True)
    T = 3 * int(d.max()) + 1
    sd0 = env.state_dict()
    res = env.rollout_expert(T, record=True, obs_every=7)
    assert np.array_equal(res.episodes.cpu().numpy(), T // d)           # every episode takes exactly dist[start] steps
    assert np.array_equal(res.done.cpu().numpy().argmax(0) + 1, d)
    from metagym_amd.metamaze import rollout_obs_steps
    assert res.obs_steps == rollout_obs_steps(T, 7) and res.obs.shape == (len(res.obs_steps),) + tuple(env._obs.shape)
    assert torch.equal(res.obs[-1], env._obs)
    sd1 = env.state_dict()
    env.load_state_dict(sd0)
    obs, _, _, _ = env.rollout(res.actions, obs_every=7)
    assert torch.equal(obs, res.obs)
    env.load_state_dict(sd1)
    _check_replay(env, res, sd0, ("escape, auto_reset", n), walls, ref, task_id)


@pytest.mark.parametrize("auto_reset", [False, True], ids=["noreset", "autoreset"])
def test_closed_loop_survival_replays(auto_reset):
    """SURVIVAL: the expert descends the field it is given (here: the goal's); the replay identity is the same."""
    env, walls, d, ref, task_id = _closed_loop(9, "SURVIVAL", auto_reset, seed=1)
    env.max_steps = 25
    sd0 = env.state_dict()
    res = env.rollout_expert(60, record=True)
    assert bool(res.done.any())                                         # episodes ended (max_steps) inside the rollout
    _check_replay(env, res, sd0, ("survival", auto_reset), walls, ref, task_id)


# ------------------------------------------------------------------------------------------------ 4. discrete 3-D, capture
def test_discrete_3d_loop_reaches_the_goal_at_dist_of_start():
    table = sample_table(8, 9, 77)
    walls, start, goal = table_arrays(table)
    env = make("disc", 16)
    env.set_task(table)
    env.reset()
    ref = ex.distance_field_reference(walls, goal_masks(9, goal), ex.TURNS)
    task_id = env.task_id.cpu().numpy()
    d = np.array([ref[t, 0][tuple(start[t])] for t in task_id])         # ori_idx is 0 at reset
    first = np.zeros(16, np.int64)
    for k in range(1, int(d.max()) + 1):
        want = _reference_actions(ref, walls, task_id, env.grid.cpu().numpy(), env.ori_idx.cpu().numpy())
        a = env.expert_action()
        assert np.array_equal(a.cpu().numpy(), want), k
        _, _, done, _ = env.step(a)
        dn = done.cpu().numpy()
        first = np.where((first == 0) & dn, k, first)
    assert np.array_equal(first, d), (first, d)


def test_graph_capture_of_step_expert_action():
    from test_graph_capture_gpu import _capture
    table = sample_table(8, 9, 91)
    eager, env = (make("2d", 64, auto_reset=True) for _ in range(2))
    for e in (eager, env):
        e.set_task(table)
        e.reset()
    sd0 = env.state_dict()
    out = {}

    def run():
        out["step"] = env.step(env.expert_action())

    graph = _capture(run)
    env.load_state_dict(sd0)                                            # the warm-up and the capture pass advanced the state
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        act = eager.expert_action().clone()
        o, r, d, _ = eager.step(act)
        go, gr, gd, _ = out["step"]
        assert torch.equal(env._expert_action, act) and torch.equal(go, o) and torch.equal(gr, r) and torch.equal(gd, d), rep
        _same_sd(env.state_dict(), eager.state_dict(), rep)
    assert int(env.steps.max()) == 2


def test_graph_capture_of_rollout_expert():
    from test_graph_capture_gpu import _capture
    table = sample_table(8, 9, 92)
    eager, env = (make("2d", 64, auto_reset=True) for _ in range(2))
    for e in (eager, env):
        e.set_task(table)
        e.reset()
    sd0 = env.state_dict()
    out = {}

    def run():
        out["res"] = env.rollout_expert(11, record=True, obs_every=4)

    graph = _capture(run)
    env.load_state_dict(sd0)
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        want, got = eager.rollout_expert(11, record=True, obs_every=4), out["res"]
        for name in ("actions", "reward", "reward64", "done", "obs", "ret_total", "ret_episode", "episode_len", "episodes"):
            assert torch.equal(getattr(got, name), getattr(want, name)), (rep, name)
        _same_sd(env.state_dict(), eager.state_dict(), rep)
    assert bool(out["res"].done.any())


# ------------------------------------------------------------------------------------------------ 5. refused calls
def test_refused_calls_leave_the_env_and_the_field_unchanged():
    fresh = make("2d", 8)
    for call in (fresh.distance_field, fresh.expert_action, lambda: fresh.rollout_expert(3)):
        with pytest.raises(Exception, match="set_task"):
            call()
    table = sample_table(4, 9, 41)
    fresh.set_task(table)
    fresh.distance_field()                                              # needs the table only
    for call in (fresh.expert_action, lambda: fresh.rollout_expert(3)):
        with pytest.raises(Exception, match="reset"):
            call()

    env = make("2d", 8)
    env.set_task(table)
    env.reset()
    env.rollout_expert(2)
    good = env.distance_field()
    other_n, other_T = make("2d", 8), make("2d", 8)
    other_n.set_task(sample_table(4, 15, 42))
    other_T.set_task(sample_table(5, 9, 43))
    fields = {"another n": other_n.distance_field(), "another T": other_T.distance_field(),
              "another kind": env.distance_field(kind=ex.CELLS_3D), "turns": env.distance_field(kind=ex.TURNS),
              "another device": ex.MazeDistanceField(good.dist.cpu(), ex.MOVES_2D, 9)}
    keep = {k: f.dist.clone() for k, f in fields.items()}
    sd, obs = env.state_dict(), env._obs.clone()

    def unchanged(what):
        _same_sd(env.state_dict(), sd, what)
        assert torch.equal(env._obs, obs), what
        for k, f in fields.items():
            assert torch.equal(f.dist, keep[k]), (what, k)

    for what, f in fields.items():
        for call in (lambda: env.expert_action(f), lambda: env.rollout_expert(3, f)):
            with pytest.raises(ValueError):
                call()
            unchanged(what)
    for call in (lambda: env.expert_action(good.dist), lambda: env.rollout_expert(3, good.numpy())):
        with pytest.raises(TypeError):
            call()
    for steps in (0, -2):
        with pytest.raises(ValueError):
            env.rollout_expert(steps)
    with pytest.raises(ValueError):
        env.rollout_expert(3, obs_every=-1)
    for bad in (torch.zeros(4, 9, 8, dtype=torch.bool), torch.zeros(3, 9, 9, dtype=torch.uint8), torch.zeros(4, 9, 9)):
        with pytest.raises(ValueError):
            env.distance_field(bad)
    with pytest.raises(ValueError):
        env.distance_field(kind=3)
    unchanged("the rest")
    assert env.distance_field() is good                                 # and the cache survived all of it

    cont = make("cont", 2)
    cont.set_task(table)
    cont.reset()
    with pytest.raises(NotImplementedError):
        cont.expert_action()
    disc = make("disc", 2)
    disc.set_task(table)
    disc.reset()
    with pytest.raises(ValueError):
        disc.expert_action(good)                                        # a MOVES_2D field for the env of turns
    assert not hasattr(disc, "rollout_expert")
