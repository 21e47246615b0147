"""MetaMaze shortest-path fields and the expert, host side (no GPU):
  1. `distance_field_reference` against an independent all-pairs relaxation (tests/maze_expert_oracle.py) for the three
     kinds, on hand-built n = 5 and n = 7 tables and host-sampled n = 9 mazes;
  2. `expert_action_reference` played through the pinned CPU oracle of the maze (oracle/maze_oracle.c) from reset reaches the
     goal at exactly step dist[start], in the 2-D env and in the discrete 3-D one, and at no earlier step;
  3. the Python-side refusals, and the library's host-side ones."""
import ctypes as C

import numpy as np
import pytest

import maze_expert_oracle as mx
from metagym_amd.metamaze import MAZE_TASK_MANAGER
from metagym_amd.metamaze import expert as ex
from oracle import maze as mo

KINDS = [ex.MOVES_2D, ex.CELLS_3D, ex.TURNS]
KIND_IDS = ["moves2d", "cells3d", "turns"]


def _sampled(n, seeds):
    return [MAZE_TASK_MANAGER.sample_task(n=n, allow_loops=bool(s % 2), step_reward=-0.01, goal_reward=1.0, seed=s) for s in seeds]


def _goal_mask(tasks):
    n = np.shape(tasks[0].cell_walls)[0]
    return np.stack([mx.mask(n, [tuple(t.goal)]) for t in tasks])


def test_constants_match_the_header_and_the_helper():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "metagym_hip.h")).read()
    m = re.search(r"enum \{ MG_MAZE_FIELD_MOVES_2D = (\d), MG_MAZE_FIELD_CELLS_3D = (\d), MG_MAZE_FIELD_TURNS = (\d) \}", text)
    assert m and tuple(int(v) for v in m.groups()) == (ex.MOVES_2D, ex.CELLS_3D, ex.TURNS) == (mx.MOVES_2D, mx.CELLS_3D, mx.TURNS)
    assert [ex.orientations(k) for k in KINDS] == [1, 1, 4]
    assert [ex.check_kind(name) for name in ("MOVES_2D", "CELLS_3D", "TURNS")] == KINDS


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("n", [5, 7])
def test_reference_is_the_relaxation_on_hand_built_tables(n, kind):
    tables = mx.hand_tables(n)
    walls = np.stack([w for _, w, _ in tables])
    src = np.stack([s for _, _, s in tables])
    got = ex.distance_field_reference(walls, src, kind)
    want = mx.relaxation_field(walls, src, kind)
    assert got.dtype == np.int32 and got.shape == (len(tables), ex.orientations(kind), n, n)
    for i, (name, _, _) in enumerate(tables):
        assert np.array_equal(got[i], want[i]), (name, n, kind)
    by_name = {name: got[i] for i, (name, _, _) in enumerate(tables)}
    # what the tables are for, stated once on the reference itself
    assert (by_name["no_source"] == -1).all()
    assert (by_name["room"] >= 0).sum() > 0 and (by_name["room"][:, 1, 1] == 0).all()         # 0 in every orientation
    if kind != ex.TURNS:
        x, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        inside = mx.room(n) == 0
        assert np.array_equal(by_name["room"][0][inside], (np.abs(x - 1) + np.abs(y - 1))[inside])   # the Manhattan distance
        far = by_name["minus_one"][0, n - 2, n - 2]
        assert (far > 0) if kind == ex.MOVES_2D else (far == -1)                          # -1 is a door for the 2-D rule only
    # no wrap: the cell (n - 1, n - 1) is one wrapped step from the source (0, n - 1) and many real ones
    assert by_name["free_border"][0, n - 1, n - 1] != 1
    if n >= 7:
        assert (by_name["enclosed"][:, 1, 1] == -1).all() and by_name["enclosed"][:, n // 2, n // 2 + 1].min() == 1


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_reference_is_the_relaxation_on_sampled_mazes(kind):
    tasks = _sampled(9, range(40, 46))
    walls = np.stack([np.asarray(t.cell_walls) for t in tasks])
    src = _goal_mask(tasks)
    got = ex.distance_field_reference(walls, src, kind)
    assert np.array_equal(got, mx.relaxation_field(walls, src, kind))
    for t, task in enumerate(tasks):                                    # a sampled maze is connected: the start reaches the goal
        assert got[t, 0][tuple(task.start)] > 0
    one = ex.distance_field_reference(walls[2], src[2], kind)           # one task without the leading axis
    assert np.array_equal(one[0], got[2])


def _oracle_task(t):
    return mo.Task(start=t.start, goal=t.goal, cell_walls=t.cell_walls, cell_texts=t.cell_texts, cell_size=t.cell_size,
                   wall_height=t.wall_height, agent_height=t.agent_height, initial_life=t.initial_life, max_life=t.max_life,
                   step_reward=t.step_reward, goal_reward=t.goal_reward, food_rewards=t.food_rewards, food_interval=t.food_interval)


def _tasks_for_play():
    hand = [mx.task_of(mx.serpentine(7), (1, 1), (5, 5)), mx.task_of(mx.room(7), (5, 1), (1, 4)),
            mx.task_of(mx.with_minus_one(7), (1, 1), (5, 5))]
    return hand + _sampled(9, range(50, 54)) + _sampled(15, range(60, 62))


@pytest.mark.parametrize("env", ["2d", "disc"])
def test_the_expert_reaches_the_goal_at_exactly_dist_of_start_in_the_cpu_oracle(env):
    kind = ex.MOVES_2D if env == "2d" else ex.TURNS
    step = mo.step_2d if env == "2d" else mo.step_disc3d
    played = 0
    for task in _tasks_for_play():
        walls = np.asarray(task.cell_walls)
        if env == "disc" and (walls < 0).any():
            continue                                                    # the -1 door is a wall for the 3-D rule
        n = walls.shape[0]
        field = ex.distance_field_reference(walls, mx.mask(n, [tuple(task.goal)]), kind)[0]
        want = int(field[0][tuple(task.start)])                         # ori_idx is 0 at reset
        assert want > 0
        ot = _oracle_task(task)
        st = mo.State(ot)
        mo.reset(ot, mo.ESCAPE, st)
        assert (st.c.grid[0], st.c.grid[1], st.c.ori_idx) == (task.start[0], task.start[1], 0)
        for k in range(1, want + 1):
            here = int(field[st.c.ori_idx & 3 if env == "disc" else 0, st.c.grid[0], st.c.grid[1]])
            assert here == want - (k - 1)                               # every step is one nearer
            a = ex.expert_action_reference(field, task, (st.c.grid[0], st.c.grid[1]), st.c.ori_idx)
            r, done = step(ot, mo.ESCAPE, 10 ** 6, st, a)
            assert done == (k == want), (env, k, want)
        assert (st.c.grid[0], st.c.grid[1]) == tuple(task.goal) and r == task.step_reward + task.goal_reward
        played += 1
    assert played >= 8


def test_expert_action_reference_rules():
    walls = mx.room(5)
    f2 = ex.distance_field_reference(walls, mx.mask(5, [(1, 3)]), ex.MOVES_2D)[0]
    assert ex.expert_action_reference(f2, walls, (3, 1)) == 0            # ties: (-1, 0) and (0, 1) both descend, the lowest wins
    assert ex.expert_action_reference(f2, walls, (1, 1)) == 3
    assert ex.expert_action_reference(f2, walls, (1, 3)) == 0            # on the source
    assert ex.expert_action_reference(f2, walls, (-1, 2)) == 0 and ex.expert_action_reference(f2, walls, (2, 5)) == 0
    none = ex.distance_field_reference(walls, mx.mask(5, []), ex.MOVES_2D)[0]
    assert ex.expert_action_reference(none, walls, (2, 2)) == 0          # unreachable
    f4 = ex.distance_field_reference(walls, mx.mask(5, [(3, 1)]), ex.TURNS)[0]
    assert ex.expert_action_reference(f4, walls, (1, 1), 0) == 3         # heading +x: forward
    assert ex.expert_action_reference(f4, walls, (1, 1), 2) == 2         # heading -x: backward is as short
    assert ex.expert_action_reference(f4, walls, (1, 1), 1) == 0 and f4[1, 1, 1] == 3   # +y: turn -1 to +x, then two forward
    assert ex.expert_action_reference(f4, walls, (1, 1), 5) == 0         # heading taken mod 4
    # the wrap of the 2-D step is never chosen: from (0, 4) the wrapped move up lands on (-1, 4)
    fb = mx.free_border(5)
    ff = ex.distance_field_reference(fb, mx.mask(5, [(4, 0)]), ex.MOVES_2D)[0]
    assert ex.expert_action_reference(ff, fb, (0, 0)) != 0 or ff[0, 0, 0] <= 0


def test_python_side_refusals():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        ex.check_kind(3)
    with pytest.raises(ValueError):
        ex.check_kind("MOVES")
    with pytest.raises(ValueError):
        ex.check_kind(1.0)
    walls = np.stack([mx.room(5)] * 2)
    with pytest.raises(ValueError):
        ex.distance_field_reference(walls, np.zeros((1, 5, 5), np.uint8), ex.MOVES_2D)        # masks of another T
    with pytest.raises(ValueError):
        ex.distance_field_reference(np.zeros((2, 5, 4)), np.zeros((2, 5, 4)), ex.MOVES_2D)   # not square
    with pytest.raises(ValueError):
        ex.distance_field_reference(walls, np.zeros((2, 5, 5)), 7)
    with pytest.raises(ValueError):
        ex.expert_action_reference(np.zeros((2, 5, 5), np.int32), walls[0], (1, 1))           # K is 1 or 4
    with pytest.raises(ValueError):
        ex.expert_action_reference(np.zeros((1, 5, 5), np.int32), mx.room(7), (1, 1))         # walls of another n
    ok = torch.zeros(2, 1, 5, 5, dtype=torch.int32)
    f = ex.MazeDistanceField(ok, ex.MOVES_2D, 5)
    assert (f.kind, f.n, f.num_tasks) == (ex.MOVES_2D, 5, 2) and f.numpy().shape == (2, 1, 5, 5)
    ex.MazeDistanceField(torch.zeros(2, 4, 5, 5, dtype=torch.int32), "TURNS", 5)
    for bad, kind, n in ((ok, ex.TURNS, 5), (ok, ex.MOVES_2D, 7), (ok.long(), ex.MOVES_2D, 5), (ok[0], ex.MOVES_2D, 5),
                         (ok.numpy(), ex.MOVES_2D, 5), (torch.zeros(2, 1, 5, 10, dtype=torch.int32)[..., ::2], ex.MOVES_2D, 5),
                         (ok, 9, 5)):
        with pytest.raises(ValueError):
            ex.MazeDistanceField(bad, kind, n)


def test_library_refusals_on_the_host():
    """Refused before anything is launched or dereferenced: an unknown kind, a NULL dist, a table the maze calls refuse, and
    the expert for the continuous maze's kind. The queue capacity is a positive constant."""
    from metagym_amd import _lib
    lib = _lib.load()
    cap = lib.mg_maze_distance_queue_capacity()
    assert cap > 0 and cap == lib.mg_maze_distance_queue_capacity()
    fake = C.c_void_p(64)                                               # never dereferenced by a refused call
    t = _lib.MazeTasks()
    t.n, t.n_tasks = 9, 1
    for k in ("start", "goal", "walls", "texts", "scalars"):
        setattr(t, k, 64)
    st = _lib.MazeState()
    st.task_id = st.grid = st.steps = 64
    NULL_POINTER, BAD_SIZE, BAD_CONFIG = -1001, -1002, -1003
    assert lib.mg_maze_distance_field(t, 3, None, fake, None) == BAD_CONFIG and b"kind" in lib.mg_last_error()
    assert lib.mg_maze_distance_field(t, -1, None, fake, None) == BAD_CONFIG
    assert lib.mg_maze_distance_field(t, ex.TURNS, None, None, None) == NULL_POINTER
    assert lib.mg_maze_distance_field(None, ex.TURNS, None, fake, None) == NULL_POINTER
    for n in (2, 256):
        t.n = n
        assert lib.mg_maze_distance_field(t, ex.MOVES_2D, None, fake, None) == BAD_SIZE
    t.n, t.walls = 9, None
    assert lib.mg_maze_distance_field(t, ex.MOVES_2D, None, fake, None) == NULL_POINTER
    t.walls = 64
    assert lib.mg_maze_expert_action(t, ex.CELLS_3D, fake, 4, st, fake, None) == BAD_CONFIG and b"expert" in lib.mg_last_error()
    assert lib.mg_maze_expert_action(t, 5, fake, 4, st, fake, None) == BAD_CONFIG
    assert lib.mg_maze_expert_action(t, ex.MOVES_2D, None, 4, st, fake, None) == NULL_POINTER
    assert lib.mg_maze_expert_action(t, ex.MOVES_2D, fake, 0, st, fake, None) == BAD_SIZE
    assert lib.mg_maze_expert_action(t, ex.TURNS, fake, 4, st, fake, None) == NULL_POINTER and b"ori_idx" in lib.mg_last_error()
    roll = lambda steps, every, dist=fake: lib.mg_maze2d_expert_rollout(t, 0, 100, 2, 0, 4, st, steps, every, dist, fake, fake, fake,
                                                                        fake, fake, None, None, None, None, None, None)
    assert roll(0, 0) == BAD_SIZE and roll(1, -1) == BAD_SIZE and roll(1, 0, None) == NULL_POINTER
