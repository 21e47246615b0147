"""Test helper for the maze distance fields: an oracle that shares no code with metagym_amd.metamaze.expert, and the
hand-built tables both test files use.

`relaxation_field` states every step rule FORWARDS, as a successor table succ[s, a] written from the reference's own lines
(maze_2d.py:24-29 without the negative-index wrap, maze_discrete_3d.py:51-72), and relaxes
    d[s] = 0 on a source, else min(d[s], 1 + min_a d[succ[s, a]])
over all states at once until nothing changes (Bellman-Ford, at most S rounds). No queue, no search order."""
import numpy as np

MOVES_2D, CELLS_3D, TURNS = 0, 1, 2
MOVES = [(-1, 0), (1, 0), (0, -1), (0, 1)]                # DISCRETE_ACTIONS maze_env.py:14
INF = np.int64(1) << 40


def successor_table(walls, kind):
    """int64 [K * n * n, 4]: the state each action leads to (state = k * n * n + x * n + y). A blocked move stays."""
    walls = np.asarray(walls)
    n = walls.shape[0]
    K = 4 if kind == TURNS else 1
    x, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    enter = (walls < 1) if kind == MOVES_2D else (walls == 0)
    succ = np.zeros((K, n, n, 4), np.int64)

    def moved(k, dx, dy):
        tx, ty = x + dx, y + dy
        inside = (tx >= 0) & (tx < n) & (ty >= 0) & (ty < n)
        ok = inside & enter[np.clip(tx, 0, n - 1), np.clip(ty, 0, n - 1)]
        return k * n * n + np.where(ok, tx, x) * n + np.where(ok, ty, y)

    if kind == TURNS:
        heading = [(1, 0), (0, 1), (-1, 0), (0, -1)]      # ori_idx 0..3: +x, +y, -x, -y (maze_discrete_3d.py:51-60)
        for k in range(4):
            succ[k, :, :, 0] = ((k - 1) % 4) * n * n + x * n + y
            succ[k, :, :, 1] = ((k + 1) % 4) * n * n + x * n + y
            succ[k, :, :, 2] = moved(k, -heading[k][0], -heading[k][1])
            succ[k, :, :, 3] = moved(k, heading[k][0], heading[k][1])
    else:
        for a, (dx, dy) in enumerate(MOVES):
            succ[0, :, :, a] = moved(0, dx, dy)
    return succ.reshape(K * n * n, 4)


def relaxation_field(walls, sources, kind):
    """int32 [T, K, n, n] for walls / sources [T, n, n]."""
    walls, sources = np.asarray(walls), np.asarray(sources)
    T, n = walls.shape[0], walls.shape[1]
    K = 4 if kind == TURNS else 1
    out = np.zeros((T, K, n, n), np.int32)
    for t in range(T):
        succ = successor_table(walls[t], kind)
        src = np.broadcast_to(sources[t].astype(bool), (K, n, n)).reshape(-1)
        d = np.where(src, 0, INF)
        for _ in range(K * n * n + 1):
            new = np.where(src, 0, np.minimum(d, 1 + d[succ].min(axis=1)))
            if np.array_equal(new, d):
                break
            d = new
        else:
            raise AssertionError("the relaxation did not settle in S rounds")
        out[t] = np.where(d >= INF, -1, d).reshape(K, n, n).astype(np.int32)
    return out


def widest_level(field):
    """The largest number of states any one distance has, per task: the widest frontier of a level-synchronous search."""
    return [int(np.bincount(f[f >= 0].ravel()).max()) if (f >= 0).any() else 0 for f in field]


# ---------------------------------------------------------------------------------------------- tables
def room(n):
    """Border walls, free inside."""
    w = np.ones((n, n), np.int32)
    w[1:-1, 1:-1] = 0
    return w


def serpentine(n):
    """One corridor snaking through the odd rows: row 1 left to right, down at the end, row 3 back, ... (n odd)."""
    w = np.ones((n, n), np.int32)
    for i, r in enumerate(range(1, n - 1, 2)):
        w[r, 1:-1] = 0
        if r + 2 < n - 1:
            w[r + 1, n - 2 if i % 2 == 0 else 1] = 0
    return w


def enclosed(n):
    """A room with a walled 3 x 3 chamber in the middle: from outside, the chamber's centre cannot be reached."""
    w = room(n)
    c = n // 2
    w[c - 2:c + 3, c - 2:c + 3] = 1
    w[c - 1:c + 2, c - 1:c + 2] = 0
    return w


def free_border(n):
    """No border at all on two sides and gaps in the others: a step rule that wrapped would find shortcuts here."""
    w = np.zeros((n, n), np.int32)
    w[n // 2, 1:] = 1                                     # a wall across, open only at column 0
    w[-1, 2:-2] = 1
    return w


def with_minus_one(n):
    """A room cut in two by a wall whose only gap holds -1: a door for the 2-D rule (walls < 1), a wall for walls == 0."""
    w = room(n)
    w[n // 2, :] = 1
    w[n // 2, n // 2] = -1
    return w


def mask(n, cells):
    m = np.zeros((n, n), np.uint8)
    for c in cells:
        m[c] = 1
    return m


def hand_tables(n):
    """[(name, walls [n, n], sources [n, n])] for an odd n >= 5 (the n = 5 chamber is a single cell)."""
    c = n // 2
    out = [("room", room(n), mask(n, [(1, 1)])),
           ("serpentine", serpentine(n), mask(n, [(1, 1)])),
           ("free_border", free_border(n), mask(n, [(0, n - 1)])),
           ("minus_one", with_minus_one(n), mask(n, [(1, 1)])),
           ("multi_source", room(n), mask(n, [(1, 1), (n - 2, n - 2), (1, n - 2)])),
           ("no_source", room(n), mask(n, [])),
           ("source_in_wall", room(n), mask(n, [(0, 0), (c, c)]))]
    if n >= 7:
        out.append(("enclosed", enclosed(n), mask(n, [(c, c)])))
    return out


def task_of(walls, start, goal, step_reward=-0.01, goal_reward=1.0):
    """A TaskConfig around hand-built walls (no food)."""
    from metagym_amd.metamaze import TaskConfig
    walls = np.asarray(walls, np.int32)
    n = walls.shape[0]
    texts = np.where(walls > 0, 1, 0).astype(np.int64)
    return TaskConfig(start=tuple(start), goal=tuple(goal), cell_walls=walls, cell_texts=texts, cell_size=2.0, wall_height=3.2,
                      agent_height=1.6, initial_life=1.0, max_life=2.0, step_reward=step_reward, goal_reward=goal_reward,
                      food_rewards=np.zeros((n, n), np.float64), food_interval=np.zeros((n, n), np.int32))
