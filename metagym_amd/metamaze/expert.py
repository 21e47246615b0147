"""MetaMaze shortest-path fields and the expert that descends them — the host side of csrc/maze_expert.hip.

The reference has no such function. The numbers are defined here, by `distance_field_reference` and
`expert_action_reference`, and tied to the reference's step rules by the tests (tests/test_maze_expert.py plays the expert
through the CPU oracle of the maze).

`dist[t, k, x, y]` is the smallest number of env steps that takes state (orientation k, cell (x, y)) of task t onto a source
cell: 0 on a source in every orientation, -1 where no source can be reached. A step is judged by the cell it enters, as the
env's step does, so a wall cell beside a free one has a distance too. Three kinds (include/metagym_hip.h):

  MOVES_2D (K = 1)  MetaMaze2D: a move into c' is possible iff c' is inside the grid and walls[c'] < 1 (maze_2d.py:27).
                    Off-grid is impassable: the reference's negative-index wrap is not followed (sampled mazes have closed
                    borders, so the difference never shows there).
  CELLS_3D (K = 1)  the same with walls[c'] == 0 (maze_discrete_3d.py:63-65): the cell-level field of the continuous maze.
  TURNS    (K = 4)  MetaMazeDiscrete3D: state (ori_idx, cell); turn -1, turn +1, one cell backward, one cell forward cost one
                    step each (maze_discrete_3d.py:51-72), into walls == 0 inside the grid.
"""
from collections import deque

import numpy as np

MOVES_2D, CELLS_3D, TURNS = 0, 1, 2                       # MG_MAZE_FIELD_*
KIND_NAMES = {MOVES_2D: "MOVES_2D", CELLS_3D: "CELLS_3D", TURNS: "TURNS"}
DISCRETE_ACTIONS = [(-1, 0), (1, 0), (0, -1), (0, 1)]     # maze_env.py:14
HEADINGS = [(1, 0), (0, 1), (-1, 0), (0, -1)]             # maze_discrete_3d.py:51-60: the cell one step forward of ori_idx 0..3


def check_kind(kind):
    """The kind as an int; a name ("MOVES_2D", ...) is accepted too. ValueError for anything else."""
    if isinstance(kind, str):
        for k, name in KIND_NAMES.items():
            if name == kind:
                return k
        raise ValueError("unknown distance-field kind %r (one of %s)" % (kind, sorted(KIND_NAMES.values())))
    if isinstance(kind, (bool, float)) or int(kind) not in KIND_NAMES:
        raise ValueError("unknown distance-field kind %r (MOVES_2D = 0, CELLS_3D = 1, TURNS = 2)" % (kind,))
    return int(kind)


def orientations(kind):
    return 4 if check_kind(kind) == TURNS else 1


def passable(walls, kind):
    """The cells a step can enter, bool, same shape as `walls`."""
    walls = np.asarray(walls)
    return walls < 1 if check_kind(kind) == MOVES_2D else walls == 0


class MazeDistanceField(object):
    """A field on the device: `dist` int32 [T, K, n, n], its `kind` and `n`. What `env.distance_field` returns and
    `env.expert_action` / `MetaMaze2D.rollout_expert` take."""
    __slots__ = ("dist", "kind", "n")

    def __init__(self, dist, kind, n):
        kind, n = check_kind(kind), int(n)
        if getattr(dist, "dim", None) is None or dist.dim() != 4 or tuple(dist.shape[1:]) != (orientations(kind), n, n):
            raise ValueError("dist must be [T, %d, %d, %d] for kind %s, got %s"
                             % (orientations(kind), n, n, KIND_NAMES[kind], tuple(getattr(dist, "shape", ()))))
        import torch
        if dist.dtype != torch.int32 or not dist.is_contiguous():
            raise ValueError("dist must be a contiguous int32 tensor")
        self.dist, self.kind, self.n = dist, kind, n

    @property
    def num_tasks(self):
        return int(self.dist.shape[0])

    @property
    def device(self):
        return self.dist.device

    def numpy(self):
        return self.dist.cpu().numpy()


def _successor(walls, kind, ori, x, y, action):
    """The state after `action` under the step's own rule; None when the 2-D step leaves the grid (its negative-index wrap)."""
    n = walls.shape[0]
    if kind == TURNS:
        # maze_env.py:59-75 -> maze_discrete_3d.py:51-72: turn first, then move along the new heading
        turn, step = DISCRETE_ACTIONS[action]
        ori = (ori + turn) % 4
        tx, ty = x + step * HEADINGS[ori][0], y + step * HEADINGS[ori][1]
        if 0 <= tx < n and 0 <= ty < n and walls[tx, ty] == 0:
            x, y = tx, ty
        return ori, x, y
    tx, ty = x + DISCRETE_ACTIONS[action][0], y + DISCRETE_ACTIONS[action][1]
    if tx < n and ty < n and walls[tx, ty] < 1:              # maze_2d.py:24-29, python's negative index included
        if tx < 0 or ty < 0:
            return None
        x, y = tx, ty
    return 0, x, y


def distance_field_reference(walls, sources, kind):
    """The definition, on the host: a breadth-first search backwards from the sources, task by task. `walls` [T, n, n] (or
    [n, n]: one task), `sources` a mask of the same shape (nonzero = source). Returns int32 [T, K, n, n]."""
    kind = check_kind(kind)
    walls = np.asarray(walls)
    sources = np.asarray(sources)
    if walls.ndim == 2:
        walls, sources = walls[None], sources[None] if sources.ndim == 2 else sources
    if walls.ndim != 3 or walls.shape[1] != walls.shape[2] or sources.shape != walls.shape:
        raise ValueError("walls and sources must both be [T, n, n], got %s and %s" % (walls.shape, sources.shape))
    T, n = walls.shape[0], walls.shape[1]
    K = orientations(kind)
    out = np.full((T, K, n, n), -1, np.int32)
    for t in range(T):
        free = passable(walls[t], kind).tolist()
        d = [[[-1] * n for _ in range(n)] for _ in range(K)]
        queue = deque()
        for x, y in zip(*np.nonzero(sources[t])):
            for k in range(K):
                d[k][x][y] = 0
                queue.append((k, int(x), int(y)))
        while queue:
            k, x, y = queue.popleft()
            nxt = d[k][x][y] + 1
            if kind == TURNS:                        # the states one action leads here from
                preds = [((k + 1) % 4, x, y), ((k + 3) % 4, x, y)]
                if free[x][y]:
                    hx, hy = HEADINGS[k]
                    preds += [(k, x - hx, y - hy), (k, x + hx, y + hy)]
            else:
                preds = [(0, x - 1, y), (0, x + 1, y), (0, x, y - 1), (0, x, y + 1)] if free[x][y] else []
            for pk, px, py in preds:
                if 0 <= px < n and 0 <= py < n and d[pk][px][py] < 0:
                    d[pk][px][py] = nxt
                    queue.append((pk, px, py))
        out[t] = np.asarray(d, np.int32)
    return out


def expert_action_reference(field, task, grid, ori_idx=0):
    """The expert's action in one state, on the host: the lowest a in 0..3 whose successor under the step's own rule has
    dist == dist(current) - 1; 0 if there is none (on a source, in an unreachable state, off the grid). `field` is the task's
    slice [K, n, n] of a field (numpy; K = 1: the 2-D env's moves, K = 4: the discrete 3-D env's turns and moves), `task` the
    TaskConfig (or its cell_walls [n, n]) whose walls the step rule reads, `grid` the agent's cell (x, y), `ori_idx` its
    heading (K = 4 only). A successor off the grid (the 2-D step's wrap through a free border cell) is never chosen."""
    field = np.asarray(field)
    if field.ndim != 3 or field.shape[0] not in (1, 4) or field.shape[1] != field.shape[2]:
        raise ValueError("field must be one task's [K, n, n] slice with K = 1 or 4, got %s" % (field.shape,))
    kind = TURNS if field.shape[0] == 4 else MOVES_2D
    walls = np.asarray(getattr(task, "cell_walls", task))
    n = field.shape[-1]
    if walls.shape != (n, n):
        raise ValueError("the task's walls are %s, the field is for n = %d" % (walls.shape, n))
    x, y = int(grid[0]), int(grid[1])
    o = int(ori_idx) & 3 if kind == TURNS else 0
    if not (0 <= x < n and 0 <= y < n):
        return 0
    d0 = int(field[o, x, y])
    if d0 <= 0:
        return 0
    for a in range(4):
        nxt = _successor(walls, kind, o, x, y, a)
        if nxt is not None and int(field[nxt]) == d0 - 1:
            return a
    return 0


STEER_TAN9 = float(np.float32(0.15838444))                # tan(9 deg) as a float32: half of the 18 deg one step at turn +-1 rotates


def steer_action_reference(field, task, grid, loc, ori):
    """The steering expert of the continuous maze in one state, on the host: the (turn, walk) that takes the agent one cell
    down a CELLS_3D field, one of (0, 0), (0, 1), (1, 0), (-1, 0). The device code (csrc/maze_expert.hip me_steer_pick)
    reproduces it bit for bit; every decision is a comparison. `field` is the task's slice [1, n, n], `task` the TaskConfig
    (or a pair (cell_walls [n, n], cell_size)), `grid` the agent's cell, `loc` its float32 location, `ori` its float64
    heading.
      1. off the grid, or d0 = field[cell] <= 0 (a source, unreachable): (0, 0);
      2. the target cell is the first of DISCRETE_ACTIONS' four neighbours inside the grid with walls == 0 and field == d0 - 1;
         none: (0, 0);
      3. the target point is that cell's centre in float32, v = p - loc in float32, widened to float64;
      4. the heading is (float32(cos(ori)), float32(sin(ori))), cos / sin of the float64 `ori` as the renderer takes them,
         widened to float64: a last-bit difference between two libms cannot move a comparison;
      5. c = hx * vy - hy * vx, d = hx * vx + hy * vy in float64 (the products are exact, one rounding each);
      6. d > 0 and |c| <= STEER_TAN9 * d: walk, (0, 1); else turn towards the target, (c >= 0 ? 1 : -1, 0). The target exactly
         behind (c == 0, d <= 0) turns +1."""
    field = np.asarray(field)
    if field.ndim != 3 or field.shape[0] != 1 or field.shape[1] != field.shape[2]:
        raise ValueError("field must be one task's [1, n, n] slice of a CELLS_3D field, got %s" % (field.shape,))
    if hasattr(task, "cell_walls"):
        walls, cell_size = np.asarray(task.cell_walls), task.cell_size
    else:
        walls, cell_size = np.asarray(task[0]), task[1]
    n = field.shape[-1]
    if walls.shape != (n, n):
        raise ValueError("the task's walls are %s, the field is for n = %d" % (walls.shape, n))
    x, y = int(grid[0]), int(grid[1])
    if not (0 <= x < n and 0 <= y < n):
        return (0.0, 0.0)
    d0 = int(field[0, x, y])
    if d0 <= 0:
        return (0.0, 0.0)
    target = None
    for dx, dy in DISCRETE_ACTIONS:
        tx, ty = x + dx, y + dy
        if 0 <= tx < n and 0 <= ty < n and walls[tx, ty] == 0 and int(field[0, tx, ty]) == d0 - 1:
            target = (tx, ty)
            break
    if target is None:
        return (0.0, 0.0)
    f32 = np.float32
    cs = f32(cell_size)
    px, py = (f32(target[0]) + f32(0.5)) * cs, (f32(target[1]) + f32(0.5)) * cs
    vx, vy = np.float64(px - f32(loc[0])), np.float64(py - f32(loc[1]))
    ori = np.float64(ori)
    hx, hy = np.float64(f32(np.cos(ori))), np.float64(f32(np.sin(ori)))
    c = hx * vy - hy * vx
    d = hx * vx + hy * vy
    if d > 0 and abs(c) <= np.float64(STEER_TAN9) * d:
        return (0.0, 1.0)
    return (1.0 if c >= 0 else -1.0, 0.0)
