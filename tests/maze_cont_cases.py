"""Test helper for the continuous 3-D maze move: a restatement of the reference's formulas that counts every branch it
takes, and the placed cases the CPU and GPU tests of the move share (tests/test_maze_cont_edges.py, ..._gpu.py).

The restatement is written from dynamics.py:17-92 and maze_continuous_3d.py:47-56 (plus get_loc_grid / evaluation_rule,
maze_base.py:65-95, :199-202) in plain Python on NumPy scalars. It shares no code with oracle/maze_oracle.c or
csrc/maze.hip. Operand widths are spelled out with F (float32) and D (float64) at every operation, under the reading
DESIGN.md fixes ("NumPy 2.2.6 + emulated numba typing"):
  * float32 array elements stay float32 among themselves; numpy.sum over a two-element float32 array is one float32 add;
  * a python float argument of an @njit function and the result of max(...) are float64;
  * `f32_array /= f64` and `f32_array *= f64` compute in float64 and round the result to float32;
  * `dist` in collision_force is float64 both before and after nearest_point (numba unifies the two assignments);
  * numpy.float32(...) factors are float64 expressions rounded once;
  * vector_move_with_collision is plain NumPy: `exp_pos / cell_size` and `loc / cell_size` divide by a weak python
    float, so they are float32 divisions by float32(cell_size).

Nothing here needs a GPU, and nothing at module level imports the oracle."""
import collections
import functools

import numpy as np

F, D = np.float32, np.float64
PI, T_PI = D(3.1415926), D(6.2831852)                      # dynamics.py:6-7
CORNER_A, CORNER_B = (F(0.5), F(0.5)), (F(-0.5), F(0.5))   # OFFSET_10, OFFSET_01   dynamics.py:10-13
CORNER_C, CORNER_D = (F(-0.5), F(-0.5)), (F(0.5), F(-0.5))  # OFFSET_m0, OFFSET_0m
ESCAPE, SURVIVAL = 0, 1

# every census key; `GUARD_EDGE_NORM` cannot be taken (the four edges are constants of length 1) and is asserted to stay 0
KEYS_EDGES = ("edge_AB", "edge_BC", "edge_CD", "edge_DA")
KEYS_NEAREST = ("nearest_end_2", "nearest_end_1", "nearest_within")
KEYS_GUARDS = ("guard_inside_dist", "guard_ori_norm")
GUARD_EDGE_NORM = "guard_edge_norm"
KEYS_PUSHING = ("pushing_0", "pushing_1", "pushing_2", "pushing_3", "pushing_4")
KEYS_HEADING = ("wrap_down", "wrap_up", "clamp_turn_lo", "clamp_turn_hi", "clamp_walk_lo", "clamp_walk_hi", "backward_half")
ALL_KEYS = (("far", "inside") + KEYS_EDGES + KEYS_NEAREST + ("force", "no_force") + KEYS_GUARDS + ("neighbour_out_of_grid",)
            + KEYS_PUSHING + KEYS_HEADING)
# the comparisons of collision_force / nearest_point, as they appear in a trace
COMPARISONS = ("cmp_far", "cmp_in0", "cmp_in1", "cmp_xpos", "cmp_ypos", "cmp_gt_edge", "cmp_lt_zero", "cmp_eff_lt_d")


class Census(collections.Counter):
    """Branch counts; with `trace` a list, also the outcome of every comparison in the order evaluated."""
    trace = None

    def hit(self, key):
        self[key] += 1

    def cmp(self, name, outcome):
        if self.trace is not None:
            self.trace.append((name, bool(outcome)))
        return bool(outcome)


def _sum2(a, b):
    return F(a + b)                                         # numpy.sum of a float32 pair


def nearest_point(pos, l1, l2, cen):
    """dynamics.py:17-29 -> (float32 distance, float32 point)."""
    u0, u1 = F(l2[0] - l1[0]), F(l2[1] - l1[1])             # :18 f32
    edge_norm = F(np.sqrt(_sum2(F(u0 * u0), F(u1 * u1))))   # :19 f32
    if D(edge_norm) < D(1.0e-6):
        cen.hit(GUARD_EDGE_NORM)
    m = max(D(1.0e-6), D(edge_norm))                        # :20 max(...) is f64
    u0, u1 = F(D(u0) / m), F(D(u1) / m)                     #     f32 array /= f64: f64 quotient, rounded to f32
    dist_1 = _sum2(F(F(pos[0] - l1[0]) * u0), F(F(pos[1] - l1[1]) * u1))   # :22 f32
    if cen.cmp("cmp_gt_edge", dist_1 > edge_norm):          # :23 f32 against f32
        cen.hit("nearest_end_2")
        p = l2
    elif cen.cmp("cmp_lt_zero", dist_1 < 0):                # :25
        cen.hit("nearest_end_1")
        p = l1
    else:                                                   # :28 f32
        cen.hit("nearest_within")
        p = (F(l1[0] + F(dist_1 * u0)), F(l1[1] + F(dist_1 * u1)))
    d0, d1 = F(pos[0] - p[0]), F(pos[1] - p[1])
    return F(np.sqrt(_sum2(F(d0 * d0), F(d1 * d1)))), p


def collision_force(dv, cell_size, col_dist, cen):
    """dynamics.py:32-56 -> (float32 pair, pushes?). dv a float32 pair, cell_size / col_dist python floats (float64 inside)."""
    cs, cd = D(cell_size), D(col_dist)
    dist = D(F(np.sqrt(_sum2(F(dv[0] * dv[0]), F(dv[1] * dv[1])))))   # :33 f32 norm, float(...) -> f64
    eff = D(cd / cs)                                        # :34 f64
    if cen.cmp("cmp_far", dist > D(0.708) + eff):           # :35 f64
        cen.hit("far")
        return (F(0.0), F(0.0)), False
    if cen.cmp("cmp_in0", abs(dv[0]) < 0.5) and cen.cmp("cmp_in1", abs(dv[1]) < 0.5):   # :37
        cen.hit("inside")
        if not dist > D(1.0e-6):
            cen.hit("guard_inside_dist")
        k = F(D(0.50) / max(dist, D(1.0e-6)) * (D(0.708) + eff - dist) * cs)   # :38 f64 expression -> numpy.float32
        return (F(k * dv[0]), F(k * dv[1])), True
    x_pos = cen.cmp("cmp_xpos", F(dv[0] + dv[1]) > 0)       # :39 f32 sum
    y_pos = cen.cmp("cmp_ypos", F(dv[1] - dv[0]) > 0)       # :40
    if x_pos and y_pos:
        cen.hit("edge_AB")
        d, p = nearest_point(dv, CORNER_A, CORNER_B, cen)
    elif (not x_pos) and y_pos:
        cen.hit("edge_BC")
        d, p = nearest_point(dv, CORNER_B, CORNER_C, cen)
    elif (not x_pos) and (not y_pos):
        cen.hit("edge_CD")
        d, p = nearest_point(dv, CORNER_C, CORNER_D, cen)
    else:
        cen.hit("edge_DA")
        d, p = nearest_point(dv, CORNER_D, CORNER_A, cen)
    dist = D(d)                                             # f64 after the unification
    if cen.cmp("cmp_eff_lt_d", eff < dist):                 # :50
        cen.hit("no_force")
        return (F(0.0), F(0.0)), False
    cen.hit("force")
    o0, o1 = F(dv[0] - p[0]), F(dv[1] - p[1])               # :53 f32
    on = F(np.sqrt(_sum2(F(o0 * o0), F(o1 * o1))))          # :54 f32
    if D(on) < D(1.0e-6):
        cen.hit("guard_ori_norm")
    r = D(1.0) / max(D(1.0e-6), D(on))                      # :55 f64
    o0, o1 = F(D(o0) * r), F(D(o1) * r)                     #     f32 array *= f64: f64 product, rounded to f32
    k = F(D(0.50) * (eff - dist) * cs)                      # :56 f64 expression -> numpy.float32
    return (F(k * o0), F(k * o1)), True


def move(walls, cell_size, col_dist, loc, ori, turn, walk, cen, visited=None):
    """maze_continuous_3d.py:48-53 + dynamics.py:59-92: one env step without the evaluation rule. loc a float32 pair, ori
    float64, turn / walk python floats (the float32 action widened, as the env's step receives it). `visited` collects
    every sub-step's expected and final position. -> (ori f64, loc f32 pair, grid int pair)."""
    n = walls.shape[0]
    turn, walk = D(turn), D(walk)
    if turn < -1:                                           # numpy.clip(x, -1, 1), f64
        cen.hit("clamp_turn_lo")
        turn = D(-1.0)
    elif turn > 1:
        cen.hit("clamp_turn_hi")
        turn = D(1.0)
    if walk < -1:
        cen.hit("clamp_walk_lo")
        walk = D(-1.0)
    elif walk > 1:
        cen.hit("clamp_walk_hi")
        walk = D(1.0)
    turn_rate = D(turn * PI)
    walk_speed = walk
    if walk_speed < 0:                                      # dynamics.py:73-74
        cen.hit("backward_half")
        walk_speed = D(walk_speed * D(0.50))
    ori = D(ori)
    p0, p1 = F(loc[0]), F(loc[1])
    cs32 = F(cell_size)
    for _ in range(int(100 * 0.10)):                        # :76
        fin = D(ori + D(turn_rate * D(0.01)))               # vector_move :60-69, all f64
        off_ori = D(D(0.5) * D(fin + ori))
        off = D(walk_speed * D(0.01))
        d_x, d_y = F(D(np.cos(off_ori)) * off), F(D(np.sin(off_ori)) * off)
        while fin > T_PI:
            cen.hit("wrap_down")
            fin = D(fin - T_PI)
        while fin < 0:
            cen.hit("wrap_up")
            fin = D(fin + T_PI)
        ori = fin
        e0, e1 = F(p0 + d_x), F(p1 + d_y)                   # :78 f32
        c0, c1 = F(e0 / cs32), F(e1 / cs32)                 # :79 f32 / weak python float
        col0, col1 = F(0.0), F(0.0)
        pushing = 0
        for i in range(-1, 2):
            for j in range(-1, 2):
                w_i, w_j = i + int(c0), j + int(c1)         # :85-86 int() truncates
                if w_i > -1 and w_i < n and w_j > -1 and w_j < n:
                    if walls[w_i, w_j] > 0:                 # :88
                        dv = (F(F(c0 - F(np.floor(c0))) - F(i + 0.5)), F(F(c1 - F(np.floor(c1))) - F(j + 0.5)))   # :89
                        f, pushes = collision_force(dv, cell_size, col_dist, cen)
                        col0, col1 = F(col0 + f[0]), F(col1 + f[1])      # :90
                        pushing += int(pushes)
                else:
                    cen.hit("neighbour_out_of_grid")
        cen.hit("pushing_%d" % pushing)
        p0, p1 = F(col0 + e0), F(col1 + e1)                 # :91
        if visited is not None:
            visited.extend(((e0, e1), (p0, p1)))
    return ori, (p0, p1), (int(F(p0 / cs32)), int(F(p1 / cs32)))       # get_loc_grid maze_base.py:199-202


class Agent(object):
    """One env of the reference: reset (maze_base.py:40-63), do_action and evaluation_rule (:65-95)."""

    def __init__(self, task, task_type, max_steps, col_dist=0.20):
        self.task, self.task_type, self.max_steps, self.col_dist = task, task_type, int(max_steps), float(col_dist)
        self.walls = np.asarray(task["cell_walls"])
        self.census = Census()
        self.reset()

    def reset(self):
        t = self.task
        cs = float(t["cell_size"])
        self.grid = (int(t["start"][0]), int(t["start"][1]))
        self.loc = (F(self.grid[0] * cs + 0.5 * cs), F(self.grid[1] * cs + 0.5 * cs))      # get_cell_center -> f32 on use
        self.ori = D(0.0)
        self.steps = 0
        if self.task_type == SURVIVAL:
            self.wait = np.zeros(self.walls.shape, np.int32)
            self.food = np.array(t["food_rewards"], np.float64)
            self.revival = np.array(t["food_interval"], np.int32)
            self.life = float(t["initial_life"])

    def place(self, loc, ori):
        self.loc = (F(loc[0]), F(loc[1]))
        self.ori = D(ori)
        cs32 = F(float(self.task["cell_size"]))
        self.grid = (int(F(self.loc[0] / cs32)), int(F(self.loc[1] / cs32)))

    def step(self, turn, walk, visited=None):
        t = self.task
        self.ori, self.loc, self.grid = move(self.walls, float(t["cell_size"]), self.col_dist, self.loc, self.ori, float(turn),
                                             float(walk), self.census, visited)
        self.steps += 1
        if self.task_type == SURVIVAL:
            g = self.grid
            if self.food[g] > 1.0e-2:
                reward = float(self.food[g])
                self.wait[g] = 1
                self.food[g] = 0.0
            else:
                reward = 0.0
            self.life = min(self.life + (reward + float(t["step_reward"])), float(t["max_life"]))
            done = self.life < 0.0 or self.steps > self.max_steps - 1
            self.revival -= self.wait
            again = self.revival < 0
            self.food[again] = np.asarray(t["food_rewards"], np.float64)[again]
            self.revival[again] = np.asarray(t["food_interval"], np.int32)[again]
            self.wait[again] = 0
        else:
            goal = self.grid == (int(t["goal"][0]), int(t["goal"][1]))
            reward = float(t["step_reward"]) + goal * float(t["goal_reward"])
            done = goal or self.steps > self.max_steps - 1
        return reward, bool(done)


def task_from_golden(g):
    return {k[5:]: g[k] for k in g.files if k.startswith("task_")}


# ------------------------------------------------------------------------------------------------ mazes and tasks
def _room(n):
    w = np.ones((n, n), np.int32)
    w[1:-1, 1:-1] = 0
    return w


def maze7():
    """Border, a pillar in the middle, a stub off the border (two inner corners), a filled corner."""
    w = _room(7)
    w[3, 3] = 1
    w[1, 4] = 1
    w[5, 5] = 1
    return w


def maze9():
    """Border, a 2 x 2 block, a corridor that ends dead, a pillar, a filled corner."""
    w = _room(9)
    w[4:6, 4:6] = 1
    w[1:4, 2] = 1
    w[4, 1] = 1
    w[2, 6] = 1
    w[7, 7] = 1
    return w


CELL_SIZES = (2.0, 1.5, 0.75)          # no uniform size: per-task route; 1.5: e / cell is no scaling in float32
COL_DISTS = (0.20, 0.35)
MAX_STEPS = 1000


def tables():
    """{n: [task dict per cell size]}; the fields of TaskConfig. Food on three free cells (SURVIVAL), goal in a free cell."""
    out = {}
    for n, walls, start, goal, food_cells in ((7, maze7(), (1, 1), (5, 1), ((2, 2), (3, 5), (5, 3))),
                                              (9, maze9(), (1, 1), (7, 3), ((1, 1), (6, 2), (3, 7)))):
        food = np.zeros((n, n), np.float64)
        interval = np.zeros((n, n), np.int32)
        for k, c in enumerate(food_cells):
            assert walls[c] == 0 and walls[start] == 0 and walls[goal] == 0
            food[c], interval[c] = 0.25 + 0.125 * k, 2 + k
        out[n] = [dict(start=start, goal=goal, cell_walls=walls.copy(), cell_texts=np.where(walls > 0, 1, 0).astype(np.int32),
                       cell_size=cs, wall_height=3.2, agent_height=1.6, initial_life=1.0, max_life=2.0, step_reward=-0.01,
                       goal_reward=1.0, food_rewards=food.copy(), food_interval=interval.copy()) for cs in CELL_SIZES]
    return out


Case = collections.namedtuple("Case", "n task loc ori actions col_dist kind")
# n: the table (7 or 9), task: its row, loc float32 pair, ori float64, actions ((turn, walk) float32 pairs, one per step),
# kind "exact" / "general"


def first_trace(walls, cell_size, col_dist, loc):
    """What classifies a placement: per neighbouring wall cell (absolute index), the comparison outcomes of the first sub-step of
    a step that does not walk (exp_pos = loc), in the order evaluated."""
    n = walls.shape[0]
    cs32 = F(cell_size)
    c0, c1 = F(F(loc[0]) / cs32), F(F(loc[1]) / cs32)
    out = []
    for i in range(-1, 2):
        for j in range(-1, 2):
            w_i, w_j = i + int(c0), j + int(c1)
            if w_i > -1 and w_i < n and w_j > -1 and w_j < n and walls[w_i, w_j] > 0:
                cen = Census()
                cen.trace = []
                dv = (F(F(c0 - F(np.floor(c0))) - F(i + 0.5)), F(F(c1 - F(np.floor(c1))) - F(j + 0.5)))
                collision_force(dv, cell_size, col_dist, cen)
                out.append(((w_i, w_j), tuple(cen.trace)))
    return tuple(out)


def flipped(ta, tb):
    """The comparisons that two placements' traces decide differently for one and the same wall cell."""
    ta, names = dict(ta), set()
    for cell, b in tb:
        for x, y in zip(ta.get(cell, ()), b):
            if x != y:
                if x[0] == y[0]:
                    names.add(x[0])
                break
    return names


def bisect_flip(walls, cell_size, col_dist, a, b, axis):
    """Two placements that differ in one coordinate and in their trace -> two float32-adjacent placements (1 ulp apart in
    that coordinate) that still differ in their trace."""
    a, b = [F(a[0]), F(a[1])], [F(b[0]), F(b[1])]
    ta = first_trace(walls, cell_size, col_dist, a)
    while np.nextafter(a[axis], b[axis]) != b[axis]:
        m = list(a)
        m[axis] = F((D(a[axis]) + D(b[axis])) / 2)
        if m[axis] == a[axis] or m[axis] == b[axis]:
            break
        if first_trace(walls, cell_size, col_dist, m) == ta:
            a = m
        else:
            b = m
    return tuple(a), tuple(b)


def run_case(tab, case, task_type=ESCAPE, cen=None):
    """-> (per-step (ori, loc, grid, reward, done), visited positions) by the restatement, from a fresh reset with the agent
    placed (steps 0, food as reset leaves it)."""
    ag = Agent(tab[case.n][case.task], task_type, MAX_STEPS, case.col_dist)
    if cen is not None:
        ag.census = cen
    ag.place(case.loc, case.ori)
    visited, out = [], []
    for turn, walk in case.actions:
        r, d = ag.step(float(turn), float(walk), visited)
        out.append((ag.ori, ag.loc, ag.grid, r, d))
    return out, visited


def in_grid(case, visited, tab):
    lim = case.n * float(tab[case.n][case.task]["cell_size"])
    return all(0.0 <= float(p[0]) < lim and 0.0 <= float(p[1]) < lim for p in visited)


_WALK_ONLY = tuple(F(x) for x in (1.0, -1.0, 0.37, 1.5, -1.5))
_TURNS = tuple(F(x) for x in (0.0, 1.0, -1.0, 0.3, -0.7, 1.3, -1.3, float(np.nextafter(F(1), F(2))), float(np.nextafter(F(-1), F(-2)))))
QUOTA = 2            # boundary pairs kept per comparison, table, task and collision distance


Built = collections.namedtuple("Built", "tab exact general expect census flips")
# expect[case]: the restatement's per-step (ori, loc, grid, reward, done) in ESCAPE; census: the branches the exact cases take;
# flips: per comparison, the float32-adjacent placement pairs that straddle it


@functools.lru_cache(maxsize=None)
def build_cases():
    """-> Built. Deterministic (seeded). A candidate placement that breaks a condition on the inputs is dropped HERE, before it is a
    case; `check_conditions` then asserts the conditions on what was kept."""
    tab = tables()
    rs = np.random.RandomState(20240611)
    exact, general, expect = [], [], {}
    flips, census = collections.Counter(), Census()

    def headings(k):
        near = [D(0.0), D(T_PI), D(0.02), D(T_PI - D(0.02)), D(0.031415926), D(T_PI - D(0.031415926))]
        return near[k % len(near)] if k % 3 else D(rs.uniform(0.0, float(T_PI)))

    def exact_actions(k, steps):
        """walk = 0 with any turn (k even), or turn = 0 from heading 0 with the listed walks (k odd)."""
        if k % 2 == 0:
            return headings(k // 2), tuple((_TURNS[(k // 2 + 3 * s) % len(_TURNS)], F(0.0)) for s in range(steps))
        return D(0.0), tuple((F(0.0), _WALK_ONLY[(k // 2 + 2 * s) % len(_WALK_ONLY)]) for s in range(steps))

    def add_exact(n, ti, loc, cd, k):
        """Three steps; a candidate that would leave the grid is dropped here, before it becomes a case."""
        ori, actions = exact_actions(k, 3)
        return keep(Case(n, ti, (F(loc[0]), F(loc[1])), ori, actions, cd, "exact"))

    def keep(c):
        cen = Census()
        out, visited = run_case(tab, c, ESCAPE, cen)
        if in_grid(c, visited, tab):
            exact.append(c)
            expect[c] = out
            census.update(cen)
            return True
        return False

    k = 0
    for n in sorted(tab):
        for ti, task in enumerate(tab[n]):
            walls, cs = task["cell_walls"], float(task["cell_size"])
            lo, hi = 0.55 * cs, (n - 0.55) * cs
            wall_cells = np.argwhere(walls > 0)
            for cd in COL_DISTS:
                # ---- random placements between 0.55 and n - 0.55 cells (free cells and the inner part of border walls)
                for _ in range(36):
                    k += add_exact(n, ti, (rs.uniform(lo, hi), rs.uniform(lo, hi)), cd, k)
                # ---- the equal cases float32 hits exactly: a wall cell's centre, a wall face (|dv| = 0.5), the two diagonals
                #      of a wall cell (dv[0] + dv[1] = 0, dv[1] - dv[0] = 0), an edge's first corner (dist_1 = 0)
                inner = [c for c in wall_cells if 0 < c[0] < n - 1 and 0 < c[1] < n - 1]
                for c in inner[:3]:
                    cx, cy = (c[0] + 0.5) * cs, (c[1] + 0.5) * cs
                    for dx, dy in ((0.0, 0.0), (0.5, 0.25), (-0.5, -0.25), (0.25, 0.5), (0.25, -0.5), (0.5, 0.5), (-0.5, 0.5),
                                   (-0.5, -0.5), (0.5, -0.5), (0.625, 0.625), (-0.625, 0.625), (0.625, -0.625), (-0.625, -0.625),
                                   (0.25, 0.25), (-0.25, 0.25), (0.5625, 0.0), (0.0, -0.5625), (-0.5625, 0.0), (0.0, 0.5625)):
                        k += add_exact(n, ti, (cx + dx * cs, cy + dy * cs), cd, k)
                # the projection onto an edge exactly at its first corner (dist_1 = 0) and at its second (dist_1 = edge_norm)
                cx, cy = (inner[0][0] + 0.5) * cs, (inner[0][1] + 0.5) * cs
                for dx, dy in ((0.5625, -0.5), (0.5, 0.5625), (-0.5625, 0.5), (-0.5, -0.5625),
                               (0.5625, 0.5), (-0.5, 0.5625), (-0.5625, -0.5), (0.5, -0.5625)):
                    k += add_exact(n, ti, (cx + dx * cs, cy + dy * cs), cd, k - k % 2)
                # one or two float32 steps off each face of a pillar, anywhere along it: the nearest point is the agent's own
                # projection and |ori| is below the 1e-6 guard without being 0
                for c in inner[:2]:
                    for axis in (0, 1):
                        for side in (0, 1):
                            for m in range(2):
                                v = F((c[axis] + side) * cs)
                                for _ in range(1 + m % 3):
                                    v = np.nextafter(v, F(np.inf if side else -np.inf))
                                loc = [0.0, 0.0]
                                loc[axis], loc[1 - axis] = v, (c[1 - axis] + rs.uniform(0.02, 0.98)) * cs
                                k += add_exact(n, ti, loc, cd, k - k % 2)
                # inside the corner block of the border: four walls push at once
                for fx, fy in ((n - 0.96, n - 0.96), (n - 0.9, n - 0.95)):
                    k += add_exact(n, ti, (fx * cs, fy * cs), cd, k)
                # ---- both sides of every comparison: pairs of placements, bisected to float32 neighbours
                have = collections.Counter()
                for _ in range(4000):
                    if all(have[c] >= QUOTA for c in COMPARISONS):
                        break
                    axis = int(rs.randint(2))
                    a = [F(rs.uniform(lo, hi)), F(rs.uniform(lo, hi))]
                    b = list(a)
                    b[axis] = F(min(hi, max(lo, float(a[axis]) + rs.uniform(-0.4, 0.4) * cs)))
                    if first_trace(walls, cs, cd, a) == first_trace(walls, cs, cd, b):
                        continue
                    a, b = bisect_flip(walls, cs, cd, a, b, axis)
                    which = flipped(first_trace(walls, cs, cd, a), first_trace(walls, cs, cd, b))
                    if all(have[w] >= QUOTA for w in which):
                        continue
                    if add_exact(n, ti, a, cd, k - k % 2) and add_exact(n, ti, b, cd, k - k % 2):
                        k += 3
                        for w in which:
                            have[w] += 1
                            flips[w] += 1
                assert all(have[c] >= QUOTA for c in COMPARISONS), (n, ti, cd, dict(have))
                # 0.708: on the diagonal off a pillar's corner, where the corner is nearer than eff but the centre is not
                # nearer than 0.707 + eff
                eff = cd / cs
                c = inner[0]
                for s0, s1 in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
                    for shrink in (2.0e-5, 6.0e-5):
                        r = (0.5 + (eff - shrink) / np.sqrt(2.0))
                        k += add_exact(n, ti, ((c[0] + 0.5 + s0 * r) * cs, (c[1] + 0.5 + s1 * r) * cs), cd, k - k % 2)
                # ---- general cases: free cells beside walls and corners, random heading, three steps
                free = [c for c in np.argwhere(walls == 0)
                        if walls[c[0] - 1:c[0] + 2, c[1] - 1:c[1] + 2].sum() > 0]
                got = 0
                while got < 10:
                    c = free[rs.randint(len(free))]
                    loc = (F((c[0] + rs.uniform(0.3, 0.7)) * cs), F((c[1] + rs.uniform(0.3, 0.7)) * cs))
                    acts = tuple((F(rs.uniform(-1.3, 1.3)), F(rs.uniform(-0.6, 1.3))) for _ in range(3))
                    g = Case(n, ti, loc, D(rs.uniform(0.0, float(T_PI))), acts, cd, "general")
                    if general_ok(tab, g):
                        general.append(g)
                        expect[g] = run_case(tab, g)[0]
                        got += 1
    # ---- heading edges that need no placement search: the wrap comparisons at equality, the action clamps at and around +-1
    one_up, one_dn = float(np.nextafter(F(1), F(2))), float(np.nextafter(F(1), F(0)))
    for n in sorted(tab):
        cs = float(tab[n][1]["cell_size"])
        loc = (F(1.5 * cs), F(1.5 * cs))
        for ori, turn in ((T_PI, 0.0), (D(0.0), 0.0), (np.nextafter(T_PI, D(7)), 0.0), (np.nextafter(T_PI, D(0)), 0.0),
                          (D(0.0), -1.0), (T_PI, 1.0), (D(0.0), 1.0), (D(0.0), one_up), (D(0.0), one_dn), (D(0.0), -one_up),
                          (D(0.0), -one_dn), (D(3.0), 1.3), (D(3.0), -1.3)):
            assert keep(Case(n, 1, loc, D(ori), ((F(turn), F(0.0)),) * 3, 0.20, "exact"))
        for walk in (1.0, one_up, one_dn, -1.0, -one_up, -one_dn, 1.5, -1.5, 0.37, float(np.nextafter(F(0), F(-1))), -0.0):
            assert keep(Case(n, 1, loc, D(0.0), ((F(0.0), F(walk)),) * 3, 0.20, "exact"))
    built = Built(tab, tuple(exact), tuple(general), expect, census, flips)
    check_conditions(built)
    return built


def general_ok(tab, case):
    """No inside-a-wall formula, no evaluation of its switch within 1e-4 of |dv| = 0.5 on both axes, no step that ends
    within 1e-4 cells of a cell boundary, no position outside the grid."""
    cen = Census()
    ag = Agent(tab[case.n][case.task], ESCAPE, MAX_STEPS, case.col_dist)
    ag.census = cen
    ag.place(case.loc, case.ori)
    cs = float(tab[case.n][case.task]["cell_size"])
    walls, n = ag.walls, case.n
    visited = []
    for turn, walk in case.actions:
        before = len(visited)
        ag.step(float(turn), float(walk), visited)
        for e in visited[before::2]:                            # the expected positions: where the forces were evaluated
            c0, c1 = float(e[0]) / cs, float(e[1]) / cs
            for i in range(-1, 2):
                for j in range(-1, 2):
                    w_i, w_j = int(c0) + i, int(c1) + j
                    if 0 <= w_i < n and 0 <= w_j < n and walls[w_i, w_j] > 0:
                        d0, d1 = abs(c0 - (w_i + 0.5)), abs(c1 - (w_j + 0.5))
                        if max(d0, d1) < 0.5 + 1.0e-4 and np.hypot(d0, d1) <= 0.708 + case.col_dist / cs + 1.0e-4:
                            return False
        for p in ag.loc:
            f = float(p) / cs
            if abs(f - round(f)) < 1.0e-4:
                return False
    return cen["inside"] == 0 and in_grid(case, visited, tab)


def check_conditions(built):
    """The conditions on the INPUTS, asserted on the host before anything is launched; no case is left out afterwards. (That
    every sub-step of every exact case stays inside the grid is what `keep` admitted it on; its census was taken there.)"""
    for c in built.exact:
        assert c.kind == "exact" and len(c.actions) == 3 and c in built.expect
        assert all(float(w) == 0.0 for _, w in c.actions) or (float(c.ori) == 0.0 and all(float(t) == 0.0 for t, _ in c.actions))
        lim = F(c.n * float(built.tab[c.n][c.task]["cell_size"]))
        assert all(0 <= x < lim for step in built.expect[c] for x in step[1]) and all(0 <= x < lim for x in c.loc)
    missing = [key for key in ALL_KEYS if built.census[key] == 0]
    assert not missing, "census keys the exact cases never take: %s" % missing
    assert built.census[GUARD_EDGE_NORM] == 0            # the edges have length 1: this guard is dead code
    short = [c for c in COMPARISONS if built.flips[c] < QUOTA * len(built.tab) * len(CELL_SIZES) * len(COL_DISTS)]
    assert not short, "comparisons without a float32-adjacent pair on both sides: %s" % short
    assert len(built.general) >= 100 and all(c in built.expect and general_ok(built.tab, c) for c in built.general)


def golden_census(paths):
    """Replays the goldens through the restatement -> (census, largest |difference| of loc / ori / grid over all steps)."""
    cen = Census()
    worst = 0.0
    for path in paths:
        g = np.load(path)
        tt = SURVIVAL if "survival" in path else ESCAPE
        ag = Agent(task_from_golden(g), tt, int(g["max_steps"]))
        ag.census = cen
        for t, a in enumerate(g["actions"]):
            if g["reset_before"][t]:
                ag.reset()
            ag.step(float(a[0]), float(a[1]))
            worst = max(worst, abs(float(ag.loc[0]) - g["loc"][t][0]), abs(float(ag.loc[1]) - g["loc"][t][1]),
                        abs(float(ag.ori) - float(g["ori"][t])), abs(ag.grid[0] - g["grid"][t][0]), abs(ag.grid[1] - g["grid"][t][1]))
    return cen, worst
