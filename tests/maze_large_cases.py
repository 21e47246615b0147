"""Large-maze fixtures shared by tests/test_maze_large.py (CPU) and tests/test_maze_large_gpu.py: synthetic task tables of any
size (the Python sampler takes seconds per task above n = 31), the open field whose long rays cross more translucent cells than
the 3-D renderer keeps, and a numpy restatement of the renderer's ray walk that counts those cells (column_pass, maze.hip; DDA_2D
of the reference's ray_caster_utils.py:11-62 and the overlay span of :195-203)."""
import math

import numpy as np

PI = 3.1415926
MAX_RAY_RECORDS = 127          # the renderer's per-ray bound (mg_maze_view.max_ray_records)


def task_config(**kw):
    from metagym_amd.metamaze import TaskConfig
    return TaskConfig(**kw)


def synthetic_task(n, seed, cell_size=2.0, wall_frac=0.2, food_frac=0.5, crumb_frac=0.15, n_texts=7, interval=(2, 6)):
    """An n x n TaskConfig built with numpy: a border wall, random interior walls, start and goal free; food in [0.1, 0.5] with an
    interval on `food_frac` of the free cells, crumbs <= 1e-2 (nonzero, some with an interval) on `crumb_frac` of them."""
    rs = np.random.RandomState(seed)
    walls = (rs.rand(n, n) < wall_frac).astype(np.int32)
    walls[0, :] = walls[-1, :] = walls[:, 0] = walls[:, -1] = 1
    start = (int(rs.randint(1, n - 1)), int(rs.randint(1, n - 1)))
    goal = (int(rs.randint(1, n - 1)), int(rs.randint(1, n - 1)))
    if goal == start:
        goal = (n - 1 - start[0], start[1]) if n - 1 - start[0] != start[0] else (start[0], n - 1 - start[1])
    walls[start] = walls[goal] = 0
    # a free 3 x 3 around the start: the agent can move at once whatever the draw
    walls[max(1, start[0] - 1):min(n - 1, start[0] + 2), max(1, start[1] - 1):min(n - 1, start[1] + 2)] = 0
    texts = rs.randint(1, n_texts, size=(n, n)).astype(np.int64)
    texts[walls < 1] = 0
    u = rs.rand(n, n)
    food = np.where(u < food_frac, rs.uniform(0.1, 0.5, (n, n)), 0.0)
    crumbs = (u >= food_frac) & (u < food_frac + crumb_frac)
    food = np.where(crumbs, rs.uniform(1.0e-4, 1.0e-2, (n, n)), food) * (1 - walls)
    ivl = rs.randint(interval[0], interval[1] + 1, size=(n, n)).astype(np.int32)
    food_interval = np.where((food > 1.0e-2) | (crumbs & (rs.rand(n, n) < 0.3)), ivl, 0).astype(np.int32) * (1 - walls)
    return task_config(start=start, goal=goal, cell_walls=walls, cell_texts=texts, cell_size=float(cell_size),
                       wall_height=1.6 * cell_size, agent_height=0.8 * cell_size, initial_life=1.0, max_life=2.0,
                       step_reward=-0.01, goal_reward=1.0, food_rewards=food, food_interval=food_interval.astype(np.int32))


def open_field_task(n, cell_size, near_food=0.02, far_food=1.0, split=129, n_texts=7):
    """The record-bound probe: an open n x n field (border wall only), food on every free cell, the agent in corner cell (1, 1)
    facing +x (discrete heading 0), so the columns near 45 degrees cross the field diagonally. Cells with i + j < split hold
    `near_food`, the others `far_food`: the overlay of a translucent cell blends toward green with strength food * 0.5 + 0.1 and
    truncates to a fixed point after a few dozen blends, so only records PAST the first ~127 with ANOTHER strength can change a
    pixel — a field of one food value would hide dropped records."""
    walls = np.zeros((n, n), np.int32)
    walls[0, :] = walls[-1, :] = walls[:, 0] = walls[:, -1] = 1
    texts = (1 + (np.arange(n * n).reshape(n, n) % (n_texts - 1))).astype(np.int64)
    texts[walls < 1] = 0
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    food = np.where(ii + jj < split, near_food, far_food) * (1 - walls)
    return task_config(start=(1, 1), goal=(n - 2, 1), cell_walls=walls, cell_texts=texts, cell_size=float(cell_size),
                       wall_height=3.2, agent_height=1.6, initial_life=1.0, max_life=2.0, step_reward=-0.01, goal_reward=1.0,
                       food_rewards=food.astype(np.float64), food_interval=np.where(food > 0, 100, 0).astype(np.int32))


def column_tables(H, fov=0.6 * PI, l_focal=0.20):
    """mg_maze_view_tables (ray_caster_utils.py:82-90): cos_hp, sin_hp per column, tan_hp accumulated like the reference loop."""
    tan_half = float(np.tan(fov / 2))
    pixel_factor = (2.0 * tan_half * l_focal / H) / l_focal
    tan_hp = (-0.5 - H / 2.0) * pixel_factor
    cc, ss = np.zeros(H), np.zeros(H)
    for d in range(H):
        tan_hp += pixel_factor
        chp = math.sqrt(1.0 / (1.0 + tan_hp * tan_hp))
        cc[d], ss[d] = chp, tan_hp * chp
    return cc, ss, tan_half


def _to_int_clamped(x, lo, hi):
    if not (x > lo - 1.0):
        return lo
    if x >= hi + 1.0:
        return hi + 1
    return int(x)


def ray_records(task, res, ori_idx=0, max_vision=12.0, fov=0.6 * PI, l_focal=0.20):
    """Per screen column of a discrete-3D agent standing on its start cell with the task's food as the translucent map: (cells
    crossed with food > 1e-2, overlay records with a non-empty span e2 > s2, whether the ray hits a wall within max_vision — the
    overlay is drawn only then, the food values of the recorded cells in ray order — their blend strengths). Restates
    column_pass / add_record (maze.hip) without the record bound."""
    H, V = int(res[0]), int(res[1])
    cc, ss, tan_half = column_tables(H, fov, l_focal)
    walls = np.asarray(task.cell_walls)
    transp = np.asarray(task.food_rewards, np.float64)
    n, cs = walls.shape[0], float(task.cell_size)
    half_h = tan_half * l_focal
    half_v, pixel_size = half_h * V / H, 2.0 * half_h / H
    ori = np.asarray([0.0, 0.5, 1.0, 1.5], dtype="float32") * PI
    s_ori, c_ori = float(np.sin(ori).astype(np.float32)[ori_idx]), float(np.cos(ori).astype(np.float32)[ori_idx])
    px0, px1 = task.start[0] * cs + 0.5 * cs, task.start[1] * cs + 0.5 * cs
    vh, ceil_h = float(task.agent_height), float(task.wall_height)
    out = []
    for col in range(H):
        chp, shp = cc[col], ss[col]
        s = float(np.float32(shp * c_ori + chp * s_ori))
        c = float(np.float32(chp * c_ori - shp * s_ori))
        cos_hp = float(np.float32(chp))
        i0, j0 = int(px0 / cs), int(px1 / cs)
        cz, sz = abs(c) < 1.0e-6, abs(s) < 1.0e-6
        delta_x = 1.0e+6 if cz else abs(cs / c)
        delta_y = 1.0e+6 if sz else abs(cs / s)
        d_x = ((i0 + 1) * cs - px0) if c > 0 else (i0 * cs - px0)
        d_y = ((j0 + 1) * cs - px1) if s > 0 else (j0 * cs - px1)
        side_x = 1.0e+6 if cz else d_x / c
        side_y = 1.0e+6 if sz else d_y / s
        di, dj = (1 if c > 0 else -1), (1 if s > 0 else -1)
        hi, hj, hit_dist = i0, j0, 0.0
        crossed, recs = 0, []

        def record(dist):
            r2 = dist * cos_hp / l_focal
            tv, bv = (ceil_h - vh) / r2, vh / r2
            s2 = max(0, _to_int_clamped((half_v - tv) / pixel_size, 0, V))
            e2 = min(V, _to_int_clamped((half_v + bv) / pixel_size, -1, V - 1))
            return e2 > s2

        if 0 <= hi < n and 0 <= hj < n and transp[hi, hj] > 0.01:
            crossed += 1
            if record(min(side_x, side_y)):
                recs.append(float(transp[hi, hj]))
        while hit_dist < max_vision:
            xs = side_x < side_y
            if xs:
                hi += di
                side_y -= side_x
                hit_dist += side_x
            else:
                hj += dj
                side_x -= side_y
                hit_dist += side_y
            if hi < 0 or hi >= n:
                if hj < 0 or hj >= n:
                    hit_dist = 1.0e+6
                    break
            elif 0 <= hj < n:
                if transp[hi, hj] > 0.01:
                    crossed += 1
                    if record(hit_dist):
                        recs.append(float(transp[hi, hj]))
                if walls[hi, hj] > 0:
                    break
            if xs:
                side_x = delta_x
            else:
                side_y = delta_y
        out.append((crossed, len(recs), hit_dist <= max_vision, recs))
    return out


def documented_record_bound(n, cell_size, max_vision=12.0):
    """min(2n+1, max_ray_records) with the env's max_ray_records = 2 * int(max_vision / cell_size) + 5 (include/metagym_hip.h)."""
    return min(2 * n + 1, 2 * int(max_vision / cell_size) + 5)


def dropped_record_columns(task, res, bound=MAX_RAY_RECORDS):
    """Columns where a record bound of `bound` changes what is drawn: the ray hits a wall within sight (else no overlay at all),
    records more than `bound` translucent cells, and some record past the bound blends with another strength than the last kept
    one. (Blending is a truncating fixed-point iteration: a run of records of ONE strength settles a pixel after a few dozen, so
    dropping more of the same strength changes nothing — only a different strength past the bound does.)"""
    return [k for k, (_, nrec, hit, vals) in enumerate(ray_records(task, res))
            if hit and nrec > bound and any(v != vals[bound - 1] for v in vals[bound:])]
