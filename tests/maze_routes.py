"""Launch routes of the maze3d renderer (mg_maze3d_step, metagym_amd/csrc/maze.hip) and the comparison body the route tests
share: tests/test_maze3d_routes_gpu.py runs it in the pytest process (the default library's routes) and
tests/maze_route_child.py runs it in a fresh child process per process-wide knob (MG_MAZE3D_U8_PACKED, MG_MAZE3D_NO_SMALL,
MG_MAZE3D_WAVES, MG_MAZE3D_GENERIC are read once per process).

maze3d_route() RESTATES the launch choice of mg_maze3d_step. When that rule changes in maze.hip, change it here too (the C++ side
carries the same note); test_maze3d_route_map_covers_every_route then says whether the case lists still reach every route."""
import math
import os

import numpy as np

KNOBS = ("MG_MAZE3D_U8_PACKED", "MG_MAZE3D_NO_SMALL", "MG_MAZE3D_WAVES", "MG_MAZE3D_GENERIC")
PI = 3.1415926
SLAB, MZ_WAVES, WAVE = 32, 4, 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _parse_waves(value):
    """MG_MAZE3D_WAVES="<waves>[,<slab>]" as mg_maze3d_step reads it (sscanf "%d,%d"): (waves, slab) or None."""
    if value is None:
        return None
    parts = value.split(",")
    try:
        w = int(parts[0])
    except ValueError:
        return None
    if w not in (1, 2, 4):
        return None
    sl = 0
    if len(parts) > 1:
        try:
            sl = int(parts[1])
        except ValueError:
            sl = 0
    return w, (sl if sl in (32, 64) else SLAB)


# sizeof of the kernel's LDS structs (maze.hip): EnvShared (Agent: 4 int + 2 double + 2 float, then reward, done, pos[2], s_ori,
# c_ori) rounded up to 16, RowRec (3 double + 2 int, 16-aligned), ColRecLds (static_assert'ed 64)
ENV_SHARED_LDS, ROW_REC, COL_REC_LDS = 96, 32, 64
LDS_LIMIT = 160 * 1024


def maze3d_route(n, res, cell_sizes, text_size=1.0, tex_size=64, obs_dtype="int32", knobs=None, max_vision=12.0,
                 fov=0.6 * PI):
    """The kernel instantiation and launch geometry mg_maze3d_step picks for a batch of n x n mazes whose tasks have the cell
    sizes `cell_sizes`, rendered at res = (res_h, res_v) by the Python env (which passes uniform_cell_size = the one cell size of
    the table, or 0 when they differ). `knobs`: the process environment's MG_MAZE3D_* variables (name -> value).
    Also the per-ray record bound `t_max` (min(2n+1, the env's max_ray_records); above 127 the launch is refused) and the
    dynamic LDS bytes `lds` the launch asks for (above LDS_LIMIT it is refused with MG_ERR_BAD_SIZE, naming this number)."""
    knobs = knobs or {}
    H, V = int(res[0]), int(res[1])
    px = H * V
    n_waves = 1 if px <= 64 * 64 else (2 if px < 128 * 128 else MZ_WAVES)
    slab = SLAB
    ov = _parse_waves(knobs.get("MG_MAZE3D_WAVES"))
    if ov:
        n_waves, slab = ov
    rec = 1 if (V < 4096 and n * n <= 256) else 2
    small = n_waves == 1 and "MG_MAZE3D_NO_SMALL" not in knobs
    sizes = set(float(c) for c in cell_sizes)
    ucs = sizes.pop() if len(sizes) == 1 else 0.0
    stock = False
    if ucs > 0.0 and "MG_MAZE3D_GENERIC" not in knobs:
        ttc = text_size / ucs
        eff_max = max_vision * math.sqrt(1.0 + math.tan(fov / 2) ** 2) * 1.0001
        stock = (math.frexp(ucs)[0] == 0.5 and math.frexp(ttc)[0] == 0.5 and math.frexp(text_size)[0] == 0.5 and
                 (tex_size & (tex_size - 1)) == 0 and 1.0 / ttc >= 1.0 and
                 (eff_max + ucs * n) * (tex_size / text_size) < 1073741824.0)
    if obs_dtype == "uint8":
        u8 = "packed" if ("MG_MAZE3D_U8_PACKED" in knobs and V % 4 == 0) else "bytes"
    else:
        u8 = "none"
    # the kernel's column deal (maze3d_step_kernel, phase 2): columns per wave and waves left without a column
    eff_slab = min(slab, (H + n_waves - 1) // n_waves)
    col_step = n_waves if n_waves >= 4 else 1
    idle = 0
    for gbase in range(0, H, n_waves * eff_slab):
        for w in range(n_waves):
            cbase = gbase + w * eff_slab if col_step == 1 else gbase + w
            ncols = min(eff_slab, H - cbase) if col_step == 1 else min(eff_slab, (H - cbase + n_waves - 1) // n_waves)
            idle += ncols <= 0
    t_max = min(2 * n + 1, 2 * int(max_vision / min(float(c) for c in cell_sizes)) + 5)
    lds = (ENV_SHARED_LDS + 8 * n * n + 4 * rec * slab * t_max * n_waves + 2 * ((n * n + 15) & ~15) +
           ROW_REC * ((V + 63) & ~63) + 32 + (COL_REC_LDS * slab if small else 0))
    return dict(waves=n_waves, slab=slab, rec=rec, stock=stock, small=small, u8=u8, eff_slab=eff_slab,
                chunks=(V + 63) // 64, idle_wave_groups=idle, t_max=t_max, lds=lds)


def route_key(r):
    """The instantiation a route runs: maze3d_step_kernel<REC, STOCK, SMALL, U8> at 1, 2 or 4 waves per env."""
    return (r["rec"], "stock" if r["stock"] else "general", r["u8"] != "none", r["waves"])


def default_routes():
    """Every route the default library (no knobs) can reach: REC {1, 2} x {general, stock} x {int32, uint8} x {1, 2, 4 waves}.
    (SMALL is implied by one wave; the byte / packed uint8 store is a knob.)"""
    return {(rec, kind, u8, w) for rec in (1, 2) for kind in ("general", "stock") for u8 in (False, True) for w in (1, 2, 4)}


# ---- cases ------------------------------------------------------------------------------------------------------------------
# A case is a JSON-able dict: the child process receives it on its command line.
# cells: one cell size per task (3 - 6 tasks); [2.0] is the stock configuration, 1.5 / 0.75 and tables mixing 2.0 with 1.0
# (uniform_cell_size = 0) run the general kernels. n = 17 gives REC = 2 (17 * 17 > 256 cells). Shapes: ragged last 64-row chunks
# (V = 40, 90, 100, 150), several column groups per wave (H > slab * waves), V % 4 != 0 for uint8.

def _case(name, n, res, cells, dtype="int32", ident="discrete", task_type="SURVIVAL", envs=24, steps=8, seed=0):
    return dict(name=name, n=n, res=list(res), cells=list(cells), dtype=dtype, ident=ident, task_type=task_type, envs=envs,
                steps=steps, seed=seed, max_steps=4)


MIXED = [2.0, 1.0, 2.0, 1.0]

DEFAULT_CASES = [
    # REC 1
    _case("r1_general_i32_w1", 15, (40, 100), [1.5] * 4, seed=11),
    _case("r1_general_i32_w2", 9, (72, 150), MIXED, task_type="ESCAPE", seed=12),
    _case("r1_general_i32_w4", 15, (136, 150), [0.75] * 3, ident="continuous", envs=16, seed=13),
    _case("r1_general_u8_w1", 9, (24, 30), [2.0, 1.0, 1.0], dtype="uint8", seed=14),
    _case("r1_general_u8_w2", 15, (84, 90), [1.5] * 4, dtype="uint8", task_type="ESCAPE", seed=15),
    _case("r1_general_u8_w4", 9, (130, 150), [0.75] * 5, dtype="uint8", envs=16, seed=16),
    _case("r1_stock_i32_w1", 9, (48, 40), [2.0] * 4, ident="continuous", task_type="ESCAPE", seed=17),
    _case("r1_stock_i32_w2", 15, (100, 100), [2.0] * 3, seed=18),
    _case("r1_stock_i32_w4", 9, (256, 96), [2.0] * 6, envs=12, seed=19),
    _case("r1_stock_u8_w1", 9, (40, 100), [2.0] * 4, dtype="uint8", seed=20),
    _case("r1_stock_u8_w2", 9, (72, 150), [2.0] * 3, dtype="uint8", task_type="ESCAPE", seed=21),
    _case("r1_stock_u8_w4", 15, (136, 150), [2.0] * 4, dtype="uint8", ident="continuous", envs=16, seed=22),
    # REC 2
    _case("r2_general_i32_w1", 17, (60, 60), [0.75] * 3, seed=31),
    _case("r2_general_i32_w2", 17, (100, 100), MIXED, seed=32),
    _case("r2_general_i32_w4", 17, (128, 128), [1.5] * 3, task_type="ESCAPE", envs=16, seed=33),
    _case("r2_general_u8_w1", 17, (33, 7), [1.5] * 4, dtype="uint8", seed=34),
    _case("r2_general_u8_w2", 17, (72, 150), [0.75] * 3, dtype="uint8", ident="continuous", seed=35),
    _case("r2_general_u8_w4", 17, (136, 150), MIXED, dtype="uint8", envs=16, seed=36),
    _case("r2_stock_i32_w1", 17, (64, 64), [2.0] * 3, ident="continuous", seed=37),
    _case("r2_stock_i32_w2", 17, (84, 84), [2.0] * 4, task_type="ESCAPE", seed=38),
    _case("r2_stock_i32_w4", 17, (136, 150), [2.0] * 3, envs=16, seed=39),
    _case("r2_stock_u8_w1", 17, (24, 30), [2.0] * 3, dtype="uint8", seed=40),
    _case("r2_stock_u8_w2", 17, (96, 90), [2.0] * 5, dtype="uint8", seed=41),
    _case("r2_stock_u8_w4", 17, (130, 150), [2.0] * 3, dtype="uint8", task_type="ESCAPE", envs=16, seed=42),
]

# one child process per knob setting: (test id, knob, value, cases)
KNOB_CASES = [
    ("u8_packed", "MG_MAZE3D_U8_PACKED", "1", [
        # the shapes of test_maze_gpu.py::test_maze3d_uint8_byte_store_shapes_equal_clamped_int32, here against the oracle with the packed store switched on
        _case("packed_40x100_stock", 9, (40, 100), [2.0] * 3, dtype="uint8", seed=51),
        _case("packed_24x30_general", 9, (24, 30), [1.5] * 3, dtype="uint8", seed=52),       # V % 4 != 0: byte stores
        _case("packed_64x64_general", 9, (64, 64), MIXED, dtype="uint8", seed=53),
        _case("packed_64x64_stock", 9, (64, 64), [2.0] * 3, dtype="uint8", task_type="ESCAPE", seed=54),
        _case("packed_20x256_stock", 9, (20, 256), [2.0] * 3, dtype="uint8", seed=55),
        _case("packed_33x7_stock_cont", 9, (33, 7), [2.0] * 3, dtype="uint8", ident="continuous", seed=56),
        _case("packed_32x132_general_cont", 9, (32, 132), [0.75] * 3, dtype="uint8", ident="continuous", seed=57),
        _case("packed_84x84_general", 15, (84, 84), [1.5] * 4, dtype="uint8", seed=58),
        _case("packed_136x152_stock_rec2", 17, (136, 152), [2.0] * 3, dtype="uint8", envs=12, seed=59),
        _case("packed_128x128_general", 9, (128, 128), [1.5] * 3, dtype="uint8", envs=12, seed=60),
        _case("packed_130x150_stock", 9, (130, 150), [2.0] * 3, dtype="uint8", envs=12, seed=61),   # V % 4 != 0, four waves
    ]),
    ("no_small", "MG_MAZE3D_NO_SMALL", "1", [
        _case("nosmall_64x64_stock", 9, (64, 64), [2.0] * 4, seed=71),
        _case("nosmall_72x40_general", 15, (72, 40), [1.5] * 3, seed=72),
        _case("nosmall_60x60_stock_u8", 9, (60, 60), [2.0] * 3, dtype="uint8", seed=73),
        _case("nosmall_24x24_general_cont", 17, (24, 24), MIXED, ident="continuous", seed=74),
    ]),
    ("waves_1", "MG_MAZE3D_WAVES", "1", [
        _case("w1_128x128_stock", 9, (128, 128), [2.0] * 3, envs=12, seed=81),
        _case("w1_256x96_general", 15, (256, 96), [0.75] * 3, envs=12, seed=82),
        _case("w1_128x128_stock_u8_rec2", 17, (128, 128), [2.0] * 3, dtype="uint8", envs=12, seed=83),
    ]),
    ("waves_2_64", "MG_MAZE3D_WAVES", "2,64", [
        _case("w2s64_84x84_stock", 9, (84, 84), [2.0] * 3, seed=91),
        _case("w2s64_84x84_general_rec2", 17, (84, 84), [1.5] * 3, seed=92),
    ]),
    ("waves_4", "MG_MAZE3D_WAVES", "4", [
        _case("w4_32x32_stock", 9, (32, 32), [2.0] * 4, seed=101),
        _case("w4_32x32_general_u8", 9, (32, 32), MIXED, dtype="uint8", seed=102),
        _case("w4_3x64_stock", 9, (3, 64), [2.0] * 3, seed=103),
        _case("w4_3x64_general_cont", 9, (3, 64), [1.5] * 3, ident="continuous", seed=104),
    ]),
    ("waves_4_64", "MG_MAZE3D_WAVES", "4,64", [
        _case("w4s64_136x150_stock", 9, (136, 150), [2.0] * 3, envs=12, seed=111),
        _case("w4s64_136x150_general_rec2", 17, (136, 150), [0.75] * 3, envs=12, seed=112),
    ]),
    ("generic", "MG_MAZE3D_GENERIC", "1", [
        _case("generic_64x64_i32", 9, (64, 64), [2.0] * 4, seed=121),
        _case("generic_64x64_u8", 9, (64, 64), [2.0] * 4, dtype="uint8", seed=122),
        _case("generic_256x256_i32", 9, (256, 256), [2.0] * 3, envs=12, steps=6, seed=123),
        _case("generic_256x256_u8", 9, (256, 256), [2.0] * 3, dtype="uint8", envs=12, steps=6, seed=124),
    ]),
]


def case_route(case, knobs=None):
    return maze3d_route(case["n"], case["res"], case["cells"], obs_dtype=case["dtype"], knobs=knobs)


def required_knob_routes():
    """What each knob child must reach (section by section of the knob list): (test id, description, predicate on a route and
    its case)."""
    return [
        ("u8_packed", "packed store, SMALL", lambda r, c: r["u8"] == "packed" and r["small"]),
        ("u8_packed", "packed store, 2 waves", lambda r, c: r["u8"] == "packed" and r["waves"] == 2),
        ("u8_packed", "packed store, 4 waves", lambda r, c: r["u8"] == "packed" and r["waves"] == 4),
        ("u8_packed", "packed store, stock table", lambda r, c: r["u8"] == "packed" and r["stock"]),
        ("u8_packed", "packed store, general table", lambda r, c: r["u8"] == "packed" and not r["stock"]),
        ("u8_packed", "packed store, continuous", lambda r, c: r["u8"] == "packed" and c["ident"] == "continuous"),
        ("u8_packed", "V % 4 != 0 falls back to byte stores", lambda r, c: r["u8"] == "bytes"),
        ("no_small", "one wave, general instantiation", lambda r, c: r["waves"] == 1 and not r["small"]),
        ("no_small", "one wave, general instantiation, ragged chunk", lambda r, c: not r["small"] and c["res"][1] % 64 != 0),
        ("waves_1", "SMALL, several chunks per column, >= 128 columns",
         lambda r, c: r["small"] and r["chunks"] > 1 and c["res"][0] >= 128),
        ("waves_2_64", "2 waves, 64-column slab", lambda r, c: r["waves"] == 2 and r["slab"] == 64),
        ("waves_4", "4 waves, 8 round-robin columns each", lambda r, c: r["waves"] == 4 and r["eff_slab"] == 8),
        ("waves_4", "4 waves, a wave without a column", lambda r, c: r["waves"] == 4 and r["idle_wave_groups"] > 0),
        ("waves_4_64", "4 waves, 64-column slab", lambda r, c: r["waves"] == 4 and r["slab"] == 64 and r["eff_slab"] > 32),
        ("generic", "general kernel on a stock table, int32", lambda r, c: not r["stock"] and c["cells"] == [2.0] * len(c["cells"]) and r["u8"] == "none"),
        ("generic", "general kernel on a stock table, uint8", lambda r, c: not r["stock"] and c["cells"] == [2.0] * len(c["cells"]) and r["u8"] != "none"),
        ("generic", "general kernel on a stock table, 4 waves", lambda r, c: not r["stock"] and r["waves"] == 4),
    ]


# (n, res, cell sizes, dtype) of the 3-D renderer cases in tests/test_maze_gpu.py, for the coverage table
EXISTING_MAZE_GPU_PARAMS = [
    (9, (64, 64), [2.0], "int32"), (9, (40, 24), [2.0], "int32"),                          # batch_matches_oracle
    (9, (72, 40), [2.0], "int32"), (9, (128, 32), [2.0], "int32"), (9, (24, 24), [2.0], "int32"),
    (9, (64, 48), [2.0], "int32"), (9, (48, 20), [2.0], "int32"), (9, (60, 60), [2.0], "int32"),   # small_frame_renderer
    (9, (32, 24), [2.0], "int32"),                                                          # ragged_batch
    (9, (32, 32), [2.0], "int32"), (9, (256, 256), [2.0], "int32"),                        # full_size_properties, c3
    (15, (64, 48), [2.0], "int32"), (21, (32, 32), [2.0], "int32"), (15, (32, 32), [0.75], "int32"),
    (15, (136, 150), [1.5], "int32"), (9, (70, 200), [2.0], "int32"),                      # larger_mazes
    (9, (32, 32), [2.0, 1.5], "int32"),                                                     # wrong_uniform_cell_size (mixed)
    (9, (48, 64), [2.0], "uint8"),                                                          # uint8 clamped (GPU vs GPU)
    (9, (40, 100), [2.0], "uint8"), (9, (24, 30), [2.0], "uint8"), (9, (64, 64), [2.0], "uint8"),
    (9, (32, 132), [2.0], "uint8"), (9, (20, 256), [2.0], "uint8"), (9, (33, 7), [2.0], "uint8"),   # uint8 byte-store shapes
]


# ---- the comparison body ------------------------------------------------------------------------------------------------------

def use_reference_textures():
    """Render with the reference's textures (tests/golden/maze_textures.npz), in every process alike."""
    from metagym_amd.metamaze import MAZE_TASK_MANAGER
    tex = np.load(os.path.join(GOLDEN, "maze_textures.npz"))
    MAZE_TASK_MANAGER.set_textures(tex["grounds"], tex["ceil"])


def make_tasks(case):
    from metagym_amd.metamaze import MazeTaskSampler
    # dense food (SURVIVAL: translucent cells on most rays), short corridors with loops so rays travel far
    return [MazeTaskSampler(n=case["n"], allow_loops=True, crowd_ratio=0.25, cell_size=cs, wall_height=1.6 * cs,
                            agent_height=0.8 * cs, step_reward=-0.01, goal_reward=1.0, food_density=0.3, food_interval=3,
                            seed=case["seed"] * 10 + k) for k, cs in enumerate(case["cells"])]


def run_case(case, device="cuda:0"):
    """Step a batch of case["envs"] envs case["steps"] times with masked resets of finished envs, and compare reward, done, the
    per-env state and EVERY pixel of every frame (the reset frame, every step's frame, every re-rendered reset frame) with
    oracle/maze_oracle.c. int32 frames bit-exact; uint8 frames == min(oracle frame, 255); continuous envs: pose within 1e-5 and
    every pixel exact wherever the pose is bit-equal. Transitions raise at once; pixel mismatches are counted and returned."""
    import torch
    import metagym_amd
    from metagym_amd.metamaze import MAZE_TASK_MANAGER
    from oracle import maze as mo

    use_reference_textures()
    tasks = make_tasks(case)
    N, res, steps, max_steps = case["envs"], tuple(case["res"]), case["steps"], case["max_steps"]
    cont = case["ident"] == "continuous"
    u8 = case["dtype"] == "uint8"
    tt_name = case["task_type"]
    tt = mo.TASK_TYPES[tt_name]
    ident = "meta-maze-continuous-3D-v0" if cont else "meta-maze-discrete-3D-v0"
    env = metagym_amd.make(ident, num_envs=N, device=device, max_steps=max_steps, resolution=res, task_type=tt_name,
                           obs_dtype=torch.uint8 if u8 else torch.int32)
    env.set_task(tasks)
    expect_ucs = float(case["cells"][0]) if len(set(case["cells"])) == 1 else 0.0
    assert env._uniform_cell_size == expect_ucs, (env._uniform_cell_size, expect_ucs)
    ids = env.task_id.cpu().numpy()
    otasks = [mo.Task(**t._asdict()) for t in tasks]
    states = [mo.State(otasks[i]) for i in ids]
    for s, i in zip(states, ids):
        mo.reset(otasks[i], tt, s)
    view = mo.View(MAZE_TASK_MANAGER.grounds.astype(np.uint8), MAZE_TASK_MANAGER.ceil, res[0], res[1])
    out = dict(case=case["name"], route=case_route(case, {k: os.environ[k] for k in KNOBS if k in os.environ}),
               frames=0, values=0, bad=0, first_bad=None, pose_not_bit_equal=0, resets=0, max_ref=0)

    def compare(ob, envs, label):
        for e in envs:
            s = states[e]
            ref = mo.observe_3d(otasks[ids[e]], tt, view, s, int(cont))
            out["max_ref"] = max(out["max_ref"], int(ref.max()))
            want = np.minimum(ref, 255) if u8 else ref
            got = ob[e].astype(np.int32)
            assert got.shape == want.shape, (got.shape, want.shape)
            d = int((got != want).sum())
            if cont:
                loc, ori = env.loc[:, e].cpu().numpy(), float(env.ori[e])
                assert np.allclose(loc, np.asarray(s.c.loc[:]), rtol=1e-5, atol=1e-5), (label, e, loc, s.c.loc[:])
                assert abs(ori - s.c.ori) <= 1e-5 * max(1.0, abs(s.c.ori)), (label, e, ori, s.c.ori)
                if not (np.array_equal(loc, np.asarray(s.c.loc[:], np.float32)) and ori == s.c.ori):
                    out["pose_not_bit_equal"] += 1
                    continue
            out["frames"] += 1
            out["values"] += want.size
            if d:
                out["bad"] += d
                if out["first_bad"] is None:
                    rows = np.nonzero((got != want).any(axis=(0, 2)))[0]
                    cols = np.nonzero((got != want).any(axis=(1, 2)))[0]
                    out["first_bad"] = dict(at=label, env=int(e), values=d, max_abs=int(np.abs(got - want).max()),
                                            columns=[int(cols.min()), int(cols.max())], rows=[int(rows.min()), int(rows.max())])

    def check_state(label):
        grid, stp = env.grid.cpu().numpy(), env.steps.cpu().numpy()
        life = env.life.cpu().numpy()
        oidx = env.ori_idx.cpu().numpy()
        food = [x.cpu().numpy() for x in (env.cur_food, env.wait_refresh, env.revival)] if tt_name == "SURVIVAL" else None
        for e in range(N):
            s = states[e]
            assert (grid[0, e], grid[1, e], stp[e]) == (s.c.grid[0], s.c.grid[1], s.c.steps), (label, e)
            if tt_name == "SURVIVAL":
                assert life[e] == s.c.life, (label, e)
            if not cont:
                assert oidx[e] == s.c.ori_idx, (label, e)
            if food is not None:
                assert (np.array_equal(food[0][e], s.cur_food) and np.array_equal(food[1][e], s.wait) and
                        np.array_equal(food[2][e], s.revival)), (label, e)

    ob = env.reset().cpu().numpy()
    assert ob.dtype == (np.uint8 if u8 else np.int32) and ob.shape == (N, res[0], res[1], 3)
    compare(ob, range(N), "reset")
    rs = np.random.RandomState(case["seed"])
    for t in range(steps):
        if cont:
            a = np.stack([rs.uniform(-1.2, 1.2, N), rs.uniform(-0.5, 1.2, N)], 1).astype(np.float32)
        else:
            a = rs.choice(4, size=N, p=[0.2, 0.2, 0.1, 0.5]).astype(np.int32)
        obs, rew, done, info = env.step(torch.as_tensor(a))
        ob, r64, d = obs.cpu().numpy(), env.reward64.cpu().numpy(), done.cpu().numpy()
        for e in range(N):
            if cont:
                r, dd = mo.step_cont3d(otasks[ids[e]], tt, max_steps, states[e], float(a[e, 0]), float(a[e, 1]))
            else:
                r, dd = mo.step_disc3d(otasks[ids[e]], tt, max_steps, states[e], int(a[e]))
            assert r == r64[e] and dd == bool(d[e]), ("step", t, e, r, r64[e], dd, d[e])
        check_state("step %d" % t)
        compare(ob, range(N), "step %d" % t)
        if d.any():
            ob2 = env.reset(mask=done).cpu().numpy()
            ended = np.nonzero(d)[0]
            for e in ended:
                mo.reset(otasks[ids[e]], tt, states[e])
            out["resets"] += len(ended)
            kept = ~d.astype(bool)
            assert np.array_equal(ob2[kept], ob[kept]), "a masked reset re-rendered an env it did not reset differently"
            check_state("reset after step %d" % t)
            compare(ob2, ended, "reset after step %d" % t)
    return out
