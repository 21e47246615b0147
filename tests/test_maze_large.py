"""CPU side of the large-maze limits (tests/test_maze_large_gpu.py runs the kernels): the int16 food lists the env builds and
the library's refusal of lists it cannot index, the refusal of a per-ray record bound above 127, and the numpy restatement of
the ray walk those tests rely on. No GPU: the library's checks run on the host before anything is launched."""
import ctypes as C

import numpy as np
import torch

import maze_large_cases as L
import maze_routes as mr


def _lists(n, seed=0, T=2, by_slot=True):
    from metagym_amd.metamaze.maze_env import food_lists
    tasks = [L.synthetic_task(n, seed + k) for k in range(T)]
    food = torch.from_numpy(np.stack([np.asarray(t.food_rewards, np.float64).ravel() for t in tasks]))
    ivl = torch.from_numpy(np.stack([np.asarray(t.food_interval, np.int32).ravel() for t in tasks]))
    return tasks, food, ivl, food_lists(food, ivl, by_slot)


def test_int16_cell_index_wraps_past_32767():
    """Why the bound exists: the list builder's int16 cast sends cell 32 768 (n = 183 has 33 489 cells) to -32 768."""
    idx = torch.arange(183 * 183)
    wrapped = idx.to(torch.int16)
    first = int(torch.nonzero(wrapped.long() != idx)[0])
    assert first == 32768 and int(wrapped[first]) == -32768
    assert torch.equal(torch.arange(181 * 181).to(torch.int16).long(), torch.arange(181 * 181))


def test_food_lists_round_trip_at_n_181():
    """n = 181 (32 761 cells, the largest odd n under the bound): every listed index is its cell, ascending; cell_slot inverts the
    list; slot_food / slot_interval hold the listed cells' values; unlisted cells keep -1 / -2."""
    n = 181
    tasks, food, ivl, lists = _lists(n)
    assert lists is not None
    can = (ivl > 0) | (food > 1.0e-2)
    assert int(torch.nonzero(can)[:, 1].max()) > 32000                  # food near the top of the int16 range
    cells, slot = lists["food_cells"].long(), lists["cell_slot"].long()
    assert lists["food_cells"].dtype == torch.int16 and lists["cell_slot"].dtype == torch.int16
    for t in range(len(tasks)):
        k = int(lists["n_food"][t])
        want = torch.nonzero(can[t]).ravel()
        assert k == len(want) and torch.equal(cells[t, :k], want)
        assert torch.equal(slot[t, want], torch.arange(k))
        rest = torch.ones(n * n, dtype=torch.bool)
        rest[want] = False
        assert torch.equal(slot[t, rest], torch.where(food[t, rest] != 0.0, -2, -1))
        assert torch.equal(lists["slot_food"][:k, t], food[t, want])
        assert torch.equal(lists["slot_interval"][:k, t], ivl[t, want])


def test_food_lists_refused_past_the_int16_bound():
    """n = 183 and 255: no list (the env then passes NULL and keeps the SURVIVAL arrays by cell) — slot layout or not."""
    for n in (183, 255):
        for by_slot in (True, False):
            tasks, food, ivl, lists = _lists(n, by_slot=by_slot)
            assert lists is None
            assert int(torch.nonzero((ivl > 0) | (food > 1.0e-2))[:, 1].max()) >= 32768


def _tasks_struct(n, p, lists=True):
    t = _mz().MazeTasks()
    t.n, t.n_tasks = n, 1
    for f in ("start", "goal", "walls", "texts", "food_rewards", "food_interval", "scalars"):
        setattr(t, f, p)
    if lists:
        t.food_cells, t.n_food, t.max_food, t.cell_slot, t.slot_food, t.slot_interval = p, p, 1, p, p, p
    return t


def _mz():
    from metagym_amd import _lib
    return _lib


def _state_struct(p, by_slot):
    st = _mz().MazeState()
    for f in ("task_id", "grid", "steps", "ori_idx", "ori", "loc", "life", "cur_food", "wait_refresh", "revival"):
        setattr(st, f, p)
    st.food_by_slot = by_slot
    return st


def test_library_refuses_int16_lists_on_tables_past_32768_cells():
    """mg_maze_reset / mg_maze2d_step / mg_maze3d_step: a food_cells or cell_slot list on a table with more than 32 768 cells is
    MG_ERR_BAD_SIZE naming n, decided on the host before any launch (non-NULL dummy pointers, no GPU)."""
    lib = _mz().load()
    fake = C.create_string_buffer(1024)
    p = C.addressof(fake)
    view = _view(p)
    for n in (183, 255):
        for which in ("food_cells", "cell_slot"):
            t = _tasks_struct(n, p)
            setattr(t, "cell_slot" if which == "food_cells" else "food_cells", None)
            for by_slot in (0, 1):
                st = _state_struct(p, by_slot)
                assert lib.mg_maze_reset(t, 1, 4, st, None, None) == -1002
                assert b"maze n=%d" % n in lib.mg_last_error() and b"32 768" in lib.mg_last_error()
                assert lib.mg_maze2d_step(t, 1, 10, 2, 0, 4, st, p, p, p, p, p, None) == -1002
            assert lib.mg_maze3d_step(t, view, 0, 10, 0, 0, 4, _state_struct(p, 0), p, p, p, p, p, None) == -1002
            assert b"maze n=%d" % n in lib.mg_last_error()
    # the bound itself: n = 181 with lists passes check_tasks (and then fails later on the 3-D record bound, not on the lists)
    t = _tasks_struct(181, p)
    view.max_ray_records = 0
    assert lib.mg_maze3d_step(t, view, 0, 10, 0, 0, 4, _state_struct(p, 0), p, p, p, p, p, None) == -1004
    assert b"translucent" in lib.mg_last_error()


def _view(p, res=(32, 32), mrr=17):
    v = _mz().MazeView()
    v.res_h, v.res_v = res
    v.max_vision, v.l_focal, v.text_size, v.tan_half_fov, v.collision_dist = 12.0, 0.2, 1.0, float(np.tan(0.3 * L.PI)), 0.2
    v.col_cos = v.col_sin = v.textures = v.ceil_texture = p
    v.n_textures, v.tex_size, v.max_ray_records = 7, 64, mrr
    return v


def test_library_refuses_record_bounds_above_127():
    """mg_maze3d_step: min(2n+1, max_ray_records or no bound) above 127 is MG_ERR_UNSUPPORTED before anything runs — it used to be
    clamped to 127 silently, dropping the farthest translucent cells of long rays. A bound of 127 or less passes this check; the
    frame here is 4000 rows tall, so every such call then stops at the next host-side refusal (LDS > 160 KiB, MG_ERR_BAD_SIZE)
    and nothing is ever launched on the dummy pointers, GPU or not."""
    lib = _mz().load()
    fake = C.create_string_buffer(1024)
    p = C.addressof(fake)
    st = _state_struct(p, 0)
    res = (32, 4000)
    for n, mrr, refused in ((63, 0, False), (64, 0, True), (65, 127, False), (65, 128, True), (101, 245, True), (101, 125, False),
                            (255, 0, True), (255, 17, False)):
        t = _tasks_struct(n, p, lists=False)
        rc = lib.mg_maze3d_step(t, _view(p, res=res, mrr=mrr), 0, 10, 0, 0, 4, st, p, p, p, p, p, None)
        err = lib.mg_last_error()
        if refused:
            assert rc == -1004 and b"127" in err and b"maze n=%d" % n in err, (n, mrr, rc, err)
        else:
            t_max = min(2 * n + 1, mrr or 2 * n + 1)
            assert mr.maze3d_route(n, res, [2.0])["lds"] > mr.LDS_LIMIT                 # (the restatement agrees it is refused)
            assert rc == -1002 and b"of LDS" in err and b"maze n=%d" % n in err, (n, mrr, t_max, rc, err)


def test_env_record_bound_matches_the_library_rule():
    """The env's set_task check restates min(2n+1, 2 * int(max_vision / cell size) + 5) > 127: n <= 63 never trips it, and from
    n = 64 on a cell size at or below 12 / 62 does."""
    assert L.documented_record_bound(63, 0.01) == 127
    assert L.documented_record_bound(64, 12.0 / 62) == 129 and L.documented_record_bound(64, 0.194) == 127
    assert L.documented_record_bound(255, 2.0) == 17


def test_record_premise_restatement_agrees_with_the_documented_bound():
    """The numpy ray walk (maze_large_cases.ray_records): no column crosses more translucent cells than the bound
    mg_maze_view.max_ray_records documents (2 * floor(max_vision / cell size) + 4, and 2n + 1) and records are a subset of the
    crossings — so wherever that bound is <= 127 no record can be dropped. The GPU test's field (n = 81, cell 0.1) has columns
    that hit the far wall within sight with records of the far strength past the 127th (the premise of its divergence); the
    same field with ONE food value has columns past 127 records too, but nothing a dropped record would change."""
    for n, cs, res in ((81, 0.1, (64, 64)), (81, 0.1, (128, 64)), (101, 0.1, (64, 64)), (81, 0.2, (64, 64)), (33, 0.5, (48, 32))):
        task = L.open_field_task(n, cs)
        recs = L.ray_records(task, res)
        bound = 2 * int(12.0 / cs) + 4
        assert all(r[1] == len(r[3]) <= r[0] <= min(bound, 2 * n + 1) for r in recs), (n, cs, res)
        if L.documented_record_bound(n, cs) <= L.MAX_RAY_RECORDS:
            assert not L.dropped_record_columns(task, res), (n, cs, res)
    for res in ((64, 64), (128, 64)):
        assert L.dropped_record_columns(L.open_field_task(81, 0.1), res), res
        flat = L.open_field_task(81, 0.1, near_food=0.5, far_food=0.5)
        assert any(r[2] and r[1] > L.MAX_RAY_RECORDS for r in L.ray_records(flat, res))
        assert not L.dropped_record_columns(flat, res)
    for seed in range(3):
        task = L.synthetic_task(101, seed, cell_size=0.25, wall_frac=0.02, food_frac=0.9)
        assert all(r[0] <= 2 * int(12.0 / 0.25) + 4 for r in L.ray_records(task, (64, 48)))


def test_lds_restatement_refuses_past_160_kib():
    """maze_routes.maze3d_route's `lds` grows with n; at the stock cell size a 32 x 32 frame fits n = 124 (the figure in
    include/metagym_hip.h), and the GPU test checks the refused size's bytes against the library's own message."""
    sizes = [mr.maze3d_route(n, (32, 32), [2.0])["lds"] for n in range(3, 256)]
    assert sizes == sorted(sizes)
    n_max = max(n for n in range(3, 256) if mr.maze3d_route(n, (32, 32), [2.0])["lds"] <= mr.LDS_LIMIT)
    assert n_max == 124


def test_golden_maze_tasks_keep_their_earlier_cases_byte_identical():
    """tests/golden/maze_tasks.npz gained cases 8 and 9 (n = 41 and n = 63, drawn by the unmodified reference sampler through
    oracle/gen_golden_maze_tasks.py); test_oracle_maze_sampler.py and the device golden test cover them like the others. Cases
    0-7 and the shared keys are pinned by digest: appending must not have changed one byte of them."""
    import hashlib
    import json
    import os
    g = np.load(os.path.join(mr.GOLDEN, "maze_tasks.npz"))
    cases = json.loads(str(g["cases"]))
    assert [(c["n"], c.get("allow_loops")) for c in cases[8:]] == [(41, True), (63, False)]
    assert hashlib.sha256(json.dumps(cases[:8]).encode()).hexdigest() == \
        "4d86d1941b793ec0479ab6c8056fb28b765af156e71dbe35f82fe801cd52ac63"
    h = hashlib.sha256()
    for k in sorted(g.files):
        if k == "cases" or k.startswith(("c8_", "c9_")):
            continue
        a = g[k]
        h.update(k.encode())
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == "0ad02b0514806ad1e5c16da5d5f7a78ec0ec086189b0316f41988478d7b5dd84"
    assert all("c%d_s%d_walls" % (c, s) in g.files for c in (8, 9) for s in g["seeds"])
