"""The continuous 3-D maze move, branch by branch, on the CPU: what ties oracle/maze_oracle.c to the reference in the
branches the two golden walks never take.

  goldens (recorded from the reference)  ->  restatement (tests/maze_cont_cases.py), bit for bit over both walks;
  restatement's collision_force is equivariant under the quarter turn (x, y) -> (-y, x), bit for bit, so the one edge the
      goldens take (C-D) vouches for the other three;
  restatement  ->  C oracle, bit for bit on placed cases that take every branch and stand on both sides of every comparison.

Conditions on the INPUTS (asserted by the case builder before anything runs; no case is left out of a comparison):
  * every sub-step position of every case lies inside [0, n * cell) in both axes;
  * every census key is taken by the exact cases (`guard_edge_norm`, max(1e-6, edge_norm), is dead code: the edges have length
    1; it is asserted to stay at 0);
  * an exact case either does not walk (any heading, any turn) or walks straight from heading 0 (cos 0 = 1, sin 0 = 0): no
    transcendental then reaches the location, so everything is compared bit for bit;
  * a general case never evaluates the inside-a-wall formula, never evaluates its switch within 1e-4 of |dv| = 0.5 (the one
    discontinuity of the force), and never ends a step within 1e-4 cells of a cell boundary; its location is compared to the
    project's 1e-5 (the sin / cos of glibc, NumPy and the device may differ in the last place), its heading bit for bit."""
import glob
import os

import numpy as np
import pytest

import maze_cont_cases as mc
from oracle import maze as mo

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "maze3d_cont_*.npz")))


@pytest.fixture(scope="module")
def built():
    return mc.build_cases()


def test_restatement_replays_the_goldens_bit_for_bit():
    """Location, heading and grid of every step of both walks, resets included; reward and done too."""
    assert len(GOLDEN) == 2
    for path in GOLDEN:
        g = np.load(path)
        ag = mc.Agent(mc.task_from_golden(g), mc.SURVIVAL if "survival" in path else mc.ESCAPE, int(g["max_steps"]))
        for t, a in enumerate(g["actions"]):
            if g["reset_before"][t]:
                ag.reset()
            r, d = ag.step(float(a[0]), float(a[1]))
            assert (float(ag.loc[0]), float(ag.loc[1])) == tuple(g["loc"][t]), (path, t)
            assert float(ag.ori) == float(g["ori"][t]), (path, t)
            assert list(ag.grid) == list(g["grid"][t]), (path, t)
            assert r == g["reward"][t] and d == bool(g["done"][t]) and ag.steps == g["steps"][t], (path, t)
            if "survival" in path:
                assert ag.life == g["life"][t], (path, t)


def test_goldens_take_one_edge_only():
    """Why the rest of this file exists: the census of the two golden walks. If new goldens ever take more, say so in DESIGN.md."""
    cen, worst = mc.golden_census(GOLDEN)
    assert worst == 0.0
    print(dict(cen))
    assert cen["edge_CD"] > 0 and cen["nearest_within"] == cen["edge_CD"] == cen["force"] + cen["no_force"]
    for key in ("edge_AB", "edge_BC", "edge_DA", "nearest_end_1", "nearest_end_2", "inside", "neighbour_out_of_grid",
                "guard_inside_dist", "guard_ori_norm", "pushing_2", "pushing_3", "pushing_4"):
        assert cen[key] == 0, key


@pytest.mark.parametrize("cell_size", mc.CELL_SIZES)
@pytest.mark.parametrize("col_dist", mc.COL_DISTS)
def test_collision_force_quarter_turn_equivariance(cell_size, col_dist):
    """force(-y, x) == (-f_y, f_x) bit for bit (zeros compared with ==), 17 000 seeded float32 vectors per combination, 102 000
    in all; vectors on a diagonal, where the edge choice is not symmetric, are skipped, counted and capped at 1 %."""
    rs = np.random.RandomState(int(cell_size * 100) + int(col_dist * 1000))
    n = 17000
    v = rs.uniform(-1.3, 1.3, (n, 2)).astype(np.float32)
    v[: n // 10] = np.round(v[: n // 10] * 16) / 16                      # a tenth on a 1/16 grid: faces, corners, diagonals
    cen = mc.Census()
    skipped = 0
    for x, y in v:
        if abs(x) == abs(y):
            skipped += 1
            continue
        f, _ = mc.collision_force((x, y), cell_size, col_dist, cen)
        g, _ = mc.collision_force((mc.F(-y), x), cell_size, col_dist, cen)
        assert g[0] == -f[1] and g[1] == f[0], (x, y, f, g)
    assert skipped <= n // 100
    assert all(cen[k] > 0 for k in ("inside", "force", "no_force", "nearest_end_1", "nearest_end_2") + mc.KEYS_EDGES)


def _oracle_run(otask, tt, case, steps=None):
    st = mo.State(otask)
    mo.reset(otask, tt, st)
    st.c.loc[0], st.c.loc[1] = float(case.loc[0]), float(case.loc[1])
    st.c.ori = float(case.ori)
    cs32 = np.float32(otask.c.cell_size)
    st.c.grid[0], st.c.grid[1] = int(np.float32(case.loc[0]) / cs32), int(np.float32(case.loc[1]) / cs32)
    out = []
    for turn, walk in case.actions[:steps]:
        r, d = mo.step_cont3d(otask, tt, mc.MAX_STEPS, st, float(turn), float(walk), case.col_dist)
        out.append((np.float64(st.c.ori), (np.float32(st.c.loc[0]), np.float32(st.c.loc[1])), (st.c.grid[0], st.c.grid[1]), r, d))
    return out


def _same_bits(got, want):
    """heading (float64) and location (float32 pair) of a step record, by their bytes."""
    return (np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes()
            and np.asarray(got[1], np.float32).tobytes() == np.asarray(want[1], np.float32).tobytes())


def test_builder_conditions_and_census(built):
    """Every census key, every comparison with a float32-adjacent pair on both sides, every input condition: asserted again
    here so that an edit of the case list cannot silently drop a branch."""
    mc.check_conditions(built)
    for key in mc.ALL_KEYS:
        assert built.census[key] > 0, key


def test_oracle_matches_restatement_on_exact_cases(built):
    """Location, heading, grid, reward and done bit for bit, three steps from every placed exact case."""
    otasks = {n: [mo.Task(**t) for t in ts] for n, ts in built.tab.items()}
    for c in built.exact:
        got = _oracle_run(otasks[c.n][c.task], mo.ESCAPE, c)
        for s, (g, w) in enumerate(zip(got, built.expect[c])):
            assert _same_bits(g, w), (c, s, g, w)
            assert tuple(g[2]) == tuple(w[2]) and g[3] == w[3] and g[4] == w[4], (c, s, g, w)


def test_oracle_matches_restatement_survival(built):
    """One SURVIVAL step from every exact case of the 7 x 7 table (some placements lie on food cells)."""
    otasks = [mo.Task(**t) for t in built.tab[7]]
    ate = 0
    for c in built.exact:
        if c.n != 7:
            continue
        got = _oracle_run(otasks[c.task], mo.SURVIVAL, c, 1)[0]
        cut = c._replace(actions=c.actions[:1])
        want = mc.run_case(built.tab, cut, mc.SURVIVAL)[0][0]
        assert _same_bits(got, want) and tuple(got[2]) == tuple(want[2]), (c, got, want)
        assert got[3] == want[3] and got[4] == want[4], c
        ate += int(want[3] > 0)
    assert ate > 5


def test_oracle_matches_restatement_on_general_cases(built):
    """Heading bit for bit; grid, reward and done equal; location within 1e-5."""
    otasks = {n: [mo.Task(**t) for t in ts] for n, ts in built.tab.items()}
    worst = 0.0
    for c in built.general:
        got = _oracle_run(otasks[c.n][c.task], mo.ESCAPE, c)
        for s, (g, w) in enumerate(zip(got, built.expect[c])):
            assert np.float64(g[0]).tobytes() == np.float64(w[0]).tobytes(), (c, s)
            assert tuple(g[2]) == tuple(w[2]) and g[3] == w[3] and g[4] == w[4], (c, s)
            assert np.allclose(g[1], w[1], rtol=1e-5, atol=1e-5), (c, s, g[1], w[1])
            worst = max(worst, abs(float(g[1][0]) - float(w[1][0])), abs(float(g[1][1]) - float(w[1][1])))
    print("general cases: largest location difference oracle - restatement", worst)
