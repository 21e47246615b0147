"""Every launch route of the maze3d renderer (mg_maze3d_step: maze3d_step_kernel<REC, STOCK, SMALL, U8> at 1, 2 or 4 waves per
env, 32- or 64-column slabs, byte or packed uint8 stores) against oracle/maze_oracle.c: reward, done, the per-env state and every
pixel of every frame. The default library's routes run in this process; the routes behind the process-wide MG_MAZE3D_* knobs run
in one fresh child process per knob setting (tests/maze_route_child.py). tests/maze_routes.py holds the route map, the case lists
and the comparison body. GPU box only (-m gpu)."""
import fcntl
import gc
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import maze_routes as mr
from oracle import maze as mo

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHILD = os.path.join(HERE, "maze_route_child.py")
LOCK = os.path.join(tempfile.gettempdir(), "metagym_amd_maze_route_child.lock")   # one child at a time, even under xdist
CHILD_TIMEOUT_S = 420
_first_abnormal_end = None       # set by the first child that ends with a signal, an abort / segfault exit or a time-out


def _assert_clean(summary):
    assert summary["frames"] > 0 and summary["resets"] > 0, summary       # masked resets happened inside the compared steps
    assert summary["bad"] == 0, "%s: %d of %d pixel values differ from the oracle; first: %s" % (
        summary["case"], summary["bad"], summary["values"], summary["first_bad"])


def _line(s):
    r = s["route"]
    return ("%-30s REC %d %-7s SMALL %d waves %d slab %d u8 %-6s: %4d frames, %9d values, %d differ, %d resets, %d frames "
            "skipped (pose not bit-equal), max oracle value %d" % (
                s["case"], r["rec"], "stock" if r["stock"] else "general", r["small"], r["waves"], r["slab"], r["u8"],
                s["frames"], s["values"], s["bad"], s["resets"], s["pose_not_bit_equal"], s["max_ref"]))


@pytest.mark.parametrize("case", mr.DEFAULT_CASES, ids=[c["name"] for c in mr.DEFAULT_CASES])
def test_maze3d_default_route_matches_oracle(case):
    assert not any(k in os.environ for k in mr.KNOBS), "the default routes are tested without MG_MAZE3D_* knobs"
    s = mr.run_case(case)
    print(_line(s))
    _assert_clean(s)


@pytest.mark.parametrize("tid,knob,value,cases", mr.KNOB_CASES, ids=[k[0] for k in mr.KNOB_CASES])
def test_maze3d_knob_route_matches_oracle(tid, knob, value, cases):
    global _first_abnormal_end
    if _first_abnormal_end is not None:
        pytest.fail("not started: an earlier route child ended abnormally (%s)" % _first_abnormal_end)
    env = {k: v for k, v in os.environ.items() if k not in mr.KNOBS}
    env[knob] = value
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD, json.dumps(cases)]
    with open(LOCK, "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            _first_abnormal_end = "%s=%s: timed out after %d s" % (knob, value, CHILD_TIMEOUT_S)
            pytest.fail(_first_abnormal_end)
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _first_abnormal_end = "%s=%s: exit status %d" % (knob, value, p.returncode)
        pytest.fail("%s\n%s" % (_first_abnormal_end, p.stderr[-4000:]))
    assert p.returncode == 0, "%s=%s child failed (exit %d):\n%s" % (knob, value, p.returncode, p.stderr[-6000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("MAZE_ROUTE_CHILD ")]
    assert len(lines) == 1, p.stdout[-2000:]
    summaries = json.loads(lines[0][len("MAZE_ROUTE_CHILD "):])
    assert [s["case"] for s in summaries] == [c["name"] for c in cases]
    for s, c in zip(summaries, cases):
        print("%s=%s " % (knob, value) + _line(s))
        assert s["route"] == mr.case_route(c, {knob: value})          # the child saw the knob
    u8 = [s["max_ref"] for s, c in zip(summaries, cases) if c["dtype"] == "uint8"]
    assert not u8 or max(u8) > 255                                     # the uint8 saturation is exercised
    for s in summaries:
        _assert_clean(s)


def test_shared_task_table_survives_the_other_env():
    """Two envs on one device-sampled task table: when env A goes away (collected, or moved to another table by set_task), env B's
    checked uniform_cell_size must stay checked — B.step() captured into a hipGraph right after succeeds (no hidden readback), and
    its replays equal an eager twin's steps and the oracle, frame for frame."""
    import metagym_amd
    from metagym_amd.metamaze import MAZE_TASK_MANAGER
    mr.use_reference_textures()
    kw = dict(n=9, allow_loops=False, step_reward=-0.01, goal_reward=1.0, food_density=0.2, food_interval=3)
    n_envs, max_steps, res = 8, 5, (32, 32)
    for how in ("collect", "set_task"):
        table = MAZE_TASK_MANAGER.sample_tasks_device(3, device="cuda:0", seed=500, **kw)
        mk = lambda: metagym_amd.make("meta-maze-discrete-3D-v0", num_envs=n_envs, device="cuda:0", max_steps=max_steps,
                                      resolution=res, task_type="SURVIVAL", auto_reset=True)
        a, b, twin = mk(), mk(), mk()
        for e in (a, b, twin):
            e.set_task(table)
        b.reset()
        twin.reset()
        if how == "collect":
            del a
            gc.collect()
        else:
            a.set_task(MAZE_TASK_MANAGER.sample_tasks_device(2, device="cuda:0", seed=900, **kw))
        torch.cuda.synchronize()
        act = torch.zeros(n_envs, dtype=torch.int32, device="cuda:0")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):        # the first step of B after A's change: must not need to re-read the table
            b.step(act)
        tasks = table.to_task_configs()
        ids = b.task_id.cpu().numpy()
        otasks = [mo.Task(**t._asdict()) for t in tasks]
        states = [mo.State(otasks[i]) for i in ids]
        for s, i in zip(states, ids):
            mo.reset(otasks[i], mo.SURVIVAL, s)
        view = mo.View(MAZE_TASK_MANAGER.grounds.astype(np.uint8), MAZE_TASK_MANAGER.ceil, res[0], res[1])
        rs = np.random.RandomState(4)
        ends = 0
        for t in range(12):
            a_np = rs.choice(4, size=n_envs, p=[0.2, 0.2, 0.1, 0.5]).astype(np.int32)
            act.copy_(torch.as_tensor(a_np))
            g.replay()
            ob_t, r_t, d_t, _ = twin.step(act)
            torch.cuda.synchronize()
            assert torch.equal(b._obs, ob_t) and torch.equal(b.reward64, twin.reward64) and torch.equal(b._done, d_t), (how, t)
            ob, r64, d = b._obs.cpu().numpy(), b.reward64.cpu().numpy(), b._done.cpu().numpy()
            for e in range(n_envs):
                r, dd = mo.step_disc3d(otasks[ids[e]], mo.SURVIVAL, max_steps, states[e], int(a_np[e]))
                assert r == r64[e] and dd == bool(d[e]), (how, t, e)
                if dd:
                    mo.reset(otasks[ids[e]], mo.SURVIVAL, states[e])
                    ends += 1
                assert np.array_equal(ob[e], mo.observe_3d(otasks[ids[e]], mo.SURVIVAL, view, states[e], 0)), (how, t, e)
        assert ends >= n_envs, (how, ends)
        del g
