"""BASELINE configs[4] / SURVEY.md §8(d) C5 and the north-star batch size under test (GPU box, -m gpu):
  * the mixed two-stream step bench.py times (`bench.MixedStep`: quadrotor launch + maze3d launch on two HIP streams)
    is, bit for bit, each family stepped alone — with episodes ending (fused auto-reset) inside the compared steps;
  * Quadrotor hovering_control at 2^20 envs on one GPU (north_star's total batch; 2^17 is its per-GPU share) and at
    2^17: 256 sampled envs of the fused-auto-reset run against the CPU oracle, bit-exact state and counters."""
import numpy as np
import pytest
import torch

import bench
from oracle import quadrotor as qo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _maze_state(env):
    return {k: v.clone() for k, v in env.state_dict().items() if torch.is_tensor(v)}


def test_mixed_two_stream_step_equals_each_family_alone():
    dev = torch.device(DEV)
    n, T = 4096, 40
    plan = bench.shard_plan(0, 1, n, "mixed")
    # short episodes so both families restart envs inside the compared steps (quadrotor: clock nt = 7 staggered by
    # env id + floor hits; maze: max_steps = 9 and SURVIVAL deaths)
    mk_q = lambda: bench.QuadrotorShard(dev, plan, n, preroll=0, nt=7)
    mk_m = lambda: bench.MazeShard(dev, plan, n, res=64, max_steps=9)
    quad, maze = mk_q(), mk_m()
    quad_alone, maze_alone = mk_q(), mk_m()
    torch.cuda.synchronize()
    both = bench.MixedStep(dev, quad, maze)
    q_ends = m_ends = 0
    for t in range(T):
        both(t)
        quad_alone.step(t)
        maze_alone.step(t)
        torch.cuda.synchronize()
        for a, b in ((quad.env._obs, quad_alone.env._obs), (quad.env._reward, quad_alone.env._reward),
                     (quad.env._reward64, quad_alone.env._reward64), (quad.env._done, quad_alone.env._done),
                     (quad.env._failed, quad_alone.env._failed),
                     (maze.env._obs, maze_alone.env._obs), (maze.env._reward, maze_alone.env._reward),
                     (maze.env._done, maze_alone.env._done)):
            assert torch.equal(a, b), t
        q_ends += int(quad.env._done.sum())
        m_ends += int(maze.env._done.sum())
    sa, sb = quad.env.state_dict(), quad_alone.env.state_dict()
    for k in ("pos", "vel", "omega", "propw", "rot", "ct", "episode"):
        assert torch.equal(sa[k], sb[k]), k
    ma, mb = _maze_state(maze.env), _maze_state(maze_alone.env)
    assert ma.keys() == mb.keys()
    for k in ma:
        assert torch.equal(ma[k], mb[k]), k
    assert q_ends >= 4 * n and m_ends >= 3 * n        # every env restarted several times inside the compared steps
    assert int(quad.env.episode.min()) >= 4


@pytest.mark.parametrize("n", [1 << 17, 1 << 20])
def test_north_star_batch_sampled_against_oracle(n):
    """The north-star batch (2^20 quadrotors; 2^17 = one GPU's share of it on 8 GPUs) through the launch bench.py
    times — fused auto-reset, clocks staggered by global env id — 256 sampled envs replayed on the CPU oracle:
    final state, clock and episode counter bit-exact, with clock wraps and floor hits inside."""
    import metagym_amd
    nt, T, seed, base = 13, 30, 1000, 3 << 20
    env = metagym_amd.make("quadrotor-v0", num_envs=n, device=DEV, task="hovering_control", nt=nt, auto_reset=True,
                           seed=seed, env_id_base=base)
    env.reset(seed=5)
    ids = torch.arange(n, device=DEV, dtype=torch.int64) + base
    sd = env.state_dict()
    sd["ct"] = ((ids * 977) % nt).to(torch.int32)
    sd["pos"][2, ::5] = -4.98                        # a fifth start 2 cm above the floor: collision episode ends
    env.load_state_dict(sd)
    idx = np.sort(np.random.RandomState(n & 0xFFFF).choice(n, 256, replace=False))
    idx[0], idx[-1] = 0, n - 1                       # both ends of the batch (last wave, last lane)
    idx_t = torch.as_tensor(idx, device=DEV)
    st0 = {k: sd[k][..., idx_t].cpu().numpy() for k in ("pos", "vel", "omega", "propw", "rot", "ct")}
    g = torch.Generator(device=DEV)
    g.manual_seed(11)
    acts_s = np.zeros((T, 256, 4), np.float32)
    dones = torch.zeros(n, dtype=torch.int64, device=DEV)
    for t in range(T):
        a = torch.rand(n, 4, device=DEV, generator=g) * 14.9 + 0.1
        acts_s[t] = a[idx_t].cpu().numpy()
        obs, rew, done, info = env.step(a)
        dones += done
    assert int(dones.min()) >= 2 and int(info["failed"].max()) == 0
    fin = env.state_dict()
    c = qo.default_consts(nt=nt)
    collided = 0
    for j, e in enumerate(idx):
        st = qo.make_states(st0["pos"].T[[j]], st0["vel"].T[[j]], st0["omega"].T[[j]], st0["propw"].T[[j]], st0["rot"].T[[j]])
        ct, epo = st0["ct"][[j]].astype(np.int32), np.zeros(1, np.uint32)
        ar = qo.default_autoreset(seed=seed, env_id_base=base + int(e))
        for t in range(T):
            before = int(ct[0])
            out = qo.batch_env_step_autoreset(c, ar, st, ct, epo, acts_s[t][[j]])
            collided += int(out[2][0] != 0 and before + 1 != nt)
        o = qo.states_to_arrays(st)
        for k, kk in (("pos", "pos"), ("vel", "vel"), ("omega", "omega"), ("propw", "propw"), ("rot", "R")):
            assert np.array_equal(fin[k][..., e].cpu().numpy(), o[kk][0]), (k, e)
        assert int(fin["ct"][e]) == int(ct[0]) and int(fin["episode"][e]) == int(epo[0])
    assert collided > 0


def test_c5_per_gpu_size_sampled_against_both_oracles():
    """C5 at its per-GPU size: 65 536 quadrotors + 65 536 MetaMazeDiscrete3D envs (9x9, 64x64 int32 frames: the SMALL kernel over a
    grid of 65 536 workgroups, envs rotated over the XCDs by mg::env_of_block) through bench.MixedStep, with short episodes so both
    families restart inside the 12 compared steps. 128 sampled envs of each family, env 0 and env n-1 among them, replayed with the
    shards' resident action batches: quadrotors on oracle/quadrotor.py's auto-reset step (final state, clock and episode
    bit-exact), mazes on oracle/maze.py (reward, done, the whole per-env state and every pixel of every step bit-exact)."""
    from metagym_amd.metamaze import MAZE_TASK_MANAGER
    from oracle import maze as mo
    dev = torch.device(DEV)
    n, nt, max_steps, T = 65536, 5, 4, 12
    plan = bench.shard_plan(0, 1, n, "mixed")
    quad = bench.QuadrotorShard(dev, plan, n, nt=nt)
    maze = bench.MazeShard(dev, plan, n, res=64, max_steps=max_steps)
    torch.cuda.synchronize()
    step = bench.MixedStep(dev, quad, maze)
    rs = np.random.RandomState(65536)
    qs = np.sort(rs.choice(np.arange(1, n - 1), 126, replace=False))
    ms = np.sort(rs.choice(np.arange(1, n - 1), 126, replace=False))
    qs, ms = np.concatenate([[0], qs, [n - 1]]), np.concatenate([[0], ms, [n - 1]])
    qs_t, ms_t = torch.as_tensor(qs, device=DEV), torch.as_tensor(ms, device=DEV)

    # quadrotor: the sampled envs' state after the shard's pre-roll, and the action rows they will get
    sd = quad.env.state_dict()
    st0 = {k: sd[k][..., qs_t].cpu().numpy() for k in ("pos", "vel", "omega", "propw", "rot", "ct", "episode")}
    q_act = [quad.action_list[i % bench.N_ACTION_BATCHES][qs_t].cpu().numpy() for i in range(T)]
    # maze: the sampled envs start from reset() (checked against the oracle's reset state and frame)
    tasks = bench.maze_tasks()
    ids = maze.env.task_id.cpu().numpy()
    assert np.array_equal(ids, plan["maze_task_ids"])
    otasks = [mo.Task(**t._asdict()) for t in tasks]
    tt = mo.SURVIVAL
    states = {int(e): mo.State(otasks[ids[e]]) for e in ms}
    for e in ms:
        mo.reset(otasks[ids[e]], tt, states[int(e)])
    view = mo.View(MAZE_TASK_MANAGER.grounds.astype(np.uint8), MAZE_TASK_MANAGER.ceil, 64, 64)
    m_act = [maze.actions[i % 4][ms_t].cpu().numpy() for i in range(T)]

    def maze_matches(label):
        ob = maze.env._obs[ms_t].cpu().numpy()
        grid, steps, life = (maze.env.grid[:, ms_t].cpu().numpy(), maze.env.steps[ms_t].cpu().numpy(),
                             maze.env.life[ms_t].cpu().numpy())
        oidx = maze.env.ori_idx[ms_t].cpu().numpy()
        food, wait, rev = (x[ms_t].cpu().numpy() for x in (maze.env.cur_food, maze.env.wait_refresh, maze.env.revival))
        for k, e in enumerate(ms):
            s = states[int(e)]
            assert (grid[0, k], grid[1, k], steps[k], oidx[k]) == (s.c.grid[0], s.c.grid[1], s.c.steps, s.c.ori_idx), (label, e)
            assert life[k] == s.c.life, (label, e)
            assert np.array_equal(food[k], s.cur_food) and np.array_equal(wait[k], s.wait) and np.array_equal(rev[k], s.revival), (label, e)
            ref = mo.observe_3d(otasks[ids[e]], tt, view, s, 0)
            d = int((ob[k] != ref).sum())
            assert d == 0, "%s env %d: %d pixel values differ" % (label, e, d)

    maze_matches("reset")
    m_ends = 0
    for i in range(T):
        step(i)
        torch.cuda.synchronize()
        r64, d = maze.env.reward64[ms_t].cpu().numpy(), maze.env._done[ms_t].cpu().numpy()
        for k, e in enumerate(ms):
            s, task = states[int(e)], otasks[ids[e]]
            r, dd = mo.step_disc3d(task, tt, max_steps, s, int(m_act[i][k]))
            assert r == r64[k] and dd == bool(d[k]), (i, e)
            if dd:                                          # fused auto-reset
                mo.reset(task, tt, s)
                m_ends += 1
        maze_matches("step %d" % i)
    assert m_ends >= 2 * len(ms), m_ends

    fin = quad.env.state_dict()
    c = qo.default_consts(nt=nt)
    q_ends = 0
    for j, e in enumerate(qs):
        st = qo.make_states(st0["pos"].T[[j]], st0["vel"].T[[j]], st0["omega"].T[[j]], st0["propw"].T[[j]], st0["rot"].T[[j]])
        ct, epo = st0["ct"][[j]].astype(np.int32), st0["episode"][[j]].astype(np.int64).astype(np.uint32)
        ar = qo.default_autoreset(seed=plan["job_seed"], env_id_base=plan["env_id_base"] + int(e))
        for i in range(T):
            out = qo.batch_env_step_autoreset(c, ar, st, ct, epo, q_act[i][[j]])
            q_ends += int(out[2][0] != 0)
        o = qo.states_to_arrays(st)
        for k, kk in (("pos", "pos"), ("vel", "vel"), ("omega", "omega"), ("propw", "propw"), ("rot", "R")):
            assert np.array_equal(fin[k][..., e].cpu().numpy(), o[kk][0]), (k, e)
        assert int(fin["ct"][e]) == int(ct[0]) and (int(fin["episode"][e]) & 0xFFFFFFFF) == int(epo[0]), e
    assert q_ends >= 2 * len(qs), q_ends
