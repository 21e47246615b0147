"""`MetaMaze2D.rollout_policy` with a softmax-sampled policy (mg_maze2d_policy_rollout_sampled, csrc/maze_policy.hip and
csrc/mg_sample.h): the move of every env at every step is a Gumbel-max draw from softmax(l / temperature) inside the launch.
  1. the full closed loop on the host, `MazePolicy.reference` alternated with the CPU maze oracle (oracle/maze_oracle.c),
     every record, observation, result, the end carry and the env state bit for bit; 2. replay identity through `rollout`;
  3. splitting a rollout; 4. record=False; 5. epsilon with a temperature; 7. hipGraph capture.
GPU box only (-m gpu)."""
import numpy as np
import pytest
import torch

from maze_large_cases import synthetic_task
from metagym_amd.metamaze import MazePolicy, MazePolicyState
from oracle import maze as mo
from test_maze_gpu import _oracle_batch, reference_textures  # noqa: F401  (module fixture: the reference's textures)
from test_maze_policy_gpu import _same_carry, _same_sd, check_results_against_records, make_policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
MAX_STEPS = 11
TEMPS = np.array([0.25, 1.0, 4.0], F)


def sampled(pol, temperature=TEMPS, epsilon=None):
    return MazePolicy(pol.wx, pol.wh, pol.b, pol.wo, pol.bo, epsilon=epsilon, temperature=temperature)


def make_env(N, task_type, n, view_grid, auto_reset=True):
    """A device batch on six synthetic n x n tasks (maze_large_cases: any n, food and crumbs for SURVIVAL), reset, and the
    oracle's tasks and states of the same batch."""
    import metagym_amd
    tasks = [synthetic_task(n, 40 + s) for s in range(6)]
    env = metagym_amd.make("meta-maze-2D-v0", num_envs=N, device=DEV, max_steps=MAX_STEPS, task_type=task_type,
                           auto_reset=auto_reset, view_grid=view_grid)
    env.set_task(tasks)
    ids = env.task_id.cpu().numpy()
    otasks, states = _oracle_batch(tasks, ids, mo.TASK_TYPES[task_type])
    env.reset()
    return env, (otasks, states, ids)


def host_closed_loop(pol, pids, host, task_type, view_grid, auto_reset, T, state0, seed, episodic=False):
    """`MazePolicy.reference` for the move, the CPU oracle for the step, per env; advances the oracle states in place.
    Returns the records (actions, reward64, done, obs after every step), the end carry and the explored mask."""
    otasks, states, ids = host
    tt, N = mo.TASK_TYPES[task_type], len(states)
    observe = lambda: np.stack([mo.observe_2d(otasks[ids[e]], tt, states[e], view_grid) for e in range(N)]).astype(F)
    st = state0.numpy()
    win = observe()
    acts, r64, dn, obs, expl = [], [], [], [], []
    for t in range(T):
        a, hn, ex = pol.reference(win, pids, st, seed=seed, return_explored=True)
        r, d = np.zeros(N), np.zeros(N, bool)
        for e in range(N):
            r[e], d[e] = mo.step_2d(otasks[ids[e]], tt, MAX_STEPS, states[e], int(a[e]))
            if d[e] and auto_reset:
                mo.reset(otasks[ids[e]], tt, states[e])
        st = MazePolicyState(hn, a.copy(), r.astype(F), d.astype(np.uint8), st.step + 1)
        if episodic and auto_reset:
            st.h[d], st.prev_action[d], st.prev_reward[d], st.prev_done[d] = 0, -1, 0, 0
        win = observe()
        for lst, v in ((acts, a), (r64, r), (dn, d), (obs, win), (expl, ex)):
            lst.append(v)
    return dict(actions=np.stack(acts), reward64=np.stack(r64), done=np.stack(dn), obs=np.stack(obs)), st, np.stack(expl)


def check_against_host(res, env, rec, carry, host, what):
    got = {k: getattr(res, k).cpu().numpy() for k in ("actions", "reward64", "done", "obs", "reward")}
    assert np.array_equal(got["actions"], rec["actions"]), (what, "first difference at step %d"
                                                            % int(np.argmax((got["actions"] != rec["actions"]).any(1))))
    assert np.array_equal(got["reward64"].view(np.uint64), rec["reward64"].view(np.uint64)), (what, "reward64")
    assert np.array_equal(got["reward"].view(np.uint32), rec["reward64"].astype(F).view(np.uint32)), (what, "reward")
    assert np.array_equal(got["done"], rec["done"]), (what, "done")
    assert np.array_equal(got["obs"].view(np.uint32), rec["obs"].view(np.uint32)), (what, "obs")
    assert torch.equal(env._obs, res.obs[-1])
    _same_carry(res.state, carry, what)
    check_results_against_records(res)
    states = host[1]
    assert np.array_equal(env.steps.cpu().numpy(), np.asarray([s.c.steps for s in states])), (what, "steps")
    assert np.array_equal(env.grid.cpu().numpy().T, np.asarray([list(s.c.grid) for s in states])), (what, "grid")


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("task_type,n,view_grid,H,ids_kind", [
    ("ESCAPE", 5, 1, 5, "one id per wave"), ("SURVIVAL", 5, 2, 64, "mixed ids"),
    ("ESCAPE", 15, 2, 5, "mixed ids"), ("SURVIVAL", 15, 1, 64, "one id per wave")])
def test_full_closed_loop_oracle(task_type, n, view_grid, H, ids_kind):
    """N = 130 (two full waves and a partial one), T = 40 at max_steps = 11 with auto_reset: at least three episodes end per
    env. One id per wave stages the policy in LDS, mixed ids read it per lane; the temperatures differ per policy; the
    counter crosses 2^32."""
    N, T, P = 130, 40, 3
    env, host = make_env(N, task_type, n, view_grid)
    pol = sampled(make_policy(P, H, view_grid, 7 * n + H))
    pids = (np.arange(N) // 64) % P if ids_kind == "one id per wave" else np.arange(N) % P
    state0 = MazePolicyState.zeros(N, H, DEV)
    state0.step = (1 << 32) - 20
    before = state0.clone()
    seed = (5 << 32) | 17
    res = env.rollout_policy(pol, T, policy_ids=pids, state=state0, seed=seed, record=True, obs_every=1)
    _same_carry(state0, before, "the carry handed in is not written")
    assert res.state.step == state0.step + T and res.actions.shape == (T, N) and res.obs_steps == list(range(T))
    rec, carry, explored = host_closed_loop(pol, pids, host, task_type, view_grid, True, T, before, seed)
    check_against_host(res, env, rec, carry, host, (task_type, n, view_grid, H, ids_kind))
    # the case does what it is for: all four moves are drawn, by every policy, and episodes end
    assert not explored.any() and (rec["done"].sum(0) >= 3).all()
    for p in range(P):
        assert sorted(set(rec["actions"][:, pids == p].ravel().tolist())) == [0, 1, 2, 3], p


# ---------------------------------------------------------------------------------------------------------- 2, 3, 4
def test_replay_splitting_and_record_false():
    N, T, H, vg, P = 130, 40, 5, 2, 3
    env, _ = make_env(N, "SURVIVAL", 15, vg)
    pol = sampled(make_policy(P, H, vg, 12))
    sd0 = env.state_dict()
    whole = env.rollout_policy(pol, T, seed=9, record=True, obs_every=1)
    sd1, steps1 = env.state_dict(), env.steps.clone()
    # 2. the recorded actions through `rollout` from the same snapshot
    env.load_state_dict(sd0)
    obs, rew, done, info = env.rollout(whole.actions, obs_every=1)
    assert torch.equal(rew, whole.reward) and torch.equal(env.rollout_reward64, whole.reward64) and torch.equal(done, whole.done)
    assert torch.equal(obs, whole.obs) and torch.equal(info["steps"], steps1)
    _same_sd(env.state_dict(), sd1, "replay")
    # 3. T1 = 13 then T2 = 27 through one carry
    env.load_state_dict(sd0)
    a = env.rollout_policy(pol, 13, seed=9, record=True, obs_every=1)
    b = env.rollout_policy(pol, 27, state=a.state, seed=9, record=True, obs_every=1)
    for name in ("actions", "reward", "reward64", "done", "obs"):
        assert torch.equal(torch.cat([getattr(a, name), getattr(b, name)]), getattr(whole, name)), name
    _same_sd(env.state_dict(), sd1, "split")
    _same_carry(b.state, whole.state, "split")
    assert (a.state.step, b.state.step) == (13, 40) and torch.equal(a.episodes + b.episodes, whole.episodes)
    # 4. record=False
    env.load_state_dict(sd0)
    lean = env.rollout_policy(pol, T, seed=9)
    assert lean.actions is None and lean.reward is None and lean.reward64 is None and lean.done is None
    for name in ("ret_total", "ret_episode", "episode_len", "episodes"):
        assert torch.equal(getattr(lean, name), getattr(whole, name)), name
    assert torch.equal(lean.obs, whole.obs[-1])
    _same_sd(env.state_dict(), sd1, "record=False")
    _same_carry(lean.state, whole.state, "record=False")
    # another seed: other draws
    env.load_state_dict(sd0)
    assert not torch.equal(env.rollout_policy(pol, T, seed=10, record=True).actions, whole.actions)


# ---------------------------------------------------------------------------------------------------------- 5
def test_epsilon_with_a_temperature():
    N, T, H, vg, P = 130, 40, 5, 1, 3
    seed, step0 = (9 << 32) | 4, (1 << 32) - 7
    base = make_policy(P, H, vg, 31)
    pids = np.arange(N) % P

    def run(epsilon, episodic=False):
        env, host = make_env(N, "ESCAPE", 15, vg)
        st = MazePolicyState.zeros(N, H, DEV)
        st.step = step0
        pol = sampled(base, epsilon=epsilon)
        res = env.rollout_policy(pol, T, state=st, seed=seed, record=True, obs_every=1, episodic=episodic)
        return res, env, host, pol, st
    none = run(None)[0]
    mid, env, host, pol, st = run(np.array([0.25, 0.0, 0.6]), episodic=True)
    rec, carry, explored = host_closed_loop(pol, pids, host, "ESCAPE", vg, True, T, st, seed, episodic=True)
    check_against_host(mid, env, rec, carry, host, "epsilon and temperature, episodic")
    from metagym_amd._policy import philox4x32_10
    n = step0 + np.arange(T, dtype=np.uint64)[:, None]
    out = philox4x32_10(np.arange(N, dtype=np.uint64)[None, :], n & np.uint64(0xFFFFFFFF), n >> np.uint64(32), 0x4D5A, 4, 9)
    assert np.array_equal(explored, out[0] < pol.thresholds[pids][None, :])
    assert not explored[:, pids == 1].any() and 0 < explored[:, pids == 0].sum() < explored[:, pids == 0].size
    # where the draw fires the move is out[1] & 3; at step 0 (one shared history) the sampled move stands elsewhere
    acts = mid.actions.cpu().numpy()
    assert np.array_equal(acts[explored], (out[1] & np.uint32(3)).astype(np.int32)[explored])
    assert np.array_equal(acts[0][~explored[0]], none.actions.cpu().numpy()[0][~explored[0]])
    assert (acts[0][explored[0]] != none.actions.cpu().numpy()[0][explored[0]]).any()
    zero = run(np.zeros(P))[0]
    assert torch.equal(zero.actions, none.actions) and torch.equal(zero.obs, none.obs)


# ---------------------------------------------------------------------------------------------------------- 7
def test_graph_capture_of_one_call():
    """Captured once and replayed twice, the call equals eager calls on a twin env. step0 is an argument of the launch, so a
    replay draws with the counters of the captured call: the eager twin is handed the same step."""
    from test_graph_capture_gpu import _capture
    N, T, H, vg, P = 130, 25, 5, 2, 3
    pol = sampled(make_policy(P, H, vg, 17))
    pol.to(DEV)
    pol.inv_temperature_on(DEV)
    eager, _ = make_env(N, "SURVIVAL", 15, vg)
    env, _ = make_env(N, "SURVIVAL", 15, vg)
    static = MazePolicyState.zeros(N, H, DEV)
    names = ("h", "prev_action", "prev_reward", "prev_done")
    out = {}

    def run():
        res = env.rollout_policy(pol, T, state=static, seed=5, record=True)
        for name in names:
            getattr(static, name).copy_(getattr(res.state, name))
        out["res"] = res

    sd0 = env.state_dict()
    graph = _capture(run)
    env.load_state_dict(sd0)
    zero = MazePolicyState.zeros(N, H, DEV)
    for name in names:
        getattr(static, name).copy_(getattr(zero, name))
    st = None
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        if st is not None:
            st.step = 0
        want = eager.rollout_policy(pol, T, state=st, seed=5, record=True)
        st = want.state
        for name in ("actions", "reward", "reward64", "done", "ret_total", "ret_episode", "episode_len", "episodes"):
            assert torch.equal(getattr(out["res"], name), getattr(want, name)), (rep, name)
        assert torch.equal(static.h.view(torch.int32), st.h.view(torch.int32)) and torch.equal(static.prev_action, st.prev_action)
        _same_sd(env.state_dict(), eager.state_dict(), rep)
        assert torch.equal(env._obs, eager._obs)
    assert bool(out["res"].done.any())
