"""`MetaMaze2D.rollout_policy` (mg_maze2d_policy_rollout, csrc/maze_policy.hip): closed-loop rollouts with per-env recurrent
policies inside the launch.
  1. replay identity: the recorded actions through `rollout` from the same snapshot give the same records, observations and
     end state; `MazePolicy.reference`, fed the recorded observations, reproduces every action and the end carry bit for bit;
     the four per-env results equal their definition computed from the records;
  2. exploration; 3. splitting a rollout; 4. episodic=True; 5. staged and per-lane weight reads; 6. -0 and NaN
     pre-activations on the device; 7. record=False; 8. hipGraph capture; 9. refused calls.
GPU box only (-m gpu)."""
import numpy as np
import pytest
import torch

from metagym_amd.metamaze.policy import MazePolicy, MazePolicyState, input_dim, philox4x32_10
from test_maze_gpu import reference_textures  # noqa: F401  (module fixture: the task sampler counts the reference's textures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
MAX_STEPS = 11


def make_tasks(n, count=6, seed0=10):
    from metagym_amd.metamaze import MazeTaskSampler
    return [MazeTaskSampler(n=n, allow_loops=True, step_reward=-0.01, goal_reward=1.0, food_density=0.1, food_interval=4,
                            initial_life=0.3, seed=seed0 + s) for s in range(count)]


def make_env(n_envs, task_type, auto_reset, view_grid, n=9, tasks=None, max_steps=MAX_STEPS, task_ids=None):
    import metagym_amd
    env = metagym_amd.make("meta-maze-2D-v0", num_envs=n_envs, device=DEV, max_steps=max_steps, task_type=task_type,
                           auto_reset=auto_reset, view_grid=view_grid)
    env.set_task(make_tasks(n) if tasks is None else tasks, task_ids=task_ids)
    env.reset()
    return env


def make_policy(P, H, view_grid, seed, epsilon=None):
    """Random weights scaled by 1 / sqrt(fan-in): pre-activations of order one, so the clamp is hit on both sides and not
    always, and logits close enough for every move to win somewhere."""
    rs = np.random.RandomState(seed)
    D = input_dim(view_grid)
    fan = np.sqrt(D + H)
    return MazePolicy((rs.randn(P, H, D) * (3.0 / fan)).astype(F), (rs.randn(P, H, H) * (3.0 / fan)).astype(F),
                      (0.3 * rs.randn(P, H)).astype(F), (rs.randn(P, 4, H) / np.sqrt(H)).astype(F), (0.2 * rs.randn(P, 4)).astype(F),
                      epsilon)


def _same_sd(sa, sb, what):
    assert sorted(sa) == sorted(sb)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), (what, key)


def _same_carry(a, b, what):
    a, b = a.numpy(), b.numpy()
    assert np.array_equal(a.h.view(np.uint32), b.h.view(np.uint32)), (what, "h")
    assert np.array_equal(a.prev_action, b.prev_action), (what, "prev_action")
    assert np.array_equal(a.prev_reward.view(np.uint32), b.prev_reward.view(np.uint32)), (what, "prev_reward")
    assert np.array_equal(a.prev_done, b.prev_done), (what, "prev_done")
    assert a.step == b.step, (what, "step")


def first_window(env):
    """The window of the state the env holds: the observe-only launch `reset` ends with."""
    return env._observe().clone().cpu().numpy()


def reference_rollout(pol, ids, win0, res, state0, seed, clear_at_done):
    """`MazePolicy.reference` step by step on the recorded observations (win0 for step 0), carrying h itself; prev_reward and
    prev_done come from the reward and done records, prev_action is the reference's own action. `clear_at_done`: restart from
    a zero carry at every done (episodic=True with auto_reset). Returns the actions [T, N], the end carry, the explored mask."""
    obs, rew, dn = res.obs.cpu().numpy(), res.reward.cpu().numpy(), res.done.cpu().numpy()
    T, N = rew.shape
    assert res.obs_steps == list(range(T)) and obs.shape[0] == T
    st = state0.numpy()
    win, acts, expl = win0, [], []
    for t in range(T):
        a, hn, ex = pol.reference(win, ids, st, seed=seed, return_explored=True)
        acts.append(a)
        expl.append(ex)
        st = MazePolicyState(hn, a.copy(), rew[t].copy(), dn[t].astype(np.uint8), st.step + 1)
        if clear_at_done:
            d = dn[t].astype(bool)
            st.h[d] = 0
            st.prev_action[d] = -1
            st.prev_reward[d] = 0
            st.prev_done[d] = 0
        win = obs[t]
    return np.stack(acts), st, np.stack(expl)


def check_results_against_records(res):
    """ret_total: the T float64 rewards added in step order; ret_episode / episode_len: up to and including the first done;
    episodes: the number of steps with done."""
    r64, dn = res.reward64.cpu().numpy(), res.done.cpu().numpy().astype(bool)
    T, N = r64.shape
    total, epi = np.zeros(N), np.zeros(N)
    length, ended = np.zeros(N, np.int32), np.zeros(N, bool)
    for t in range(T):
        total = total + r64[t]
        epi = np.where(ended, epi, epi + r64[t])
        length = length + (~ended).astype(np.int32)
        ended = ended | dn[t]
    assert np.array_equal(res.ret_total.cpu().numpy(), total)
    assert np.array_equal(res.ret_episode.cpu().numpy(), epi)
    assert np.array_equal(res.episode_len.cpu().numpy(), length)
    assert np.array_equal(res.episodes.cpu().numpy(), dn.sum(0).astype(np.int32))
    assert np.array_equal(res.reward.cpu().numpy(), r64.astype(F))


def check_replay_identity(env, pol, ids, T, state=None, seed=0, episodic=False, what=None):
    """Parts 1 and 2 of the identity, and the per-env results; returns (result, explored mask)."""
    N = env.num_envs
    state = MazePolicyState.zeros(N, pol.hidden, DEV) if state is None else state
    before = state.clone()
    sd0 = env.state_dict()
    win0 = first_window(env)
    res = env.rollout_policy(pol, T, policy_ids=ids, state=state, seed=seed, record=True, obs_every=1, episodic=episodic)
    _same_carry(state, before, (what, "the carry handed in is not written"))
    assert res.actions.shape == (T, N) and res.actions.dtype == torch.int32 and res.done.dtype == torch.bool
    assert res.obs.shape == (T,) + tuple(env._obs.shape) and res.state.step == state.step + T
    sd1, steps1, last1 = env.state_dict(), env.steps.clone(), env._obs.clone()
    assert torch.equal(last1, res.obs[-1])
    # 1: the recorded actions through rollout() from the same snapshot
    env.load_state_dict(sd0)
    obs, rew, done, info = env.rollout(res.actions, obs_every=1)
    assert torch.equal(rew, res.reward) and torch.equal(env.rollout_reward64, res.reward64) and torch.equal(done, res.done), what
    assert torch.equal(obs, res.obs) and torch.equal(info["steps"], steps1), what
    _same_sd(env.state_dict(), sd1, what)
    # 2: the policy half
    ids_h = np.arange(N) % pol.num_policies if ids is None else np.asarray(ids)
    acts, carry, expl = reference_rollout(pol, ids_h, win0, res, before, seed, episodic and env.auto_reset)
    got = res.actions.cpu().numpy()
    assert np.array_equal(got, acts), (what, "first difference at step %d" % int(np.argmax((got != acts).any(1))))
    _same_carry(res.state, carry, what)
    check_results_against_records(res)
    return res, expl


CASES = [   # task_type, auto_reset, view_grid, n, H, N, T, P, weight seed
    ("ESCAPE", True, 1, 9, 5, 1, 40, 1, 0),      # (one env, one policy: a seed whose single trajectory takes all four moves)
    ("SURVIVAL", True, 3, 15, 64, 65, 40, 3, 1),
    ("SURVIVAL", False, 2, 9, 1, 130, 7, 5, 2),
    ("ESCAPE", False, 3, 9, 64, 130, 1, 64, 3),
    ("ESCAPE", True, 2, 15, 5, 65, 40, 65, 4),
    ("SURVIVAL", True, 1, 9, 64, 130, 40, 2, 5),
    ("ESCAPE", False, 1, 15, 1, 65, 40, 4, 6),
]


def test_the_grid_holds_every_value_the_cases_must_cover():
    cols = list(zip(*CASES))
    assert set(cols[0]) == {"ESCAPE", "SURVIVAL"} and set(cols[1]) == {True, False} and set(cols[2]) == {1, 2, 3}
    assert set(cols[3]) == {9, 15} and set(cols[4]) == {1, 5, 64} and set(cols[5]) == {1, 65, 130} and set(cols[6]) == {1, 7, 40}
    assert any(c[2] == 3 and c[4] == 64 and c[5] == 65 for c in CASES)


@pytest.mark.parametrize("task_type,auto_reset,view_grid,n,H,N,T,P,wseed", CASES)
def test_replay_identity(task_type, auto_reset, view_grid, n, H, N, T, P, wseed):
    env = make_env(N, task_type, auto_reset, view_grid, n=n)
    pol = make_policy(P, H, view_grid, wseed)
    res, _ = check_replay_identity(env, pol, None, T, what=(task_type, auto_reset, view_grid, n, H, N, T))
    acts, dn = res.actions.cpu().numpy(), res.done.cpu().numpy()
    print("actions", np.bincount(acts.ravel(), minlength=4), "dones per env", dn.sum(0).min(), dn.sum(0).max())
    assert sorted(set(acts.ravel().tolist())) == [0, 1, 2, 3]                   # the weights were chosen for it
    if T == 40 and auto_reset:
        assert (dn.sum(0) >= 3).all()                                          # max_steps = 11: at least three episodes end
    if N * H >= 64:                                                            # the clamp acts somewhere and not everywhere
        h = res.state.h.cpu().numpy()
        assert (np.abs(h) == 1).any() and (np.abs(h) < 1).any()


def test_exploration():
    N, T, H, vg, P = 130, 40, 5, 2, 4
    eps = np.array([0.25, 0.25, 0.0, 0.0])
    pol = make_policy(P, H, vg, 11, epsilon=eps)
    env = make_env(N, "SURVIVAL", True, vg)
    sd0 = env.state_dict()
    st0 = MazePolicyState.zeros(N, H, DEV)
    st0.step = (1 << 32) - 7                                                   # the counter crosses 2^32 inside the rollout
    seed = (5 << 32) | 17
    res, expl = check_replay_identity(env, pol, None, T, state=st0, seed=seed, what="exploration")
    ids = np.arange(N) % P
    first = expl[:, ids < 2]
    assert 0 < first.sum() < first.size and not expl[:, ids >= 2].any()
    print("exploratory draws", int(first.sum()), "of", first.size)
    # the numpy Philox is the device function
    from metagym_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(0)
    inp = rs.randint(0, 2 ** 32, (512, 6), dtype=np.uint64).astype(np.uint32)
    inp[0] = [3, 0xFFFFFFFF, 0, 0x4D5A, 17, 5]
    d_in = torch.as_tensor(inp.view(np.int32)).to(DEV)
    d_out = torch.zeros(len(inp), 4, dtype=torch.int32, device=DEV)
    _lib.check(lib.mg_selftest_philox(_lib.ptr(d_in), _lib.ptr(d_out), len(inp), _lib.current_stream(d_out.device)), "philox")
    want = np.stack(philox4x32_10(*[inp[:, k] for k in range(6)]), 1)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)
    # the same seed gives the same actions, another seed other actions
    env.load_state_dict(sd0)
    again = env.rollout_policy(pol, T, state=st0, seed=seed, record=True)
    assert torch.equal(again.actions, res.actions)
    env.load_state_dict(sd0)
    other = env.rollout_policy(pol, T, state=st0, seed=seed + 1, record=True)
    assert not torch.equal(other.actions, res.actions)


def test_splitting_a_rollout():
    N, H, vg, P = 65, 5, 1, 3
    pol = make_policy(P, H, vg, 12, epsilon=np.array([0.2, 0.0, 1.0]))
    env = make_env(N, "SURVIVAL", True, vg)
    sd0 = env.state_dict()
    whole = env.rollout_policy(pol, 40, seed=9, record=True, obs_every=1)
    sd_whole = env.state_dict()
    env.load_state_dict(sd0)
    a = env.rollout_policy(pol, 3, seed=9, record=True, obs_every=1)
    b = env.rollout_policy(pol, 37, state=a.state, seed=9, record=True, obs_every=1)
    for name in ("actions", "reward", "reward64", "done", "obs"):
        assert torch.equal(torch.cat([getattr(a, name), getattr(b, name)]), getattr(whole, name)), name
    _same_sd(env.state_dict(), sd_whole, "split")
    _same_carry(b.state, whole.state, "split")
    assert (a.state.step, b.state.step, whole.state.step) == (3, 40, 40)
    assert torch.equal(a.episodes + b.episodes, whole.episodes)


def test_episodic_clears_the_carry_at_a_done():
    N, T, H, vg, P = 65, 40, 5, 1, 3
    pol = make_policy(P, H, vg, 13)
    env = make_env(N, "ESCAPE", True, vg)
    sd0 = env.state_dict()
    res, _ = check_replay_identity(env, pol, None, T, episodic=True, what="episodic")      # (restarts from a zero carry)
    assert (res.done.sum(0) >= 3).all()
    env.load_state_dict(sd0)
    trial = env.rollout_policy(pol, T, record=True)
    assert not torch.equal(trial.actions, res.actions)                         # the flag acts
    first = int(res.done.any(1).cpu().numpy().argmax())                        # up to the first done nothing differs
    assert torch.equal(trial.actions[:first + 1], res.actions[:first + 1])
    # without auto_reset nothing restarts and the flag changes nothing
    env2 = make_env(N, "ESCAPE", False, vg)
    sd = env2.state_dict()
    x = env2.rollout_policy(pol, T, record=True, episodic=True)
    env2.load_state_dict(sd)
    y = env2.rollout_policy(pol, T, record=True)
    assert torch.equal(x.actions, y.actions) and bool(x.done.any())
    _same_carry(x.state, y.state, "no auto_reset")


@pytest.mark.parametrize("H,view_grid", [(5, 2), (64, 3)])
def test_staged_and_per_lane_weight_reads_agree(H, view_grid):
    """The same (env, policy) pairs laid out one id per wave (the staged route) and interleaved (per-lane reads)."""
    N, T, P = 192, 12, 3
    tasks = make_tasks(9)
    pol = make_policy(P, H, view_grid, 14)
    e = np.arange(N)
    staged_ids, staged_task = e // 64, (e % 64) % len(tasks)
    perm = (e % 3) * 64 + e // 3                       # interleaved position q holds the pair of staged position perm[q]
    mixed_ids, mixed_task = staged_ids[perm], staged_task[perm]
    assert all(len(set(staged_ids[w * 64:(w + 1) * 64])) == 1 for w in range(3))
    assert all(len(set(mixed_ids[w * 64:(w + 1) * 64])) == 3 for w in range(3))
    out = []
    for ids, tid in ((staged_ids, staged_task), (mixed_ids, mixed_task)):
        env = make_env(N, "SURVIVAL", True, view_grid, tasks=tasks, task_ids=torch.as_tensor(tid.astype(np.int32)))
        out.append(env.rollout_policy(pol, T, policy_ids=ids, record=True, obs_every=1))
    s, m = out
    p = torch.as_tensor(perm, device=DEV)
    for name in ("actions", "reward64", "done"):
        assert torch.equal(getattr(s, name)[:, p], getattr(m, name)), name
    assert torch.equal(s.obs[:, p], m.obs)
    assert torch.equal(s.state.h[p].view(torch.int32), m.state.h.view(torch.int32))
    for name in ("ret_total", "ret_episode", "episode_len", "episodes"):
        assert torch.equal(getattr(s, name)[p], getattr(m, name)), name
    assert len(set(s.actions.cpu().numpy().ravel().tolist())) == 4


@pytest.mark.parametrize("H", [2, 3])
def test_negative_zero_and_nan_pre_activations_on_the_device(H):
    """Two policies on one open SURVIVAL maze (walls on the border only, start in the middle, life 2.5), H = 2, and H = 3,
    where the partial quad adds v.x, v.y and v.z and skips one padding float (0 * -0 is -0, so a read too far would not
    show in a zero; the poisoned padding of test_policy_sizes_gpu.py is what shows it), three steps.
    Policy 0 keeps a pre-activation of exactly -0: a sum is -0 only if every addend is, so b = -0, every input weight is -0
    (all its inputs are >= 0: no wall is in view for three steps, and the previous reward of SURVIVAL is the food eaten), and
    the recurrent weights are +0 on a carry handed in as -0 (+0 * -0 = -0). bo prefers move 0, which keeps the window clear of
    the border for the three steps. Policy 1 overflows to NaN in unit 0 at the first step: 3e38 * life = +inf, then -3e38
    times a handed-in previous reward of 2 = -inf. From then on every unit of it is NaN (0 * NaN) and every logit too: move
    0. Actions and h equal the reference's; the NaN payload is not compared."""
    from metagym_amd.metamaze import MazeTaskSampler
    N, T, vg = 65, 3, 1
    D, ww = input_dim(vg), 9
    base = MazeTaskSampler(n=9, allow_loops=True, step_reward=-0.01, food_density=0.1, food_interval=4, initial_life=2.5,
                           max_life=4.0, seed=20)
    walls = np.zeros_like(np.asarray(base.cell_walls))
    walls[0, :] = walls[-1, :] = walls[:, 0] = walls[:, -1] = 1
    env = make_env(N, "SURVIVAL", True, vg, tasks=[base._replace(cell_walls=walls, start=(4, 4))])
    assert float(env.life.min()) >= 2.0
    wx, wh, b = np.zeros((2, H, D), F), np.zeros((2, H, H), F), np.zeros((2, H), F)
    wo, bo = np.zeros((2, 4, H), F), np.zeros((2, 4), F)
    wx[0], b[0] = -0.0, -0.0
    bo[:, 0] = 1.0
    wx[1, 0, 4], wx[1, 0, ww + 4] = 3e38, -3e38                    # the centre of the window (the life), the previous reward
    wx[1, 1, :ww], wo[1, 1:, 1] = 0.1, 1.0                         # an ordinary unit beside it
    pol = MazePolicy(wx, wh, b, wo, bo)
    ids = (np.arange(N) % 2).astype(np.int32)
    st0 = MazePolicyState.zeros(N, H, DEV)
    st0.h[torch.as_tensor(ids == 0, device=DEV)] = -0.0
    st0.prev_reward[torch.as_tensor(ids == 1, device=DEV)] = 2.0
    assert bool(torch.signbit(st0.h[0]).all())
    win0, sd0 = first_window(env), env.state_dict()
    assert (win0[:, 1, 1] >= 2.0).all() and (win0 >= 0).all()
    res = env.rollout_policy(pol, T, policy_ids=ids, state=st0, record=True, obs_every=1)
    assert (res.obs[:-1].cpu().numpy() >= 0).all()                 # no wall came into a window the policy read
    acts, carry, _ = reference_rollout(pol, ids, win0, res, st0, 0, False)
    assert np.array_equal(res.actions.cpu().numpy(), acts) and not acts.any()
    h, want = res.state.h.cpu().numpy(), carry.h
    assert np.array_equal(h[ids == 0].view(np.uint32), want[ids == 0].view(np.uint32))
    assert (h[ids == 0] == 0).all() and np.signbit(h[ids == 0]).all()                 # -0 after three steps
    assert np.isnan(h[ids == 1]).all() and np.isnan(want[ids == 1]).all()
    # one step alone: unit 0 is NaN, unit 1 (computed from the carry before the step) is still the ordinary value
    env.load_state_dict(sd0)
    one = env.rollout_policy(pol, 1, policy_ids=ids, state=st0, record=True, obs_every=1)
    a1, c1, _ = reference_rollout(pol, ids, win0, one, st0, 0, False)
    h1 = one.state.h.cpu().numpy()
    assert np.isnan(h1[ids == 1, 0]).all() and np.isnan(c1.h[ids == 1, 0]).all()
    assert np.array_equal(h1[ids == 1, 1].view(np.uint32), c1.h[ids == 1, 1].view(np.uint32)) and (h1[ids == 1, 1] > 0).all()
    assert np.array_equal(one.actions.cpu().numpy(), a1)


def test_record_false_returns_the_same_results_and_end_state():
    N, T, H, vg, P = 130, 40, 5, 2, 7
    pol = make_policy(P, H, vg, 15, epsilon=np.full(P, 0.1))
    env = make_env(N, "SURVIVAL", True, vg)
    sd0 = env.state_dict()
    full = env.rollout_policy(pol, T, seed=3, record=True, obs_every=3)
    sd_full, obs_full = env.state_dict(), env._obs.clone()
    env.load_state_dict(sd0)
    env._obs.zero_()
    lean = env.rollout_policy(pol, T, seed=3)
    assert lean.actions is None and lean.reward is None and lean.reward64 is None and lean.done is None
    assert lean.obs.data_ptr() == env._obs.data_ptr() and lean.obs_steps == [T - 1]
    assert full.obs_steps == [2, 5, 8, 11, 14, 17, 20, 23, 26, 29, 32, 35, 38, 39] and full.obs.shape[0] == 14
    assert torch.equal(lean.obs, obs_full) and torch.equal(full.obs[-1], obs_full)
    for name in ("ret_total", "ret_episode", "episode_len", "episodes"):
        assert torch.equal(getattr(lean, name), getattr(full, name)), name
    _same_sd(env.state_dict(), sd_full, "record=False")
    _same_carry(lean.state, full.state, "record=False")
    assert bool((full.episodes >= 3).all())


def test_graph_capture_of_one_call():
    """Captured once and replayed twice, the call equals two eager calls on a twin env (the end carry is copied back into the
    captured input inside the graph; without epsilon no argument depends on the step counter)."""
    from test_graph_capture_gpu import _capture
    N, T, H, vg, P = 65, 9, 5, 2, 3
    pol = make_policy(P, H, vg, 16)
    eager, env = (make_env(N, "SURVIVAL", True, vg) for _ in range(2))
    static = MazePolicyState.zeros(N, H, DEV)
    out = {}

    def run():
        res = env.rollout_policy(pol, T, state=static, record=True, obs_every=4)
        for name in ("h", "prev_action", "prev_reward", "prev_done"):
            getattr(static, name).copy_(getattr(res.state, name))
        out["res"] = res

    sd0 = env.state_dict()
    graph = _capture(run)
    env.load_state_dict(sd0)                                      # the warm-up and the capture pass advanced the state
    zero = MazePolicyState.zeros(N, H, DEV)
    for name in ("h", "prev_action", "prev_reward", "prev_done"):
        getattr(static, name).copy_(getattr(zero, name))
    st = None
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        want = eager.rollout_policy(pol, T, state=st, record=True, obs_every=4)
        st = want.state
        got = out["res"]
        for name in ("actions", "reward", "reward64", "done", "obs", "ret_total", "ret_episode", "episode_len", "episodes"):
            assert torch.equal(getattr(got, name), getattr(want, name)), (rep, name)
        assert torch.equal(static.h.view(torch.int32), st.h.view(torch.int32)) and torch.equal(static.prev_action, st.prev_action)
        _same_sd(env.state_dict(), eager.state_dict(), rep)
    assert bool(out["res"].done.any())


def test_refused_calls_leave_the_env_and_the_carry_unchanged():
    import metagym_amd
    N, H, vg, P = 65, 5, 2, 3
    pol = make_policy(P, H, vg, 17)
    fresh = metagym_amd.make("meta-maze-2D-v0", num_envs=N, device=DEV, max_steps=MAX_STEPS, task_type="ESCAPE", view_grid=vg)
    with pytest.raises(Exception, match="set_task"):
        fresh.rollout_policy(pol, 3)
    fresh.set_task(make_tasks(9))
    with pytest.raises(Exception, match="reset"):
        fresh.rollout_policy(pol, 3)
    env = make_env(N, "SURVIVAL", True, vg)
    st = env.rollout_policy(pol, 5).state
    sd0, st0, obs0 = env.state_dict(), st.clone(), env._obs.clone()
    bad_ids = np.arange(N) % P
    bad_ids[-1] = P
    neg_ids = np.arange(N) % P
    neg_ids[0] = -1
    refusals = [
        (ValueError, dict(policy_ids=bad_ids)),                                    # an id out of range
        (ValueError, dict(policy_ids=neg_ids)),
        (ValueError, dict(policy_ids=np.zeros(N - 1, int))),
        (ValueError, dict(policy=make_policy(P, H, 1, 17))),                       # a policy built for another view_grid
        (ValueError, dict(state=MazePolicyState.zeros(N - 1, H, DEV))),            # a carry of another N
        (ValueError, dict(state=MazePolicyState.zeros(N, H + 1, DEV))),            # ... of another H
        (ValueError, dict(steps=0)),
        (ValueError, dict(steps=-3)),
        (ValueError, dict(obs_every=-1)),
        (TypeError, dict(policy="greedy")),
    ]
    for exc, kw in refusals:
        args = dict(policy=pol, steps=4, state=st)
        args.update(kw)
        with pytest.raises(exc):
            env.rollout_policy(**args)
        _same_sd(env.state_dict(), sd0, kw)
        _same_carry(st, st0, kw)
        assert torch.equal(env._obs, obs0)
    # and the env still runs
    res = env.rollout_policy(pol, 4, state=st)
    assert res.state.step == 9
    from metagym_amd.metamaze import MetaMazeContinuous3D, MetaMazeDiscrete3D
    assert not hasattr(MetaMazeDiscrete3D, "rollout_policy") and not hasattr(MetaMazeContinuous3D, "rollout_policy")


def test_a_device_policy_ids_tensor_is_kept_until_it_is_written():
    """The same device tensor, unchanged, is not read back on a repeated call and gives the same rollout; an in-place write
    is seen, validated again, and gives what a fresh env gives for that assignment as a host array."""
    N, P, H, T, vg = 65, 2, 2, 4, 1                                   # one full wave and one ragged wave
    pol = make_policy(P, H, vg, 31)
    env = make_env(N, "SURVIVAL", True, vg)
    sd0 = env.state_dict()
    ids = torch.from_numpy((np.arange(N) % P).astype(np.int32)).to(DEV)
    records = ("actions", "reward", "reward64", "done")
    first = env.rollout_policy(pol, T, policy_ids=ids, record=True)
    keep = env._policy_ids_keep
    assert keep[2] is ids and keep[3] == ids._version
    env.load_state_dict(sd0)
    again = env.rollout_policy(pol, T, policy_ids=ids, record=True)
    assert env._policy_ids_keep is keep                               # the fast path: nothing read back, nothing stored
    for name in records:
        assert torch.equal(getattr(again, name), getattr(first, name)), name
    other = ((np.arange(N) // 3 + 1) % P).astype(np.int32)
    ids.copy_(torch.from_numpy(other))
    env.load_state_dict(sd0)
    changed = env.rollout_policy(pol, T, policy_ids=ids, record=True)
    assert env._policy_ids_keep is not keep and env._policy_ids_keep[3] == ids._version
    fresh = make_env(N, "SURVIVAL", True, vg)
    fresh.load_state_dict(sd0)
    want = fresh.rollout_policy(pol, T, policy_ids=other, record=True)
    for name in records:
        assert torch.equal(getattr(changed, name), getattr(want, name)), name
    _same_sd(env.state_dict(), fresh.state_dict(), "in-place write")
    _same_carry(changed.state, want.state, "in-place write")
    assert not torch.equal(changed.actions, first.actions)            # the two assignments do play differently
