"""The seven in-launch networks at the sizes tests/policy_size_cases.py derives from their remainder code, on the GPU.

  1. Replay identity, one test per launch, at every added size: a short closed loop whose recorded actions, run through
     `rollout()`, give the same records and end state, and whose actions and end carry are `reference` of the records, bit
     for bit. The helpers are the older tests' own. N = 130 with lanes 0..63 on one policy id (staged in LDS) and the rest
     mixed (per-lane reads), P = 3, T = 12; the walker, one workgroup per env, N = 65 and T = 6; LiftSim T = 60 with three
     envs on the Python oracle and all 130 on the reference loop.
  2. Poisoned padding, one test per padded layout: the same launch twice, the second time with a quiet NaN in every padding
     float of the device copy the kernel reads. The kernels promise that padding never enters a sum (0 * h would turn a -0
     into +0, 0 * inf is NaN); with the zeros pack() writes, a read one entry too far gives the same bits as a correct one.
     Everything the launch returns must be equal bit for bit. A NaN can only reach a sum: no index is computed from a weight.

The -0 constructions at a partial quad are the older tests', parametrized over H where they stand. GPU box only (-m gpu)."""
import numpy as np
import pytest
import torch

import liftsim_policy_cases as PC
import policy_size_cases as SC
import quadrotor_policy_cases as pc
import test_bandits_policy_gpu as bd
import test_liftsim_policy_gpu as ls
import test_maze_policy_gpu as mz
import test_quadrotor_policy_gpu as qm
import test_quadrotor_rpolicy_gpu as qr
import test_walker_policy_gpu as wm
import test_walker_rpolicy_gpu as wr
from test_maze_gpu import reference_textures  # noqa: F401  (module fixture: the task sampler counts the reference's textures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, P, T = SC.N, SC.P, SC.T


def _ids():
    ids = SC.layout_ids()
    assert len(set(ids[:64].tolist())) == 1 and len(set(ids[64:128].tolist())) == P       # one launch, both weight routes
    assert np.array_equal(ids, pc.layout_ids())
    return ids


def _two_distinct(actions, what):
    a = actions.cpu().numpy()
    rows = a.reshape(-1, a.shape[-1]) if a.dtype.kind == "f" else a.reshape(-1, 1)
    assert len(np.unique(rows, axis=0)) >= 2, (what, "one action only: the weights decide nothing")


def _clamp_acts_somewhere_and_not_everywhere(h, what):
    """Required where N * H >= 64, which holds at every size of this grid (N = 130 or 65)."""
    h = h.cpu().numpy()
    if h.size < 64:
        return
    print(what, "|h| == 1:", int((np.abs(h) == 1).sum()), "|h| < 1:", int((np.abs(h) < 1).sum()), "of", h.size)
    assert (np.abs(h) == 1).any() and (np.abs(h) < 1).any(), what


# ---------------------------------------------------------------------------------------------- 1. replay identity
def _quadrotor_make(D):
    return (lambda: qr._env()) if D == 16 else (lambda: qr._env(task="velocity_control", nt=40, seed=6))


@pytest.mark.parametrize("H,D", SC.QUADROTOR_RECURRENT_ADDED)
def test_quadrotor_recurrent_replay_identity(H, D):
    env, res = qr._replay_identity(_quadrotor_make(D), qr._reset(), SC.quadrotor_recurrent((H, D)), _ids(), steps=T)
    assert res.obs.shape == (T, N, D) and res.state.h.shape == (N, H)
    _two_distinct(res.actions, (H, D))
    _clamp_acts_somewhere_and_not_everywhere(res.state.h, ("quadrotor recurrent", H, D))


@pytest.mark.parametrize("H", SC.QUADROTOR_MLP_ADDED)
def test_quadrotor_mlp_replay_identity(H):
    """H = 256 stages 1 537 16-byte pieces through the 64-lane copy loop into 24 592 bytes of dynamic LDS."""
    pol = SC.quadrotor_mlp(H)
    assert pol.param_count * 4 == 16 + 96 * H
    env, res = qm._replay_identity(lambda: qm._env(), qm._reset(), pol, _ids(), steps=T)
    _two_distinct(res.actions, H)


@pytest.mark.parametrize("view_grid,H", SC.MAZE_ADDED)
def test_maze_replay_identity(view_grid, H):
    env = mz.make_env(N, "SURVIVAL" if H % 2 else "ESCAPE", True, view_grid)
    pol = SC.maze_policy((view_grid, H))
    res, _ = mz.check_replay_identity(env, pol, _ids(), T, what=(view_grid, H))
    print("actions", np.bincount(res.actions.cpu().numpy().ravel(), minlength=4))
    _two_distinct(res.actions, (view_grid, H))
    _clamp_acts_somewhere_and_not_everywhere(res.state.h, ("maze", view_grid, H))


def _bandits_start(K, H):
    """A batch and its host mirror with the streams at different positions, the policy set, the ids, a fresh carry."""
    env, host = bd.make_env(N, K, 7, "Classical" if K % 2 else "Uniform", pre_steps=(5 * np.arange(N)) % 23, seed0=2000 + K)
    return env, host, SC.bandits_policy((K, H)), _ids(), bd.BanditPolicyState.zeros(N, H, DEV)


@pytest.mark.parametrize("K,H", SC.BANDITS_ADDED)
def test_bandits_closed_loop_oracle_and_replay(K, H):
    """max_steps = 7 and T = 12: every env ends an episode, and draws its next task, inside the launch."""
    env, host, pol, ids, state0 = _bandits_start(K, H)
    before, sd0 = state0.clone(), env.state_dict()
    res = env.rollout_policy(pol, T, policy_ids=ids, state=state0, record=True)
    bd.same_carry(state0, before, "the carry handed in is not written")
    rec, out, carry, _ = bd.host_rollout(pol, ids, host, before, T, True, True)
    bd.check_against_host(res, env, rec, out, carry, host, (K, H))
    assert rec["done"].sum(0).min() >= 1 and not rec["invalid"].any()
    # the recorded actions through rollout() from the same snapshot
    sd1 = env.state_dict()
    env.load_state_dict(sd0)
    reward, done, info = env.rollout(res.actions)
    assert torch.equal(reward.view(torch.int32), res.reward.view(torch.int32)) and torch.equal(done, res.done)
    assert torch.equal(info["steps"], res.info_steps) and torch.equal(info["invalid"], res.invalid)
    assert torch.equal(info["expected_gain"].view(torch.int64), res.expected_gain.view(torch.int64))
    bd.same_sd(env.state_dict(), sd1, (K, H))
    print("arms used", int((np.bincount(rec["actions"].ravel(), minlength=K) > 0).sum()), "of", K)
    _two_distinct(res.actions, (K, H))
    _clamp_acts_somewhere_and_not_everywhere(res.state.h, ("bandits", K, H))


@pytest.mark.parametrize("F,E,H", SC.LIFTSIM_ADDED)
def test_liftsim_closed_loop_oracle_replay_and_reference_loop(F, E, H):
    """Every added size fits a workgroup's LDS with its policy staged (policy_size_cases.liftsim_stages_the_policy, the sum of
    lp_lds_layout; the env does not expose the route), so lanes 0..63, on one id, read the staged copy and the other waves,
    whose ids are mixed, read global memory."""
    assert SC.liftsim_stages_the_policy((F, E, H))
    case, pol, ids = SC.liftsim_case((F, E, H)), SC.liftsim_policy((F, E, H)), _ids()
    sample, steps = list(case["sample"]), case["steps"]
    run = PC.run_closed_loop(case, pol, ids[sample])
    env, twin, loop = ls._env(case), ls._env(case), ls._env(case)
    out = env.rollout_policy(pol, steps, policy_ids=ids, record=ls.ALL)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got["actions"].shape == (steps, N, 2 * E)
    assert got["actions"][:, sample].tolist() == run["actions"].tolist()
    assert got["reward"][:, sample].tolist() == run["rows"][:, :, 0].tolist()
    assert got["time_consume"][:, sample].tolist() == run["rows"][:, :, 1].tolist()
    assert got["energy_consume"][:, sample].tolist() == run["rows"][:, :, 2].tolist()
    assert got["given_up_persons"][:, sample].tolist() == run["rows"][:, :, 3].astype(np.int64).tolist()
    assert got["return"].tolist() == ls._ordered_sum(got["reward"]).tolist()
    for j, e in enumerate(sample):
        assert env.mansion_state(e) == run["states"][j], e
    # the recorded actions through rollout(), and the reference loop on the device for all N envs
    rep = twin.rollout(out["actions"], record=ls.ALL[:4])
    for k in ls.ALL[:4]:
        assert torch.equal(rep[k], out[k]), k
    assert torch.equal(rep["return"], out["return"]) and torch.equal(twin.arena, env.arena)
    ls._reference_loop(loop, pol, ids, steps)
    assert torch.equal(loop.arena, env.arena)
    ls._no_flags(env)
    print("choices taken", len(run["choices"]), "of", 2 * F + 2)
    assert len(run["choices"]) >= 2 and len(np.unique(got["actions"].reshape(-1, 2 * E), axis=0)) >= 2


def _walker_ids():
    return [int(v) for v in np.arange(SC.WALKER_N) % P]


@pytest.mark.parametrize("robot,H", SC.WALKER_RECURRENT_ADDED)
def test_walker_recurrent_closed_loop_is_the_definition(robot, H):
    """max_steps = 5 and T = 6: an episode ends at step 4 at the latest, and the step after it runs on a kept carry with pd = 1."""
    env, twin = wr._make(robot, SC.WALKER_N), wr._make(robot, SC.WALKER_N)
    assert env.obs_dim + env.n_joints + 2 == SC.N_IN[robot]
    pol, ids = SC.walker_policy((robot, H), True), _walker_ids()
    x0 = env._obs.clone()
    start = wr._fresh(env, H)
    start.h.uniform_(-1.0, 1.0, generator=torch.Generator(device=DEV).manual_seed(5))
    start.prev_action.fill_(0.25)
    start.prev_reward.fill_(-0.5)
    start.prev_done[1] = 1
    st = start.clone()
    res = env.rollout_policy(pol, SC.WALKER_T, ids, record=True, obs_every=1, state=st)
    assert res.state is st and res.actions.shape == (SC.WALKER_T, SC.WALKER_N, env.n_joints)
    for name in ("actions", "reward", "obs"):
        assert torch.isfinite(getattr(res, name)).all(), name
    assert bool(res.done.any())
    wr._assert_actions_and_carry_are_the_definition(pol, ids, x0, start, res, False)
    wr._assert_twin_rollout_reproduces(twin, env, res)
    wr._assert_returns_are_their_definitions(res)
    _two_distinct(res.actions, (robot, H))
    _clamp_acts_somewhere_and_not_everywhere(res.state.h, ("walker recurrent", robot, H))


@pytest.mark.parametrize("robot,H", SC.WALKER_MLP_ADDED)
def test_walker_mlp_closed_loop_is_the_definition(robot, H):
    env, twin = wm._make(robot, SC.WALKER_N), wm._make(robot, SC.WALKER_N)
    pol, ids = SC.walker_policy((robot, H), False), _walker_ids()
    x0 = env._obs.clone()
    res = env.rollout_policy(pol, SC.WALKER_T, ids, record=True, obs_every=1)
    for name in ("actions", "reward", "obs"):
        assert torch.isfinite(getattr(res, name)).all(), name
    assert bool(res.done.any())
    wm._assert_actions_are_the_definition(pol, ids, x0, res)
    wm._assert_twin_rollout_reproduces(twin, env, res)
    wm._assert_returns_are_their_definitions(res)
    _two_distinct(res.actions, (robot, H))


# ---------------------------------------------------------------------------------------------- 2. poisoned padding
def _write_nan(params, pol, where):
    """A quiet NaN into the cached device copy, for all P policies: into every padding float (where = "padding"), or into the
    one real weight at index `where`, the positive control. Returns the device mask of the floats written."""
    assert tuple(params.shape) == (pol.num_policies, pol.param_count) and not bool(torch.isnan(params).any())
    mask = SC.padding_mask(pol)
    if where == "padding":
        assert mask.any()
    else:
        assert not mask[where]                                                # a float a weight maps to
        mask = np.zeros_like(mask)
        mask[where] = True
    at = torch.as_tensor(mask, device=params.device)
    if where == "padding":
        assert not bool(params[:, at].view(torch.int32).any())                # +0 before
    params[:, at] = float("nan")
    return at


def _launch_read_the_poisoned_copy(again, params, at):
    """After the launch: the env asked the policy for its device copy and got the very tensor that was written, NaNs in place."""
    assert again is params and again.data_ptr() == params.data_ptr()
    assert bool(torch.isnan(params[:, at]).all()) and int(torch.isnan(params).sum()) == params.shape[0] * int(at.sum())


def _bitwise_equal(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        if x.dtype.is_floating_point:
            assert not bool(torch.isnan(x).any()), (what, k, "the clean run holds a NaN")
            as_int = torch.int32 if x.dtype == torch.float32 else torch.int64
            x, y = x.contiguous().view(as_int), y.contiguous().view(as_int)
        assert torch.equal(x, y), (what, k, "the poisoned padding reached the result")


def _check(run, control, what):
    """run(where) -> the launch's outputs. Poisoned padding changes no bit; a NaN in one real weight (`control`: its index, or
    None for no control) changes the actions, so the launch does read the tensor the test writes."""
    clean = run(None)
    _bitwise_equal(clean, run("padding"), what)
    if control is not None:
        assert not torch.equal(clean["actions"], run(control)["actions"]), (what, "a NaN in a weight changed nothing")


def _tensors(prefix, obj, names):
    return {prefix + k: getattr(obj, k).clone() for k in names}


def _quadrotor_run(make_policy, D, where):
    env, pol = _quadrotor_make(D)(), make_policy()
    env.reset(seed=3)
    params = pol.to(DEV)
    at = None if where is None else _write_nan(params, pol, where)
    recurrent = hasattr(pol, "wh")
    res = env.rollout_policy(pol, T, _ids(), record=True, **(dict(state=qr._fresh(N, pol.hidden)) if recurrent else {}))
    if at is not None:
        _launch_read_the_poisoned_copy(pol.to(env.device), params, at)
    out = _tensors("", res, qr.RECORDS + qr.RETURNS)
    if recurrent:
        out.update(_tensors("carry.", res.state, qr.CARRY))
    out.update({"env." + k: v.clone() for k, v in env.state_dict().items() if torch.is_tensor(v)})
    return out


@pytest.mark.parametrize("H", SC.QUADROTOR_MLP_ADDED)
def test_poisoned_padding_quadrotor_mlp(H):
    """D = 16: three padding floats per record, loaded with the 16-byte reads of w[16..19] and never used. The control is b1
    of unit 0 (float 4 + 16): its pre-activation becomes NaN and its h +0, so no NaN reaches the step."""
    _check(lambda where: _quadrotor_run(lambda: SC.quadrotor_mlp(H), 16, where), 4 + 16, ("quadrotor mlp", H))


@pytest.mark.parametrize("H,D", [(35, 16), (39, 19)])
def test_poisoned_padding_quadrotor_recurrent(H, D):
    """The fourth float of (b, wr, wd, 0), the partial quad's v.w behind wh, and at D = 19 the float behind wx. No control
    here: every weight of this form reaches the voltages, and a NaN voltage is not an input the step is pinned at."""
    assert (H, D) in SC.QUADROTOR_RECURRENT_ADDED
    _check(lambda where: _quadrotor_run(lambda: SC.quadrotor_recurrent((H, D)), D, where), None, ("quadrotor recurrent", H, D))


def _carry_tensors(state):
    return {"carry." + k: getattr(state, k).clone() for k in ("h", "prev_action", "prev_reward", "prev_done")}


@pytest.mark.parametrize("view_grid,H", [(1, 2), (1, 7)])
def test_poisoned_padding_maze(view_grid, H):
    """The control is bo[0] (float 0): logit 0 is NaN, nothing compares greater, the move is 0."""
    assert (view_grid, H) in SC.MAZE_ADDED

    def run(where):
        env = mz.make_env(N, "SURVIVAL", True, view_grid)
        pol = SC.maze_policy((view_grid, H))
        params = pol.to(DEV)[0]
        at = None if where is None else _write_nan(params, pol, where)
        res = env.rollout_policy(pol, T, policy_ids=_ids(), seed=0, record=True, obs_every=1)
        if at is not None:
            _launch_read_the_poisoned_copy(pol.to(env.device)[0], params, at)
        out = _tensors("", res, ("actions", "reward", "reward64", "done", "obs", "ret_total", "ret_episode", "episode_len", "episodes"))
        out.update(_carry_tensors(res.state))
        out.update({"env." + k: v.clone() for k, v in env.state_dict().items() if torch.is_tensor(v)})
        return out

    _check(run, 0, ("maze", view_grid, H))


@pytest.mark.parametrize("K,H", [(5, 2), (63, 7)])
def test_poisoned_padding_bandits(K, H):
    """K % 4 = 1 and 3: the lookup r[4 + prev_action] of the last arm sits next to the wa padding. The control is bo[0], the
    first float behind the H unit records: logit 0 is NaN and arm 0 is played."""
    assert (K, H) in SC.BANDITS_ADDED

    def run(where):
        env, _, pol, ids, state0 = _bandits_start(K, H)
        params = pol.to(DEV)[0]
        at = None if where is None else _write_nan(params, pol, where)
        res = env.rollout_policy(pol, T, policy_ids=ids, state=state0, seed=0, record=True)
        if at is not None:
            _launch_read_the_poisoned_copy(pol.to(env.device)[0], params, at)
        out = _tensors("", res, bd.RECORDS + bd.RESULTS)
        out.update(_carry_tensors(res.state))
        out.update({"env." + k: v.clone() for k, v in env.state_dict().items() if torch.is_tensor(v)})
        return out

    _check(run, H * (4 + SC._pad4(K) + SC._pad4(H)), ("bandits", K, H))


@pytest.mark.parametrize("F,E,H", [(5, 2, 2), (7, 3, 3)])
def test_poisoned_padding_liftsim(F, E, H):
    """The control is bo[0], the first float behind the H unit records: logit 0 is NaN and every elevator takes choice 0."""
    assert (F, E, H) in SC.LIFTSIM_ADDED
    case = SC.liftsim_case((F, E, H))

    def run(where):
        env, pol = ls._env(case), SC.liftsim_policy((F, E, H))
        params = pol.to(env.device)
        at = None if where is None else _write_nan(params, pol, where)
        out = dict(env.rollout_policy(pol, case["steps"], policy_ids=_ids(), record=ls.ALL))
        if at is not None:
            _launch_read_the_poisoned_copy(pol.to(env.device), params, at)
        out["arena"] = env.arena.clone()
        ls._no_flags(env)
        return out

    _check(run, H * (12 + SC._pad4(E) + SC._pad4(F + 1) + 3 * SC._pad4(F)), ("liftsim", F, E, H))
