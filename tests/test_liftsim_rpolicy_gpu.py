"""LiftSim recurrent dispatchers on the GPU: mg_liftsim_rpolicy_rollout (LiftSim.rollout_policy with a LiftRecurrentPolicy)
against the oracle stepped with LiftRecurrentPolicy.reference, against the replay of its own recorded actions, and against
the reference loop on the device. All comparisons are exact: the actions, the records, the arena and the carry's bits."""
import os
import sys

import numpy as np
import pytest

import liftsim_cases as LC
import liftsim_policy_cases as PC
import liftsim_rpolicy_cases as RC

pytestmark = pytest.mark.gpu

ALL = ("reward", "time_consume", "energy_consume", "given_up_persons", "actions")


def _env(case, **kw):
    from metagym_amd.liftsim import LiftSim
    args = dict(case["kw"])
    if case.get("flow") is not None:
        args["flow"] = case["flow"]
    args.update(kw)
    return LiftSim(num_envs=case["N"], seed=case["seed"], **args)


def _no_flags(env):
    assert not env.overflow.any() and not env.unsupported.any() and not env.invalid.any()


def _ordered_sum(reward):
    acc = np.zeros(reward.shape[1])
    for t in range(reward.shape[0]):
        acc = acc + reward[t]
    return acc


def _same_carry(a, b):
    a, b = a.numpy(), b.numpy()
    return (a.h.tobytes() == b.h.tobytes() and a.prev_choice.tolist() == b.prev_choice.tolist()
            and a.prev_reward.tobytes() == b.prev_reward.tobytes())


def _reference_loop(env, pol, ids, steps, carry=None):
    """`steps` steps of the reference on the device: the policy in numpy float32 on the env's observation and the numpy
    carry, then step(), then the reward into the carry. Returns the end carry."""
    from metagym_amd.liftsim import LiftPolicyState
    if carry is None:
        carry = LiftPolicyState.zeros(env.num_envs, env.E, pol.hidden)
    for _ in range(steps):
        a, carry = pol.reference(ids, env.observation(), carry)
        _, reward, _, _ = env.step(a)
        carry = carry.observed(reward)
    return carry


def _uniform3(H=7):
    case = RC.CASES["uniform3"]()
    assert case["H"] == 7
    return case, RC.policies(10, 4, H), RC.case_ids(case)


# ---------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("name", ["f2_n1", "f2_n65", "uniform3", "custom_rush", "big"])
def test_rollout_policy_matches_the_oracle_closed_loop(name):
    import torch
    from metagym_amd.liftsim import LiftPolicyState
    run = RC.closed_loop(name)
    case, pol = run["case"], run["policy"]
    sample, T, E, N = list(case["sample"]), case["steps"], pol.elevators, case["N"]
    env = _env(case)
    ids = RC.case_ids(case)
    assert ids[sample].tolist() == run["ids"].tolist()
    out = env.rollout_policy(pol, T, policy_ids=ids, record=ALL)
    assert sorted(out) == sorted(ALL + ("return", "state"))
    state = out.pop("state")
    assert isinstance(state, LiftPolicyState) and state.device == env.device
    # the [N, ...] attributes are views of storage with the env index fastest
    assert tuple(state.h.shape) == (N, E, pol.hidden) and state.h.permute(1, 2, 0).is_contiguous()
    assert tuple(state.prev_choice.shape) == (N, E) and state.prev_choice.t().is_contiguous()
    assert state.h.dtype == torch.float32 and state.prev_choice.dtype == torch.int32 and state.prev_reward.dtype == torch.float32
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert out["actions"].shape == (T, N, 2 * E) and out["actions"].dtype == np.int32
    assert out["actions"][:, sample].tolist() == run["actions"].tolist()
    assert out["reward"][:, sample].tolist() == run["rows"][:, :, 0].tolist()
    assert out["time_consume"][:, sample].tolist() == run["rows"][:, :, 1].tolist()
    assert out["energy_consume"][:, sample].tolist() == run["rows"][:, :, 2].tolist()
    assert out["given_up_persons"][:, sample].tolist() == run["rows"][:, :, 3].astype(np.int64).tolist()
    assert out["return"].tolist() == _ordered_sum(out["reward"]).tolist()
    for j, e in enumerate(sample):
        assert env.mansion_state(e) == run["states"][j], e
        py_key, py_pos, np_key, np_pos = run["streams"][j]
        py = env.random_state(e)
        assert list(py[1][:624]) == py_key.tolist() and py[1][624] == py_pos, e
        st = env.numpy_state(e)
        assert st[1].tolist() == np_key.tolist() and st[2] == np_pos, e
    got, want = state.numpy(), run["carry"]
    assert got.h.flags["C_CONTIGUOUS"] and got.h.shape == (N, E, pol.hidden)
    assert got.h[sample].tobytes() == want.h.tobytes()
    assert got.prev_choice[sample].tolist() == want.prev_choice.tolist()
    assert got.prev_reward[sample].tobytes() == want.prev_reward.tobytes()
    assert got.prev_reward.tobytes() == out["reward"][-1].astype(np.float32).tobytes()
    _no_flags(env)


# ---------------------------------------------------------------------------------------------- 2. the replay
def test_replaying_the_recorded_actions_reproduces_every_record_and_the_arena():
    import torch
    case, pol, ids = _uniform3()
    T = 60
    env, again, loop, bare = _env(case), _env(case), _env(case), _env(case)
    out = env.rollout_policy(pol, T, policy_ids=ids, record=ALL)
    rep = again.rollout(out["actions"], record=ALL[:4])
    for k in ALL[:4]:
        assert torch.equal(rep[k], out[k]), k
    assert torch.equal(rep["return"], out["return"]) and torch.equal(again.arena, env.arena)
    for t in range(T):
        loop.step(out["actions"][t])
        assert torch.equal(loop.reward, out["reward"][t]) and torch.equal(loop.time_consume, out["time_consume"][t])
        assert torch.equal(loop.energy_consume, out["energy_consume"][t])
        assert torch.equal(loop.given_up_persons, out["given_up_persons"][t])
    assert torch.equal(loop.arena, env.arena)
    none = bare.rollout_policy(pol, T, policy_ids=ids)          # records on and off change neither the arena nor the carry
    assert sorted(none) == ["return", "state"]
    assert torch.equal(bare.arena, env.arena) and torch.equal(none["return"], out["return"])
    assert _same_carry(none["state"], out["state"])
    _no_flags(env)


# ---------------------------------------------------------------------------------------------- 3. staging does not change bits
@pytest.mark.parametrize("ids_kind", ["one_id", "mixed_ids"])
def test_staged_and_global_weights_match_the_reference_loop(ids_kind):
    import torch
    case, pol, ids = _uniform3()
    N = case["N"]
    if ids_kind == "one_id":
        ids = np.full(N, 4, np.int32)                                # every wave stages policy 4
    else:
        for w in range(0, N, 64):
            assert len(set(ids[w:w + 64].tolist())) > 1              # mixed inside every wave: global reads
    env, loop = _env(case), _env(case)
    out = env.rollout_policy(pol, 60, policy_ids=ids)
    carry = _reference_loop(loop, pol, ids, 60)
    assert torch.equal(env.arena, loop.arena) and _same_carry(out["state"], carry)
    assert (out["return"] < 0).all()
    _no_flags(env)


def test_a_policy_too_large_to_stage_matches_the_reference_loop():
    import torch
    from metagym_amd.liftsim import LiftRecurrentPolicy
    F, E, H, N = 128, 32, 64, 5
    pol = LiftRecurrentPolicy(**RC.random_weights(np.random.RandomState(8), 2, H, F, E, 0.25))
    assert pol.param_count * 4 > 160 * 1024                       # the parameters alone pass a workgroup's LDS
    case = dict(kw=dict(generator="UNIFORM", floors=F, elevators=E, **LC.BIG_KW), N=N, seed=LC.BIG_SEED)
    ids = np.ones(N, np.int32)                                    # one id in the wave, and still no room to stage it
    env, loop = _env(case), _env(case)
    out = env.rollout_policy(pol, 40, policy_ids=ids, record=("actions",))
    carry = _reference_loop(loop, pol, ids, 40)
    assert torch.equal(env.arena, loop.arena) and _same_carry(out["state"], carry)
    assert len(np.unique(out["actions"].cpu().numpy()[:, :, 0::2])) > 4
    _no_flags(env)


# ---------------------------------------------------------------------------------------------- 4. calls continue one another
def test_two_calls_through_one_state_equal_one_and_a_step_in_between_is_not_seen():
    import torch
    from metagym_amd.liftsim import LiftPolicyState
    case, pol, ids = _uniform3()
    N, T1, T2 = case["N"], 37, 23
    one, two = _env(case), _env(case)
    whole = one.rollout_policy(pol, T1 + T2, policy_ids=ids, record=ALL)            # state=None: a fresh carry
    state = LiftPolicyState.zeros(N, 4, pol.hidden, two.device)
    first = two.rollout_policy(pol, T1, policy_ids=ids, record=ALL, state=state)
    assert first["state"] is state
    second = two.rollout_policy(pol, T2, policy_ids=ids, record=ALL, state=state)
    assert second["state"] is state
    assert torch.equal(one.arena, two.arena) and _same_carry(whole["state"], state)
    for k in ALL:
        assert torch.equal(torch.cat([first[k], second[k]]), whole[k]), k
    rew = whole["reward"].cpu().numpy()
    assert first["return"].cpu().numpy().tolist() == _ordered_sum(rew[:T1]).tolist()
    assert second["return"].cpu().numpy().tolist() == _ordered_sum(rew[T1:]).tolist()
    # a step() between two launches: the reference loop with that step in its place, the carry (its pr too) left alone
    mixed, loop = _env(case), _env(case)
    a = torch.from_numpy(LC.random_actions(77, 2, N, 10, 4)[1]).to(mixed.device)
    st = mixed.rollout_policy(pol, T1, policy_ids=ids)["state"]
    kept = st.clone()
    mixed.step(a)
    assert _same_carry(st, kept)
    mixed.rollout_policy(pol, T2, policy_ids=ids, state=st)
    carry = _reference_loop(loop, pol, ids, T1)
    loop.step(a)
    carry = _reference_loop(loop, pol, ids, T2, carry)
    assert torch.equal(mixed.arena, loop.arena) and _same_carry(st, carry)
    assert not _same_carry(st, kept)
    _no_flags(mixed)


# ---------------------------------------------------------------------------------------------- 5. hidden sizes
@pytest.mark.parametrize("H", [1, 3, 4, 5, 63, 64])
def test_every_hidden_size_path_matches_the_reference_loop(H):
    import torch
    case = dict(kw=dict(generator="UNIFORM", **PC.CONF[3]), N=65, seed=40)
    pol = RC.policies(10, 4, H, sigma=0.5 if H < 60 else 0.25)
    ids = ((7 * np.arange(65) + 3) % RC.N_POLICIES).astype(np.int32)
    env, loop = _env(case), _env(case)
    out = env.rollout_policy(pol, 20, policy_ids=ids)
    carry = _reference_loop(loop, pol, ids, 20)
    assert torch.equal(env.arena, loop.arena) and _same_carry(out["state"], carry)
    _no_flags(env)


# ---------------------------------------------------------------------------------------------- 6. poisoned padding
def test_nan_in_every_padding_float_changes_nothing():
    import torch
    from metagym_amd.liftsim import LiftRecurrentPolicy
    from metagym_amd.liftsim import policy as LP
    case, pol, ids = _uniform3()
    H, F, E, A = pol.hidden, 10, 4, 22
    poisoned = LiftRecurrentPolicy(**{name: getattr(pol, name) for name in RC.NAMES})
    groups, ru = LP.recurrent_unit_groups(H, F, E)
    rc = 4 + ((H + 3) & ~3)
    used = np.zeros(pol.param_count, bool)
    for j in range(H):
        for _, o, n in groups:
            used[j * ru + o:j * ru + o + n] = True
    for c in range(A):
        used[H * ru + c * rc] = True
        used[H * ru + c * rc + 4:H * ru + c * rc + 4 + H] = True
    assert (~used).sum() == H * (2 + 1 + 2 * 3 + 2 + 1) + A * (3 + 1)          # wt 11, wr wu wd 10, wc 22, wh 7; wo 7
    dev = poisoned.to("cuda")
    dev[:, torch.from_numpy(~used).to(dev.device)] = float("nan")
    assert poisoned.to("cuda") is dev and int(torch.isnan(dev).sum()) == 6 * int((~used).sum())
    for kind in ("one_id", "mixed_ids"):
        use = np.full(case["N"], 2, np.int32) if kind == "one_id" else ids
        clean, dirty = _env(case), _env(case)
        want = clean.rollout_policy(pol, 40, policy_ids=use, record=ALL)
        got = dirty.rollout_policy(poisoned, 40, policy_ids=use, record=ALL)
        for k in ALL + ("return",):
            assert torch.equal(got[k], want[k]), (kind, k)
        assert torch.equal(dirty.arena, clean.arena) and _same_carry(got["state"], want["state"]), kind


# ---------------------------------------------------------------------------------------------- 7. a frozen env
def test_an_overflowing_env_freezes_alone_and_keeps_the_carry_of_its_last_step():
    c, run = RC.FROZEN, RC.frozen_run()
    pol, T, N = run["policy"], c["steps"], c["N"]
    case = dict(kw=c["kw"], N=N, seed=c["seed"])
    ids = (np.arange(N) % RC.N_POLICIES).astype(np.int32)
    small, twin = _env(case, queue_capacity=c["Q"]), _env(case)
    out = small.rollout_policy(pol, T, policy_ids=ids, record=ALL)
    end = out.pop("state").numpy()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    flagged = small.overflow.cpu().numpy().astype(bool)
    assert 0 < flagged.sum() < N and not small.unsupported.any() and not small.invalid.any()
    first = {int(e): int(np.nonzero(out["reward"][:, e] == 0)[0][0]) for e in np.nonzero(flagged)[0]}   # a step that ran: reward < 0
    for j, e in enumerate(c["sample"]):                           # the oracle says who overflows, and in which step
        assert flagged[e] == (run["first"][j] >= 0), e
        if flagged[e]:
            assert first[e] == run["first"][j], e
        upto = T if not flagged[e] else first[e]
        assert out["actions"][:upto + 1, e].tolist() == run["actions"][:upto + 1, j].tolist()
        assert out["reward"][:upto, e].tolist() == run["rows"][:upto, j, 0].tolist()
    # the unfrozen twin (default capacity), stopped after first + 1 steps for every first that occurs, and at T
    stops = sorted(set(f + 1 for f in first.values()) | {T})
    assert 0 < stops[0] and stops[-1] == T
    state, done, at, parts = None, 0, {}, []
    for stop in stops:
        part = twin.rollout_policy(pol, stop - done, policy_ids=ids, record=ALL, state=state)
        state, done = part.pop("state"), stop
        at[stop] = state.numpy()
        parts.append({k: v.cpu().numpy() for k, v in part.items()})
    assert not twin.overflow.any() and not twin.unsupported.any()
    ref = {k: np.concatenate([p[k] for p in parts]) for k in ALL}
    for e in range(N):
        if flagged[e]:
            f = first[e]
            for k in ALL[:4]:
                assert not out[k][f:, e].any(), (k, e)             # zero outputs from the freeze on
                assert out[k][:f, e].tolist() == ref[k][:f, e].tolist(), (k, e)
            # the step that overflowed still ran the policy; from the next one on (0, 0) per elevator
            assert out["actions"][:f + 1, e].tolist() == ref["actions"][:f + 1, e].tolist()
            assert not out["actions"][f + 1:, e].any()
            assert end.h[e].tobytes() == at[f + 1].h[e].tobytes(), e
            assert end.prev_choice[e].tolist() == at[f + 1].prev_choice[e].tolist(), e
            assert end.prev_reward[e] == 0 and at[f + 1].prev_reward[e] < 0, e
            continue
        for k in ALL:
            assert out[k][:, e].tolist() == ref[k][:, e].tolist(), (k, e)
        assert end.h[e].tobytes() == at[T].h[e].tobytes() and end.prev_choice[e].tolist() == at[T].prev_choice[e].tolist()
        assert end.prev_reward[e] == at[T].prev_reward[e]
        assert small.mansion_state(e) == twin.mansion_state(e)
        assert small.random_state(e) == twin.random_state(e)


# ---------------------------------------------------------------------------------------------- 8. refused calls
def test_a_refused_call_raises_and_leaves_the_arena_and_the_state_untouched():
    import torch
    from metagym_amd.liftsim import LiftPolicy, LiftPolicyState
    from metagym_amd.metamaze.policy import MazePolicyState
    case, pol, ids = _uniform3()
    N, E, H = case["N"], 4, pol.hidden
    env = _env(case)
    state = env.rollout_policy(pol, 5)["state"]                   # policy_ids=None: policy 0 for all
    before, kept = env.arena.clone(), state.clone()
    dev = env.device
    with pytest.raises(TypeError):
        env.rollout_policy(pol, 5, state=MazePolicyState.zeros(N, H, dev))         # a state of another class
    with pytest.raises(TypeError):
        env.rollout_policy(pol, 5, state=(state.h, state.prev_choice, state.prev_reward))
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, state=LiftPolicyState.zeros(N, E, H))           # a numpy carry
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, state=LiftPolicyState.zeros(N, E, H, "cpu"))    # another device
    for shape in ((N + 1, E, H), (N, E, H + 1), (N, E - 1, H)):
        with pytest.raises(ValueError):
            env.rollout_policy(pol, 5, state=LiftPolicyState.zeros(*shape, dev))
    good = lambda: LiftPolicyState.zeros(N, E, H, dev)
    for field, bad in (("h", good().h.double()), ("prev_choice", good().prev_choice.long()),
                       ("prev_reward", good().prev_reward.double()),
                       ("h", torch.zeros(N, E, H, device=dev)),                    # [N][E][H] storage: not env index fastest
                       ("prev_choice", torch.full((N, E), -1, dtype=torch.int32, device=dev))):
        s = good()
        setattr(s, field, bad)
        with pytest.raises(ValueError):
            env.rollout_policy(pol, 5, state=s)
    with pytest.raises(ValueError):
        env.rollout_policy(RC.policies(11, 4, H), 5, state=state)                  # another F
    with pytest.raises(ValueError):
        env.rollout_policy(RC.policies(10, 5, H), 5, state=state)                  # another E
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, policy_ids=np.full(N, 6), state=state)          # an id out of range
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, policy_ids=np.full(N, -1), state=state)
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, policy_ids=np.zeros(N + 1, np.int64), state=state)
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 0, state=state)
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, record=("observations",), state=state)
    # the feed-forward policy takes no state, and without one answers with the keys it always had
    mlp = LiftPolicy(pol.ws, pol.we, pol.wt, pol.wr, pol.wu, pol.wd, pol.b, pol.wo, pol.bo)
    with pytest.raises(ValueError):
        env.rollout_policy(mlp, 5, state=state)
    torch.cuda.synchronize()
    assert torch.equal(env.arena, before) and _same_carry(state, kept)
    out = env.rollout_policy(mlp, 5, record=("reward",))
    assert sorted(out) == ["return", "reward"]
    assert _same_carry(state, kept)


# ---------------------------------------------------------------------------------------------- 9. one hipGraph capture
def test_graph_capture_of_a_recurrent_rollout_replays_like_eager():
    import torch
    from metagym_amd.liftsim import LiftPolicyState
    case, pol, _ = _uniform3()
    eager, graphed = _env(case), _env(case)
    ids = torch.from_numpy(RC.case_ids(case)).to(eager.device)
    T = 30
    se, sg = (LiftPolicyState.zeros(case["N"], 4, pol.hidden, eager.device) for _ in range(2))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        graphed.rollout_policy(pol, T, policy_ids=ids, state=sg)  # warm-up on a side stream: uploads the policy and the ids
    torch.cuda.current_stream().wait_stream(s)
    eager.rollout_policy(pol, T, policy_ids=ids, state=se)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = graphed.rollout_policy(pol, T, policy_ids=ids, record=("reward", "actions"), state=sg)
    assert out["state"] is sg
    for k in range(4):
        g.replay()
        want = eager.rollout_policy(pol, T, policy_ids=ids, record=("reward", "actions"), state=se)
        torch.cuda.synchronize()
        assert torch.equal(out["return"], want["return"]) and torch.equal(out["reward"], want["reward"])
        assert torch.equal(out["actions"], want["actions"])
        assert _same_carry(sg, se)
    assert torch.equal(graphed.arena, eager.arena)
    _no_flags(eager)


# ---------------------------------------------------------------------------------------------- 10. the example
def test_the_recurrent_search_example_runs_two_generations(capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    try:
        import liftsim_recurrent_search
    finally:
        sys.path.pop(0)
    res = liftsim_recurrent_search.main(["--candidates", "4", "--seeds", "8", "--steps", "40", "--generations", "2", "--hidden", "4"])
    text = capsys.readouterr().out
    assert text.count("generation") == 2 and "rule dispatcher" in text and "MLP search" in text
    assert len(res["history"]) == 2 and res["rule"] < 0 and all(p < 0 and b < 0 and b >= p for p, b in res["history"])
    assert len(res["mlp_history"]) == 2 and all(b < 0 for _, b in res["mlp_history"])
