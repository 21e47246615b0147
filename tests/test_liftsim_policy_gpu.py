"""LiftSim learned dispatchers on the GPU: mg_liftsim_policy_rollout (LiftSim.rollout_policy) against the oracle stepped with
LiftPolicy.reference, against the replay of its own recorded actions, and against the reference loop on the device. All
comparisons are exact."""
import os
import sys

import numpy as np
import pytest

import liftsim_cases as LC
import liftsim_policy_cases as PC

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


def _reference_loop(env, pol, ids, steps):
    """`steps` steps of the reference on the device: the policy in numpy float32 on the env's observation, then step()."""
    for _ in range(steps):
        env.step(pol.reference(ids, env.observation()))


# ---------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("name", ["uniform3", "big", "f2_n1", "f2_n65", "custom_rush"])
def test_rollout_policy_matches_the_oracle_closed_loop(name):
    run = PC.closed_loop(name)
    case, pol = run["case"], run["policy"]
    sample, T, E = list(case["sample"]), case["steps"], pol.elevators
    env = _env(case)
    ids = PC.case_ids(case)
    assert ids[sample].tolist() == run["ids"].tolist()
    out = env.rollout_policy(pol, T, policy_ids=ids, record=ALL)
    assert sorted(out) == sorted(ALL + ("return",))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert out["actions"].shape == (T, case["N"], 2 * E) and out["actions"].dtype == np.int32
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
    _no_flags(env)


# ---------------------------------------------------------------------------------------------- 2. the replay
def test_replaying_the_recorded_actions_reproduces_every_record_and_the_arena():
    import torch
    case = PC.CASES["uniform3"]()
    pol = PC.policies(10, 4, case["H"])
    ids = PC.case_ids(case)
    T, N = case["steps"], case["N"]
    env, again, loop, bare = _env(case), _env(case), _env(case), _env(case)
    for other in (again, loop, bare):
        assert torch.equal(other.arena, env.arena)
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
    assert out["return"].cpu().numpy().tolist() == _ordered_sum(out["reward"].cpu().numpy()).tolist()
    none = bare.rollout_policy(pol, T, policy_ids=ids)          # records on and off do not change the run
    assert sorted(none) == ["return"]
    assert torch.equal(bare.arena, env.arena) and torch.equal(none["return"], out["return"])
    a = out["actions"].cpu().numpy()
    assert a[:, :, 0::2].min() >= -1 and a[:, :, 0::2].max() <= 10 and set(np.unique(a[:, :, 1::2]).tolist()) == {-1, 1}
    _no_flags(env)


# ---------------------------------------------------------------------------------------------- 3. staging does not change bits
@pytest.mark.parametrize("ids_kind", ["one_id", "mixed_ids"])
def test_staged_and_global_weights_match_the_reference_loop(ids_kind):
    import torch
    case = PC.CASES["uniform3"]()
    pol = PC.policies(10, 4, case["H"])
    N = case["N"]
    ids = np.full(N, 4, np.int32) if ids_kind == "one_id" else PC.case_ids(case)     # one id: every wave stages policy 4
    if ids_kind == "mixed_ids":
        for w in range(0, N, 64):
            assert len(set(ids[w:w + 64].tolist())) > 1                            # mixed inside every wave: global reads
    env, loop = _env(case), _env(case)
    out = env.rollout_policy(pol, 60, policy_ids=ids)
    _reference_loop(loop, pol, ids, 60)
    assert torch.equal(env.arena, loop.arena)
    assert (out["return"] < 0).all()
    _no_flags(env)


def test_a_policy_too_large_to_stage_matches_the_reference_loop():
    import torch
    from metagym_amd.liftsim import LiftPolicy
    F, E, H, N = 128, 32, 64, 5
    w = PC.random_weights(np.random.RandomState(8), 2, H, F, E)
    pol = LiftPolicy(*w)
    assert pol.param_count * 4 > 160 * 1024                       # the parameters alone pass a workgroup's LDS
    case = dict(kw=dict(generator="UNIFORM", floors=F, elevators=E, **LC.BIG_KW), N=N, seed=LC.BIG_SEED)
    ids = np.ones(N, np.int32)                                    # one id in the wave, and still no room to stage it
    env, loop = _env(case), _env(case)
    out = env.rollout_policy(pol, 60, policy_ids=ids, record=("actions",))
    _reference_loop(loop, pol, ids, 60)
    assert torch.equal(env.arena, loop.arena)
    assert len(np.unique(out["actions"].cpu().numpy()[:, :, 0::2])) > 4
    _no_flags(env)


# ---------------------------------------------------------------------------------------------- 4. calls continue one another
def test_two_calls_equal_one_and_a_step_in_between_continues():
    import torch
    case = PC.CASES["uniform3"]()
    pol = PC.policies(10, 4, case["H"])
    ids = PC.case_ids(case)
    T1, T2 = 37, 23
    one, two = _env(case), _env(case)
    whole = one.rollout_policy(pol, T1 + T2, policy_ids=ids, record=ALL)
    first = two.rollout_policy(pol, T1, policy_ids=ids, record=ALL)
    second = two.rollout_policy(pol, T2, policy_ids=ids, record=ALL)
    assert torch.equal(one.arena, two.arena)
    for k in ALL:
        assert torch.equal(torch.cat([first[k], second[k]]), whole[k]), k
    rew = whole["reward"].cpu().numpy()
    assert first["return"].cpu().numpy().tolist() == _ordered_sum(rew[:T1]).tolist()
    assert second["return"].cpu().numpy().tolist() == _ordered_sum(rew[T1:]).tolist()
    # a step() between two launches: the same as the reference loop with that step in its place
    mixed, loop = _env(case), _env(case)
    a = torch.from_numpy(LC.random_actions(77, 2, case["N"], 10, 4)[1]).to(mixed.device)
    mixed.rollout_policy(pol, T1, policy_ids=ids)
    mixed.step(a)
    mixed.rollout_policy(pol, T2, policy_ids=ids)
    _reference_loop(loop, pol, ids, T1)
    loop.step(a)
    _reference_loop(loop, pol, ids, T2)
    assert torch.equal(mixed.arena, loop.arena)
    assert not mixed.overflow.any() and not mixed.unsupported.any()


# ---------------------------------------------------------------------------------------------- 5. a frozen env
def test_an_overflowing_env_freezes_alone_and_records_zero_actions():
    c, run = PC.FROZEN, PC.frozen_run()
    pol, T, N = run["policy"], c["steps"], c["N"]
    case = dict(kw=c["kw"], N=N, seed=c["seed"])
    ids = (np.arange(N) % PC.N_POLICIES).astype(np.int32)
    small, big = _env(case, queue_capacity=c["Q"]), _env(case)
    out = small.rollout_policy(pol, T, policy_ids=ids, record=ALL)
    ref = big.rollout_policy(pol, T, policy_ids=ids, record=ALL)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    ref = {k: v.cpu().numpy() for k, v in ref.items()}
    flagged = small.overflow.cpu().numpy().astype(bool)
    assert 0 < flagged.sum() < N and not big.overflow.any() and not small.unsupported.any() and not small.invalid.any()
    for j, e in enumerate(c["sample"]):                           # the oracle says who overflows, and in which step
        first = run["first"][j]
        assert flagged[e] == (first >= 0), e
        upto = T if first < 0 else first
        assert out["actions"][:upto + 1, e].tolist() == run["actions"][:upto + 1, j].tolist()
        assert out["reward"][:upto, e].tolist() == run["rows"][:upto, j, 0].tolist()
        if first >= 0:
            assert int(np.nonzero(out["reward"][:, e] == 0)[0][0]) == first
    for e in range(N):
        if flagged[e]:
            first = int(np.nonzero(out["reward"][:, e] == 0)[0][0])   # a step that ran has a negative reward
            assert 0 < first < T - 1
            for k in ALL[:4]:
                assert not out[k][first:, e].any(), (k, e)         # zero outputs from the freeze on
                assert out[k][:first, e].tolist() == ref[k][:first, e].tolist(), (k, e)
            # the step that overflowed still records the policy's actions; from the next one on (0, 0) per elevator
            assert out["actions"][:first + 1, e].tolist() == ref["actions"][:first + 1, e].tolist()
            assert not out["actions"][first + 1:, e].any()
            assert out["return"][e] == _ordered_sum(out["reward"][:first, e][:, None])[0]
            continue
        for k in ALL:
            assert out[k][:, e].tolist() == ref[k][:, e].tolist(), (k, e)
        assert out["return"][e] == ref["return"][e]
        assert small.mansion_state(e) == big.mansion_state(e)
        assert small.statistics_of(e) == big.statistics_of(e)
        assert small.random_state(e) == big.random_state(e)


# ---------------------------------------------------------------------------------------------- 6. refused calls
def test_a_refused_call_raises_and_leaves_the_arena_untouched():
    import torch
    case = PC.CASES["uniform3"]()
    env = _env(case)
    pol = PC.policies(10, 4, 8)
    env.rollout_policy(pol, 5)                                    # policy_ids=None: policy 0 for all
    before = env.arena.clone()
    N = case["N"]
    with pytest.raises(ValueError):
        env.rollout_policy(PC.policies(11, 4, 8), 5)              # another F
    with pytest.raises(ValueError):
        env.rollout_policy(PC.policies(10, 5, 8), 5)              # another E
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, policy_ids=np.full(N, 6))      # an id out of range
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, policy_ids=np.full(N, -1))
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, policy_ids=np.zeros(N + 1, np.int64))
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 0)
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, record=("observations",))
    with pytest.raises(TypeError):
        env.rollout_policy("rule", 5)
    torch.cuda.synchronize()
    assert torch.equal(env.arena, before)
    # policy_ids=None is all zeros
    a, b = _env(case), _env(case)
    a.rollout_policy(pol, 20)
    b.rollout_policy(pol, 20, policy_ids=torch.zeros(N, dtype=torch.int32))
    assert torch.equal(a.arena, b.arena)


# ---------------------------------------------------------------------------------------------- 7. one hipGraph capture
def test_graph_capture_of_a_policy_rollout_replays_like_eager():
    import torch
    case = PC.CASES["uniform3"]()
    pol = PC.policies(10, 4, 8)
    eager, graphed = _env(case), _env(case)
    ids = torch.from_numpy(PC.case_ids(case)).to(eager.device)
    T = 30
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        graphed.rollout_policy(pol, T, policy_ids=ids)            # warm-up on a side stream: uploads the policy and the ids
    torch.cuda.current_stream().wait_stream(s)
    eager.rollout_policy(pol, T, policy_ids=ids)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = graphed.rollout_policy(pol, T, policy_ids=ids, record=("reward", "actions"))
    for k in range(4):
        g.replay()
        want = eager.rollout_policy(pol, T, policy_ids=ids, record=("reward", "actions"))
        torch.cuda.synchronize()
        assert torch.equal(out["return"], want["return"]) and torch.equal(out["reward"], want["reward"])
        assert torch.equal(out["actions"], want["actions"])
    assert torch.equal(graphed.arena, eager.arena)
    _no_flags(eager)


# ---------------------------------------------------------------------------------------------- 8. the example
def test_the_search_example_runs_two_generations(capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    try:
        import liftsim_policy_search
    finally:
        sys.path.pop(0)
    res = liftsim_policy_search.main(["--candidates", "4", "--seeds", "8", "--steps", "40", "--generations", "2", "--hidden", "4"])
    text = capsys.readouterr().out
    assert text.count("generation") == 2 and "rule dispatcher" in text
    assert len(res["history"]) == 2 and res["rule"] < 0 and all(p < 0 and b < 0 and b >= p for p, b in res["history"])
