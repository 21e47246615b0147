"""metagym_amd/_policy.py on the CPU: the one `policy_ids` validator and its cache, the argument helpers, and the carry the
continuous-action recurrent policies share. The env is a stub (num_envs, device); nothing here needs a GPU."""
import re

import numpy as np
import pytest
import torch

from metagym_amd import _policy
from metagym_amd.metalocomotion.policy import WalkerPolicyState
from metagym_amd.quadrotor.policy import QuadrotorPolicyState

N, P = 5, 3
IDS = [2, 0, 1, 1, 2]


class _Env(object):
    def __init__(self, num_envs=N):
        self.num_envs, self.device = num_envs, torch.device("cpu")


# ---------------------------------------------------------------------------------------------- policy_ids
def test_policy_ids_defaults():
    ids = _policy.policy_ids(_Env(), None, P)
    assert ids.dtype == torch.int32 and ids.device.type == "cpu" and ids.is_contiguous()
    assert ids.tolist() == [0, 1, 2, 0, 1]
    assert _policy.policy_ids(_Env(), None, P, default="zero").tolist() == [0] * N
    with pytest.raises(ValueError):
        _policy.policy_ids(_Env(), None, P, default="first")
    env = _Env()
    first = _policy.policy_ids(env, None, P)
    keep = env._policy_ids_keep
    assert _policy.policy_ids(env, None, P) is first and env._policy_ids_keep is keep    # kept: no array is built again
    assert _policy.policy_ids(env, [0, 1, 2, 0, 1], P) is first                          # the same ids from the host
    assert _policy.policy_ids(env, None, P, default="zero").tolist() == [0] * N          # another rule is not the kept one
    assert _policy.policy_ids(env, None, P).tolist() == [0, 1, 2, 0, 1]


def test_policy_ids_same_ids_same_kept_tensor():
    """A host list, a numpy int64 array and a torch tensor with the same ids answer with one kept device tensor."""
    env = _Env()
    first = _policy.policy_ids(env, IDS, P)
    assert first.dtype == torch.int32 and first.tolist() == IDS
    assert _policy.policy_ids(env, IDS, P) is first
    assert _policy.policy_ids(env, np.array(IDS, np.int64), P) is first
    assert _policy.policy_ids(env, torch.tensor(IDS, dtype=torch.int32), P) is first
    assert _policy.policy_ids(env, torch.tensor(IDS, dtype=torch.int64), P) is first


def test_policy_ids_unchanged_tensor_is_not_converted_again():
    env, t = _Env(), torch.tensor(IDS, dtype=torch.int32)
    first = _policy.policy_ids(env, t, P)
    keep = env._policy_ids_keep
    assert keep[2] is t and keep[3] == t._version
    assert _policy.policy_ids(env, t, P) is first
    assert env._policy_ids_keep is keep                    # the fast path: nothing was read, compared or stored again


def test_policy_ids_version_bump_revalidates():
    env, t = _Env(), torch.tensor(IDS, dtype=torch.int32)
    first = _policy.policy_ids(env, t, P)
    version = t._version
    t.copy_(torch.tensor([0, 0, 1, 2, 2], dtype=torch.int32))
    assert t._version != version
    second = _policy.policy_ids(env, t, P)
    assert second is not first and second.tolist() == [0, 0, 1, 2, 2]
    assert env._policy_ids_keep[3] == t._version
    t[4] = P                                               # out of range: refused, and the kept entry is the last valid one
    with pytest.raises(ValueError, match=re.escape("policy_ids must be in [0, %d)" % P)):
        _policy.policy_ids(env, t, P)
    assert env._policy_ids_keep[1] is second
    assert _policy.policy_ids(env, [0, 0, 1, 2, 2], P) is second


def test_policy_ids_change_of_P_revalidates():
    env = _Env()
    t = torch.tensor(IDS, dtype=torch.int32)
    first = _policy.policy_ids(env, t, P)
    wider = _policy.policy_ids(env, t, P + 1)
    assert wider is not first and wider.tolist() == IDS and env._policy_ids_keep[0] == P + 1
    with pytest.raises(ValueError, match=re.escape("policy_ids must be in [0, 2)")):
        _policy.policy_ids(env, t, 2)                      # the same unchanged tensor, now out of range
    assert _policy.policy_ids(env, None, 2).tolist() == [0, 1, 0, 1, 0]


@pytest.mark.parametrize("name", ["policy_ids", "learner_ids"])
def test_policy_ids_refusals(name):
    env = _Env()
    cases = ((np.zeros(N + 1, np.int32), "%s must have shape (%d,), got (%d,)" % (name, N, N + 1)),
             (np.zeros((N, 1), np.int32), "%s must have shape (%d,), got (%d, 1)" % (name, N, N)),
             (np.zeros(N, np.float32), "%s must be integers, got float32" % name),
             (torch.zeros(N, dtype=torch.float64), "%s must be integers, got float64" % name),
             ([0, 1, -1, 0, 0], "%s must be in [0, %d)" % (name, P)),
             ([0, 1, P, 0, 0], "%s must be in [0, %d)" % (name, P)))
    for ids, message in cases:
        with pytest.raises(ValueError, match=re.escape(message)):
            _policy.policy_ids(env, ids, P, name=name)
    assert getattr(env, "_policy_ids_keep", None) is None  # a refused call keeps nothing
    assert _policy.policy_ids(_Env(0), np.zeros(0, np.int64), P).shape == (0,)            # no env: nothing to range-check


# ---------------------------------------------------------------------------------------------- the argument helpers
def test_f32_array():
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    out = _policy.f32_array("w", a.T, 2)                   # accepted, made contiguous
    assert out.flags.c_contiguous and out.dtype == np.float32 and np.array_equal(out, a.T)
    assert np.array_equal(_policy.f32_array("w", torch.from_numpy(a), 2), a)              # a torch tensor
    with pytest.raises(TypeError, match=re.escape("w must be float32, got float64")):
        _policy.f32_array("w", a.astype(np.float64), 2)
    with pytest.raises(ValueError, match=re.escape("w must have 3 dimensions, got shape (3, 4)")):
        _policy.f32_array("w", a, 3)
    for v in (np.inf, np.nan):
        bad = a.copy()
        bad[1, 2] = v
        with pytest.raises(ValueError, match="w holds a value that is not finite"):
            _policy.f32_array("w", bad, 2)


def test_check_epsilon():
    eps = _policy.check_epsilon(np.array([0.0, 0.25, 0.5, 1.0])[::2], 2)                  # accepted, made contiguous
    assert eps.dtype == np.float64 and eps.flags.c_contiguous and eps.tolist() == [0.0, 0.5]
    assert _policy.check_epsilon(torch.tensor([1.0], dtype=torch.float64), 1).tolist() == [1.0]
    with pytest.raises(TypeError, match=re.escape("epsilon must be float64, got float32")):
        _policy.check_epsilon(np.zeros(2, np.float32), 2)
    with pytest.raises(ValueError, match=re.escape("epsilon must have shape (2,), got (3,)")):
        _policy.check_epsilon(np.zeros(3), 2)
    for bad in (-1e-9, 1.0 + 1e-9, np.nan):
        with pytest.raises(ValueError, match=re.escape("epsilon must be in [0, 1]")):
            _policy.check_epsilon(np.array([0.5, bad]), 2)


def test_eps_threshold_keeps_the_shape():
    thr = _policy.eps_threshold(np.array([[0.0, 0.5], [1.0, 2.0 ** -32]]))
    assert thr.dtype == np.uint32 and thr.shape == (2, 2)
    assert [int(v) for v in thr.ravel()] == [0, 1 << 31, 0xFFFFFFFF, 1]                   # 1.0 is clamped to 2^32 - 1
    assert int(_policy.eps_threshold(0.25)) == 1 << 30 and _policy.eps_threshold(0.25).shape == ()


def test_pad4_and_moved_names():
    from metagym_amd.metamaze import policy as maze
    assert [_policy.pad4(n) for n in (0, 1, 4, 5, 63, 64)] == [0, 4, 4, 8, 64, 64]
    assert maze.philox4x32_10 is _policy.philox4x32_10 and maze.eps_threshold is _policy.eps_threshold


# ---------------------------------------------------------------------------------------------- the shared carry
def _numpy_carry(cls):
    """One numpy carry with N = 3, H = 2 and no zero in it; A = 4."""
    st = cls.zeros(3, 2) if cls is QuadrotorPolicyState else cls(3, 2, 4)
    st.h[:] = np.arange(1, 7, dtype=np.float32).reshape(3, 2)
    st.prev_action[:] = -np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    st.prev_reward[:] = [0.5, 1.5, 2.5]
    st.prev_done[:] = [1, 0, 1]
    return st


@pytest.mark.parametrize("cls", [QuadrotorPolicyState, WalkerPolicyState])
def test_shared_carry(cls):
    assert issubclass(cls, _policy.ContinuousPolicyState)
    assert cls.__slots__ == ("h", "prev_action", "prev_reward", "prev_done")
    st = _numpy_carry(cls)
    assert (st.num_envs, st.hidden, st.n_act, st.device) == (3, 2, 4, None)
    fields = cls.__slots__

    c = st.clone()
    assert type(c) is cls
    for name in fields:
        assert np.array_equal(getattr(c, name), getattr(st, name)) and not np.shares_memory(getattr(c, name), getattr(st, name))

    t = cls.of(*[torch.from_numpy(getattr(st, name)).to(torch.float64 if name != "prev_done" else torch.int64) for name in fields])
    host = t.numpy()                                       # the right dtypes, whatever the tensors held
    assert type(host) is cls and t.device == torch.device("cpu")
    assert [getattr(host, name).dtype for name in fields] == [np.float32, np.float32, np.float32, np.uint8]
    for name in fields:
        assert np.array_equal(getattr(host, name), getattr(st, name))

    reward, done, clear = np.array([7.0, 8.0, 9.0]), np.array([False, True, True]), np.array([False, False, True])
    plain = st.observed(reward, done)
    assert type(plain) is cls and plain.prev_reward.dtype == np.float32 and plain.prev_done.dtype == np.uint8
    assert np.array_equal(plain.h, st.h) and np.array_equal(plain.prev_action, st.prev_action)
    assert plain.prev_reward.tolist() == [7.0, 8.0, 9.0] and plain.prev_done.tolist() == [0, 1, 1]
    out = st.observed(reward, done, clear)
    for name in fields:                                    # exactly the cleared rows are zero, the others are `plain`'s
        assert np.array_equal(getattr(out, name)[:2], getattr(plain, name)[:2]) and not getattr(out, name)[2].any()
        assert getattr(plain, name)[:2].all() or name == "prev_done"
    assert np.array_equal(st.prev_reward, np.array([0.5, 1.5, 2.5], np.float32))          # `observed` writes nothing back

    for bad in (np.zeros(2, bool), np.zeros((3, 1), bool), np.zeros(4, bool)):
        with pytest.raises(ValueError, match=re.escape("clear must have shape (3,)")):
            st.observed(reward, done, bad)
    with pytest.raises(ValueError, match=re.escape("reward and done must have shape (3,)")):
        st.observed(reward[:2], done)
