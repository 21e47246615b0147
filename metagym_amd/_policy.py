"""What the Python front ends of the closed-loop rollouts share (quadrotor, MetaLocomotion, MetaMaze 2-D, bandits, LiftSim):
the argument helpers, Philox and the exploration threshold, the exact float32 `log32` / `u01` and the Gumbel-max draw of the
softmax-sampled policies built on them, the upload-once cache of a packed policy set, the carry of the
continuous-action recurrent policies, the validator and cache of `policy_ids`, and the carry checks of `rollout_policy`.
LiftSim's recurrent form (`LiftRecurrentPolicy`, `liftsim/policy.py`) takes the argument helpers, `PackedPolicySet` and
`policy_ids`; its carry (`LiftPolicyState`: a memory per elevator, stored env index fastest) and that carry's checks stay
with it, since no other family shares their shape.

What differs per env stays with the env: the `reference` arithmetic, `pack` / `unpack` and the layout constants, and the ctypes
calls. Nothing here needs a GPU to import; torch is imported inside the functions."""
import math

import numpy as np


def to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def f32_array(name, x, ndim):
    a = to_numpy(x)
    if a.dtype != np.float32:
        raise TypeError("%s must be float32, got %s" % (name, a.dtype))
    if a.ndim != ndim:
        raise ValueError("%s must have %d dimensions, got shape %s" % (name, ndim, a.shape))
    if not np.isfinite(a).all():
        raise ValueError("%s holds a value that is not finite" % name)
    return np.ascontiguousarray(a)


def pad4(n):
    return (int(n) + 3) & ~3


def eps_threshold(epsilon):
    """thr = min(floor(epsilon * 2^32), 2^32 - 1) as uint32, elementwise; epsilon float64 in [0, 1]."""
    e = np.asarray(epsilon, np.float64)
    return np.asarray([min(int(math.floor(v * 4294967296.0)), 0xFFFFFFFF) for v in e.ravel()], np.uint32).reshape(e.shape)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on numpy integers, the function of csrc/mg_philox.h: uint32 arrays (or scalars) in,
    four uint32 arrays out."""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(v, np.uint64) & m32 for v in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


F = np.float32
SAMPLE_TAG = 0x53000000      # c3 of a sampling block: tag | (action >> 2)

# the constants of log32, by their float32 bits
LG1, LG2, LG3, LG4 = (np.array([b], np.uint32).view(F)[0] for b in (0x3f2aaaaa, 0x3eccce13, 0x3e91e9ee, 0x3e789e26))
LN2_HI, LN2_LO = (np.array([b], np.uint32).view(F)[0] for b in (0x3f317180, 0x3717f7d1))


def log32(x):
    """fdlibm's single-precision log, one operation at a time (written out in bandits/learner.py), on a float32 array of
    positive normal numbers (any shape), in numpy float32."""
    x = np.asarray(x)
    if x.dtype != F:
        raise TypeError("log32 takes float32, got %s" % x.dtype)
    shape = x.shape
    i = np.ascontiguousarray(x).reshape(-1).view(np.uint32) + np.uint32(0x3f800000 - 0x3f3504f3)
    k = (i >> np.uint32(23)).astype(np.int32) - np.int32(127)
    m = ((i & np.uint32(0x007fffff)) + np.uint32(0x3f3504f3)).view(F)
    one, two, half = F(1.0), F(2.0), F(0.5)
    with np.errstate(all="ignore"):
        f = m - one
        s = f / (two + f)
        z = s * s
        w = z * z
        t1 = w * (LG2 + w * LG4)
        t2 = z * (LG1 + w * LG3)
        R = t2 + t1
        hfsq = (half * f) * f
        dk = k.astype(F)
        out = (((s * (hfsq + R) + dk * LN2_LO) - hfsq) + f) + dk * LN2_HI
    assert out.dtype == F
    return out.reshape(shape)


def u01(word):
    """(float)(((word >> 9) << 1) | 1) * 2^-24 on uint32 words: an odd 24-bit integer, so exact, never 0 and never 1."""
    w = np.asarray(word, np.uint32)
    return (((w >> np.uint32(9)) << np.uint32(1)) | np.uint32(1)).astype(F) * F(2.0 ** -24)


def gumbel32(words):
    """g = -log32(-log32(u01(word))) on uint32 words, float32: the standard Gumbel value of the sampled policies. -log32(u)
    is a positive normal float for every u that u01 returns, so both applications meet log32's precondition; g is finite."""
    return -log32(-log32(u01(words)))


def check_temperature(temperature, P):
    """The temperatures of P policies as a contiguous float32 [P] array, finite and > 0, whose float32 inverse
    float32(1) / temperature is finite and > 0 too."""
    t = to_numpy(temperature)
    if t.dtype != F:
        raise TypeError("temperature must be float32, got %s" % t.dtype)
    if t.shape != (P,):
        raise ValueError("temperature must have shape (%d,), got %s" % (P, t.shape))
    if not (np.isfinite(t) & (t > 0)).all():
        raise ValueError("temperature must be finite and > 0")
    inv = inverse_temperature(t)
    if not (np.isfinite(inv) & (inv > 0)).all():
        raise ValueError("1 / temperature must be a finite float32 > 0")
    return np.ascontiguousarray(t)


def inverse_temperature(temperature):
    """inv_t = float32(1) / float32(temperature), elementwise in numpy float32: what the kernel receives."""
    with np.errstate(all="ignore"):
        return (F(1.0) / np.asarray(temperature, F)).astype(F)


def sample_actions(logits, inv_t, env_ids, step, seed):
    """The Gumbel-max draw of include/metagym_hip.h on float32 logits [N, K]: score[k] = logits[k] * inv_t + g[k] (one float32
    multiply, then one float32 add), g[k] from word k & 3 of the Philox block with c3 = SAMPLE_TAG | (k >> 2) of env
    env_ids[e] at carry step `step`; the lowest index among the maxima. inv_t float32 [N]. Returns int32 [N]."""
    logits, inv_t = np.asarray(logits), np.asarray(inv_t)
    assert logits.dtype == F and inv_t.dtype == F
    N, K = logits.shape
    e = np.asarray(env_ids).astype(np.uint64)
    n, s = int(step), int(seed)
    action = np.zeros(N, np.int32)
    best = None
    with np.errstate(all="ignore"):
        for k in range(K):
            if k % 4 == 0:
                out = philox4x32_10(e, n & 0xFFFFFFFF, (n >> 32) & 0xFFFFFFFF, SAMPLE_TAG | (k >> 2), s & 0xFFFFFFFF,
                                    (s >> 32) & 0xFFFFFFFF)
            score = logits[:, k] * inv_t + gumbel32(out[k & 3])
            assert score.dtype == F
            if k == 0:
                best = score
            else:
                better = score > best
                action = np.where(better, np.int32(k), action)
                best = np.where(better, score, best)
    return action


def check_epsilon(epsilon, P):
    """The exploration rates of P policies as a contiguous float64 [P] array in [0, 1]."""
    eps = to_numpy(epsilon)
    if eps.dtype != np.float64:
        raise TypeError("epsilon must be float64, got %s" % eps.dtype)
    if eps.shape != (P,):
        raise ValueError("epsilon must have shape (%d,), got %s" % (P, eps.shape))
    if not ((eps >= 0.0) & (eps <= 1.0)).all():
        raise ValueError("epsilon must be in [0, 1]")
    return np.ascontiguousarray(eps)


class PackedPolicySet(object):
    """The base of a packed policy set: `len()`, `to(device)` and, for a set with an `epsilon` attribute (float64 [P] or
    None), `thresholds`. A subclass sets `num_policies`; `_host` says what `to` uploads."""

    def __len__(self):
        return self.num_policies

    @property
    def thresholds(self):
        """uint32 [P]: thr[p] = min(floor(epsilon[p] * 2^32), 2^32 - 1); zeros without epsilon."""
        if self.epsilon is None:
            return np.zeros(len(self), np.uint32)
        return eps_threshold(self.epsilon)

    def _threshold_bits(self):
        """The thresholds as they travel: the int32 array with the uint32's bits, None without epsilon."""
        return None if self.epsilon is None else self.thresholds.view(np.int32).copy()

    def _host(self):
        """What `to` uploads: one numpy array, or a tuple of arrays and Nones. Here the packed parameters alone."""
        return self.pack()

    temperature = None       # float32 [P] on a set that samples its actions (the discrete-action policies), else None

    @property
    def inv_temperature(self):
        """float32 [P]: float32(1) / temperature[p], what the sampled kernels multiply the logits with; None without."""
        return None if self.temperature is None else inverse_temperature(self.temperature)

    def inv_temperature_on(self, device):
        """`inv_temperature` as a torch tensor on `device`, uploaded once per device and kept apart from what `to` returns."""
        import torch
        from . import _lib
        if self.temperature is None:
            return None
        cache = self.__dict__.setdefault("_inv_t_device", {})
        key = str(_lib.canonical_device(device))
        if key not in cache:
            cache[key] = torch.from_numpy(self.inv_temperature).to(_lib.canonical_device(device)).contiguous()
        return cache[key]

    def to(self, device):
        """The arrays of `_host` as contiguous torch tensors on `device` (uploaded once per device), None staying None."""
        import torch
        from . import _lib
        dev = _lib.canonical_device(device)
        cache = self.__dict__.setdefault("_device", {})
        key = str(dev)
        if key not in cache:
            up = lambda a: None if a is None else torch.from_numpy(a).to(dev).contiguous()
            host = self._host()
            cache[key] = tuple(up(a) for a in host) if isinstance(host, tuple) else up(host)
        return cache[key]


class ContinuousPolicyState(object):
    """The carry of a recurrent closed-loop rollout with continuous actions, the policy's memory of each env: h float32
    [N, H], prev_action float32 [N, A] (unclamped), prev_reward float32 [N], prev_done uint8 [N]. Torch tensors on the env's
    device, updated in place by a launch, or numpy arrays, for a policy's `reference`. All zero when fresh. The subclasses
    (`QuadrotorPolicyState`, `WalkerPolicyState`) name the four fields in their `__slots__` and say how a fresh carry is
    spelled."""
    __slots__ = ()

    @classmethod
    def of(cls, h, prev_action, prev_reward, prev_done):
        """A carry that holds the given arrays (not copied)."""
        self = cls.__new__(cls)
        self.h, self.prev_action, self.prev_reward, self.prev_done = h, prev_action, prev_reward, prev_done
        return self

    @staticmethod
    def _zero_arrays(N, H, A, device):
        """(h, prev_action, prev_reward, prev_done) of a fresh carry. device None: numpy arrays."""
        if device is None:
            return np.zeros((N, H), np.float32), np.zeros((N, A), np.float32), np.zeros(N, np.float32), np.zeros(N, np.uint8)
        import torch
        return (torch.zeros(N, H, dtype=torch.float32, device=device), torch.zeros(N, A, dtype=torch.float32, device=device),
                torch.zeros(N, dtype=torch.float32, device=device), torch.zeros(N, dtype=torch.uint8, device=device))

    @property
    def num_envs(self):
        return int(self.h.shape[0])

    @property
    def hidden(self):
        return int(self.h.shape[1])

    @property
    def n_act(self):
        return int(self.prev_action.shape[1])

    @property
    def device(self):
        """The torch device of the arrays; None for a numpy carry."""
        return self.h.device if hasattr(self.h, "detach") else None

    def clone(self):
        c = (lambda v: v.clone()) if hasattr(self.h, "clone") else (lambda v: v.copy())
        return self.of(c(self.h), c(self.prev_action), c(self.prev_reward), c(self.prev_done))

    def numpy(self):
        """A host copy, as numpy arrays: what the recurrent policy's `reference` takes."""
        return self.of(to_numpy(self.h).astype(np.float32), to_numpy(self.prev_action).astype(np.float32),
                       to_numpy(self.prev_reward).astype(np.float32), to_numpy(self.prev_done).astype(np.uint8))

    def observed(self, reward, done, clear=None):
        """The numpy carry after the env step that followed `reference`: prev_reward = float32(reward), prev_done = done, h
        and prev_action kept. `clear` (bool [N] or None): the envs whose four fields are zeroed afterwards, which is what
        `episodic=True` does at a done with `auto_reset`."""
        out = self.of(to_numpy(self.h).astype(np.float32), to_numpy(self.prev_action).astype(np.float32),
                      to_numpy(reward).astype(np.float32), (to_numpy(done) != 0).astype(np.uint8))
        if out.prev_reward.shape != (self.num_envs,) or out.prev_done.shape != (self.num_envs,):
            raise ValueError("reward and done must have shape (%d,)" % self.num_envs)
        if clear is not None:
            c = to_numpy(clear).astype(bool)
            if c.shape != (self.num_envs,):
                raise ValueError("clear must have shape (%d,)" % self.num_envs)
            out.h[c] = 0.0
            out.prev_action[c] = 0.0
            out.prev_reward[c] = 0.0
            out.prev_done[c] = 0
        return out


_DEFAULT_IDS = {"modulo": lambda N, P: np.arange(N, dtype=np.int64) % P, "zero": lambda N, P: np.zeros(N, np.int64)}


def policy_ids(env, policy_ids, P, default="modulo", name="policy_ids"):
    """int32 [N] device tensor of validated policy ids for `env` (anything with `num_envs` and `device`). None is e % P
    (default="modulo") or policy 0 for all (default="zero"). The last answer is kept on the env as `_policy_ids_keep`: a
    repeated call (a search loop, a hipGraph capture after its warm-up) with None, the same host ids, or the same tensor
    object with an unchanged `_version` neither uploads nor reads back; any other device tensor is read back once. None
    and the unchanged tensor are recognised by identity, before any array is built."""
    import torch
    if default not in _DEFAULT_IDS:
        raise ValueError("default must be 'modulo' or 'zero', got %r" % (default,))
    N = env.num_envs
    keep = getattr(env, "_policy_ids_keep", None)          # (P, device ids, source, its version, the ids' bytes)
    # the source: the caller's tensor, the rule that stands for None, or nothing for host ids
    src = _DEFAULT_IDS[default] if policy_ids is None else policy_ids if isinstance(policy_ids, torch.Tensor) else None
    version = getattr(src, "_version", None)
    if src is not None and keep is not None and keep[0] == P and src is keep[2] and version == keep[3]:
        return keep[1]
    if policy_ids is None:
        ids_h = src(N, P)
    else:
        ids_h = to_numpy(policy_ids)
        if ids_h.shape != (N,):
            raise ValueError("%s must have shape (%d,), got %s" % (name, N, tuple(ids_h.shape)))
        if ids_h.dtype.kind not in "iu":
            raise ValueError("%s must be integers, got %s" % (name, ids_h.dtype))
        if N and (int(ids_h.min()) < 0 or int(ids_h.max()) >= P):
            raise ValueError("%s must be in [0, %d)" % (name, P))
    ids_h = ids_h.astype(np.int32)
    data = ids_h.tobytes()
    same = keep is not None and keep[0] == P and keep[4] == data
    ids_d = keep[1] if same else torch.as_tensor(ids_h, device=env.device).contiguous()
    env._policy_ids_keep = (P, ids_d, src, version, data)
    return ids_d


def check_discrete_carry(state, cls, N, H, T, seed, device):
    """The seed and carry checks of a discrete-action `rollout_policy` (maze, bandits): returns (state, seed), the state a
    fresh `cls.zeros(N, H, device)` when None was passed. Nothing is written."""
    import torch
    seed = int(seed)
    if not (0 <= seed < 2 ** 64):
        raise ValueError("seed must be in [0, 2^64), got %d" % seed)
    if state is None:
        state = cls.zeros(N, H, device)
    elif not isinstance(state, cls):
        raise TypeError("state must be a %s, got %s" % (cls.__name__, type(state).__name__))
    want = (("h", (N, H), torch.float32), ("prev_action", (N,), torch.int32), ("prev_reward", (N,), torch.float32),
            ("prev_done", (N,), torch.uint8))
    for name, shape, dtype in want:
        v = getattr(state, name)
        if not isinstance(v, torch.Tensor) or tuple(v.shape) != shape or v.dtype != dtype:
            raise ValueError("state.%s must be a %s tensor of shape %s (this env has %d envs, the policy %d hidden units)"
                             % (name, dtype, shape, N, H))
    if not (0 <= state.step < 2 ** 64 - T):
        raise ValueError("state.step = %d is outside [0, 2^64 - steps)" % state.step)
    return state, seed


def check_continuous_carry(state, cls, N, H, A, device, fresh, sizes):
    """The carry checks of a continuous-action recurrent `rollout_policy` (quadrotor, walker) for a state that is not None:
    the class, torch tensors, the device, then shape, dtype and contiguity field by field. `fresh` is how a fresh carry is
    spelled and `sizes` the sizes as the messages name them."""
    import torch
    if not isinstance(state, cls):
        raise TypeError("state must be a %s, got %s" % (cls.__name__, type(state).__name__))
    fields = (state.h, state.prev_action, state.prev_reward, state.prev_done)
    if not all(isinstance(t, torch.Tensor) for t in fields):
        raise ValueError("state must hold torch tensors on %s (%s)" % (device, fresh))
    if any(t.device != device for t in fields):
        raise ValueError("state lives on %s, the env on %s" % (state.h.device, device))
    want = (((N, H), torch.float32), ((N, A), torch.float32), ((N,), torch.float32), ((N,), torch.uint8))
    for t, (shape, dtype), name in zip(fields, want, ("h", "prev_action", "prev_reward", "prev_done")):
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
            raise ValueError("state.%s must be a contiguous %s tensor of shape %s (%s), got %s %s"
                             % (name, dtype, shape, sizes, t.dtype, tuple(t.shape)))
