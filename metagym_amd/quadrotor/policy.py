"""Quadrotor policies for `Quadrotor.rollout_policy`: P small MLPs (or linear maps) from the float32 observation to
four voltages, evaluated inside the rollout launch (include/metagym_hip.h, mg_quadrotor_policy_rollout).

The arithmetic is defined exactly, so the closed loop can be replayed bit for bit. x[D] is the observation (D = 16, or
19 for velocity_control), H the number of hidden ReLU units (0 <= H <= 256, H = 0 is a linear policy). Every operation
is float32, rounded once, never fused, in this order:

    H > 0:  for j in 0..H-1:  z = b1[j];  for i in 0..D-1: z = z + w1[j][i] * x[i];   h[j] = (z > 0) ? z : 0
            for k in 0..3:    a[k] = b2[k];  for j in 0..H-1: a[k] = a[k] + w2[k][j] * h[j]
    H = 0:  for k in 0..3:    a[k] = b[k];   for i in 0..D-1: a[k] = a[k] + w[k][i] * x[i]

`a` goes into the step unclamped; the step clamps it to the voltage range like any caller's action.
`QuadrotorPolicy.reference` evaluates exactly this in numpy float32. Nothing here needs a GPU to import.

    pol = QuadrotorPolicy.linear(w, b)                     # w [P, 4, 16], b [P, 4], float32
    res = env.rollout_policy(pol, steps=64)                # env e flies policy e % P
"""
import numpy as np

MAX_HIDDEN = 256
OBS_DIMS = (16, 19)
_HEAD, _REC, _W2_AT = 4, 24, 20     # packed layout, see param_count / pack


def param_count(hidden, obs_dim):
    """Floats per packed policy (what mg_quadrotor_policy_param_count returns)."""
    return _HEAD + _REC * hidden if hidden > 0 else _HEAD + 4 * obs_dim


def _f32(name, x, ndim):
    if hasattr(x, "detach"):                               # a torch tensor
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.dtype != np.float32:
        raise TypeError("%s must be float32, got %s" % (name, a.dtype))
    if a.ndim != ndim:
        raise ValueError("%s must have %d dimensions, got shape %s" % (name, ndim, a.shape))
    if not np.isfinite(a).all():
        raise ValueError("%s holds a value that is not finite" % name)
    return np.ascontiguousarray(a)


class QuadrotorPolicy(object):
    """P policies with one hidden ReLU layer: w1 [P, H, D], b1 [P, H], w2 [P, 4, H], b2 [P, 4], all float32 and finite.
    `QuadrotorPolicy.linear(w, b)` builds the H = 0 form."""

    def __init__(self, w1, b1, w2, b2):
        w1, b1, w2, b2 = _f32("w1", w1, 3), _f32("b1", b1, 2), _f32("w2", w2, 3), _f32("b2", b2, 2)
        P, H, D = w1.shape
        if P < 1:
            raise ValueError("a policy set needs at least one policy")
        if not (1 <= H <= MAX_HIDDEN):
            raise ValueError("hidden units must be in [1, %d] (QuadrotorPolicy.linear for none), got %d" % (MAX_HIDDEN, H))
        if D not in OBS_DIMS:
            raise ValueError("the observation has 16 entries (19 for velocity_control), w1 has %d" % D)
        if b1.shape != (P, H) or w2.shape != (P, 4, H) or b2.shape != (P, 4):
            raise ValueError("shapes must be w1 [P,H,D], b1 [P,H], w2 [P,4,H], b2 [P,4]; got %s %s %s %s"
                             % (w1.shape, b1.shape, w2.shape, b2.shape))
        self.w1, self.b1, self.w2, self.b2 = w1, b1, w2, b2
        self.num_policies, self.hidden, self.obs_dim = P, H, D
        self._device = {}

    @classmethod
    def linear(cls, w, b):
        """a = b + w @ x in the order of the definition: w [P, 4, D], b [P, 4]."""
        w, b = _f32("w", w, 3), _f32("b", b, 2)
        P, four, D = w.shape
        if P < 1:
            raise ValueError("a policy set needs at least one policy")
        if four != 4 or b.shape != (P, 4):
            raise ValueError("shapes must be w [P,4,D], b [P,4]; got %s %s" % (w.shape, b.shape))
        if D not in OBS_DIMS:
            raise ValueError("the observation has 16 entries (19 for velocity_control), w has %d" % D)
        self = cls.__new__(cls)
        self.w1 = self.b1 = None
        self.w2, self.b2 = w, b                            # the output layer, read straight from x
        self.num_policies, self.hidden, self.obs_dim = P, 0, D
        self._device = {}
        return self

    def __len__(self):
        return self.num_policies

    @property
    def param_count(self):
        return param_count(self.hidden, self.obs_dim)

    def pack(self):
        """float32 [P, param_count]: the layout the kernel reads (documented in include/metagym_hip.h).
        H > 0: b2[0..3], then per hidden unit j a record of 24 floats: w1[j][0..D-1], b1[j], zeros up to 20, w2[0..3][j].
        H = 0: b[0..3], then w[k][i] at 4 + 4 i + k."""
        P, H, D = self.num_policies, self.hidden, self.obs_dim
        out = np.zeros((P, self.param_count), np.float32)
        out[:, :_HEAD] = self.b2
        if H == 0:
            out[:, _HEAD:] = self.w2.transpose(0, 2, 1).reshape(P, 4 * D)
            return out
        rec = out[:, _HEAD:].reshape(P, H, _REC)
        rec[:, :, :D] = self.w1
        rec[:, :, D] = self.b1
        rec[:, :, _W2_AT:] = self.w2.transpose(0, 2, 1)
        return out

    @classmethod
    def unpack(cls, packed, hidden, obs_dim):
        """The inverse of `pack`."""
        packed = _f32("packed", packed, 2)
        P = packed.shape[0]
        if obs_dim not in OBS_DIMS or not (0 <= hidden <= MAX_HIDDEN) or packed.shape[1] != param_count(hidden, obs_dim):
            raise ValueError("packed has shape %s, hidden=%d and obs_dim=%d need [P, %d]"
                             % (packed.shape, hidden, obs_dim, param_count(max(hidden, 0), obs_dim)))
        b2 = packed[:, :_HEAD].copy()
        if hidden == 0:
            return cls.linear(packed[:, _HEAD:].reshape(P, obs_dim, 4).transpose(0, 2, 1).copy(), b2)
        rec = packed[:, _HEAD:].reshape(P, hidden, _REC)
        return cls(rec[:, :, :obs_dim].copy(), rec[:, :, obs_dim].copy(), rec[:, :, _W2_AT:].transpose(0, 2, 1).copy(), b2)

    def to(self, device):
        """The packed parameters as a torch tensor on `device` (uploaded once per device)."""
        import torch
        from .. import _lib
        key = str(_lib.canonical_device(device))
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.pack()).to(_lib.canonical_device(device)).contiguous()
        return self._device[key]

    def reference(self, obs, policy_ids):
        """The definition above in numpy float32, with exactly that association: obs [N, D] float32, policy_ids [N]
        -> float32 [N, 4]. The oracle of the policy half of a closed-loop rollout."""
        x = np.asarray(obs)
        ids = np.asarray(policy_ids)
        if x.dtype != np.float32 or x.ndim != 2 or x.shape[1] != self.obs_dim:
            raise ValueError("obs must be float32 [N, %d], got %s %s" % (self.obs_dim, x.dtype, x.shape))
        if ids.shape != (x.shape[0],) or ids.dtype.kind not in "iu":
            raise ValueError("policy_ids must be %d integers" % x.shape[0])
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.num_policies):
            raise ValueError("policy_ids must be in [0, %d)" % self.num_policies)
        N, D, H = x.shape[0], self.obs_dim, self.hidden
        a = self.b2[ids].copy()                            # [N, 4]
        with np.errstate(all="ignore"):
            if H == 0:
                w = self.w2[ids]                           # [N, 4, D]
                for i in range(D):
                    a = a + w[:, :, i] * x[:, i:i + 1]
                return a
            w1, b1, w2 = self.w1[ids], self.b1[ids], self.w2[ids]
            for j in range(H):
                z = b1[:, j].copy()
                for i in range(D):
                    z = z + w1[:, j, i] * x[:, i]
                h = np.where(z > 0, z, np.float32(0.0))
                a = a + w2[:, :, j] * h[:, None]
        assert a.dtype == np.float32 and a.shape == (N, 4)
        return a


class PolicyRollout(object):
    """What `Quadrotor.rollout_policy` returns. Always: ret_total f64 [N] (the T float64 rewards added in step order),
    ret_episode f64 [N] (the rewards up to and including the first done), episode_len int32 [N] (steps added into
    ret_episode; T if the env was never done). With record=True also actions [T,N,4] (unclamped), obs [T,N,D],
    reward [T,N], reward64 [T,N], done [T,N] bool, failed [T,N] uint8; otherwise those are None."""
    __slots__ = ("ret_total", "ret_episode", "episode_len", "actions", "obs", "reward", "reward64", "done", "failed")

    def __init__(self, ret_total, ret_episode, episode_len, actions=None, obs=None, reward=None, reward64=None, done=None,
                 failed=None):
        self.ret_total, self.ret_episode, self.episode_len = ret_total, ret_episode, episode_len
        self.actions, self.obs, self.reward, self.reward64, self.done, self.failed = actions, obs, reward, reward64, done, failed
