"""Walker policies for `WalkerBatchEnv.rollout_policy`: P small MLPs (or linear maps) from the float32 observation to the
n_joints torque actions, evaluated inside the rollout launch (include/metagym_hip.h, mg_walker_policy_rollout).

The arithmetic is defined exactly, as for the quadrotor (metagym_amd/quadrotor/policy.py), so the closed loop can be replayed
bit for bit. x[D] is the observation (D = 8 + 2 n_joints + n_feet: 44 for the humanoid, 28 for the ant), A = n_joints the
number of outputs, H the number of hidden ReLU units (0 <= H <= 256, H = 0 is a linear policy). Every operation is float32,
rounded once, never fused, in this order:

    H > 0:  for j in 0..H-1:  z = b1[j];  for i in 0..D-1: z = z + w1[j][i] * x[i];   h[j] = (z > 0) ? z : 0
            for k in 0..A-1:  a[k] = b2[k];  for j in 0..H-1: a[k] = a[k] + w2[k][j] * h[j]
    H = 0:  for k in 0..A-1:  a[k] = b[k];   for i in 0..D-1: a[k] = a[k] + w[k][i] * x[i]

`a` goes into the step unclamped; the step clamps it to [-1, 1] like any caller's action.
`WalkerPolicy.reference` evaluates exactly this in numpy float32. Nothing here needs a GPU to import. D and A are checked
against the env when a policy is used, not when it is built.

    pol = WalkerPolicy.linear(w, b)                        # w [P, 8, 28], b [P, 8], float32: P linear policies for the ant
    res = env.rollout_policy(pol, steps=64)                # env e runs policy e % P
"""
import numpy as np

MAX_HIDDEN = 256


def param_count(hidden, obs_dim, n_act):
    """Floats per packed policy (what mg_walker_policy_param_count returns)."""
    return hidden + obs_dim * hidden + n_act + hidden * n_act if hidden > 0 else n_act + obs_dim * n_act


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


class WalkerPolicy(object):
    """P policies with one hidden ReLU layer: w1 [P, H, D], b1 [P, H], w2 [P, A, H], b2 [P, A], all float32 and finite,
    1 <= H <= 256. `WalkerPolicy.linear(w, b)` builds the H = 0 form."""

    def __init__(self, w1, b1, w2, b2):
        w1, b1, w2, b2 = _f32("w1", w1, 3), _f32("b1", b1, 2), _f32("w2", w2, 3), _f32("b2", b2, 2)
        P, H, D = w1.shape
        A = w2.shape[1]
        if P < 1 or D < 1 or A < 1:
            raise ValueError("a policy set needs at least one policy, one input and one output; got w1 %s, w2 %s" % (w1.shape, w2.shape))
        if not (1 <= H <= MAX_HIDDEN):
            raise ValueError("hidden units must be in [1, %d] (WalkerPolicy.linear for none), got %d" % (MAX_HIDDEN, H))
        if b1.shape != (P, H) or w2.shape != (P, A, H) or b2.shape != (P, A):
            raise ValueError("shapes must be w1 [P,H,D], b1 [P,H], w2 [P,A,H], b2 [P,A]; got %s %s %s %s"
                             % (w1.shape, b1.shape, w2.shape, b2.shape))
        self.w1, self.b1, self.w2, self.b2 = w1, b1, w2, b2
        self.num_policies, self.hidden, self.obs_dim, self.n_act = P, H, D, A
        self._device = {}

    @classmethod
    def linear(cls, w, b):
        """a = b + w @ x in the order of the definition: w [P, A, D], b [P, A]."""
        w, b = _f32("w", w, 3), _f32("b", b, 2)
        P, A, D = w.shape
        if P < 1 or D < 1 or A < 1:
            raise ValueError("a policy set needs at least one policy, one input and one output; got w %s" % (w.shape,))
        if b.shape != (P, A):
            raise ValueError("shapes must be w [P,A,D], b [P,A]; got %s %s" % (w.shape, b.shape))
        self = cls.__new__(cls)
        self.w1 = self.b1 = None
        self.w2, self.b2 = w, b                            # the output layer, read straight from x
        self.num_policies, self.hidden, self.obs_dim, self.n_act = P, 0, D, A
        self._device = {}
        return self

    def __len__(self):
        return self.num_policies

    @property
    def param_count(self):
        return param_count(self.hidden, self.obs_dim, self.n_act)

    def pack(self):
        """float32 [P, param_count]: the layout the kernel reads (documented in include/metagym_hip.h), chosen so that the lanes
        of a wave read consecutive floats.
        H > 0: b1[H], w1 input-major [D][H], b2[A], w2 hidden-major [H][A].
        H = 0: b[A], w input-major [D][A]."""
        P, H, D, A = self.num_policies, self.hidden, self.obs_dim, self.n_act
        tail = [self.b2, self.w2.transpose(0, 2, 1).reshape(P, -1)]             # [P, A], [P, (H or D) * A]
        head = [] if H == 0 else [self.b1, self.w1.transpose(0, 2, 1).reshape(P, D * H)]
        out = np.ascontiguousarray(np.concatenate(head + tail, axis=1), dtype=np.float32)
        assert out.shape == (P, self.param_count)
        return out

    @classmethod
    def unpack(cls, packed, hidden, obs_dim, n_act):
        """The inverse of `pack`."""
        packed = _f32("packed", packed, 2)
        P, H, D, A = packed.shape[0], int(hidden), int(obs_dim), int(n_act)
        if not (0 <= H <= MAX_HIDDEN) or D < 1 or A < 1 or packed.shape[1] != param_count(H, D, A):
            raise ValueError("packed has shape %s, hidden=%d, obs_dim=%d and n_act=%d need [P, %d]"
                             % (packed.shape, H, D, A, param_count(min(max(H, 0), MAX_HIDDEN), max(D, 1), max(A, 1))))
        if H == 0:
            return cls.linear(packed[:, A:].reshape(P, D, A).transpose(0, 2, 1).copy(), packed[:, :A].copy())
        at = H + D * H
        return cls(packed[:, H:at].reshape(P, D, H).transpose(0, 2, 1).copy(), packed[:, :H].copy(),
                   packed[:, at + A:].reshape(P, H, A).transpose(0, 2, 1).copy(), packed[:, at:at + A].copy())

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
        -> float32 [N, A]. The oracle of the policy half of a closed-loop rollout."""
        x = obs.detach().cpu().numpy() if hasattr(obs, "detach") else np.asarray(obs)
        ids = policy_ids.detach().cpu().numpy() if hasattr(policy_ids, "detach") else np.asarray(policy_ids)
        if x.dtype != np.float32 or x.ndim != 2 or x.shape[1] != self.obs_dim:
            raise ValueError("obs must be float32 [N, %d], got %s %s" % (self.obs_dim, x.dtype, x.shape))
        if ids.shape != (x.shape[0],) or ids.dtype.kind not in "iu":
            raise ValueError("policy_ids must be %d integers" % x.shape[0])
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.num_policies):
            raise ValueError("policy_ids must be in [0, %d)" % self.num_policies)
        N, D, H, A = x.shape[0], self.obs_dim, self.hidden, self.n_act
        a = self.b2[ids].copy()                            # [N, A]
        with np.errstate(all="ignore"):
            if H == 0:
                w = self.w2[ids]                           # [N, A, D]
                for i in range(D):
                    a = a + w[:, :, i] * x[:, i:i + 1]
                return a
            w1, b1, w2 = self.w1[ids], self.b1[ids], self.w2[ids]
            z = b1.copy()                                  # [N, H]: every unit's own sum, i ascending
            for i in range(D):
                z = z + w1[:, :, i] * x[:, i:i + 1]
            h = np.where(z > 0, z, np.float32(0.0))
            for j in range(H):
                a = a + w2[:, :, j] * h[:, j:j + 1]
        assert a.dtype == np.float32 and a.shape == (N, A)
        return a


class WalkerPolicyRollout(object):
    """What `WalkerBatchEnv.rollout_policy` returns. Always: ret_total f64 [N] (the T float32 rewards widened and added in step
    order), ret_episode f64 [N] (the rewards up to and including the first done), episode_len int32 [N] (steps added into
    ret_episode; T if the env was never done), obs (the persistent [N, D] buffer for obs_every = 0, else [K, N, D]) and
    obs_steps (the K recorded step indices). With record=True also actions [T,N,nj] (unclamped), reward [T,N], done [T,N]
    bool, rewards5 [T,N,5]; otherwise those are None."""
    __slots__ = ("ret_total", "ret_episode", "episode_len", "obs", "obs_steps", "actions", "reward", "done", "rewards5")

    def __init__(self, ret_total, ret_episode, episode_len, obs, obs_steps, actions=None, reward=None, done=None, rewards5=None):
        self.ret_total, self.ret_episode, self.episode_len, self.obs, self.obs_steps = ret_total, ret_episode, episode_len, obs, obs_steps
        self.actions, self.reward, self.done, self.rewards5 = actions, reward, done, rewards5
