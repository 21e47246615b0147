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

`QuadrotorRecurrentPolicy` is the form with a memory (mg_quadrotor_rpolicy_rollout). Besides x it reads pa[4], the previous
*unclamped* action (the value the `actions` record holds), pr, the float32 of the previous step's reward record, pd, the
previous done, and its memory h[H], 1 <= H <= 64. Again every operation is float32, rounded once, never fused, in this order:

    for j in 0..H-1:  z = b[j]
                      for i in 0..D-1: z = z + wx[j][i] * x[i]
                      for k in 0..3:   z = z + wa[j][k] * pa[k]
                      z = z + wr[j] * pr
                      z = z + wd[j] * (pd ? 1 : 0)
                      for i in 0..H-1: z = z + wh[j][i] * h[i]
                      hn[j] = z > 1 ? 1 : (z < -1 ? -1 : z)
    h = hn
    for k in 0..3:    a[k] = bo[k];  for j in 0..H-1: a[k] = a[k] + wo[k][j] * h[j]

A NaN pre-activation stays NaN, -0 stays -0, and the padding of a packed record is never multiplied in. The carry
(`QuadrotorPolicyState`: h, prev_action, prev_reward, prev_done) lives on the device, is updated in place by a launch and is
all zero when fresh: T1 steps and then T2 steps with one state object equal T1 + T2 steps in one call. The memory survives a
done; `episodic=True` (with `auto_reset`) clears the carry of an env at its done instead.

    pol = QuadrotorRecurrentPolicy(wx, wa, wr, wd, wh, b, wo, bo)
    res = env.rollout_policy(pol, steps=64)                       # from a fresh carry
    res = env.rollout_policy(pol, steps=64, state=res.state)      # and goes on, memory kept
"""
import numpy as np

from .._policy import ContinuousPolicyState, PackedPolicySet, f32_array, pad4, to_numpy

MAX_HIDDEN = 256
MAX_RECURRENT_HIDDEN = 64
OBS_DIMS = (16, 19)
_HEAD, _REC, _W2_AT = 4, 24, 20     # packed layout, see param_count / pack


def param_count(hidden, obs_dim):
    """Floats per packed policy (what mg_quadrotor_policy_param_count returns)."""
    return _HEAD + _REC * hidden if hidden > 0 else _HEAD + 4 * obs_dim


class QuadrotorPolicy(PackedPolicySet):
    """P policies with one hidden ReLU layer: w1 [P, H, D], b1 [P, H], w2 [P, 4, H], b2 [P, 4], all float32 and finite.
    `QuadrotorPolicy.linear(w, b)` builds the H = 0 form."""

    def __init__(self, w1, b1, w2, b2):
        w1, b1, w2, b2 = f32_array("w1", w1, 3), f32_array("b1", b1, 2), f32_array("w2", w2, 3), f32_array("b2", b2, 2)
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

    @classmethod
    def linear(cls, w, b):
        """a = b + w @ x in the order of the definition: w [P, 4, D], b [P, 4]."""
        w, b = f32_array("w", w, 3), f32_array("b", b, 2)
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
        return self

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
        packed = f32_array("packed", packed, 2)
        P = packed.shape[0]
        if obs_dim not in OBS_DIMS or not (0 <= hidden <= MAX_HIDDEN) or packed.shape[1] != param_count(hidden, obs_dim):
            raise ValueError("packed has shape %s, hidden=%d and obs_dim=%d need [P, %d]"
                             % (packed.shape, hidden, obs_dim, param_count(max(hidden, 0), obs_dim)))
        b2 = packed[:, :_HEAD].copy()
        if hidden == 0:
            return cls.linear(packed[:, _HEAD:].reshape(P, obs_dim, 4).transpose(0, 2, 1).copy(), b2)
        rec = packed[:, _HEAD:].reshape(P, hidden, _REC)
        return cls(rec[:, :, :obs_dim].copy(), rec[:, :, obs_dim].copy(), rec[:, :, _W2_AT:].transpose(0, 2, 1).copy(), b2)

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


def _rrecord(hidden, obs_dim):
    return pad4(obs_dim) + pad4(hidden) + 12


def recurrent_param_count(hidden, obs_dim):
    """Floats per packed recurrent policy (what mg_quadrotor_rpolicy_param_count returns): 4 + H (DP + HP + 12), DP and HP
    being D and H rounded up to a multiple of four."""
    if not (1 <= int(hidden) <= MAX_RECURRENT_HIDDEN):
        raise ValueError("hidden units must be in [1, %d], got %r" % (MAX_RECURRENT_HIDDEN, hidden))
    if obs_dim not in OBS_DIMS:
        raise ValueError("the observation has 16 entries (19 for velocity_control), got %r" % (obs_dim,))
    return _HEAD + int(hidden) * _rrecord(hidden, obs_dim)


class QuadrotorPolicyState(ContinuousPolicyState):
    """The carry of a recurrent closed-loop rollout (`ContinuousPolicyState` with four actions): h float32 [N, H], prev_action
    float32 [N, 4] (unclamped), prev_reward float32 [N], prev_done uint8 [N]. `QuadrotorPolicyState.zeros(N, H, device)` is
    the fresh carry."""
    __slots__ = ("h", "prev_action", "prev_reward", "prev_done")

    def __init__(self, h, prev_action, prev_reward, prev_done):
        self.h, self.prev_action, self.prev_reward, self.prev_done = h, prev_action, prev_reward, prev_done

    @classmethod
    def zeros(cls, num_envs, hidden, device=None):
        """The fresh carry: zeros everywhere. device None: numpy arrays."""
        N, H = int(num_envs), int(hidden)
        if N < 1 or not (1 <= H <= MAX_RECURRENT_HIDDEN):
            raise ValueError("a carry needs num_envs >= 1 and hidden in [1, %d], got %d and %d" % (MAX_RECURRENT_HIDDEN, N, H))
        return cls(*cls._zero_arrays(N, H, 4, device))


class QuadrotorRecurrentPolicy(PackedPolicySet):
    """P recurrent policies: wx [P, H, D], wa [P, H, 4], wr [P, H], wd [P, H], wh [P, H, H], b [P, H], wo [P, 4, H], bo [P, 4],
    all float32 and finite. 1 <= H <= 64, D = 16, or 19 for velocity_control."""

    def __init__(self, wx, wa, wr, wd, wh, b, wo, bo):
        wx, wa, wr, wd = f32_array("wx", wx, 3), f32_array("wa", wa, 3), f32_array("wr", wr, 2), f32_array("wd", wd, 2)
        wh, b, wo, bo = f32_array("wh", wh, 3), f32_array("b", b, 2), f32_array("wo", wo, 3), f32_array("bo", bo, 2)
        P, H, D = wx.shape
        if P < 1:
            raise ValueError("a policy set needs at least one policy")
        if not (1 <= H <= MAX_RECURRENT_HIDDEN):
            raise ValueError("hidden units must be in [1, %d], got %d" % (MAX_RECURRENT_HIDDEN, H))
        if D not in OBS_DIMS:
            raise ValueError("the observation has 16 entries (19 for velocity_control), wx has %d" % D)
        if wa.shape != (P, H, 4) or wr.shape != (P, H) or wd.shape != (P, H) or wh.shape != (P, H, H) or b.shape != (P, H) or \
                wo.shape != (P, 4, H) or bo.shape != (P, 4):
            raise ValueError("shapes must be wx [P,H,D], wa [P,H,4], wr [P,H], wd [P,H], wh [P,H,H], b [P,H], wo [P,4,H], bo [P,4]; "
                             "got %s %s %s %s %s %s %s %s" % (wx.shape, wa.shape, wr.shape, wd.shape, wh.shape, b.shape, wo.shape,
                                                              bo.shape))
        self.wx, self.wa, self.wr, self.wd, self.wh, self.b, self.wo, self.bo = wx, wa, wr, wd, wh, b, wo, bo
        self.num_policies, self.hidden, self.obs_dim = P, H, D

    @property
    def param_count(self):
        return recurrent_param_count(self.hidden, self.obs_dim)

    def pack(self):
        """float32 [P, param_count]: the layout the kernel reads (documented in include/metagym_hip.h). bo[0..3], then per
        hidden unit j a record of DP + HP + 12 floats (DP, HP: D, H rounded up to a multiple of 4): wx[j][0..D-1], zeros up
        to DP; b[j], wr[j], wd[j], 0; wa[j][0..3]; wh[j][0..H-1], zeros up to HP; wo[0..3][j]. Every piece starts on a
        multiple of four floats, so every 16-byte read is aligned."""
        P, H, D = self.num_policies, self.hidden, self.obs_dim
        DP, HP = pad4(D), pad4(H)
        out = np.zeros((P, self.param_count), np.float32)
        out[:, :_HEAD] = self.bo
        rec = out[:, _HEAD:].reshape(P, H, _rrecord(H, D))
        rec[:, :, :D] = self.wx
        rec[:, :, DP] = self.b
        rec[:, :, DP + 1] = self.wr
        rec[:, :, DP + 2] = self.wd
        rec[:, :, DP + 4:DP + 8] = self.wa
        rec[:, :, DP + 8:DP + 8 + H] = self.wh
        rec[:, :, DP + 8 + HP:] = self.wo.transpose(0, 2, 1)
        return out

    @classmethod
    def unpack(cls, packed, hidden, obs_dim):
        """The inverse of `pack`."""
        packed = f32_array("packed", packed, 2)
        P, H, D = packed.shape[0], int(hidden), obs_dim
        if packed.shape[1] != recurrent_param_count(H, D):
            raise ValueError("packed has shape %s, hidden=%d and obs_dim=%d need [P, %d]"
                             % (packed.shape, H, D, recurrent_param_count(H, D)))
        DP, HP = pad4(D), pad4(H)
        rec = packed[:, _HEAD:].reshape(P, H, _rrecord(H, D))
        return cls(rec[:, :, :D].copy(), rec[:, :, DP + 4:DP + 8].copy(), rec[:, :, DP + 1].copy(), rec[:, :, DP + 2].copy(),
                   rec[:, :, DP + 8:DP + 8 + H].copy(), rec[:, :, DP].copy(), rec[:, :, DP + 8 + HP:].transpose(0, 2, 1).copy(),
                   packed[:, :_HEAD].copy())

    def reference(self, obs, policy_ids, state):
        """One step of the definition above in numpy float32, with exactly that association: the sums run one term at a
        time over arrays of envs (x units), as in `QuadrotorPolicy.reference`. obs float32 [N, D], policy_ids [N], state a
        `QuadrotorPolicyState` (read, never written). Returns (actions float32 [N, 4], new state): the new state is a numpy
        carry with h = hn and prev_action = the actions; its prev_reward and prev_done are still the old ones, since they
        come from the env step that follows (`QuadrotorPolicyState.observed`). The oracle of the policy half of a
        recurrent closed-loop rollout."""
        x = to_numpy(obs)
        ids = to_numpy(policy_ids)
        P, H, D = self.num_policies, self.hidden, self.obs_dim
        if x.dtype != np.float32 or x.ndim != 2 or x.shape[1] != D:
            raise ValueError("obs must be float32 [N, %d], got %s %s" % (D, x.dtype, x.shape))
        N = x.shape[0]
        if ids.shape != (N,) or ids.dtype.kind not in "iu":
            raise ValueError("policy_ids must be %d integers" % N)
        if N and (int(ids.min()) < 0 or int(ids.max()) >= P):
            raise ValueError("policy_ids must be in [0, %d)" % P)
        h, pa, pr, pd = to_numpy(state.h), to_numpy(state.prev_action), to_numpy(state.prev_reward), to_numpy(state.prev_done)
        if h.shape != (N, H) or h.dtype != np.float32:
            raise ValueError("state.h must be float32 [%d, %d], got %s %s" % (N, H, h.dtype, h.shape))
        if pa.shape != (N, 4) or pa.dtype != np.float32 or pr.shape != (N,) or pr.dtype != np.float32 or pd.shape != (N,):
            raise ValueError("state.prev_action (float32 [N, 4]) / prev_reward (float32 [N]) / prev_done ([N]) for N = %d" % N)
        pdf = (pd != 0).astype(np.float32)
        wx, wa, wr, wd, wh, b = self.wx[ids], self.wa[ids], self.wr[ids], self.wd[ids], self.wh[ids], self.b[ids]
        wo = self.wo[ids]
        one = np.float32(1.0)
        hn = np.empty((N, H), np.float32)
        a = self.bo[ids].copy()                            # [N, 4]
        with np.errstate(all="ignore"):
            for j in range(H):
                z = b[:, j].copy()
                for i in range(D):
                    z = z + wx[:, j, i] * x[:, i]
                for k in range(4):
                    z = z + wa[:, j, k] * pa[:, k]
                z = z + wr[:, j] * pr
                z = z + wd[:, j] * pdf
                for i in range(H):
                    z = z + wh[:, j, i] * h[:, i]
                hn[:, j] = np.where(z > one, one, np.where(z < -one, -one, z))
            for j in range(H):
                a = a + wo[:, :, j] * hn[:, j:j + 1]
        assert a.dtype == np.float32 and a.shape == (N, 4) and hn.dtype == np.float32
        return a, QuadrotorPolicyState(hn, a.copy(), pr.astype(np.float32), (pd != 0).astype(np.uint8))


class PolicyRollout(object):
    """What `Quadrotor.rollout_policy` returns. Always: ret_total f64 [N] (the T float64 rewards added in step order),
    ret_episode f64 [N] (the rewards up to and including the first done), episode_len int32 [N] (steps added into
    ret_episode; T if the env was never done). With record=True also actions [T,N,4] (unclamped), obs [T,N,D],
    reward [T,N], reward64 [T,N], done [T,N] bool, failed [T,N] uint8; otherwise those are None. state: the end carry
    (a `QuadrotorPolicyState`) of a call with a `QuadrotorRecurrentPolicy`, else None."""
    __slots__ = ("ret_total", "ret_episode", "episode_len", "actions", "obs", "reward", "reward64", "done", "failed", "state")

    def __init__(self, ret_total, ret_episode, episode_len, actions=None, obs=None, reward=None, reward64=None, done=None,
                 failed=None, state=None):
        self.ret_total, self.ret_episode, self.episode_len = ret_total, ret_episode, episode_len
        self.actions, self.obs, self.reward, self.reward64, self.done, self.failed = actions, obs, reward, reward64, done, failed
        self.state = state
