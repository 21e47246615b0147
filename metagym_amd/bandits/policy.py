"""Recurrent bandit policies for `Bandits.rollout_policy`: P small recurrent networks from the env's previous action, reward
and done to one of the K arms, evaluated inside the rollout launch (include/metagym_hip.h, mg_bandits_policy_rollout).

The arithmetic is defined exactly, so the closed loop can be replayed bit for bit. K arms (2 <= K <= 64), H hidden units
(1 <= H <= 64). The bandit has no observation: the input of an env at a step is its previous action (-1: none), the previous
reward as the float32 the reward record holds, and the previous done. Every operation is float32, rounded once, never fused,
in this order (h: the recurrent state before the step):

    for j in 0..H-1:  z = b[j]
                      if prev_action >= 0: z = z + wa[j][prev_action]
                      z = z + wr[j] * prev_reward
                      z = z + wd[j] * (prev_done ? 1 : 0)
                      for i in 0..H-1: z = z + wh[j][i] * h[i]
                      hn[j] = z > 1 ? 1 : (z < -1 ? -1 : z)
    h = hn
    for k in 0..K-1:  l[k] = bo[k];  for j in 0..H-1: l[k] = l[k] + wo[k][j] * h[j]
    greedy = 0;  for k in 1..K-1: if l[k] > l[greedy]: greedy = k

The one-hot of the previous action is a lookup (one add, or none), not K multiply-adds: that is part of the definition (a
pre-activation of -0 stays -0 whatever wa holds). A NaN stays NaN, -0 stays -0; ties and NaN logits resolve to the lowest
index. Exploration is integer arithmetic only: thr[p] = min(floor(epsilon[p] * 2^32), 2^32 - 1); for env e at carry step n,
out = philox4x32_10(c0 = e, c1 = n & 0xFFFFFFFF, c2 = n >> 32, c3 = 0x4241, k0 = seed & 0xFFFFFFFF, k1 = seed >> 32) and
action = (out[0] < thr) ? (out[1] % K) : greedy, with an unsigned modulo.

A set with `temperature` (float32 [P], finite and > 0) SAMPLES its action from softmax(l / temperature) instead of taking the
argmax, by a Gumbel-max draw that is defined bit for bit (so a recorded trajectory has a likelihood, and still replays). The
host computes inv_t[p] = float32(1) / float32(temperature[p]) in numpy float32 (a set whose inv_t is not finite or not > 0 is
refused); the kernel receives inv_t. The logits are exactly the ones above, in that order. For env e at carry step n and arm k:

    out = philox4x32_10(c0 = e, c1 = n & 0xFFFFFFFF, c2 = n >> 32, c3 = 0x53000000 | (k >> 2), k0, k1 as above)
    u = u01(out[k & 3]);  g = -log32(-log32(u));  score[k] = l[k] * inv_t + g      (one multiply, then one add)
    action = 0; best = score[0]; for k >= 1: if score[k] > best: action = k, best = score[k]

with `u01` and `log32` the bandit learners' (learner.py writes them out; _policy.py holds them). One Philox block serves four
arms, so K arms draw ceil(K / 4) blocks. g is finite, in [-2.8116, 16.6356], and within 5.32e-7 of the float64 Gumbel value.
With `epsilon` as well, the exploration draw is made as above and overrides the sampled action. Without `temperature` nothing
changes. `BanditPolicyNet` (policy_net.py) is the same network as a torch module, for the gradient of a recorded rollout.

`BanditPolicy.reference` evaluates exactly this in numpy float32 and numpy integers. Nothing here needs a GPU to import. The
carry is the maze policies' (metamaze/policy.py); the Philox function and the threshold rule are shared (_policy.py).

    pol = BanditPolicy(wa, wr, wd, wh, b, wo, bo)           # wa [P, H, K], wr wd b [P, H], wh [P, H, H], wo [P, K, H], bo [P, K]
    res = env.rollout_policy(pol, steps=256)                # env e plays policy e % P; res.regret is the per-env regret
    res = env.rollout_policy(pol, steps=256, state=res.state)   # and goes on, memory kept
"""
import numpy as np

from .._policy import PackedPolicySet, check_epsilon, check_temperature, f32_array, pad4, philox4x32_10, sample_actions, to_numpy
from ..metamaze.policy import MazePolicyState

MAX_HIDDEN = 64
MAX_ARMS = 64
PHILOX_TAG = 0x4241          # c3 of the exploration draw

BanditPolicyState = MazePolicyState   # h [N, H], prev_action [N] (-1 = none), prev_reward [N], prev_done [N], step


def param_count(hidden, arms):
    """Floats per packed policy (what mg_bandits_policy_param_count returns)."""
    if not (1 <= int(hidden) <= MAX_HIDDEN):
        raise ValueError("hidden units must be in [1, %d], got %r" % (MAX_HIDDEN, hidden))
    if not (2 <= int(arms) <= MAX_ARMS):
        raise ValueError("arms must be in [2, %d], got %r" % (MAX_ARMS, arms))
    H, K = int(hidden), int(arms)
    return H * (4 + pad4(K) + pad4(H)) + K * (4 + pad4(H))


class BanditPolicy(PackedPolicySet):
    """P recurrent policies: wa [P, H, K], wr [P, H], wd [P, H], wh [P, H, H], b [P, H], wo [P, K, H], bo [P, K], all float32
    and finite; epsilon float64 [P] in [0, 1] or None (no exploration); temperature float32 [P], finite and > 0, or None (the
    greedy action, not a sampled one). 1 <= H <= 64, 2 <= K <= 64."""

    def __init__(self, wa, wr, wd, wh, b, wo, bo, epsilon=None, temperature=None):
        wa, wr, wd, wh = f32_array("wa", wa, 3), f32_array("wr", wr, 2), f32_array("wd", wd, 2), f32_array("wh", wh, 3)
        b, wo, bo = f32_array("b", b, 2), f32_array("wo", wo, 3), f32_array("bo", bo, 2)
        P, H, K = wa.shape
        if P < 1:
            raise ValueError("a policy set needs at least one policy")
        if not (1 <= H <= MAX_HIDDEN):
            raise ValueError("hidden units must be in [1, %d], got %d" % (MAX_HIDDEN, H))
        if not (2 <= K <= MAX_ARMS):
            raise ValueError("arms must be in [2, %d], got %d" % (MAX_ARMS, K))
        if wr.shape != (P, H) or wd.shape != (P, H) or wh.shape != (P, H, H) or b.shape != (P, H) or wo.shape != (P, K, H) \
                or bo.shape != (P, K):
            raise ValueError("shapes must be wa [P,H,K], wr [P,H], wd [P,H], wh [P,H,H], b [P,H], wo [P,K,H], bo [P,K]; "
                             "got %s %s %s %s %s %s %s" % (wa.shape, wr.shape, wd.shape, wh.shape, b.shape, wo.shape, bo.shape))
        self.wa, self.wr, self.wd, self.wh, self.b, self.wo, self.bo = wa, wr, wd, wh, b, wo, bo
        self.epsilon = None if epsilon is None else check_epsilon(epsilon, P)
        self.temperature = None if temperature is None else check_temperature(temperature, P)
        self.num_policies, self.hidden, self.arms = P, H, K

    @property
    def param_count(self):
        return param_count(self.hidden, self.arms)

    def pack(self):
        """float32 [P, param_count]: the layout the kernel reads (documented in include/metagym_hip.h). With HP and KP = H
        and K rounded up to a multiple of 4: per hidden unit j a record of RU = 4 + KP + HP floats (b[j], wr[j], wd[j], 0,
        wa[j][0..K-1], zeros up to KP, wh[j][0..H-1], zeros up to HP), then per arm k a record of RA = 4 + HP floats (bo[k],
        0, 0, 0, wo[k][0..H-1], zeros up to HP). Every record is a multiple of four floats, so every 16-byte read is
        aligned."""
        P, H, K = self.num_policies, self.hidden, self.arms
        kp, hp = pad4(K), pad4(H)
        ru, ra = 4 + kp + hp, 4 + hp
        out = np.zeros((P, self.param_count), np.float32)
        unit = out[:, :H * ru].reshape(P, H, ru)
        unit[:, :, 0], unit[:, :, 1], unit[:, :, 2] = self.b, self.wr, self.wd
        unit[:, :, 4:4 + K] = self.wa
        unit[:, :, 4 + kp:4 + kp + H] = self.wh
        arm = out[:, H * ru:].reshape(P, K, ra)
        arm[:, :, 0] = self.bo
        arm[:, :, 4:4 + H] = self.wo
        return out

    @classmethod
    def unpack(cls, packed, hidden, arms, epsilon=None, temperature=None):
        """The inverse of `pack`."""
        packed = f32_array("packed", packed, 2)
        P, H, K = packed.shape[0], int(hidden), int(arms)
        if packed.shape[1] != param_count(H, K):
            raise ValueError("packed has shape %s, hidden=%d and arms=%d need [P, %d]" % (packed.shape, H, K, param_count(H, K)))
        kp, hp = pad4(K), pad4(H)
        ru, ra = 4 + kp + hp, 4 + hp
        unit = packed[:, :H * ru].reshape(P, H, ru)
        arm = packed[:, H * ru:].reshape(P, K, ra)
        return cls(unit[:, :, 4:4 + K].copy(), unit[:, :, 1].copy(), unit[:, :, 2].copy(), unit[:, :, 4 + kp:4 + kp + H].copy(),
                   unit[:, :, 0].copy(), arm[:, :, 4:4 + H].copy(), arm[:, :, 0].copy(), epsilon, temperature)

    def _host(self):
        """`to(device)` gives (packed parameters, thresholds or None); the thresholds travel as the int32 tensor with the
        uint32's bits."""
        return self.pack(), self._threshold_bits()

    def reference(self, policy_ids, state, seed=0, env_ids=None, return_explored=False, return_logits=False):
        """One step of the definition above in numpy float32 (and numpy integers for the exploration), with exactly that
        association: the sums run over i and j one term at a time, each term an array over the envs (and the units or arms,
        which are independent of each other). policy_ids [N]; state: a `BanditPolicyState` (its h, prev_action, prev_reward,
        prev_done and step are read; nothing is written); env e draws with counter c0 = env_ids[e] (default e). Returns
        (actions int32 [N], next h float32 [N, H]), and with `return_explored` also the bool [N] mask of the envs whose
        action was the exploratory draw, and with `return_logits` last the float32 [N, K] logits. A set with a temperature
        draws the action from its scores (the module docstring) where a set without takes the greedy one. The oracle of the
        policy half of a closed-loop rollout."""
        P, H, K = self.num_policies, self.hidden, self.arms
        ids = to_numpy(policy_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("policy_ids must be a vector of integers")
        N = ids.shape[0]
        if N and (int(ids.min()) < 0 or int(ids.max()) >= P):
            raise ValueError("policy_ids must be in [0, %d)" % P)
        h = to_numpy(state.h)
        pa, pr, pd = to_numpy(state.prev_action), to_numpy(state.prev_reward), to_numpy(state.prev_done)
        if h.shape != (N, H) or h.dtype != np.float32:
            raise ValueError("state.h must be float32 [%d, %d], got %s %s" % (N, H, h.dtype, h.shape))
        if pa.shape != (N,) or pr.shape != (N,) or pd.shape != (N,) or pr.dtype != np.float32:
            raise ValueError("state.prev_action / prev_reward (float32) / prev_done must have shape (%d,)" % N)
        if N and (int(pa.min()) < -1 or int(pa.max()) >= K):
            raise ValueError("state.prev_action must be in [-1, %d)" % K)
        wa, wr, wd, wh = self.wa[ids], self.wr[ids], self.wd[ids], self.wh[ids]
        b, wo, bo = self.b[ids], self.wo[ids], self.bo[ids]
        one = np.float32(1.0)
        with np.errstate(all="ignore"):
            z = b.copy()                                     # [N, H]: unit j in column j
            has = pa >= 0
            looked = wa[np.arange(N), :, np.where(has, pa, 0)]
            z = np.where(has[:, None], z + looked, z)
            z = z + wr * pr[:, None]
            z = z + wd * (pd != 0).astype(np.float32)[:, None]
            for i in range(H):
                z = z + wh[:, :, i] * h[:, i:i + 1]
            hn = np.where(z > one, one, np.where(z < -one, -one, z))
            logits = bo.copy()                               # [N, K]
            for j in range(H):
                logits = logits + wo[:, :, j] * hn[:, j:j + 1]
            greedy = np.zeros(N, np.int32)
            best = logits[:, 0].copy()
            for k in range(1, K):
                better = logits[:, k] > best
                greedy = np.where(better, np.int32(k), greedy)
                best = np.where(better, logits[:, k], best)
        assert hn.dtype == np.float32 and logits.dtype == np.float32
        thr = self.thresholds[ids]
        e = np.arange(N, dtype=np.uint64) if env_ids is None else to_numpy(env_ids).astype(np.uint64)
        n, s = int(state.step), int(seed)
        if self.temperature is not None:
            greedy = sample_actions(logits, self.inv_temperature[ids], e, n, s)
        out = philox4x32_10(e, n & 0xFFFFFFFF, (n >> 32) & 0xFFFFFFFF, PHILOX_TAG, s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF)
        explored = out[0] < thr
        actions = np.where(explored, (out[1] % np.uint32(K)).astype(np.int32), greedy).astype(np.int32)
        return (actions, hn) + ((explored,) if return_explored else ()) + ((logits,) if return_logits else ())


class BanditsPolicyRollout(object):
    """What `Bandits.rollout_policy` returns. Always: ret_total f64 [N] (the rewards of the steps the env took, added in step
    order), ret_episode f64 [N] (the rewards up to and including the first done), episode_len int32 [N] (steps added into
    ret_episode; 0 for an env that was over from the start), episodes int32 [N] (the number of steps with done), regret f64
    [N] (the sum over the steps the env took of best - gain: the best expected gain of the task in force minus the chosen
    arm's) and state (the end carry, a `BanditPolicyState`). With record=True also, each [T, N]: actions int32 (-1 where the
    env was over), reward float32, done bool, info_steps int32, expected_gain f64, best_gain f64 and invalid uint8 (2 where
    the env was over); otherwise those are None."""
    __slots__ = ("ret_total", "ret_episode", "episode_len", "episodes", "regret", "state", "actions", "reward", "done",
                 "info_steps", "expected_gain", "best_gain", "invalid")

    def __init__(self, ret_total, ret_episode, episode_len, episodes, regret, state, actions=None, reward=None, done=None,
                 info_steps=None, expected_gain=None, best_gain=None, invalid=None):
        self.ret_total, self.ret_episode, self.episode_len, self.episodes = ret_total, ret_episode, episode_len, episodes
        self.regret, self.state = regret, state
        self.actions, self.reward, self.done, self.info_steps = actions, reward, done, info_steps
        self.expected_gain, self.best_gain, self.invalid = expected_gain, best_gain, invalid
