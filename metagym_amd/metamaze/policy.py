"""Recurrent MetaMaze policies for `MetaMaze2D.rollout_policy`: P small recurrent networks from the env's window, its previous
action, reward and done to one of the four moves, evaluated inside the rollout launch (include/metagym_hip.h,
mg_maze2d_policy_rollout).

The arithmetic is defined exactly, so the closed loop can be replayed bit for bit. w = 2 * view_grid + 1 (view_grid 1, 2 or
3), D = w * w + 6 (15, 31 or 55), H hidden units (1 <= H <= 64). The input x[D] of an env at a step is its current window
row-major (x[0 .. w*w-1], exactly the floats `step` returns, the SURVIVAL life entry in the centre included), the one-hot of
its previous action (x[w*w + k] = prev_action == k, prev_action = -1: none), the previous reward as the float32 the reward
record holds (x[w*w + 4]) and the previous done (x[w*w + 5]). Every operation is float32, rounded once, never fused, in this
order (h: the recurrent state before the step):

    for j in 0..H-1:  z = b[j]
                      for i in 0..D-1: z = z + wx[j][i] * x[i]
                      for i in 0..H-1: z = z + wh[j][i] * h[i]
                      hn[j] = z > 1 ? 1 : (z < -1 ? -1 : z)
    h = hn
    for k in 0..3:    l[k] = bo[k];  for j in 0..H-1: l[k] = l[k] + wo[k][j] * h[j]
    greedy = 0;  for k in 1..3: if l[k] > l[greedy]: greedy = k

A NaN pre-activation stays NaN, -0 stays -0; ties and NaN logits resolve to the lowest index. Exploration is integer
arithmetic only: thr[p] = min(floor(epsilon[p] * 2^32), 2^32 - 1); for env e at carry step n,
out = philox4x32_10(c0 = e, c1 = n & 0xFFFFFFFF, c2 = n >> 32, c3 = 0x4D5A, k0 = seed & 0xFFFFFFFF, k1 = seed >> 32) and
action = (out[0] < thr) ? (out[1] & 3) : greedy.

`MazePolicy.reference` evaluates exactly this in numpy float32 and numpy integers. Nothing here needs a GPU to import.

    pol = MazePolicy(wx, wh, b, wo, bo)                     # wx [P, H, D], wh [P, H, H], b [P, H], wo [P, 4, H], bo [P, 4]
    res = env.rollout_policy(pol, steps=64)                 # env e plays policy e % P
    res = env.rollout_policy(pol, steps=64, state=res.state)   # and goes on, memory kept
"""
import numpy as np

from .._policy import PackedPolicySet, check_epsilon, eps_threshold, f32_array, philox4x32_10, to_numpy  # noqa: F401

MAX_HIDDEN = 64
VIEW_GRIDS = (1, 2, 3)
PHILOX_TAG = 0x4D5A          # c3 of the exploration draw


def input_dim(view_grid):
    """D = w * w + 6 for view_grid in {1, 2, 3}."""
    if view_grid not in VIEW_GRIDS:
        raise ValueError("view_grid must be 1, 2 or 3, got %r" % (view_grid,))
    w = 2 * int(view_grid) + 1
    return w * w + 6


_VIEW_OF_DIM = {input_dim(v): v for v in VIEW_GRIDS}


def _record(hidden, d):
    return d + 1 + ((hidden + 3) & ~3) + 4


def param_count(hidden, view_grid):
    """Floats per packed policy (what mg_maze2d_policy_param_count returns)."""
    if not (1 <= int(hidden) <= MAX_HIDDEN):
        raise ValueError("hidden units must be in [1, %d], got %r" % (MAX_HIDDEN, hidden))
    return 4 + int(hidden) * _record(int(hidden), input_dim(view_grid))


class MazePolicyState(object):
    """The carry of a closed-loop rollout, the policy's memory of each env: h float32 [N, H], prev_action int32 [N] (-1 =
    none), prev_reward float32 [N], prev_done uint8 [N], and `step`, the Python int n of the exploration counter, which
    advances by T per call. The arrays are torch tensors on the env's device (or numpy arrays, for `reference`)."""
    __slots__ = ("h", "prev_action", "prev_reward", "prev_done", "step")

    def __init__(self, h, prev_action, prev_reward, prev_done, step=0):
        self.h, self.prev_action, self.prev_reward, self.prev_done, self.step = h, prev_action, prev_reward, prev_done, int(step)

    @classmethod
    def zeros(cls, num_envs, hidden, device=None):
        """The fresh carry: zeros everywhere, prev_action = -1, step = 0. device None: numpy arrays."""
        N, H = int(num_envs), int(hidden)
        if device is None:
            return cls(np.zeros((N, H), np.float32), np.full(N, -1, np.int32), np.zeros(N, np.float32), np.zeros(N, np.uint8))
        import torch
        return cls(torch.zeros(N, H, dtype=torch.float32, device=device), torch.full((N,), -1, dtype=torch.int32, device=device),
                   torch.zeros(N, dtype=torch.float32, device=device), torch.zeros(N, dtype=torch.uint8, device=device))

    @property
    def num_envs(self):
        return int(self.h.shape[0])

    @property
    def hidden(self):
        return int(self.h.shape[1])

    def clone(self):
        c = (lambda v: v.clone()) if hasattr(self.h, "clone") else (lambda v: v.copy())
        return MazePolicyState(c(self.h), c(self.prev_action), c(self.prev_reward), c(self.prev_done), self.step)

    def numpy(self):
        """The same carry on the host, as numpy arrays."""
        return MazePolicyState(to_numpy(self.h).astype(np.float32), to_numpy(self.prev_action).astype(np.int32),
                               to_numpy(self.prev_reward).astype(np.float32), to_numpy(self.prev_done).astype(np.uint8), self.step)


class MazePolicy(PackedPolicySet):
    """P recurrent policies: wx [P, H, D], wh [P, H, H], b [P, H], wo [P, 4, H], bo [P, 4], all float32 and finite; epsilon
    float64 [P] in [0, 1] or None (no exploration). 1 <= H <= 64, D = (2 view_grid + 1)^2 + 6 with view_grid in {1, 2, 3}."""

    def __init__(self, wx, wh, b, wo, bo, epsilon=None):
        wx, wh, b = f32_array("wx", wx, 3), f32_array("wh", wh, 3), f32_array("b", b, 2)
        wo, bo = f32_array("wo", wo, 3), f32_array("bo", bo, 2)
        P, H, D = wx.shape
        if P < 1:
            raise ValueError("a policy set needs at least one policy")
        if not (1 <= H <= MAX_HIDDEN):
            raise ValueError("hidden units must be in [1, %d], got %d" % (MAX_HIDDEN, H))
        if D not in _VIEW_OF_DIM:
            raise ValueError("the input has (2 view_grid + 1)^2 + 6 = 15, 31 or 55 entries, wx has %d" % D)
        if wh.shape != (P, H, H) or b.shape != (P, H) or wo.shape != (P, 4, H) or bo.shape != (P, 4):
            raise ValueError("shapes must be wx [P,H,D], wh [P,H,H], b [P,H], wo [P,4,H], bo [P,4]; got %s %s %s %s %s"
                             % (wx.shape, wh.shape, b.shape, wo.shape, bo.shape))
        self.wx, self.wh, self.b, self.wo, self.bo = wx, wh, b, wo, bo
        self.epsilon = None if epsilon is None else check_epsilon(epsilon, P)
        self.num_policies, self.hidden, self.input_dim, self.view_grid = P, H, D, _VIEW_OF_DIM[D]

    @property
    def param_count(self):
        return param_count(self.hidden, self.view_grid)

    def pack(self):
        """float32 [P, param_count]: the layout the kernel reads (documented in include/metagym_hip.h). bo[0..3], then per
        hidden unit j a record of R = D + 1 + HP + 4 floats (HP = H rounded up to a multiple of 4): wx[j][0..D-1], b[j],
        wh[j][0..H-1], zeros up to HP, wo[0..3][j]. D + 1 is a multiple of 4, so every 16-byte read is aligned."""
        P, H, D = self.num_policies, self.hidden, self.input_dim
        R = _record(H, D)
        out = np.zeros((P, self.param_count), np.float32)
        out[:, :4] = self.bo
        rec = out[:, 4:].reshape(P, H, R)
        rec[:, :, :D] = self.wx
        rec[:, :, D] = self.b
        rec[:, :, D + 1:D + 1 + H] = self.wh
        rec[:, :, R - 4:] = self.wo.transpose(0, 2, 1)
        return out

    @classmethod
    def unpack(cls, packed, hidden, view_grid, epsilon=None):
        """The inverse of `pack`."""
        packed = f32_array("packed", packed, 2)
        P, H, D = packed.shape[0], int(hidden), input_dim(view_grid)
        if packed.shape[1] != param_count(H, view_grid):
            raise ValueError("packed has shape %s, hidden=%d and view_grid=%d need [P, %d]"
                             % (packed.shape, H, view_grid, param_count(H, view_grid)))
        R = _record(H, D)
        rec = packed[:, 4:].reshape(P, H, R)
        return cls(rec[:, :, :D].copy(), rec[:, :, D + 1:D + 1 + H].copy(), rec[:, :, D].copy(),
                   rec[:, :, R - 4:].transpose(0, 2, 1).copy(), packed[:, :4].copy(), epsilon)

    def _host(self):
        """`to(device)` gives (packed parameters, thresholds or None); the thresholds travel as the int32 tensor with the
        uint32's bits."""
        return self.pack(), self._threshold_bits()

    def reference(self, obs, policy_ids, state, seed=0, env_ids=None, return_explored=False):
        """One step of the definition above in numpy float32 (and numpy integers for the exploration), with exactly that
        association. obs: the windows, float32 [N, w, w] (or [N, w*w]); policy_ids [N]; state: a `MazePolicyState` (its h,
        prev_action, prev_reward, prev_done and step are read; nothing is written); env e draws with counter c0 =
        env_ids[e] (default e). Returns (actions int32 [N], next h float32 [N, H]), and with `return_explored` also the bool
        [N] mask of the envs whose action was the exploratory draw. The oracle of the policy half of a closed-loop rollout."""
        P, H, D = self.num_policies, self.hidden, self.input_dim
        ww = D - 6
        win = to_numpy(obs)
        ids = to_numpy(policy_ids)
        if win.dtype != np.float32 or win.ndim not in (2, 3) or int(np.prod(win.shape[1:])) != ww:
            raise ValueError("obs must be float32 [N, %d] windows, got %s %s" % (ww, win.dtype, win.shape))
        N = win.shape[0]
        win = win.reshape(N, ww)
        if ids.shape != (N,) or ids.dtype.kind not in "iu":
            raise ValueError("policy_ids must be %d integers" % N)
        if N and (int(ids.min()) < 0 or int(ids.max()) >= P):
            raise ValueError("policy_ids must be in [0, %d)" % P)
        h = to_numpy(state.h)
        pa, pr, pd = to_numpy(state.prev_action), to_numpy(state.prev_reward), to_numpy(state.prev_done)
        if h.shape != (N, H) or h.dtype != np.float32:
            raise ValueError("state.h must be float32 [%d, %d], got %s %s" % (N, H, h.dtype, h.shape))
        if pa.shape != (N,) or pr.shape != (N,) or pd.shape != (N,) or pr.dtype != np.float32:
            raise ValueError("state.prev_action / prev_reward (float32) / prev_done must have shape (%d,)" % N)
        x = np.zeros((N, D), np.float32)
        x[:, :ww] = win
        for k in range(4):
            x[:, ww + k] = (pa == k).astype(np.float32)
        x[:, ww + 4] = pr
        x[:, ww + 5] = (pd != 0).astype(np.float32)
        wx, wh, b, wo, bo = self.wx[ids], self.wh[ids], self.b[ids], self.wo[ids], self.bo[ids]
        one = np.float32(1.0)
        hn = np.empty((N, H), np.float32)
        with np.errstate(all="ignore"):
            for j in range(H):
                z = b[:, j].copy()
                for i in range(D):
                    z = z + wx[:, j, i] * x[:, i]
                for i in range(H):
                    z = z + wh[:, j, i] * h[:, i]
                hn[:, j] = np.where(z > one, one, np.where(z < -one, -one, z))
            logits = bo.copy()                               # [N, 4]
            for j in range(H):
                logits = logits + wo[:, :, j] * hn[:, j:j + 1]
            greedy = np.zeros(N, np.int32)
            best = logits[:, 0].copy()
            for k in range(1, 4):
                better = logits[:, k] > best
                greedy = np.where(better, np.int32(k), greedy)
                best = np.where(better, logits[:, k], best)
        assert hn.dtype == np.float32 and logits.dtype == np.float32
        thr = self.thresholds[ids]
        e = np.arange(N, dtype=np.uint64) if env_ids is None else to_numpy(env_ids).astype(np.uint64)
        n, s = int(state.step), int(seed)
        out = philox4x32_10(e, n & 0xFFFFFFFF, (n >> 32) & 0xFFFFFFFF, PHILOX_TAG, s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF)
        explored = out[0] < thr
        actions = np.where(explored, (out[1] & np.uint32(3)).astype(np.int32), greedy).astype(np.int32)
        return (actions, hn, explored) if return_explored else (actions, hn)


class MazePolicyRollout(object):
    """What `MetaMaze2D.rollout_policy` returns. Always: ret_total f64 [N] (the T float64 rewards added in step order),
    ret_episode f64 [N] (the rewards up to and including the first done), episode_len int32 [N] (steps added into
    ret_episode; T if the env was never done), episodes int32 [N] (the number of steps with done), state (the end carry, a
    `MazePolicyState`), obs and obs_steps (the observations kept and their step indices: the env's persistent [N, w, w]
    buffer after the last step, or with obs_every >= 1 a fresh [K, N, w, w] tensor). With record=True also actions int32
    [T, N], reward float32 [T, N], reward64 float64 [T, N], done bool [T, N]; otherwise those are None."""
    __slots__ = ("ret_total", "ret_episode", "episode_len", "episodes", "state", "actions", "reward", "reward64", "done", "obs",
                 "obs_steps")

    def __init__(self, ret_total, ret_episode, episode_len, episodes, state, obs, obs_steps, actions=None, reward=None,
                 reward64=None, done=None):
        self.ret_total, self.ret_episode, self.episode_len, self.episodes = ret_total, ret_episode, episode_len, episodes
        self.state, self.obs, self.obs_steps = state, obs, obs_steps
        self.actions, self.reward, self.reward64, self.done = actions, reward, reward64, done
