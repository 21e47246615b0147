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

A set with `temperature` (float32 [P], finite and > 0) SAMPLES its action from softmax(l / temperature) instead, by the
Gumbel-max draw bandits/policy.py defines bit for bit: inv_t[p] = float32(1) / float32(temperature[p]) on the host (refused
when not finite or not > 0), one Philox block with c3 = 0x53000000 for the four moves, u = u01(out[k]), g = -log32(-log32(u)),
score[k] = l[k] * inv_t + g (one multiply, then one add), the lowest index among the maxima of the scores. With `epsilon` as
well, the exploration draw is made as above and overrides the sampled action. Without `temperature` nothing changes.
`MazePolicyNet` (policy_net.py) is the same network as a torch module, for the gradient of a recorded rollout.

`MazePolicy.reference` evaluates exactly this in numpy float32 and numpy integers. Nothing here needs a GPU to import.

    pol = MazePolicy(wx, wh, b, wo, bo)                     # wx [P, H, D], wh [P, H, H], b [P, H], wo [P, 4, H], bo [P, 4]
    res = env.rollout_policy(pol, steps=64)                 # env e plays policy e % P
    res = env.rollout_policy(pol, steps=64, state=res.state)   # and goes on, memory kept
"""
import numpy as np

from .._policy import (ContinuousPolicyState, PackedPolicySet, check_epsilon, check_temperature, eps_threshold, f32_array,  # noqa: F401
                       philox4x32_10, sample_actions, to_numpy)

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
    float64 [P] in [0, 1] or None (no exploration); temperature float32 [P], finite and > 0, or None (the greedy action, not
    a sampled one). 1 <= H <= 64, D = (2 view_grid + 1)^2 + 6 with view_grid in {1, 2, 3}."""

    def __init__(self, wx, wh, b, wo, bo, epsilon=None, temperature=None):
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
        self.temperature = None if temperature is None else check_temperature(temperature, P)
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
    def unpack(cls, packed, hidden, view_grid, epsilon=None, temperature=None):
        """The inverse of `pack`."""
        packed = f32_array("packed", packed, 2)
        P, H, D = packed.shape[0], int(hidden), input_dim(view_grid)
        if packed.shape[1] != param_count(H, view_grid):
            raise ValueError("packed has shape %s, hidden=%d and view_grid=%d need [P, %d]"
                             % (packed.shape, H, view_grid, param_count(H, view_grid)))
        R = _record(H, D)
        rec = packed[:, 4:].reshape(P, H, R)
        return cls(rec[:, :, :D].copy(), rec[:, :, D + 1:D + 1 + H].copy(), rec[:, :, D].copy(),
                   rec[:, :, R - 4:].transpose(0, 2, 1).copy(), packed[:, :4].copy(), epsilon, temperature)

    def _host(self):
        """`to(device)` gives (packed parameters, thresholds or None); the thresholds travel as the int32 tensor with the
        uint32's bits."""
        return self.pack(), self._threshold_bits()

    def reference(self, obs, policy_ids, state, seed=0, env_ids=None, return_explored=False, return_logits=False):
        """One step of the definition above in numpy float32 (and numpy integers for the exploration), with exactly that
        association. obs: the windows, float32 [N, w, w] (or [N, w*w]); policy_ids [N]; state: a `MazePolicyState` (its h,
        prev_action, prev_reward, prev_done and step are read; nothing is written); env e draws with counter c0 =
        env_ids[e] (default e). Returns (actions int32 [N], next h float32 [N, H]), and with `return_explored` also the bool
        [N] mask of the envs whose action was the exploratory draw, and with `return_logits` last the float32 [N, 4] logits.
        A set with a temperature draws the action from its scores (the module docstring) where a set without takes the
        greedy one. The oracle of the policy half of a closed-loop rollout."""
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
        if self.temperature is not None:
            greedy = sample_actions(logits, self.inv_temperature[ids], e, n, s)
        out = philox4x32_10(e, n & 0xFFFFFFFF, (n >> 32) & 0xFFFFFFFF, PHILOX_TAG, s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF)
        explored = out[0] < thr
        actions = np.where(explored, (out[1] & np.uint32(3)).astype(np.int32), greedy).astype(np.int32)
        return (actions, hn) + ((explored,) if return_explored else ()) + ((logits,) if return_logits else ())


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


# ------------------------------------------------------------------------------------------------ the 3-D mazes
# The policies of the 3-D mazes read the rendered frame (include/metagym_hip.h, mg_maze3d_policy_rollout). The frame
# F[h][v][c] (int32 or uint8, as `step` returns it) is pooled over a grid (Gh, Gv) that divides the resolution, bh = res_h / Gh,
# bv = res_v / Gv: S[gh][gv][c] is the sum of the block modulo 2^32 read as int32, x[(gh * Gv + gv) * 3 + c] = float32(S) * scale
# with scale = np.float32(1.0 / (255 * bh * bv)). After the 3 * Gh * Gv features come, discrete: the one-hot of the previous
# action, the previous reward and done (D = 3 Gh Gv + 6); continuous: the two previous actions as recorded, the previous reward
# and done (D = 3 Gh Gv + 4). The network is the one above with K = 4 logits or K = 2 steering outputs
# a[k] = l[k] != l[k] ? 0 : clamp(l[k], -1, 1); the discrete exploration draw uses c3 = 0x4D33.
MAX_GRID = 16
PHILOX_TAG_3D = 0x4D33       # c3 of the 3-D exploration draw


def check_grid(grid):
    """(Gh, Gv) as two ints in [1, 16]."""
    try:
        gh, gv = grid
    except (TypeError, ValueError):
        raise ValueError("grid must be a pair (Gh, Gv), got %r" % (grid,))
    if int(gh) != gh or int(gv) != gv or not (1 <= gh <= MAX_GRID and 1 <= gv <= MAX_GRID):
        raise ValueError("grid sides must be integers in [1, %d], got %r" % (MAX_GRID, grid))
    return int(gh), int(gv)


def check_grid_divides(grid, resolution):
    """(bh, bv) of a grid on frames of `resolution` = (res_h, res_v); ValueError when it does not divide them."""
    gh, gv = check_grid(grid)
    res_h, res_v = int(resolution[0]), int(resolution[1])
    if res_h < 1 or res_v < 1 or res_h % gh or res_v % gv:
        raise ValueError("grid %d x %d does not divide the resolution %d x %d" % (gh, gv, res_h, res_v))
    return res_h // gh, res_v // gv


def pool_scale(bh, bv):
    """np.float32(1.0 / (255 * bh * bv)): what the kernel multiplies a block sum with."""
    return np.float32(1.0 / (255 * int(bh) * int(bv)))


def pool_reference(frames, grid):
    """The features of [N, res_h, res_v, 3] int32 or uint8 frames: float32 [N, Gh, Gv, 3], block sums modulo 2^32 read as
    int32, converted to float32 (round to nearest even) and multiplied by `pool_scale(bh, bv)`."""
    f = to_numpy(frames)
    if f.ndim != 4 or f.shape[3] != 3 or f.dtype not in (np.dtype(np.int32), np.dtype(np.uint8)):
        raise ValueError("frames must be int32 or uint8 [N, res_h, res_v, 3], got %s %s" % (f.dtype, f.shape))
    gh, gv = check_grid(grid)
    bh, bv = check_grid_divides(grid, f.shape[1:3])
    N = f.shape[0]
    s = f.astype(np.int64).reshape(N, gh, bh, gv, bv, 3).sum(axis=(2, 4))         # exact: at most 2^16 terms below 2^32
    s = (s & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return s.astype(np.float32) * pool_scale(bh, bv)


def _input_dim_3d(grid, continuous):
    return 3 * grid[0] * grid[1] + (4 if continuous else 6)


def param_count_3d(hidden, grid, continuous):
    """Floats per packed 3-D policy (what mg_maze3d_policy_param_count returns)."""
    if not (1 <= int(hidden) <= MAX_HIDDEN):
        raise ValueError("hidden units must be in [1, %d], got %r" % (MAX_HIDDEN, hidden))
    gh, gv = check_grid(grid)
    H, K = int(hidden), 2 if continuous else 4
    return 4 + ((H + 3) & ~3) * (1 + _input_dim_3d((gh, gv), continuous) + H + K)


class Maze3DPolicyState(ContinuousPolicyState):
    """The carry of `MetaMazeContinuous3D.rollout_policy` (`ContinuousPolicyState` with A = 2): h float32 [N, H], prev_action
    float32 [N, 2] (the actions as recorded), prev_reward float32 [N], prev_done uint8 [N]. `Maze3DPolicyState(num_envs,
    hidden, device)` is the fresh carry, all zero; device None gives numpy arrays, for `Maze3DSteerPolicy.reference`."""
    __slots__ = ("h", "prev_action", "prev_reward", "prev_done")

    def __init__(self, num_envs, hidden, device=None):
        N, H = int(num_envs), int(hidden)
        if N < 1 or not (1 <= H <= MAX_HIDDEN):
            raise ValueError("a carry needs num_envs >= 1 and hidden in [1, %d], got %d and %d" % (MAX_HIDDEN, N, H))
        self.h, self.prev_action, self.prev_reward, self.prev_done = self._zero_arrays(N, H, 2, device)


class _Maze3DPolicyBase(PackedPolicySet):
    """What the two 3-D policy classes share: the shapes, the packed layout and the network on a batch."""
    CONTINUOUS = False

    def _init(self, wx, wh, b, wo, bo, grid):
        K = 2 if self.CONTINUOUS else 4
        wx, wh, b = f32_array("wx", wx, 3), f32_array("wh", wh, 3), f32_array("b", b, 2)
        wo, bo = f32_array("wo", wo, 3), f32_array("bo", bo, 2)
        gh, gv = check_grid(grid)
        P, H, D = wx.shape
        if P < 1:
            raise ValueError("a policy set needs at least one policy")
        if not (1 <= H <= MAX_HIDDEN):
            raise ValueError("hidden units must be in [1, %d], got %d" % (MAX_HIDDEN, H))
        if D != _input_dim_3d((gh, gv), self.CONTINUOUS):
            raise ValueError("grid %d x %d gives %d inputs, wx has %d" % (gh, gv, _input_dim_3d((gh, gv), self.CONTINUOUS), D))
        if wh.shape != (P, H, H) or b.shape != (P, H) or wo.shape != (P, K, H) or bo.shape != (P, K):
            raise ValueError("shapes must be wx [P,H,D], wh [P,H,H], b [P,H], wo [P,%d,H], bo [P,%d]; got %s %s %s %s %s"
                             % (K, K, wx.shape, wh.shape, b.shape, wo.shape, bo.shape))
        self.wx, self.wh, self.b, self.wo, self.bo = wx, wh, b, wo, bo
        self.num_policies, self.hidden, self.input_dim, self.grid, self.n_out = P, H, D, (gh, gv), K

    @property
    def param_count(self):
        return param_count_3d(self.hidden, self.grid, self.CONTINUOUS)

    def pack(self):
        """float32 [P, param_count]: the j-minor layout the kernel reads (written out in include/metagym_hip.h). With HS = H
        rounded up to a multiple of 4: bo[0..K-1] and zeros up to 4, then rows of HS floats: b, wx[:, 0] .. wx[:, D-1],
        wh[:, 0] .. wh[:, H-1], wo[0] .. wo[K-1]; entries j >= H are zero."""
        P, H, D, K = self.num_policies, self.hidden, self.input_dim, self.n_out
        HS = (H + 3) & ~3
        out = np.zeros((P, self.param_count), np.float32)
        out[:, :K] = self.bo
        rows = out[:, 4:].reshape(P, 1 + D + H + K, HS)
        rows[:, 0, :H] = self.b
        rows[:, 1:1 + D, :H] = self.wx.transpose(0, 2, 1)
        rows[:, 1 + D:1 + D + H, :H] = self.wh.transpose(0, 2, 1)
        rows[:, 1 + D + H:, :H] = self.wo
        return out

    @classmethod
    def _unpack(cls, packed, hidden, grid):
        packed = f32_array("packed", packed, 2)
        gh, gv = check_grid(grid)
        P, H, K = packed.shape[0], int(hidden), 2 if cls.CONTINUOUS else 4
        D = _input_dim_3d((gh, gv), cls.CONTINUOUS)
        if packed.shape[1] != param_count_3d(H, (gh, gv), cls.CONTINUOUS):
            raise ValueError("packed has shape %s, hidden=%d and grid=%s need [P, %d]"
                             % (packed.shape, H, (gh, gv), param_count_3d(H, (gh, gv), cls.CONTINUOUS)))
        HS = (H + 3) & ~3
        rows = packed[:, 4:].reshape(P, 1 + D + H + K, HS)
        return (rows[:, 1:1 + D, :H].transpose(0, 2, 1).copy(), rows[:, 1 + D:1 + D + H, :H].transpose(0, 2, 1).copy(),
                rows[:, 0, :H].copy(), rows[:, 1 + D + H:, :H].copy(), packed[:, :K].copy())

    def _features(self, frames, N):
        f = to_numpy(frames)
        if f.ndim != 4 or f.shape[0] != N:
            raise ValueError("frames must be [N = %d, res_h, res_v, 3], got %s" % (N, f.shape))
        return pool_reference(f, self.grid).reshape(N, -1)

    def _network(self, x, ids, h):
        """(hn [N, H], l [N, K]) of the definition, numpy float32 with exactly its association."""
        N, D = x.shape
        H, K = self.hidden, self.n_out
        assert D == self.input_dim and x.dtype == np.float32
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
            out = bo.copy()                                  # [N, K]
            for j in range(H):
                out = out + wo[:, :, j] * hn[:, j:j + 1]
        assert hn.dtype == np.float32 and out.dtype == np.float32
        return hn, out

    def _check_batch(self, policy_ids, state, prev_action_shape):
        ids = to_numpy(policy_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("policy_ids must be [N] integers")
        N, P, H = ids.shape[0], self.num_policies, self.hidden
        if N and (int(ids.min()) < 0 or int(ids.max()) >= P):
            raise ValueError("policy_ids must be in [0, %d)" % P)
        h = to_numpy(state.h)
        pa, pr, pd = to_numpy(state.prev_action), to_numpy(state.prev_reward), to_numpy(state.prev_done)
        if h.shape != (N, H) or h.dtype != np.float32:
            raise ValueError("state.h must be float32 [%d, %d], got %s %s" % (N, H, h.dtype, h.shape))
        if pa.shape != (N,) + prev_action_shape or pr.shape != (N,) or pd.shape != (N,) or pr.dtype != np.float32:
            raise ValueError("state.prev_action %s / prev_reward (float32) / prev_done must have %d rows" % (prev_action_shape, N))
        return ids, h, pa, pr, pd


class Maze3DPolicy(_Maze3DPolicyBase):
    """P recurrent policies of the discrete 3-D maze: wx [P, H, D], wh [P, H, H], b [P, H], wo [P, 4, H], bo [P, 4], all
    float32 and finite; grid = (Gh, Gv), sides in [1, 16], D = 3 Gh Gv + 6; epsilon float64 [P] in [0, 1] or None (no
    exploration). 1 <= H <= 64. The carry is a `MazePolicyState`."""
    CONTINUOUS = False

    def __init__(self, wx, wh, b, wo, bo, grid, epsilon=None):
        self._init(wx, wh, b, wo, bo, grid)
        self.epsilon = None if epsilon is None else check_epsilon(epsilon, self.num_policies)

    @classmethod
    def unpack(cls, packed, hidden, grid, epsilon=None):
        """The inverse of `pack`."""
        return cls(*cls._unpack(packed, hidden, grid), grid=grid, epsilon=epsilon)

    def _host(self):
        return self.pack(), self._threshold_bits()

    def reference(self, frames, policy_ids, state, seed=0, env_ids=None, return_explored=False):
        """One step of the definition in numpy. frames: int32 or uint8 [N, res_h, res_v, 3], the frames of the states the envs
        hold; policy_ids [N]; state: a `MazePolicyState` (read, not written); env e draws with counter c0 = env_ids[e]
        (default e). Returns (actions int32 [N], next h float32 [N, H]), with `return_explored` also the bool [N] mask of
        the exploratory draws."""
        ids, h, pa, pr, pd = self._check_batch(policy_ids, state, ())
        N, D = ids.shape[0], self.input_dim
        x = np.zeros((N, D), np.float32)
        x[:, :D - 6] = self._features(frames, N)
        for k in range(4):
            x[:, D - 6 + k] = (pa == k).astype(np.float32)
        x[:, D - 2] = pr
        x[:, D - 1] = (pd != 0).astype(np.float32)
        hn, logits = self._network(x, ids, h)
        greedy = np.zeros(N, np.int32)
        best = logits[:, 0].copy()
        with np.errstate(all="ignore"):
            for k in range(1, 4):
                better = logits[:, k] > best
                greedy = np.where(better, np.int32(k), greedy)
                best = np.where(better, logits[:, k], best)
        thr = self.thresholds[ids]
        e = np.arange(N, dtype=np.uint64) if env_ids is None else to_numpy(env_ids).astype(np.uint64)
        n, s = int(state.step), int(seed)
        out = philox4x32_10(e, n & 0xFFFFFFFF, (n >> 32) & 0xFFFFFFFF, PHILOX_TAG_3D, s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF)
        explored = out[0] < thr
        actions = np.where(explored, (out[1] & np.uint32(3)).astype(np.int32), greedy).astype(np.int32)
        return (actions, hn, explored) if return_explored else (actions, hn)


class Maze3DSteerPolicy(_Maze3DPolicyBase):
    """P recurrent policies of the continuous 3-D maze: wx [P, H, D], wh [P, H, H], b [P, H], wo [P, 2, H], bo [P, 2], all
    float32 and finite; grid = (Gh, Gv), sides in [1, 16], D = 3 Gh Gv + 4; no exploration. 1 <= H <= 64. The carry is a
    `Maze3DPolicyState`."""
    CONTINUOUS = True
    epsilon = None

    def __init__(self, wx, wh, b, wo, bo, grid):
        self._init(wx, wh, b, wo, bo, grid)

    @classmethod
    def unpack(cls, packed, hidden, grid):
        """The inverse of `pack`."""
        return cls(*cls._unpack(packed, hidden, grid), grid=grid)

    def reference(self, frames, policy_ids, state):
        """One step of the definition in numpy. frames: int32 or uint8 [N, res_h, res_v, 3]; policy_ids [N]; state: a
        `Maze3DPolicyState` (read, not written). Returns (actions float32 [N, 2] = (turn, walk), next h float32 [N, H])."""
        ids, h, pa, pr, pd = self._check_batch(policy_ids, state, (2,))
        if pa.dtype != np.float32:
            raise ValueError("state.prev_action must be float32, got %s" % pa.dtype)
        N, D = ids.shape[0], self.input_dim
        x = np.zeros((N, D), np.float32)
        x[:, :D - 4] = self._features(frames, N)
        x[:, D - 4:D - 2] = pa
        x[:, D - 2] = pr
        x[:, D - 1] = (pd != 0).astype(np.float32)
        hn, out = self._network(x, ids, h)
        one = np.float32(1.0)
        with np.errstate(all="ignore"):
            a = np.where(out != out, np.float32(0.0), np.where(out > one, one, np.where(out < -one, -one, out)))
        return a.astype(np.float32), hn
