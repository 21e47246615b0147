"""`MazePolicyNet`: ONE policy of a `MazePolicy` set as a `torch.nn.Module`, for the gradient of a recorded rollout.

    net = MazePolicyNet.from_policy(pol)                                        # policy 0 of the set
    obs0 = env_obs.clone()                                                      # the observation standing before the call
    res = env.rollout_policy(net.to_policy(temperature=1.0), steps=T, record=True, obs_every=1)
    logits = net.replay(obs0, res.obs, res.actions, res.reward, res.done)      # [T, N, 4], differentiable
"""
import torch

from .._policy_net import RecurrentPolicyNet, log_prob, one_temperature  # noqa: F401
from .policy import MazePolicy


class MazePolicyNet(RecurrentPolicyNet):
    """The network of metamaze/policy.py with its weights as parameters: wx [H, D], wh [H, H], b [H], wo [4, H], bo [4]."""

    def __init__(self, hidden, view_grid):
        super().__init__()
        H, w = int(hidden), 2 * int(view_grid) + 1
        self.hidden, self.view_grid, self.input_dim = H, int(view_grid), w * w + 6
        for name, shape in (("wx", (H, w * w + 6)), ("wh", (H, H)), ("b", (H,)), ("wo", (4, H)), ("bo", (4,))):
            setattr(self, name, torch.nn.Parameter(torch.zeros(shape, dtype=torch.float32)))

    @classmethod
    def from_policy(cls, policy, index=0):
        """The net of policy `index` of a `MazePolicy` set (float32 parameters, copied)."""
        if not isinstance(policy, MazePolicy):
            raise TypeError("policy must be a MazePolicy, got %s" % type(policy).__name__)
        net = cls(policy.hidden, policy.view_grid)
        with torch.no_grad():
            for name, p in net.named_parameters():
                p.copy_(torch.from_numpy(getattr(policy, name)[index]))
        return net

    def to_policy(self, epsilon=None, temperature=None):
        """The P = 1 `MazePolicy` of the current weights (as float32), with `epsilon` (float64 [1]) and `temperature`
        (float32 [1], or a number) as given."""
        w = self._weights()
        return MazePolicy(w["wx"], w["wh"], w["b"], w["wo"], w["bo"], epsilon, one_temperature(temperature))

    def _drive(self, window, prev_action, prev_reward, prev_done):
        one_hot = (prev_action[:, None] == torch.arange(4, device=prev_action.device)).to(window.dtype)
        x = torch.cat([window, one_hot, prev_reward[:, None], prev_done[:, None]], dim=1)
        return self.b + x @ self.wx.t()

    def replay(self, obs0, obs, actions, reward, done, state0=None, episodic=False, auto_reset=True):
        """The logits [T, N, 4] of the T recorded steps of N envs, differentiable: obs0 float32 [N, w, w], the observation
        standing before the call; obs float32 [T, N, w, w], the `obs_every=1` record (the window after every step);
        actions int [T, N], reward float32 [T, N], done bool [T, N] as `MetaMaze2D.rollout_policy(record=True)` returns
        them; `state0` the carry the launch started from (None = a fresh one), `episodic` as it was passed to the launch
        and `auto_reset` as the env was built. Runs in the parameters' dtype on their device."""
        dev, dtype = self.wh.device, self.wh.dtype
        obs0 = torch.as_tensor(obs0, device=dev).to(dtype)
        obs = torch.as_tensor(obs, device=dev).to(dtype)
        T, N = obs.shape[0], obs.shape[1]
        ww = self.input_dim - 6
        if obs0.numel() != N * ww or obs.numel() != T * N * ww:
            raise ValueError("obs0 must be [N, w, w] and obs [T, N, w, w] with w = %d" % (2 * self.view_grid + 1))
        windows = torch.cat([obs0.reshape(1, N, ww), obs.reshape(T, N, ww)[:T - 1]])   # the window step t was chosen on
        return self._replay(windows, actions, reward, done, state0, episodic, auto_reset)
