"""`BanditPolicyNet`: ONE policy of a `BanditPolicy` set as a `torch.nn.Module`, for the gradient of a recorded rollout (RL^2
with policy gradients: roll out a trial in one launch with sampled actions, `replay` the records, `log_prob`, step, repack).

    net = BanditPolicyNet.from_policy(pol)                                     # policy 0 of the set
    res = env.rollout_policy(net.to_policy(temperature=1.0), steps=T, record=True)
    logits = net.replay(res.actions, res.reward, res.done)                     # [T, N, K], differentiable
    loss = -(log_prob(logits, res.actions, 1.0) * advantage).sum()
"""
import torch

from .._policy_net import RecurrentPolicyNet, log_prob, one_temperature  # noqa: F401
from .policy import BanditPolicy


class BanditPolicyNet(RecurrentPolicyNet):
    """The network of bandits/policy.py with its weights as parameters: wa [H, K], wr [H], wd [H], wh [H, H], b [H],
    wo [K, H], bo [K]."""

    def __init__(self, hidden, arms):
        super().__init__()
        H, K = int(hidden), int(arms)
        self.hidden, self.arms = H, K
        for name, shape in (("wa", (H, K)), ("wr", (H,)), ("wd", (H,)), ("wh", (H, H)), ("b", (H,)), ("wo", (K, H)), ("bo", (K,))):
            setattr(self, name, torch.nn.Parameter(torch.zeros(shape, dtype=torch.float32)))

    @classmethod
    def from_policy(cls, policy, index=0):
        """The net of policy `index` of a `BanditPolicy` set (float32 parameters, copied)."""
        if not isinstance(policy, BanditPolicy):
            raise TypeError("policy must be a BanditPolicy, got %s" % type(policy).__name__)
        net = cls(policy.hidden, policy.arms)
        with torch.no_grad():
            for name, p in net.named_parameters():
                p.copy_(torch.from_numpy(getattr(policy, name)[index]))
        return net

    def to_policy(self, epsilon=None, temperature=None):
        """The P = 1 `BanditPolicy` of the current weights (as float32), with `epsilon` (float64 [1]) and `temperature`
        (float32 [1], or a number) as given."""
        w = self._weights()
        return BanditPolicy(w["wa"], w["wr"], w["wd"], w["wh"], w["b"], w["wo"], w["bo"], epsilon, one_temperature(temperature))

    def _drive(self, window, prev_action, prev_reward, prev_done):
        has = prev_action >= 0                                            # the one-hot is a lookup: one add, or none
        looked = self.wa.t()[prev_action.clamp(min=0)]                    # [N, H]
        z = torch.where(has[:, None], self.b + looked, self.b.expand_as(looked))
        return z + self.wr * prev_reward[:, None] + self.wd * prev_done[:, None]

    def replay(self, actions, reward, done, state0=None, episodic=False, auto_reset=True):
        """The logits [T, N, K] of the T recorded steps of N envs, differentiable: actions int [T, N] (-1 where the env was
        over), reward float32 [T, N], done bool [T, N] as `Bandits.rollout_policy(record=True)` returns them; `state0` the
        carry the launch started from (None = a fresh one), `episodic` as it was passed to the launch and `auto_reset` as
        the env was built. Runs in the parameters' dtype on their device."""
        return self._replay(None, actions, reward, done, state0, episodic, auto_reset)
