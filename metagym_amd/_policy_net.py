"""The torch side of the softmax-sampled discrete policies (bandits, MetaMaze 2-D): what `BanditPolicyNet` and
`MazePolicyNet` share. A net holds the weights of ONE policy of a set as parameters and replays the [T, N] records of a
`rollout_policy(record=True)` launch through the same network in ordinary torch ops, so the logits of every recorded step
come back with autograd attached; `log_prob` turns them into the log-likelihood of the recorded actions. The launch samples
(csrc/mg_sample.h), the replay differentiates: policy gradients need nothing else. This is not hot-path code.

The replay rebuilds every step's inputs from the records exactly as the kernel carries them: the previous action is a lookup
(-1: none), the previous reward is the float32 the record holds, the memory h survives a done (or is cleared with
`episodic`, at a done with `auto_reset`), and an env that was over at a step (recorded action -1) keeps its carry. The sums
are torch's (a matrix product), not the definition's term-by-term order: the logits equal `reference`'s to rounding, and
exactly when every sum is exact."""
import numpy as np
import torch

from ._policy import to_numpy


def log_prob(logits, actions, temperature):
    """log softmax(logits / temperature) at the recorded actions: logits [..., K], actions integers [...] (-1 = the env was
    over: the entry is 0 and carries no gradient), temperature a float or a tensor that broadcasts against logits[..., 0].
    Returns [...] in the logits' dtype."""
    t = torch.as_tensor(temperature, dtype=logits.dtype, device=logits.device)
    lp = torch.log_softmax(logits / t.unsqueeze(-1), dim=-1)
    a = torch.as_tensor(actions, device=logits.device).long()
    took = a >= 0
    picked = lp.gather(-1, a.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    return torch.where(took, picked, torch.zeros_like(picked))


def one_temperature(temperature):
    """`to_policy`'s temperature argument as float32 [1] (a Python number is taken as is), or None."""
    if temperature is None or np.ndim(temperature) != 0:
        return temperature
    return np.full(1, temperature, np.float32)


class RecurrentPolicyNet(torch.nn.Module):
    """The replay loop. A subclass registers its parameters (among them wh [H, H], wo [K, H], bo [K]) and says in `_drive`
    what enters a hidden unit besides the memory."""

    def forward(self, *args, **kwargs):
        """`replay`."""
        return self.replay(*args, **kwargs)

    def _weights(self):
        """The parameters as float32 numpy arrays with a leading policy axis of 1, by name."""
        return {k: to_numpy(v)[None].astype(np.float32) for k, v in self.named_parameters()}

    def _replay(self, windows, actions, reward, done, state0, episodic, auto_reset):
        wh = self.wh
        dev, dtype, H = wh.device, wh.dtype, wh.shape[0]
        actions = torch.as_tensor(actions, device=dev).long()
        reward = torch.as_tensor(reward, device=dev).to(dtype)
        done = torch.as_tensor(done, device=dev) != 0
        if actions.dim() != 2 or reward.shape != actions.shape or done.shape != actions.shape:
            raise ValueError("actions, reward and done must be [T, N] records of one launch")
        T, N = actions.shape
        if state0 is None:
            h = torch.zeros(N, H, dtype=dtype, device=dev)
            pa = torch.full((N,), -1, dtype=torch.long, device=dev)
            pr = torch.zeros(N, dtype=dtype, device=dev)
            pd = torch.zeros(N, dtype=torch.bool, device=dev)
        else:
            h = torch.as_tensor(to_numpy(state0.h), device=dev).to(dtype)
            pa = torch.as_tensor(to_numpy(state0.prev_action), device=dev).long()
            pr = torch.as_tensor(to_numpy(state0.prev_reward), device=dev).to(dtype)
            pd = torch.as_tensor(to_numpy(state0.prev_done), device=dev) != 0
            if h.shape != (N, H) or pa.shape != (N,) or pr.shape != (N,) or pd.shape != (N,):
                raise ValueError("state0 must be the carry of %d envs and %d hidden units" % (N, H))
        clear = bool(episodic) and bool(auto_reset)
        out = []
        for t in range(T):
            z = self._drive(None if windows is None else windows[t], pa, pr, pd.to(dtype)) + h @ wh.t()
            hn = z.clamp(-1.0, 1.0)
            out.append(self.bo + hn @ self.wo.t())
            took = actions[t] >= 0                                       # an env that was over is left alone
            fresh = took & done[t] if clear else torch.zeros_like(took)
            h = torch.where((took & ~fresh)[:, None], hn, torch.where(fresh[:, None], torch.zeros_like(h), h))
            pa = torch.where(fresh, torch.full_like(pa, -1), torch.where(took, actions[t], pa))
            pr = torch.where(fresh, torch.zeros_like(pr), torch.where(took, reward[t], pr))
            pd = torch.where(fresh, torch.zeros_like(pd), torch.where(took, done[t], pd))
        return torch.stack(out)
