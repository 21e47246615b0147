"""Bandits (reference metagym/bandits/bandits_env.py) for N envs at once, stepped by `mg_bandits_step` on the GPU."""
import numpy as np

from .. import _lib
from ..spaces import Discrete

# name -> MG_BANDITS_* code
DISTRIBUTIONS = {"Classical": 1, "Uniform": 2, "Gaussian": 3}
REC = 625   # u32 words of one stream record: 624 key words, pos


def classical_lo_hi(K, mean, dev):
    """The two values of a Classical task (every arm lo, one arm hi), in the reference's float64 order and clipped."""
    fac = np.sqrt(K - 1)
    lo, hi = np.clip(np.array([mean - dev / fac, mean + fac * dev]), 0.0, 1.0)
    return float(lo), float(hi)


def _distribution(name):
    if name not in DISTRIBUTIONS:
        raise Exception("No such distribution_settings: %s", name)
    return DISTRIBUTIONS[name]


class Bandits(object):
    """`num_envs` K-armed Bernoulli bandits: the reference's Bandits(arms, max_steps), each env on its own numpy legacy
    stream, numpy.random.seed(seed + e) or seeds[e] (32-bit values).

    Env e's sequence of sample_task / set_task / reset / step calls reproduces, bit for bit, the reference's single env run
    after numpy.random.seed(that seed) with the same calls: gains, rewards, done, info and the final stream state. The one
    semantic addition: the reference's "Uniform" and "Gaussian" distributions raise; here they are what its docstring
    intends, Uniform = clip((random_sample(K) - 0.5) * 3.464 + mean, 0, 1) and Gaussian = clip(normal(mean, dev, K), 0, 1)
    (legacy gauss; its cached second value carries into the next draw). Gaussian gains may differ from numpy's by up to
    2 ulp (the device's log); every draw count is exact.

    auto_reset: an env whose episode ends restarts inside the same launch; with resample_task (a distribution name, or a
    (name, mean, dev) tuple) it first draws its next task from its own stream (the reference's sample_task(); set_task();
    reset()). step() never synchronises with the host (graph-capturable) unless check=True. Outputs live in persistent
    buffers, overwritten by the next step; copy_outputs=True returns copies. There is no CPU path.
    """

    def __init__(self, num_envs=1, arms=10, max_steps=5000, device="cuda", seed=0, seeds=None, auto_reset=False,
                 resample_task=None, copy_outputs=False):
        import torch
        self.max_steps = max_steps
        self.action_space = Discrete(arms)
        self.observation_space = None
        self.K = arms
        assert self.K > 1 and self.max_steps > 1
        if self.K >= 2 ** 31 or self.max_steps >= 2 ** 31:
            raise ValueError("arms and max_steps must fit int32")
        if torch.device(device).type != "cuda":
            raise _lib.MetaGymHipError("metagym_amd runs on an AMD GPU only (got device %r); there is no CPU fallback"
                                       % (device,))
        self.device = _lib.canonical_device(device)
        self.num_envs = N = int(num_envs)
        if N <= 0:
            raise ValueError("num_envs must be positive")
        self.auto_reset = bool(auto_reset)
        if resample_task is None or isinstance(resample_task, str):
            resample_task = None if resample_task is None else (resample_task, 0.5, 0.05)
        self.resample_task = None if resample_task is None else \
            (resample_task[0], float(resample_task[1]), float(resample_task[2]))
        if self.resample_task is not None:
            _distribution(self.resample_task[0])
        self.copy_outputs = bool(copy_outputs)
        self._lib = _lib.load()
        dev = self.device
        self.mt = torch.empty(N, REC, dtype=torch.int32, device=dev)          # u32 words
        self.has_gauss = torch.zeros(N, dtype=torch.int32, device=dev)
        self.gauss = torch.zeros(N, dtype=torch.float64, device=dev)
        self.gains = torch.zeros(N, self.K, dtype=torch.float64, device=dev)
        self.steps = torch.zeros(N, dtype=torch.int32, device=dev)
        self.over = torch.ones(N, dtype=torch.uint8, device=dev)               # need_reset
        self.has_task = False
        self.reward = torch.zeros(N, dtype=torch.float32, device=dev)
        self.done = torch.zeros(N, dtype=torch.bool, device=dev)
        self.info_steps = torch.zeros(N, dtype=torch.int32, device=dev)
        self.expected_gain = torch.zeros(N, dtype=torch.float64, device=dev)
        self.invalid = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._state = _lib.BanditsState(*[t.data_ptr() for t in (self.mt, self.has_gauss, self.gauss, self.gains,
                                                                   self.steps, self.over)])
        self.seed(seed, seeds)

    # ------------------------------------------------------------------ plumbing
    def _cfg(self, distribution=None, mean=0.5, dev=0.05):
        c = _lib.BanditsConfig()
        c.arms, c.max_steps, c.auto_reset = self.K, self.max_steps, int(self.auto_reset)
        if distribution is not None:
            c.distribution = _distribution(distribution)
            c.mean, c.dev = float(mean), float(dev)
            c.classical_lo, c.classical_hi = classical_lo_hi(self.K, c.mean, c.dev)
        return c

    def _stream(self):
        return _lib.current_stream(self.device)

    def _mask(self, mask):
        import torch
        if mask is None:
            return None
        m = torch.as_tensor(mask, device=self.device)
        if tuple(m.shape) != (self.num_envs,):
            raise ValueError("mask must have shape [%d]" % self.num_envs)
        return (m != 0).to(torch.uint8).contiguous()

    def _actions(self, action, T=None):
        import torch
        a = torch.as_tensor(action, device=self.device)
        shape = (self.num_envs,) if T is None else (T, self.num_envs)
        if a.dim() == 0 and T is None:
            a = a.expand(self.num_envs)
        if tuple(a.shape) != shape:
            raise ValueError("actions must have shape %s" % (list(shape),))
        if a.dtype != torch.int32:
            a = a.to(torch.int32)
        return a.contiguous()

    # ------------------------------------------------------------------ seeding and streams
    def seed(self, seed=0, seeds=None):
        """numpy.random.seed(seed + e) or seeds[e] for every env e (32-bit values); clears the gauss cache."""
        import torch
        N = self.num_envs
        seeds_t = None
        if seeds is not None:
            arr = np.asarray(seeds.cpu().numpy() if hasattr(seeds, "cpu") else seeds, dtype=np.int64)
            if arr.shape != (N,) or arr.min() < 0 or arr.max() >= 2 ** 32:
                raise ValueError("seeds must be %d values in [0, 2^32)" % N)
            seeds_t = torch.from_numpy(arr.astype(np.uint32).view(np.int32)).to(self.device)
            seed = 0
        if not (0 <= int(seed) and int(seed) + N <= 2 ** 32):
            raise ValueError("seeds are 32-bit (numpy.random.seed's integer range): need 0 <= seed and seed + N <= 2^32")
        rc = self._lib.mg_bandits_seed(N, int(seed), _lib.ptr(seeds_t), self._state, self._stream())
        _lib.check(rc, "mg_bandits_seed")
        return [seed] if seeds is None else list(seeds)

    def rng_state(self):
        """Every env's stream: {"mt": int32 [N, 625] (u32 key words, pos), "has_gauss": [N], "gauss": [N]} (copies)."""
        return {"mt": self.mt.clone(), "has_gauss": self.has_gauss.clone(), "gauss": self.gauss.clone()}

    def set_rng_state(self, st):
        self.mt.copy_(st["mt"])
        self.has_gauss.copy_(st["has_gauss"])
        self.gauss.copy_(st["gauss"])

    def numpy_state(self, e):
        """Env e's stream as numpy.random.get_state() spells it: ('MT19937', key, pos, has_gauss, cached_gaussian)."""
        rec = self.mt[e].cpu().numpy().view(np.uint32)
        return ("MT19937", rec[:624].copy(), int(rec[624]), int(self.has_gauss[e].item()), float(self.gauss[e].item()))

    def set_numpy_state(self, e, st):
        """Continue env e from a numpy.random.get_state() tuple (`set_numpy_state(0, numpy.random.get_state())` makes env 0
        the continuation of the global stream)."""
        import torch
        if st[0] != "MT19937":
            raise ValueError("not an MT19937 state")
        key = np.asarray(st[1], dtype=np.uint32)
        if key.shape != (624,) or not 0 <= int(st[2]) <= 624:
            raise ValueError("an MT19937 state has 624 key words and 0 <= pos <= 624")
        rec = np.empty(REC, np.uint32)
        rec[:624] = key
        rec[624] = int(st[2])
        self.mt[e].copy_(torch.from_numpy(rec.view(np.int32)))
        self.has_gauss[e] = int(st[3]) if len(st) > 3 else 0
        self.gauss[e] = float(st[4]) if len(st) > 4 else 0.0

    # ------------------------------------------------------------------ the reference's interface
    def sample_task(self, distribution_settings="Classical", mean=0.50, dev=0.05, mask=None):
        """One task per env (envs outside `mask` draw nothing and keep their row of the current gains): a device float64
        [N, K] tensor to hand to set_task."""
        cfg = self._cfg(distribution_settings, mean, dev)
        out = self.gains.clone()
        rc = self._lib.mg_bandits_sample_task(cfg, self.num_envs, self._state, _lib.ptr(self._mask(mask)), _lib.ptr(out),
                                              self._stream())
        _lib.check(rc, "mg_bandits_sample_task")
        return out

    def set_task(self, task_config, mask=None):
        """Gains [K] (every env) or [N, K]; the envs set must be reset before they step, as in the reference."""
        import torch
        g = torch.as_tensor(task_config, dtype=torch.float64, device=self.device)
        if tuple(g.shape) not in ((self.K,), (self.num_envs, self.K)):
            raise AssertionError("task_config must have shape (%d,) or (%d, %d)" % (self.K, self.num_envs, self.K))
        m = self._mask(mask)
        if m is None:
            self.gains.copy_(g.expand(self.num_envs, self.K))
            self.over.fill_(1)
        else:
            sel = m.bool()
            self.gains.copy_(torch.where(sel[:, None], g.expand(self.num_envs, self.K), self.gains))
            self.over.masked_fill_(sel, 1)
        self.has_task = True

    def reset(self, mask=None):
        if not self.has_task:
            raise Exception("Must call \"set_task\" before reset")
        rc = self._lib.mg_bandits_reset(self._cfg(), self.num_envs, self._state, _lib.ptr(self._mask(mask)),
                                         self._stream())
        _lib.check(rc, "mg_bandits_reset")
        return None

    def _launch(self, a, T, reward, done, info_steps, expected_gain, invalid):
        cfg = self._cfg(*(self.resample_task or (None,)))
        rc = self._lib.mg_bandits_step(cfg, self.num_envs, self._state, T, _lib.ptr(a), _lib.ptr(reward), _lib.ptr(done),
                                       _lib.ptr(info_steps), _lib.ptr(expected_gain), _lib.ptr(invalid), self._stream())
        _lib.check(rc, "mg_bandits_step")

    def _raise_invalid(self, invalid, actions):
        inv = invalid.cpu().numpy().reshape(-1)
        bad = np.nonzero(inv)[0]
        if len(bad):
            i = int(bad[0])
            if inv[i] == 2:
                raise Exception("Must \"reset\" before doing any actions (env %d)" % (i % self.num_envs))
            raise IndexError("action %d is out of bounds for %d arms (env %d)"
                             % (int(actions.reshape(-1)[i]), self.K, i % self.num_envs))

    def step(self, action, check=False):
        """One step of every env: (None, reward [N] f32 0/1, done [N] bool, info) with info = {"steps", "expected_gain",
        "invalid"} ([N] each; invalid 1 = action outside [-K, K), 2 = episode over / not reset: that env drew nothing and
        kept its state). check=True reads `invalid` back and raises the reference's exception for the first such env."""
        a = self._actions(action)
        self._launch(a, 1, self.reward, self.done, self.info_steps, self.expected_gain, self.invalid)
        if check:
            self._raise_invalid(self.invalid, a)
        out = (self.reward, self.done, self.info_steps, self.expected_gain, self.invalid)
        if self.copy_outputs:
            out = tuple(t.clone() for t in out)
        reward, done, steps, gain, invalid = out
        return None, reward, done, {"steps": steps, "expected_gain": gain, "invalid": invalid}

    def rollout(self, actions, check=False):
        """T steps of every env in one launch, actions [T, N]: (reward [T, N], done [T, N], info of [T, N] tensors), equal
        to T step() calls."""
        import torch
        a = torch.as_tensor(actions)
        if a.dim() != 2:
            raise ValueError("actions must have shape [T, %d]" % self.num_envs)
        T = int(a.shape[0])
        a = self._actions(a, T)
        N, dev = self.num_envs, self.device
        reward = torch.empty(T, N, dtype=torch.float32, device=dev)
        done = torch.empty(T, N, dtype=torch.bool, device=dev)
        info_steps = torch.empty(T, N, dtype=torch.int32, device=dev)
        gain = torch.empty(T, N, dtype=torch.float64, device=dev)
        invalid = torch.empty(T, N, dtype=torch.uint8, device=dev)
        self._launch(a, T, reward, done, info_steps, gain, invalid)
        if check:
            self._raise_invalid(invalid, a)
        return reward, done, {"steps": info_steps, "expected_gain": gain, "invalid": invalid}

    def expected_upperbound(self):
        """max_steps * max(gains), float64 [N]."""
        return self.max_steps * self.gains.max(dim=1).values

    def state_dict(self):
        return {"mt": self.mt.clone(), "has_gauss": self.has_gauss.clone(), "gauss": self.gauss.clone(),
                "gains": self.gains.clone(), "steps": self.steps.clone(), "over": self.over.clone(),
                "has_task": self.has_task}

    def load_state_dict(self, sd):
        for k in ("mt", "has_gauss", "gauss", "gains", "steps", "over"):
            getattr(self, k).copy_(sd[k])
        self.has_task = bool(sd["has_task"])
