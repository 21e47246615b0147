"""Bandits (reference metagym/bandits/bandits_env.py) for N envs at once, stepped by `mg_bandits_step` on the GPU."""
import numpy as np

from .. import _lib, _policy
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

    def rollout_policy(self, policy, steps, policy_ids=None, state=None, seed=0, record=False, episodic=False):
        """`steps` closed-loop env steps in ONE launch: env e evaluates policy `policy_ids[e]` of `policy` (a `BanditPolicy`;
        `policy_ids=None` = e % P) on its previous action, reward and done inside the kernel and pulls the arm it chooses
        (bandits/policy.py defines the arithmetic exactly). `state` is the carry of the previous call (a `BanditPolicyState`;
        None = a fresh one); it is not written, the end carry comes back as `.state` of the result with `step` advanced by
        `steps`. `seed` keys the exploration draws of a policy with epsilon and the sampling draws of a policy with a
        temperature (which goes through mg_bandits_policy_rollout_sampled; everything else here is the same). The step is `rollout`'s, draw for draw, with
        `auto_reset` and `resample_task` as the env was built. The policy's memory survives a done (the next step sees
        prev_done = 1 and the ending step's reward and action); `episodic=True` clears the carry at a done with auto_reset
        instead. An env that is over when a step begins (never reset, or finished without auto_reset) does nothing in that
        step: its memory, stream and returns stay, its records are action -1, reward 0, done 0, invalid 2. Returns a
        `BanditsPolicyRollout`: ret_total, ret_episode, episode_len, episodes, regret and state always; actions, reward,
        done, info_steps, expected_gain, best_gain, invalid [steps, N] when `record=True`, else None (the launch then writes
        nothing per step). Nothing synchronises when `policy_ids` is None, a host array, or the device tensor of the previous
        call (the same object, unchanged; any other device tensor is read back once to validate it), so after
        `policy.to(device)` the call can be captured in a hipGraph. A refused call (a policy of another K, an id out of range,
        a carry of another N or H, steps < 1) raises and launches nothing."""
        from .policy import BanditPolicy, BanditPolicyState
        if not isinstance(policy, BanditPolicy):
            raise TypeError("policy must be a BanditPolicy, got %s" % type(policy).__name__)
        T, N, dev, P, H = int(steps), self.num_envs, self.device, policy.num_policies, policy.hidden
        if T < 1:
            raise ValueError("steps must be at least 1, got %d" % T)
        if policy.arms != self.K:
            raise ValueError("the policy was built for %d arms, the env has %d" % (policy.arms, self.K))
        state, seed = _policy.check_discrete_carry(state, BanditPolicyState, N, H, T, seed, dev)
        ids_d = _policy.policy_ids(self, policy_ids, P)
        params, thr = policy.to(dev)
        inv_t = policy.inv_temperature_on(dev)
        # everything is checked: from here on the env and the new carry are written
        carry = BanditPolicyState(*[v.to(dev).clone().contiguous() for v in (state.h, state.prev_action, state.prev_reward,
                                                                             state.prev_done)], step=state.step + T)
        desc = _lib.BanditsPolicyDesc(params.data_ptr(), thr.data_ptr() if thr is not None else None, P, H, policy.arms)
        carry_c = _lib.BanditsPolicyCarry(carry.h.data_ptr(), carry.prev_action.data_ptr(), carry.prev_reward.data_ptr(),
                                          carry.prev_done.data_ptr())
        res = self._rollout_results(T, record, carry)
        cfg = self._cfg(*(self.resample_task or (None,)))
        head = (cfg, N, self._state, T, desc, _lib.ptr(ids_d), carry_c)
        tail = (seed, state.step, int(bool(episodic)), _lib.ptr(res.ret_total), _lib.ptr(res.ret_episode),
                _lib.ptr(res.episode_len), _lib.ptr(res.episodes), _lib.ptr(res.regret), _lib.ptr(res.actions),
                _lib.ptr(res.reward), _lib.ptr(res.done), _lib.ptr(res.info_steps), _lib.ptr(res.expected_gain),
                _lib.ptr(res.best_gain), _lib.ptr(res.invalid), self._stream())
        if inv_t is None:
            _lib.check(self._lib.mg_bandits_policy_rollout(*(head + tail)), "mg_bandits_policy_rollout")
        else:
            _lib.check(self._lib.mg_bandits_policy_rollout_sampled(*(head + (_lib.ptr(inv_t),) + tail)),
                       "mg_bandits_policy_rollout_sampled")
        return res

    def _rollout_results(self, T, record, carry):
        """The `BanditsPolicyRollout` of a T-step launch, its tensors allocated: the five results always, the seven [T, N]
        records with `record`, else None. `rollout_policy` and `rollout_learner` share it."""
        import torch
        from .policy import BanditsPolicyRollout
        N, dev = self.num_envs, self.device
        f64 = lambda: torch.empty(N, dtype=torch.float64, device=dev)
        i32 = lambda: torch.empty(N, dtype=torch.int32, device=dev)
        res = BanditsPolicyRollout(f64(), f64(), i32(), i32(), f64(), carry)
        if record:
            res.actions = torch.empty(T, N, dtype=torch.int32, device=dev)
            res.reward = torch.empty(T, N, dtype=torch.float32, device=dev)
            res.done = torch.empty(T, N, dtype=torch.bool, device=dev)
            res.info_steps = torch.empty(T, N, dtype=torch.int32, device=dev)
            res.expected_gain = torch.empty(T, N, dtype=torch.float64, device=dev)
            res.best_gain = torch.empty(T, N, dtype=torch.float64, device=dev)
            res.invalid = torch.empty(T, N, dtype=torch.uint8, device=dev)
        return res

    def _learner_call(self, learner, state, learner_ids, seed, T):
        """The checks `rollout_learner` and `learner_scores` share: (state, ids, params, thr, table, desc) or an exception."""
        import torch
        from .learner import KINDS, BanditLearner, BanditLearnerState
        if not isinstance(learner, BanditLearner):
            raise TypeError("learner must be a BanditLearner, got %s" % type(learner).__name__)
        N, K, dev, P = self.num_envs, self.K, self.device, learner.num_learners
        if learner.arms != K:
            raise ValueError("the learner was built for %d arms, the env has %d" % (learner.arms, K))
        if not (0 <= int(seed) < 2 ** 64):
            raise ValueError("seed must be in [0, 2^64), got %d" % int(seed))
        if state is None:
            state = BanditLearnerState.zeros(N, K, dev)
        elif not isinstance(state, BanditLearnerState):
            raise TypeError("state must be a BanditLearnerState, got %s" % type(state).__name__)
        for name in ("pulls", "wins"):
            v = getattr(state, name)
            if not isinstance(v, torch.Tensor) or tuple(v.shape) != (N, K) or v.dtype != torch.int32 or v.device != dev:
                raise ValueError("state.%s must be an int32 tensor of shape (%d, %d) on %s" % (name, N, K, dev))
        if not (0 <= state.step < 2 ** 64 - T):
            raise ValueError("state.step = %d is outside [0, 2^64 - steps)" % state.step)
        ids_d = _policy.policy_ids(self, learner_ids, P, name="learner_ids")
        params, thr, table = learner.to(dev)
        desc = _lib.BanditsLearnerDesc(KINDS[learner.kind], P, K, params.data_ptr(), thr.data_ptr() if thr is not None else None,
                                       table.data_ptr() if table is not None else None, learner.table_cap, learner.max_attempts)
        return state, ids_d, (params, thr, table), desc

    def rollout_learner(self, learner, steps, learner_ids=None, state=None, seed=0, record=False, episodic=True):
        """`steps` pulls of every env in ONE launch with a classical learner inside the kernel: env e plays parameter row
        `learner_ids[e]` of `learner` (a `BanditLearner`: greedy, UCB, an index table or Thompson sampling; None = e % P)
        from its own counts (bandits/learner.py defines the arithmetic exactly, so `BanditLearner.reference` reproduces every
        action). `state` is the carry of the previous call (a `BanditLearnerState`; None = a fresh one); it is not written,
        the end carry comes back as `.state` of the result with `step` advanced by `steps`. `seed` keys the sampler's and the
        exploration draws. The step is `rollout`'s, draw for draw, with `auto_reset` and `resample_task` as the env was
        built. `episodic=True` (the default here: a classical learner must not carry counts into a redrawn task) zeroes an
        env's counts at a done with auto_reset; `episodic=False` keeps them. An env that is over when a step begins does
        nothing in that step, as in `rollout_policy`. Returns a `BanditsLearnerRollout` (the fields of
        `BanditsPolicyRollout`; records [steps, N] only with `record=True`). Nothing synchronises when `learner_ids` is None,
        a host array, or the device tensor of the previous call (the same object, unchanged; any other device tensor is read
        back once to validate it), so after `learner.to(device)` the call can be captured in a hipGraph. The counts
        of `state` must satisfy 0 <= wins <= pulls (`state.validate()` checks; the kernel reads nothing out of bounds
        whatever they hold). A refused call raises and launches nothing."""
        from .learner import BanditLearnerState
        T, N = int(steps), self.num_envs
        if T < 1:
            raise ValueError("steps must be at least 1, got %d" % T)
        state, ids_d, keep, desc = self._learner_call(learner, state, learner_ids, seed, T)
        # everything is checked: from here on the env and the new carry are written
        carry = BanditLearnerState(state.pulls.clone().contiguous(), state.wins.clone().contiguous(), step=state.step + T)
        carry_c = _lib.BanditsLearnerCarry(carry.pulls.data_ptr(), carry.wins.data_ptr())
        res = self._rollout_results(T, record, carry)
        cfg = self._cfg(*(self.resample_task or (None,)))
        rc = self._lib.mg_bandits_learner_rollout(cfg, N, self._state, T, desc, _lib.ptr(ids_d), carry_c, int(seed), state.step,
                                                  int(bool(episodic)), _lib.ptr(res.ret_total), _lib.ptr(res.ret_episode),
                                                  _lib.ptr(res.episode_len), _lib.ptr(res.episodes), _lib.ptr(res.regret),
                                                  _lib.ptr(res.actions), _lib.ptr(res.reward), _lib.ptr(res.done),
                                                  _lib.ptr(res.info_steps), _lib.ptr(res.expected_gain), _lib.ptr(res.best_gain),
                                                  _lib.ptr(res.invalid), self._stream())
        _lib.check(rc, "mg_bandits_learner_rollout")
        return res

    def learner_scores(self, learner, state, learner_ids=None, seed=0, return_attempts=False):
        """The K scores the next `rollout_learner` step would compute for every env from `state`, float32 [N, K], from one
        launch that steps nothing and changes nothing: posterior draws (Thompson), indices, means. UCB with an unpulled arm:
        +inf for the unpulled arms and 0 for the others. `return_attempts=True` returns (scores, attempts int32 [N, K, 2]):
        the attempts the sampler made for X and Y, max_attempts + 1 where its fallback was taken (zeros unless Thompson)."""
        import torch
        N, K, dev = self.num_envs, self.K, self.device
        state, ids_d, keep, desc = self._learner_call(learner, state, learner_ids, seed, 1)
        scores = torch.empty(N, K, dtype=torch.float32, device=dev)
        attempts = torch.zeros(N, K, 2, dtype=torch.int32, device=dev) if return_attempts else None
        carry_c = _lib.BanditsLearnerCarry(state.pulls.contiguous().data_ptr(), state.wins.contiguous().data_ptr())
        rc = self._lib.mg_bandits_learner_scores(N, desc, _lib.ptr(ids_d), carry_c, int(seed), state.step, _lib.ptr(scores),
                                                 _lib.ptr(attempts), self._stream())
        _lib.check(rc, "mg_bandits_learner_scores")
        return (scores, attempts) if return_attempts else scores

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
