"""LiftSim (reference metagym/liftsim/environment/env.py) for N buildings at once, stepped by `mg_liftsim_step` on the GPU;
the reference's rule-based dispatcher (`rule_policy`) and whole rollouts in one launch (`rollout`, and `rollout_policy` with
learned dispatchers in the loop) run there too."""
import collections
import configparser
import ctypes as C
import math
import random

import numpy as np

from .. import _lib, _policy

CUSTOM, UNIFORM = 0, 1
QN = 16           # MG_LIFTSIM_QN
REC = 1248        # u32 words of one stream record: two 624-word key blocks
MAX_FLOORS, MAX_ELEVATORS = 128, 32
MAXIMUM_SPEED, MAXIMUM_LOAD = 2.0, 1600

# the reference's namedtuples (utils.py), so reference-style dispatchers work and states compare with ==
ElevatorState = collections.namedtuple("ElevatorState", [
    "Floor", "MaximumFloor", "Velocity", "MaximumSpeed", "Direction", "DoorState", "CurrentDispatchTarget",
    "DispatchTargetDirection", "LoadWeight", "MaximumLoad", "ReservedTargetFloors", "OverloadedAlarm",
    "DoorIsOpening", "DoorIsClosing"])
MansionState = collections.namedtuple("MansionState", ["ElevatorStates", "RequiringUpwardFloors",
                                                       "RequiringDownwardFloors"])
MansionAttribute = collections.namedtuple("MansionAttribute", ["ElevatorNumber", "NumberOfFloor", "FloorHeight"])

# the reference's config.ini (metagym/liftsim/config.ini); UNIFORM's two settings as its commented-out lines give them
DEFAULTS = dict(floors=10, elevators=4, floor_height=4.0, dt=0.5, generator="CUSTOM", particle_number=12,
                generation_interval=150.0)


def read_config(path):
    """A reference config.ini as keyword arguments of LiftSim (env.py:29-60; the log settings are ignored)."""
    c = configparser.ConfigParser()
    if not c.read(path):
        raise FileNotFoundError(path)
    g = c["PersonGenerator"]
    kw = dict(dt=float(c["Configuration"]["RunningTimeStep"]), floors=int(c["MansionInfo"]["NumberOfFloors"]),
              floor_height=float(c["MansionInfo"]["FloorHeight"]), elevators=int(c["MansionInfo"]["ElevatorNumber"]),
              generator=g["PersonGeneratorType"])
    if "ParticleNumber" in g:
        kw["particle_number"] = int(g["ParticleNumber"])
    if "GenerationInterval" in g:
        kw["generation_interval"] = float(g["GenerationInterval"])
    return kw


def resolve_config(config_file=None, **settings):
    """The settings a LiftSim runs with: config.ini's defaults, then `config_file` (parsed like env.py:29-60), then every
    setting passed explicitly (not None), which wins over the file. An unknown setting is a TypeError."""
    unknown = set(settings) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown LiftSim settings: %s" % sorted(unknown))
    cfg = dict(DEFAULTS)
    if config_file is not None:
        cfg.update(read_config(config_file))
    cfg.update({k: v for k, v in settings.items() if v is not None})
    return cfg


def custom_tables(flow, floors, dt):
    """The CUSTOM generator's tables (custom_generator.py:38-69, 111-135) from a flow array [T, 2 + F (F + 1)], with the
    reference's float32 / NEP 50 expressions for lambda and the category probabilities, and glibc (Python's math) for the
    exp / log values that decide draw counts. Returns a dict of numpy arrays named as in mg_liftsim_config."""
    flow = np.asarray(flow, dtype=np.float64)
    F = int(floors)
    if flow.ndim != 2 or flow.shape[0] < 1:
        raise ValueError("the flow table must be a 2-D array")
    if int(flow[0][0]) != F:
        raise AssertionError("The dimension of the data file does not match the floor number, %d and %d"
                             % (int(flow[0][0]), F))
    pf = flow[:, 1:]
    if pf.shape[1] != 1 + F * (F + 1):
        raise AssertionError("The column of the dataset file do not match the mansion, %d and %d"
                             % (pf.shape[1], 1 + F * (F + 1)))
    if not pf[-1][0] < 86400:
        raise AssertionError("The time of the day must < 86400 sec")
    if not pf[0][0] <= 0.0:
        raise AssertionError("The start time of the day must <= 0.0 sec")
    T = pf.shape[0]
    dens = np.zeros([T, F], dtype="float32")
    out = np.zeros([T, F, F], dtype="float32")
    for i in range(T):
        gap = pf[i + 1][0] - pf[i][0] if i < T - 1 else 86400 - pf[i][0]
        if not gap > 0.0:
            raise AssertionError("The time interval must be above zero")
        for j in range(F):
            dens[i][j] = 1.0 / gap * pf[i][j * (F + 1) + 1]
            out[i][j] = pf[i][(j * (F + 1) + 2):((j + 1) * (F + 1) + 1)]
    lam = dens * np.float32(dt)                       # float32, as numpy computes it for the nominal interval
    enlam = np.array([[math.exp(-float(x)) for x in row] for row in lam], dtype=np.float64)
    prob = np.zeros([T, F, F], dtype="float32")
    pp = np.zeros([T, F, F])
    flip = np.zeros([T, F, F], dtype=np.int32)
    logq = np.zeros([T, F, F])
    qn = np.zeros([T, F, F, QN])
    for i in range(T):
        for j in range(F):
            prob[i, j] = out[i][j] / (1.0e-5 + out[i][j].sum())
            pix = prob[i, j].astype(np.float64)
            rem = 1.0
            for c in range(F - 1):                    # random_multinomial: p_c / remaining_p, then random_binomial's flip
                if rem == 0.0:                        # a category with p == 1 took every person: numpy has left its loop
                    break
                p = float(pix[c]) / rem
                rem -= float(pix[c])
                if p > 0.5:
                    p, flip[i, j, c] = 1.0 - p, 1
                pp[i, j, c] = p
                lq = math.log(1.0 - p)
                logq[i, j, c] = lq
                qn[i, j, c] = [math.exp(float(n) * lq) for n in range(1, QN + 1)]
    return dict(times=pf[:, 0].copy(), dens=dens, out_prob=out, prob=prob, enlam=enlam, pp=pp, flip=flip, logq=logq,
                qn=qn)


def _random_state(key, p):
    """(key block, pos) of a two-block record at read position p, as numpy / CPython state: the block of word p - 1."""
    q = (p + REC - 1) % REC
    blk = q // 624
    return key[blk * 624:(blk + 1) * 624], q % 624 + 1


class LiftSim(object):
    """`num_envs` LiftSim buildings: env e is the reference's LiftSim after env.seed(seed + e) (or seeds[e]), bit for bit
    (state, reward, info, statistics and both streams), given the same actions and reset() calls.

    Configuration: the reference's config.ini defaults, then `config_file=` (parsed like env.py), then keyword settings,
    which win over the file (resolve_config). `seed()` on a live object also resets every env and clears the statistics,
    the CUSTOM time index and the flags: it starts env e over as a fresh `LiftSim(); env.seed(s_e)`, where the
    reference's env.seed() only reseeds its two streams. A CUSTOM
    env takes the flow table as `flow_file=` (the reference's mansion_flow.npy) or `flow=` (the array); it does not ship
    here. Actions: int32 [N, 2E] in the reference's flat order. An env with an out-of-range entry sets `invalid` and does
    not advance (the reference asserts mid-step; step(check=True) raises its AssertionError instead). An env whose queue
    would pass `queue_capacity` sets `overflow`, one whose draws need a path not built here sets `unsupported`; both freeze
    the env until the next seed(). step() never synchronises with the host unless check=True; outputs live in persistent
    buffers (copy_outputs=True returns copies). There is no CPU path.
    """

    def __init__(self, num_envs=1, config_file=None, flow_file=None, flow=None, device="cuda", seed=0, seeds=None,
                 floors=None, elevators=None, floor_height=None, dt=None, generator=None, particle_number=None,
                 generation_interval=None, queue_capacity=128, copy_outputs=False, **kwargs):
        import torch
        cfg = resolve_config(config_file, floors=floors, elevators=elevators, floor_height=floor_height, dt=dt,
                             generator=generator, particle_number=particle_number,
                             generation_interval=generation_interval, **kwargs)
        if not float(cfg["dt"]) <= 1:
            raise AssertionError("RunningTimeStep in config.ini must be less than 1 in order to ensure accuracy")
        if cfg["generator"] not in ("CUSTOM", "UNIFORM"):
            raise RuntimeError("No such generator type: %s" % cfg["generator"])
        self.F, self.E = int(cfg["floors"]), int(cfg["elevators"])
        self.floor_height, self.dt = float(cfg["floor_height"]), float(cfg["dt"])
        self.generator = cfg["generator"]
        if not (2 <= self.F <= MAX_FLOORS and 1 <= self.E <= MAX_ELEVATORS):
            raise ValueError("LiftSim here needs 2 <= floors <= %d and 1 <= elevators <= %d" % (MAX_FLOORS, MAX_ELEVATORS))
        if self.generator == "CUSTOM" and flow is None and flow_file is None:
            raise ValueError("a CUSTOM LiftSim needs the flow table: pass flow_file= (the reference's "
                             "mansion_flow.npy, its CustomDataFile) or flow=")
        if torch.device(device).type != "cuda":
            raise _lib.MetaGymHipError("metagym_amd runs on an AMD GPU only (got device %r); there is no CPU fallback"
                                       % (device,))
        self.device = _lib.canonical_device(device)
        self.num_envs = N = int(num_envs)
        if N <= 0:
            raise ValueError("num_envs must be positive")
        self.copy_outputs = bool(copy_outputs)
        self.window = int(600 / self.dt)
        c = _lib.LiftsimConfig()
        c.floors, c.elevators, c.queue_capacity, c.window = self.F, self.E, int(queue_capacity), self.window
        c.floor_height, c.dt, c.nv_magic = self.floor_height, self.dt, random.NV_MAGICCONST
        self._tables = {}
        if self.generator == "CUSTOM":
            if flow is None:
                flow = np.load(flow_file)
            tb = custom_tables(flow, self.F, self.dt)
            c.generator, c.table_len = CUSTOM, len(tb["times"])
            for name in ("times", "dens", "enlam", "pp", "flip", "logq", "qn"):
                t = torch.from_numpy(np.ascontiguousarray(tb[name])).to(self.device)
                self._tables[name] = t
                setattr(c, name, t.data_ptr())
            self.tables = tb
        else:
            c.generator = UNIFORM
            c.particle_number = int(cfg["particle_number"])
            c.generation_interval = float(cfg["generation_interval"])
        self._cfg = c
        self._lib = _lib.load()
        offs = (C.c_int64 * len(_lib.LIFTSIM_FIELDS))()
        total = C.c_int64()
        _lib.check(self._lib.mg_liftsim_layout(c, N, offs, total), "mg_liftsim_layout")
        self.arena = torch.zeros(int(total.value), dtype=torch.uint8, device=self.device)
        self._off = dict(zip(_lib.LIFTSIM_FIELDS, [int(o) for o in offs]))
        E, F, Q, W = self.E, self.F, int(queue_capacity), self.window
        f64, i32, u8 = torch.float64, torch.int32, torch.uint8
        v = self._view
        # observations: [N, ...] views of the [item][N] state
        self.floor = v("floor", f64, (E, N)).t()
        self.velocity = v("vel", f64, (E, N)).t()
        self.direction = v("dir", i32, (E, N)).t()
        self.door_state = v("door", f64, (E, N)).t()
        self.dispatch_target = v("dispatch", i32, (E, N)).t()
        self.dispatch_target_direction = v("dispatch_dir", i32, (E, N)).t()
        self.load_weight = v("load", f64, (E, N)).t()
        self.reserved_target_floors = v("targets", i32, (E, F, N)).permute(2, 0, 1)
        self.reserved_count = v("ntarget", i32, (E, N)).t()
        self.overloaded_alarm = v("alarm", f64, (E, N)).t()
        b = torch.bool   # the kernel writes these bytes as 0 / 1: bool views, no copies
        self.door_is_opening = v("opening", b, (E, N)).t()
        self.door_is_closing = v("closing", b, (E, N)).t()
        self.requiring_upward = v("up", b, (F, N)).t()
        self.requiring_downward = v("down", b, (F, N)).t()
        self.reward = v("reward", f64, (N,))
        self.time_consume = v("timec", f64, (N,))
        self.energy_consume = v("energy", f64, (N,))
        self.given_up_persons = v("given", i32, (N,))
        self.invalid = v("invalid", u8, (N,))
        self.overflow = v("overflow", u8, (N,))
        self.unsupported = v("unsupported", u8, (N,))
        self.done = torch.zeros(N, dtype=torch.bool, device=self.device)   # always False, as in the reference
        self.queue_capacity, self._Q, self._W = Q, Q, W
        self._rule_actions = torch.zeros(N, 2 * E, dtype=i32, device=self.device)   # rule_policy()'s output
        self.seed(seed, seeds)

    # ------------------------------------------------------------------ plumbing
    def _view(self, name, dtype, shape):
        import torch
        n = 1
        for s in shape:
            n *= s
        size = n * torch.empty((), dtype=dtype).element_size()
        o = self._off[name]
        return self.arena[o:o + size].view(dtype).view(shape)

    def _stream(self):
        return _lib.current_stream(self.device)

    @property
    def attribute(self):
        """The reference's MansionAttribute namedtuple."""
        return MansionAttribute(self.E, self.F, self.floor_height)

    # ------------------------------------------------------------------ API
    def seed(self, seed=0, seeds=None):
        """env.seed(seed + e) or seeds[e] for every env (32-bit values): both streams, the statistics, the time index and
        the flags start over, and every env is reset, so env e is a fresh LiftSim after env.seed(s_e). (The reference's
        env.seed() on a running env reseeds its streams only.)"""
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
            raise ValueError("seeds are 32-bit: need 0 <= seed and seed + N <= 2^32")
        _lib.check(self._lib.mg_liftsim_seed(self._cfg, N, _lib.ptr(self.arena), int(seed), _lib.ptr(seeds_t),
                                             self._stream()), "mg_liftsim_seed")
        return [seed] if seeds is None else list(seeds)

    def reset(self, mask=None):
        """env.reset() for every env (or those with mask[e] != 0). Statistics, streams and the time index carry over."""
        import torch
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device)
            if tuple(m.shape) != (self.num_envs,):
                raise ValueError("mask must have shape [%d]" % self.num_envs)
            m = (m != 0).to(torch.uint8).contiguous()
        _lib.check(self._lib.mg_liftsim_reset(self._cfg, self.num_envs, _lib.ptr(self.arena), _lib.ptr(m),
                                              self._stream()), "mg_liftsim_reset")
        return self.observation()

    def observation(self):
        obs = dict(Floor=self.floor, Velocity=self.velocity, Direction=self.direction, DoorState=self.door_state,
                   CurrentDispatchTarget=self.dispatch_target, DispatchTargetDirection=self.dispatch_target_direction,
                   LoadWeight=self.load_weight, ReservedTargetFloors=self.reserved_target_floors,
                   ReservedTargetCount=self.reserved_count, OverloadedAlarm=self.overloaded_alarm,
                   DoorIsOpening=self.door_is_opening, DoorIsClosing=self.door_is_closing,
                   RequiringUpwardFloors=self.requiring_upward, RequiringDownwardFloors=self.requiring_downward)
        if self.copy_outputs:
            obs = {k: t.clone() for k, t in obs.items()}
        return obs

    def step(self, action, check=False):
        """One env.step(action) per env: action int32 [N, 2E]. Returns (observation, reward, done, info)."""
        import torch
        a = torch.as_tensor(action, device=self.device)
        if tuple(a.shape) != (self.num_envs, 2 * self.E):
            raise ValueError("actions must have shape [%d, %d]" % (self.num_envs, 2 * self.E))
        if a.dtype != torch.int32:
            a = a.to(torch.int32)
        a = a.contiguous()
        if check:
            t, d = a[:, 0::2], a[:, 1::2]
            if bool(((t < -1) | (t > self.F)).any()):
                raise AssertionError("action.TargetFloor >= -1 and action.TargetFloor <= number_of_floors")
            if bool(((d < -1) | (d > 1)).any()):
                raise AssertionError("action.DirectionIndicator in [-1, 0, 1]")
        _lib.check(self._lib.mg_liftsim_step(self._cfg, self.num_envs, _lib.ptr(self.arena), _lib.ptr(a),
                                             self._stream()), "mg_liftsim_step")
        info = dict(time_consume=self.time_consume, energy_consume=self.energy_consume,
                    given_up_persons=self.given_up_persons, invalid=self.invalid, overflow=self.overflow,
                    unsupported=self.unsupported)
        reward, done = self.reward, self.done
        if self.copy_outputs:
            info = {k: t.clone() for k, t in info.items()}
            reward, done = reward.clone(), done.clone()
        return self.observation(), reward, done, info

    def rule_policy(self):
        """The reference's rule-based dispatcher (tests/rule_benchmark/dispatcher.py Rule_dispatcher.policy) on every
        env's current state: int32 [N, 2E], so `env.step(env.rule_policy())` is one step of its run_dispacher. One launch,
        no host synchronisation; the result is a persistent buffer (a copy with copy_outputs=True)."""
        _lib.check(self._lib.mg_liftsim_rule_policy(self._cfg, self.num_envs, _lib.ptr(self.arena),
                                                    _lib.ptr(self._rule_actions), self._stream()),
                   "mg_liftsim_rule_policy")
        return self._rule_actions.clone() if self.copy_outputs else self._rule_actions

    RECORDS = ("reward", "time_consume", "energy_consume", "given_up_persons", "actions")

    def rollout(self, actions=None, steps=None, policy=None, record=("reward",)):
        """T steps of every env in one launch: over `actions` (int32 [T, N, 2E]), or with policy="rule" and steps=T over
        the rule dispatcher's own actions (run_dispacher's loop); exactly one of the two. Returns a dict: "return" [N],
        the T rewards added in step order from 0.0, and the [T, N] records named in `record` (of RECORDS; "actions",
        [T, N, 2E], with policy="rule" only). The arena, and so every observation view, ends as after T step() calls.
        No host synchronisation; the returned tensors are new ones."""
        import torch
        N, E = self.num_envs, self.E
        if (actions is None) == (policy is None):
            raise ValueError("rollout takes either actions or policy=\"rule\" with steps")
        if policy is not None:
            if policy != "rule":
                raise ValueError("unknown policy %r (the one built here is \"rule\")" % (policy,))
            if steps is None or int(steps) < 1:
                raise ValueError("rollout(policy=\"rule\") needs steps >= 1")
            T, a, mode = int(steps), None, _lib.LIFTSIM_POLICY_RULE
        else:
            a = torch.as_tensor(actions, device=self.device)
            if a.dim() != 3 or tuple(a.shape[1:]) != (N, 2 * E) or a.shape[0] < 1:
                raise ValueError("actions must have shape [T, %d, %d] with T >= 1" % (N, 2 * E))
            if steps is not None and int(steps) != a.shape[0]:
                raise ValueError("steps = %d but actions holds %d steps" % (int(steps), a.shape[0]))
            if a.dtype != torch.int32:
                a = a.to(torch.int32)
            a = a.contiguous()
            T, mode = int(a.shape[0]), _lib.LIFTSIM_POLICY_ACTIONS
        record = (record,) if isinstance(record, str) else tuple(record or ())
        unknown = set(record) - set(self.RECORDS)
        if unknown:
            raise ValueError("unknown records: %s (known: %s)" % (sorted(unknown), list(self.RECORDS)))
        if "actions" in record and mode != _lib.LIFTSIM_POLICY_RULE:
            raise ValueError("the actions record is for policy=\"rule\"; given actions are the caller's already")
        out = {"return": torch.empty(N, dtype=torch.float64, device=self.device)}
        for name in record:
            if name == "actions":
                out[name] = torch.empty(T, N, 2 * E, dtype=torch.int32, device=self.device)
            else:
                out[name] = torch.empty(T, N, dtype=torch.int32 if name == "given_up_persons" else torch.float64,
                                        device=self.device)
        _lib.check(self._lib.mg_liftsim_rollout(
            self._cfg, N, _lib.ptr(self.arena), mode, _lib.ptr(a), T, _lib.ptr(out["return"]),
            _lib.ptr(out.get("reward")), _lib.ptr(out.get("time_consume")), _lib.ptr(out.get("energy_consume")),
            _lib.ptr(out.get("given_up_persons")), _lib.ptr(out.get("actions")), self._stream()), "mg_liftsim_rollout")
        return out

    def rollout_policy(self, policy, steps, policy_ids=None, record=(), state=None):
        """`steps` closed-loop env steps of every building in ONE launch: building e is dispatched by policy
        `policy_ids[e]` of `policy` (a `LiftPolicy`; `policy_ids=None` = policy 0 for all), evaluated inside the kernel
        once per elevator on the state before each step (liftsim/policy.py defines the arithmetic exactly). The step is
        `step()`'s: replaying the recorded actions through `rollout(actions)` or `step()` from the same arena gives the
        same records and the same end arena, bit for bit. Returns the dict of `rollout()`: "return" [N] and the records
        named in `record` (of RECORDS; "actions" [T, N, 2E] holds the policy's actions, (0, 0) for an env that was
        frozen when the step began). The ids are validated once: nothing synchronises when `policy_ids` is None, a host
        array, or the (unchanged) tensor of the previous call, so after `policy.to(device)` the call can be captured in a hipGraph. A refused call
        (a policy for another F or E, an id out of range, steps < 1) raises and leaves the arena untouched.

        With a `LiftRecurrentPolicy` every elevator has a memory, kept in `state` (a `LiftPolicyState` on this device,
        updated in place; None: a fresh `LiftPolicyState.zeros(N, E, H, device)`), and the dict also holds "state", that
        same object: the end carry. T1 steps and then T2 steps through one state equal T1 + T2 steps in one call. The
        carry sees `rollout_policy` steps only: a `step()` or `rollout(actions)` between two calls moves the arena, and
        prev_reward stays the last `rollout_policy` reward. An env that is frozen when a step begins keeps its carry; in
        the step in which it overflows the policy has run and prev_reward becomes the recorded 0. A refused call (also: a
        state of another class, on another device, or of wrong shapes, dtypes or layout) leaves arena and state
        untouched. With a `LiftPolicy`, passing `state` is a ValueError."""
        import torch
        from .policy import LiftPolicy, LiftPolicyState, LiftRecurrentPolicy
        if not isinstance(policy, LiftPolicy):
            raise TypeError("policy must be a LiftPolicy or a LiftRecurrentPolicy, got %s" % type(policy).__name__)
        recurrent = isinstance(policy, LiftRecurrentPolicy)
        if state is not None and not recurrent:
            raise ValueError("a LiftPolicy has no memory: state is for a LiftRecurrentPolicy")
        T, N, E = int(steps), self.num_envs, self.E
        if T < 1:
            raise ValueError("steps must be at least 1, got %d" % T)
        if policy.floors != self.F or policy.elevators != E:
            raise ValueError("the policy was built for %d floors and %d elevators, the env has %d and %d"
                             % (policy.floors, policy.elevators, self.F, E))
        record = (record,) if isinstance(record, str) else tuple(record or ())
        unknown = set(record) - set(self.RECORDS)
        if unknown:
            raise ValueError("unknown records: %s (known: %s)" % (sorted(unknown), list(self.RECORDS)))
        if recurrent:
            H = policy.hidden
            if state is None:
                state = LiftPolicyState.zeros(N, E, H, self.device)
            elif not isinstance(state, LiftPolicyState):
                raise TypeError("state must be a LiftPolicyState, got %s" % type(state).__name__)
            # (field, shape, dtype, the permutation that gives the storage order: env index fastest)
            want = (("h", (N, E, H), torch.float32, (1, 2, 0)), ("prev_choice", (N, E), torch.int32, (1, 0)),
                    ("prev_reward", (N,), torch.float32, (0,)))
            for name, shape, dtype, order in want:
                v = getattr(state, name)
                if not isinstance(v, torch.Tensor):
                    raise ValueError("state must hold torch tensors on %s (LiftPolicyState.zeros(N, E, H, device))" % (self.device,))
                if v.device != self.device:
                    raise ValueError("state lives on %s, the env on %s" % (v.device, self.device))
                if tuple(v.shape) != shape or v.dtype != dtype or not v.permute(*order).is_contiguous():
                    raise ValueError("state.%s must be a %s tensor of shape %s stored env index fastest (this env has %d envs "
                                     "and %d elevators, the policy %d hidden units), got %s %s"
                                     % (name, dtype, shape, N, E, H, v.dtype, tuple(v.shape)))
        ids = _policy.policy_ids(self, policy_ids, policy.num_policies, default="zero")
        params = policy.to(self.device)
        desc_cls = _lib.LiftsimRPolicyDesc if recurrent else _lib.LiftsimPolicyDesc
        desc = desc_cls(params.data_ptr(), policy.num_policies, policy.hidden, policy.floors, policy.elevators,
                        (C.c_float * 8)(*[float(v) for v in policy.scale]))
        out = {"return": torch.empty(N, dtype=torch.float64, device=self.device)}
        for name in record:
            if name == "actions":
                out[name] = torch.empty(T, N, 2 * E, dtype=torch.int32, device=self.device)
            else:
                out[name] = torch.empty(T, N, dtype=torch.int32 if name == "given_up_persons" else torch.float64,
                                        device=self.device)
        if recurrent:
            carry = _lib.LiftsimPolicyState(state.h.data_ptr(), state.prev_choice.data_ptr(), state.prev_reward.data_ptr())
            _lib.check(self._lib.mg_liftsim_rpolicy_rollout(
                self._cfg, N, _lib.ptr(self.arena), T, desc, _lib.ptr(ids), carry, _lib.ptr(out["return"]),
                _lib.ptr(out.get("reward")), _lib.ptr(out.get("time_consume")), _lib.ptr(out.get("energy_consume")),
                _lib.ptr(out.get("given_up_persons")), _lib.ptr(out.get("actions")), self._stream()),
                "mg_liftsim_rpolicy_rollout")
            out["state"] = state
            return out
        _lib.check(self._lib.mg_liftsim_policy_rollout(
            self._cfg, N, _lib.ptr(self.arena), T, desc, _lib.ptr(ids), _lib.ptr(out["return"]),
            _lib.ptr(out.get("reward")), _lib.ptr(out.get("time_consume")), _lib.ptr(out.get("energy_consume")),
            _lib.ptr(out.get("given_up_persons")), _lib.ptr(out.get("actions")), self._stream()),
            "mg_liftsim_policy_rollout")
        return out

    def statistics_tensors(self):
        """env.statistics of every env as [N] tensors (one launch, no host synchronisation)."""
        _lib.check(self._lib.mg_liftsim_statistics(self._cfg, self.num_envs, _lib.ptr(self.arena), self._stream()),
                   "mg_liftsim_statistics")
        import torch
        N, i64, f64 = self.num_envs, torch.int64, torch.float64
        return {"DeliveredPersons(10Minutes)": self._view("st_d", i64, (N,)),
                "GeneratedPersons(10Minutes)": self._view("st_g", i64, (N,)),
                "AbandonedPersons(10Minutes)": self._view("st_a", i64, (N,)),
                "EnergyConsumption(10Minutes)": self._view("st_e", f64, (N,)),
                "TotalWaitingTime(10Minutes)": self._view("st_w", f64, (N,))}

    @property
    def statistics(self):
        """[N] tensors of the reference's statistics dict (copies)."""
        return {k: t.clone() for k, t in self.statistics_tensors().items()}

    def statistics_of(self, e):
        """Env e's statistics as the reference's dict of Python numbers."""
        st = self.statistics_tensors()
        return {k: (int(t[e].item()) if "Persons" in k else float(t[e].item())) for k, t in st.items()}

    def mansion_state(self, e):
        """Env e's state as the reference's MansionState namedtuple (host copy)."""
        F = self.F
        fl = self.floor[e].tolist()
        vel = self.velocity[e].tolist()
        dr = self.direction[e].tolist()
        door = self.door_state[e].tolist()
        dt_ = self.dispatch_target[e].tolist()
        dd = self.dispatch_target_direction[e].tolist()
        lw = self.load_weight[e].tolist()
        rt = self.reserved_target_floors[e].tolist()
        rc = self.reserved_count[e].tolist()
        al = self.overloaded_alarm[e].tolist()
        op = self.door_is_opening[e].tolist()
        cl = self.door_is_closing[e].tolist()
        els = [ElevatorState(fl[k], F, vel[k], MAXIMUM_SPEED, dr[k], door[k], dt_[k], dd[k], lw[k], MAXIMUM_LOAD,
                             rt[k][:rc[k]], al[k], bool(op[k]), bool(cl[k])) for k in range(self.E)]
        up = self.requiring_upward[e].tolist()
        down = self.requiring_downward[e].tolist()
        return MansionState(els, [i + 1 for i in range(F) if up[i]], [i + 1 for i in range(F) if down[i]])

    def random_state(self, e):
        """Env e's CPython `random` stream as random.getstate() spells it."""
        import torch
        key = self._view("pykey", torch.int32, (self.num_envs, REC))[e].cpu().numpy().view(np.uint32)
        p = int(self._view("pyp", torch.int32, (self.num_envs,))[e].item())
        blk, pos = _random_state(key, p)
        return (3, tuple(int(x) for x in blk) + (pos,), None)

    def numpy_state(self, e):
        """Env e's numpy stream as numpy.random.get_state() spells it."""
        import torch
        key = self._view("npkey", torch.int32, (self.num_envs, REC))[e].cpu().numpy().view(np.uint32)
        p = int(self._view("npp", torch.int32, (self.num_envs,))[e].item())
        blk, pos = _random_state(key, p)
        return ("MT19937", blk.copy(), pos, 0, 0.0)

