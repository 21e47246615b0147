"""LiftSim edge fixtures shared by tests/test_liftsim_edges.py (CPU), tests/test_liftsim_edges_gpu.py and
scripts/gen_golden_liftsim_edges.py: synthetic flow tables, the case tables, and an oracle env (`Tracked`) that reports
what the kernels' edges depend on: the words each step draws from both streams, the poisson counts, and where the
device's queue rings stand. Every expected value comes from tests/liftsim_oracle.py and tests/liftsim_rule_oracle.py;
runs are cached, so the tests of one session share them."""
import collections
import functools
import random

import numpy as np

import liftsim_oracle as O
import liftsim_rule_oracle as R

MT = 624
REC = 2 * MT      # a lane's stream record: the key block being read and its refill (mg_mt19937.h LaneStream)


# ---------------------------------------------------------------------------------------------- flow tables
def synth_flow(F, rows):
    """A flow array [T, 2 + F (F + 1)] from rows (start_time, rate_per_second[F], weights[F, F]), in the column layout
    custom_tables reads: F, the start time, then per floor the count over the row's interval and its F out-weights."""
    T = len(rows)
    flow = np.zeros((T, 2 + F * (F + 1)))
    for i, (start, rate, weights) in enumerate(rows):
        gap = (rows[i + 1][0] if i < T - 1 else 86400.0) - start
        rate, weights = np.asarray(rate, np.float64), np.asarray(weights, np.float64)
        assert rate.shape == (F,) and weights.shape == (F, F) and gap > 0
        flow[i, 0], flow[i, 1] = F, start
        for j in range(F):
            flow[i, 2 + j * (F + 1)] = rate[j] * gap
            flow[i, 3 + j * (F + 1):3 + j * (F + 1) + F] = weights[j]
    return flow


ONLY = 1.0e7      # a weight so large that float32(w / (1e-5 + w)) == 1: the binomial's p == 1, so pp == 0 with flip set
HEAVY, LIMIT = 9.6, 10.5    # poisson rates per step: just inside the multiplication method, and past it (PTRS, not built)
CUSTOM = {        # F -> (E, dt); float32(0.3) is inexact, so dt = 0.3 runs on the enlam table of an inexact lambda
    2: (1, 0.5), 8: (3, 0.5), 9: (3, 0.3), 16: (8, 0.5)}
CUSTOM_N, CUSTOM_SEED, CUSTOM_Q = 70, 300, 1024
CUSTOM_SAMPLE = (0, 1, 17, 38, 62, 63, 64, 69)
ROW1_AT, ROW2_AT = 20.0, 40.0


def _skewed(rs, F):
    w = rs.rand(F) ** 4
    w[rs.randint(F)] *= 20.0          # one category well above one half: a flipped binomial
    return w


def edge_rows(F, dt):
    """The three rows of the synthetic CUSTOM table as (start, rate per second, weights): heavy, the same at a hundredth, and the heavy
    one with one floor past the limit (floor 1; floor 6 at F = 8 and 16, where the kernel has drawn for five floors by then)."""
    rs = np.random.RandomState(100 + F)
    lam = np.full(F, 0.4)
    w = np.stack([_skewed(rs, F) for _ in range(F)])
    if F == 2:
        # two floors cannot hold every pattern at once: the quiet row gets other weights (below)
        lam[:] = HEAVY
        w[0] = [2.0, 1.0]             # two thirds of floor 1's persons have src == dst (a flipped binomial with pp > 0)
        w[1] = [ONLY, 0.0]            # the top floor sends everybody to floor 1
    else:
        lam[0] = lam[5] = HEAVY       # skewed random weights
        lam[1] = 0.0                  # nobody arrives here
        lam[2] = lam[3] = lam[4] = 1.5
        w[2] = 0.0
        w[2, F - 1] = 2.0             # the whole weight on the top floor
        w[3] = 0.0                    # all-zero: numpy's multinomial sends every person to the last category
        w[4] = 0.0
        w[4, 4] = 1.0                 # only itself: src == dst, counted as generated and never enqueued
        lam[F - 1] = 3.0
        w[F - 1] = 0.0
        w[F - 1, 0] = ONLY            # the top floor sends everybody to floor 1
    quiet_w = w
    if F == 2:
        quiet_w = np.array([[0.0, 0.0], [0.0, 2.0]])   # an all-zero floor, and the top floor only to itself
    over = lam.copy()
    over[5 if F in (8, 16) else 0] = LIMIT
    return [(0.0, lam / dt, w), (ROW1_AT, lam * 0.01 / dt, quiet_w), (ROW2_AT, over / dt, w)]


def edge_flow(F):
    return synth_flow(F, edge_rows(F, CUSTOM[F][1]))


def one_row_flow_f2():
    """F = 2 on a one-row table (T = 1 in the time search): nobody arrives at the top floor."""
    return synth_flow(2, [(0.0, np.array([4.0, 0.0]) / 0.5, [[0.2, 0.8], [1.0, 1.0]])])


# ---------------------------------------------------------------------------------------------- the tracked oracle env
class CountingRandom(random.Random):
    """random.Random that counts the 32-bit words it draws. Both random() (2 words) and getrandbits(k) (ceil(k / 32)
    words) are overridden: with only one of them CPython would pick another _randbelow, and other draws."""
    words = 0

    def random(self):
        self.words += 2
        return super().random()

    def getrandbits(self, k):
        self.words += (k + 31) // 32
        return super().getrandbits(k)


class RecordingNumpy(object):
    """A proxy for an env's np.random.RandomState that keeps the poisson counts of the last step and the largest one."""

    def __init__(self, rs):
        self.rs, self.last, self.max_count = rs, None, 0

    def poisson(self, lam, size=None):
        n = self.rs.poisson(lam, size=size)
        self.last = n
        self.max_count = max(self.max_count, int(np.max(n)))
        return n

    def multinomial(self, n, p):
        return self.rs.multinomial(n, p)

    def get_state(self):
        return self.rs.get_state()


def _next_block(key):
    rs = np.random.RandomState(0)
    rs.set_state(("MT19937", key, MT))
    rs.bytes(4)                        # one word: the generator twists the block first
    return rs.get_state()[1]


def words_between(key0, pos0, key1, pos1):
    """The number of 32-bit words an MT19937 stream drew between two (key, pos) states, found by twisting key0 forward."""
    key = np.asarray(key0, np.uint32)
    key1 = np.asarray(key1, np.uint32)
    for twists in range(8):
        if np.array_equal(key, key1) and twists * MT + pos1 - pos0 >= 0:
            return twists * MT + pos1 - pos0
        key = _next_block(key)
    raise AssertionError("the second state is not within 7 key blocks of the first")


def past_horizon(words_in_step, pos):
    """Whether a step that draws `words_in_step` words from a stream at CPython / numpy position `pos` (1..624, the
    words of the current key block already used) reads past the next key block.

    From LaneStream in csrc/mg_mt19937.h: a lane's record holds the block being read and its refill, `ready` covers one
    block boundary per step, and the word that would cross a second boundary sets `bad`. So a step can draw the 624 - pos
    words left in the current block and the 624 of the next one, 1248 - pos in all. A freshly seeded stream has pos = 624
    (its first block is all used up, as numpy and CPython seed it), so its first step may draw 624 words."""
    return words_in_step > REC - pos


class _Ring(collections.deque):
    """One queue of the oracle (newest at index 0) that also models the device's ring of Q slots: `head` is the number of
    give-ups (pop) since the queue was last empty at a step's end, mod Q; boarding (del) compacts towards the head and
    leaves it alone; arrivals go to head + len."""

    def start(self, Q, log):
        self.Q, self.log, self.head, self.pops = Q, log, 0, 0

    def pop(self):
        self.pops += 1
        return super().pop()

    def __delitem__(self, i):
        n = len(self)
        self.log["boarded"] += 1
        self.log["mid_deque_delete"] += i != n - 1
        self.log["boarded_while_wrapped"] += self.head + n > self.Q
        super().__delitem__(i)

    def end_step(self):
        if self.head + self.pops >= self.Q and len(self) > 0:
            self.log["give_up_past_last_slot"] += 1
        self.head = (self.head + self.pops) % self.Q if len(self) > 0 else 0
        self.pops = 0
        if self.head + len(self) > self.Q:
            self.log["wrapped"] += 1


class Tracked(object):
    """An oracle env whose streams and queues are watched. After step(): `crossed` (this step read past the horizon of one
    of its streams; the device flags the env `unsupported` in it), `py_words` / `np_words`, and the counters in `log`."""

    def __init__(self, cfg, seed, Q=1 << 30):
        self.env = env = O.Env(cfg, seed)
        env.py = CountingRandom(seed)          # reset() drew nothing from the stream this one replaces
        env.np = RecordingNumpy(env.np)
        self.F, self.Q = cfg.F, Q
        self.log = collections.Counter()
        for side in (env.up, env.down):
            for f in range(cfg.F):
                side[f] = _Ring()
                side[f].start(Q, self.log)
        self.crossed = False
        self.first_cross = -1
        self.steps = 0
        self.max_words = 0
        self.delivered = 0

    def step(self, action):
        env = self.env
        py0 = env.py.getstate()[1]
        np0 = env.np.get_state()
        env.py.words = 0
        out = env.step(action)
        self.py_words = env.py.words
        np1 = env.np.get_state()
        self.np_words = words_between(np0[1], np0[2], np1[1], np1[2])
        self.py_pos, self.np_pos = py0[MT], np0[2]
        self.crossed = past_horizon(self.py_words, py0[MT]) or past_horizon(self.np_words, np0[2])
        if self.crossed and self.first_cross < 0:
            self.first_cross = self.steps
        self.max_words = max(self.max_words, self.py_words, self.np_words)
        self.steps += 1
        self.delivered += env.stats[0][0]
        self.log["alarm"] += any(e.alarm > 0 for e in env.elev)
        self.log["give_up"] += out[1]["given_up_persons"]
        for side in (env.up, env.down):
            for q in side:
                q.end_step()
        return out

    def queue(self, qd):
        """(qhead, qlen) of the device's queue qd = 2 * (floor - 1) + (0 up, 1 down)."""
        q = (self.env.up, self.env.down)[qd % 2][qd // 2]
        return q.head, len(q)

    def wrapped_queues(self):
        return [qd for qd in range(2 * self.F) if sum(self.queue(qd)) > self.Q]


def row(r, info):
    """One step's outputs as the GPU tests compare them: reward, time_consume, energy_consume, given_up_persons."""
    return [r, info["time_consume"], info["energy_consume"], float(info["given_up_persons"])]


def random_actions(seed, T, N, F, E):
    """int32 [T, N, 2E]: targets in [-1, F] and directions in {-1, 0, 1}, with target -1, target F and direction 0 forced
    into the first steps of env 0 so that they occur whatever the draw."""
    rs = np.random.RandomState(seed)
    a = np.empty((T, N, 2 * E), np.int32)
    a[:, :, 0::2] = rs.randint(-1, F + 1, size=(T, N, E))
    a[:, :, 1::2] = rs.randint(-1, 2, size=(T, N, E))
    a[0, 0, 0:2] = [-1, 0]
    a[1, 0, 0:2] = [F, 0]
    return a


def held_actions(seed, T, N, F, E, hold=16):
    """random_actions for a tall building: an elevator gets a new target every `hold` steps (floor 1, floor F or any
    value in [-1, F]) and target -1, "no new dispatch", in between, so that cars stop, open and take persons on. The
    last car is sent to floor F in step 0 and then left alone."""
    rs = np.random.RandomState(seed)
    a = random_actions(seed, T, N, F, E)
    fresh = rs.randint(0, hold, size=(1, N, E)) == np.arange(T)[:, None, None] % hold
    kind = rs.randint(0, 4, size=(T, N, E))
    tgt = np.where(kind == 0, 1, np.where(kind == 1, F, a[:, :, 0::2]))
    a[:, :, 0::2] = np.where(fresh, tgt, -1)
    a[:, :, 2 * E - 2] = -1           # the last car is sent to floor F once and left alone: it gets there if T allows
    a[0, :, 2 * E - 2] = F
    a[0, 0, 0:2] = [-1, 0]
    a[1, 0, 0:2] = [F, 0]
    return a


def streams(env):
    """Both streams of an oracle env as (py key, py pos, np key, np pos)."""
    py, st = env.py.getstate()[1], env.np.get_state()
    return np.asarray(py[:MT], np.uint32), int(py[MT]), np.asarray(st[1], np.uint32), int(st[2])


# ---------------------------------------------------------------------------------------------- the big buildings
BIG_KW = dict(dt=1.0, particle_number=40, generation_interval=4.0)
# (F, E) -> steps of the dispatcher run. A car needs (F - 1) * 4 m / 2 m/s seconds and its acceleration to reach floor F;
# the counts are the smallest round ones at which test_liftsim_edges.py's coverage asserts hold.
BIG = {(128, 32): 290, (65, 32): 200, (64, 17): 200, (33, 5): 150, (32, 2): 150}
BIG_RANDOM_STEPS = 120
BIG_N, BIG_SEED = 130, 7
BIG_SAMPLE = (0, 63, 64, 127, 128, 129)


def big_config(F, E):
    return O.Config(floors=F, elevators=E, generator="UNIFORM", **BIG_KW)


def _watch_state(ev, state, F):
    ev["at_top"] += any(e.Floor == F for e in state.ElevatorStates)
    ev["top_reserved"] += any(F in e.ReservedTargetFloors for e in state.ElevatorStates)
    ev["call_at_top"] += F in state.RequiringDownwardFloors
    ev["call_at_1"] += 1 in state.RequiringUpwardFloors


@functools.lru_cache(maxsize=None)
def big_rule_run(F, E):
    """The sampled envs of a big building under the rule dispatcher, in the oracle: per step the actions and outputs, states at the
    checkpoints, and the events."""
    T, cfg = BIG[(F, E)], big_config(F, E)
    S = len(BIG_SAMPLE)
    out = dict(T=T, checks=sorted({T // 2, T}), actions=np.zeros((T, S, 2 * E), np.int32), rows=np.zeros((T, S, 4)),
               states={}, stats={}, ev=collections.Counter(), crossed=0, envs=[])
    for j, e in enumerate(BIG_SAMPLE):
        tr = Tracked(cfg, BIG_SEED + e)
        for k in range(T):
            state = tr.env.mansion_state()
            a = R.policy(state, out["stats"])
            out["actions"][k, j] = a
            out["rows"][k, j] = row(*tr.step(a))
            out["crossed"] += tr.crossed
            _watch_state(out["ev"], tr.env.mansion_state(), F)
            if k + 1 in out["checks"]:
                out["states"][(k + 1, e)] = tr.env.mansion_state()
        out["envs"].append(tr)
    out["max_queue"] = max(tr.env.max_queue for tr in out["envs"])
    return out


@functools.lru_cache(maxsize=None)
def big_random_run(F, E):
    """The sampled envs of a big building under held_actions, in the oracle."""
    T, cfg = BIG_RANDOM_STEPS, big_config(F, E)
    acts = held_actions(1000 + F, T, BIG_N, F, E)
    out = dict(T=T, actions=acts, rows=np.zeros((T, len(BIG_SAMPLE), 4)), ev=collections.Counter(), crossed=0, envs=[])
    for j, e in enumerate(BIG_SAMPLE):
        tr = Tracked(cfg, BIG_SEED + e)
        for k in range(T):
            out["rows"][k, j] = row(*tr.step([int(x) for x in acts[k, e]]))
            out["crossed"] += tr.crossed
            _watch_state(out["ev"], tr.env.mansion_state(), F)
        out["envs"].append(tr)
    return out


# ---------------------------------------------------------------------------------------------- CUSTOM on synthetic tables
def custom_config(F, flow):
    E, dt = CUSTOM[F]
    return O.Config(floors=F, elevators=E, dt=dt, generator="CUSTOM", flow=flow)


def steps_to_row2(dt):
    """The 0-based step in which int(time) % 86400 first passes ROW2_AT (the time search's `<` is strict), with the
    oracle's own accumulation of the time."""
    t, k = 0.0, 0
    while True:
        t += dt
        if int(t) % 86400 > ROW2_AT:
            return k
        k += 1


@functools.lru_cache(maxsize=None)
def custom_run(F, one_row=False):
    """The synthetic CUSTOM table for F in the oracle: all CUSTOM_N envs step under random_actions up to the step that enters row 2
    (one-row table: 60 steps). Keeps the sampled envs' per-step outputs and every env's horizon and queue findings."""
    flow = one_row_flow_f2() if one_row else edge_flow(F)
    cfg = custom_config(F, flow)
    E, dt = CUSTOM[F]
    K2 = 60 if one_row else steps_to_row2(dt)
    acts = random_actions(2000 + F + one_row, K2 + 30, CUSTOM_N, F, E)
    out = dict(flow=flow, K2=K2, actions=acts, rows=np.zeros((K2, len(CUSTOM_SAMPLE), 4)), envs={}, crossed=0,
               max_queue=0, max_count_sampled=0, log=collections.Counter(), src_eq_dst=0)
    for e in range(CUSTOM_N):
        tr = Tracked(cfg, CUSTOM_SEED + e)
        for k in range(K2):
            r = row(*tr.step([int(x) for x in acts[k, e]]))
            out["crossed"] += tr.crossed
            if e in CUSTOM_SAMPLE:
                out["rows"][k, CUSTOM_SAMPLE.index(e)] = r
        assert one_row or tr.env.time_index == 1
        out["max_queue"] = max(out["max_queue"], tr.env.max_queue)
        if e in CUSTOM_SAMPLE:
            out["envs"][e] = tr
            out["max_count_sampled"] = max(out["max_count_sampled"], tr.env.np.max_count)
            out["log"].update(tr.log)
    return out


# ---------------------------------------------------------------------------------------------- the stream horizon
HORIZON_A = dict(F=12, E=4, dt=0.5, Q=512, steps=40, N=96, total_lam=96.0)
HORIZON_B = dict(particle_number=250, steps=30, N=64, seed=500)
HORIZON_C = dict(particle_number=700, N=64, seed=600)


def horizon_a_flow():
    c = HORIZON_A
    F = c["F"]
    return synth_flow(F, [(0.0, np.full(F, c["total_lam"] / F / c["dt"]), np.ones((F, F)))])


@functools.lru_cache(maxsize=None)
def horizon_a_run():
    """Case A in the oracle: seeds 0..N-1, actions [-1, 0] * E. Per env the step of its first crossing (-1: never), the
    outputs up to it, and the oracle envs at the end of their run; those of flagged envs have gone through the crossing
    step, which the device does not finish, and compare with nothing."""
    c = HORIZON_A
    flow = horizon_a_flow()
    cfg = O.Config(floors=c["F"], elevators=c["E"], dt=c["dt"], generator="CUSTOM", flow=flow)
    act = [-1, 0] * c["E"]
    first = np.full(c["N"], -1)
    rows = np.zeros((c["steps"], c["N"], 4))
    envs, longest = [], 0
    for e in range(c["N"]):
        tr = Tracked(cfg, e)
        for k in range(c["steps"]):
            r = row(*tr.step(act))
            if tr.crossed:
                first[e] = k
                break
            rows[k, e] = r
        envs.append(tr)
        longest = max(longest, tr.env.max_queue)
    return dict(flow=flow, first=first, rows=rows, envs=envs, max_queue=longest)


@functools.lru_cache(maxsize=None)
def horizon_b_run():
    """Case B in the oracle: the default building with 250 particles, random actions. Every env runs for the horizon
    count; every 8th and the last keep their outputs for the comparison."""
    c = HORIZON_B
    cfg = O.Config(generator="UNIFORM", dt=0.5, particle_number=c["particle_number"], generation_interval=150.0)
    acts = random_actions(3000, c["steps"], c["N"], 10, 4)
    sample = tuple(range(0, c["N"], 8)) + (c["N"] - 1,)
    out = dict(actions=acts, sample=sample, rows=np.zeros((c["steps"], len(sample), 4)), envs=[], crossed=0,
               min_words=1 << 30, block_crossings=0)
    for e in range(c["N"]):
        tr = Tracked(cfg, c["seed"] + e)
        for k in range(c["steps"]):
            r = row(*tr.step([int(x) for x in acts[k, e]]))
            out["crossed"] += tr.crossed
            out["min_words"] = min(out["min_words"], tr.py_words)
            out["block_crossings"] += tr.py_words > MT - tr.py_pos
            if e in sample:
                out["rows"][k, sample.index(e)] = r
        if e in sample:
            out["envs"].append(tr)
    return out


# ---------------------------------------------------------------------------------------------- a wrapped queue ring
WRAP = dict(F=4, E=1, dt=1.0, rates=(0.25, 0.05, 0.05, 0.25), steps=1200, N=24, seed=0)
WRAP_SAMPLE = (0, 6, 14, 23)


def wrap_flow():
    return synth_flow(4, [(0.0, np.asarray(WRAP["rates"]), np.ones((4, 4)) - np.eye(4))])


def wrap_actions():
    """Random targets and directions held for 8 steps each, so that the one car gets somewhere and opens its door."""
    c = WRAP
    a = random_actions(4000, (c["steps"] + 7) // 8, c["N"], c["F"], c["E"])
    return np.repeat(a, 8, axis=0)[:c["steps"]].copy()


@functools.lru_cache(maxsize=None)
def wrap_run():
    """The wrapped-ring case in the oracle. First every env plainly, for the longest queue: Q is that plus 1. Then the sampled envs with the
    ring model at that Q; `probes` holds, per sampled env that wraps, (env, step, queue, head, len) of its first wrapped
    queue at a step's end."""
    c = WRAP
    flow, acts = wrap_flow(), wrap_actions()
    cfg = O.Config(floors=c["F"], elevators=c["E"], dt=c["dt"], generator="CUSTOM", flow=flow)
    longest = 0
    for e in range(c["N"]):
        env = O.Env(cfg, c["seed"] + e)
        for k in range(c["steps"]):
            env.step([int(x) for x in acts[k, e]])
        longest = max(longest, env.max_queue)
    Q = longest + 1
    out = dict(flow=flow, actions=acts, Q=Q, rows=np.zeros((c["steps"], len(WRAP_SAMPLE), 4)), envs=[], probes=[],
               log=collections.Counter(), delivered=0, crossed=0)
    for j, e in enumerate(WRAP_SAMPLE):
        tr = Tracked(cfg, c["seed"] + e, Q=Q)
        for k in range(c["steps"]):
            out["rows"][k, j] = row(*tr.step([int(x) for x in acts[k, e]]))
            out["crossed"] += tr.crossed
            wrapped = tr.wrapped_queues()
            if wrapped and not any(p[0] == e for p in out["probes"]):
                out["probes"].append((e, k, wrapped[0]) + tr.queue(wrapped[0]))
        out["envs"].append(tr)
        out["log"].update(tr.log)
        out["delivered"] += tr.delivered
    return out
