"""Host restatement of the reference's LiftSim (metagym/liftsim/environment/), one random.Random and one
np.random.RandomState per env.

TEST INFRASTRUCTURE. `Env` is one building on its own two streams (the reference's env.seed(s) seeds the global
`random` and `numpy.random` modules with s; here they are private objects seeded the same way). It is written from the
reference's behaviour, step for step in the reference's order, and pinned to runs of the
unmodified reference in tests/golden/liftsim.npz. `mansion_state()` returns the reference's MansionState namedtuple.
"""
import collections
import configparser
import random

import numpy as np

EPSILON = 1.0e-2
GRAVITY = 9.80
GIVE_UP = 300

ElevatorState = collections.namedtuple("ElevatorState", [
    "Floor", "MaximumFloor", "Velocity", "MaximumSpeed", "Direction", "DoorState", "CurrentDispatchTarget",
    "DispatchTargetDirection", "LoadWeight", "MaximumLoad", "ReservedTargetFloors", "OverloadedAlarm",
    "DoorIsOpening", "DoorIsClosing"])
MansionState = collections.namedtuple("MansionState", ["ElevatorStates", "RequiringUpwardFloors",
                                                       "RequiringDownwardFloors"])

# MansionConfig defaults (mansion_config.py)
MAX_ACC, MAX_SPD, ENTER_T, DOOR_V, DOOR_P, STANDBY_P = 1.0, 2.0, 2.0, 0.5, 350, 100
MAX_LOAD, MPEE, RATED, NET, PULLEY, MOTOR_EFF = 1600, 2, 600, 300, 0.27, 0.8


class Config(object):
    """The reference's config.ini sections as plain values."""

    def __init__(self, floors=10, elevators=4, floor_height=4.0, dt=0.5, generator="CUSTOM", flow=None,
                 particle_number=12, generation_interval=150.0):
        if not dt <= 1:
            raise AssertionError("RunningTimeStep in config.ini must be less than 1 in order to ensure accuracy")
        if generator not in ("CUSTOM", "UNIFORM"):
            raise RuntimeError("No such generator type: %s" % generator)
        self.F, self.E, self.h, self.dt = int(floors), int(elevators), float(floor_height), float(dt)
        self.generator = generator
        self.particle_number, self.generation_interval = int(particle_number), float(generation_interval)
        self.window = int(600 / self.dt)
        self.tables = custom_tables(flow, self.F) if generator == "CUSTOM" else None


def read_config(path):
    """(floors, elevators, floor_height, dt, generator, custom_data_file, particle_number, interval) of a config.ini."""
    c = configparser.ConfigParser()
    c.read(path)
    g = c["PersonGenerator"]
    return dict(dt=float(c["Configuration"]["RunningTimeStep"]), floors=int(c["MansionInfo"]["NumberOfFloors"]),
                floor_height=float(c["MansionInfo"]["FloorHeight"]), elevators=int(c["MansionInfo"]["ElevatorNumber"]),
                generator=g["PersonGeneratorType"], custom_data_file=g.get("CustomDataFile"),
                particle_number=int(g.get("ParticleNumber", 12)),
                generation_interval=float(g.get("GenerationInterval", 150)))


class Tables(object):
    pass


def custom_tables(flow, F):
    """The CUSTOM generator's tables from the flow array ([T, 2 + F (F + 1)] float64), with the reference's float32 / NEP 50
    expressions: start times [T], in_density float32 [T, F], sample_prob float32 [T, F, F]."""
    flow = np.asarray(flow)
    t = Tables()
    T = flow.shape[0]
    if int(flow[0][0]) != F:
        raise AssertionError("The dimension of the data file does not match the floor number, %d and %d"
                             % (int(flow[0][0]), F))
    pf = flow[:, 1:]
    if pf.shape[1] != 1 + F * (F + 1):
        raise AssertionError("The column of the dataset file do not match the mansion")
    dens = np.zeros([T, F], dtype="float32")
    out = np.zeros([T, F, F], dtype="float32")
    for i in range(T):
        gap = pf[i + 1][0] - pf[i][0] if i < T - 1 else 86400 - pf[i][0]
        if not gap > 0.0:
            raise AssertionError("The time interval must be above zero")
        for j in range(F):
            dens[i][j] = 1.0 / gap * pf[i][j * (F + 1) + 1]
            out[i][j] = pf[i][(j * (F + 1) + 2):((j + 1) * (F + 1) + 1)]
    prob = np.zeros([T, F, F], dtype="float32")
    for i in range(T):
        for j in range(F):
            prob[i, j] = out[i][j] / (1.0e-5 + out[i][j].sum())
    t.times, t.dens, t.out, t.prob, t.T = pf[:, 0].copy(), dens, out, prob, T
    return t


class Elevator(object):
    def __init__(self, cfg):
        self.c = cfg
        self.pos = 0.0
        self.vel = 0.0
        self.load = 0.0
        self.door = 0.0
        self.opening = False
        self.closing = False
        self.keep_left = 0.0
        self.lag = 2.0 + cfg.dt
        self.targets = []
        self.clicked = set()
        self.dispatch = 0
        self.dispatch_dir = 1
        self.loaded = [[] for _ in range(cfg.F)]   # per target floor: (weight, appear)
        self.entering = []                         # [weight, target, appear, left]
        self.exiting = []                          # [weight, appear, left]
        self.unloading = False
        self.is_entering = False
        self.direction = 0
        self.alarm = 0.0

    def state(self):
        return ElevatorState(self.pos / self.c.h + 1, self.c.F, self.vel, MAX_SPD, self.direction, self.door,
                             self.dispatch, self.dispatch_dir, self.load, MAX_LOAD, list(self.targets), self.alarm,
                             self.opening, self.closing)

    def nearest(self):
        cf = self.pos / self.c.h + 1.0
        n = int(cf + 0.5)
        return n, n - float(cf)

    def stopped(self):
        return abs(self.vel) < EPSILON

    def fully_open(self):
        return self.door > 1.0 - EPSILON

    def valid_target(self, f):
        if f < 1 or f > self.c.F:
            return False
        cf = self.pos / self.c.h + 1.0
        if abs(cf - f) < EPSILON and abs(self.vel) < EPSILON:
            return True
        sign = -1 if self.vel < 0.0 else 1
        stop = self.pos + sign * (0.5 * self.vel * self.vel / MAX_ACC)
        tp = (f - 1) * self.c.h
        if self.direction > 0:
            return not (tp + 0.5 * EPSILON < stop)
        if self.direction < 0:
            return not (tp > stop + 0.5 * EPSILON)
        return True

    def insert(self, f):
        if f in self.targets:
            return
        at = len(self.targets)
        for i, x in enumerate(self.targets):
            if (self.direction >= 0 and x > f) or (self.direction < 0 and x < f):
                at = i
                break
        self.targets.insert(at, f)

    def true_target(self):
        first = self.targets[0] if self.targets else 0
        if self.alarm > EPSILON or not self.valid_target(self.dispatch):
            return first
        if not self.targets:
            return self.dispatch
        if self.direction >= 0:
            return self.dispatch if self.dispatch < first else first
        return self.dispatch if self.dispatch > first else first

    def request_open(self):
        if self.stopped() and self.door < 1.0 - EPSILON and self.alarm < EPSILON:
            self.opening = True
            self.keep_left = self.lag
            self.closing = False

    def request_close(self):
        if self.door > EPSILON and not self.opening and not self.unloading and not self.is_entering \
                and self.keep_left < EPSILON:
            self.closing = True

    def person_in(self, p):
        weight, src = p[0], p[3]
        cf = self.pos / self.c.h + 1.0
        if abs(src - cf) > EPSILON or abs(self.vel) > EPSILON or self.door < 1.0 - 2.0 * EPSILON:
            return False
        if len(self.entering) >= MPEE:
            return False
        w = self.load
        for q in self.entering:
            w += q[0]
        if w + weight > MAX_LOAD:
            self.alarm = 2.0
            self.request_close()
            return False
        self.entering.append([weight, p[1], p[2], ENTER_T])
        return True

    def run(self, now):
        c = self.c
        dt = c.dt
        tf = self.true_target()
        offset = 0.0 if tf <= 0 else (tf - 1) * c.h - self.pos
        no_reserved = len(self.targets) < 1
        if self.stopped() and tf > 0 and abs(offset) < EPSILON:
            if self.door > 1.0 - EPSILON:
                self.clicked.discard(tf)
                if tf in self.targets:
                    self.targets.remove(tf)
                self.dispatch = 0
            self.request_open()
        digit = self.pos / c.h + 1.0
        if no_reserved and self.stopped() and self.door < EPSILON:
            self.direction = 0
        if self.direction == 0 and self.stopped() and self.dispatch > 0 and abs(self.dispatch - digit) < EPSILON \
                and self.dispatch_dir in (1, -1):
            self.direction = self.dispatch_dir
        if self.stopped() and self.pos <= EPSILON:
            self.direction = 1
        if self.stopped() and self.pos >= (c.F - 1) * c.h - EPSILON:
            self.direction = -1
        if self.targets and self.direction == 0:
            if self.targets[0] > digit:
                self.direction = -1
            elif self.targets[0] < digit:
                self.direction = 1
        for b in sorted(self.clicked):
            if b not in self.targets and self.valid_target(b):
                self.insert(b)
        if tf > 0:
            df = float(tf) - 1.0 - self.pos / c.h
            if df * self.direction < -EPSILON and tf in self.targets:
                self.targets.remove(tf)
        if abs(self.vel) > EPSILON:
            if self.opening:
                self.opening = False
            elif self.door > EPSILON:
                self.closing = True
        if self.door < EPSILON:
            self.closing = False
        elif self.door > 1.0 - EPSILON:
            self.opening = False
        if self.entering or self.exiting:
            self.closing = False
            if self.door < 1.0 - EPSILON:
                self.opening = True
                self.keep_left = self.lag
        if self.opening:
            self.door = min(1.0, self.door + DOOR_V)
        elif self.closing:
            self.door = max(0.0, self.door - DOOR_V)
        hold = self.opening or self.closing or self.door > EPSILON
        eff = dt
        if hold:
            if abs(self.vel) < dt * MAX_ACC:
                nv = 0.0
                eff = abs(self.vel) / MAX_ACC
            elif self.vel > 0:
                nv = self.vel - dt * MAX_ACC
            else:
                nv = self.vel + dt * MAX_ACC
        else:
            nv, eff = plan(self.vel, offset, MAX_ACC, MAX_SPD, dt)
        self.pos += 0.5 * (nv + self.vel) * eff + nv * (dt - eff)
        acc = (nv - self.vel) / max(eff, EPSILON)
        f1 = (NET + self.load) * (GRAVITY + acc)
        f2 = RATED * (GRAVITY - acc)
        m = abs(f1 - f2) * PULLEY / 1.0 / 1.0
        energy = m * abs((self.vel + nv) / 2) / 1.0 * 1.0 / MOTOR_EFF * eff + STANDBY_P * dt
        self.vel = nv
        if self.opening or self.closing:
            energy += DOOR_P * dt
        self.alarm = max(0.0, self.alarm - dt)
        if self.fully_open():
            self.keep_left = max(0.0, self.keep_left - dt)
        delivered = 0
        done = []
        for i, q in enumerate(self.exiting):
            q[2] -= dt
            if q[2] < EPSILON:
                done.append(i)
        for i in reversed(done):
            q = self.exiting.pop(i)
            self.load -= q[0]
            delivered += 1
        floor, dd = self.nearest()
        fi = floor - 1
        done = []
        for i, q in enumerate(self.entering):
            q[3] -= dt
            if q[3] < EPSILON:
                done.append(i)
        for i in reversed(done):
            q = self.entering.pop(i)
            self.loaded[q[1] - 1].append((q[0], q[2]))
            self.load += q[0]
            if 0 < q[1] <= c.F:
                self.clicked.add(q[1])
        if self.stopped() and self.fully_open() and abs(dd) < EPSILON and self.loaded[fi] \
                and len(self.exiting) < MPEE:
            w, t = self.loaded[fi].pop(0)
            self.exiting.append([w, t, ENTER_T])
        self.is_entering = len(self.entering) > 0
        self.unloading = len(self.exiting) > 0 or len(self.loaded[fi]) > 0
        if self.fully_open():
            self.request_close()
        return energy, delivered, sum(len(r) for r in self.loaded)


def plan(v, x, acc, spd, dt):
    """utils.velocity_planner: (velocity at the end of the step, time spent accelerating)."""
    def clip(a, m):
        return max(-m, min(m, a))
    sv = 1.0 if v > 0 else -1.0
    eff = dt
    if 0.1 * EPSILON > abs(x):
        if abs(v) < abs(acc * dt):
            eff = abs(v) / abs(acc)
        return v - sv * acc * eff, eff
    sx = 1.0 if x > 0 else -1.0
    rs = 0.5 * v * abs(v) / acc + v * dt
    ve = clip(v + sx * acc * dt, spd)
    re = 0.5 * ve * abs(ve) / acc + 0.5 * (ve + v) * dt
    if (sx > 0 and x > re - 0.1 * EPSILON) or (sx < 0 and x < re + 0.1 * EPSILON):
        return ve, eff
    if (sx > 0 and x > rs - 0.1 * EPSILON) or (sx < 0 and x < rs + 0.1 * EPSILON):
        fs, fe, fm = 0.0, 1.0, 0.5
        out = v
        for _ in range(5):
            tv = clip(v + sx * fm * acc * dt, spd)
            r = 0.5 * tv * abs(tv) / acc + 0.5 * (tv + v) * dt
            if (x > 0 and x > r) or (x < 0 and x < r):
                fs = fm
                out = tv
            else:
                fe = fm
            fm = 0.5 * (fs + fe)
        return out, eff
    if abs(x) < 0.1 * EPSILON:
        if abs(v) < abs(acc * dt):
            eff = abs(v) / abs(acc)
        return v - sv * acc * eff, eff
    ra = clip(-0.5 * abs(v * v / x) * sv, acc)
    if abs(v) < abs(ra * dt):
        eff = abs(v) / abs(ra)
    return v + ra * eff, eff


class Env(object):
    """One building on its own streams: Env(cfg, seed) is the reference's LiftSim after env.seed(seed)."""

    def __init__(self, cfg, seed=0):
        self.c = cfg
        self.py = random.Random(seed)
        self.np = np.random.RandomState(seed)
        self.time_index = 0   # the CUSTOM generator's _cur_time_index: reset() keeps it
        self.stats = collections.deque()   # newest first: (delivered, generated, abandoned, waiting, energy)
        self.reset()

    def reset(self):
        c = self.c
        self.elev = [Elevator(c) for _ in range(c.E)]
        self.time = 0.0
        self.last_gen = 0.0
        self.button = [[False, False] for _ in range(c.F)]
        self.up = [collections.deque() for _ in range(c.F)]     # newest at index 0; person = (weight, target, appear, src)
        self.down = [collections.deque() for _ in range(c.F)]
        self.max_queue = 0
        return self.mansion_state()

    def mansion_state(self):
        return MansionState([e.state() for e in self.elev], [i + 1 for i in range(self.c.F) if self.button[i][0]],
                            [i + 1 for i in range(self.c.F) if self.button[i][1]])

    # ------------------------------------------------------------------ generators
    def _weight(self):
        w = self.py.normalvariate(50, 10)
        while w < 20 or w > 100:
            w = self.py.normalvariate(50, 10)
        return w

    def _search(self, beg, end, t):
        times, T = self.c.tables.times, self.c.tables.T
        while True:
            if beg >= T - 1 or not times[beg + 1] < t:
                return beg
            if not times[end] > t:
                return end
            m = (beg + end) // 2
            if times[m] < t:
                beg, end = m, end - 1
            else:
                beg, end = beg + 1, m

    def _custom(self):
        tb, F = self.c.tables, self.c.F
        gap = self.time - self.last_gen
        t = int(self.time) % 86400
        if self.time_index + 1 < tb.T and tb.times[self.time_index + 1] < t:
            self.time_index = self._search(self.time_index + 1, tb.T - 1, t)
        if tb.times[self.time_index] > t:
            self.time_index = self._search(0, self.time_index, t)
        lam = tb.dens[self.time_index] * gap
        n = self.np.poisson(lam, size=lam.shape)
        out = []
        for i in range(F):
            if n[i] > 0:
                k = self.np.multinomial(n[i], tb.prob[self.time_index][i])
                for j in range(F):
                    for _ in range(k[j]):
                        out.append((self._weight(), i + 1, j + 1))
        return out

    def _uniform(self):
        c, r = self.c, self.py
        gap = self.time - self.last_gen
        out = []
        for _ in range(c.particle_number):
            if r.random() < gap / c.generation_interval:
                s, t = r.randint(1, c.F), r.randint(1, c.F)
                while s == t:
                    s, t = r.randint(1, c.F), r.randint(1, c.F)
                out.append((r.uniform(20, 100), s, t))
        return out

    # ------------------------------------------------------------------ one step
    def step(self, action):
        c = self.c
        if len(action) != 2 * c.E:
            raise AssertionError("Action is supposed to be a list with length ElevatorNumber * 2")
        for k in range(c.E):
            tf, d = int(action[2 * k]), int(action[2 * k + 1])
            if not (-1 <= tf <= c.F) or d not in (-1, 0, 1):
                raise AssertionError("invalid action")
        self.time += c.dt
        persons = self._custom() if c.generator == "CUSTOM" else self._uniform()
        self.last_gen = self.time
        for w, s, t in persons:
            if s < t:
                self.up[s - 1].appendleft((w, t, self.time, s))
            elif s > t:
                self.down[s - 1].appendleft((w, t, self.time, s))
        for k in range(c.E):
            tf, d = int(action[2 * k]), int(action[2 * k + 1])
            if 0 <= tf <= c.F:
                self.elev[k].dispatch = tf
                self.elev[k].dispatch_dir = d
        energy = [0.0] * c.E
        delivered = loaded = 0
        for k in range(c.E):
            energy[k], dv, ld = self.elev[k].run(self.time)
            delivered += dv
            loaded += ld
        for f in range(c.F):
            self.button[f][0] = len(self.up[f]) > 0
            self.button[f][1] = len(self.down[f]) > 0
            self.max_queue = max(self.max_queue, len(self.up[f]), len(self.down[f]))
        order = list(range(c.E))
        self.py.shuffle(order)
        for k in order:
            e = self.elev[k]
            floor, dd = e.nearest()
            is_open = e.fully_open() and abs(dd) < 0.05
            ready = not e.unloading and not e.is_entering
            fi = floor - 1
            if is_open:
                if e.direction == 1:
                    self.button[fi][0] = False
                elif e.direction == -1:
                    self.button[fi][1] = False
            if ready and is_open and e.direction != 0:
                q = self.up[fi] if e.direction == 1 else self.down[fi]
                for i in range(len(q) - 1, -1, -1):
                    if e.person_in(q[i]):
                        del q[i]
                    elif not e.alarm:
                        break
        given_up = 0
        for f in range(c.F):
            for q in (self.up[f], self.down[f]):
                while q and self.time - q[-1][2] > GIVE_UP:
                    q.pop()
                    given_up += 1
        waiting = 0
        for f in range(c.F):
            waiting += c.dt * len(self.up[f])
            waiting += c.dt * len(self.down[f])
        waiting += loaded * c.dt
        en = float(sum(energy))
        self.stats.appendleft((delivered, len(persons), given_up, waiting, en))
        if len(self.stats) > c.window:
            self.stats.pop()
        reward = -(waiting + 5e-4 * en + 300 * given_up) * 1.0e-4
        return reward, dict(time_consume=waiting, energy_consume=en, given_up_persons=given_up)

    def statistics(self):
        s = [0, 0, 0, 0, 0]
        for row in self.stats:
            for i in range(5):
                s[i] += row[i]
        return {"DeliveredPersons(10Minutes)": int(s[0]), "GeneratedPersons(10Minutes)": int(s[1]),
                "AbandonedPersons(10Minutes)": int(s[2]), "EnergyConsumption(10Minutes)": float(s[4]),
                "TotalWaitingTime(10Minutes)": float(s[3])}


def scripted_actions(seed, steps, F, E):
    """The golden runs' actions: int32 [steps, 2E], targets in [-1, F] and directions in {-1, 0, 1}, from a private
    RandomState (so -1 targets and 0 directions occur)."""
    rs = np.random.RandomState(1000 + seed)
    a = np.empty((steps, 2 * E), np.int32)
    a[:, 0::2] = rs.randint(-1, F + 1, size=(steps, E))
    a[:, 1::2] = rs.randint(-1, 2, size=(steps, E))
    return a


def step_digest(h, reward, info, state):
    """Feed one step into a hashlib object: reward, info and the hall buttons."""
    h.update(np.array([reward, info["time_consume"], info["energy_consume"]], np.float64).tobytes())
    h.update(np.array([info["given_up_persons"]], np.int64).tobytes())
    h.update(np.array(state.RequiringUpwardFloors + [0] + state.RequiringDownwardFloors + [0], np.int16).tobytes())


def state_array(state):
    """A MansionState as float64 [E, 14 + F] (ReservedTargetFloors 0-padded after its count) plus the button lists."""
    F = state.ElevatorStates[0].MaximumFloor
    rows = []
    for s in state.ElevatorStates:
        r = [s.Floor, s.MaximumFloor, s.Velocity, s.MaximumSpeed, s.Direction, s.DoorState, s.CurrentDispatchTarget,
             s.DispatchTargetDirection, s.LoadWeight, s.MaximumLoad, len(s.ReservedTargetFloors), s.OverloadedAlarm,
             s.DoorIsOpening, s.DoorIsClosing]
        rows.append(r + list(s.ReservedTargetFloors) + [0] * (F - len(s.ReservedTargetFloors)))
    up = np.zeros(F, np.uint8)
    down = np.zeros(F, np.uint8)
    up[np.asarray(state.RequiringUpwardFloors, int) - 1] = 1
    down[np.asarray(state.RequiringDownwardFloors, int) - 1] = 1
    return np.asarray(rows, np.float64), up, down
