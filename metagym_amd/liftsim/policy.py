"""Learned dispatchers for `LiftSim.rollout_policy`: P small networks, each shared by its building's elevators, evaluated
inside the rollout launch (include/metagym_hip.h, mg_liftsim_policy_rollout).

The arithmetic is defined exactly, so the closed loop can be replayed bit for bit. F floors, E elevators, H hidden ReLU
units (1 <= H <= 64), A = 2F + 2 choices. Every operation is float32, rounded once, never fused, in this order; a double
input is first converted to float32 (round to nearest even). For elevator el of a building, from the state before the step:

    x[0..7] = f32(raw[i]) * scale[i]
              raw = Floor, Velocity, Direction, DoorState, LoadWeight, OverloadedAlarm, DoorIsOpening (0/1),
                    DoorIsClosing (0/1)
    for j in 0..H-1:
        z = b[j]
        for i in 0..7:  z = z + ws[j][i] * x[i]
        z = z + we[j][el]
        d = CurrentDispatchTarget;  if 0 <= d <= F:  z = z + wt[j][d]
        for f in 1..F ascending, if f in ReservedTargetFloors[el]:   z = z + wr[j][f-1]
        for f in 1..F ascending, if f in RequiringUpwardFloors:      z = z + wu[j][f-1]
        for f in 1..F ascending, if f in RequiringDownwardFloors:    z = z + wd[j][f-1]
        h[j] = (z > 0) ? z : 0
    for c in 0..A-1:  l[c] = bo[c];  for j in 0..H-1:  l[c] = l[c] + wo[c][j] * h[j]
    choice = 0;  for c in 1..A-1:  if l[c] > l[choice]:  choice = c

One-hot and bit inputs are lookups: each costs one add, or none, never a multiply-add (a pre-activation of -0 stays -0
whatever the weights hold). Ties and NaN logits resolve to the lowest index. Choice c < F is (c + 1, +1), F <= c < 2F is
(c - F + 1, -1), c = 2F is (0, 1), the rule dispatcher's "nothing", and c = 2F + 1 is (-1, 1): no new dispatch.

`LiftPolicy.reference` evaluates exactly this in numpy float32. Nothing here needs a GPU to import.

    pol = LiftPolicy(ws, we, wt, wr, wu, wd, b, wo, bo)     # [P,H,8] [P,H,E] [P,H,F+1] [P,H,F] x3 [P,H] [P,A,H] [P,A]
    out = env.rollout_policy(pol, steps=600, policy_ids=ids, record=("reward", "actions"))

The recurrent form (`LiftRecurrentPolicy`, mg_liftsim_rpolicy_rollout): the network is still shared by its building's
elevators, and each elevator has a memory of its own. h[el] is elevator el's memory before the step, pc[el] its previous
choice (-1: none), pr the building's previous reward; H hidden units clamped to [-1, 1]:

    x[0..7] = f32(raw[i]) * scale[i]      (raw as for mg_liftsim_policy)
    for j in 0..H-1:
        z = b[j]
        for i in 0..7:  z = z + ws[j][i] * x[i]
        z = z + we[j][el]
        d = CurrentDispatchTarget;  if 0 <= d <= F:  z = z + wt[j][d]
        for f in 1..F ascending, if f in ReservedTargetFloors[el]:   z = z + wr[j][f-1]
        for f in 1..F ascending, if f in RequiringUpwardFloors:      z = z + wu[j][f-1]
        for f in 1..F ascending, if f in RequiringDownwardFloors:    z = z + wd[j][f-1]
        if pc[el] >= 0:  z = z + wc[j][pc[el]]
        z = z + wq[j] * pr
        for i in 0..H-1:  z = z + wh[j][i] * h[el][i]
        hn[j] = z > 1 ? 1 : (z < -1 ? -1 : z)
    h[el] = hn
    for c in 0..A-1:  l[c] = bo[c];  for j in 0..H-1:  l[c] = l[c] + wo[c][j] * h[el][j]
    choice = 0;  for c in 1..A-1:  if l[c] > l[choice]:  choice = c
    pc[el] = choice

The E elevators of a step are all evaluated on the same pre-step state and see the same pr; after the step pr = f32(reward),
the value the reward record holds. wc is a lookup like the others: one add or none. An env that is frozen (`overflow` /
`unsupported`) when a step begins evaluates nothing, records (0, 0) per elevator and keeps its carry as it stood; in the step
in which it overflows the policy has run (h and pc are that step's) and pr is f32 of the 0 the reward record holds. There
is no done input (LiftSim.step never returns done) and no exploration draw.

    rpol = LiftRecurrentPolicy(ws, we, wt, wr, wu, wd, wc, wq, wh, b, wo, bo)     # wc [P,H,A], wq [P,H], wh [P,H,H]
    out = env.rollout_policy(rpol, steps=300, policy_ids=ids)                    # out["state"]: the end carry
    out = env.rollout_policy(rpol, steps=300, policy_ids=ids, state=out["state"])
"""
import numpy as np

from .._policy import PackedPolicySet, f32_array, pad4, to_numpy

MAX_HIDDEN = 64
MAX_FLOORS, MAX_ELEVATORS = 128, 32
N_SCALARS = 8
MAXIMUM_LOAD = 1600
RAW = ("Floor", "Velocity", "Direction", "DoorState", "LoadWeight", "OverloadedAlarm", "DoorIsOpening", "DoorIsClosing")


def _check_sizes(hidden, floors, elevators):
    if not (1 <= int(hidden) <= MAX_HIDDEN):
        raise ValueError("hidden units must be in [1, %d], got %r" % (MAX_HIDDEN, hidden))
    if not (2 <= int(floors) <= MAX_FLOORS):
        raise ValueError("floors must be in [2, %d], got %r" % (MAX_FLOORS, floors))
    if not (1 <= int(elevators) <= MAX_ELEVATORS):
        raise ValueError("elevators must be in [1, %d], got %r" % (MAX_ELEVATORS, elevators))
    return int(hidden), int(floors), int(elevators)


def unit_groups(floors, elevators):
    """(name, offset, length) of the groups of one hidden unit's record, and the record's length RU."""
    F, E = int(floors), int(elevators)
    groups, o = [], 0
    for name, n in (("b", 1), ("ws", N_SCALARS), ("we", E), ("wt", F + 1), ("wr", F), ("wu", F), ("wd", F)):
        groups.append((name, o, n))
        o += pad4(n)
    return groups, o


def param_count(hidden, floors, elevators):
    """Floats per packed policy (what mg_liftsim_policy_param_count returns)."""
    H, F, E = _check_sizes(hidden, floors, elevators)
    return H * unit_groups(F, E)[1] + (2 * F + 2) * (4 + pad4(H))


def default_scale(floors):
    """[f32(1) / f32(F), 0.5, 1, 1, f32(1) / f32(1600), 1, 1, 1], computed in float32."""
    one = np.float32(1.0)
    return np.array([one / np.float32(int(floors)), 0.5, 1.0, 1.0, one / np.float32(MAXIMUM_LOAD), 1.0, 1.0, 1.0], np.float32)


class LiftPolicy(PackedPolicySet):
    """P dispatcher networks: ws [P, H, 8], we [P, H, E], wt [P, H, F+1], wr wu wd [P, H, F], b [P, H], wo [P, A, H], bo [P, A]
    with A = 2F + 2, all float32 and finite; scale float32 [8], the same for all policies (None: `default_scale(F)`)."""

    def __init__(self, ws, we, wt, wr, wu, wd, b, wo, bo, scale=None):
        ws, we, wt = f32_array("ws", ws, 3), f32_array("we", we, 3), f32_array("wt", wt, 3)
        wr, wu, wd = f32_array("wr", wr, 3), f32_array("wu", wu, 3), f32_array("wd", wd, 3)
        b, wo, bo = f32_array("b", b, 2), f32_array("wo", wo, 3), f32_array("bo", bo, 2)
        P, H, E = we.shape
        F = wr.shape[2]
        if P < 1:
            raise ValueError("a policy set needs at least one policy")
        _check_sizes(H, F, E)
        A = 2 * F + 2
        want = dict(ws=(P, H, N_SCALARS), we=(P, H, E), wt=(P, H, F + 1), wr=(P, H, F), wu=(P, H, F), wd=(P, H, F), b=(P, H),
                    wo=(P, A, H), bo=(P, A))
        got = dict(ws=ws, we=we, wt=wt, wr=wr, wu=wu, wd=wd, b=b, wo=wo, bo=bo)
        for name, shape in want.items():
            if got[name].shape != shape:
                raise ValueError("shapes must be ws [P,H,8], we [P,H,E], wt [P,H,F+1], wr wu wd [P,H,F], b [P,H], wo [P,A,H], "
                                 "bo [P,A] with A = 2F + 2; %s is %s, not %s" % (name, got[name].shape, shape))
        scale = default_scale(F) if scale is None else f32_array("scale", scale, 1)
        if scale.shape != (N_SCALARS,):
            raise ValueError("scale must have shape (8,), got %s" % (scale.shape,))
        self.ws, self.we, self.wt, self.wr, self.wu, self.wd, self.b, self.wo, self.bo = ws, we, wt, wr, wu, wd, b, wo, bo
        self.scale = scale
        self.num_policies, self.hidden, self.floors, self.elevators, self.choices = P, H, F, E, A
        self._gathered = None

    @property
    def param_count(self):
        return param_count(self.hidden, self.floors, self.elevators)

    def pack(self):
        """float32 [P, param_count]: the layout the kernel reads (documented in include/metagym_hip.h). Per hidden unit j a
        record of RU floats holding the groups b[j] | ws[j] | we[j] | wt[j] | wr[j] | wu[j] | wd[j], each zero-padded to a
        multiple of four floats; then per choice c a record of 4 + HP floats (bo[c], 0, 0, 0, wo[c][0..H-1], zeros up to
        HP). Every record and every group starts on a multiple of four floats."""
        P, H, F, E, A = self.num_policies, self.hidden, self.floors, self.elevators, self.choices
        groups, ru = unit_groups(F, E)
        rc = 4 + pad4(H)
        out = np.zeros((P, self.param_count), np.float32)
        unit = out[:, :H * ru].reshape(P, H, ru)
        for name, o, n in groups:
            unit[:, :, o:o + n] = getattr(self, name).reshape(P, H, n)
        choice = out[:, H * ru:].reshape(P, A, rc)
        choice[:, :, 0] = self.bo
        choice[:, :, 4:4 + H] = self.wo
        return out

    @classmethod
    def unpack(cls, packed, hidden, floors, elevators, scale=None):
        """The inverse of `pack`."""
        packed = f32_array("packed", packed, 2)
        H, F, E = _check_sizes(hidden, floors, elevators)
        P, A = packed.shape[0], 2 * F + 2
        if packed.shape[1] != param_count(H, F, E):
            raise ValueError("packed has shape %s, hidden=%d floors=%d elevators=%d need [P, %d]"
                             % (packed.shape, H, F, E, param_count(H, F, E)))
        groups, ru = unit_groups(F, E)
        rc = 4 + pad4(H)
        unit = packed[:, :H * ru].reshape(P, H, ru)
        choice = packed[:, H * ru:].reshape(P, A, rc)
        g = {name: unit[:, :, o:o + n].copy() for name, o, n in groups}
        return cls(g["ws"], g["we"], g["wt"], g["wr"], g["wu"], g["wd"], g["b"][:, :, 0].copy(), choice[:, :, 4:4 + H].copy(),
                   choice[:, :, 0].copy(), scale)

    @staticmethod
    def actions_of(choices, floors):
        """The (DispatchTarget, DispatchTargetDirection) pairs of an integer array of choices: int32, shape + (2,)."""
        c = np.asarray(choices)
        F = int(floors)
        if c.dtype.kind not in "iu":
            raise ValueError("choices must be integers")
        if c.size and (int(c.min()) < 0 or int(c.max()) > 2 * F + 1):
            raise ValueError("choices must be in [0, %d]" % (2 * F + 1))
        c = c.astype(np.int64)
        target = np.where(c < F, c + 1, np.where(c < 2 * F, c - F + 1, np.where(c == 2 * F, 0, -1)))
        direction = np.where((c >= F) & (c < 2 * F), -1, 1)
        return np.stack([target, direction], axis=-1).astype(np.int32)

    def _gather(self, ids):
        """The parameters of the envs' policies, [n, ...] each; the last gather is kept (a loop passes the same ids)."""
        key = ids.tobytes()
        if self._gathered is None or self._gathered[0] != key:
            self._gathered = (key, tuple(getattr(self, name)[ids] for name in ("ws", "we", "wt", "wr", "wu", "wd", "b", "wo", "bo")))
        return self._gathered[1]

    def inputs(self, obs):
        """(x float32 [n, E, 8], d int [n, E], reserved bool [n, E, F], up bool [n, F], down bool [n, F]) of the arrays of
        `env.observation()` (torch or numpy)."""
        F, E = self.floors, self.elevators
        raw = [to_numpy(obs[name]) for name in RAW]
        n = raw[0].shape[0]
        for name, a in zip(RAW, raw):
            if a.shape != (n, E):
                raise ValueError("obs[%r] must have shape (%d, %d), got %s" % (name, n, E, a.shape))
        x = np.stack([(a != 0).astype(np.float32) if a.dtype == np.bool_ else a.astype(np.float32) for a in raw], axis=-1)
        x = x * self.scale
        d = to_numpy(obs["CurrentDispatchTarget"]).astype(np.int64)
        targets = to_numpy(obs["ReservedTargetFloors"]).astype(np.int64)
        count = to_numpy(obs["ReservedTargetCount"]).astype(np.int64)
        up, down = to_numpy(obs["RequiringUpwardFloors"]) != 0, to_numpy(obs["RequiringDownwardFloors"]) != 0
        if d.shape != (n, E) or targets.shape != (n, E, F) or count.shape != (n, E) or up.shape != (n, F) or down.shape != (n, F):
            raise ValueError("the observation does not belong to %d buildings of %d floors and %d elevators" % (n, F, E))
        listed = np.arange(F)[None, None, :] < count[:, :, None]
        floor = np.where(listed & (targets >= 1) & (targets <= F), targets, 0)
        member = np.zeros((n, E, F + 1), np.bool_)
        np.put_along_axis(member, floor, True, axis=2)
        assert x.dtype == np.float32
        return x, d, member[:, :, 1:], up, down

    def preactivations(self, policy_ids, x, d, reserved, up, down):
        """z float32 [n, E, H] of the definition: the sums run one term at a time, each term an array over the envs, the
        elevators and the units (which are independent of each other); the floor loops are sequential."""
        F = self.floors
        ws, we, wt, wr, wu, wd, b = self._gather(policy_ids)[:7]
        n = x.shape[0]
        with np.errstate(all="ignore"):
            z = np.broadcast_to(b[:, None, :], (n, self.elevators, self.hidden)).copy()
            for i in range(N_SCALARS):
                z = z + ws[:, None, :, i] * x[:, :, None, i]
            z = z + we.transpose(0, 2, 1)
            looked_up = (d >= 0) & (d <= F)
            looked = wt.transpose(0, 2, 1)[np.arange(n)[:, None], np.where(looked_up, d, 0)]      # [n, E, H]
            z = np.where(looked_up[:, :, None], z + looked, z)
            for f in range(F):
                if reserved[:, :, f].any():
                    z = np.where(reserved[:, :, f, None], z + wr[:, None, :, f], z)
            for f in range(F):
                if up[:, f].any():
                    z = np.where(up[:, f, None, None], z + wu[:, None, :, f], z)
            for f in range(F):
                if down[:, f].any():
                    z = np.where(down[:, f, None, None], z + wd[:, None, :, f], z)
        assert z.dtype == np.float32
        return z

    def reference(self, policy_ids, obs, return_choices=False):
        """One step of the definition above in numpy float32, vectorised over envs, elevators and units. policy_ids [n];
        obs: the arrays of `env.observation()` for n buildings (torch or numpy; [n, E], [n, E, F] with
        ReservedTargetCount, [n, F]). Returns the int32 [n, 2E] actions, ready for `env.step`, and with `return_choices`
        also the int32 [n, E] choices. The oracle of the policy half of a closed-loop rollout."""
        ids = to_numpy(policy_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("policy_ids must be a vector of integers")
        n = ids.shape[0]
        if n and (int(ids.min()) < 0 or int(ids.max()) >= self.num_policies):
            raise ValueError("policy_ids must be in [0, %d)" % self.num_policies)
        ids = ids.astype(np.int64)
        x, d, reserved, up, down = self.inputs(obs)
        if x.shape[0] != n:
            raise ValueError("policy_ids holds %d ids, the observation %d buildings" % (n, x.shape[0]))
        z = self.preactivations(ids, x, d, reserved, up, down)
        wo, bo = self._gather(ids)[7:]
        zero = np.float32(0.0)
        with np.errstate(all="ignore"):
            h = np.where(z > zero, z, zero)
            logits = np.broadcast_to(bo[:, None, :], (n, self.elevators, self.choices)).copy()
            for j in range(self.hidden):
                logits = logits + wo[:, None, :, j] * h[:, :, j:j + 1]
            choice = np.zeros((n, self.elevators), np.int32)
            best = logits[:, :, 0].copy()
            for c in range(1, self.choices):
                better = logits[:, :, c] > best
                choice = np.where(better, np.int32(c), choice)
                best = np.where(better, logits[:, :, c], best)
        assert h.dtype == np.float32 and logits.dtype == np.float32
        actions = self.actions_of(choice, self.floors).reshape(n, 2 * self.elevators)
        return (actions, choice) if return_choices else actions


# ---------------------------------------------------------------------------------------------- the recurrent form
def recurrent_unit_groups(hidden, floors, elevators):
    """(name, offset, length) of the groups of one hidden unit's record of a recurrent policy, and the record's length RU.
    b[j] and wq[j] share the first group: floats 0 and 1."""
    H, F, E = int(hidden), int(floors), int(elevators)
    groups, o = [], 0
    for name, n in (("b", 1), ("ws", N_SCALARS), ("we", E), ("wt", F + 1), ("wr", F), ("wu", F), ("wd", F), ("wc", 2 * F + 2),
                    ("wh", H)):
        groups.append((name, o, n))
        o += pad4(n)
    groups.insert(1, ("wq", 1, 1))
    return groups, o


def recurrent_param_count(hidden, floors, elevators):
    """Floats per packed recurrent policy (what mg_liftsim_rpolicy_param_count returns)."""
    H, F, E = _check_sizes(hidden, floors, elevators)
    return H * recurrent_unit_groups(H, F, E)[1] + (2 * F + 2) * (4 + pad4(H))


class LiftPolicyState(object):
    """The carry of a recurrent LiftSim rollout, the memory of every elevator of every building: h float32 [N, E, H],
    prev_choice int32 [N, E] (-1: none), prev_reward float32 [N]. Fresh: zeros, prev_choice = -1.

    On a device the storage is lane-coalesced, the arena's convention (env index fastest): h as [E][H][N], prev_choice as
    [E][N], prev_reward as [N]; the [N, ...] attributes are permuted views of it, no copies, and a launch updates them in
    place. `numpy()` gives contiguous [N, ...] arrays, what `LiftRecurrentPolicy.reference` takes.

    The carry sees `rollout_policy` steps only: a `step()` or `rollout(actions)` between two calls changes the arena and
    not the carry, so prev_reward stays the last `rollout_policy` reward."""
    __slots__ = ("h", "prev_choice", "prev_reward")

    def __init__(self, h, prev_choice, prev_reward):
        self.h, self.prev_choice, self.prev_reward = h, prev_choice, prev_reward

    @classmethod
    def zeros(cls, num_envs, elevators, hidden, device=None):
        """The fresh carry. device None: numpy arrays."""
        N, E, H = int(num_envs), int(elevators), int(hidden)
        if N < 1 or not (1 <= E <= MAX_ELEVATORS) or not (1 <= H <= MAX_HIDDEN):
            raise ValueError("a carry needs num_envs >= 1, elevators in [1, %d] and hidden in [1, %d], got %d, %d and %d"
                             % (MAX_ELEVATORS, MAX_HIDDEN, N, E, H))
        if device is None:
            return cls(np.zeros((N, E, H), np.float32), np.full((N, E), -1, np.int32), np.zeros(N, np.float32))
        import torch
        return cls(torch.zeros(E, H, N, dtype=torch.float32, device=device).permute(2, 0, 1),
                   torch.full((E, N), -1, dtype=torch.int32, device=device).t(),
                   torch.zeros(N, dtype=torch.float32, device=device))

    @property
    def num_envs(self):
        return int(self.h.shape[0])

    @property
    def elevators(self):
        return int(self.h.shape[1])

    @property
    def hidden(self):
        return int(self.h.shape[2])

    @property
    def device(self):
        """The torch device of the arrays; None for a numpy carry."""
        return self.h.device if hasattr(self.h, "detach") else None

    def clone(self):
        if self.device is None:
            return type(self)(self.h.copy(), self.prev_choice.copy(), self.prev_reward.copy())
        # clone the storage in its own order, then view it the same way
        return type(self)(self.h.permute(1, 2, 0).clone().permute(2, 0, 1), self.prev_choice.t().clone().t(),
                          self.prev_reward.clone())

    def numpy(self):
        """A host copy, contiguous [N, ...] numpy arrays."""
        return type(self)(np.ascontiguousarray(to_numpy(self.h), np.float32), np.ascontiguousarray(to_numpy(self.prev_choice), np.int32),
                          np.ascontiguousarray(to_numpy(self.prev_reward), np.float32).copy())

    def observed(self, reward):
        """The numpy carry after the env step that followed `reference`: prev_reward = float32(reward), the rest kept."""
        out = self.numpy()
        r = to_numpy(reward).astype(np.float32)
        if r.shape != (self.num_envs,):
            raise ValueError("reward must have shape (%d,), got %s" % (self.num_envs, r.shape))
        out.prev_reward = r
        return out


class LiftRecurrentPolicy(LiftPolicy):
    """P recurrent dispatcher networks: LiftPolicy's ws, we, wt, wr, wu, wd, b, wo, bo and wc [P, H, A] (the previous choice, a
    lookup), wq [P, H] (the previous reward), wh [P, H, H] (the recurrence), all float32 and finite. The module docstring
    defines the arithmetic."""
    NAMES = ("ws", "we", "wt", "wr", "wu", "wd", "b", "wo", "bo", "wc", "wq", "wh")

    def __init__(self, ws, we, wt, wr, wu, wd, wc, wq, wh, b, wo, bo, scale=None):
        LiftPolicy.__init__(self, ws, we, wt, wr, wu, wd, b, wo, bo, scale)
        wc, wq, wh = f32_array("wc", wc, 3), f32_array("wq", wq, 2), f32_array("wh", wh, 3)
        P, H, A = self.num_policies, self.hidden, self.choices
        for name, a, shape in (("wc", wc, (P, H, A)), ("wq", wq, (P, H)), ("wh", wh, (P, H, H))):
            if a.shape != shape:
                raise ValueError("shapes must be wc [P,H,A], wq [P,H], wh [P,H,H] with A = 2F + 2; %s is %s, not %s"
                                 % (name, a.shape, shape))
        self.wc, self.wq, self.wh = wc, wq, wh

    @property
    def param_count(self):
        return recurrent_param_count(self.hidden, self.floors, self.elevators)

    def pack(self):
        """float32 [P, param_count]: the layout the kernel reads (include/metagym_hip.h, mg_liftsim_rpolicy). Per hidden unit
        j a record of RU floats: b[j] wq[j] 0 0 | ws[j] | we[j] | wt[j] | wr[j] | wu[j] | wd[j] | wc[j] | wh[j], each group
        zero-padded to a multiple of four floats; then per choice c the MLP's record of 4 + HP floats."""
        P, H, F, E, A = self.num_policies, self.hidden, self.floors, self.elevators, self.choices
        groups, ru = recurrent_unit_groups(H, F, E)
        rc = 4 + pad4(H)
        out = np.zeros((P, self.param_count), np.float32)
        unit = out[:, :H * ru].reshape(P, H, ru)
        for name, o, n in groups:
            unit[:, :, o:o + n] = getattr(self, name).reshape(P, H, n)
        choice = out[:, H * ru:].reshape(P, A, rc)
        choice[:, :, 0] = self.bo
        choice[:, :, 4:4 + H] = self.wo
        return out

    @classmethod
    def unpack(cls, packed, hidden, floors, elevators, scale=None):
        """The inverse of `pack`."""
        packed = f32_array("packed", packed, 2)
        H, F, E = _check_sizes(hidden, floors, elevators)
        P, A = packed.shape[0], 2 * F + 2
        if packed.shape[1] != recurrent_param_count(H, F, E):
            raise ValueError("packed has shape %s, hidden=%d floors=%d elevators=%d need [P, %d]"
                             % (packed.shape, H, F, E, recurrent_param_count(H, F, E)))
        groups, ru = recurrent_unit_groups(H, F, E)
        rc = 4 + pad4(H)
        unit = packed[:, :H * ru].reshape(P, H, ru)
        choice = packed[:, H * ru:].reshape(P, A, rc)
        g = {name: unit[:, :, o:o + n].copy() for name, o, n in groups}
        return cls(g["ws"], g["we"], g["wt"], g["wr"], g["wu"], g["wd"], g["wc"], g["wq"][:, :, 0].copy(), g["wh"],
                   g["b"][:, :, 0].copy(), choice[:, :, 4:4 + H].copy(), choice[:, :, 0].copy(), scale)

    def _gather(self, ids):
        key = ids.tobytes()
        if self._gathered is None or self._gathered[0] != key:
            self._gathered = (key, tuple(getattr(self, name)[ids] for name in self.NAMES))
        return self._gathered[1]

    def reference(self, policy_ids, obs, state, return_choices=False):
        """One step of the definition in numpy float32, vectorised over envs, elevators and units. policy_ids [n]; obs: the
        arrays of `env.observation()` for n buildings; state: their `LiftPolicyState` (torch or numpy; not modified).
        Returns the int32 [n, 2E] actions, ready for `env.step`, and the new numpy carry: h and prev_choice are this
        step's, prev_reward is still the old one, since it comes from the env step that follows
        (`LiftPolicyState.observed`). With `return_choices` also the int32 [n, E] choices, as a third value."""
        ids = to_numpy(policy_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("policy_ids must be a vector of integers")
        n = ids.shape[0]
        if n and (int(ids.min()) < 0 or int(ids.max()) >= self.num_policies):
            raise ValueError("policy_ids must be in [0, %d)" % self.num_policies)
        ids = ids.astype(np.int64)
        if not isinstance(state, LiftPolicyState):
            raise TypeError("state must be a LiftPolicyState, got %s" % type(state).__name__)
        E, H, A = self.elevators, self.hidden, self.choices
        st = state.numpy()
        if st.h.shape != (n, E, H) or st.prev_choice.shape != (n, E) or st.prev_reward.shape != (n,):
            raise ValueError("state must hold h [%d, %d, %d], prev_choice [%d, %d] and prev_reward [%d]" % (n, E, H, n, E, n))
        if n and (int(st.prev_choice.min()) < -1 or int(st.prev_choice.max()) >= A):
            raise ValueError("state.prev_choice must be in [-1, %d)" % A)
        x, d, reserved, up, down = self.inputs(obs)
        if x.shape[0] != n:
            raise ValueError("policy_ids holds %d ids, the observation %d buildings" % (n, x.shape[0]))
        z = self.preactivations(ids, x, d, reserved, up, down)
        wo, bo, wc, wq, wh = self._gather(ids)[7:]
        one = np.float32(1.0)
        pc, pr, h = st.prev_choice.astype(np.int64), st.prev_reward, st.h
        with np.errstate(all="ignore"):
            chosen = pc >= 0
            looked = wc.transpose(0, 2, 1)[np.arange(n)[:, None], np.where(chosen, pc, 0)]       # [n, E, H]
            z = np.where(chosen[:, :, None], z + looked, z)
            z = z + wq[:, None, :] * pr[:, None, None]
            for i in range(H):
                z = z + wh[:, None, :, i] * h[:, :, i:i + 1]
            hn = np.where(z > one, one, np.where(z < -one, -one, z))
            logits = np.broadcast_to(bo[:, None, :], (n, E, A)).copy()
            for j in range(H):
                logits = logits + wo[:, None, :, j] * hn[:, :, j:j + 1]
            choice = np.zeros((n, E), np.int32)
            best = logits[:, :, 0].copy()
            for c in range(1, A):
                better = logits[:, :, c] > best
                choice = np.where(better, np.int32(c), choice)
                best = np.where(better, logits[:, :, c], best)
        assert z.dtype == np.float32 and hn.dtype == np.float32 and logits.dtype == np.float32
        actions = self.actions_of(choice, self.floors).reshape(n, 2 * E)
        new = LiftPolicyState(np.ascontiguousarray(hn), choice.astype(np.int32), st.prev_reward.copy())
        return (actions, new, choice) if return_choices else (actions, new)
