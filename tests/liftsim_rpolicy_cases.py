"""Fixtures shared by tests/test_liftsim_rpolicy.py (CPU) and tests/test_liftsim_rpolicy_gpu.py: the recurrent policy sets, a
scalar restatement of the recurrent dispatcher written straight from the definition in include/metagym_hip.h, and the closed
loop on the oracle (tests/liftsim_oracle.Env stepped with LiftRecurrentPolicy.reference and LiftPolicyState.observed). Runs
are cached, so the tests of one session share them. Nothing here touches the kernel under test."""
import collections
import functools

import numpy as np

import liftsim_cases as LC
import liftsim_oracle as O
import liftsim_policy_cases as PC

N_POLICIES = PC.N_POLICIES
NAMES = ("ws", "we", "wt", "wr", "wu", "wd", "wc", "wq", "wh", "b", "wo", "bo")      # the constructor's order


def random_weights(rs, P, H, F, E, sigma):
    A = 2 * F + 2
    shapes = dict(ws=(P, H, 8), we=(P, H, E), wt=(P, H, F + 1), wr=(P, H, F), wu=(P, H, F), wd=(P, H, F), wc=(P, H, A),
                  wq=(P, H), wh=(P, H, H), b=(P, H), wo=(P, A, H), bo=(P, A))
    return {name: (rs.randn(*shapes[name]) * sigma).astype(np.float32) for name in NAMES}


@functools.lru_cache(maxsize=None)
def policies(F, E, H, seed=5, sigma=0.5, memory=True):
    """Six recurrent policies with N(0, sigma^2) float32 weights; policy q prefers one edge choice (+3 on its bo, the bumps
    of liftsim_policy_cases.policies). memory=False: the same set with wc, wq and wh zeroed."""
    from metagym_amd.liftsim import LiftRecurrentPolicy
    w = random_weights(np.random.RandomState(seed), N_POLICIES, H, F, E, sigma)
    for q, c in enumerate(PC.edge_choices(F)):
        w["bo"][q, c] += np.float32(3.0)
    if not memory:
        for name in ("wc", "wq", "wh"):
            w[name][:] = 0.0
    return LiftRecurrentPolicy(**w)


def scalar_policy(pol, q, state, el, h, pc, pr):
    """Policy q of `pol` for elevator `el` of one MansionState with the memory h (H float32), the previous choice pc and the
    previous reward pr, straight from the definition: Python loops, one np.float32 operation at a time. Returns the choice
    and the new memory as a list of np.float32."""
    f32 = np.float32
    F, H, A = pol.floors, pol.hidden, pol.choices
    es = state.ElevatorStates[el]
    raw = [es.Floor, es.Velocity, es.Direction, es.DoorState, es.LoadWeight, es.OverloadedAlarm,
           1 if es.DoorIsOpening else 0, 1 if es.DoorIsClosing else 0]
    pr = f32(pr)
    with np.errstate(all="ignore"):
        x = [f32(np.float64(raw[i])) * pol.scale[i] for i in range(8)]
        hn = []
        for j in range(H):
            z = pol.b[q, j]
            for i in range(8):
                z = f32(z + f32(pol.ws[q, j, i] * x[i]))
            z = f32(z + pol.we[q, j, el])
            d = int(es.CurrentDispatchTarget)
            if 0 <= d <= F:
                z = f32(z + pol.wt[q, j, d])
            for f in range(1, F + 1):
                if f in es.ReservedTargetFloors:
                    z = f32(z + pol.wr[q, j, f - 1])
            for f in range(1, F + 1):
                if f in state.RequiringUpwardFloors:
                    z = f32(z + pol.wu[q, j, f - 1])
            for f in range(1, F + 1):
                if f in state.RequiringDownwardFloors:
                    z = f32(z + pol.wd[q, j, f - 1])
            if pc >= 0:
                z = f32(z + pol.wc[q, j, pc])
            z = f32(z + f32(pol.wq[q, j] * pr))
            for i in range(H):
                z = f32(z + f32(pol.wh[q, j, i] * f32(h[i])))
            assert isinstance(z, np.float32)
            hn.append(f32(1.0) if z > 1 else (f32(-1.0) if z < -1 else z))
        logits = []
        for c in range(A):
            v = pol.bo[q, c]
            for j in range(H):
                v = f32(v + f32(pol.wo[q, c, j] * hn[j]))
            logits.append(v)
        choice = 0
        for c in range(1, A):
            if logits[c] > logits[choice]:
                choice = c
    return choice, hn


def scalar_step(pol, ids, states, carry):
    """The scalar restatement for n buildings: ([n][2E] actions with the choice-to-action table spelt out, [n][E] choices,
    float32 [n, E, H] new memories)."""
    F, E = pol.floors, pol.elevators
    actions, choices, h = [], [], np.zeros((len(states), E, pol.hidden), np.float32)
    for i, (q, st) in enumerate(zip(ids, states)):
        row, crow = [], []
        for el in range(E):
            c, hn = scalar_policy(pol, int(q), st, el, carry.h[i, el], int(carry.prev_choice[i, el]), carry.prev_reward[i])
            h[i, el] = hn
            crow.append(c)
            row += [c + 1, 1] if c < F else [c - F + 1, -1] if c < 2 * F else [0, 1] if c == 2 * F else [-1, 1]
        actions.append(row)
        choices.append(crow)
    return actions, choices, h


# ---------------------------------------------------------------------------------------------- the closed loop on the oracle
# name -> what LiftSim takes, N, seed, the sampled envs, steps, H, and (seed, sigma) of the policy set, chosen on the CPU so
# that test_liftsim_rpolicy.py's conditions (a)-(d) hold. Sampled env sample[i] plays policy i % 6.
def _case(kw, N, seed, sample, steps, H, pseed, sigma, flow=None):
    return dict(kw=kw, N=N, seed=seed, sample=tuple(sample), steps=steps, H=H, pseed=pseed, sigma=sigma, flow=flow)


CASES = {
    "f2_n1": lambda: _case(dict(generator="UNIFORM", **PC.CONF[1]), 1, 11, (0,), 200, 1, 442, 4.0),
    "f2_n65": lambda: _case(dict(generator="UNIFORM", **PC.CONF[1]), 65, 11, (0, 1, 31, 62, 63, 64), 200, 1, 442, 4.0),
    "uniform3": lambda: _case(dict(generator="UNIFORM", **PC.CONF[3]), 130, 40, (0, 1, 63, 64, 127, 128, 129), 150, 7, 5, 0.5),
    "custom_rush": lambda: _case(dict(generator="CUSTOM"), 70, 21, (0, 1, 33, 63, 64, 69), 120, 64, 5, 0.25,
                                 flow=PC.rush_flow()),
    "big": lambda: _case(dict(generator="UNIFORM", floors=128, elevators=32, **LC.BIG_KW), LC.BIG_N, LC.BIG_SEED, LC.BIG_SAMPLE,
                         100, 4, 5, 0.5),
}
case_ids = PC.case_ids
oracle_config = PC.oracle_config


def case_policies(case, memory=True):
    cfg = oracle_config(case)
    return policies(cfg.F, cfg.E, case["H"], case["pseed"], case["sigma"], memory)


def run_closed_loop(case, pol, ids, steps=None, until_differs_from=None):
    """The sampled envs of `case` in the oracle under `pol` from a fresh carry; ids[i] is the policy of case["sample"][i].
    Per step the actions and outputs, at the end the states, both streams and the carry, and what the run covered.
    `until_differs_from` ([T, S, 2E] actions): stop at the first step whose actions differ and report it as "differs"."""
    from metagym_amd.liftsim import LiftPolicyState
    cfg = oracle_config(case)
    F, E, S = cfg.F, cfg.E, len(case["sample"])
    T = case["steps"] if steps is None else steps
    envs = [O.Env(cfg, case["seed"] + e) for e in case["sample"]]
    carry = LiftPolicyState.zeros(S, E, pol.hidden)
    out = dict(case=case, policy=pol, ids=ids, actions=np.zeros((T, S, 2 * E), np.int32), rows=np.zeros((T, S, 4)),
               choices=collections.Counter(), h_hi=0, h_lo=0, h_inside=0, differs=-1)
    for k in range(T):
        states = [env.mansion_state() for env in envs]
        a, carry, c = pol.reference(ids, PC.obs_of(states, F, E), carry, return_choices=True)
        out["choices"].update(c.ravel().tolist())
        out["h_hi"] += int((carry.h == 1).sum())
        out["h_lo"] += int((carry.h == -1).sum())
        out["h_inside"] += int((np.abs(carry.h) < 1).sum())
        out["actions"][k] = a
        if until_differs_from is not None and a.tolist() != until_differs_from[k].tolist():
            out["differs"] = k
            break
        for j, env in enumerate(envs):
            out["rows"][k, j] = LC.row(*env.step([int(v) for v in a[j]]))
        carry = carry.observed(out["rows"][k, :, 0])
    out["states"] = [env.mansion_state() for env in envs]
    out["streams"] = [LC.streams(env) for env in envs]
    out["carry"] = carry
    out["max_queue"] = max(env.max_queue for env in envs)
    return out


@functools.lru_cache(maxsize=None)
def closed_loop(name):
    case = CASES[name]()
    return run_closed_loop(case, case_policies(case), case_ids(case)[list(case["sample"])])


@functools.lru_cache(maxsize=None)
def memory_decides(name):
    """The first step at which the memoryless twin of a case's policy set (wc, wq, wh zeroed) acts differently from the
    set itself on the run of `closed_loop` (-1: never)."""
    run = closed_loop(name)
    case = run["case"]
    twin = run_closed_loop(case, case_policies(case, memory=False), run["ids"], until_differs_from=run["actions"])
    return twin["differs"]


# ---------------------------------------------------------------------------------------------- a queue that overflows
# liftsim_policy_cases.FROZEN's inputs (queue_capacity 33, seed 5, 64 envs of CONF[3]) under recurrent policies: env e plays
# policy e % 6.
FROZEN = dict(PC.FROZEN, H=8, pseed=5, sigma=0.5)


@functools.lru_cache(maxsize=None)
def frozen_run():
    """The sampled envs of FROZEN in the oracle (whose queues are unbounded): per step the actions and outputs, and per env the
    step in which its longest queue first passes Q, which is the step in which it overflows on the device (-1: none)."""
    from metagym_amd.liftsim import LiftPolicyState
    c = FROZEN
    cfg = O.Config(**c["kw"])
    F, E, T, S = cfg.F, cfg.E, c["steps"], len(c["sample"])
    pol = policies(F, E, c["H"], c["pseed"], c["sigma"])
    ids = np.array(c["sample"]) % N_POLICIES
    envs = [O.Env(cfg, c["seed"] + e) for e in c["sample"]]
    carry = LiftPolicyState.zeros(S, E, pol.hidden)
    out = dict(policy=pol, actions=np.zeros((T, S, 2 * E), np.int32), rows=np.zeros((T, S, 4)), first=[-1] * S)
    for k in range(T):
        a, carry = pol.reference(ids, PC.obs_of([env.mansion_state() for env in envs], F, E), carry)
        out["actions"][k] = a
        for j, env in enumerate(envs):
            out["rows"][k, j] = LC.row(*env.step([int(v) for v in a[j]]))
            if out["first"][j] < 0 and env.max_queue > c["Q"]:
                out["first"][j] = k
        carry = carry.observed(out["rows"][k, :, 0])
    return out
