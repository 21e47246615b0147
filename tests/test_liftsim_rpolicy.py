"""LiftSim recurrent dispatchers on the CPU: LiftRecurrentPolicy.reference against a scalar restatement written straight from
the definition, the packed layout, the carry class, the closed loop on the oracle with its coverage, the host-side refusals
of mg_liftsim_rpolicy_rollout, and what the new translation unit emits. All comparisons are exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import liftsim_oracle as O
import liftsim_policy_cases as PC
import liftsim_rpolicy_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from metagym_amd import _lib
    return _lib, _lib.load()


def _elevator(F, d):
    """An idle car at floor 1 with CurrentDispatchTarget d."""
    return O.ElevatorState(Floor=1.0, MaximumFloor=F, Velocity=0.0, MaximumSpeed=2.0, Direction=0, DoorState=0.0,
                           CurrentDispatchTarget=d, DispatchTargetDirection=1, LoadWeight=0.0, MaximumLoad=1600,
                           ReservedTargetFloors=[], OverloadedAlarm=0.0, DoorIsOpening=False, DoorIsClosing=False)


def _oracle_states(cfg, seed, steps, every, rs):
    """States of an oracle run under random held actions, one every `every` steps."""
    env, out = O.Env(cfg, seed), []
    a = [0, 1] * cfg.E
    for k in range(steps):
        if k % 6 == 0:
            a = []
            for _ in range(cfg.E):
                a += [int(rs.randint(-1, cfg.F + 1)), int(rs.randint(-1, 2))]
        env.step(a)
        if k % every == every - 1:
            out.append(env.mansion_state())
    return out


# ---------------------------------------------------------------------------------------------- 1. reference against the scalar form
@pytest.mark.parametrize("conf", [1, 3])
@pytest.mark.parametrize("H", [1, 3, 4, 5, 64])
def test_reference_matches_the_scalar_restatement_on_oracle_states(conf, H):
    from metagym_amd.liftsim import LiftPolicyState
    kw = PC.CONF[conf]
    F, E = kw["floors"], kw["elevators"]
    pol = RC.policies(F, E, H)
    rs = np.random.RandomState(10 * conf + H)
    steps = 600 if conf == 1 else 240
    states = _oracle_states(O.Config(generator="UNIFORM", **kw), 3, steps, steps // 12, rs)
    n = len(states)
    assert any(st.RequiringUpwardFloors for st in states) and any(st.RequiringDownwardFloors for st in states)
    ids = np.arange(n) % RC.N_POLICIES
    # a carry with every kind of entry: memories at both bounds, inside them, -0; previous choices none, first, last
    carry = LiftPolicyState.zeros(n, E, H)
    carry.h[:] = rs.uniform(-1, 1, (n, E, H)).astype(np.float32)
    carry.h[0::4] = np.float32(1.0)
    carry.h[1::4, :, 0] = np.float32(-1.0)
    carry.h[2::4, :, -1] = np.float32(-0.0)
    carry.prev_choice[:] = rs.randint(-1, 2 * F + 2, (n, E))
    carry.prev_choice[0, 0], carry.prev_choice[-1, -1] = 2 * F + 1, 0
    carry.prev_reward[:] = (-rs.rand(n) * 1e-2).astype(np.float32)
    before = (carry.h.copy(), carry.prev_choice.copy(), carry.prev_reward.copy())
    for _ in range(2):                                               # a second step on the first one's carry
        obs = PC.obs_of(states, F, E)
        got, new, choices = pol.reference(ids, obs, carry, return_choices=True)
        two = pol.reference(ids, obs, carry)
        assert len(two) == 2 and two[0].tolist() == got.tolist()
        assert got.dtype == np.int32 and got.shape == (n, 2 * E) and choices.shape == (n, E)
        assert new.h.dtype == np.float32 and new.h.shape == (n, E, H) and new.prev_choice.dtype == np.int32
        want_a, want_c, want_h = RC.scalar_step(pol, ids, states, carry)
        assert got.tolist() == want_a and choices.tolist() == want_c
        assert new.h.tobytes() == want_h.tobytes()
        assert new.prev_choice.tolist() == want_c
        assert new.prev_reward.tobytes() == carry.prev_reward.tobytes()      # the reward comes from the env step
        assert got.tolist() == pol.actions_of(choices, F).reshape(n, 2 * E).tolist()
        carry = new.observed(-np.arange(n) * 1e-4)
        assert carry.prev_reward.tobytes() == (-np.arange(n) * 1e-4).astype(np.float32).tobytes()
        assert carry.h.tobytes() == new.h.tobytes() and carry.prev_choice.tolist() == want_c
    assert before[0].tobytes() != carry.h.tobytes()


def test_a_memoryless_recurrent_policy_has_the_mlp_preactivations_and_clamps_them():
    """wc = wq = wh = 0 and a fresh carry: z is LiftPolicy's z (+ 0 * pr, which keeps a non-zero z), clamped instead of
    rectified."""
    from metagym_amd.liftsim import LiftPolicy, LiftPolicyState
    F, E, H = 10, 4, 5
    pol = RC.policies(F, E, H, memory=False)
    mlp = LiftPolicy(pol.ws, pol.we, pol.wt, pol.wr, pol.wu, pol.wd, pol.b, pol.wo, pol.bo)
    states = _oracle_states(O.Config(generator="UNIFORM", **PC.CONF[3]), 3, 120, 10, np.random.RandomState(1))
    ids = np.arange(len(states)) % RC.N_POLICIES
    obs = PC.obs_of(states, F, E)
    z = mlp.preactivations(ids.astype(np.int64), *mlp.inputs(obs))
    _, new = pol.reference(ids, obs, LiftPolicyState.zeros(len(states), E, H))
    assert (z != 0).all() and new.h.tobytes() == np.clip(z, np.float32(-1), np.float32(1)).tobytes()


def test_a_negative_zero_preactivation_stays_negative_zero_and_padding_is_not_added():
    """b = -0, every dense weight -0 and no lookup that applies: z stays -0 through wc (pc = -1: no add), wq * pr
    (-0 * 0 = -0) and wh * h (-0 * +h = -0); a lookup with pc >= 0 is exactly one add."""
    from metagym_amd.liftsim import LiftPolicyState, LiftRecurrentPolicy
    F, E, H = 4, 2, 3
    w = RC.random_weights(np.random.RandomState(3), 1, H, F, E, 0.5)
    for name in ("b", "ws", "we", "wq", "wh"):
        w[name][:] = np.float32(-0.0)
    pol = LiftRecurrentPolicy(**w)
    st = O.MansionState([_elevator(F, -1), _elevator(F, F + 1)], [], [])
    carry = LiftPolicyState.zeros(1, E, H)
    carry.h[:] = np.float32(0.5)
    _, new = pol.reference(np.array([0]), PC.obs_of([st], F, E), carry)
    assert (new.h == 0).all() and np.signbit(new.h).all()
    assert RC.scalar_step(pol, [0], [st], carry)[2].tobytes() == new.h.tobytes()
    carry.prev_choice[0] = [0, 2 * F + 1]
    _, new = pol.reference(np.array([0]), PC.obs_of([st], F, E), carry)
    want = np.clip(np.stack([pol.wc[0, :, 0], pol.wc[0, :, 2 * F + 1]]), np.float32(-1), np.float32(1))
    assert new.h[0].tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------- 2. the packed layout
@pytest.mark.parametrize("F,E,H", [(2, 1, 1), (10, 4, 7), (33, 5, 3), (128, 32, 64), (127, 31, 5), (7, 3, 4), (9, 3, 63)])
def test_pack_round_trip_count_and_zero_padding(F, E, H):
    from metagym_amd.liftsim import LiftRecurrentPolicy
    from metagym_amd.liftsim import policy as LP
    _, lib = _lib()
    pol = LiftRecurrentPolicy(**RC.random_weights(np.random.RandomState(1), 3, H, F, E, 0.5))
    count = lib.mg_liftsim_rpolicy_param_count(H, F, E)
    assert count == pol.param_count == LP.recurrent_param_count(H, F, E) and count % 4 == 0
    packed = pol.pack()
    assert packed.shape == (3, count) and packed.dtype == np.float32
    back = LiftRecurrentPolicy.unpack(packed, H, F, E)
    for name in RC.NAMES + ("scale",):
        assert getattr(back, name).tobytes() == getattr(pol, name).tobytes(), name
    # the layout as the header spells it, restated here: every record and group on a multiple of four floats
    p4 = lambda n: (n + 3) & ~3
    A = 2 * F + 2
    ru = 12 + p4(E) + p4(F + 1) + 3 * p4(F) + p4(A) + p4(H)
    rc = 4 + p4(H)
    assert count == H * ru + A * rc
    used = np.zeros(count, bool)
    want = np.zeros((3, count), np.float32)
    for j in range(H):
        o = j * ru
        want[:, o], want[:, o + 1] = pol.b[:, j], pol.wq[:, j]
        used[o:o + 2] = True
        o += 4
        for name, n in (("ws", 8), ("we", E), ("wt", F + 1), ("wr", F), ("wu", F), ("wd", F), ("wc", A), ("wh", H)):
            assert o % 4 == 0
            want[:, o:o + n] = getattr(pol, name)[:, j]
            used[o:o + n] = True
            o += p4(n)
        assert o == (j + 1) * ru
    for c in range(A):
        o = H * ru + c * rc
        want[:, o], want[:, o + 4:o + 4 + H] = pol.bo[:, c], pol.wo[:, c]
        used[o] = True
        used[o + 4:o + 4 + H] = True
    assert packed.tobytes() == want.tobytes()
    assert not packed[:, ~used].any()                                    # every padding float is zero
    ones = LiftRecurrentPolicy(**{name: np.ones_like(getattr(pol, name)) for name in RC.NAMES}).pack()
    assert (ones[:, used] == 1).all() and not ones[:, ~used].any()


def test_param_count_of_the_largest_policy_and_its_refusals():
    _, lib = _lib()
    assert lib.mg_liftsim_rpolicy_param_count(64, 128, 32) == 74120
    for args in ((0, 10, 4), (65, 10, 4), (8, 1, 4), (8, 129, 4), (8, 10, 0), (8, 10, 33)):
        assert lib.mg_liftsim_rpolicy_param_count(*args) == -1002, args


def test_recurrent_policy_refuses_bad_parameters():
    from metagym_amd.liftsim import LiftPolicyState, LiftRecurrentPolicy
    F, E, H = 5, 2, 3
    good = RC.random_weights(np.random.RandomState(0), 2, H, F, E, 0.5)
    pol = LiftRecurrentPolicy(**good)
    for name in ("wc", "wq", "wh"):
        w = dict(good)
        w[name] = good[name].copy()
        w[name].flat[1] = np.inf
        with pytest.raises(ValueError):
            LiftRecurrentPolicy(**w)
        w[name] = good[name].astype(np.float64)
        with pytest.raises(TypeError):
            LiftRecurrentPolicy(**w)
        w[name] = np.delete(good[name], 0, axis=-1)
        with pytest.raises(ValueError):
            LiftRecurrentPolicy(**w)
    st = O.MansionState([_elevator(F, 0)] * E, [], [])
    obs = PC.obs_of([st], F, E)
    with pytest.raises(TypeError):
        pol.reference(np.array([0]), obs, None)
    with pytest.raises(ValueError):
        pol.reference(np.array([0]), obs, LiftPolicyState.zeros(1, E, H + 1))
    with pytest.raises(ValueError):
        pol.reference(np.array([0]), obs, LiftPolicyState.zeros(2, E, H))
    with pytest.raises(ValueError):
        pol.reference(np.array([2]), obs, LiftPolicyState.zeros(1, E, H))
    bad = LiftPolicyState.zeros(1, E, H)
    bad.prev_choice[0, 0] = 2 * F + 2
    with pytest.raises(ValueError):
        pol.reference(np.array([0]), obs, bad)


# ---------------------------------------------------------------------------------------------- 3. the carry
def test_the_numpy_carry():
    from metagym_amd.liftsim import LiftPolicyState
    s = LiftPolicyState.zeros(5, 3, 7)
    assert s.h.shape == (5, 3, 7) and s.h.dtype == np.float32 and not s.h.any()
    assert s.prev_choice.shape == (5, 3) and s.prev_choice.dtype == np.int32 and (s.prev_choice == -1).all()
    assert s.prev_reward.shape == (5,) and s.prev_reward.dtype == np.float32 and not s.prev_reward.any()
    assert (s.num_envs, s.elevators, s.hidden, s.device) == (5, 3, 7, None)
    c = s.clone()
    c.h[:] = 1
    c.prev_choice[:] = 2
    assert not s.h.any() and (s.prev_choice == -1).all()
    o = c.observed(np.arange(5) * 0.1)
    assert o.prev_reward.tobytes() == (np.arange(5) * 0.1).astype(np.float32).tobytes() and not c.prev_reward.any()
    n = o.numpy()
    assert all(getattr(n, k).flags["C_CONTIGUOUS"] for k in ("h", "prev_choice", "prev_reward"))
    with pytest.raises(ValueError):
        c.observed(np.zeros(4))
    for args in ((0, 3, 7), (5, 0, 7), (5, 33, 7), (5, 3, 0), (5, 3, 65)):
        with pytest.raises(ValueError):
            LiftPolicyState.zeros(*args)
    assert "step()" in LiftPolicyState.__doc__ and "rollout(actions)" in LiftPolicyState.__doc__


# ---------------------------------------------------------------------------------------------- 4. the definition, said twice
def _definition_block(text, strip):
    lines = [re.sub(strip, "", line).rstrip() for line in text.splitlines()]
    starts = [i for i, line in enumerate(lines) if "(raw as for mg_liftsim_policy)" in line]
    assert len(starts) == 1
    end = next(i for i in range(starts[0], len(lines)) if lines[i].strip() == "pc[el] = choice")
    block = lines[starts[0]:end + 1]
    indent = len(block[0]) - len(block[0].lstrip())
    return [line[indent:] for line in block]


def test_the_header_and_the_module_docstring_define_the_same_policy():
    from metagym_amd.liftsim import policy as LP
    header = open(os.path.join(ROOT, "include", "metagym_hip.h")).read()
    a = _definition_block(header, r"^ \*")
    b = _definition_block(LP.__doc__, r"^$")
    assert a == b and len(a) == 17
    assert a[9:13] == ["    if pc[el] >= 0:  z = z + wc[j][pc[el]]", "    z = z + wq[j] * pr",
                       "    for i in 0..H-1:  z = z + wh[j][i] * h[el][i]", "    hn[j] = z > 1 ? 1 : (z < -1 ? -1 : z)"]


# ---------------------------------------------------------------------------------------------- 5. the closed loop and its coverage
@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_closed_loop_cases_use_their_memory_and_cover_the_choices(name):
    run = RC.closed_loop(name)
    case, F = run["case"], run["policy"].floors
    # (a) memory decides something
    assert 0 <= RC.memory_decides(name) < case["steps"]
    # (b) the memories reach both bounds and lie strictly inside them too
    assert run["h_hi"] > 0 and run["h_lo"] > 0 and run["h_inside"] > 0
    # (c) no queue passes the env's default queue_capacity: nothing freezes on the device
    assert 0 < run["max_queue"] <= 128
    # (d) every choice class
    ch = run["choices"]
    assert sum(v for c, v in ch.items() if c < F) > 0 and sum(v for c, v in ch.items() if F <= c < 2 * F) > 0
    assert ch[2 * F] > 0 and ch[2 * F + 1] > 0
    assert min(ch) >= 0 and max(ch) <= 2 * F + 1
    assert (run["rows"][:, :, 0] < 0).all()
    assert sorted(set(run["ids"].tolist())) == list(range(min(len(case["sample"]), 6)))
    assert run["carry"].prev_reward.tobytes() == run["rows"][-1, :, 0].astype(np.float32).tobytes()


def test_the_frozen_case_overflows_its_queues_under_the_recurrent_policies():
    run = RC.frozen_run()
    first = dict(zip(RC.FROZEN["sample"], run["first"]))
    assert sum(1 for v in first.values() if 0 < v < RC.FROZEN["steps"] - 1) >= 2, first
    assert sum(1 for v in first.values() if v == -1) >= 2, first


# ---------------------------------------------------------------------------------------------- 6. refusals that need no device
def test_rpolicy_rollout_refuses_on_the_host():
    L, lib = _lib()
    cfg = L.LiftsimConfig()
    cfg.floors, cfg.elevators, cfg.generator, cfg.queue_capacity, cfg.window = 10, 4, 1, 128, 1200
    cfg.particle_number, cfg.floor_height, cfg.dt, cfg.generation_interval = 12, 4.0, 0.5, 150.0
    fake = C.create_string_buffer(256)
    base = (C.addressof(fake) + 15) & ~15
    p = C.c_void_p(base)

    def desc(**kw):
        d = L.LiftsimRPolicyDesc(base, 2, 8, 10, 4, (C.c_float * 8)(*([1.0] * 8)))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def carry(**kw):
        s = L.LiftsimPolicyState(base, base + 16, base + 32)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(cfg=cfg, n=4, arena=p, steps=5, pol=None, ids=p, st=None, ret=p):
        return lib.mg_liftsim_rpolicy_rollout(cfg, n, arena, steps, desc() if pol is None else pol, ids,
                                              carry() if st is None else st, ret, None, None, None, None, None, None)

    NULL, SIZE, CONFIG = -1001, -1002, -1003
    assert call(cfg=None) == NULL and call(arena=None) == NULL and call(ids=None) == NULL and call(ret=None) == NULL
    assert lib.mg_liftsim_rpolicy_rollout(cfg, 4, p, 5, None, p, carry(), p, None, None, None, None, None, None) == NULL
    assert lib.mg_liftsim_rpolicy_rollout(cfg, 4, p, 5, desc(), p, None, p, None, None, None, None, None, None) == NULL
    assert call(pol=desc(params=None)) == NULL and b"params" in lib.mg_last_error()
    for field in ("h", "prev_choice", "prev_reward"):
        assert call(st=carry(**{field: None})) == NULL and b"mg_liftsim_policy_state" in lib.mg_last_error(), field
        assert call(st=carry(**{field: base + 2})) == CONFIG and b"4-byte" in lib.mg_last_error(), field
    assert call(steps=0) == SIZE and b"n_steps" in lib.mg_last_error()
    assert call(n=0) == SIZE
    assert call(pol=desc(n_policies=0)) == SIZE
    assert call(pol=desc(hidden=0)) == SIZE and call(pol=desc(hidden=65)) == SIZE and b"hidden" in lib.mg_last_error()
    assert call(pol=desc(floors=11)) == CONFIG and b"floors" in lib.mg_last_error()
    assert call(pol=desc(elevators=3)) == CONFIG
    assert call(pol=desc(params=base + 4)) == CONFIG and b"16-byte" in lib.mg_last_error()
    bad = L.LiftsimConfig.from_buffer_copy(cfg)
    bad.queue_capacity = 0                             # what mg_liftsim_step refuses in cfg
    assert call(cfg=bad) == CONFIG and b"queue_capacity" in lib.mg_last_error()
    bad = L.LiftsimConfig.from_buffer_copy(cfg)
    bad.generator, bad.table_len = 0, 3                # CUSTOM without its tables
    assert call(cfg=bad) == CONFIG


# ---------------------------------------------------------------------------------------------- 7. the translation unit
def _kernels(tmp_path, src):
    """Demangled-prefix names of the kernels in the device assembly of one unit, compiled with build.py's own flags."""
    from metagym_amd import build as hip_build
    out = tmp_path / (src + ".s")
    cmd = [hip_build.HIPCC] + hip_build.COMPILE_FLAGS + hip_build.FILE_FLAGS.get(src, []) + \
          ["--cuda-device-only", "-S", os.path.join(hip_build.CSRC, src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    symbols = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", out.read_text(), re.M)
    names = []
    for s in symbols:
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", s)
        assert m, s
        names.append(s[m.end():m.end() + int(m.group(1))])
    return sorted(names)


def test_liftsim_rpolicy_emits_its_own_kernel_only(tmp_path):
    assert _kernels(tmp_path, "liftsim_rpolicy.hip") == ["liftsim_rpolicy_rollout_kernel"]
    from metagym_amd import build as hip_build
    assert "liftsim_rpolicy.hip" not in hip_build.FILE_FLAGS             # the default flags: -ffp-contract=off among them
    assert "-ffp-contract=off" in hip_build.COMPILE_FLAGS
