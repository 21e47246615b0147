"""LiftSim's edge cases without a GPU: the oracle alone reaches every edge that tests/test_liftsim_edges_gpu.py holds the
kernels to (tests/liftsim_cases.py has the cases), the oracle and the host tables reproduce the reference's runs at these
edges (tests/golden/liftsim_edges.npz), and the configurations nobody runs are refused."""
import collections
import ctypes as C
import json
import math
import os
import random

import numpy as np
import pytest

import liftsim_cases as LC
import liftsim_oracle as O
import liftsim_rule_oracle as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "liftsim_edges.npz"))


# ---------------------------------------------------------------------------------------------- the instruments
def test_counting_random_draws_like_random_and_counts_every_word():
    plain, counted = random.Random(12), LC.CountingRandom(12)
    for r in (plain, counted):
        r.out = [r.random(), r.randint(1, 128), r.uniform(20, 100), r.normalvariate(50, 10), r.getrandbits(70)]
        order = list(range(32))
        r.shuffle(order)
        r.out.append(order)
    assert plain.out == counted.out and plain.getstate() == counted.getstate()
    s0, s1 = random.Random(12).getstate()[1], counted.getstate()[1]
    assert counted.words == LC.words_between(s0[:624], s0[624], s1[:624], s1[624]) > 40


def test_words_between_counts_across_key_blocks():
    for n in (1, 523, 524, 525, 623, 624, 625, 1247, 1248, 1249, 3000):
        rs = np.random.RandomState(5)
        rs.bytes(4 * 100)
        a = rs.get_state()
        rs.bytes(4 * n)
        b = rs.get_state()
        assert LC.words_between(a[1], a[2], b[1], b[2]) == n


def test_horizon_predicate():
    # a freshly seeded stream (pos 624) may draw one block in its first step; one at pos 1 may draw 1247 words
    assert random.Random(3).getstate()[1][624] == 624 == np.random.RandomState(3).get_state()[2]
    assert not LC.past_horizon(624, 624) and LC.past_horizon(625, 624)
    assert not LC.past_horizon(1247, 1) and LC.past_horizon(1248, 1)


def test_a_tracked_env_steps_like_a_plain_one():
    cfg = LC.custom_config(8, LC.edge_flow(8))
    plain, tr = O.Env(cfg, 4), LC.Tracked(cfg, 4, Q=64)
    acts = O.scripted_actions(4, 60, 8, 3)
    for k in range(60):
        a = [int(x) for x in acts[k]]
        py0 = plain.py.getstate()[1]
        assert plain.step(a) == tr.step(a)
        py1 = plain.py.getstate()[1]
        assert tr.py_words == LC.words_between(py0[:624], py0[624], py1[:624], py1[624]) and tr.py_pos == py0[624]
        assert tr.np_words > 0
    assert plain.mansion_state() == tr.env.mansion_state() and plain.py.getstate() == tr.env.py.getstate()
    assert [len(q) for q in plain.up + plain.down] == [len(q) for q in tr.env.up + tr.env.down]


# ---------------------------------------------------------------------------------------------- the big buildings
@pytest.mark.parametrize("F,E", list(LC.BIG))
def test_big_buildings_reach_floor_f_and_fill_the_fifo(F, E):
    rule, rand = LC.big_rule_run(F, E), LC.big_random_run(F, E)
    assert rule["crossed"] == 0 and rand["crossed"] == 0          # no step of a sampled env is past the stream horizon
    for run in (rule, rand):
        ev = run["ev"]
        assert ev["top_reserved"] > 0                              # bit F - 1 of a clicked set, slot F of a target list
        assert ev["call_at_top"] > 0 and ev["call_at_1"] > 0       # the first and the last bit of the hall-call sets
    # a car stands at floor F in every config: under the dispatcher wherever there are cars enough to get there (at 10
    # arrivals a step the two cars of (32, 2) never leave the lower floors, in 150 steps or in 400), and under the
    # scripted car of the random run where its 120 steps reach it (F <= 33)
    assert rule["ev"]["at_top"] + rand["ev"]["at_top"] > 0
    if E >= 5:
        assert rule["ev"]["at_top"] > 0
    if F <= 33:
        assert rand["ev"]["at_top"] > 0
    st = rule["stats"]
    assert st["max_line"] == E                                     # the dispatcher's FIFO was full: cnt == RING at E = 32
    assert st["calls_with_displacement"] > 0 and st["displace_up"] > 0 and st["max_taken"] > E
    # an idle car (Direction 0) or one moving down takes a call from another only where cars are idle or come down while
    # calls wait: this saturated traffic keeps the 2 cars of (32, 2) going up and stopping, and the 5 of (33, 5) never
    # displace downwards; 400 steps instead of 150 add no such event to either, so the small configs assert what occurs
    if E >= 5:
        assert st["displace_zero_up"] > 0
    if E >= 17:
        assert st["displace_down"] > 0
    assert rule["max_queue"] < 128                                 # the default queue_capacity holds
    a = rand["actions"]
    assert (a[:, :, 0::2] == -1).any() and (a[:, :, 0::2] == F).any() and (a[:, :, 1::2] == 0).any()
    assert sum(tr.log["boarded"] for tr in rand["envs"]) > 0


def test_big_case_table():
    assert sorted(LC.BIG) == [(32, 2), (33, 5), (64, 17), (65, 32), (128, 32)]
    assert LC.BIG_N == 130 and LC.BIG_SAMPLE == (0, 63, 64, 127, 128, 129)
    assert LC.BIG_KW == dict(dt=1.0, particle_number=40, generation_interval=4.0)


# ---------------------------------------------------------------------------------------------- CUSTOM on synthetic tables
@pytest.mark.parametrize("F", [2, 8, 9, 16])
def test_custom_tables_hold_the_edge_rows(F):
    from metagym_amd.liftsim import custom_tables
    E, dt = LC.CUSTOM[F]
    tb = custom_tables(LC.edge_flow(F), F, dt)
    lam = tb["dens"] * np.float32(dt)
    assert lam.dtype == np.float32 and tb["times"].tolist() == [0.0, LC.ROW1_AT, LC.ROW2_AT]
    assert 9.0 < lam[0].max() < 10.0 and lam[1].max() < 0.1 and lam[2].max() >= 10.0
    flip, pp = tb["flip"][:, :, :F - 1], tb["pp"][:, :, :F - 1]
    assert (flip == 1).any() and ((pp == 0.0) & (flip == 1)).any()       # p > 0.5, and p == 1 exactly
    assert ((pp > 0.0) & (flip == 1)).any() and (pp <= 0.5).all()
    assert (tb["prob"][0].sum(axis=1) == 0.0).any() or F == 2           # an all-zero floor (F = 2: in the quiet row)
    assert (tb["prob"][1].sum(axis=1) == 0.0).any()
    if F > 2:
        assert (lam[0] == 0.0).any()
        assert tb["prob"][0, 2, F - 1] > 0.99 and tb["prob"][0, F - 1, 0] == 1.0 and tb["prob"][0, 4, 4] > 0.99
    if dt == 0.3:
        assert float(np.float32(dt)) != dt                               # the enlam table of an inexact float32 interval
    assert tb["enlam"].tolist() == [[math.exp(-float(x)) for x in r] for r in lam]


@pytest.mark.parametrize("F", [2, 8, 9, 16])
def test_custom_runs_reach_their_edges(F):
    run = LC.custom_run(F)
    assert run["crossed"] == 0                       # no step of any of the 70 envs is past the stream horizon
    assert run["max_count_sampled"] > 16             # a sampled env draws a binomial with n > 16: exp(n log q) on the device
    assert run["log"]["alarm"] > 0 and run["log"]["mid_deque_delete"] > 0
    assert 128 < run["max_queue"] < LC.CUSTOM_Q
    assert run["K2"] == LC.steps_to_row2(LC.CUSTOM[F][1]) and run["K2"] * LC.CUSTOM[F][1] <= LC.ROW2_AT + 1.0
    assert set((63, 64, 69)) <= set(LC.CUSTOM_SAMPLE) and len(LC.CUSTOM_SAMPLE) == 8 and LC.CUSTOM_N == 70
    # persons with src == dst were drawn: generated counts them, no queue ever held them
    tr = run["envs"][LC.CUSTOM_SAMPLE[0]]
    generated = tr.env.statistics()["GeneratedPersons(10Minutes)"]
    held = sum(len(q) for q in tr.env.up + tr.env.down) + tr.log["boarded"] + tr.log["give_up"]
    assert generated > held > 0
    # the step after the last compared one enters row 2, where numpy itself leaves the multiplication method
    nxt = O.Env(LC.custom_config(F, run["flow"]), 1)
    for k in range(run["K2"]):
        nxt.step([-1, 0] * LC.CUSTOM[F][0])
    assert nxt.time_index == 1
    nxt.step([-1, 0] * LC.CUSTOM[F][0])
    assert nxt.time_index == 2


def test_custom_one_row_table():
    run = LC.custom_run(2, True)
    assert run["flow"].shape == (1, 8) and run["crossed"] == 0 and run["max_queue"] < LC.CUSTOM_Q
    assert run["log"]["boarded"] > 0


# ---------------------------------------------------------------------------------------------- the stream horizon
def test_horizon_case_a_flags_some_envs_and_not_others():
    c, run = LC.HORIZON_A, LC.horizon_a_run()
    first = run["first"]
    assert (first >= 0).sum() >= 4 and (first > 0).sum() >= 2 and (first < 0).sum() >= c["N"] // 2
    assert (first[:64] >= 0).any() and (first[64:] >= 0).any()      # in the full wave and in the partial one
    assert c["total_lam"] / c["F"] < 10.0 and run["max_queue"] < c["Q"]
    # a flagged lane has unflagged neighbours on both sides in its wave
    assert any(first[e - 1] < 0 and first[e + 1] < 0 for e in np.nonzero(first >= 0)[0] if 0 < e % 64 < 63 and e + 1 < c["N"])


def test_horizon_case_b_crosses_a_block_in_almost_every_step_and_never_the_horizon():
    run = LC.horizon_b_run()
    steps = LC.HORIZON_B["steps"] * LC.HORIZON_B["N"]              # all 64 envs count, not the compared sample alone
    assert run["crossed"] == 0 and run["min_words"] >= 500
    assert run["block_crossings"] > 0.75 * steps


def test_horizon_case_c_is_past_every_horizon_in_the_first_step():
    c = LC.HORIZON_C
    cfg = O.Config(generator="UNIFORM", dt=0.5, particle_number=c["particle_number"], generation_interval=150.0)
    for e in (0, 1, c["N"] - 1):
        tr = LC.Tracked(cfg, c["seed"] + e)
        tr.step([-1, 0] * 4)
        assert tr.py_words >= 2 * c["particle_number"] > LC.REC and tr.crossed and tr.env.max_queue < 128


# ---------------------------------------------------------------------------------------------- a wrapped queue ring
def test_a_queue_ring_wraps_and_persons_board_from_it():
    run = LC.wrap_run()
    log = run["log"]
    assert run["Q"] <= 128 and run["crossed"] == 0
    assert run["delivered"] > 0                                  # these actions serve the building
    assert log["wrapped"] > 0 and log["boarded_while_wrapped"] > 0 and log["give_up_past_last_slot"] > 0
    assert len(run["probes"]) >= 2
    for e, k, qd, head, n in run["probes"]:
        assert head + n > run["Q"] and 0 < head < run["Q"] and n <= run["Q"] - 1 and 300 < k < LC.WRAP["steps"]


def test_ring_model_follows_a_hand_made_queue():
    log = collections.Counter()
    q = LC._Ring()
    q.start(4, log)
    for x in range(3):
        q.appendleft(x)
    q.end_step()
    assert (q.head, len(q)) == (0, 3) and not log["wrapped"]
    q.pop()                      # a give-up: the head moves on
    q.pop()
    q.appendleft(3)
    q.appendleft(4)
    q.end_step()
    assert (q.head, len(q)) == (2, 3) and log["wrapped"] == 1     # slots 2, 3, 0
    del q[len(q) - 1]            # the oldest boards: compaction keeps the head
    assert log["boarded_while_wrapped"] == 1 and log["mid_deque_delete"] == 0
    q.pop()
    q.pop()
    q.end_step()
    assert (q.head, len(q)) == (0, 0)                             # empty at a step's end: the head returns to slot 0


# ---------------------------------------------------------------------------------------------- the reference's runs
def _final(golden, name, env):
    st, up, down = O.state_array(env.mansion_state())
    np.testing.assert_array_equal(st, golden[name + "_state"])
    np.testing.assert_array_equal(up, golden[name + "_up"])
    np.testing.assert_array_equal(down, golden[name + "_down"])
    assert env.statistics() == json.loads(str(golden[name + "_statistics"]))
    pk, pp, nk, npos = LC.streams(env)
    np.testing.assert_array_equal(pk, golden[name + "_py_key"])
    np.testing.assert_array_equal(nk, golden[name + "_np_key"])
    assert (pp, npos) == (int(golden[name + "_py_pos"]), int(golden[name + "_np_pos"]))


def test_the_reference_accepted_every_edge_config(golden):
    assert set(json.loads(str(golden["refusals"])).values()) == {"none"}
    assert json.loads(str(golden["runs"])) == sorted(["big_0", "big_1"] + ["custom%d_%d" % (F, s) for F in (2, 9, 16)
                                                                            for s in (0, 1)])


@pytest.mark.parametrize("F", [2, 9, 16])
@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_reproduces_the_reference_on_the_synthetic_tables(golden, F, seed):
    name = "custom%d_%d" % (F, seed)
    E, dt = LC.CUSTOM[F]
    steps = int(golden[name + "_steps"])
    assert steps == LC.steps_to_row2(dt)
    env = O.Env(LC.custom_config(F, LC.edge_flow(F)), seed)
    acts = O.scripted_actions(seed, steps, F, E)
    for k in range(steps):
        r, info = env.step([int(x) for x in acts[k]])
        assert LC.row(r, info) == [golden[name + "_reward"][k]] + golden[name + "_info"][k].tolist(), k
    # the oracle measures its longest queue before boarding, the fixture after the step
    assert env.time_index == 1 and 128 < int(golden[name + "_max_queue"]) <= env.max_queue < LC.CUSTOM_Q
    _final(golden, name, env)


@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_reproduces_the_reference_dispatcher_at_128_floors(golden, seed):
    name = "big_%d" % seed
    steps = int(golden[name + "_steps"])
    assert steps == LC.BIG[(128, 32)]
    env = O.Env(LC.big_config(128, 32), seed)
    stats = {}
    for k in range(steps):
        a = R.policy(env.mansion_state(), stats)
        assert a == golden[name + "_actions"][k].tolist(), k
        r, info = env.step(a)
        assert LC.row(r, info) == [golden[name + "_reward"][k]] + golden[name + "_info"][k].tolist(), k
    _final(golden, name, env)
    ev = json.loads(str(golden[name + "_events"]))
    assert ev["max_line"] == stats["max_line"] == 32               # the reference's own queue was 32 long


@pytest.mark.parametrize("F", [2, 9, 16])
def test_host_tables_equal_the_references_at_other_floor_counts(golden, F):
    from metagym_amd.liftsim import custom_tables
    E, dt = LC.CUSTOM[F]
    tb = custom_tables(LC.edge_flow(F), F, dt)
    assert tb["dens"].dtype == np.float32 == golden["custom%d_in_density" % F].dtype
    np.testing.assert_array_equal(tb["dens"], golden["custom%d_in_density" % F])
    np.testing.assert_array_equal(tb["out_prob"], golden["custom%d_out_prob" % F])
    lam = golden["custom%d_in_density" % F] * dt          # the reference's own expression: float32 times a Python float
    assert lam.dtype == np.float32
    assert tb["enlam"].tolist() == [[math.exp(-float(x)) for x in r] for r in lam]
    ot = O.custom_tables(LC.edge_flow(F), F)
    np.testing.assert_array_equal(ot.dens, tb["dens"])
    np.testing.assert_array_equal(ot.prob, tb["prob"])


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from metagym_amd import _lib
    from metagym_amd.liftsim import LiftSim, custom_tables
    lib = _lib.load()
    c = _lib.LiftsimConfig()
    c.floors, c.elevators, c.queue_capacity, c.window, c.dt, c.floor_height = 17, 2, 128, 1200, 0.5, 4.0
    c.generator, c.table_len = 0, 1
    for name in ("times", "dens", "enlam", "pp", "flip", "logq", "qn"):
        setattr(c, name, 8)                                # not NULL; the check reads no table
    offs = (C.c_int64 * len(_lib.LIFTSIM_FIELDS))()
    total = C.c_int64()
    assert lib.mg_liftsim_layout(c, 64, offs, total) == -1003
    with pytest.raises(_lib.MetaGymHipError, match="need <= 16"):      # what LiftSim's constructor raises through
        _lib.check(lib.mg_liftsim_layout(c, 64, offs, total), "mg_liftsim_layout")
    c.floors = 16
    assert lib.mg_liftsim_layout(c, 64, offs, total) == 0
    with pytest.raises(AssertionError, match="column of the dataset"):
        custom_tables(LC.edge_flow(8)[:, :-1], 8, 0.5)
    with pytest.raises(AssertionError, match="column of the dataset"):
        LiftSim(num_envs=4, floors=8, elevators=2, flow=np.concatenate([LC.edge_flow(8), np.zeros((3, 2))], axis=1))
    with pytest.raises(ValueError):
        LiftSim(num_envs=4, floors=129, elevators=4, generator="UNIFORM")
    with pytest.raises(ValueError):
        LiftSim(num_envs=4, floors=10, elevators=33, generator="UNIFORM")
