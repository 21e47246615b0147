"""The sizes at which the seven in-launch networks are pinned, derived from the kernels' own remainder code.

H, K, F, E and D are run-time values, and every policy kernel walks them with hand-written loops: groups of 32, whole quads,
a partial quad, units striped over 64 lanes, records padded to four floats. For each launch a small function below restates
those loop bounds (with the default group size, 32) and names the paths a size takes; beside it stand the sizes the older
tests run (EXISTING) and the ones tests/test_policy_sizes_gpu.py adds (ADDED). tests/test_policy_sizes.py checks that the two
together reach every path the function can name, so a trimmed grid fails on the CPU.

`paths(launch, size)` is the set of named facts about the loops: which stage runs, which stage follows which, where the walk
ends. `padding_mask(policy)` is the bool mask of the packed floats no weight maps to, computed from the layouts documented in include/metagym_hip.h, not from pack().
Nothing here touches a kernel or needs a GPU."""
import numpy as np

from metagym_amd._policy import pad4 as _pad4

GROUP = 32          # RP_H_GROUP (csrc/quadrotor_policy.hip) and MG_WALKER_RP_GROUP (csrc/walker_core.h), their defaults
WAVE = 64
N, P, T = 130, 3, 12          # two waves and a 2-lane tail; lanes 0..63 on one policy id, the rest mixed (layout_ids)
WALKER_N, WALKER_T = 65, 6    # one workgroup per env
LIFT_T, LIFT_SAMPLE = 60, (0, 64, 129)


def layout_ids(n=N):
    """quadrotor_policy_cases.layout_ids: one id over lanes 0..63 (staged in LDS), e % 3 over 64..127 (per-lane reads), the
    tail on one id."""
    ids = np.arange(n) % P
    ids[:64] = 1
    ids[128:] = 2
    return ids.astype(np.int32)


# ---------------------------------------------------------------------------------------------- walks
def _quad_walk(n, group=0, prefix=""):
    """The named paths of a sum over n terms that is read as whole groups of `group` terms (0: the kernel has no group
    loop), then whole quads, then a partial quad of n % 4."""
    g = n // group if group else 0
    q = (n - g * group) // 4
    p = n % 4
    out = set()
    if g:
        out.add("group")
        out.add("single_group" if g == 1 else "two_groups")       # the loop leaves after its first pass / takes its back edge
    if q:
        out.add("quad")
        if g:
            out.add("quad_after_group")                           # the quad loop is entered at i = 32
        if q == 1 and g == 0 and p == 0:
            out.add("one_whole_quad_only")                        # the body runs once with every guard true, and nothing follows
    if p:
        out.add("partial%d" % p)
        if q:
            out.add("partial_after_quad")
        elif g:
            out.add("partial_after_group")
    out.add("ends_on_partial" if p else ("ends_on_quad" if q else "ends_on_group"))
    return {prefix + name for name in out}


def _limits(value, limit, name="", under=True):
    """The limit itself, and one under it where the walk there differs from the limit's (a partial quad after whole ones)."""
    return {name + "max_size"} if value == limit else ({name + "max_minus_1"} if under and value == limit - 1 else set())


# ---------------------------------------------------------------------------------------------- quadrotor, recurrent
# rpolicy_eval: for (; i < hgroup; i += 32) / for (; i < hfull; i += 4) / if (hfull < hidden) with the v.y and v.z guards.
# size = (H, D). D = 19 pads wx to DP = 20 (w[19] is loaded and never multiplied) and moves rh = r + DP + 8: what starts at
# i = 32 is named a second time for it.
def quadrotor_recurrent_paths(size):
    H, D = size
    paths = _quad_walk(H, GROUP) | _limits(H, 64)
    if D == 19:
        paths = paths | {"wx_padded"} | {p + "_DP20" for p in ("group", "quad_after_group", "partial_after_group", "max_size") if p in paths}
    return paths


QUADROTOR_RECURRENT_RANGE = [(H, D) for D in (16, 19) for H in range(1, 65)]
QUADROTOR_RECURRENT_EXISTING = [(1, 16), (5, 16), (64, 16), (5, 19), (64, 19)]   # quadrotor_rpolicy_cases.HIDDEN; the velocity tests
QUADROTOR_RECURRENT_ADDED = [(H, 16) for H in (2, 3, 4, 32, 33, 35, 36, 39, 63)] + [(39, 19), (35, 19)]


# ---------------------------------------------------------------------------------------------- quadrotor, MLP
# policy_eval's j loop has no remainder; what changes with H is the staging copy, for (i = lane; i < count / 4; i += 64),
# and the dynamic LDS it fills (24 592 bytes at H = 256). size = H, at D = 16. H = 32 copies 193 pieces, three passes and one
# lane; H = 33 is the first size whose copy ends, after whole passes, on a pass of several lanes.
def _mlp_pieces(H):
    return (4 + 24 * H) // 4 if H else (4 + 4 * 16) // 4


def quadrotor_mlp_paths(H):
    pieces = _mlp_pieces(H)
    passes, tail = -(-pieces // WAVE), pieces % WAVE
    paths = {"linear"} if H == 0 else {"hidden_loop"}
    paths.add("copy_one_pass" if passes == 1 else "copy_several_passes")
    paths.add("copy_tail_one_lane" if tail == 1 else "copy_tail_partial")          # (pieces is odd: never a full tail)
    if passes > 1 and tail > 1:
        paths.add("partial_tail_after_full_pass")
    return paths | _limits(H, 256, under=False)


QUADROTOR_MLP_RANGE = list(range(0, 257))
QUADROTOR_MLP_EXISTING = [0, 1, 5, 32]
QUADROTOR_MLP_ADDED = [33, 256]


# ---------------------------------------------------------------------------------------------- maze
# policy_eval<D>: for (i = 0; i < hp; i += 4) with if (i + 1/2/3 < hidden). size = (view_grid, H); the walk depends on H only.
def maze_paths(size):
    return _quad_walk(size[1]) | _limits(size[1], 64)


MAZE_RANGE = [(vg, H) for vg in (1, 2, 3) for H in range(1, 65)]
MAZE_EXISTING = [(1, 5), (3, 64), (2, 1), (2, 5), (1, 64), (1, 1)]                 # test_maze_policy_gpu.CASES
MAZE_ADDED = [(1, 2), (2, 3), (3, 6), (1, 7), (2, 4), (3, 63)]
MAZE_SEEDS = {(1, 2): 31, (2, 3): 32, (3, 6): 33, (1, 7): 34, (2, 4): 35, (3, 63): 36}    # weight seeds of make_policy


# ---------------------------------------------------------------------------------------------- bandits
# bp_eval: the guarded quad over h twice (units, arms); K only pads the wa group to KP, which moves rh = r + 4 + kp and puts
# the lookup r[4 + prev_action] next to padding. The one older K that is a multiple of four is the limit, 64. size = (K, H).
def bandits_paths(size):
    K, H = size
    paths = _quad_walk(H) | {"K_mod4_%d" % (K % 4)} | _limits(H, 64, "H_") | _limits(K, 64, "K_")
    if K % 4 == 0 and K < 64:
        paths.add("K_whole_quads_below_the_limit")
    return paths


BANDITS_RANGE = [(K, H) for K in range(2, 65) for H in range(1, 65)]
BANDITS_EXISTING = [(2, 1), (3, 3), (10, 5), (64, 64)]                              # test_full_closed_loop_oracle
BANDITS_ADDED = [(5, 2), (4, 4), (7, 6), (63, 7), (6, 63)]
BANDITS_SEEDS = {(5, 2): 41, (4, 4): 42, (7, 6): 43, (63, 7): 44, (6, 63): 45}


# ---------------------------------------------------------------------------------------------- liftsim
# lp_eval: units four at a time (unit_heads of liftsim_policy_core.h clamps the records with min(j + u, hidden - 1), lp_eval
# guards the stores with j + u < hidden); argmax_choice of that header: choices four at a time (A = 2F + 2: A % 4 is 2 for an
# even F and 0 for an odd one, and every older case has an even F); inside, the guarded quad over h. F and E pad the groups
# we | wt | wr | wu | wd, and F sets the words of the three floor sets (nb = min(32, F - 32 w) bits each). size = (F, E, H).
def liftsim_paths(size):
    F, E, H = size
    paths = _quad_walk(H, prefix="logit_")
    if H >= 4:
        paths.add("unit_block_full")
    if H % 4:
        paths.add("unit_block_partial%d" % (H % 4))
        if H > 4:
            paths.add("unit_block_partial_after_full")
    paths.add("choice_blocks_all_full" if (2 * F + 2) % 4 == 0 else "choice_block_partial2")
    paths |= {"F_mod4_%d" % (F % 4), "E_mod4_%d" % (E % 4)}
    words = -(-F // 32)
    paths.add("floor_set_one_word" if words == 1 else "floor_set_several_words")
    paths.add("floor_set_last_word_partial" if F % 32 else "floor_set_last_word_full")
    if words > 1 and F % 32:
        paths.add("floor_set_partial_word_after_full")
    return paths | _limits(H, 64, "H_")


LIFTSIM_RANGE = [(F, E, H) for F in (2, 3, 4, 5, 7, 9, 10, 32, 33, 128) for E in (1, 2, 3, 4, 32) for H in range(1, 65)]
LIFTSIM_EXISTING = [(10, 4, 8), (128, 32, 4), (2, 1, 1), (10, 4, 64)]               # liftsim_policy_cases.CASES
LIFTSIM_ADDED = [(5, 2, 2), (7, 3, 3), (33, 2, 5), (5, 3, 6), (7, 2, 7), (9, 3, 63)]
# weight seeds; with 59 nine choices occur on the three sampled envs of (7, 2, 7), where 55 gave two
LIFTSIM_SEEDS = {(5, 2, 2): 51, (7, 3, 3): 52, (33, 2, 5): 53, (5, 3, 6): 54, (7, 2, 7): 59, (9, 3, 63): 56}
# Busy halls, but with five floors to queue on the longest queue of 22 sampled envs stays at 34 of the 128 an env can hold
# (liftsim_cases.BIG_KW, 40 persons every 4 s, reaches 127 in 60 steps). At F = 33 down-calls at the top floor, bit 0 of the
# second word, occur in most steps.
LIFTSIM_KW = dict(generator="UNIFORM", dt=1.0, particle_number=16, generation_interval=8.0)
LIFTSIM_ENV_SEED = 17


def liftsim_stages_the_policy(size):
    """lp_lds_layout(stage = true).bytes <= 160 KiB, as mg_liftsim_policy_rollout decides it: the packed policy, H lane-minor
    columns, the 624 stream words and the three action/shuffle arrays of 32 x 64 entries (1, 2 and 1 bytes each)."""
    F, E, H = size
    unit = 12 + _pad4(E) + _pad4(F + 1) + 3 * _pad4(F)
    count = H * unit + (2 * F + 2) * (4 + _pad4(H))
    return 4 * count + 4 * 64 * H + 4 * 624 + 32 * 64 * (1 + 2 + 1) <= 160 * 1024


# ---------------------------------------------------------------------------------------------- walker (MetaLocomotion)
# Hidden unit u runs on lane u % 64: for (u = lane; u < H; u += 64). wave_rpolicy_sum reads whole groups of 32 terms, then a
# scalar rest; a recurrent unit's sum is two such runs, over in[] (n_in = D + A + 2: 38 for the ant, 63 for the humanoid) and
# over h[] (H terms), and the output layer is a third, over hn[] (H terms). size = (robot, H).
N_IN = {"ant": 28 + 8 + 2, "humanoid": 44 + 17 + 2}


def _lane_paths(H):
    most, least = -(-H // WAVE), H // WAVE
    paths = {"units_per_lane_%d" % most}
    if least == 0:
        paths.add("some_lanes_idle")
    if H % WAVE == 0:
        paths.add("full_wave_exact")
        if H == WAVE:
            paths.add("one_unit_on_every_lane")
    elif H > WAVE:
        paths |= {"uneven_lanes", "uneven_lanes_%d" % most}          # lanes below H % 64 run `most` units, the others one fewer
    return paths


def walker_mlp_paths(size):
    H = size[1]
    return {"linear"} if H == 0 else _lane_paths(H) | _limits(H, 256, under=False)


def walker_recurrent_paths(size):
    robot, H = size
    groups, rest = H // GROUP, H % GROUP
    paths = _lane_paths(H) | _limits(H, 256, under=False) | {"n_in_%d" % N_IN[robot]}
    paths.add("h_no_group" if groups == 0 else ("h_one_group" if groups == 1 else "h_several_groups"))
    paths.add("h_rest" if rest else "h_no_rest")
    if groups and rest:
        paths.add("h_rest_after_group")
    if rest == GROUP - 1:
        paths.add("h_rest_one_short_of_a_group")                     # the scalar loop at its longest
    return paths


WALKER_MLP_RANGE = [(r, H) for r in ("ant", "humanoid") for H in range(0, 257)]
WALKER_MLP_EXISTING = [(r, H) for r in ("ant", "humanoid") for H in (0, 1, 70, 256)]
WALKER_MLP_ADDED = [("ant", 64), ("ant", 129), ("ant", 193)]         # (193: four units on lane 0 and three on the others)
WALKER_RECURRENT_RANGE = [(r, H) for r in ("ant", "humanoid") for H in range(1, 257)]
WALKER_RECURRENT_EXISTING = [(r, H) for r in ("ant", "humanoid") for H in (1, 64, 65, 256)]
WALKER_RECURRENT_ADDED = [("ant", H) for H in (31, 32, 33, 129, 193)] + [("humanoid", 33)]


# ---------------------------------------------------------------------------------------------- the seven launches
LAUNCHES = {   # name -> (paths, every size the launch accepts (or a sample that reaches every path), existing, added)
    "quadrotor_recurrent": (quadrotor_recurrent_paths, QUADROTOR_RECURRENT_RANGE, QUADROTOR_RECURRENT_EXISTING, QUADROTOR_RECURRENT_ADDED),
    "quadrotor_mlp": (quadrotor_mlp_paths, QUADROTOR_MLP_RANGE, QUADROTOR_MLP_EXISTING, QUADROTOR_MLP_ADDED),
    "maze": (maze_paths, MAZE_RANGE, MAZE_EXISTING, MAZE_ADDED),
    "bandits": (bandits_paths, BANDITS_RANGE, BANDITS_EXISTING, BANDITS_ADDED),
    "liftsim": (liftsim_paths, LIFTSIM_RANGE, LIFTSIM_EXISTING, LIFTSIM_ADDED),
    "walker_recurrent": (walker_recurrent_paths, WALKER_RECURRENT_RANGE, WALKER_RECURRENT_EXISTING, WALKER_RECURRENT_ADDED),
    "walker_mlp": (walker_mlp_paths, WALKER_MLP_RANGE, WALKER_MLP_EXISTING, WALKER_MLP_ADDED),
}


def paths(launch, size):
    return set(LAUNCHES[launch][0](size))


# ---------------------------------------------------------------------------------------------- the padding of a packed policy
def _used(policy):
    """bool [param_count]: the floats a weight maps to, by the layouts documented in include/metagym_hip.h."""
    kind = type(policy).__name__
    used = np.zeros(policy.param_count, bool)
    H = policy.hidden
    if kind in ("WalkerPolicy", "WalkerRecurrentPolicy"):          # dense: b | one input-major matrix | bo | wo
        used[:] = True
    elif kind == "QuadrotorPolicy":                                 # b2[4], then H records of 24: w1[D], b1, zeros to 20, w2[4]
        if H == 0:
            used[:] = True
        else:
            D = policy.obs_dim
            used[:4] = True
            rec = used[4:].reshape(H, 24)
            rec[:, :D + 1] = True
            rec[:, 20:] = True
    elif kind == "QuadrotorRecurrentPolicy":      # bo[4], then H records: wx[D] to DP | b wr wd 0 | wa[4] | wh[H] to HP | wo[4]
        D, DP, HP = policy.obs_dim, _pad4(policy.obs_dim), _pad4(H)
        used[:4] = True
        rec = used[4:].reshape(H, DP + HP + 12)
        rec[:, :D] = True
        rec[:, DP:DP + 3] = True
        rec[:, DP + 4:DP + 8 + H] = True
        rec[:, DP + 8 + HP:] = True
    elif kind == "MazePolicy":                                      # bo[4], then H records: wx[D], b, wh[H] to HP, wo[4]
        D, HP = policy.input_dim, _pad4(H)
        used[:4] = True
        rec = used[4:].reshape(H, D + 1 + HP + 4)
        rec[:, :D + 1 + H] = True
        rec[:, D + 1 + HP:] = True
    elif kind == "BanditPolicy":                  # H records: b wr wd 0 | wa[K] to KP | wh[H] to HP; K records: bo 0 0 0 | wo[H] to HP
        K, KP, HP = policy.arms, _pad4(policy.arms), _pad4(H)
        unit = used[:H * (4 + KP + HP)].reshape(H, 4 + KP + HP)
        unit[:, :3] = True
        unit[:, 4:4 + K] = True
        unit[:, 4 + KP:4 + KP + H] = True
        arm = used[H * (4 + KP + HP):].reshape(K, 4 + HP)
        arm[:, 0] = True
        arm[:, 4:4 + H] = True
    elif kind == "LiftPolicy":        # H records: b | ws[8] | we[E] | wt[F+1] | wr[F] | wu[F] | wd[F], each to a multiple of 4;
        F, E, HP = policy.floors, policy.elevators, _pad4(H)       # A records: bo 0 0 0 | wo[H] to HP
        sizes = (1, 8, E, F + 1, F, F, F)
        ru = sum(_pad4(n) for n in sizes)
        unit = used[:H * ru].reshape(H, ru)
        o = 0
        for n in sizes:
            unit[:, o:o + n] = True
            o += _pad4(n)
        choice = used[H * ru:].reshape(2 * F + 2, 4 + HP)
        choice[:, 0] = True
        choice[:, 4:4 + H] = True
    else:
        raise TypeError("no packed layout is known for %s" % kind)
    return used


def padding_mask(policy):
    """bool [param_count]: True at the packed floats no weight maps to (the same for each of the P policies)."""
    return ~_used(policy)


def padding_count(policy):
    """Padding floats per packed policy, by the closed forms of the header's record definitions."""
    kind = type(policy).__name__
    H = policy.hidden
    hpad = _pad4(H) - H
    if kind in ("WalkerPolicy", "WalkerRecurrentPolicy"):
        return 0
    if kind == "QuadrotorPolicy":
        return H * (19 - policy.obs_dim)
    if kind == "QuadrotorRecurrentPolicy":
        return H * (_pad4(policy.obs_dim) - policy.obs_dim + 1 + hpad)
    if kind == "MazePolicy":
        return H * hpad
    if kind == "BanditPolicy":
        K = policy.arms
        return H * (1 + _pad4(K) - K + hpad) + K * (3 + hpad)
    if kind == "LiftPolicy":
        F, E = policy.floors, policy.elevators
        return H * (3 + _pad4(E) - E + _pad4(F + 1) - (F + 1) + 3 * (_pad4(F) - F)) + (2 * F + 2) * (3 + hpad)
    raise TypeError("no packed layout is known for %s" % kind)


# ---------------------------------------------------------------------------------------------- policies at a size (CPU)
F32 = np.float32


def quadrotor_mlp(H, D=16):
    import quadrotor_policy_cases as pc
    return pc.make_policy(H, D)


def quadrotor_recurrent(size):
    import quadrotor_rpolicy_cases as rc
    return rc.make_rpolicy(size[0], size[1])


def maze_policy(size, seed=None, n_policies=P):
    """test_maze_policy_gpu.make_policy: weights scaled by 3 / sqrt(fan-in), so the clamp is hit on both sides and not always."""
    from metagym_amd.metamaze.policy import MazePolicy, input_dim
    vg, H = size
    rs = np.random.RandomState(MAZE_SEEDS[size] if seed is None else seed)
    D = input_dim(vg)
    fan = np.sqrt(D + H)
    return MazePolicy((rs.randn(n_policies, H, D) * (3.0 / fan)).astype(F32), (rs.randn(n_policies, H, H) * (3.0 / fan)).astype(F32),
                      (0.3 * rs.randn(n_policies, H)).astype(F32), (rs.randn(n_policies, 4, H) / np.sqrt(H)).astype(F32),
                      (0.2 * rs.randn(n_policies, 4)).astype(F32))


def bandits_policy(size, seed=None, n_policies=P):
    """test_bandits_policy_gpu.make_policy: inputs of order one, wh and wo scaled by 1 / sqrt(H)."""
    from metagym_amd.bandits import BanditPolicy
    K, H = size
    rs = np.random.RandomState(BANDITS_SEEDS[size] if seed is None else seed)
    return BanditPolicy((1.5 * rs.randn(n_policies, H, K)).astype(F32), (1.5 * rs.randn(n_policies, H)).astype(F32),
                        rs.randn(n_policies, H).astype(F32), (rs.randn(n_policies, H, H) * (2.0 / np.sqrt(H))).astype(F32),
                        (0.3 * rs.randn(n_policies, H)).astype(F32), (rs.randn(n_policies, K, H) / np.sqrt(H)).astype(F32),
                        (0.2 * rs.randn(n_policies, K)).astype(F32))


def liftsim_policy(size, seed=None, n_policies=P):
    """liftsim_policy_cases.random_weights (N(0, 0.5^2)), the output layer scaled by 1 / sqrt(H)."""
    import liftsim_policy_cases as PC
    from metagym_amd.liftsim import LiftPolicy
    F, E, H = size
    w = PC.random_weights(np.random.RandomState(LIFTSIM_SEEDS[size] if seed is None else seed), n_policies, H, F, E)
    w[7] = (w[7] / np.sqrt(H)).astype(F32)
    return LiftPolicy(*w)


def liftsim_case(size):
    import liftsim_policy_cases as PC
    F, E, H = size
    return PC._case(dict(floors=F, elevators=E, **LIFTSIM_KW), N, LIFTSIM_ENV_SEED, LIFT_SAMPLE, LIFT_T, H)


def walker_dims(robot):
    return {"ant": (28, 8), "humanoid": (44, 17)}[robot]


def walker_policy(size, recurrent, seed=17, n_policies=P):
    """test_walker_policy_gpu._policy / test_walker_rpolicy_gpu._policy: weights uniform in +-0.05, biases in +-0.1. The
    recurrent form's hidden biases are uniform in +-1.5 instead: the weighted inputs add a few tenths, so the units with |b|
    near 1.5 end at the clamp and the others inside it."""
    from metagym_amd.metalocomotion import WalkerPolicy, WalkerRecurrentPolicy
    robot, H = size
    D, A = walker_dims(robot)
    g = np.random.RandomState(seed)
    u = lambda s, *shape: g.uniform(-s, s, size=shape).astype(F32)
    Pn = n_policies
    if recurrent:
        return WalkerRecurrentPolicy(u(0.05, Pn, H, D), u(0.05, Pn, H, A), u(0.05, Pn, H), u(0.05, Pn, H), u(0.05, Pn, H, H),
                                     u(1.5, Pn, H), u(0.05, Pn, A, H), u(0.1, Pn, A))
    return WalkerPolicy(u(0.05, Pn, H, D), u(0.1, Pn, H), u(0.05, Pn, A, H), u(0.1, Pn, A))


def added_policies():
    """(launch, size, policy) for every added size of every launch."""
    out = [("quadrotor_recurrent", s, quadrotor_recurrent(s)) for s in QUADROTOR_RECURRENT_ADDED]
    out += [("quadrotor_mlp", H, quadrotor_mlp(H)) for H in QUADROTOR_MLP_ADDED]
    out += [("maze", s, maze_policy(s)) for s in MAZE_ADDED]
    out += [("bandits", s, bandits_policy(s)) for s in BANDITS_ADDED]
    out += [("liftsim", s, liftsim_policy(s)) for s in LIFTSIM_ADDED]
    out += [("walker_recurrent", s, walker_policy(s, True)) for s in WALKER_RECURRENT_ADDED]
    out += [("walker_mlp", s, walker_policy(s, False)) for s in WALKER_MLP_ADDED]
    return out
