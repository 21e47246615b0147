"""The size grid of the in-launch networks, host side (no GPU): every path the kernels' remainder code can take is walked by a
size some GPU test runs (tests/policy_size_cases.py restates the loop bounds), and at every size tests/test_policy_sizes_gpu.py
adds, the packed layout round-trips, has the library's count, and holds +0 in exactly the floats `padding_mask` names."""
import numpy as np
import pytest

import policy_size_cases as SC

LAUNCHES = sorted(SC.LAUNCHES)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1. path coverage
@pytest.mark.parametrize("launch", LAUNCHES)
def test_existing_and_added_sizes_walk_every_path(launch):
    paths, legal, existing, added = SC.LAUNCHES[launch]
    full = set().union(*[paths(s) for s in legal])
    old = set().union(*[paths(s) for s in existing])
    new = set().union(*[paths(s) for s in added])
    assert all(s in legal for s in existing + added) and not set(existing) & set(added)
    assert old | new == full, (launch, "no size walks", sorted(full - old - new))
    for s in added:                                        # every added size walks a path no older size does
        assert paths(s) - old, (launch, s, "adds nothing")


def test_the_path_functions_on_sizes_worked_out_by_hand():
    """H = 39 = 32 + 4 + 3: one group, one quad entered at i = 32, then v.x, v.y and v.z of the partial quad. H = 64: two
    groups and nothing else. H = 5: one quad and v.x alone."""
    assert SC.paths("quadrotor_recurrent", (39, 16)) == {"group", "single_group", "quad", "quad_after_group", "partial3",
                                                         "partial_after_quad", "ends_on_partial"}
    assert SC.paths("quadrotor_recurrent", (64, 16)) == {"group", "two_groups", "ends_on_group", "max_size"}
    assert SC.paths("quadrotor_recurrent", (5, 16)) == {"quad", "partial1", "partial_after_quad", "ends_on_partial"}
    assert SC.paths("quadrotor_recurrent", (35, 16)) == {"group", "single_group", "partial3", "partial_after_group", "ends_on_partial"}
    assert SC.paths("quadrotor_recurrent", (35, 19)) == SC.paths("quadrotor_recurrent", (35, 16)) | {
        "wx_padded", "group_DP20", "partial_after_group_DP20"}
    assert SC.paths("quadrotor_recurrent", (63, 16)) >= {"quad_after_group", "partial_after_quad", "max_minus_1"}
    assert SC.paths("maze", (2, 4)) == {"quad", "one_whole_quad_only", "ends_on_quad"}
    assert SC.paths("maze", (3, 63)) == {"quad", "partial3", "partial_after_quad", "ends_on_partial", "max_minus_1"}
    assert SC.paths("bandits", (5, 2)) == {"partial2", "ends_on_partial", "K_mod4_1"}
    assert "K_whole_quads_below_the_limit" in SC.paths("bandits", (4, 4)) and "K_whole_quads_below_the_limit" not in SC.paths("bandits", (64, 64))
    assert "choice_blocks_all_full" in SC.paths("liftsim", (5, 2, 2)) and "choice_block_partial2" in SC.paths("liftsim", (10, 4, 8))
    assert SC.paths("liftsim", (33, 2, 5)) >= {"floor_set_partial_word_after_full", "unit_block_partial_after_full", "F_mod4_1"}
    assert SC.paths("walker_recurrent", ("ant", 193)) >= {"units_per_lane_4", "uneven_lanes_4", "h_several_groups", "h_rest_after_group"}
    assert SC.paths("walker_recurrent", ("ant", 32)) >= {"h_one_group", "h_no_rest", "some_lanes_idle"}
    assert "h_rest_one_short_of_a_group" in SC.paths("walker_recurrent", ("ant", 31))
    assert SC.paths("walker_mlp", ("ant", 64)) == {"units_per_lane_1", "full_wave_exact", "one_unit_on_every_lane"}
    assert SC.paths("quadrotor_mlp", 256) == {"hidden_loop", "copy_several_passes", "copy_tail_one_lane", "max_size"}
    assert SC.paths("quadrotor_mlp", 33) - SC.paths("quadrotor_mlp", 32) == {"copy_tail_partial", "partial_tail_after_full_pass"}
    assert SC._mlp_pieces(256) == 1537 and 4 * 1537 * 4 == 24592
    import quadrotor_rpolicy_cases as rc
    assert [s[0] for s in SC.QUADROTOR_RECURRENT_EXISTING[:3]] == list(rc.HIDDEN)
    assert all(SC.liftsim_stages_the_policy(s) for s in SC.LIFTSIM_ADDED) and not SC.liftsim_stages_the_policy((128, 32, 64))


# ---------------------------------------------------------------------------------------------- 2. the layout at every added size
ADDED = SC.added_policies()
IDS = ["%s-%s" % (launch, "x".join(str(v) for v in (size if isinstance(size, tuple) else (size,)))) for launch, size, _ in ADDED]


def _library_count(lib, launch, pol):
    if launch == "quadrotor_mlp":
        return lib.mg_quadrotor_policy_param_count(pol.hidden, pol.obs_dim)
    if launch == "quadrotor_recurrent":
        return lib.mg_quadrotor_rpolicy_param_count(pol.hidden, pol.obs_dim)
    if launch == "maze":
        return lib.mg_maze2d_policy_param_count(pol.hidden, pol.view_grid)
    if launch == "bandits":
        return lib.mg_bandits_policy_param_count(pol.hidden, pol.arms)
    if launch == "liftsim":
        return lib.mg_liftsim_policy_param_count(pol.hidden, pol.floors, pol.elevators)
    if launch == "walker_mlp":
        return lib.mg_walker_policy_param_count(pol.hidden, pol.obs_dim, pol.n_act)
    return lib.mg_walker_rpolicy_param_count(pol.hidden, pol.obs_dim, pol.n_act)


def _unpack(launch, pol, packed):
    cls = type(pol)
    if launch in ("quadrotor_mlp", "quadrotor_recurrent"):
        return cls.unpack(packed, pol.hidden, pol.obs_dim)
    if launch == "maze":
        return cls.unpack(packed, pol.hidden, pol.view_grid)
    if launch == "bandits":
        return cls.unpack(packed, pol.hidden, pol.arms)
    if launch == "liftsim":
        return cls.unpack(packed, pol.hidden, pol.floors, pol.elevators)
    return cls.unpack(packed, pol.hidden, pol.obs_dim, pol.n_act)


WEIGHTS = {"quadrotor_mlp": ("w1", "b1", "w2", "b2"), "quadrotor_recurrent": ("wx", "wa", "wr", "wd", "wh", "b", "wo", "bo"),
           "maze": ("wx", "wh", "b", "wo", "bo"), "bandits": ("wa", "wr", "wd", "wh", "b", "wo", "bo"),
           "liftsim": ("ws", "we", "wt", "wr", "wu", "wd", "b", "wo", "bo"), "walker_mlp": ("w1", "b1", "w2", "b2"),
           "walker_recurrent": ("wx", "wa", "wr", "wd", "wh", "b", "wo", "bo")}


@pytest.mark.parametrize("launch,size,pol", ADDED, ids=IDS)
def test_layout_at_an_added_size(launch, size, pol):
    from metagym_amd import _lib
    lib = _lib.load()
    packed = pol.pack()
    assert packed.dtype == np.float32 and packed.shape == (SC.P, pol.param_count)
    assert _library_count(lib, launch, pol) == pol.param_count
    back = _unpack(launch, pol, packed)
    for name in WEIGHTS[launch]:
        assert np.array_equal(_bits(getattr(pol, name)), _bits(getattr(back, name))), name
    assert np.array_equal(_bits(back.pack()), _bits(packed))
    # the padding: where the documented layout puts no weight, and nowhere else; its count is the header's closed form
    mask = SC.padding_mask(pol)
    assert mask.dtype == np.bool_ and mask.shape == (pol.param_count,)
    assert int(mask.sum()) == SC.padding_count(pol)
    if launch.startswith("walker"):
        assert not mask.any()                                                 # the walker layouts are dense
    else:
        assert pol.param_count % 4 == 0 and (mask.any() or (launch, size) == ("maze", (2, 4)))      # H = 4: HP = H
    assert not _bits(packed[:, mask]).any()                                   # the bit pattern of +0, not just == 0
    ones = type(pol).__new__(type(pol))
    ones.__dict__.update(pol.__dict__)
    for name in WEIGHTS[launch]:
        setattr(ones, name, np.ones_like(getattr(pol, name)))
    one = ones.pack()
    assert np.array_equal(one == 0, np.broadcast_to(mask, one.shape)) and (one[:, ~mask] == 1).all()
    # a weight set that is nowhere zero lands nowhere in the padding either
    assert (packed[:, ~mask] != 0).mean() > 0.99


def test_padding_masks_of_the_older_sizes_and_the_dense_layouts():
    """The closed forms at sizes with and without padding: H a multiple of four, D = 19 (the MLP record is full, the recurrent
    one pads wx by one), K and F multiples of four, and the linear forms."""
    assert int(SC.padding_mask(SC.quadrotor_mlp(5, 16)).sum()) == 15 and not SC.padding_mask(SC.quadrotor_mlp(5, 19)).any()
    assert not SC.padding_mask(SC.quadrotor_mlp(0, 16)).any()
    assert int(SC.padding_mask(SC.quadrotor_recurrent((64, 16))).sum()) == 64           # the fourth float of (b, wr, wd, 0)
    assert int(SC.padding_mask(SC.quadrotor_recurrent((5, 19))).sum()) == 5 * (1 + 1 + 3)
    assert not SC.padding_mask(SC.maze_policy((1, 64), seed=1)).any()
    assert int(SC.padding_mask(SC.maze_policy((2, 5), seed=1)).sum()) == 5 * 3
    assert int(SC.padding_mask(SC.bandits_policy((64, 64), seed=1)).sum()) == 64 + 3 * 64
    assert int(SC.padding_mask(SC.liftsim_policy((128, 32, 64), seed=1)).sum()) == 64 * (3 + 3) + 258 * 3
    for pol in (SC.walker_policy(("ant", 0 + 70), False), SC.walker_policy(("humanoid", 65), True)):
        assert not SC.padding_mask(pol).any() and SC.padding_count(pol) == 0
