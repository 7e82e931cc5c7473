"""Ordered IK groups on the device (rt_skeleton_solve_ik_groups, rt_crowd_set_ik_chain_groups + rt_crowd_solve_ik; include/dxr_amd.h "Posed
skeletons", inverse kinematics, GROUPS): a grouped call leaves pose, joints and palette exactly as one rt_skeleton_solve_ik per group in
order does, and as the numpy statement (tests/ik_group_cases.py) says, byte for byte -- on a skeleton, and for every actor of a crowd from
host and from device memory; the shapes a list may take; values the host never sees; sequences; every refusal with its message, and nothing
changed by it; an attached scene and a skinned model; the example.  Every dependent case is one whose result differs in bits from the whole
list solved side by side from the one input pose, so a kernel that forgot the walk between its stages fails.  No tolerance but the example's."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import crowd_ik_cases as CI
import ik_cases as IK
import ik_group_cases as G
import skeleton_cases as S
import skin_cases as K
from test_gpu_crowd import reads, skeleton_with
from test_gpu_crowd_device import assert_same, on_device
from test_gpu_crowd_ik import assert_actor, solve
from test_gpu_instance_attach import check_equals_build, gpu_scene
from test_gpu_model_deform import own_scene, close_all
from test_gpu_model_skin import assert_vertices
from test_gpu_skeleton import assert_floats, gentle_clip
from test_gpu_skeleton_ik import written
from util import random_xforms

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
RIGS = {name: (parents, groups) for name, parents, groups in G.skeleton_rigs()}
NAMES = ("pose", "joints", "palette")


def one_by_one(sk, pose, groups):
    """(pose, joints, palette) of a skeleton given set_pose and one solve_ik per group, in order"""
    sk.set_pose(pose)
    for g in groups:
        sk.solve_ik(g)
    return reads(sk)


def grouped(sk, pose, groups):
    sk.set_pose(pose)
    sk.solve_ik_groups(groups)
    return reads(sk)


def assert_reads(got, want, what, nans=False):
    for name, g, w in zip(NAMES, got, want):
        assert_floats(g, w, "%s: %s" % (what, name), nans)


# ---- a skeleton: the grouped call == the calls one by one == numpy ---------------------------------------------------------------------------
@pytest.mark.parametrize("rig", list(RIGS))
def test_skeleton_grouped_equals_successive_calls_equals_numpy(gpu, capi, rig):
    """every rig of ik_group_cases.skeleton_rigs -- the four-joint chain, the comb, the edges of the block widths and of LDS, and one joint
    above LDS, where the call is the loop -- from a unit pose and from a raw one"""
    parents, groups = RIGS[rig]
    n = len(parents)
    ib = S.inverse_binds(n, 1100 + n)
    sk, other = capi.Skeleton(gpu, parents, ib), capi.Skeleton(gpu, parents, ib)
    keep = ~written(parents, G.flat(groups))
    for family in ("unit", "raw"):
        pose = S.pose(family, parents, 1110 + n)
        assert G.is_dependent(parents, ib, pose, groups), "%s: the case would pass without the walk between the stages" % rig
        want = G.solved_and_posed(parents, ib, pose, groups)
        what = "%s, %s pose" % (rig, family)
        assert_reads(one_by_one(other, pose, groups), want, what + ": one call per group vs numpy")
        got = grouped(sk, pose, groups)
        assert_reads(got, want, what + ": the grouped call vs numpy")
        assert got[0].view(np.uint32)[keep].tobytes() == pose.view(np.uint32)[keep].tobytes(), what + ": a float that no constraint writes changed"
    # a list of one group is rt_skeleton_solve_ik itself
    assert_reads(grouped(sk, pose, groups[:1]), one_by_one(other, pose, groups[:1]), rig + ": one group")
    sk.close(); other.close()


# ---- a crowd: every actor == its skeleton == numpy -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,n_actors", [("chain 4", 1), ("chain 4", 2), ("comb 65", 2), ("comb 65", 300), ("random 257", 2), ("random %d" % CI.LDS, 1)])
def test_crowd_equals_skeletons_equals_numpy(gpu, capi, rig, n_actors):
    """from host and from device memory, with poles and weights and with the chains' own: pose, joints and palette of an actor == a Skeleton
    given set_pose of the actor's prior pose and solve_ik_groups == the numpy statement; every float that no chain writes keeps its bits"""
    parents, groups = RIGS[rig]
    n, flat = len(parents), G.flat(groups)
    ib = S.inverse_binds(n, 1200 + n)
    shared, single = capi.Skeleton(gpu, parents, ib), capi.Skeleton(gpu, parents, ib)
    crowd = capi.Crowd(shared, n_actors)
    assert crowd.ik_chain_groups() == [] and crowd.ik_chains() == 0
    crowd.set_ik_chain_groups(groups)
    assert crowd.ik_chain_groups() == G.sizes_of(groups) and crowd.ik_chains() == len(flat)
    checked = CI.checked_actors(n_actors, shared.info()[1])
    targets, poles, weights = G.values(n_actors, len(flat), 1210 + n)
    prior = CI.prior_poses(parents, n_actors, 1220 + n)
    keep = ~written(parents, flat)
    for brought in (True, False):
        p, w = (poles, weights) if brought else (None, None)
        want = {}
        for a in checked:
            mine = G.actor_groups(groups, targets, p, w, a)
            want[a] = G.solved_and_posed(parents, ib, prior[a], mine)
            assert_reads(grouped(single, prior[a], mine), want[a], "%s, actor %d: the skeleton vs numpy" % (rig, a))
        assert all(G.is_dependent(parents, ib, prior[a], G.actor_groups(groups, targets, p, w, a)) for a in checked), "a case that would pass without the walk between the stages"
        for mem in ("host", "device"):
            what = "%s, %d actors, %s values, %s" % (rig, n_actors, mem, "poles and weights" if brought else "the chains' own")
            crowd.set_poses(prior)
            solve(gpu, crowd, targets, p, w, mem)
            got = reads(crowd, 0, n_actors)
            for a in checked:
                assert_actor(got, a, want[a], what)
            assert got[0].view(np.uint32)[:, keep].tobytes() == prior.view(np.uint32)[:, keep].tobytes(), what + ": a float that no chain writes changed"
    crowd.close(); single.close(); shared.close()


# ---- the shapes a list may take ----------------------------------------------------------------------------------------------------------------
def shapes():
    comb = IK.comb()
    chain8, aims = G.aims_down_a_chain(1301)
    chain4, reaches = G.two_reaches(1302)
    return {"8 x 4": (comb, G.comb_reach_then_aim(1303, (4,) * 8)), "25 and seven": (comb, G.comb_25_and_seven(1304)), "eight aims down a chain": (chain8, aims),
            "two reaches of one chain": (chain4, reaches)}


@pytest.mark.parametrize("shape", ["8 x 4", "25 and seven", "eight aims down a chain", "two reaches of one chain"])
def test_group_shapes(gpu, capi, shape):
    """32 constraints as 8 x 4 and as (25, 1, 1, 1, 1, 1, 1, 1); eight single aims down an eight-joint chain, each reading the W its parent
    got one stage earlier; two groups that write the same joints: a skeleton and three actors of a crowd, from device memory, == numpy"""
    parents, groups = shapes()[shape]
    n, flat, n_actors = len(parents), G.flat(groups), 3
    assert G.validate(G.sizes_of(groups), flat, parents, True)[0] == 0
    ib = S.inverse_binds(n, 1310 + n)
    shared = capi.Skeleton(gpu, parents, ib)
    crowd = capi.Crowd(shared, n_actors)
    crowd.set_ik_chain_groups(groups)
    assert crowd.ik_chain_groups() == G.sizes_of(groups)
    targets, poles, _ = CI.values(n_actors, len(flat), 1320 + n)
    weights = None                                       # (the chains' own: an actor's weight of 0 on its first reach would make the second group the only one)
    prior = CI.prior_poses(parents, n_actors, 1330 + n)
    crowd.set_poses(prior)
    solve(gpu, crowd, targets, poles, weights, "device")
    got = reads(crowd, 0, n_actors)
    for a in range(n_actors):
        mine = G.actor_groups(groups, targets, poles, weights, a)
        assert G.is_dependent(parents, ib, prior[a], mine), shape
        want = G.solved_and_posed(parents, ib, prior[a], mine)
        assert_actor(got, a, want, shape)
        if a == 0:
            assert_reads(grouped(shared, prior[a], mine), want, shape + ": the skeleton")
    crowd.close(); shared.close()


def test_a_list_of_one_group_is_set_ik_chains(gpu, capi):
    """rt_crowd_set_ik_chain_groups with one group == rt_crowd_set_ik_chains with the same list, bit for bit; set_ik_chains says 1, {n}"""
    parents = IK.comb()
    n, n_actors = len(parents), 4
    ib = S.inverse_binds(n, 1340)
    shared = capi.Skeleton(gpu, parents, ib)
    crowd = capi.Crowd(shared, n_actors)
    chains = IK.comb_constraints(32, 1341)
    targets, poles, weights = CI.values(n_actors, 32, 1342)
    prior = CI.prior_poses(parents, n_actors, 1343)
    got = []
    for grouped_call in (False, True):
        if grouped_call:
            crowd.set_ik_chain_groups([chains])
        else:
            crowd.set_ik_chains(chains)
        assert crowd.ik_chain_groups() == [32] and crowd.ik_chains() == 32
        crowd.set_poses(prior)
        solve(gpu, crowd, targets, poles, weights, "device")
        got.append(reads(crowd, 0, n_actors))
    assert_same(got[1], got[0], "one group vs set_ik_chains")
    assert got[0][0].tobytes() != prior.tobytes()
    crowd.close(); shared.close()


# ---- values the host never sees ----------------------------------------------------------------------------------------------------------------
def test_device_values_the_host_never_sees(gpu, capi):
    """a NaN weight in group 0 writes (0, 0, 0, 1) and group 1 solves against the pose that gives; NaN and infinite targets and poles: every
    actor equals the numpy statement, NaNs where it has them; the same NaN weight from host memory is refused by actor and constraint, and
    nothing changes"""
    parents, groups = IK.comb(), G.comb_reach_then_aim(1401)
    n, n_actors, flat = len(parents), 5, G.flat(groups)
    ib = S.inverse_binds(n, 1402)
    shared = capi.Skeleton(gpu, parents, ib)
    crowd = capi.Crowd(shared, n_actors)
    crowd.set_ik_chain_groups(groups)
    targets, poles, weights = CI.values(n_actors, 32, 1403)
    prior = CI.prior_poses(parents, n_actors, 1404)
    weights[1, 0] = weights[1, 5] = NAN                  # reaches of limbs 0 and 5, in group 0; their aims stand in group 1
    weights[2, 31] = NAN                                 # the last lane, in group 1
    targets[3, 0] = (np.nan, 0.5, 0.5); targets[3, 1] = (np.inf, 0.0, 1.0); targets[3, 17] = (-np.inf, np.inf, np.nan); targets[3, 18] = (np.inf, 1.0, 0.0)
    poles[3, 2] = (np.nan, np.nan, np.nan); poles[3, 3] = (np.inf, 1.0, 0.0); poles[3, 19] = (np.nan, 0.0, 1.0); poles[3, 20] = (-np.inf, 0.0, 0.0)
    crowd.set_poses(prior)
    solve(gpu, crowd, targets, poles, weights, "device")
    got = reads(crowd, 0, n_actors)
    for a in range(n_actors):
        assert_actor(got, a, G.solved_and_posed(parents, ib, prior[a], G.actor_groups(groups, targets, poles, weights, a)), "values the host never sees", nans=True)
    for l in (0, 5):                                     # the reach wrote the identity into a and b; the aim of the tip then solved against that pose
        assert got[0][1, [1 + 3 * l, 2 + 3 * l], 3:7].tolist() == [[0, 0, 0, 1]] * 2
        assert got[0][1, 3 + 3 * l, 3:7].tobytes() != prior[1, 3 + 3 * l, 3:7].tobytes() and np.isfinite(got[0][1]).all()
    assert got[0][2, 3 + 3 * 15, 3:7].tolist() == [0, 0, 0, 1]
    with pytest.raises(capi.RtError, match=r"rt_crowd_solve_ik: actor 1: the weight of constraint 0 is NaN") as e:
        crowd.solve_ik(targets, poles, weights)
    assert e.value.code == -1
    late = weights.copy()
    late[1] = 1.0
    with pytest.raises(capi.RtError, match=r"rt_crowd_solve_ik: actor 2: the weight of constraint 31 is NaN"):
        crowd.solve_ik(targets, None, late)
    assert_same(reads(crowd, 0, n_actors), got, "a refused host call")
    crowd.close(); shared.close()


# ---- sequences -------------------------------------------------------------------------------------------------------------------------------
def test_sequences(gpu, capi):
    """two grouped solves in a row; grouped solves interleaved with set_blend_device and set_poses; a grouped list replaced by a plain one
    and back: every actor equals its skeleton given the same sequence"""
    parents, groups = IK.comb(), G.comb_reach_then_aim(1501, (16, 8, 8))
    n, n_actors, flat = len(parents), 4, G.flat(G.comb_reach_then_aim(1501, (16, 8, 8)))
    ib = S.inverse_binds(n, 1502)
    clips = [S.clip(parents, 3, 1503), S.clip(parents, 2, 1504)]
    shared = skeleton_with(capi, gpu, parents, ib, clips)
    skeletons = [skeleton_with(capi, gpu, parents, ib, clips) for _ in range(n_actors)]
    crowd = capi.Crowd(shared, n_actors)
    crowd.set_ik_chain_groups(groups)
    crowd.set_layout([[(a % 2, NAN)] for a in range(n_actors)])
    times = np.array([[0.15 + 0.3 * a] for a in range(n_actors)], F)
    calls = [CI.values(n_actors, 32, 1510 + k) for k in range(3)]
    bufs = [on_device(gpu, times)] + [on_device(gpu, x) for call in calls for x in call]
    crowd.set_blend_device(bufs[0].ptr)                  # back to back on the stream: nothing is read in between
    crowd.solve_ik_device(bufs[1].ptr, bufs[2].ptr, bufs[3].ptr)
    crowd.solve_ik_device(bufs[4].ptr, bufs[5].ptr, bufs[6].ptr)
    for a, sk in enumerate(skeletons):
        sk.set_time(a % 2, float(times[a, 0]))
        for t, p, w in calls[:2]:
            sk.solve_ik_groups(G.actor_groups(groups, t, p, w, a))
    got = reads(crowd, 0, n_actors)
    for a, sk in enumerate(skeletons):
        assert_actor(got, a, reads(sk), "set_blend_device and two grouped solves in a row")
    prior = CI.prior_poses(parents, n_actors, 1520)
    crowd.set_poses(prior)
    crowd.solve_ik(*calls[2])                            # host values: the one upload, then the grouped launch
    crowd.set_blend_device(bufs[0].ptr)
    crowd.solve_ik_device(bufs[7].ptr, None, bufs[9].ptr)
    for a, sk in enumerate(skeletons):
        sk.set_pose(prior[a])
        sk.solve_ik_groups(G.actor_groups(groups, *calls[2], a))
        after_host = reads(sk)
        sk.set_time(a % 2, float(times[a, 0]))
        sk.solve_ik_groups(G.actor_groups(groups, calls[2][0], None, calls[2][2], a))
        assert after_host[0].tobytes() != prior[a].tobytes()
    got = reads(crowd, 0, n_actors)
    for a, sk in enumerate(skeletons):
        assert_actor(got, a, reads(sk), "set_poses, a host solve, set_blend_device, a device solve")
    # a grouped list replaced by a plain one and back
    plain = IK.comb_constraints(7, 1530)
    crowd.set_ik_chains(plain)
    assert crowd.ik_chain_groups() == [7]
    t7, p7, w7 = CI.values(n_actors, 7, 1531)
    solve(gpu, crowd, t7, p7, w7, "device")
    crowd.set_ik_chain_groups(groups)
    assert crowd.ik_chain_groups() == [16, 8, 8] and crowd.ik_chains() == 32
    solve(gpu, crowd, *calls[0], "host")
    for a, sk in enumerate(skeletons):
        sk.solve_ik(CI.constraints_of(plain, t7, p7, w7, a))
        sk.solve_ik_groups(G.actor_groups(groups, *calls[0], a))
    got = reads(crowd, 0, n_actors)
    for a, sk in enumerate(skeletons):
        assert_actor(got, a, reads(sk), "a plain list, then the grouped one again")
    for b in bufs:
        b.close()
    crowd.close(); shared.close()
    for sk in skeletons:
        sk.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_messages(gpu, capi):
    """every refusal with its code and message, in the order the header gives, on both objects; a refused call leaves pose, joints and
    palette byte-identical and the crowd keeps the list it had; a NaN host weight is refused by actor and constraint"""
    parents = np.array([-1, 0, 1, 2, 3, -1, 5], np.int32)
    n, n_actors = len(parents), 3
    ib = S.inverse_binds(n, 1600)
    shared, sk = capi.Skeleton(gpu, parents, ib), capi.Skeleton(gpu, parents, ib)
    crowd = capi.Crowd(shared, n_actors)
    z, x, nan = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), NAN
    reach, aim, other = (IK.TWO_BONE, 3, (0.5, 0.5, 0.2), x, 1.0), (IK.AIM, 3, (0.1, 0.9, 0.3), x, 1.0), (IK.AIM, 6, z, x, 1.0)
    with pytest.raises(capi.RtError, match=r"rt_skeleton_solve_ik_groups: the skeleton has no pose yet \(rt_skeleton_set_pose or rt_skeleton_set_time gives it one\)") as e:
        sk.solve_ik_groups([[reach], [aim]])
    assert e.value.code == -4
    with pytest.raises(capi.RtError, match="rt_skeleton_solve_ik_groups: constraint 1 has kind 2"):     # (an argument's refusal before the state's)
        sk.solve_ik_groups([[reach], [(2, 0, z, x, 1.0)]])
    crowd.set_ik_chain_groups([[reach, other], [aim]])   # (a list needs no pose)
    assert crowd.ik_chain_groups() == [2, 1]
    sk.set_pose(S.pose("unit", parents, 1601))
    prior = CI.prior_poses(parents, n_actors, 1602)
    crowd.set_poses(prior)
    before_sk, before_crowd = reads(sk), reads(crowd, 0, n_actors)
    refusals = [
        ([], r"0 groups: 1 \.\. 8 are supported"),
        ([[other]] * 9, r"9 groups: 1 \.\. 8 are supported"),
        ([[reach], [], [aim]], "group 1 is empty: every group holds at least one constraint"),
        ([[]], "group 0 is empty"),
        ([[other] * 33], r"33 constraints: 1 \.\. 32 are supported"),
        ([[other] * 16, [other] * 16, [other]], r"33 constraints: 1 \.\. 32 are supported"),
        ([[reach], [(2, 0, z, x, 1.0)]], r"constraint 1 has kind 2: RT_IK_TWO_BONE \(0\) or RT_IK_AIM \(1\)"),
        ([[reach, other], [(IK.AIM, 7, z, x, 1.0)]], "constraint 2 names joint 7: the skeleton has 7"),
        ([[reach], [aim], [(IK.TWO_BONE, 6, z, x, 1.0)]], "constraint 2 names joint 6 for the tip of a two-bone chain: it has fewer than two ancestors"),
        ([[reach], [(IK.AIM, 3, z, x, nan)]], "the weight of constraint 1 is NaN"),
        ([[reach, aim]], r"constraints 1 and 0 of group 0 depend on one another: constraint 1 writes joint 3, which constraint 0 reads \(its joint or an ancestor of it\); put the reader in a later group"),
        ([[other], [aim, reach]], r"constraints 2 and 1 of group 1 depend on one another: constraint 2 writes joint 2, which constraint 1 reads"),
        ([[reach], [other], [reach, (IK.AIM, 4, z, x, 1.0)]], r"constraints 2 and 3 of group 2 depend on one another: constraint 2 writes joint 2, which constraint 3 reads"),
        ([[reach, aim], [(IK.AIM, 9, z, x, nan)]], "constraint 2 names joint 9"),       # (every constraint's own refusal before any pair's)
    ]
    for groups, message in refusals:
        want = G.validate(G.sizes_of(groups), G.flat(groups), parents, True)[0]
        assert want in (2, 3, 4, 5, 6, 9, 10, 11), message
        for who, call in (("rt_skeleton_solve_ik_groups", sk.solve_ik_groups), ("rt_crowd_set_ik_chain_groups", crowd.set_ik_chain_groups)):
            with pytest.raises(capi.RtError, match=who + ": " + message) as e:
                call(groups)
            assert e.value.code == -1, message
    assert crowd.ik_chain_groups() == [2, 1] and crowd.ik_chains() == 3, "a refused list leaves the list the crowd had"
    assert_reads(reads(sk), before_sk, "the skeleton after the refusals")
    t = np.full((n_actors, 3, 3), 0.5, F)
    bad = np.ones((n_actors, 3), F)
    bad[2, 1] = nan
    with pytest.raises(capi.RtError, match=r"rt_crowd_solve_ik: actor 2: the weight of constraint 1 is NaN") as e:
        crowd.solve_ik(t, None, bad)
    assert e.value.code == -1
    with pytest.raises(capi.RtError, match="solve_ik: .* of shape"):
        crowd.solve_ik(t[:, :2])                         # (the arrays run over the whole list)
    assert_same(reads(crowd, 0, n_actors), before_crowd, "the crowd after the refusals")
    crowd.solve_ik(t)                                    # ... and the list it kept solves
    want = G.solved_and_posed(parents, ib, prior[1], G.actor_groups([[reach, other], [aim]], t, None, None, 1))
    assert_actor(reads(crowd, 0, n_actors), 1, want, "the list the crowd kept")
    crowd.close(); sk.close(); shared.close()


# ---- the scene -------------------------------------------------------------------------------------------------------------------------------
def test_a_scene_follows_a_grouped_solve(gpu, capi, oracle):
    """instances attached to joints of a crowd's actors and a skinned model posed from one actor's palette: after a grouped solve +
    rt_scene_update every scene array equals a fresh build of the final state; the vertices == skin_cases.skinned over the numpy solve"""
    parents = np.array([-1, 0, 1, 2, 0, 4, -1], np.int32)
    n, n_actors, actor = len(parents), 4, 2
    ib = K.gentle_palette(n, 1700, angle=0.2, spread=0.2)
    clip = gentle_clip(parents, 3, 1701)
    rest, idx, bones, weights, _ = K.case("convex", 257, 4, n, 1702)
    shared = skeleton_with(capi, gpu, parents, ib, [clip])
    crowd = capi.Crowd(shared, n_actors)
    groups = [[(IK.TWO_BONE, 3, (0, 0, 0), (0.0, 0.0, 1.0), 1.0), (IK.AIM, 6, (0, 0, 0), (1.0, 0.0, 0.0), 1.0)], [(IK.AIM, 3, (0, 0, 0), (0.0, 1.0, 0.0), 0.75)]]
    crowd.set_ik_chain_groups(groups)
    start = random_xforms(2 * n_actors + 1, 1703, spread=3.0)
    boxes = gpu_scene(capi, gpu, list(start))
    actors = np.repeat(np.arange(n_actors, dtype=np.uint32), 2)
    joints = np.tile(np.array([3, 6], np.uint32), n_actors)
    local = np.stack(random_xforms(2 * n_actors, 1704, spread=1.0)).astype(F).reshape(-1, 12)
    boxes.attach_crowd(0, crowd, actors, joints, local)
    inst = [(0, None), (0, random_xforms(2, 1705, spread=3.0)[1])]
    skinned, gm = own_scene(capi, gpu, [(rest, idx)], inst)
    gm[0].set_skin(bones, weights, n)
    times = [0.2 + 0.2 * a for a in range(n_actors)]
    crowd.set_times([0] * n_actors, times)
    targets = np.array([[(0.3 - 0.1 * a, 0.2 + 0.05 * a, 0.1), (-0.2, 0.35, 0.15 * a), (0.3, 0.2 * a, 0.4)] for a in range(n_actors)], F)
    solve(gpu, crowd, targets, None, None, "device")
    gm[0].set_bones_from_crowd(crowd, actor)
    boxes.update(); skinned.update()
    got = reads(crowd, 0, n_actors)
    want = [G.solved_and_posed(parents, ib, S.sampled(*clip, times[a]), G.actor_groups(groups, targets, None, None, a)) for a in range(n_actors)]
    for a in range(n_actors):
        assert_actor(got, a, want[a], "the attached crowd")
    final = np.concatenate([np.stack([S.compose(want[actors[k]][1][joints[k]][None], local[k][None])[0] for k in range(2 * n_actors)]), start[-1:]])
    check_equals_build(capi, gpu, oracle, boxes, final, "after a grouped solve")
    new = K.skinned(rest, bones, weights, want[actor][2])
    assert new.tobytes() != rest.tobytes()
    assert_vertices(gm[0].geometry()[0], new, "the skinned model")
    boxes.close()
    close_all(skinned, gm)
    crowd.close(); shared.close()


# ---- the example -------------------------------------------------------------------------------------------------------------------------------
def test_crowd_grasp_example_through_the_cpp_mirror(tmp_path):
    """examples/realtime_crowd_grasp.cpp as the Makefile built it: it exits 0 and writes an image; actor 0 equals a skeleton byte for byte;
    the largest tip-to-target distance is within 4 x the recorded bound of tests/golden/ik_bounds.json times the chain length, the rule of
    test_crowd_reach_example_through_the_cpp_mirror; and the largest aim angle is the one tests/golden/make_ik_group_bounds.py computed on
    the CPU from the numpy statement over the example's own inputs (tests/golden/ik_group_bounds.json), to one unit of the last digit
    printed: the kernel equals the statement bit for bit, so the angle is a fixed number, not a bound"""
    exe = os.path.join(S.ROOT, "dxrexperiments_amd", "lib", "realtime_crowd_grasp")
    out = tmp_path / "out.pfm"
    fixture = json.load(open(os.path.join(S.ROOT, "tests", "golden", "ik_group_bounds.json")))
    r = subprocess.run([exe, "96", "64", str(fixture["frames"]), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    assert "784 boxes on 4 joints of 196 actors, 2 groups of 1 chain per actor solved on the device: %d frames" % fixture["frames"] in r.stdout and "TLAS update" in r.stdout
    assert "actor 0 equals a skeleton given the same pose and solveIKGroups, byte for byte: yes" in r.stdout
    got = re.search(r"largest tip-to-target distance (\S+) of a chain (\S+) long, over 196 actors", r.stdout)
    assert got, r.stdout
    tip, length = (float(v) for v in got.groups())
    bounds = json.load(open(os.path.join(S.ROOT, "tests", "golden", "ik_bounds.json")))
    assert length == 1.5
    assert tip <= 4.0 * bounds["tip_over_chain_length"] * length, r.stdout
    got = re.search(r"largest angle between the aimed axis and the direction to the target (\S+) rad, over 196 actors", r.stdout)
    assert got, r.stdout
    angle, want = float(got.group(1)), fixture["aim_angle"]
    unit = 10.0 ** (math.floor(math.log10(want)) - 3)    # ("%.3e": three digits behind the first)
    print("aim angle %r, the fixture's %r, one unit of the last printed digit %r; tip %r, the fixture's %r" % (angle, want, unit, tip, fixture["tip_to_target"]))
    assert abs(angle - want) <= unit, r.stdout
    raw = out.read_bytes()
    head = b"PF\n96 64\n-1.0\n"
    assert raw.startswith(head)
    image = np.frombuffer(raw[len(head):], "<f4").reshape(64, 96, 3)
    assert image.max() > 0.1 and image.std() > 0.01      # an image, not a constant
