"""Crowds (rt_crowd_*; include/dxr_amd.h "Posed skeletons", crowds): every actor of a crowd is, byte for byte, a skeleton of its own given
the same call -- rt_crowd_set_poses, rt_crowd_set_times, rt_crowd_set_blend -- and the numpy statement of tests/skeleton_cases.py and
tests/skeleton_blend_cases.py; neighbouring actors that differ in every way the definition branches on; the held pose as a base; every
refusal with its message, and nothing changed by it; instances attached to actors' joints against the same scene attached to skeletons and
against a fresh build; skins; lifetimes; the example.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import crowd_cases as CC
import skeleton_blend_cases as B
import skeleton_cases as S
from dxrexperiments_amd import rtypes as T
from test_gpu_model_deform import all_arrays, close_all, own_scene
from test_gpu_model_skin import assert_vertices
from test_gpu_scene_update import arrays, assert_bytes_equal, box_meshes, gpu_models
from test_gpu_skeleton import assert_floats, skinned_model
from util import assert_hits_equal, random_xforms

pytestmark = pytest.mark.gpu

F = np.float32
IDENTITY = np.array(T.IDENTITY_3X4, F).reshape(12)


def skeleton_with(capi, gpu, parents, ib, clips, masks=()):
    sk = capi.Skeleton(gpu, parents, ib)
    assert [sk.add_clip(t, k) for t, k in clips] == list(range(len(clips)))
    assert [sk.add_mask(m) for m in masks] == list(range(len(masks)))
    return sk


def reads(x, first=0, count=None):
    """(pose, joints, palette) of a skeleton, or of actors of a crowd"""
    return (x.pose(), x.joints(), x.palette()) if count is None else (x.pose(first, count), x.joints(first, count), x.palette(first, count))


def assert_actors(crowd, skeletons, what, nans=False):
    """every actor's three reads against the same reads of its skeleton"""
    got = reads(crowd, 0, crowd.n_actors)
    for a, sk in enumerate(skeletons):
        for name, g, w in zip(("pose", "joints", "palette"), got, reads(sk)):
            assert_floats(g[a], w, "%s: actor %d: %s" % (what, a, name), nans)
    return got


def assert_numpy(got, a, parents, ib, trs, what, nans=False):
    Wm, M = S.posed(parents, ib, trs)
    for name, g, w in zip(("pose", "joints", "palette"), got, (np.ascontiguousarray(trs, F), Wm, M)):
        assert_floats(g[a], w, "%s: actor %d: %s vs numpy" % (what, a, name), nans)


# ---- crowd == skeletons ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_actors", CC.ACTORS)
@pytest.mark.parametrize("family,n", CC.RIGS)
def test_crowd_equals_skeletons(gpu, capi, family, n, n_actors):
    """set_poses, set_times and set_blend (3 layers, and 8 on the small rigs): pose, joints and palette of every actor == those of n_actors
    separate skeletons with the same clips and masks, each given that actor's call; and == numpy"""
    parents, ib, clips, masks = CC.rig(family, n)
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    crowd = capi.Crowd(shared, n_actors)
    assert crowd.info() == (shared.h.value, n_actors, n)
    skeletons = [skeleton_with(capi, gpu, parents, ib, clips, masks) for _ in range(n_actors)]
    n_levels = shared.info()[1]
    held = CC.numpy_actors(n_actors, n_levels)
    what = "%s %d, %d actors" % (family, n, n_actors)

    poses = CC.actor_poses(parents, n_actors, seed=3)
    crowd.set_poses(poses)
    for a, sk in enumerate(skeletons):
        sk.set_pose(poses[a])
    got = assert_actors(crowd, skeletons, what + ": set_poses")
    for a in held:
        assert_numpy(got, a, parents, ib, poses[a], what + ": set_poses")

    times = CC.actor_times(clips, n_actors)
    crowd.set_times([c for c, _ in times], [t for _, t in times])
    for sk, (c, t) in zip(skeletons, times):
        sk.set_time(c, t)
    got = assert_actors(crowd, skeletons, what + ": set_times")
    for a in held:
        assert_numpy(got, a, parents, ib, S.sampled(*clips[times[a][0]], times[a][1]), what + ": set_times")

    for n_layers in (3, 8) if n <= 65 else (3,):
        layers = CC.actor_layers(clips, len(masks), n_actors, n_layers, seed=n)
        crowd.set_blend(layers)
        for sk, mine in zip(skeletons, layers):
            sk.set_blend(mine)
        got = assert_actors(crowd, skeletons, what + ": set_blend, %d layers" % n_layers)
        for a in held:
            assert_numpy(got, a, parents, ib, B.blended(clips, masks, layers[a]), what + ": set_blend, %d layers" % n_layers)
    # a sub-range of the actors reads the same bytes
    if n_actors > 2:
        assert crowd.joints(n_actors - 2, 2).tobytes() == got[1][n_actors - 2:].tobytes() and crowd.pose(1, 1).tobytes() == got[0][1:2].tobytes()
    crowd.close()
    for sk in skeletons + [shared]:
        sk.close()


# ---- neighbouring actors that differ -------------------------------------------------------------------------------------------------------
def test_neighbouring_actors_diverge(gpu, capi):
    """65 joints, ten actors side by side: different clips; times before the first key, after the last and exactly on a key; a one-key clip;
    an additive layer beside a replacing one; a masked layer beside an unmasked one; both shortest-path signs; the (0, 0, 0, 1) fallback; and
    one actor on a clip with NaN, inf, zero and negative scales -- with that actor on a clean clip instead, no other actor's bit moves"""
    n = 65
    parents = S.hierarchy("roots", n, 50)
    ib = S.inverse_binds(n, 51)
    a0 = S.pose("unit", parents, 53)
    neg = a0.copy(); neg[:, 3:7] = -a0[:, 3:7]
    zero = a0.copy(); zero[:, 3:7] = 0
    one = np.array([0.0], F)
    three = S.clip(parents, 3, 60)
    poison = S.clip(parents, 2, 61, "nan_inf")
    poison[1][1, :, 7:10] *= np.where(np.arange(n)[:, None] % 3 == 0, F(-1), np.where(np.arange(n)[:, None] % 3 == 1, F(0), F(1))).astype(F)
    clips = [(one, a0[None]), (one, neg[None]), three, S.clip(parents, 2, 62, "raw"), (one, zero[None]), poison]
    masks = B.masks_for(n, 63)
    t3 = three[0]
    actors = [
        [(2, float(t3[0]) - 1.0), (0, 0.0, 0.5, None, B.BLEND)],                        # before the first key; replaces
        [(2, float(t3[2]) + 1.0), (0, 0.0, 0.5, None, B.ADDITIVE)],                     # after the last key; additive where its neighbour replaces
        [(2, float(t3[1])), (3, 0.3, 0.5, 0, B.BLEND)],                                 # exactly on a key; masked
        [(2, float(t3[1])), (3, 0.3, 0.5, None, B.BLEND)],                              # ... and its neighbour is not
        [(0, 0.0), (1, 0.0, 0.25, None, B.BLEND)],                                      # S = -P: d < 0, the layer is turned back
        [(0, 0.0), (0, 0.0, 0.25, None, B.BLEND)],                                      # d > 0
        [(4, 0.0), (4, 0.0, 1.0, None, B.BLEND)],                                       # zero quaternions: (0, 0, 0, 1)
        [(0, 0.0), (3, float("inf"), 1.0, 2, B.ADDITIVE)],                              # a one-key base under a masked additive layer
        [(5, 0.4), (5, 0.9, 0.5, None, B.BLEND)],                                       # NaN, inf, zero and negative scales: this actor only
        [(3, float("-inf")), (2, float(t3[1]), 1.5, 1, B.ADDITIVE)],
    ]
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    crowd = capi.Crowd(shared, len(actors))
    skeletons = [skeleton_with(capi, gpu, parents, ib, clips, masks) for _ in actors]
    crowd.set_blend(actors)
    for sk, mine in zip(skeletons, actors):
        sk.set_blend(mine)
    got = assert_actors(crowd, skeletons, "divergent actors", nans=True)
    for a, mine in enumerate(actors):
        assert_numpy(got, a, parents, ib, B.blended(clips, masks, mine), "divergent actors", nans=True)
    assert not np.isfinite(got[1][8]).all() and all(np.isfinite(got[1][a]).all() for a in range(len(actors)) if a != 8)
    assert got[0][6][:, 3:7].tolist() == [[0, 0, 0, 1]] * n
    clean = [list(mine) for mine in actors]
    clean[8] = [(2, 0.4), (2, 0.9, 0.5, None, B.BLEND)]
    crowd.set_blend(clean)
    again = reads(crowd, 0, len(actors))
    for a in range(len(actors)):
        if a != 8:
            for g, w in zip(again, got):
                assert g[a].tobytes() == w[a].tobytes(), "actor %d moved with actor 8's clip" % a
    # set_times: neighbours on different clips, on a key, beyond both ends, on the one-key clip
    times = [(2, float(t3[0]) - 1.0), (3, 0.2), (2, float(t3[1])), (0, 5.0), (2, float("inf")), (1, float("-inf")), (4, 0.0), (3, 9.0), (5, 0.7), (2, float(t3[2]))]
    crowd.set_times([c for c, _ in times], [t for _, t in times])
    for sk, (c, t) in zip(skeletons, times):
        sk.set_time(c, t)
    assert_actors(crowd, skeletons, "divergent times", nans=True)
    crowd.close()
    for sk in skeletons + [shared]:
        sk.close()


def test_the_held_pose_as_a_base(gpu, capi):
    """set_poses, then set_blend with layer 0 RT_SKELETON_CURRENT_POSE twice in a row: each actor starts from its OWN held pose, as its
    skeleton does; the pose count moves once per call (an attached scene sees one change)"""
    n, n_actors = 65, 7
    parents, ib, clips, masks = CC.rig("random", n, seed=9)
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    crowd = capi.Crowd(shared, n_actors)
    skeletons = [skeleton_with(capi, gpu, parents, ib, clips, masks) for _ in range(n_actors)]
    poses = CC.actor_poses(parents, n_actors, seed=11)
    crowd.set_poses(poses)
    for sk, trs in zip(skeletons, poses):
        sk.set_pose(trs)
    current = [p for p in poses]
    for step in range(2):
        layers = [[(None, 0.0), (a % 3, 0.3 + 0.1 * a + step, 0.5, (a % 4) - 1 if a % 4 else None, (a + step) % 2)] for a in range(n_actors)]
        crowd.set_blend(layers)
        for sk, mine in zip(skeletons, layers):
            sk.set_blend(mine)
        got = assert_actors(crowd, skeletons, "current pose, step %d" % step)
        for a in range(n_actors):
            current[a] = B.blended(clips, masks, layers[a], current[a])
            assert_numpy(got, a, parents, ib, current[a], "current pose, step %d" % step)
    assert len({got[0][a].tobytes() for a in range(n_actors)}) == n_actors
    crowd.close()
    for sk in skeletons + [shared]:
        sk.close()


def test_clips_added_later_are_seen(gpu, capi):
    """clips and masks added to the skeleton after the crowd was made are there for the next call"""
    parents, ib, clips, masks = CC.rig("random", 9, seed=4)
    shared = skeleton_with(capi, gpu, parents, ib, clips[:1])
    crowd = capi.Crowd(shared, 2)
    with pytest.raises(capi.RtError, match=r"actor 1: clip 1: the skeleton has 1") as e:
        crowd.set_times([0, 1], [0.0, 0.0])
    assert e.value.code == -4
    shared.add_clip(*clips[1]); shared.add_mask(masks[0])
    layers = [[(0, 0.0), (1, 0.7, 0.5, 0, B.BLEND)], [(1, 0.2), (0, 0.0, 0.25, None, B.ADDITIVE)]]
    crowd.set_blend(layers)
    got = reads(crowd, 0, 2)
    for a in range(2):
        assert_numpy(got, a, parents, ib, B.blended(clips, masks, layers[a]), "a clip and a mask added later")
    crowd.set_times([1, 0], [0.2, 0.0])
    assert_numpy(reads(crowd, 0, 2), 0, parents, ib, S.sampled(*clips[1], 0.2), "a clip added later")
    crowd.close(); shared.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_messages(gpu, capi):
    """every refusal, with its code and message; the refused call leaves every read unchanged"""
    lib = capi.lib()
    n, n_actors = 9, 4
    parents, ib, clips, masks = CC.rig("random", n, seed=2)
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    with pytest.raises(capi.RtError, match="at least one actor") as e:
        capi.Crowd(shared, 0)
    assert e.value.code == -1
    big = capi.Skeleton(gpu, S.hierarchy("random", CC.LDS + 1, 1), S.inverse_binds(CC.LDS + 1, 2))
    with pytest.raises(capi.RtError, match=r"a skeleton of %d joints: a crowd poses rigs of up to %d" % (CC.LDS + 1, CC.LDS)) as e:
        capi.Crowd(big, 2)
    assert e.value.code == -6
    big.close()
    lib.rt_debug_set_alloc_limit(48 * n * 1000 - 1)                 # pose fits, joints do not
    with pytest.raises(capi.RtError, match="hipMalloc") as e:
        capi.Crowd(shared, 1000)
    assert e.value.code == -5
    lib.rt_debug_set_alloc_limit(0)
    crowd = capi.Crowd(shared, n_actors)
    # an unposed crowd
    out = np.zeros((n_actors, n, 12), F)
    h = C.c_void_p()
    for rc in (lib.rt_crowd_read_pose(crowd.h, 0, 1, out.ctypes.data_as(C.c_void_p)), lib.rt_crowd_read_joints(crowd.h, 0, 1, out.ctypes.data_as(C.c_void_p)),
               lib.rt_crowd_read_palette(crowd.h, 0, 1, out.ctypes.data_as(C.c_void_p)), lib.rt_crowd_get_joints_device_ptr(crowd.h, C.byref(h)),
               lib.rt_crowd_get_palette_device_ptr(crowd.h, C.byref(h))):
        assert rc == -4 and b"the crowd has no pose yet (rt_crowd_set_poses" in lib.rt_last_error()
    ok = [(0, 0.0), (1, 0.5, 0.5, None, B.BLEND)]
    with pytest.raises(capi.RtError, match=r"actor 2: layer 0 names RT_SKELETON_CURRENT_POSE: the crowd has no pose yet \(rt_crowd_set_poses") as e:
        crowd.set_blend([ok, ok, [(None, 0.0), ok[1]], ok])
    assert e.value.code == -4
    model, *_ = skinned_model(capi, gpu, n)
    with pytest.raises(capi.RtError, match="rt_model_set_bones_from_crowd: the crowd has no pose yet") as e:
        model.set_bones_from_crowd(crowd, 0)
    assert e.value.code == -4
    crowd.set_times([0, 1, 2, 1], [0.0, 0.5, 0.2, 9.0])
    before = reads(crowd, 0, n_actors)

    def unchanged(what):
        for g, w in zip(reads(crowd, 0, n_actors), before):
            assert g.tobytes() == w.tobytes(), what

    nan = float("nan")
    for layers, code, message in (
            ([ok, [(0, 0.0), (1, 0.5, 0.5, None, 2)], ok, ok], -1, r"actor 1: layer 1 has mode 2"),
            ([ok, ok, ok, [(0, 0.0, 1.0, None, B.ADDITIVE), ok[1]]], -1, r"actor 3: layer 0 is additive"),
            ([[(0, 0.0), (None, 0.0)], ok, ok, ok], -1, r"actor 0: layer 1 names RT_SKELETON_CURRENT_POSE: only layer 0 may"),
            ([ok, ok, [(0, 0.0), (1, nan)], ok], -1, r"actor 2: the time of layer 1 is NaN"),
            ([[(7, 0.0), ok[1]], ok, ok, [(0, nan), ok[1]]], -1, r"actor 3: the time of layer 0 is NaN"),          # arguments before state, across actors
            ([ok, [(3, 0.0), ok[1]], ok, [(9, 0.0), ok[1]]], -4, r"actor 1: layer 0 names clip 3: the skeleton has 3"),
            ([ok, ok, ok, [(0, 0.0), (1, 0.5, 0.5, 3, B.BLEND)]], -4, r"actor 3: layer 1 names mask 3: the skeleton has 3")):
        with pytest.raises(capi.RtError, match=message) as e:
            crowd.set_blend(layers)
        assert e.value.code == code, message
        unchanged(message)
    for n_layers in (0, 9):
        a = np.zeros((n_actors, n_layers), T.SKELETON_LAYER)
        assert lib.rt_crowd_set_blend(crowd.h, n_layers, a.ctypes.data_as(C.c_void_p)) == -1 and b"layers: 1 .. 8 are supported" in lib.rt_last_error()
    with pytest.raises(capi.RtError, match=r"actor 2: the time is NaN") as e:
        crowd.set_times([9, 0, 0, 0], [0.0, 0.0, nan, 0.0])
    assert e.value.code == -1
    with pytest.raises(capi.RtError, match=r"actor 0: clip 9: the skeleton has 3") as e:
        crowd.set_times([9, 0, 0, 0], [0.0, 0.0, 0.0, 0.0])
    assert e.value.code == -4
    unchanged("set_times refused")
    # actors out of range
    for fn in (lib.rt_crowd_read_pose, lib.rt_crowd_read_joints, lib.rt_crowd_read_palette):
        assert fn(crowd.h, 3, 2, out.ctypes.data_as(C.c_void_p)) == -1 and b"the crowd has 4" in lib.rt_last_error()
        assert fn(crowd.h, 5, 0, out.ctypes.data_as(C.c_void_p)) == -1
    with pytest.raises(capi.RtError, match=r"actor 4: the crowd has 4") as e:
        model.set_bones_from_crowd(crowd, 4)
    assert e.value.code == -1
    other, *_ = skinned_model(capi, gpu, n + 1)
    with pytest.raises(capi.RtError, match=r"a skin of %d bones and a crowd of %d joints" % (n + 1, n)) as e:
        other.set_bones_from_crowd(crowd, 0)
    assert e.value.code == -4
    plain = capi.Model(gpu, *box_meshes()[0])
    with pytest.raises(capi.RtError, match=r"the model has no skin \(rt_model_set_skin") as e:
        plain.set_bones_from_crowd(crowd, 0)
    assert e.value.code == -4
    # OOM when the table must grow: nothing changes
    lib.rt_debug_set_alloc_limit(64)
    with pytest.raises(capi.RtError, match="hipMalloc") as e:
        crowd.set_blend([ok + [ok[1]] * 6] * n_actors)
    assert e.value.code == -5
    lib.rt_debug_set_alloc_limit(0)
    unchanged("the table could not grow")
    # cleared clips: a layer that names a clip is a state error
    shared.clear_clips()
    with pytest.raises(capi.RtError, match=r"actor 0: layer 0 names clip 0: the skeleton has 0") as e:
        crowd.set_blend([ok] * n_actors)
    assert e.value.code == -4
    with pytest.raises(capi.RtError, match=r"actor 0: clip 0: the skeleton has 0") as e:
        crowd.set_times([0] * n_actors, [0.0] * n_actors)
    assert e.value.code == -4
    unchanged("cleared clips")
    crowd.set_blend([[(None, 0.0)]] * n_actors)             # the held pose needs no clip
    unchanged("the held pose, posed again")
    # different contexts
    ctx2 = capi.Context(0)
    m2, *_ = skinned_model(capi, ctx2, n)
    with pytest.raises(capi.RtError, match="the model and the crowd belong to different contexts") as e:
        m2.set_bones_from_crowd(crowd, 0)
    assert e.value.code == -4
    sc2 = capi.Scene(ctx2)
    sc2.add_model(m2)
    with pytest.raises(capi.RtError, match="the scene and the crowd belong to different contexts") as e:
        sc2.attach_crowd(0, crowd, [0], [0])
    assert e.value.code == -4
    sc2.close(); m2.close(); ctx2.close()
    for x in (model, other, plain, crowd, shared):
        x.close()


# ---- attachments ---------------------------------------------------------------------------------------------------------------------------
def scene_of(capi, gpu, xf, build=True):
    gm = gpu_models(capi, gpu)
    sc = capi.Scene(gpu)
    for k, x in enumerate(xf):
        sc.add_model(gm[k % len(gm)], x)
    if build:
        sc.build()
    return sc


def rays(n, seed):
    r = np.random.default_rng(seed)
    o = np.zeros((n, 4), F); d = np.zeros((n, 4), F)
    o[:, :3] = r.uniform(-12, 12, (n, 3))
    v = -o[:, :3] + r.uniform(-3, 3, (n, 3))
    d[:, :3] = v / np.linalg.norm(v, axis=1, keepdims=True)
    d[:, 3] = 1e30
    return o, d


RAYS = rays(384, 5)


@pytest.mark.parametrize("with_locals", (True, False))
def test_attached_to_a_crowd_equals_attached_to_skeletons(gpu, capi, with_locals):
    """13 instances attached to (actor, joint) pairs of a crowd of 5: after pose + update, and after a second pose, the scene == the same scene
    attached to five separate skeletons == a fresh build with the composed transforms, array for array; 384 rays agree; the transform setters
    are refused over a crowd-attached instance; detaching keeps the last transform"""
    n, n_actors, n_inst = 9, 5, 13
    parents, ib, clips, masks = CC.rig("random", n, seed=8)
    for t, keys in clips:
        keys[:, :, 0:3] *= F(4.0)                          # (apart enough for a tree with some depth)
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    crowd = capi.Crowd(shared, n_actors)
    skeletons = [skeleton_with(capi, gpu, parents, ib, clips, masks) for _ in range(n_actors)]
    r = np.random.default_rng(3)
    actors = r.integers(0, n_actors, n_inst).astype(np.uint32)
    actors[:2] = (0, n_actors - 1)
    joints = r.integers(0, n, n_inst).astype(np.uint32)
    local = np.stack(random_xforms(n_inst, 21, spread=3.0)).astype(F).reshape(n_inst, 12) if with_locals else None
    start = random_xforms(n_inst, 3, spread=6.0)
    a, b = scene_of(capi, gpu, start), scene_of(capi, gpu, start)
    a.attach_crowd(0, crowd, actors, joints, local)
    assert a.attachment(0) is None and a.crowd_attachment(1) == (crowd, n_actors - 1, int(joints[1])) and b.crowd_attachment(0) is None
    for k in range(n_inst):
        b.attach(k, skeletons[actors[k]], joints[k:k + 1], None if local is None else local[k:k + 1])
    with pytest.raises(capi.RtError, match=r"instance 0 is attached to a crowd that has no pose yet \(rt_crowd_set_poses") as e:
        a.update()
    assert e.value.code == -4
    for step in range(2):
        times = [(x % 3, 0.2 + 0.37 * x + step) for x in range(n_actors)]
        crowd.set_times([c for c, _ in times], [t for _, t in times])
        for sk, (c, t) in zip(skeletons, times):
            sk.set_time(c, t)
        a.update(); b.update()
        what = "locals %s, pose %d" % (with_locals, step)
        W = crowd.joints()
        want = np.stack([W[actors[k], joints[k]] if local is None else S.compose(W[actors[k], joints[k]][None], local[k][None])[0] for k in range(n_inst)])
        assert a.transforms().tobytes() == want.tobytes() == b.transforms().tobytes(), what
        got = arrays(a, n_inst)
        assert_bytes_equal(got, arrays(b, n_inst), what + " vs the scene attached to skeletons")
        fresh = scene_of(capi, gpu, list(want))
        assert_bytes_equal(got, arrays(fresh, n_inst), what + " vs a fresh build")
        assert_hits_equal(a.trace(*RAYS), b.trace(*RAYS), what + ": rays vs the scene attached to skeletons")
        assert_hits_equal(a.trace(*RAYS), fresh.trace(*RAYS), what + ": rays vs a fresh build")
        fresh.close()
    assert (a.trace(*RAYS)["inst"] != T.RT_NO_HIT).sum() > 20
    for call in (lambda: a.set_transform(2, None), lambda: a.set_transforms(1, [None, None]), lambda: a.set_transforms_device(0, crowd.joints_ptr(), 1)):
        with pytest.raises(capi.RtError, match=r"is attached to joint \d+ of actor \d+ of a crowd, which gives it its transform \(rt_scene_detach_instances") as e:
            call()
        assert e.value.code == -4
    a.detach(0, n_inst)
    assert a.crowd_attachment(1) is None and a.transforms().tobytes() == want.tobytes(), "detaching keeps the last transform"
    crowd.set_times([0] * n_actors, [0.0] * n_actors)
    a.update()
    assert a.transforms().tobytes() == want.tobytes(), "a detached instance follows no pose"
    a.close(); b.close(); crowd.close()
    for sk in skeletons + [shared]:
        sk.close()


def test_one_mixed_scene(gpu, capi):
    """one update over a host-set, a device-set, a skeleton-attached and crowd-attached instances == a fresh build of that state; entries
    out of range are refused and nothing changes"""
    n, n_actors = 9, 3
    parents, ib, clips, masks = CC.rig("random", n, seed=12)
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    crowd = capi.Crowd(shared, n_actors)
    single = skeleton_with(capi, gpu, parents, ib, clips, masks)
    start = random_xforms(6, 4, spread=6.0)
    sc = scene_of(capi, gpu, start)
    with pytest.raises(capi.RtError, match=r"entry 1 names actor 3: the crowd has 3") as e:
        sc.attach_crowd(3, crowd, [0, 3], [1, 1])
    assert e.value.code == -1
    with pytest.raises(capi.RtError, match=r"entry 0 names joint 9: the crowd has 9") as e:
        sc.attach_crowd(3, crowd, [0, 1], [9, 1])
    assert e.value.code == -1
    assert sc.crowd_attachment(3) is None and sc.crowd_attachment(4) is None
    sc.attach_crowd(3, crowd, [2, 0, 1], [1, 8, 4])
    sc.attach(2, single, [5])
    host = random_xforms(1, 30, spread=4.0)[0]
    dev = np.ascontiguousarray(random_xforms(1, 31, spread=4.0)[0], F).reshape(12)
    buf = gpu.upload(dev)
    sc.set_transform(0, host)
    sc.set_transforms_device(1, buf.ptr, 1)
    crowd.set_times([0, 1, 2], [0.0, 0.8, 0.3])
    single.set_time(1, 0.6)
    sc.update()
    W, Ws = crowd.joints(), single.joints()
    want = np.stack([np.asarray(host, F).reshape(12), dev, Ws[5], W[2, 1], W[0, 8], W[1, 4]])
    assert sc.transforms().tobytes() == want.tobytes()
    fresh = scene_of(capi, gpu, list(want))
    assert_bytes_equal(arrays(sc, 6), arrays(fresh, 6), "a mixed update vs a fresh build")
    assert sc.attachment(2) == (single, 5) and sc.attachment(3) is None and sc.crowd_attachment(2) is None and sc.crowd_attachment(4) == (crowd, 0, 8)
    fresh.close(); sc.close(); buf.close(); crowd.close(); single.close(); shared.close()


# ---- skins -----------------------------------------------------------------------------------------------------------------------------
def test_bones_from_a_crowd(gpu, capi):
    """set_bones_from_crowd(crowd, a) + update gives the vertices and the BLAS of set_bones_from(actor a's skeleton): the first and the
    last actor; and the crowd is destroyed right after the call"""
    n, n_actors = 7, 6
    parents = S.hierarchy("random", n, 110)
    import skin_cases as K
    from test_gpu_skeleton import gentle_clip
    ib = K.gentle_palette(n, 111, angle=0.2, spread=0.2)
    clip = gentle_clip(parents, 3, 112)
    rest, idx, bones, weights, _ = K.case("convex", 257, 4, n, 113)
    shared = skeleton_with(capi, gpu, parents, ib, [clip])
    times = [0.1 + 0.25 * a for a in range(n_actors)]
    inst = [(0, None)]
    for actor in (0, n_actors - 1):
        crowd = capi.Crowd(shared, n_actors)
        crowd.set_times([0] * n_actors, times)
        single = skeleton_with(capi, gpu, parents, ib, [clip])
        single.set_time(0, times[actor])
        got_sc, got_m = own_scene(capi, gpu, [(rest, idx)], inst)
        want_sc, want_m = own_scene(capi, gpu, [(rest, idx)], inst)
        got_m[0].set_skin(bones, weights, n); want_m[0].set_skin(bones, weights, n)
        got_m[0].set_bones_from_crowd(crowd, actor)
        crowd.close()                                      # (joins the stream: the skin kernel already queued reads a live palette)
        want_m[0].set_bones_from(single)
        got_sc.update(); want_sc.update()
        _, M = S.posed(parents, ib, S.sampled(*clip, times[actor]))
        assert_vertices(got_m[0].geometry()[0], K.skinned(rest, bones, weights, M), "actor %d" % actor)
        assert_bytes_equal(all_arrays(got_sc, got_m, inst), all_arrays(want_sc, want_m, inst), "actor %d: crowd vs skeleton" % actor)
        close_all(got_sc, got_m); close_all(want_sc, want_m); single.close()
    shared.close()


# ---- lifetime --------------------------------------------------------------------------------------------------------------------------
def test_lifetimes(gpu, capi):
    """the skeleton destroyed while the crowd lives: the crowd still poses; the crowd destroyed after attaching: the scene holds it, the
    instances are posed by the update and keep their transform"""
    n = 9
    parents, ib, clips, masks = CC.rig("random", n, seed=14)
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    crowd = capi.Crowd(shared, 3)
    shared.close()
    crowd.set_times([0, 1, 2], [0.0, 0.7, 0.3])
    got = reads(crowd, 0, 3)
    for a, (c, t) in enumerate(((0, 0.0), (1, 0.7), (2, 0.3))):
        assert_numpy(got, a, parents, ib, S.sampled(*clips[c], t), "the skeleton's handle is gone")
    sc = scene_of(capi, gpu, random_xforms(2, 6, spread=5.0))
    sc.attach_crowd(0, crowd, [2, 1], [3, 4])
    W = crowd.joints()
    lib = capi.lib()
    assert lib.rt_crowd_destroy(crowd.h) == 0              # (the wrapper's reference; the scene's remains)
    crowd.h = None
    sc.update()
    assert sc.transforms().tobytes() == np.stack([W[2, 3], W[1, 4]]).tobytes()
    sc._crowds.clear()
    sc.close()


# ---- the example -----------------------------------------------------------------------------------------------------------------------
def test_crowd_example_through_the_cpp_mirror(tmp_path):
    """examples/realtime_crowd.cpp: RtSkeleton::create + addClip + RtCrowd::create + RtScene::attach(crowd) once, one RtCrowd::setTimes and
    one RtScene::update per frame, end to end; driven by one skeleton per actor instead, the frame is the same frame"""
    exe = os.path.join(S.ROOT, "dxrexperiments_amd", "lib", "realtime_crowd")
    images = []
    for frames, how in ((1, "crowd"), (3, "crowd"), (3, "skeletons")):
        out = tmp_path / ("out%d%s.pfm" % (frames, how))
        r = subprocess.run([exe, "96", "64", str(frames), str(out)] + (["skeletons"] if how == "skeletons" else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "actors, posed as %s: %d frames" % ("a crowd" if how == "crowd" else "skeletons", frames) in r.stdout and "TLAS update" in r.stdout
        raw = out.read_bytes()
        head = b"PF\n96 64\n-1.0\n"
        assert raw.startswith(head)
        images.append(np.frombuffer(raw[len(head):], "<f4").reshape(64, 96, 3))
    assert images[0].max() > 0.1 and images[0].std() > 0.01            # an image, not a constant
    assert not np.array_equal(images[0], images[1]), "the crowd did not move"
    assert np.array_equal(images[1], images[2]), "a crowd and its skeletons give different frames"
