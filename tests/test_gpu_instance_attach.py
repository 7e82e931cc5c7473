"""Instance transforms from the device (include/dxr_amd.h "Attached instances"): rt_scene_set_instance_transforms_mem(RT_MEM_DEVICE),
rt_scene_get_instance_transforms and instances attached to the joints of a posed skeleton (rt_scene_attach_instances).  The composition is its
definition, bit for bit against the numpy restatement of tests/skeleton_cases.py; a scene after attach + pose + update is, array for array, the
scene a fresh build gives for the numpy transforms, and the oracle's; a pose alone touches no scene; the device setter gives the bytes the host
setter gives; keyed rigid animation end to end through trace and both pipelines; every refusal with its message; lifetimes; a seeded sequence of
edits against a small model of the state; the example through the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import skeleton_cases as K
from dxrexperiments_amd import rtypes as T, scenes
from skeleton_cases import clip, compose, hierarchy, pose, posed, sample_times, sampled
from test_gpu_batch import frames_of
from test_gpu_pipeline import make_gpu_pipeline, make_oracle_scene
from test_gpu_realtime_denoise import realtime_pair
from test_gpu_scene_update import arrays, assert_bytes_equal, assert_equals_oracle, box_meshes, gpu_models, light_scene, oracle_frames
from util import assert_hits_equal, primary_rays, random_xforms, triangle_soup

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = K.ROOT
IDENTITY = np.array(T.IDENTITY_3X4, F).reshape(12)
_cache = {}


def same_bits(a, b):
    """float32 arrays equal bit for bit -- the signs of zero count -- with NaNs compared as NaNs"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def rows(xf):
    """a list of transforms (None: identity) as float32[n, 12]"""
    return np.stack([IDENTITY if x is None else np.asarray(x, F).reshape(12) for x in xf])


def random_locals(n, seed):
    return rows(random_xforms(n, seed, spread=3.0))


def skeleton_of(capi, gpu, parents):
    return capi.Skeleton(gpu, parents, K.inverse_binds(len(parents), 5))


def transforms_of(W, joints, local):
    """T = W_joint o local, or W_joint itself"""
    return W[joints].copy() if local is None else compose(W[joints], local)


def gpu_scene(capi, gpu, xf, masks=None, models=None, build=True):
    gm = gpu_models(capi, gpu) if models is None else models
    sc = capi.Scene(gpu)
    for k, x in enumerate(xf):
        sc.add_model(gm[k % len(gm)], x)
    if masks is not None:
        sc.set_masks(0, masks)
    if build:
        sc.build()
    return sc


def oracle_scene(oracle, xf, meshes=None):
    meshes = box_meshes() if meshes is None else meshes
    return make_oracle_scene(oracle, meshes, [(k % len(meshes), x) for k, x in enumerate(xf)])


def check_equals_build(capi, gpu, oracle, sc, final, what, masks=None):
    """sc against a fresh GPU scene of `final` (float32[n, 12]) and, with nothing hidden, the oracle's"""
    n = len(final)
    assert same_bits(sc.transforms(), final), what + ": the transforms the scene holds"
    got = arrays(sc, n)
    fresh = gpu_scene(capi, gpu, list(final), masks)
    assert_bytes_equal(got, arrays(fresh, n), what + " vs a fresh GPU build")
    fresh.close()
    osc = oracle_scene(oracle, list(final))
    if masks is None:
        assert_equals_oracle(got, osc, n, what)
    else:
        for k in range(n):                              # the records are those of the full list, hidden instances included
            ob, oi = osc.instance_info(k)
            assert np.array_equal(got["invs"][k], oi, equal_nan=True) and np.array_equal(got["boxes"][k], ob, equal_nan=True), (what, k)
    return got


# ---- the composition is its definition -------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 63, 64, 65, 257)
N_COMP, J_COMP = 257, 65


def composition_scene(capi, gpu):
    """257 instances of one tiny mesh, built once: what is compared is the twelve floats, whatever they do to a box"""
    if "comp" not in _cache:
        m = capi.Model(gpu, *triangle_soup(4, seed=3, extent=1.0, size=0.5))
        _cache["comp"] = gpu_scene(capi, gpu, [None] * N_COMP, models=[m])
    return _cache["comp"]


@pytest.mark.parametrize("with_locals", (True, False))
@pytest.mark.parametrize("pose_family", ("unit", "raw", "neg_zero", "nan_inf"))
@pytest.mark.parametrize("family", ("chain", "star", "random", "roots"))
def test_composition_is_its_definition(gpu, capi, family, pose_family, with_locals):
    """1, 2, 63, 64, 65 and 257 attached instances (a lane, less than a wave, a wave, a wave and one, more than a block), joints picked at random
    with repeats: after update Scene.transforms() == compose(W[joints], local) -- or W[joints] -- bit for bit, NaNs as NaNs, the others as
    they were"""
    sc = composition_scene(capi, gpu)
    parents = hierarchy(family, J_COMP, seed=2)
    sk = skeleton_of(capi, gpu, parents)
    for count in COUNTS:
        r = np.random.default_rng(count)
        first = 0 if count == N_COMP else int(r.integers(0, N_COMP - count))
        joints = r.integers(0, J_COMP, count).astype(np.uint32)
        local = random_locals(count, 7 + count) if with_locals else None
        if with_locals and count > 2:
            local[1] = IDENTITY                           # (multiplied all the same)
        before = sc.transforms()
        trs = pose(pose_family, parents, seed=11 + count)
        sc.attach(first, sk, joints, local)
        assert same_bits(sc.transforms(), before), "attaching changes no stored transform"
        sk.set_pose(trs)
        sc.update()
        W, _ = posed(parents, K.inverse_binds(J_COMP, 5), trs)
        assert same_bits(sk.joints(), W)
        want = before.copy()
        want[first:first + count] = transforms_of(W, joints, local)
        got = sc.transforms()
        assert same_bits(got, want), (family, pose_family, with_locals, count, int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()))
        if pose_family == "nan_inf":
            assert not np.isfinite(want[first:first + count]).all() or count < 8
        sc.detach(first, count)
        assert same_bits(sc.transforms(), want), "detaching keeps the last transform"
        assert sc.attachment(first) is None
        # back to finite ground for the next count (and the next test): the scene is shared
        sc.set_transforms(first, [None] * count)
        sc.update()
    sk.close()


# ---- update == build ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_locals", (True, False))
@pytest.mark.parametrize("family,n", (("chain", 13), ("star", 13), ("random", 65), ("roots", 13)))
def test_attached_update_equals_build(gpu, capi, oracle, family, n, with_locals):
    """attach every instance, pose, update: every array == a fresh scene built from the numpy transforms, == the oracle's; a second pose on top
    (-0 among its components), and a build instead of an update"""
    parents = hierarchy(family, 9, seed=4)
    sk = skeleton_of(capi, gpu, parents)
    r = np.random.default_rng(n)
    joints = r.integers(0, 9, n).astype(np.uint32)
    local = random_locals(n, 21) if with_locals else None
    sc = gpu_scene(capi, gpu, random_xforms(n, 3, spread=6.0))
    sc.attach(0, sk, joints, local)
    for step, (fam, how) in enumerate((("unit", "update"), ("neg_zero", "update"), ("raw", "build"))):
        trs = pose(fam, parents, seed=30 + step)
        trs[:, 0:3] *= F(4.0)                             # (apart enough for a tree with some depth)
        sk.set_pose(trs)
        getattr(sc, how)()
        W, _ = posed(parents, K.inverse_binds(9, 5), trs)
        check_equals_build(capi, gpu, oracle, sc, transforms_of(W, joints, local), "%s n=%d step %d" % (family, n, step))
    sc.close(); sk.close()


def test_one_mixed_update(gpu, capi, oracle):
    """one update: instances 0-4 attached, 5-6 set from the host, 7-9 from device memory, 10-11 hidden by their masks, 12's model deformed:
    == a fresh build of that state, with one bump of the generation"""
    n = 13
    meshes = box_meshes()
    gm = gpu_models(capi, gpu)
    own = capi.Model(gpu, *meshes[0])                     # (instance 12's own: the shared models stay as they are)
    start = random_xforms(n, 3, spread=6.0)
    sc = capi.Scene(gpu)
    for k in range(n):
        sc.add_model(own if k == 12 else gm[k % 2], start[k])
    sc.build()
    parents = hierarchy("random", 9, seed=4)
    sk = skeleton_of(capi, gpu, parents)
    trs = pose("unit", parents, seed=8)
    trs[:, 0:3] *= F(4.0)
    sk.set_pose(trs)
    W, _ = posed(parents, K.inverse_binds(9, 5), trs)
    joints = np.array([3, 3, 0, 8, 5], np.uint32)
    local = random_locals(5, 9)
    new = rows(random_xforms(n, 77, spread=6.0))
    final = rows(start)
    final[0:5] = transforms_of(W, joints, local)
    final[5:10] = new[5:10]
    masks = np.full(n, 0xFF, np.uint8)
    masks[10:12] = 0
    sc.attach(0, sk, joints, local)
    sc.set_transforms(5, new[5:7])
    dev = gpu.upload(new[7:10])
    sc.set_transforms_device(7, dev.ptr, 3)
    sc.set_masks(0, masks)
    v = meshes[0][0].copy()
    v["position"] = v["position"] * F(1.25) + F(0.125)
    own.set_positions(v["position"])
    p = capi.Pipeline(gpu)                                # (a pipeline sees every bump of the generation: count_work refuses after one)
    with pytest.raises(capi.RtError, match="pending"):
        sc.instance_info(0)
    sc.update()
    assert same_bits(sc.transforms(), final)
    got = arrays(sc, n)
    fresh = capi.Scene(gpu)
    moved = capi.Model(gpu, v, meshes[0][1])
    for k in range(n):
        fresh.add_model(moved if k == 12 else gm[k % 2], final[k])
    fresh.set_masks(0, masks)
    fresh.build()
    assert_bytes_equal(got, arrays(fresh, n), "the mixed update vs a fresh GPU build")
    osc = make_oracle_scene(oracle, [meshes[0], meshes[1], (v, meshes[0][1])], [(2 if k == 12 else k % 2, final[k]) for k in range(n)])
    for k in range(n):
        ob, oi = osc.instance_info(k)
        assert np.array_equal(got["invs"][k], oi, equal_nan=True) and np.array_equal(got["boxes"][k], ob, equal_nan=True), k
    # nothing pending now: an update changes nothing
    sc.update()
    assert_bytes_equal(arrays(sc, n), got, "an update with nothing pending")
    p.close(); fresh.close(); sc.close(); sk.close(); dev.close()


def test_identity_pose_flips_a_single_instance_scene(gpu, capi, oracle):
    """n = 1, no local matrix: a pose that is the identity makes the scene single-level (rays walk the BLAS), another makes it two-level, and
    back: arrays and the canonical walk's counters those of a fresh scene with that transform"""
    sk = capi.Skeleton(gpu, np.array([-1], np.int32), IDENTITY.reshape(1, 12))
    sc = gpu_scene(capi, gpu, [random_xforms(1, 9, spread=2.0)[0]])
    sc.attach(0, sk, [0])
    unit = np.array([[0, 0, 0, 0, 0, 0, 1, 1, 1, 1]], F)
    moved = pose("unit", np.array([-1], np.int32), seed=6)
    mesh = box_meshes()[0]
    lo, hi = mesh[0]["position"].min(0) - 3, mesh[0]["position"].max(0) + 3
    from util import random_rays
    O, D = random_rays(2000, 5, lo, hi)
    for step, trs in enumerate((unit, moved, unit)):
        sk.set_pose(trs)
        sc.update()
        want = K.local_of(trs)
        assert same_bits(sc.transforms(), want)
        fresh = gpu_scene(capi, gpu, [want[0]])
        assert_bytes_equal(arrays(sc, 1), arrays(fresh, 1), "n = 1 step %d" % step)
        a, b = sc.trace(O, D, canonical=True), fresh.trace(O, D, canonical=True)
        assert_hits_equal(a, b, "n = 1 step %d" % step)
        assert np.array_equal(a["nodes"], b["nodes"]) and np.array_equal(a["tris"], b["tris"])
        assert_hits_equal(sc.trace(O, D), oracle_scene(oracle, [want[0]]).trace(O, D, flags=0, mode=1, nthreads=8), "n = 1 step %d vs the oracle" % step)
        fresh.close()
    sc.close(); sk.close()


# ---- a pose alone --------------------------------------------------------------------------------------------------------------------
def rays_over(n_rays, seed):
    from util import random_rays
    return random_rays(n_rays, seed, (-8, -8, -8), (8, 8, 8))


def test_a_pose_alone_touches_no_scene(gpu, capi, oracle):
    """after set_pose with no update the scene is still built and traces the OLD state's hits (the oracle of the old transforms); the next update
    follows the pose; two scenes on one skeleton are updated at different times, each with its own record of the pose it last applied"""
    n = 5
    parents = hierarchy("roots", 6, seed=1)
    sk = skeleton_of(capi, gpu, parents)
    joints = np.array([0, 5, 2, 2, 4], np.uint32)
    local = random_locals(n, 14)
    poses = [pose("unit", parents, seed=40 + k) for k in range(3)]
    for trs in poses:
        trs[:, 0:3] *= F(3.0)
    Ts = [transforms_of(posed(parents, K.inverse_binds(6, 5), trs)[0], joints, local) for trs in poses]
    O, D = rays_over(4000, 3)
    s1, s2 = gpu_scene(capi, gpu, [None] * n), gpu_scene(capi, gpu, [None] * n)
    s1.attach(0, sk, joints, local); s2.attach(0, sk, joints, local)
    sk.set_pose(poses[0])
    s1.update(); s2.update()
    old = oracle_scene(oracle, list(Ts[0])).trace(O, D, flags=0, mode=1, nthreads=8)
    assert int((old["inst"] != T.RT_NO_HIT).sum()) > 100
    before = arrays(s1, n)
    sk.set_pose(poses[1])                                 # no update: the scene stays built, in the state of its last update
    assert_hits_equal(s1.trace(O, D), old, "s1 after a pose alone")
    assert_bytes_equal(arrays(s1, n), before, "s1 after a pose alone")
    assert same_bits(s1.transforms(), Ts[0])
    s1.update()                                           # ... and this one is no no-op
    assert_hits_equal(s1.trace(O, D), oracle_scene(oracle, list(Ts[1])).trace(O, D, flags=0, mode=1, nthreads=8), "s1 after its update")
    assert same_bits(s1.transforms(), Ts[1]) and same_bits(s2.transforms(), Ts[0])
    assert_hits_equal(s2.trace(O, D), old, "s2, not updated yet")
    sk.set_pose(poses[2])
    s2.update()                                           # s2 skips pose 1 altogether
    assert same_bits(s2.transforms(), Ts[2]) and same_bits(s1.transforms(), Ts[1])
    s1.update()
    assert same_bits(s1.transforms(), Ts[2])
    assert_bytes_equal(arrays(s1, n), arrays(s2, n), "both scenes at pose 2")
    got = arrays(s1, n)
    s1.update(); s2.update()                              # nothing posed since: no-ops
    assert_bytes_equal(arrays(s1, n), got, "an update with nothing posed since")
    s1.close(); s2.close(); sk.close()


# ---- the device setter -----------------------------------------------------------------------------------------------------------------
RANGES = {"first": (0, 1), "last": (299, 1), "run63": (100, 63), "run64": (100, 64), "run65": (100, 65), "all": (0, 300)}


def test_device_setter_gives_the_host_setter_s_bytes(gpu, capi):
    """300 instances; the first, the last, runs of 63, 64 and 65, all: set from a device array on one scene and from the host on another, the
    source array overwritten right after the call on the same stream: the same bytes in every array, and in transforms() before and after"""
    n = 300
    start = random_xforms(n, 3, spread=6.0)
    a, b = gpu_scene(capi, gpu, start), gpu_scene(capi, gpu, start)
    held = rows(start)
    for step, (name, (first, count)) in enumerate(RANGES.items()):
        new = rows(random_xforms(count, 50 + step, spread=6.0))
        dev = gpu.upload(new)
        a.set_transforms(first, new)
        b.set_transforms_device(first, dev.ptr, count)
        capi.lib().rt_device_upload(gpu.h, dev.ptr, np.full(new.shape, np.nan, F).ctypes.data, new.nbytes)    # (queued behind the copy)
        held[first:first + count] = new
        assert same_bits(b.transforms(), held), name + ": pending, downloaded on demand"
        with pytest.raises(capi.RtError, match="pending"):
            b.bvh(-1)
        a.update(); b.update()
        assert_bytes_equal(arrays(a, n), arrays(b, n), name)
        assert same_bits(b.transforms(), held) and same_bits(a.transforms(), held), name
        dev.close()
    a.close(); b.close()


@pytest.mark.parametrize("again", (True, False))
def test_device_set_on_a_scene_never_built(gpu, capi, oracle, again):
    """the floats are only stored: the next build reads them; instances added in between keep them too, whether another device set (again) or
    the build itself finds the scene's storage too short for the longer list"""
    n = 7
    start = random_xforms(n, 3, spread=6.0)
    new = rows(random_xforms(n, 60, spread=6.0))
    sc = gpu_scene(capi, gpu, start[:5], build=False)
    dev = gpu.upload(new[1:4])
    sc.set_transforms_device(1, dev.ptr, 3)
    with pytest.raises(capi.RtError, match="rt_scene_update"):
        sc.update()
    gm = gpu_models(capi, gpu)
    for k in (5, 6):
        sc.add_model(gm[k % 2], start[k])
    dev2 = gpu.upload(new[6:7])
    final = rows(start)
    final[1:4] = new[1:4]
    if again:
        sc.set_transforms_device(6, dev2.ptr, 1)          # (a longer list: the scene's storage is reserved again, what it held is kept)
        final[6] = new[6]
    assert same_bits(sc.transforms(), final)
    sc.build()
    check_equals_build(capi, gpu, oracle, sc, final, "device set before the first build")
    sc.close(); dev.close(); dev2.close()


# ---- keyed rigid animation end to end ------------------------------------------------------------------------------------------------------
W_, H_ = 48, 32


def test_keyed_rigid_animation_end_to_end(gpu, capi, oracle):
    """a skeleton of roots only with a three-key clip, twelve instances: a frame is set_time + update.  At three sample times trace, a 48 x 32
    progressive frame and the realtime AOV pair == the oracle fed the numpy transforms; then a deferred pipeline's held frames see the scene
    they were accepted with across an update"""
    models, inst, mats, _ = light_scene()
    cam = np.array([0, 2, 16, 0, 0, 0, 0, 1, 0, 0.8, W_ / H_], F)
    n = len(inst)
    parents = hierarchy("forest", n, seed=0)
    ib = K.inverse_binds(n, 5)
    times, keys = clip(parents, 3, seed=17)
    local = rows([x for _, x in inst])
    joints = np.arange(n, dtype=np.uint32)
    sk = capi.Skeleton(gpu, parents, ib)
    c = sk.add_clip(times, keys)
    env = scenes.sky_cubemap(8)
    sk.set_time(c, times[0])
    p = make_gpu_pipeline(capi, gpu, models, inst, mats, W_, H_, env=env)
    p.set_depth_limits(3, 3)
    rp, _ = realtime_pair(capi, oracle, gpu, models, inst, mats, W_, H_, env)
    sc, rsc = p._keep[0], rp._keep[0]
    sc.attach(0, sk, joints, local); rsc.attach(0, sk, joints, local)
    pfcs = frames_of(capi, cam, 4, W_, H_)
    host = capi.ProgressiveHost(10)
    O, D = primary_rays(pfcs[0], W_, H_)

    def transforms_at(t):
        return transforms_of(posed(parents, ib, sampled(times, keys, t))[0], joints, local)

    ts = sample_times(times)
    picked = (ts[3], ts[6], ts[-2])                       # inside the first segment, just below the last key, beyond the end
    for k, t in enumerate(picked):
        sk.set_time(c, t)
        sc.update(); rsc.update()
        Tn = transforms_at(t)
        assert same_bits(sc.transforms(), Tn) and same_bits(rsc.transforms(), Tn), t
        osc = make_oracle_scene(oracle, models, [(mi, Tn[i]) for i, (mi, _) in enumerate(inst)])
        assert_hits_equal(sc.trace(O, D), osc.trace(O, D, flags=0, mode=1, nthreads=8), "trace at t=%g" % t)
        p.clear_output()
        p.update(pfcs[0]); p.render()
        acc, _ = oracle_frames_small(osc, mats, pfcs[:1], env)
        got = p.read_output()
        assert np.array_equal(got, acc), "progressive frame at t=%g: %d pixels differ" % (t, int((got != acc).any(axis=2).sum()))
        pfc = host.update_realtime(cam, 0.0, 3 + k, W_, H_)
        rp.update(pfc); rp.render()
        d, ind, _ = osc.render_realtime(np.stack(mats), pfc, W_, H_, env_faces=env, nthreads=8)
        assert np.array_equal(rp.read_output(0), d) and np.array_equal(rp.read_output(1), ind), "realtime AOVs at t=%g" % t
    # deferred: two frames held, a pose (it touches no scene: they stay held), an update (it renders them first, on the scene as it was)
    old = transforms_at(picked[-1])
    p.clear_output()
    p.set_deferred(4)
    for pfc in pfcs[:2]:
        p.update(pfc); p.render()
    assert p.deferred() == (4, 2)
    sk.set_time(c, picked[0])
    assert p.deferred() == (4, 2), "posing the skeleton flushed a scene's frames"
    sc.update()
    assert p.deferred() == (4, 0), "the update did not flush the recorded frames"
    for pfc in pfcs[2:]:
        p.update(pfc); p.render()
    new = transforms_at(picked[0])
    acc, _ = oracle_frames_small(make_oracle_scene(oracle, models, [(mi, old[i]) for i, (mi, _) in enumerate(inst)]), mats, pfcs[:2], env)
    acc, _ = oracle_frames_small(make_oracle_scene(oracle, models, [(mi, new[i]) for i, (mi, _) in enumerate(inst)]), mats, pfcs[2:], env, acc)
    got = p.read_output()
    assert np.array_equal(got, acc), "deferred frames: %d pixels differ" % int((got != acc).any(axis=2).sum())
    p.close(); rp.close(); sk.close()


def oracle_frames_small(osc, mats, pfcs, env, acc=None):
    acc = np.zeros((H_, W_, 4), F) if acc is None else acc
    st = None
    for pfc in pfcs:
        acc, st = osc.render(np.stack(mats), pfc, W_, H_, accum=acc, env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
    return acc, st


# ---- refusals and their messages -----------------------------------------------------------------------------------------------------------
def test_refusals_and_their_messages(gpu, capi):
    """every rule of the header's states, and that a refused call changes nothing"""
    import ctypes as C
    lib = capi.lib()
    n = 5
    start = random_xforms(n, 3, spread=6.0)
    sc = gpu_scene(capi, gpu, start)
    parents = hierarchy("chain", 4, seed=0)
    sk = skeleton_of(capi, gpu, parents)
    local = random_locals(2, 3)
    new = rows(random_xforms(n, 8, spread=6.0))
    dev = gpu.upload(new)
    before = arrays(sc, n)
    held = sc.transforms()
    j = np.array([1, 2], np.uint32)
    pj, pl, pn = j.ctypes.data_as(C.c_void_p), local.ctypes.data_as(C.c_void_p), new.ctypes.data_as(C.c_void_p)

    def unchanged(what):
        assert_bytes_equal(arrays(sc, n), before, what)
        assert same_bits(sc.transforms(), held), what
        assert all(sc.attachment(k) is None for k in range(n)), what

    # null arguments, an unknown mem, ranges, joints, contexts
    for rc in (lib.rt_scene_attach_instances(None, 0, 2, sk.h, pj, pl), lib.rt_scene_attach_instances(sc.h, 0, 2, None, pj, pl),
               lib.rt_scene_attach_instances(sc.h, 0, 2, sk.h, None, pl), lib.rt_scene_set_instance_transforms_mem(None, 0, 1, pn, 1),
               lib.rt_scene_set_instance_transforms_mem(sc.h, 0, 1, None, 1), lib.rt_scene_get_instance_transforms(sc.h, 0, 1, None),
               lib.rt_scene_get_instance_transforms(None, 0, 1, pn), lib.rt_scene_detach_instances(None, 0, 1),
               lib.rt_scene_get_instance_attachment(None, 0, None, None), lib.rt_skeleton_get_joints_device_ptr(sk.h, None)):
        assert rc == -1 and b"null" in lib.rt_last_error()
    for mem in (2, 0xFFFFFFFF):
        assert lib.rt_scene_set_instance_transforms_mem(sc.h, 0, 1, C.c_void_p(dev.ptr), mem) == -1 and b"unknown memory selector" in lib.rt_last_error()
    unchanged("null arguments and unknown selectors")
    for call in (lambda: sc.set_transforms_device(n - 1, dev.ptr, 2), lambda: sc.set_transforms_device(n + 1, dev.ptr, 0), lambda: sc.transforms(n - 1, 2),
                 lambda: sc.attach(n - 1, sk, j, local), lambda: sc.detach(n - 1, 2), lambda: sc.attachment(n)):
        with pytest.raises(capi.RtError, match="out of range") as e:
            call()
        assert e.value.code == -4                         # RT_ERR_STATE
    with pytest.raises(capi.RtError, match=r"entry 1 names joint 4: the skeleton has 4") as e:
        sc.attach(0, sk, [3, 4], local)
    assert e.value.code == -1
    other = capi.Context(0)
    foreign = skeleton_of(capi, other, parents)
    with pytest.raises(capi.RtError, match="different contexts") as e:
        sc.attach(0, foreign, j, local)
    assert e.value.code == -4
    foreign.close(); other.close()
    unchanged("refused attachments")
    # count == 0: no-ops
    sc.set_transforms_device(n, dev.ptr, 0)
    sc.attach(n, sk, np.zeros(0, np.uint32))
    sc.detach(n, 0)
    sc.detach(0, n)                                       # (none attached)
    assert sc.transforms(n, 0).shape == (0, 12)
    unchanged("empty ranges")
    with pytest.raises(capi.RtError, match="rt_skeleton_set_pose"):
        sk.joints_ptr()
    # attached to a skeleton without a pose: stale, and update and build refuse with everything kept
    sc.attach(1, sk, j, local)
    assert sc.attachment(1) == (sk, 1) and sc.attachment(2) == (sk, 2) and sc.attachment(0) is None and sc.attachment(3) is None
    assert same_bits(sc.transforms(), held), "attaching changes no stored transform"
    with pytest.raises(capi.RtError, match="2 instance transforms pending"):
        sc.bvh(-1)
    sc.set_transform(4, new[4])
    for call in (sc.update, sc.build):
        with pytest.raises(capi.RtError, match=r"instance 1 is attached to a skeleton that has no pose yet \(rt_skeleton_set_pose") as e:
            call()
        assert e.value.code == -4
        with pytest.raises(capi.RtError, match="3 instance transforms pending"):
            sc.bvh(-1)
    # a transform setter, host or _mem, whose range holds an attached instance
    for call in (lambda: sc.set_transform(2, new[2]), lambda: sc.set_transforms(0, new[:3]), lambda: sc.set_transforms_device(0, dev.ptr, 3),
                 lambda: capi._check(lib.rt_scene_set_instance_transforms_mem(sc.h, 2, 1, pn, 0))):
        with pytest.raises(capi.RtError, match=r"instance [12] is attached to joint [12].*rt_scene_detach_instances") as e:
            call()
        assert e.value.code == -4
    held[4] = new[4]
    assert same_bits(sc.transforms(), held), "a refused setter changed a transform"
    trs = pose("unit", parents, seed=2)
    sk.set_pose(trs)
    assert sk.joints_ptr()
    sc.update()
    W, _ = posed(parents, K.inverse_binds(4, 5), trs)
    held[1:3] = transforms_of(W, j, local)
    assert same_bits(sc.transforms(), held)
    # attaching again replaces the binding; detaching keeps the transform, marks nothing, and the setters work again
    sc.attach(2, sk, [0])
    assert sc.attachment(2) == (sk, 0)
    sc.update()
    held[2] = W[0]
    assert same_bits(sc.transforms(), held)
    built = arrays(sc, n)
    sc.detach(0, n)
    assert all(sc.attachment(k) is None for k in range(n))
    assert_bytes_equal(arrays(sc, n), built, "detaching marks nothing")
    sk.set_pose(pose("unit", parents, seed=3))
    sc.update()                                           # nobody follows the skeleton any more
    assert_bytes_equal(arrays(sc, n), built, "a pose after the detachment")
    sc.set_transforms(0, new[:3])
    sc.update()
    held[:3] = new[:3]
    assert same_bits(sc.transforms(), held)
    sc.close(); sk.close(); dev.close()


# ---- lifetime ----------------------------------------------------------------------------------------------------------------------------
def test_lifetimes(gpu, capi, oracle):
    """rt_skeleton_destroy while attached, then update, trace and scene destroy; and the scene first, then the skeleton"""
    n = 3
    parents = hierarchy("chain", 3, seed=0)
    trs = pose("unit", parents, seed=5)
    W, _ = posed(parents, K.inverse_binds(3, 5), trs)
    joints = np.array([2, 0, 1], np.uint32)
    O, D = rays_over(2000, 4)
    sc = gpu_scene(capi, gpu, [None] * n)
    sk = skeleton_of(capi, gpu, parents)
    sc.attach(0, sk, joints)
    sk.set_pose(trs)
    handle = sk.h.value
    sk.close()                                            # the caller's reference: the scene holds its own
    assert sc.attachment(0) == (handle, 2)
    sc.update()
    assert same_bits(sc.transforms(), W[joints])
    assert_hits_equal(sc.trace(O, D), oracle_scene(oracle, list(W[joints])).trace(O, D, flags=0, mode=1, nthreads=8), "after the skeleton's destroy")
    sc.set_masks(0, [0xFF, 0, 0xFF])
    sc.update()                                           # the instances simply keep their last transform
    assert same_bits(sc.transforms(), W[joints])
    sc.close()
    # the other way round
    sc = gpu_scene(capi, gpu, [None] * n)
    sk = skeleton_of(capi, gpu, parents)
    sc.attach(0, sk, joints)
    sk.set_pose(trs)
    sc.update()
    sc.close()
    sk.set_pose(trs)
    assert same_bits(sk.joints(), W)
    sk.close()
    gpu.synchronize()


# ---- a seeded sequence of edits against a model of the state ---------------------------------------------------------------------------------
def test_a_seeded_sequence_of_edits(gpu, capi, oracle):
    """about 40 interleaved edits -- attach, detach, pose, host and device sets, masks, update -- against the state as this small model keeps
    it: per instance the floats held, the binding and the mask; per skeleton W.  An update gives every attached instance compose(W[joint],
    local) or W[joint]; after every update the scene == a fresh build of the model's state"""
    n, nj = 9, 6
    r = np.random.default_rng(2024)
    parents = [hierarchy("random", nj, seed=1), hierarchy("roots", nj, seed=2)]
    sks = [skeleton_of(capi, gpu, p) for p in parents]
    Ws = []
    for k in range(2):                                    # (an unposed skeleton is the refusals' business)
        trs = pose("unit", parents[k], seed=70 + k)
        sks[k].set_pose(trs)
        Ws.append(posed(parents[k], K.inverse_binds(nj, 5), trs)[0])
    held = rows(random_xforms(n, 3, spread=6.0))
    masks = np.full(n, 0xFF, np.uint8)
    bound = [None] * n                                    # (skeleton index, joint, local or None)
    sc = gpu_scene(capi, gpu, list(held))
    keep = []
    updates = 0
    for step in range(44):
        op = "update" if step % 4 == 3 else ("attach", "detach", "pose", "host", "device", "mask")[int(r.integers(0, 6))]
        first = int(r.integers(0, n))
        count = int(r.integers(1, min(4, n - first) + 1))
        if op == "attach":
            k = int(r.integers(0, 2))
            joints = r.integers(0, nj, count).astype(np.uint32)
            local = random_locals(count, 100 + step) if r.integers(0, 2) else None
            sc.attach(first, sks[k], joints, local)
            for i in range(count):
                bound[first + i] = (k, int(joints[i]), None if local is None else local[i])
        elif op == "detach":
            sc.detach(first, count)
            for i in range(first, first + count):
                bound[i] = None
        elif op == "pose":
            k = int(r.integers(0, 2))
            trs = pose("unit", parents[k], seed=200 + step)
            trs[:, 0:3] *= F(3.0)
            sks[k].set_pose(trs)
            Ws[k] = posed(parents[k], K.inverse_binds(nj, 5), trs)[0]
        elif op in ("host", "device"):
            new = rows(random_xforms(count, 300 + step, spread=6.0))
            if op == "host":
                call = lambda: sc.set_transforms(first, new)
            else:
                keep.append(gpu.upload(new))
                call = lambda: sc.set_transforms_device(first, keep[-1].ptr, count)
            if any(bound[i] is not None for i in range(first, first + count)):
                with pytest.raises(capi.RtError, match="rt_scene_detach_instances"):
                    call()
            else:
                call()
                held[first:first + count] = new
        elif op == "mask":
            m = masks.copy()
            m[first:first + count] = r.choice(np.array([0, 0xFF, 1], np.uint8), count)
            if m.any():
                masks = m
                sc.set_masks(0, masks)
        else:
            sc.update()
            updates += 1
            for i in range(n):
                if bound[i] is not None:
                    k, joint, local = bound[i]
                    held[i] = transforms_of(Ws[k], np.array([joint]), None if local is None else local.reshape(1, 12))[0]
            check_equals_build(capi, gpu, oracle, sc, held, "step %d" % step, None if masks.all() else masks)
        if op != "update":
            for i in range(n):
                got = sc.attachment(i)
                assert (got is None) == (bound[i] is None) and (got is None or got == (sks[bound[i][0]], bound[i][1])), (step, i)
    assert updates >= 10
    sc.close()
    for x in sks + keep:
        x.close()


# ---- a list that grows after an attachment or a device set ---------------------------------------------------------------------------------
N0, N1 = 5, 7


def grown_after_attachment(capi, gpu, oracle):
    """5 instances built; 1-2 attached with local matrices and 3 without, posed, updated; two more added and the scene built with no further attach
    call; a second pose, updated.  Every step checked.  Instance 6 is added where joint 1 of a second skeleton stands.  Returns the scene, both
    skeletons with their W, the transforms held and what the three are bound by"""
    gm = gpu_models(capi, gpu)
    parents = [hierarchy("random", 6, seed=1), hierarchy("chain", 3, seed=2)]
    sks = [skeleton_of(capi, gpu, p) for p in parents]

    def posed_by(k, seed):
        trs = pose("unit", parents[k], seed=seed)
        trs[:, 0:3] *= F(3.0)
        sks[k].set_pose(trs)
        return posed(parents[k], K.inverse_binds(len(parents[k]), 5), trs)[0]

    W2 = posed_by(1, 91)
    start = rows(random_xforms(N1, 3, spread=6.0))
    start[6] = W2[1]
    joints = np.array([4, 0, 2], np.uint32)
    local = random_locals(2, 33)

    def composed(W):
        return np.concatenate([transforms_of(W, joints[:2], local), transforms_of(W, joints[2:], None)])

    sc = gpu_scene(capi, gpu, list(start[:N0]))
    sc.attach(1, sks[0], joints[:2], local)
    sc.attach(3, sks[0], joints[2:])
    W = posed_by(0, 92)
    sc.update()
    held = start.copy()
    held[1:4] = composed(W)
    check_equals_build(capi, gpu, oracle, sc, held[:N0], "attached, before the list grows")
    for k in (5, 6):
        sc.add_model(gm[k % 2], start[k])
    assert same_bits(sc.transforms(), held), "adding instances changes no stored transform"
    sc.build()
    check_equals_build(capi, gpu, oracle, sc, held, "attach, lengthen, build")
    for i in range(3):
        assert sc.attachment(1 + i) == (sks[0], int(joints[i])), i
    assert all(sc.attachment(i) is None for i in (0, 4, 5, 6))
    W = posed_by(0, 93)
    sc.update()
    moved = composed(W)
    assert not (moved == held[1:4]).all(axis=1).any(), "the second pose moves all three"
    held[1:4] = moved
    check_equals_build(capi, gpu, oracle, sc, held, "attach, lengthen, build, pose, update")
    return sc, sks, parents, W2, held


def test_attach_then_lengthen_then_build(gpu, capi, oracle):
    """the bindings of 1-3 outlive two rt_scene_add_model and the build behind them: the build composes them, attachment() still answers, the new
    instances have none, and the next pose moves the three and nothing else"""
    sc, sks, _, _, _ = grown_after_attachment(capi, gpu, oracle)
    sc.close()
    for sk in sks:
        sk.close()


def test_lengthen_then_attach_into_the_new_tail(gpu, capi, oracle):
    """on that scene: instance 6 attached to a second skeleton, instance 5 set from a device array: one update == a fresh build.  Instance 6 was
    added where its joint stands, so transforms() gives the same bytes before and after the update, for all 7, whichever side holds them; the
    second skeleton's next pose then moves 6 alone"""
    sc, sks, parents, W2, held = grown_after_attachment(capi, gpu, oracle)
    new = rows(random_xforms(1, 61, spread=6.0))
    dev = gpu.upload(new)
    sc.attach(6, sks[1], [1])
    sc.set_transforms_device(5, dev.ptr, 1)
    held[5] = new[0]
    assert sc.attachment(6) == (sks[1], 1) and sc.attachment(5) is None and sc.attachment(3) == (sks[0], 2)
    with pytest.raises(capi.RtError, match="2 instance transforms pending"):
        sc.bvh(-1)
    before = sc.transforms()
    assert same_bits(before, held), "pending: the device-set floats come down on demand"
    sc.update()
    assert same_bits(sc.transforms(), before), "transforms() before and after the update"
    check_equals_build(capi, gpu, oracle, sc, held, "lengthen, attach into the tail, device set")
    trs = pose("unit", parents[1], seed=94)
    trs[:, 0:3] *= F(3.0)
    sks[1].set_pose(trs)
    sc.update()
    held[6] = posed(parents[1], K.inverse_binds(3, 5), trs)[0][1]
    assert not same_bits(held[6], W2[1])
    check_equals_build(capi, gpu, oracle, sc, held, "the second skeleton posed again")
    sc.close(); dev.close()
    for sk in sks:
        sk.close()


def test_device_held_then_lengthen_on_a_built_scene(gpu, capi, oracle):
    """built, 1-3 set from device memory and left pending, two instances added: update is refused, transforms() still brings the three down from
    the device, and the build reads them"""
    start = rows(random_xforms(N1, 3, spread=6.0))
    new = rows(random_xforms(3, 62, spread=6.0))
    gm = gpu_models(capi, gpu)
    sc = gpu_scene(capi, gpu, list(start[:N0]))
    dev = gpu.upload(new)
    sc.set_transforms_device(1, dev.ptr, 3)
    for k in (5, 6):
        sc.add_model(gm[k % 2], start[k])
    with pytest.raises(capi.RtError, match=r"rt_scene_update: the scene has not been built since its last rt_scene_add_model \(an update builds no BLAS: "
                                           r"rt_scene_build\)") as e:
        sc.update()
    assert e.value.code == -4
    final = start.copy()
    final[1:4] = new
    assert same_bits(sc.transforms(), final)
    assert same_bits(sc.transforms(1, 3), new) and same_bits(sc.transforms(3, 3), final[3:6])
    sc.build()
    check_equals_build(capi, gpu, oracle, sc, final, "device set, lengthen, build")
    sc.close(); dev.close()


def test_a_seeded_sequence_of_edits_with_a_growing_list(gpu, capi, oracle):
    """test_a_seeded_sequence_of_edits' ops and its model of the state, on a list that grows: every 13th step adds an instance and builds (a
    build applies what an update applies).  5 instances at first, 8 after the three growths; the scene == a fresh build of the model's state
    after every update and every build"""
    n, nj = N0, 6
    r = np.random.default_rng(2025)
    parents = [hierarchy("random", nj, seed=1), hierarchy("roots", nj, seed=2)]
    sks = [skeleton_of(capi, gpu, p) for p in parents]
    gm = gpu_models(capi, gpu)
    Ws = []
    for k in range(2):
        trs = pose("unit", parents[k], seed=70 + k)
        sks[k].set_pose(trs)
        Ws.append(posed(parents[k], K.inverse_binds(nj, 5), trs)[0])
    held = rows(random_xforms(n, 3, spread=6.0))
    masks = np.full(n, 0xFF, np.uint8)
    bound = [None] * n                                    # (skeleton index, joint, local or None)
    sc = gpu_scene(capi, gpu, list(held))
    keep = []
    updates = growths = 0

    def applied(what):
        for i in range(n):
            if bound[i] is not None:
                k, joint, local = bound[i]
                held[i] = transforms_of(Ws[k], np.array([joint]), None if local is None else local.reshape(1, 12))[0]
        check_equals_build(capi, gpu, oracle, sc, held, what, None if masks.all() else masks)

    for step in range(40):
        op = "grow" if step % 13 == 6 else "update" if step % 4 == 3 else ("attach", "detach", "pose", "host", "device", "mask")[int(r.integers(0, 6))]
        first = int(r.integers(0, n))
        count = int(r.integers(1, min(4, n - first) + 1))
        if op == "attach":
            k = int(r.integers(0, 2))
            joints = r.integers(0, nj, count).astype(np.uint32)
            local = random_locals(count, 100 + step) if r.integers(0, 2) else None
            sc.attach(first, sks[k], joints, local)
            for i in range(count):
                bound[first + i] = (k, int(joints[i]), None if local is None else local[i])
        elif op == "detach":
            sc.detach(first, count)
            for i in range(first, first + count):
                bound[i] = None
        elif op == "pose":
            k = int(r.integers(0, 2))
            trs = pose("unit", parents[k], seed=200 + step)
            trs[:, 0:3] *= F(3.0)
            sks[k].set_pose(trs)
            Ws[k] = posed(parents[k], K.inverse_binds(nj, 5), trs)[0]
        elif op in ("host", "device"):
            new = rows(random_xforms(count, 300 + step, spread=6.0))
            if op == "host":
                call = lambda: sc.set_transforms(first, new)
            else:
                keep.append(gpu.upload(new))
                call = lambda: sc.set_transforms_device(first, keep[-1].ptr, count)
            if any(bound[i] is not None for i in range(first, first + count)):
                with pytest.raises(capi.RtError, match="rt_scene_detach_instances"):
                    call()
            else:
                call()
                held[first:first + count] = new
        elif op == "mask":
            m = masks.copy()
            m[first:first + count] = r.choice(np.array([0, 0xFF, 1], np.uint8), count)
            if m.any():
                masks = m
                sc.set_masks(0, masks)
        elif op == "grow":
            x = rows(random_xforms(1, 400 + step, spread=6.0))
            sc.add_model(gm[n % 2], x[0])
            held = np.concatenate([held, x])
            masks = np.append(masks, np.uint8(0xFF))
            bound.append(None)
            n += 1
            assert sc.attachment(n - 1) is None and sc.masks()[n - 1] == 0xFF
            with pytest.raises(capi.RtError, match="has not been built since its last rt_scene_add_model"):
                sc.update()
            sc.build()
            growths += 1
            applied("step %d, a build of %d instances" % (step, n))
        else:
            sc.update()
            updates += 1
            applied("step %d" % step)
        if op not in ("update", "grow"):
            for i in range(n):
                got = sc.attachment(i)
                assert (got is None) == (bound[i] is None) and (got is None or got == (sks[bound[i][0]], bound[i][1])), (step, i)
    assert updates >= 8 and growths >= 3 and n == N0 + growths
    sc.close()
    for x in sks + keep:
        x.close()


def test_refusals_at_the_edge_of_a_grown_list(gpu, capi, oracle):
    """1-3 attached on a built scene, two instances added: a host set and a device set over 3-5 -- an attached instance, a free one and a new one
    -- are refused as ever and change nothing; detaching 2-6, a range that reaches into the new tail, is OK and lets 2 and 3 go"""
    start = rows(random_xforms(N1, 3, spread=6.0))
    new = rows(random_xforms(3, 63, spread=6.0))
    gm = gpu_models(capi, gpu)
    parents = hierarchy("chain", 4, seed=0)
    sk = skeleton_of(capi, gpu, parents)
    trs = pose("unit", parents, seed=2)
    trs[:, 0:3] *= F(3.0)
    sk.set_pose(trs)
    W, _ = posed(parents, K.inverse_binds(4, 5), trs)
    joints = np.array([3, 1, 2], np.uint32)
    sc = gpu_scene(capi, gpu, list(start[:N0]))
    sc.attach(1, sk, joints)
    for k in (5, 6):
        sc.add_model(gm[k % 2], start[k])
    dev = gpu.upload(new)
    bindings = [None, (sk, 3), (sk, 1), (sk, 2), None, None, None]
    for call in (lambda: sc.set_transforms(3, new), lambda: sc.set_transforms_device(3, dev.ptr, 3)):
        with pytest.raises(capi.RtError, match=r"instance 3 is attached to joint 2 of a skeleton, which gives it its transform "
                                               r"\(rt_scene_detach_instances lets it go\)") as e:
            call()
        assert e.value.code == -4
        assert same_bits(sc.transforms(), start), "a refused setter changed a transform"
        assert [sc.attachment(i) for i in range(N1)] == bindings
    sc.detach(2, 5)
    assert [sc.attachment(i) for i in range(N1)] == [None, (sk, 3)] + [None] * 5
    sc.set_transforms(3, new)                             # (free again)
    sc.build()
    final = start.copy()
    final[1] = W[3]
    final[3:6] = new
    check_equals_build(capi, gpu, oracle, sc, final, "after the refusals, the detachment and a build")
    sc.close(); sk.close(); dev.close()


def test_device_set_then_attached_before_any_update(gpu, capi, oracle):
    """an instance set from device memory and attached before an update has applied the floats keeps them -- transforms() and, once detached
    again, the update -- and attached it takes the joint's, its device-set neighbours theirs"""
    start = rows(random_xforms(N0, 3, spread=6.0))
    new = [rows(random_xforms(3, 64 + k, spread=6.0)) for k in range(2)]
    parents = hierarchy("chain", 3, seed=0)
    sk = skeleton_of(capi, gpu, parents)
    trs = pose("unit", parents, seed=7)
    trs[:, 0:3] *= F(3.0)
    sk.set_pose(trs)
    W, _ = posed(parents, K.inverse_binds(3, 5), trs)
    sc = gpu_scene(capi, gpu, list(start))
    devs = [gpu.upload(x) for x in new]
    held = start.copy()
    sc.set_transforms_device(1, devs[0].ptr, 3)
    held[1:4] = new[0]
    sc.attach(2, sk, [1])
    assert same_bits(sc.transforms(), held), "attaching changes no stored transform, wherever it is stored"
    sc.detach(2)
    assert same_bits(sc.transforms(), held) and sc.attachment(2) is None
    sc.update()
    check_equals_build(capi, gpu, oracle, sc, held, "device set, attached, detached, updated")
    sc.set_transforms_device(1, devs[1].ptr, 3)
    held[1:4] = new[1]
    sc.attach(2, sk, [1])
    assert same_bits(sc.transforms(), held)
    sc.update()
    held[2] = W[1]
    check_equals_build(capi, gpu, oracle, sc, held, "device set, attached, updated")
    sc.close(); sk.close()
    for d in devs:
        d.close()


# ---- the example -------------------------------------------------------------------------------------------------------------------------
def fnv1a(raw):
    h = 2166136261
    for b in raw:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def test_machines_example_through_the_cpp_mirror(gpu, capi, tmp_path):
    """examples/realtime_machines.cpp: per frame RtSkeleton::setTime + RtScene::update only; the checksum of the transforms its scene holds after
    5 frames == the one the Python path gives for the same hierarchy, clip, joints and local matrices"""
    exe = os.path.join(ROOT, "dxrexperiments_amd", "lib", "realtime_machines")
    frames = 5
    out = tmp_path / "machines.pfm"
    r = subprocess.run([exe, "96", "64", str(frames), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "6 boxes on 5 joints, 3 keys: %d frames" % frames in r.stdout
    raw = out.read_bytes()
    head = b"PF\n96 64\n-1.0\n"
    assert raw.startswith(head)
    image = np.frombuffer(raw[len(head):], "<f4").reshape(64, 96, 3)
    assert image.max() > 0.1 and image.std() > 0.01      # an image, not a constant
    parents = np.array([-1, 0, 1, 1, 0], np.int32)
    offsets = np.array([[0, -1, 0], [0, 1, 0], [1.25, 0.75, 0], [-1.25, 0.75, 0], [0, 0.25, -1.5]], F)
    turns = np.array([[[0, 0, 0, 1]] * 5,
                      [[0, 0.5, 0, 1], [0, 0, 0.25, 1], [0.5, 0, 0, 1], [0, 0, -0.5, 1], [0, -0.25, 0, 1]],
                      [[0, -0.25, 0, 1], [0.25, 0, -0.25, 1], [0, 0.5, 0.5, 1], [-0.5, 0, 0, 1], [0.125, 0.5, 0, 1]]], F)
    keys = np.ones((3, 5, 10), F)
    keys[:, :, 0:3] = offsets
    keys[:, :, 3:7] = turns
    times = np.array([0, 1, 2], F)
    joints = np.array([0, 1, 2, 3, 4, 2], np.uint32)
    shape = np.array([[2.5, 0.25, 2.5, 0, 0, 0], [0.5, 1.5, 0.5, 0, 0, 0], [0.75, 0.25, 0.25, 0, 0, 0], [0.75, 0.25, 0.25, 0, 0, 0],
                      [0.75, 0.75, 0.75, 0, 0, 0], [0.25, 0.25, 0.5, 0.5, 0, 0.25]], F)
    local = np.zeros((6, 12), F)
    for row in range(3):
        local[:, 5 * row] = shape[:, row]
        local[:, 4 * row + 3] = shape[:, 3 + row]
    ib = np.tile(IDENTITY, (5, 1))
    t = np.fmod(F(0.125) * F(frames), times[-1])
    want = transforms_of(posed(parents, ib, sampled(times, keys, t))[0], joints, local)
    sk = capi.Skeleton(gpu, parents, ib)
    c = sk.add_clip(times, keys)
    m = capi.Model(gpu, *triangle_soup(4, seed=3, extent=1.0, size=0.5))
    sc = gpu_scene(capi, gpu, [None] * 6, models=[m], build=False)
    sk.set_time(c, 0.0)
    sc.attach(0, sk, joints, local)
    sc.build()
    sk.set_time(c, float(t))
    sc.update()
    assert same_bits(sc.transforms(), want)
    assert "transforms checksum %08x" % fnv1a(sc.transforms().tobytes()) in r.stdout, r.stdout
    sc.close(); sk.close()
