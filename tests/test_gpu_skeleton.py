"""Posed skeletons (rt_skeleton_set_pose / rt_skeleton_set_time + rt_model_set_bones_from_skeleton + rt_scene_update): the local pose, the
world matrices and the palette the device computes are, byte for byte, the definition of DESIGN.md section 2 "Posed skeletons" restated in
numpy (tests/skeleton_cases.py) -- every hierarchy family under every pose family, both sides of a wave, of a block and of the LDS limit,
65536 joints, a chain 300 deep, host and device poses; the sampler on, between and beyond the keys of clips of 1, 2, 3 and 17 keys; the states
and their messages; and through the skin end to end: vertices, the scene array for array against a fresh build, a frame against the oracle.
No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import skeleton_cases as S
import skin_cases as K
from dxrexperiments_amd import rtypes as T, scenes
from test_gpu_batch import frames_of
from test_gpu_model_deform import RAYS, all_arrays, assert_frame, check, close_all, own_scene, pipeline_over
from test_gpu_model_skin import assert_vertices
from test_gpu_pipeline import make_oracle_scene
from test_gpu_scene_update import assert_bytes_equal
from util import random_xforms

pytestmark = pytest.mark.gpu

W, H = 96, 64
LDS = S.lds_joints()
COUNTS = {"1": 1, "2": 2, "63": 63, "64": 64, "65": 65, "257": 257, "lds": LDS, "lds+1": LDS + 1}


def assert_floats(got, want, what, nans=False):
    """byte for byte; nans: sign and payload of a NaN are the hardware's (skin_cases.canonical_nans), where one stands is not"""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    if nans:
        assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaNs stand elsewhere" % what
        got, want = K.canonical_nans(got), K.canonical_nans(want)
    assert got.tobytes() == want.tobytes(), "%s: %d joints differ" % (what, int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()))


def assert_posed(sk, parents, ib, trs, what, nans=False):
    """read_pose, read_joints and read_palette against the restatement"""
    Wm, M = S.posed(parents, ib, trs)
    assert_floats(sk.pose(), np.ascontiguousarray(trs, np.float32), what + ": pose", nans)
    assert_floats(sk.joints(), Wm, what + ": joints", nans)
    assert_floats(sk.palette(), M, what + ": palette", nans)
    return Wm, M


def assert_poison(parents, Wm, M, what):
    """NaNs and infs stand exactly in the poisoned joints and their descendants"""
    below = S.descendants(parents, S.poisoned(parents))
    for a, name in ((Wm, "joints"), (M, "palette")):
        assert np.array_equal(~np.isfinite(a).all(axis=1), below), "%s: %s: the poison stands elsewhere than in the poisoned joints and below them" % (what, name)
    assert np.isnan(M).any(), what


# ---- pose = definition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", list(COUNTS))
def test_pose_is_its_definition(gpu, capi, count):
    """n = 1, 2, 63 / 64 / 65 (both sides of a wave), 257 (both sides of the block), RT_SKELETON_LDS_JOINTS (the last skeleton posed from
    LDS) and one more (the first posed from global memory); every hierarchy family under every pose family, from a host array; then another
    pose from device memory on the same skeleton: it starts from nothing the first left"""
    n = COUNTS[count]
    seed = 100 * n
    for family in S.HIERARCHIES:
        parents = S.hierarchy(family, n, seed)
        ib = S.inverse_binds(n, seed + 1)
        sk = capi.Skeleton(gpu, parents, ib)
        order, offsets = S.levels_of(parents)
        assert sk.info() == (n, len(offsets) - 1, 0)
        for k, pose_family in enumerate(S.POSES):
            seed += 1
            what = "%d joints, %s, %s" % (n, family, pose_family)
            trs = S.pose(pose_family, parents, seed)
            sk.set_pose(trs)
            Wm, M = assert_posed(sk, parents, ib, trs, what, nans=pose_family == "nan_inf")
            if pose_family == "nan_inf":
                assert_poison(parents, Wm, M, what)
            else:
                assert np.isfinite(M).all(), what
            other = S.pose(S.POSES[(k + 1) % 4], parents, seed + 50)     # (a finite family)
            buf = gpu.upload(other)
            sk.set_pose_device(buf.ptr)
            gpu.synchronize()
            buf.close()
            assert_posed(sk, parents, ib, other, what + ", then a device pose")
        sk.close()


@pytest.mark.parametrize("family,pose_family", [("random", "unit"), ("star", "raw"), ("random", "nan_inf")])
def test_65536_joints(gpu, capi, family, pose_family):
    """the limit: a random tree and a star of 65536 joints, the largest joint and the largest parent index in use"""
    n = 65536
    parents = S.hierarchy(family, n, 9)
    if family == "random":
        parents[n - 1] = n - 2                           # (parent 65534 under joint 65535: both ends of the 16-bit fields of the level table)
    ib = S.inverse_binds(n, 10)
    trs = S.pose(pose_family, parents, 11)
    sk = capi.Skeleton(gpu, parents, ib)
    sk.set_pose(trs)
    what = "65536 joints, %s, %s" % (family, pose_family)
    Wm, M = assert_posed(sk, parents, ib, trs, what, nans=pose_family == "nan_inf")
    if pose_family == "nan_inf":
        assert_poison(parents, Wm, M, what)
    sk.close()


def test_a_chain_300_deep(gpu, capi):
    """300 levels of one joint each: the association of the recursion, 299 products deep; scales 0.5 .. 1.5 keep it finite"""
    n = 300
    parents = S.hierarchy("chain", n)
    ib = S.inverse_binds(n, 20)
    sk = capi.Skeleton(gpu, parents, ib)
    assert sk.info() == (n, n, 0)
    for seed, pose_family in enumerate(S.POSES):
        trs = S.pose(pose_family, parents, 21 + seed)
        if pose_family == "unit":
            trs[:, 7:10] = np.float32(1.0) + (trs[:, 7:10] - np.float32(1.0)) * np.float32(0.02)
        sk.set_pose(trs)
        Wm, M = assert_posed(sk, parents, ib, trs, "chain of 300, " + pose_family, nans=pose_family == "nan_inf")
        if pose_family == "unit":
            assert np.isfinite(M).all() and np.abs(Wm[-1]).max() > 0, "the end of the chain says nothing"
    sk.close()


# ---- sampler = definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 2, 3, 17])
def test_sampled_poses_are_their_definition(gpu, capi, n_keys):
    """257 joints (both sides of the sampling kernel's block) of a random tree; t below the first key, on every key, inside every segment,
    just before the next key, on the last key, beyond it and at -inf / +inf; unit keys, raw keys (zero quaternions: the (0, 0, 0, 1)
    branch) and keys with a NaN and an inf"""
    n = 257
    parents = S.hierarchy("random", n, 30)
    ib = S.inverse_binds(n, 31)
    sk = capi.Skeleton(gpu, parents, ib)
    for c, family in enumerate(("unit", "raw", "nan_inf")):
        times, keys = S.clip(parents, n_keys, 40 + 100 * c + n_keys, family)
        clip = sk.add_clip(times, keys)
        assert clip == c and sk.info() == (n, len(S.levels_of(parents)[1]) - 1, c + 1)
        ts = S.sample_times(times)
        assert len(ts) == 4 + n_keys + 2 * (n_keys - 1)
        identity = 0
        for t in (ts if family == "unit" else ts[::3]):
            trs = S.sampled(times, keys, t)
            sk.set_time(clip, float(t))
            what = "K %d, %s keys, t %r" % (n_keys, family, float(t))
            assert_posed(sk, parents, ib, trs, what, nans=family == "nan_inf")
            identity += int((trs[:, 3:7] == np.array([0, 0, 0, 1], np.float32)).all(axis=1).sum())
            if family == "unit":
                assert np.abs(np.linalg.norm(trs[:, 3:7].astype(np.float64), axis=1) - 1).max() < 1e-6, what
        if family == "raw":
            assert identity > 0, "no joint took the (0, 0, 0, 1) branch"
    sk.close()


def test_the_shortest_path_and_the_quaternion_that_vanishes(gpu, capi):
    """neighbouring keys on opposite sides of the sphere (d < 0): B is negated, the sample stays beside A instead of passing through the
    origin.  A = -B at a = 0.5: by the definition d = -|A|^2 < 0 negates B into A itself, so the sample is A normalised -- the quaternion
    does not vanish; the (0, 0, 0, 1) branch is reached by a lerp that does: zero quaternions in both keys (n = 0), and lengths whose
    squares overflow (n = inf)."""
    n = 65
    parents = S.hierarchy("roots", n, 50)
    ib = S.inverse_binds(n, 51)
    rng = np.random.default_rng(52)
    a = S.pose("unit", parents, 53)
    b = a.copy()
    b[:, 3:7] = -(a[:, 3:7] + rng.normal(scale=0.05, size=(n, 4)).astype(np.float32))          # the same rotation, nearly, the other sign
    c = a.copy()
    c[:, 3:7] = -a[:, 3:7]                               # A = -B exactly
    zero = a.copy()
    zero[::2, 3:7] = 0.0
    huge = a.copy()
    huge[:, 3:7] *= np.float32(1e30)
    times = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0], np.float32)
    keys = np.stack([a, b, a, c, zero, zero])
    sk = capi.Skeleton(gpu, parents, ib)
    clip = sk.add_clip(times, keys)
    big = sk.add_clip(times[:2], np.stack([huge, huge]))
    for t in (0.25, 0.5, 0.75):
        trs = S.sampled(times, keys, t)
        d = (a[:, 3:7].astype(np.float64) * b[:, 3:7]).sum(axis=1)
        assert (d < 0).all() and (np.abs((trs[:, 3:7].astype(np.float64) * a[:, 3:7]).sum(axis=1)) > 0.99).all(), "the restatement went the long way round"
        sk.set_time(clip, t)
        assert_posed(sk, parents, ib, trs, "d < 0, t %g" % t)
    trs = S.sampled(times, keys, 2.5)                    # A = -B at a = 0.5
    assert S.segment(times, 2.5) == (2, np.float32(0.5))
    assert np.abs(trs[:, 3:7].astype(np.float64) - a[:, 3:7]).max() < 1e-6 and not (trs[:, 3:7] == np.array([0, 0, 0, 1], np.float32)).all(axis=1).any()
    sk.set_time(clip, 2.5)
    assert_posed(sk, parents, ib, trs, "A = -B at a = 0.5")
    trs = S.sampled(times, keys, 4.5)                    # zero quaternions in both keys
    assert (trs[::2, 3:7] == np.array([0, 0, 0, 1], np.float32)).all() and not (trs[1::2, 3:7] == np.array([0, 0, 0, 1], np.float32)).all(axis=1).any()
    sk.set_time(clip, 4.5)
    assert_posed(sk, parents, ib, trs, "zero quaternions")
    trs = S.sampled(times[:2], keys=np.stack([huge, huge]), t=0.5)
    assert (trs[:, 3:7] == np.array([0, 0, 0, 1], np.float32)).all()
    sk.set_time(big, 0.5)
    assert_posed(sk, parents, ib, trs, "n = inf")
    sk.close()


def test_two_clips_on_one_skeleton(gpu, capi):
    """ids stay valid across add_clip; clear_clips removes them all and leaves the pose; ids start again"""
    n = 64
    parents = S.hierarchy("random", n, 60)
    ib = S.inverse_binds(n, 61)
    sk = capi.Skeleton(gpu, parents, ib)
    t0, k0 = S.clip(parents, 3, 62)
    t1, k1 = S.clip(parents, 17, 63, "mirror")
    c0 = sk.add_clip(t0, k0)
    sk.set_time(c0, float(t0[1]) + 0.05)
    first = assert_posed(sk, parents, ib, S.sampled(t0, k0, float(t0[1]) + 0.05), "clip 0")
    c1 = sk.add_clip(t1, k1)
    assert (c0, c1) == (0, 1) and sk.info()[2] == 2
    assert sk.palette().tobytes() == first[1].tobytes(), "add_clip changed the pose"
    for clip, (times, keys) in ((c1, (t1, k1)), (c0, (t0, k0)), (c1, (t1, k1))):
        t = float(times[1]) + 0.01
        sk.set_time(clip, t)
        assert_posed(sk, parents, ib, S.sampled(times, keys, t), "clip %d after both were added" % clip)
    last = sk.palette()
    sk.clear_clips()
    assert sk.info()[2] == 0 and sk.palette().tobytes() == last.tobytes()
    with pytest.raises(capi.RtError, match="clip 0") as e:
        sk.set_time(0, 0.0)
    assert e.value.code == -4
    assert sk.add_clip(t1, k1) == 0
    sk.set_time(0, float(t1[3]))
    assert_posed(sk, parents, ib, S.sampled(t1, k1, float(t1[3])), "after clear_clips")
    sk.close()


# ---- states ------------------------------------------------------------------------------------------------------------------------------
def skinned_model(capi, ctx, n_joints, seed=70, influences=4, n_verts=257):
    rest, idx, bones, weights, _ = K.case("convex", n_verts, influences, n_joints, seed)
    m = capi.Model(ctx, rest, idx)
    m.set_skin(bones, weights, n_joints)
    return m, rest, idx, bones, weights


def test_refusals_and_their_messages(gpu, capi):
    """every refusal, with its code and message; nothing changes when a call refuses"""
    lib = capi.lib()
    n = 7
    parents = S.hierarchy("random", n, 80)
    ib = S.inverse_binds(n, 81)
    bad = parents.copy()
    bad[4] = 4
    with pytest.raises(capi.RtError, match="joint 4 names parent 4") as e:
        capi.Skeleton(gpu, bad, ib)
    assert e.value.code == -1
    bad[4] = -2
    with pytest.raises(capi.RtError, match="joint 4 names parent -2"):
        capi.Skeleton(gpu, bad, ib)
    h = C.c_void_p()
    for count in (0, 65537):
        assert lib.rt_skeleton_create(gpu.h, count, parents.ctypes.data_as(C.c_void_p), ib.ctypes.data_as(C.c_void_p), C.byref(h)) == -1 and h.value is None
        assert b"1 .. 65536" in lib.rt_last_error()
    sk = capi.Skeleton(gpu, parents, ib)
    m, rest, idx, bones, weights = skinned_model(capi, gpu, n)
    # before the first pose
    for call in (sk.pose, sk.joints, sk.palette, sk.palette_ptr, lambda: m.set_bones_from(sk)):
        with pytest.raises(capi.RtError, match="rt_skeleton_set_pose") as e:
            call()
        assert e.value.code == -4
    assert m.geometry()[0].tobytes() == rest.tobytes()
    # clips
    times, keys = S.clip(parents, 4, 82)
    pt, pk = times.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p)
    clip = C.c_uint32(99)
    assert lib.rt_skeleton_add_clip(sk.h, 0, pt, pk, C.byref(clip)) == -1 and b"at least one key" in lib.rt_last_error()
    assert lib.rt_skeleton_add_clip(sk.h, 4, None, pk, C.byref(clip)) == -1 and lib.rt_skeleton_add_clip(sk.h, 4, pt, None, C.byref(clip)) == -1
    for wrong, message in ((np.array([0, 1, np.nan, 3], np.float32), "key 2 is not finite"), (np.array([0, 1, 2, np.inf], np.float32), "key 3 is not finite"),
                           (np.array([0, 2, 1, 3], np.float32), "key 2 at 1 after key 1 at 2"), (np.array([0, 1, 1, 3], np.float32), "key 2 at 1 after key 1 at 1")):
        with pytest.raises(capi.RtError, match=message) as e:
            sk.add_clip(wrong, keys)
        assert e.value.code == -1
    assert clip.value == 99 and sk.info() == (n, len(S.levels_of(parents)[1]) - 1, 0)
    with pytest.raises(capi.RtError, match="clip 0") as e:
        sk.set_time(0, 0.0)
    assert e.value.code == -4
    assert sk.add_clip(times, keys) == 0
    with pytest.raises(capi.RtError, match="NaN") as e:
        sk.set_time(0, float("nan"))
    assert e.value.code == -1
    with pytest.raises(capi.RtError, match="clip 1") as e:
        sk.set_time(1, 0.0)
    assert e.value.code == -4
    with pytest.raises(capi.RtError, match="rt_skeleton_set_pose"):
        sk.palette()                                     # (the refused set_time calls posed nothing)
    trs = S.pose("unit", parents, 83)
    assert lib.rt_skeleton_set_pose(sk.h, trs.ctypes.data_as(C.c_void_p), 2) == -1 and lib.rt_skeleton_set_pose(sk.h, None, 0) == -1
    with pytest.raises(capi.RtError, match="rt_skeleton_set_pose"):
        sk.palette()
    sk.set_pose(trs)
    Wm, M = assert_posed(sk, parents, ib, trs, "after the refusals")
    assert lib.rt_skeleton_read_pose(sk.h, None) == -1 and lib.rt_skeleton_read_joints(sk.h, None) == -1 and lib.rt_skeleton_read_palette(sk.h, None) == -1
    assert lib.rt_skeleton_get_palette_device_ptr(sk.h, None) == -1
    # set_bones_from: a model without a skin, another bone count, another context
    plain = capi.Model(gpu, rest, idx)
    with pytest.raises(capi.RtError, match="rt_model_set_skin") as e:
        plain.set_bones_from(sk)
    assert e.value.code == -4
    fewer, *_ = skinned_model(capi, gpu, n - 2, seed=84)
    with pytest.raises(capi.RtError, match="a skin of 5 bones and a skeleton of 7 joints") as e:
        fewer.set_bones_from(sk)
    assert e.value.code == -4
    other = capi.Context(0)
    try:
        foreign, *_ = skinned_model(capi, other, n, seed=85)
        with pytest.raises(capi.RtError, match="different contexts") as e:
            foreign.set_bones_from(sk)
        assert e.value.code == -4
        foreign.close()
    finally:
        other.close()
    assert m.geometry()[0].tobytes() == rest.tobytes() and sk.palette().tobytes() == M.tobytes()
    m.set_bones_from(sk)
    assert_vertices(m.geometry()[0], K.skinned(rest, bones, weights, M), "set_bones_from after the refusals")
    for model in (plain, fewer, m):
        model.close()
    sk.close()


def test_a_pose_leaves_a_built_scene_built(gpu, capi):
    """rt_skeleton_set_pose and rt_skeleton_set_time touch no model and no scene: the scene traces, and its arrays are what they were;
    rt_model_set_bones_from_skeleton is what leaves it stale, and the message names the pending vertices"""
    n = 6
    parents = S.hierarchy("chain", n)
    sk = capi.Skeleton(gpu, parents, S.inverse_binds(n, 90))
    m, rest, idx, bones, weights = skinned_model(capi, gpu, n, seed=91)
    sc = capi.Scene(gpu)
    sc.add_model(m, None)
    sc.build()
    inst = [(0, None)]
    before = all_arrays(sc, [m], inst)
    times, keys = S.clip(parents, 3, 92)
    clip = sk.add_clip(times, keys)
    sk.set_pose(S.pose("unit", parents, 93))
    sc.trace(*RAYS)
    sk.set_time(clip, float(times[1]))
    sc.trace(*RAYS)
    assert_bytes_equal(all_arrays(sc, [m], inst), before, "after two poses")
    m.set_bones_from(sk)
    with pytest.raises(capi.RtError, match="new vertices of the model of 1 instance pending") as e:
        sc.trace(*RAYS)
    assert e.value.code == -4
    sc.update()
    sc.trace(*RAYS)
    close_all(sc, [m])
    sk.close()


def test_destroy_right_after_set_bones_from(gpu, capi):
    """the skin kernel that rt_model_set_bones_from_skeleton queued reads the palette of a skeleton destroyed right behind it: 20,000
    vertices over 300 joints, then synchronise and read the model"""
    n, nv = 300, 20000
    parents = S.hierarchy("random", n, 95)
    ib = S.inverse_binds(n, 96)
    trs = S.pose("unit", parents, 97)
    m, rest, idx, bones, weights = skinned_model(capi, gpu, n, seed=98, n_verts=nv)
    sk = capi.Skeleton(gpu, parents, ib)
    sk.set_pose(trs)
    m.set_bones_from(sk)
    sk.close()
    gpu.synchronize()
    _, M = S.posed(parents, ib, trs)
    assert_vertices(m.geometry()[0], K.skinned(rest, bones, weights, M), "after the skeleton was destroyed")
    m.close()


# ---- the example ---------------------------------------------------------------------------------------------------------------------------
def test_character_example_through_the_cpp_mirror(tmp_path):
    """examples/realtime_character.cpp: RtSkeleton::create + addClip once, RtSkeleton::setTime + RtModel::setBones(skeleton) + RtScene::update
    per frame, end to end; after three frames the image is another than after one"""
    exe = os.path.join(K.ROOT, "dxrexperiments_amd", "lib", "realtime_character")
    images = []
    for frames in (1, 3):
        out = tmp_path / ("out%d.pfm" % frames)
        r = subprocess.run([exe, "96", "64", str(frames), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "1536 skinned vertices, 2976 triangles, 4 joints, 3 keys, posed on the device: %d frames" % frames in r.stdout and "BLAS + TLAS update" in r.stdout
        raw = out.read_bytes()
        head = b"PF\n96 64\n-1.0\n"
        assert raw.startswith(head)
        images.append(np.frombuffer(raw[len(head):], "<f4").reshape(64, 96, 3))
    assert images[0].max() > 0.1 and images[0].std() > 0.01            # an image, not a constant
    assert not np.array_equal(images[0], images[1])


# ---- through the skin, end to end ----------------------------------------------------------------------------------------------------------
def gentle_clip(parents, n_keys, seed):
    """keys that keep a mesh in its neighbourhood: turns of up to about 0.4 rad, translations of up to 0.3, scales 0.8 .. 1.25"""
    rng = np.random.default_rng(seed)
    n = len(parents)
    keys = np.zeros((n_keys, n, 10), np.float32)
    keys[:, :, 0:3] = rng.uniform(-0.3, 0.3, (n_keys, n, 3))
    q = np.concatenate([rng.normal(scale=0.1, size=(n_keys, n, 3)), np.ones((n_keys, n, 1))], axis=2)
    keys[:, :, 3:7] = q / np.linalg.norm(q, axis=2, keepdims=True)
    keys[:, :, 7:10] = rng.uniform(0.8, 1.25, (n_keys, n, 3))
    return np.array([0.0, 0.4, 1.0, 1.5][:n_keys], np.float32), keys


def test_a_character_end_to_end(gpu, capi, oracle):
    """a 257-vertex model of skin_cases, K = 4 influences, bones = the 7 joints of a random tree, two instances; per step set_time +
    set_bones_from + rt_scene_update: the vertices == skin_cases.skinned over skeleton_cases.posed, byte for byte; the scene == a fresh build
    over a fresh model of those vertices, array for array, and the oracle's; one frame, 96 x 64, == the oracle's; a second model that shares
    the skeleton gets the same palette"""
    n = 7
    parents = S.hierarchy("random", n, 110)
    ib = K.gentle_palette(n, 111, angle=0.2, spread=0.2)
    times, keys = gentle_clip(parents, 3, 112)
    rest, idx, bones, weights, _ = K.case("convex", 257, 4, n, 113)
    inst = [(0, None), (0, random_xforms(2, 114, spread=3.0)[1])]
    sc, gm = own_scene(capi, gpu, [(rest, idx)], inst)
    gm[0].set_skin(bones, weights, n)
    rest2, idx2, bones2, weights2, _ = K.case("wild", 65, 2, n, 115)
    second = capi.Model(gpu, rest2, idx2)
    second.set_skin(bones2, weights2, n)
    sk = capi.Skeleton(gpu, parents, ib)
    clip = sk.add_clip(times, keys)
    mats = [T.default_material() for _ in inst]
    env = scenes.sky_cubemap(8)
    cam = np.array([0, 2, 16, 0, 0, 0, 0, 1, 0, 0.8, W / H], np.float32)
    pfcs = frames_of(capi, cam, 3, W, H)
    p = pipeline_over(capi, gpu, sc, mats, env)
    p.update(pfcs[0]); p.render()                        # (the rest pose: what the pipeline has cached is of another mesh)
    old = None
    for step, t in enumerate((0.2, 0.85)):
        sk.set_time(clip, t)
        gm[0].set_bones_from(sk)
        second.set_bones_from(sk)
        sc.update()
        _, M = S.posed(parents, ib, S.sampled(times, keys, t))
        new = K.skinned(rest, bones, weights, M)
        assert new.tobytes() != (rest if old is None else old).tobytes()
        what = "step %d, t %g" % (step, t)
        assert_vertices(gm[0].geometry()[0], new, what)
        assert_vertices(second.geometry()[0], K.skinned(rest2, bones2, weights2, M), what + ", the second model")
        check(capi, gpu, oracle, sc, gm, [(new, idx)], inst, what)
        p.clear_output()
        p.update(pfcs[1 + step]); p.render()
        osc = make_oracle_scene(oracle, [(new, idx)], inst)
        acc, ost = osc.render(np.stack(mats), pfcs[1 + step], W, H, accum=np.zeros((H, W, 4), np.float32), env_faces=env, nthreads=8)
        assert ost["primary_hits"] > 50, "the frame shows next to nothing of the character"
        assert_frame(p, acc, ost, what)
        old = new
    p.close()
    second.close()
    close_all(sc, gm)
    sk.close()
