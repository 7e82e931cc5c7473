"""Blended and layered clips (rt_skeleton_set_blend + rt_skeleton_add_mask): the local pose, the world matrices and the palette the device
leaves are, byte for byte, the definition of include/dxr_amd.h "Posed skeletons", "blending", restated in numpy
(tests/skeleton_blend_cases.py) -- one layer against rt_skeleton_set_time, 2, 3 and 8 layers of mixed modes, masks and weights on both sides
of a wave, of a block and of the LDS limit, 65536 joints, both shortest-path branches, the (0, 0, 0, 1) branch, the pose the skeleton holds as
the base; masks and their ids; every refusal with its message, and nothing changed by it; through the skin end to end and through attached
instances; the example.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import skeleton_blend_cases as B
import skeleton_cases as S
import skin_cases as K
from dxrexperiments_amd import rtypes as T, scenes
from test_gpu_batch import frames_of
from test_gpu_model_deform import RAYS, all_arrays, assert_frame, check, close_all, own_scene
from test_gpu_model_skin import assert_vertices
from test_gpu_pipeline import make_oracle_scene
from test_gpu_scene_update import arrays, assert_bytes_equal
from test_gpu_skeleton import assert_floats, assert_posed, gentle_clip, skinned_model
from util import random_xforms, triangle_soup

pytestmark = pytest.mark.gpu

F = np.float32
LDS = S.lds_joints()
COUNTS = (1, 63, 64, 65, 255, 256, 257, LDS, LDS + 1)
IDENTITY_Q = np.array([0, 0, 0, 1], F)


def skeleton_with(capi, gpu, parents, ib, clips, masks=()):
    sk = capi.Skeleton(gpu, parents, ib)
    assert [sk.add_clip(t, k) for t, k in clips] == list(range(len(clips)))
    assert [sk.add_mask(m) for m in masks] == list(range(len(masks))) and sk.n_masks() == len(masks)
    return sk


def assert_blend(sk, parents, ib, clips, masks, layers, what, current=None, nans=False):
    """set_blend(layers), then read_pose, read_joints and read_palette against the restatement; returns the numpy pose"""
    want = B.blended(clips, masks, layers, current)
    sk.set_blend(layers)
    assert_posed(sk, parents, ib, want, what, nans)
    return want


# ---- one layer is set_time -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 2, 3, 17])
def test_one_layer_equals_set_time(gpu, capi, n_keys):
    """257 joints; t below the first key, on every key, inside every segment, just before the next key, beyond the last and at -inf / +inf:
    set_blend([(clip, t)]) leaves the pose, the joints and the palette that set_time(clip, t) leaves on a second skeleton -- and the
    restatement's; unit keys and keys with a NaN and an inf"""
    n = 257
    parents = S.hierarchy("random", n, 30)
    ib = S.inverse_binds(n, 31)
    for c, family in enumerate(("unit", "nan_inf")):
        clip = S.clip(parents, n_keys, 40 + 100 * c + n_keys, family)
        a, b = skeleton_with(capi, gpu, parents, ib, [clip]), skeleton_with(capi, gpu, parents, ib, [clip])
        for t in S.sample_times(clip[0]):
            what = "K %d, %s keys, t %r" % (n_keys, family, float(t))
            a.set_blend([(0, float(t))])
            b.set_time(0, float(t))
            for name in ("pose", "joints", "palette"):
                assert_floats(getattr(a, name)(), getattr(b, name)(), "%s: %s" % (what, name), nans=family == "nan_inf")
            assert_floats(a.pose(), S.sampled(*clip, t), what + ": the restatement", nans=family == "nan_inf")
        a.close(); b.close()


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_blend_is_its_definition(gpu, capi, n):
    """n = 1, 63 / 64 / 65 (both sides of a wave), 255 / 256 / 257 (both sides of the kernel's block), RT_SKELETON_LDS_JOINTS and one more
    (the pose behind the blend from LDS and from global memory); clips of 1, 2, 3 and 17 keys, unit and raw (zero quaternions); 2, 3 and 8
    layers of both modes, masked and not, the weights from {0, 0.25, 1, -0.5, 1.5}; one mask is arange(n) / n"""
    parents = S.hierarchy("random", n, 200 + n)
    ib = S.inverse_binds(n, 201 + n)
    clips = [S.clip(parents, k, 210 + 10 * k + n, family) for k, family in ((1, "unit"), (2, "raw"), (3, "unit"), (17, "unit"))]
    masks = B.masks_for(n, 220 + n)
    assert masks[0].tobytes() == (np.arange(n) / n).astype(F).tobytes()
    sk = skeleton_with(capi, gpu, parents, ib, clips, masks)
    differ = 0
    for n_layers in (2, 3, 8):
        for seed in range(3):
            layers = B.layer_list(n_layers, clips, len(masks), 1000 * n + 10 * n_layers + seed)
            want = assert_blend(sk, parents, ib, clips, masks, layers, "%d joints, %d layers, list %d" % (n, n_layers, seed))
            differ += want.tobytes() != B.blended(clips, masks, layers[:1]).tobytes()
            assert np.isfinite(want).all()
    assert differ > 0, "no list did more than its base layer"
    # the mask's entry is the joint's own: layer 1 alone, masked by arange(n) / n, weight 1
    layers = [(0, 0.0), (2, float(clips[2][0][1]), 1.0, 0, B.BLEND)]
    want = assert_blend(sk, parents, ib, clips, masks, layers, "%d joints, the index mask" % n)
    if n > 1:
        base, ts = B.blended(clips, masks, layers[:1]), [0, 1, 2, 7, 8, 9]
        assert want[0, ts].tobytes() == base[0, ts].tobytes() and want[n - 1, ts].tobytes() != base[n - 1, ts].tobytes()
    sk.close()


def test_65536_joints_8_layers(gpu, capi):
    """the limit: 65536 joints of a random tree, the pose from global memory, eight layers of both modes, three of them masked"""
    n = 65536
    parents = S.hierarchy("random", n, 9)
    ib = S.inverse_binds(n, 10)
    clips = [S.clip(parents, k, 300 + k) for k in (1, 2, 3)]
    masks = B.masks_for(n, 310)
    sk = skeleton_with(capi, gpu, parents, ib, clips, masks)
    layers = B.layer_list(8, clips, len(masks), 4)
    assert sum(l[3] is not None for l in layers) >= 3 and {l[4] for l in layers[1:]} == {B.BLEND, B.ADDITIVE}
    assert_blend(sk, parents, ib, clips, masks, layers, "65536 joints, 8 layers")
    sk.close()


# ---- the branches ------------------------------------------------------------------------------------------------------------------------
def test_both_shortest_paths(gpu, capi):
    """RT_LAYER_BLEND with d < 0: the layer's quaternion is the negation of the accumulated one, it is negated back and the pose stays where
    it was for every weight (up to the normalisation); the same rotation nearly, the other sign, stays beside the base instead of passing
    through the origin.  RT_LAYER_ADDITIVE with D_w < 0: the clip's second key is its first turned by 2 rad of quaternion angle, D is
    negated, and the base turns the short way"""
    n = 65
    parents = S.hierarchy("roots", n, 50)
    ib = S.inverse_binds(n, 51)
    rng = np.random.default_rng(52)
    a = S.pose("unit", parents, 53)
    neg = a.copy()
    neg[:, 3:7] = -a[:, 3:7]
    near = a.copy()
    near[:, 3:7] = -(a[:, 3:7] + rng.normal(scale=0.05, size=(n, 4)).astype(F))
    turn = np.tile(np.array([np.sin(2.0), 0, 0, np.cos(2.0)], F), (n, 1))
    turned = a.copy()
    turned[:, 3:7] = B.hamilton(a[:, 3:7], turn)
    one = np.array([0.0], F)
    clips = [(one, a[None]), (one, neg[None]), (one, near[None]), (np.array([0.0, 1.0, 2.0], F), np.stack([a, turned, turned]))]
    sk = skeleton_with(capi, gpu, parents, ib, clips)
    base = S.sampled(*clips[0], 0.0)
    for w in (0.25, 0.5, 1.0, 1.5):
        want = assert_blend(sk, parents, ib, clips, [], [(0, 0.0), (1, 0.0, w)], "S = -P, weight %g" % w)
        assert np.abs(want.astype(np.float64) - base).max() < 1e-6, "the restatement left the pose"
        want = assert_blend(sk, parents, ib, clips, [], [(0, 0.0), (2, 0.0, w)], "S nearly -P, weight %g" % w)
        assert ((want[:, 3:7].astype(np.float64) * base[:, 3:7]).sum(axis=1) > 0.95).all(), "the restatement went the long way round"
    R, Sk = S.sampled(*clips[3], -np.inf), S.sampled(*clips[3], 1.0)
    assert (B.hamilton(B.conj(R[:, 3:7]), Sk[:, 3:7])[:, 3] < -0.3).all(), "D_w is not negative"
    for w in (0.25, 1.0):
        want = assert_blend(sk, parents, ib, clips, [], [(0, 0.0), (3, 1.0, w, None, B.ADDITIVE)], "D_w < 0, weight %g" % w)
        # the short way: by pi - 2 rad of quaternion angle at weight 1, not by 2
        if w == 1.0:
            assert np.abs(np.abs((want[:, 3:7].astype(np.float64) * base[:, 3:7]).sum(axis=1)) - np.cos(np.pi - 2.0)).max() < 1e-5
    sk.close()


def test_the_fallback_and_what_is_not_finite(gpu, capi):
    """n = 0 and n not finite give (0, 0, 0, 1): zero quaternions blended with zero quaternions, lengths whose squares overflow, inf and NaN
    weights; keys with a NaN and an inf in both modes; a NaN d negates nothing.  NaNs stand where the restatement has them"""
    n = 257
    parents = S.hierarchy("random", n, 60)
    ib = S.inverse_binds(n, 61)
    unit = S.clip(parents, 2, 62)
    zero = S.clip(parents, 2, 63)
    zero[1][:, ::2, 3:7] = 0.0
    huge = S.clip(parents, 2, 64)
    huge[1][:, :, 3:7] *= F(1e30)
    bad = S.clip(parents, 3, 65, "nan_inf")
    clips = [unit, zero, huge, bad]
    masks = B.masks_for(n, 66)
    sk = skeleton_with(capi, gpu, parents, ib, clips, masks)
    t = float(unit[0][0]) + 0.3
    want = assert_blend(sk, parents, ib, clips, masks, [(1, t), (1, t, 0.5)], "zero quaternions")
    assert (want[::2, 3:7] == IDENTITY_Q).all()
    for w in (np.inf, -np.inf, np.nan):
        for mode in (B.BLEND, B.ADDITIVE):
            want = assert_blend(sk, parents, ib, clips, masks, [(0, t), (0, t + 0.2, w, None, mode)], "weight %r, mode %d" % (w, mode), nans=True)
            if mode == B.BLEND:                           # (added, such a weight leaves E without a length: E is (0, 0, 0, 1) and the rotation stays)
                assert (want[:, 3:7] == IDENTITY_Q).all(), "a blend weight that is not finite leaves (0, 0, 0, 1)"
    # an inf weight under the 0 / 1 mask: w = inf * 0 is NaN there
    want = assert_blend(sk, parents, ib, clips, masks, [(0, t), (0, t + 0.2, np.inf, 1, B.BLEND)], "inf * mask", nans=True)
    assert np.isnan(want[masks[1] == 0, 0]).all()
    assert (S.sampled(*huge, t)[:, 3:7] == IDENTITY_Q).all()
    for mode in (B.BLEND, B.ADDITIVE):
        want = assert_blend(sk, parents, ib, clips, masks, [(0, t), (2, t, 0.5, None, mode)], "a clip whose samples are (0, 0, 0, 1), mode %d" % mode)
        for tb in (float(bad[0][0]), float(bad[0][1]) + 0.1):
            want = assert_blend(sk, parents, ib, clips, masks, [(0, t), (3, tb, 0.5, 0, mode), (0, t, 0.25)], "poisoned keys at %g, mode %d" % (tb, mode), nans=True)
            j_nan, j_inf = S.poisoned(parents)
            assert not np.isfinite(want[[j_nan, j_inf]]).all(axis=1).any() and np.isfinite(np.delete(want, [j_nan, j_inf], axis=0)).all()
    # a NaN d: the base holds a NaN quaternion component, the layer is on the other side -- nothing is negated, and n is NaN: (0, 0, 0, 1)
    cur = S.sampled(*unit, t)
    cur[5, 4] = np.nan
    sk.set_pose(cur)
    want = assert_blend(sk, parents, ib, clips, masks, [(None, 0.0), (0, t, 0.5)], "a NaN d", current=cur, nans=True)
    assert (want[5, 3:7] == IDENTITY_Q).all()
    # the blend's own n = 0 and n = inf: the pose the skeleton holds has a zero quaternion (weight 0 leaves it zero) and one of length 1e30
    cur = S.sampled(*unit, t)
    cur[7, 3:7] = 0.0
    cur[9, 3:7] *= F(1e30)
    sk.set_pose(cur)
    want = assert_blend(sk, parents, ib, clips, masks, [(None, 0.0), (0, t, 0.0)], "n = 0 and n = inf in the blend", current=cur)
    assert (want[[7, 9], 3:7] == IDENTITY_Q).all() and not (want[8, 3:7] == IDENTITY_Q).all()
    sk.close()


def test_the_pose_the_skeleton_holds_is_a_base(gpu, capi):
    """RT_SKELETON_CURRENT_POSE: after set_pose of a raw pose (quaternions that are not unit, a fifth of them zero) a blend of 0.5 towards a
    clip is the restatement started from that pose, as it stands; once more from what the blend left; alone it leaves the pose bit for bit
    and counts as a pose"""
    n = 300
    parents = S.hierarchy("random", n, 70)
    ib = S.inverse_binds(n, 71)
    clips = [S.clip(parents, 3, 72), S.clip(parents, 2, 73)]
    masks = B.masks_for(n, 74)
    sk = skeleton_with(capi, gpu, parents, ib, clips, masks)
    raw = S.pose("raw", parents, 75)
    sk.set_pose(raw)
    t = float(clips[0][0][1]) + 0.1
    first = assert_blend(sk, parents, ib, clips, masks, [(None, 0.0), (0, t, 0.5)], "from a raw pose", current=raw)
    assert first.tobytes() != raw.tobytes()
    second = assert_blend(sk, parents, ib, clips, masks, [(None, 0.0, 7.0, 2), (1, 0.1, 0.5, 0), (0, t, 0.25, None, "additive")], "from the last blend", current=first)
    assert_blend(sk, parents, ib, clips, masks, [(None,)], "alone", current=second)
    assert sk.pose().tobytes() == second.tobytes()
    sk.close()


# ---- masks ---------------------------------------------------------------------------------------------------------------------------------
def test_masks_and_their_ids(gpu, capi):
    """two masks keep their ids after a third is added; clear_masks restarts the ids and leaves the pose; after clear_clips a blend is
    RT_ERR_STATE"""
    n = 64
    parents = S.hierarchy("random", n, 80)
    ib = S.inverse_binds(n, 81)
    clips = [S.clip(parents, 3, 82), S.clip(parents, 2, 83)]
    masks = B.masks_for(n, 84)
    sk = skeleton_with(capi, gpu, parents, ib, clips, masks[:2])
    t = float(clips[0][0][1])
    lists = [[(0, t), (1, 0.2, 0.75, m, mode)] for m in (0, 1) for mode in (B.BLEND, B.ADDITIVE)]
    for layers in lists:
        assert_blend(sk, parents, ib, clips, masks, layers, "two masks")
    assert sk.add_mask(masks[2]) == 2 and sk.n_masks() == 3
    for layers in lists + [[(0, t), (1, 0.2, 0.75, 2)]]:
        assert_blend(sk, parents, ib, clips, masks, layers, "after a third mask")
    last = sk.palette()
    sk.clear_masks()
    assert sk.n_masks() == 0 and sk.palette().tobytes() == last.tobytes() and sk.info()[2] == 2
    with pytest.raises(capi.RtError, match="layer 1 names mask 0: the skeleton has 0") as e:
        sk.set_blend(lists[0])
    assert e.value.code == -4
    sk.clear_masks()                                      # (nothing to clear: fine)
    assert sk.add_mask(masks[2]) == 0
    assert_blend(sk, parents, ib, clips, [masks[2]], [(0, t), (1, 0.2, 0.75, 0)], "after clear_masks")
    last = sk.pose()
    sk.clear_clips()
    with pytest.raises(capi.RtError, match="layer 0 names clip 0: the skeleton has 0") as e:
        sk.set_blend([(0, t), (1, 0.2, 0.75, 0)])
    assert e.value.code == -4
    assert sk.pose().tobytes() == last.tobytes() and sk.n_masks() == 1
    sk.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_messages(gpu, capi):
    """every refusal with its code and its message, which names the layer; a refused call changes nothing: read_pose returns the same bytes,
    and the pose counter stands -- a scene with an instance attached to the skeleton stays built and traceable, and its next update is the
    no-op of "nothing pending" (the time of the last real update stands, the arrays are what they were)"""
    lib = capi.lib()
    n = 7
    parents = S.hierarchy("random", n, 90)
    ib = S.inverse_binds(n, 91)
    clips = [S.clip(parents, 3, 92), S.clip(parents, 1, 93)]
    masks = B.masks_for(n, 94)[:2]
    sk = skeleton_with(capi, gpu, parents, ib, clips, masks)
    ok = (0, 0.5, 1.0, None, B.BLEND)
    with pytest.raises(capi.RtError, match=r"layer 0 names RT_SKELETON_CURRENT_POSE: the skeleton has no pose yet \(rt_skeleton_set_pose") as e:
        sk.set_blend([(None,), ok])
    assert e.value.code == -4
    with pytest.raises(capi.RtError, match="rt_skeleton_set_pose"):
        sk.pose()                                        # (the refused blend posed nothing)
    m = capi.Model(gpu, *triangle_soup(4, seed=3, extent=1.0, size=0.5))
    sc = capi.Scene(gpu)
    for x in random_xforms(2, 95, spread=3.0):
        sc.add_model(m, x)
    sc.build()
    sc.attach(0, sk, [2, 5])
    sk.set_blend([ok, (1, 0.0, 0.5, 1, B.ADDITIVE)])
    sc.update()
    before, pose, ms = arrays(sc, 2), sk.pose(), sc.update_ms()
    nan = float("nan")
    refusals = [
        ([], -1, r"0 layers: 1 \.\. 8 are supported"),
        ([ok] * 9, -1, r"9 layers: 1 \.\. 8 are supported"),
        ([ok, (0, nan, 1.0)], -1, "the time of layer 1 is NaN"),
        ([(0, nan)], -1, "the time of layer 0 is NaN"),
        ([ok, ok, (0, 0.0, 1.0, None, 2)], -1, "layer 2 has mode 2"),
        ([(0, 0.0, 1.0, None, B.ADDITIVE), ok], -1, "layer 0 is additive"),
        ([ok, ok, ok, (None, 0.0, 1.0)], -1, "layer 3 names RT_SKELETON_CURRENT_POSE: only layer 0 may"),
        ([(2, 0.0), ok], -4, r"layer 0 names clip 2: the skeleton has 2 \(rt_skeleton_add_clip"),
        ([ok] * 7 + [(7, 0.0, 1.0)], -4, "layer 7 names clip 7: the skeleton has 2"),
        ([ok, (1, 0.0, 1.0, 2)], -4, r"layer 1 names mask 2: the skeleton has 2 \(rt_skeleton_add_mask"),
        ([(5, 0.0), (0, nan, 1.0)], -1, "the time of layer 1 is NaN"),           # an argument's refusal comes before a state's
    ]
    for layers, code, message in refusals:
        with pytest.raises(capi.RtError, match=message) as e:
            sk.set_blend(layers)
        assert e.value.code == code, message
        assert "rt_skeleton_set_blend" in str(e.value)
    one = capi.Skeleton.layers([ok])
    assert lib.rt_skeleton_set_blend(sk.h, 1, None) == -1 and b"null" in lib.rt_last_error()
    assert lib.rt_skeleton_set_blend(None, 1, one.ctypes.data_as(C.c_void_p)) == -1 and lib.rt_skeleton_add_mask(sk.h, None, None) == -1
    assert lib.rt_skeleton_get_num_masks(sk.h, None) == -1
    with pytest.raises(capi.RtError, match="6 weights for a skeleton of 7"):
        sk.add_mask(np.zeros(6, F))
    # the base layer's weight, mask and (for the pose the skeleton holds) time are not read: no refusal
    assert sk.pose().tobytes() == pose.tobytes() and sk.n_masks() == 2 and sk.info()[2] == 2
    sc.trace(*RAYS)
    sc.update()
    assert sc.update_ms() == ms, "a refused blend counted as a pose: the scene's update was no no-op"
    assert_bytes_equal(arrays(sc, 2), before, "after the refusals")
    assert_blend(sk, parents, ib, clips, masks, [(None, nan, nan, 9), ok], "the base layer's weight, mask and time are not read", current=pose)
    sc.trace(*RAYS)                                      # (a pose alone leaves the scene built)
    sc.update()
    assert sc.update_ms() != ms or arrays(sc, 2)["invs"].tobytes() != before["invs"].tobytes(), "a blend counts as a pose"
    sc.close(); m.close(); sk.close()


# ---- through the skin, end to end ------------------------------------------------------------------------------------------------------------
W, H = 64, 64


def test_a_blended_character_end_to_end(gpu, capi, oracle):
    """a 257-vertex model of skin_cases, 4 influences, bones = the 7 joints of a random tree, two instances; per step a three-layer blend (a
    cross-fade and a masked additive layer) + set_bones_from + rt_scene_update: the vertices == skin_cases.skinned over skeleton_cases.posed
    over the numpy blend, byte for byte; the scene == a fresh build over a fresh model of those vertices, array for array, and the oracle's;
    one frame, 64 x 64, == the oracle's"""
    n = 7
    parents = S.hierarchy("random", n, 110)
    ib = K.gentle_palette(n, 111, angle=0.2, spread=0.2)
    clips = [gentle_clip(parents, 3, 112), gentle_clip(parents, 4, 116), gentle_clip(parents, 2, 117)]
    masks = [np.array([0, 0, 0.5, 1, 1, 0.25, 1], F)]
    rest, idx, bones, weights, _ = K.case("convex", 257, 4, n, 113)
    inst = [(0, None), (0, random_xforms(2, 114, spread=3.0)[1])]
    sc, gm = own_scene(capi, gpu, [(rest, idx)], inst)
    gm[0].set_skin(bones, weights, n)
    sk = skeleton_with(capi, gpu, parents, ib, clips, masks)
    mats = [T.default_material() for _ in inst]
    env = scenes.sky_cubemap(8)
    cam = np.array([0, 2, 16, 0, 0, 0, 0, 1, 0, 0.8, W / H], F)
    pfcs = frames_of(capi, cam, 3, W, H)
    p = capi.Pipeline(gpu)
    p.set_scene(sc)
    for mat in mats:
        p.add_material(mat)
    p.set_environment_cube(env)
    p.create_output(W, H)
    p.build_acceleration_structures()
    p.update(pfcs[0]); p.render()                        # (the rest pose: what the pipeline has cached is of another mesh)
    old = None
    for step, (t, fade) in enumerate(((0.2, 0.25), (0.85, 0.75))):
        layers = [(0, t), (1, 1.2 - t, fade), (2, 0.3 + t, 1.0, 0, "additive")]
        sk.set_blend(layers)
        gm[0].set_bones_from(sk)
        sc.update()
        trs = B.blended(clips, masks, layers)
        assert_floats(sk.pose(), trs, "step %d: pose" % step)
        _, M = S.posed(parents, ib, trs)
        new = K.skinned(rest, bones, weights, M)
        assert new.tobytes() != (rest if old is None else old).tobytes()
        what = "step %d, t %g" % (step, t)
        assert_vertices(gm[0].geometry()[0], new, what)
        check(capi, gpu, oracle, sc, gm, [(new, idx)], inst, what)
        p.clear_output()
        p.update(pfcs[1 + step]); p.render()
        osc = make_oracle_scene(oracle, [(new, idx)], inst)
        acc, ost = osc.render(np.stack(mats), pfcs[1 + step], W, H, accum=np.zeros((H, W, 4), F), env_faces=env, nthreads=8)
        assert ost["primary_hits"] > 50, "the frame shows next to nothing of the character"
        assert_frame(p, acc, ost, what)
        old = new
    p.close()
    close_all(sc, gm)
    sk.close()


def test_attached_instances_follow_a_blend(gpu, capi):
    """instances attached to two joints, one with a local matrix's worth each: after set_blend + rt_scene_update their transforms are
    W_joint o local of the numpy blend, bit for bit, the third instance's as it was; and again after another blend"""
    n = 9
    parents = S.hierarchy("random", n, 120)
    ib = S.inverse_binds(n, 121)
    clips = [S.clip(parents, 3, 122), S.clip(parents, 2, 123)]
    masks = B.masks_for(n, 124)
    sk = skeleton_with(capi, gpu, parents, ib, clips, masks)
    m = capi.Model(gpu, *triangle_soup(4, seed=3, extent=1.0, size=0.5))
    start = random_xforms(3, 125, spread=3.0)
    sc = capi.Scene(gpu)
    for x in start:
        sc.add_model(m, x)
    sc.build()
    joints, local = np.array([8, 3], np.uint32), random_xforms(2, 126, spread=2.0)
    sc.attach(0, sk, joints, local)
    for step, layers in enumerate(([(0, 0.3), (1, 0.2, 0.5, 0), (0, 0.9, 0.25, None, "additive")], [(None,), (1, 0.4, 1.5, 2)])):
        current = sk.pose() if step else None
        trs = B.blended(clips, masks, layers, current)
        sk.set_blend(layers)
        sc.update()
        Wm, _ = S.posed(parents, ib, trs)
        want = np.concatenate([S.compose(Wm[joints.astype(np.int64)], local), start[2:3]])
        assert_floats(sc.transforms(), want, "step %d: the transforms" % step)
        assert sc.attachment(0) is not None and sc.attachment(2) is None
    sc.close(); m.close(); sk.close()


# ---- the example -------------------------------------------------------------------------------------------------------------------------------
def test_blend_example_through_the_cpp_mirror(tmp_path):
    """examples/realtime_blend.cpp: RtSkeleton::create + addClip + addMask once, RtSkeleton::setBlend + RtModel::setBones(skeleton) +
    RtScene::update per frame, end to end; after three frames the image is another than after one; blended on the host from read-back
    samples, the way there was before, the frame is the same frame"""
    exe = os.path.join(K.ROOT, "dxrexperiments_amd", "lib", "realtime_blend")
    images = []
    for frames, where in ((1, "device"), (3, "device"), (3, "host")):
        out = tmp_path / ("out%d%s.pfm" % (frames, where))
        r = subprocess.run([exe, "96", "64", str(frames), str(out)] + (["host"] if where == "host" else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        assert "1536 skinned vertices, 2976 triangles, 4 joints, 3 clips, 3 layers, blended on the %s: %d frames" % (where, frames) in r.stdout and "BLAS + TLAS update" in r.stdout
        raw = out.read_bytes()
        head = b"PF\n96 64\n-1.0\n"
        assert raw.startswith(head)
        images.append(np.frombuffer(raw[len(head):], "<f4").reshape(64, 96, 3))
    assert images[0].max() > 0.1 and images[0].std() > 0.01            # an image, not a constant
    assert not np.array_equal(images[0], images[1])
    assert np.array_equal(images[1], images[2]), "the host's blend of the read-back samples is another pose"
