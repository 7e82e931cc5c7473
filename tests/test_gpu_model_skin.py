"""Skeletal animation (rt_model_set_skin + rt_model_set_bones + rt_scene_update): the vertices the device writes from a rest pose and a bone
palette are, byte for byte, the definition of DESIGN.md section 2 restated in numpy (tests/skin_cases.py) -- every influence count, both sides
of a wave and of a block, both palette paths at their edge, host and device palettes, every weight family; every pose starts from the rest
pose; and a scene after `set_bones + update` is, array for array, the scene a fresh build over FRESH models of the skinned arrays gives,
byte-equal to such a second GPU scene and equal to the oracle's, which is built fresh.  Then traversal, whole frames through pipelines that
had cached what the rest pose looked like, and the states in between.  No tolerance anywhere."""
import os
import subprocess
import types

import numpy as np
import pytest

import s2_truth as S
import skin_cases as K
from dxrexperiments_amd import rtypes as T, scenes
from test_gpu_batch import frames_of
from test_gpu_instance_transforms import COUNTS, two_models
from test_gpu_model_deform import (RAYS, all_arrays, assert_frame, check, close_all, instances_of, own_scene, pipeline_over, stale_calls,
                                   unsplit_grid)
from test_gpu_option_matrix import BUILD_ROWS, context
from test_gpu_pipeline import make_oracle_scene
from test_gpu_scene_update import assert_bytes_equal, box_meshes, light_scene
from test_gpu_trace import compare_all
from util import Pair, random_xforms

pytestmark = pytest.mark.gpu

W, H = 96, 64
LDS = K.lds_bones()
BONES = {"1": 1, "3": 3, "lds": LDS, "lds+1": LDS + 1}


def pose(ctx, model, palette, device=False):
    """set_bones from a host array, or from device memory (Context.upload)"""
    if not device:
        model.set_bones(palette)
        return
    buf = ctx.upload(np.ascontiguousarray(palette, np.float32))
    model.set_bones_device(buf.ptr)
    ctx.synchronize()
    buf.close()


def assert_vertices(got, want, what, nans=False):
    """byte for byte; nans: sign and payload of a NaN are the hardware's (skin_cases.canonical_nans), where one stands is not"""
    assert got.dtype == want.dtype == T.VERTEX and got.shape == want.shape
    for field in ("position", "normal"):
        g, w = got[field], want[field]
        if nans:
            assert np.array_equal(np.isnan(g), np.isnan(w)), "%s: %s: NaNs stand elsewhere" % (what, field)
            g, w = K.canonical_nans(g), K.canonical_nans(w)
        assert g.tobytes() == w.tobytes(), "%s: %d %ss differ" % (what, int((g.view(np.uint32) != w.view(np.uint32)).any(axis=1).sum()), field)


# ---- the definition --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bones", list(BONES))
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_skinned_vertices_are_their_definition(gpu, capi, k, n_bones):
    """V = 1 (one lane), 63 / 64 / 65 (both sides of a wave), 257 (both sides of a block), 901; n_bones = 1, 3, RT_SKIN_LDS_BONES (the last
    palette staged into LDS) and one more (the first gathered from global memory), the largest index in use; every weight family; the palette
    from a host array, then from device memory on the same model (the second pose starts from the rest pose as well)"""
    nb = BONES[n_bones]
    seed = 1000 * k + nb
    for nv in (1, 63, 64, 65, 257, 901):
        for family in K.FAMILIES:
            seed += 1
            rest, idx, bones, weights, palette = K.case(family, nv, k, nb, seed)
            assert bones.max() == nb - 1 and bones.shape == weights.shape == (nv, k)
            want = K.skinned(rest, bones, weights, palette)
            what = "K %d, %d bones, %d vertices, %s" % (k, nb, nv, family)
            if family == "nan_inf":
                assert np.isnan(want["position"]).any() and np.isinf(want["position"]).any(), what
            else:
                assert np.isfinite(want["position"]).all() and np.isfinite(want["normal"]).all(), what
            m = capi.Model(gpu, rest, idx)
            m.set_skin(bones, weights, nb)
            assert m.skin() == (k, nb)
            assert m.geometry()[0].tobytes() == rest.tobytes(), what + ": set_skin changed the vertices"
            for device in (False, True):
                pose(gpu, m, palette, device)
                assert_vertices(m.geometry()[0], want, what + (", device palette" if device else ", host palette"), nans=family == "nan_inf")
                if not device:
                    m.set_vertices(np.zeros(nv, T.VERTEX))          # (so that vertices the second pose did not write show)
            assert np.array_equal(m.geometry()[1], idx)
            m.close()


def test_what_the_families_are_there_for():
    """the cases are what they say: exact zeros of both signs, negative weights and sums far from 1, -0 rest coordinates, bones that repeat"""
    w = K.random_weights(901, 4, 3, "zeros")
    assert (w == 0).any() and np.signbit(w[w == 0]).any() and not np.signbit(w[w == 0]).all() and (w.sum(axis=1) > 0.99).all()
    w = K.random_weights(901, 4, 3, "wild")
    assert (w < 0).any() and (np.abs(w.sum(axis=1) - 1) > 0.5).any()
    w = K.random_weights(901, 4, 3, "one_hot")
    assert set(np.unique(w).tolist()) == {0.0, 1.0} and (w.sum(axis=1) == 1).all()
    rest, _ = K.rest_pose(901, 3, neg_zero=True)
    assert (np.signbit(rest["position"]) & (rest["position"] == 0)).any() and (np.signbit(rest["normal"]) & (rest["normal"] == 0)).any()
    b = K.random_bones(901, 8, 3, 1)
    assert (np.sort(b, axis=1)[:, 1:] == np.sort(b, axis=1)[:, :-1]).any()
    # a uniform scale and a rotation leave a unit normal a unit normal, turned by the rotation: the linear part is enough
    rest, _ = K.rest_pose(65, 4)
    out = K.skinned(rest, np.zeros((65, 1), np.uint32), np.ones((65, 1), np.float32), K.random_palette(1, 8))
    assert np.allclose(np.linalg.norm(out["normal"].astype(np.float64), axis=1), 1.0, atol=1e-6)


# ---- the rest pose -----------------------------------------------------------------------------------------------------------------------
def test_every_pose_starts_from_the_rest_pose(gpu, capi):
    nv, k, nb = 901, 4, 7
    rest, idx, bones, weights, pal_a = K.case("convex", nv, k, nb, 77)
    pal_b = K.random_palette(nb, 78)
    m = capi.Model(gpu, rest, idx)
    m.set_skin(bones, weights, nb)
    a, b = K.skinned(rest, bones, weights, pal_a), K.skinned(rest, bones, weights, pal_b)
    assert a.tobytes() != b.tobytes() and b.tobytes() != K.skinned(a, bones, weights, pal_b).tobytes()
    # pose A, then pose B: B of the rest pose, not of A
    pose(gpu, m, pal_a)
    assert_vertices(m.geometry()[0], a, "pose A")
    pose(gpu, m, pal_b, device=True)
    assert_vertices(m.geometry()[0], b, "pose B after pose A")
    # set_vertices / set_positions between two poses write the current vertices and leave the rest pose alone
    scribble = rest.copy()
    scribble["position"] += np.float32(3.0)
    m.set_vertices(scribble)
    assert m.geometry()[0].tobytes() == scribble.tobytes()
    m.set_positions(rest["position"][:100] * np.float32(2.0), 5)
    pose(gpu, m, pal_a)
    assert_vertices(m.geometry()[0], a, "pose A after set_vertices / set_positions")
    # set_skin again: the vertices as they are -- pose A -- are the new rest pose (and the new skin is another: K = 2, other bones)
    bones2, weights2 = K.random_bones(nv, 2, nb, 80), K.random_weights(nv, 2, 81)
    m.set_skin(bones2, weights2, nb)
    assert m.skin() == (2, nb)
    assert_vertices(m.geometry()[0], a, "set_skin again")
    pose(gpu, m, pal_b)
    assert_vertices(m.geometry()[0], K.skinned(a, bones2, weights2, pal_b), "pose B over the new rest pose A")
    # clear_skin: the vertices are the last pose; set_bones has nothing to work with
    last = m.geometry()[0]
    m.clear_skin()
    assert m.skin() == (0, 0)
    with pytest.raises(capi.RtError, match="rt_model_set_skin") as e:
        m.set_bones(pal_b)
    assert e.value.code == -4
    buf = gpu.upload(pal_b)
    with pytest.raises(capi.RtError, match="rt_model_set_skin") as e:
        m.set_bones_device(buf.ptr)
    assert e.value.code == -4
    buf.close()
    assert m.geometry()[0].tobytes() == last.tobytes()
    m.clear_skin()                                       # (twice is once)
    m.close()


def test_refused_skins_and_palettes(gpu, capi):
    """refused, and nothing changes: the skin the model has stays, its vertices stay"""
    nv, k, nb = 65, 2, 3
    rest, idx, bones, weights, palette = K.case("convex", nv, k, nb, 5)
    m = capi.Model(gpu, rest, idx)
    lib = capi.lib()
    pb, pw, pp = bones.ctypes.data, weights.ctypes.data, palette.ctypes.data
    with pytest.raises(capi.RtError, match="rt_model_set_skin"):
        m.set_bones(palette)                            # never had a skin
    m.set_skin(bones, weights, nb)
    bad = bones.copy()
    bad[40, 1] = nb
    with pytest.raises(capi.RtError, match="vertex 40, slot 1") as e:
        m.set_skin(bad, weights, nb)
    assert e.value.code == -1
    for kk, n in ((9, nb), (k, 0), (k, 65537)):
        assert lib.rt_model_set_skin(m.h, kk, n, pb, pw) == -1, (kk, n)
    assert lib.rt_model_set_skin(m.h, k, nb, None, pw) == -1 and lib.rt_model_set_skin(m.h, k, nb, pb, None) == -1
    assert lib.rt_model_set_bones(m.h, None, 0) == -1 and lib.rt_model_set_bones(m.h, pp, 2) == -1
    assert m.skin() == (k, nb) and m.geometry()[0].tobytes() == rest.tobytes()
    pose(gpu, m, palette)
    assert_vertices(m.geometry()[0], K.skinned(rest, bones, weights, palette), "after the refusals")
    m.close()


# ---- update == build ---------------------------------------------------------------------------------------------------------------------
def soup_skin(n_verts, k=4, n_bones=6, seed=60):
    return K.random_bones(n_verts, k, n_bones, seed), K.random_weights(n_verts, k, seed + 1), n_bones


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("count", ["1i", "13"])
def test_update_equals_build(gpu, capi, oracle, count, device):
    """the two soups of test_gpu_scene_update.py, as one identity instance and as 13 instances; model 0 skinned (K = 4, 6 bones) and posed
    twice, an update after each: the scene == a fresh GPU build over fresh models of the numpy vertices == the oracle's; the instances of the
    other model keep their boxes and inverses bit for bit"""
    meshes = list(box_meshes())
    inst = instances_of(count)
    used = [m for j, m in enumerate(meshes) if j in set(mi for mi, _ in inst)]
    sc, gm = own_scene(capi, gpu, used, inst)
    before = all_arrays(sc, gm, inst)
    bones, weights, nb = soup_skin(len(meshes[0][0]))
    gm[0].set_skin(bones, weights, nb)
    for step in range(2):
        palette = K.gentle_palette(nb, 90 + step)
        pose(gpu, gm[0], palette, device)
        sc.update()
        new = K.skinned(meshes[0][0], bones, weights, palette)
        got = check(capi, gpu, oracle, sc, gm, [(new, meshes[0][1])] + used[1:], inst, "%s, pose %d" % (count, step), before, deformed={0})
        assert got["model0.verts"].tobytes() != before["model0.verts"].tobytes() and sc.update_ms() > 0.0
    close_all(sc, gm)


def stretch_palette(n_bones, seed, bone=1):
    """a gentle pose in which one bone stretches 1000 : 1 along (20, 17, 13): what it pulls becomes long diagonal slivers"""
    p = K.gentle_palette(n_bones, seed).reshape(n_bones, 3, 4)
    u = np.array([20.0, 17.0, 13.0]) / np.linalg.norm([20.0, 17.0, 13.0])
    p[bone, :, :3] = (np.eye(3) + 999.0 * np.outer(u, u)).astype(np.float32)
    p[bone, :, 3] = 0
    return p.reshape(n_bones, 12)


def test_split_references_appear_and_disappear(gpu, capi, oracle):
    """a grid none of whose triangles is split, two influences over four bones; a pose with a 1000 : 1 stretch on one bone (split references
    appear: n_recs grows, the buffers with it), the identity pose (they vanish), the stretch again, a gentle pose"""
    v, idx = unsplit_grid()
    inst = [(0, None), (0, random_xforms(2, 3, spread=30.0)[0]), (1, random_xforms(2, 3, spread=30.0)[1])]
    meshes = [(v, idx), box_meshes()[1]]
    sc, gm = own_scene(capi, gpu, meshes, inst)
    assert sc.refs(0)[0] is None, "a triangle of the undeformed grid is split: the case does not start where it says"
    nb = 4
    bones, weights = K.random_bones(len(v), 2, nb, 70), K.random_weights(len(v), 2, 71)
    gm[0].set_skin(bones, weights, nb)
    n_refs = []
    for step, palette in enumerate((stretch_palette(nb, 72), K.identity_palette(nb), stretch_palette(nb, 72), K.gentle_palette(nb, 73))):
        pose(gpu, gm[0], palette, device=step % 2 == 1)
        sc.update()
        new = K.skinned(v, bones, weights, palette)
        got = check(capi, gpu, oracle, sc, gm, [(new, idx), meshes[1]], inst, "stretch step %d" % step)
        off = got["model0.ref_off"]
        n_refs.append(0 if off is None else int(off[-1]))
        if off is not None:
            assert got["model0.counts"][1] == len(got["model0.records"]) > len(idx), "the production layout holds no triangle as several records"
    assert n_refs[0] > len(idx) and n_refs[1] == 0 and n_refs[2] == n_refs[0], n_refs
    close_all(sc, gm)


OPTION_SETS = [{}, {"fail_ploc_rounds": 1}, BUILD_ROWS[1]]


@pytest.mark.parametrize("opts", OPTION_SETS, ids=["default", "ploc_fallback", "build_row_lbvh"])
def test_a_pose_under_builder_options(capi, oracle, opts):
    """the stretch pose on a context with the default options, with PLOC made to give up (the fallback to the LBVH layout), and under the
    BUILD_ROWS row that asks for that layout with one triangle per leaf and batched rounds: five instances of the grid and a soup"""
    v, idx = unsplit_grid()
    xf = random_xforms(5, 31, spread=3.0)
    inst = [(0, None), (1, xf[1]), (0, xf[2]), (1, xf[3]), (0, xf[4])]
    meshes = [(v, idx), box_meshes()[1]]
    nb = 4
    bones, weights = K.random_bones(len(v), 2, nb, 70), K.random_weights(len(v), 2, 71)
    palette = stretch_palette(nb, 72)
    new = K.skinned(v, bones, weights, palette)
    ctx = context(capi, opts)
    try:
        sc, gm = own_scene(capi, ctx, meshes, inst)
        before = all_arrays(sc, gm, inst)
        gm[0].set_skin(bones, weights, nb)
        pose(ctx, gm[0], palette)
        sc.update()
        got = check(capi, ctx, oracle, sc, gm, [(new, idx), meshes[1]], inst, "a pose under %s" % (opts,), before, deformed={0})
        assert got["model0.ref_off"] is not None, "no split references: the case shows less than it says"
        close_all(sc, gm)
    finally:
        ctx.close()


# ---- traversal -----------------------------------------------------------------------------------------------------------------------------
def test_traversal_after_a_pose(gpu, capi, oracle):
    """13 instances of a blob and a soup, the blob skinned (K = 4, 5 bones) and posed: 20,000 aimed + random rays, production and canonical
    walk, closest / cull / any-hit == the oracle's BVH (built fresh over the numpy vertices) and its brute force, counters too"""
    models = two_models()
    xf = random_xforms(12, 21, spread=6.0)
    inst = [(j % 2, xf[j]) for j in range(12)] + [(0, None)]
    p = Pair(oracle, capi, gpu, models, inst)
    nv, nb = len(models[0][0]), 5
    bones, weights = K.random_bones(nv, 4, nb, 40), K.random_weights(nv, 4, 41, "zeros")
    palette = K.gentle_palette(nb, 42)
    p.gmodels[0].set_skin(bones, weights, nb)
    pose(gpu, p.gmodels[0], palette)
    p.g.update()
    new = [(K.skinned(models[0][0], bones, weights, palette), models[0][1]), models[1]]
    assert new[0][0].tobytes() != np.ascontiguousarray(models[0][0], T.VERTEX).tobytes()
    pair = types.SimpleNamespace(g=p.g, o=make_oracle_scene(oracle, new, inst))
    sets = S.ray_sets(new, inst, None, 10000, 7)
    O = np.concatenate([sets["aimed"][0], sets["random"][0]])
    D = np.concatenate([sets["aimed"][1], sets["random"][1]])
    assert len(O) == 20000
    hit = pair.o.trace(O, D, flags=0, mode=1, nthreads=8)["inst"]
    assert len(np.unique(hit[hit != T.RT_NO_HIT])) == 13, "an instance no ray hits"
    compare_all(pair, O, D, brute=True)


# ---- frames ----------------------------------------------------------------------------------------------------------------------------------
def blob_skin(models, nb=5):
    nv = len(models[0][0])
    return K.random_bones(nv, 2, nb, 50), K.random_weights(nv, 2, 51), nb


def test_progressive_frames_through_three_poses(gpu, capi, oracle):
    """set_shadow_cache(16) and the free sphere, two frames of the rest pose so that both are warm; then three steps of set_bones -> update
    -> clear_output -> render on ONE scene, the palette from the host and from device memory in turn: every frame == the oracle's on fresh
    scenes over the numpy vertices, ray counts included, and another image than the same frame over the pose before"""
    models, inst, mats, cam = light_scene()
    env = scenes.sky_cubemap(8)
    pfcs = frames_of(capi, cam, 5, W, H)
    sc, gm = own_scene(capi, gpu, models, inst)
    bones, weights, nb = blob_skin(models)
    gm[0].set_skin(bones, weights, nb)
    p = pipeline_over(capi, gpu, sc, mats, env)
    p.set_depth_limits(3, 3)
    p.set_shadow_cache(16)
    osc = make_oracle_scene(oracle, models, inst)
    acc = np.zeros((H, W, 4), np.float32)
    for pfc in pfcs[:2]:
        p.update(pfc); p.render()
        acc, ost = osc.render(np.stack(mats), pfc, W, H, accum=acc, env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
    assert_frame(p, acc, ost, "the rest pose")
    for step in range(3):
        palette = K.gentle_palette(nb, 55 + step, angle=0.9, spread=0.5)
        pose(gpu, gm[0], palette, device=step % 2 == 1)
        sc.update()
        p.clear_output()
        blob = K.skinned(models[0][0], bones, weights, palette)
        assert gm[0].geometry()[0].tobytes() == blob.tobytes(), "step %d: geometry()" % step
        prev, osc = osc, make_oracle_scene(oracle, [(blob, models[0][1]), models[1]], inst)
        pfc = pfcs[2 + step]
        p.update(pfc); p.render()
        acc, ost = osc.render(np.stack(mats), pfc, W, H, accum=np.zeros((H, W, 4), np.float32), env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
        assert_frame(p, acc, ost, "step %d" % step)
        stale, _ = prev.render(np.stack(mats), pfc, W, H, accum=np.zeros((H, W, 4), np.float32), env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
        assert int((acc != stale).any(axis=2).sum()) > 50, "step %d: the same frame over the pose before is nearly the same image" % step
    p.close()
    close_all(sc, gm)


def test_realtime_frames_through_three_poses(gpu, capi, oracle):
    """the realtime pipeline had rendered the rest pose; then three poses, an update and a frame after each: both AOVs ==
    osc.render_realtime over the numpy vertices, ray counts included"""
    models, inst, mats, cam = light_scene()
    env = scenes.sky_cubemap(8)
    sc, gm = own_scene(capi, gpu, models, inst)
    bones, weights, nb = blob_skin(models)
    gm[0].set_skin(bones, weights, nb)
    p = pipeline_over(capi, gpu, sc, mats, env, capi.PIPELINE_REALTIME)
    host = capi.ProgressiveHost(10)
    pfc = host.update_realtime(cam, 0.0, 3, W, H)
    p.update(pfc); p.render()
    old = p.read_output(0)
    for step in range(3):
        palette = K.gentle_palette(nb, 55 + step, angle=0.9, spread=0.5)
        pose(gpu, gm[0], palette, device=step % 2 == 0)
        sc.update()
        blob = K.skinned(models[0][0], bones, weights, palette)
        pfc = host.update_realtime(cam, 0.0, 4 + step, W, H)
        p.update(pfc); p.render()
        osc = make_oracle_scene(oracle, [(blob, models[0][1]), models[1]], inst)
        d, ind, ost = osc.render_realtime(np.stack(mats), pfc, W, H, env_faces=env, nthreads=8)
        assert np.array_equal(p.read_output(0), d), "step %d, direct-lighting AOV: %d pixels differ" % (step, int((p.read_output(0) != d).any(axis=2).sum()))
        assert np.array_equal(p.read_output(1), ind), "step %d, indirect-specular AOV: %d pixels differ" % (step, int((p.read_output(1) != ind).any(axis=2).sum()))
        gst = p.stats()
        for key in COUNTS:
            assert gst[key] == ost[key], (step, key, gst[key], ost[key])
        assert 0 < ost["primary_hits"] < W * H and not np.array_equal(d, old)
        old = d
    p.close()
    close_all(sc, gm)


def test_deferred_frames_see_the_pose_they_were_accepted_with(gpu, capi, oracle):
    """set_deferred(4): two frames recorded, set_bones (it renders them before the first byte changes: they see the rest pose), update, two
    more, read: the image == the oracle's frames 1 - 2 on the rest pose accumulated with 3 - 4 on the new pose"""
    models, inst, mats, cam = light_scene()
    env = scenes.sky_cubemap(8)
    pfcs = frames_of(capi, cam, 4, W, H)
    sc, gm = own_scene(capi, gpu, models, inst)
    bones, weights, nb = blob_skin(models)
    p = pipeline_over(capi, gpu, sc, mats, env)
    p.set_depth_limits(3, 3)
    p.set_deferred(4)
    for pfc in pfcs[:2]:
        p.update(pfc); p.render()
    assert p.deferred() == (4, 2)
    gm[0].set_skin(bones, weights, nb)
    assert p.deferred() == (4, 2), "set_skin changes no vertex: nothing to render first"
    palette = K.gentle_palette(nb, 56, angle=0.9, spread=0.5)
    pose(gpu, gm[0], palette)
    assert p.deferred() == (4, 0), "set_bones did not render the recorded frames first"
    sc.update()
    for pfc in pfcs[2:]:
        p.update(pfc); p.render()
    assert p.deferred() == (4, 2)
    blob = K.skinned(models[0][0], bones, weights, palette)
    acc = np.zeros((H, W, 4), np.float32)
    for osc, some in ((make_oracle_scene(oracle, models, inst), pfcs[:2]), (make_oracle_scene(oracle, [(blob, models[0][1]), models[1]], inst), pfcs[2:])):
        for pfc in some:
            acc, _ = osc.render(np.stack(mats), pfc, W, H, accum=acc, env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
    got = p.read_output()
    assert np.array_equal(got, acc), "%d pixels differ" % int((got != acc).any(axis=2).sum())
    p.close()
    close_all(sc, gm)


# ---- states ----------------------------------------------------------------------------------------------------------------------------------
def test_states_and_their_messages(gpu, capi, oracle):
    meshes = list(box_meshes())
    inst = instances_of("13")[:5]
    sc, gm = own_scene(capi, gpu, meshes, inst)
    before = all_arrays(sc, gm, inst)
    bones, weights, nb = soup_skin(len(meshes[0][0]))
    # set_skin alone changes no vertex: the scene stays built, nothing is rebuilt
    gm[0].set_skin(bones, weights, nb)
    sc.trace(*RAYS)
    sc.update()
    assert_bytes_equal(all_arrays(sc, gm, inst), before, "set_skin alone")
    pl = capi.Pipeline(gpu)
    pl.set_scene(sc)
    for _ in inst:
        pl.add_material(T.default_material())
    pl.set_environment_constant((0.5, 0.5, 0.5))
    pl.create_output(32, 32)
    cam = np.array([0, 2, 16, 0, 0, 0, 0, 1, 0, 0.8, 1.0], np.float32)
    pfc = frames_of(capi, cam, 1, 32, 32)[0]
    pl.update(pfc)
    pl.render()
    # set_bones: stale, nothing traces or reads the scene; the message names the pending vertices
    palette = K.gentle_palette(nb, 61)
    pose(gpu, gm[0], palette)
    for call in stale_calls(sc):
        with pytest.raises(capi.RtError, match="new vertices of the models of 3 instances pending") as e:
            call()
        assert e.value.code == -4
    for call in (pl.render, lambda: pl.render_batch([pfc])):
        with pytest.raises(capi.RtError, match="vertices") as e:
            call()
        assert e.value.code == -4
    sc.update()
    new = K.skinned(meshes[0][0], bones, weights, palette)
    check(capi, gpu, oracle, sc, gm, [(new, meshes[0][1]), meshes[1]], inst, "set_bones + update", before, deformed={0})
    pl.render()
    # rt_scene_build instead of rt_scene_update applies a pose as well
    palette = K.gentle_palette(nb, 62)
    pose(gpu, gm[0], palette, device=True)
    with pytest.raises(capi.RtError, match="vertices"):
        sc.trace(*RAYS)
    sc.build()
    new = K.skinned(meshes[0][0], bones, weights, palette)
    check(capi, gpu, oracle, sc, gm, [(new, meshes[0][1]), meshes[1]], inst, "set_bones + build")
    pl.close()
    close_all(sc, gm)


def test_skinned_model_shared_by_two_scenes(gpu, capi, oracle, capfd):
    """after set_bones both scenes are stale; updating A rebuilds the BLAS once and leaves B stale; updating B builds no BLAS and gives B's
    fresh-build arrays (the verbose build log shows the builds)"""
    meshes = list(box_meshes())
    inst_a, inst_b = instances_of("13"), [(0, random_xforms(5, 21, spread=5.0)[j]) for j in range(4)] + [(1, None)]
    gm = [capi.Model(gpu, v, i) for v, i in meshes]
    a, b = capi.Scene(gpu), capi.Scene(gpu)
    for sc, inst in ((a, inst_a), (b, inst_b)):
        for mi, x in inst:
            sc.add_model(gm[mi], x)
        sc.build()
    bones, weights, nb = soup_skin(len(meshes[0][0]))
    gm[0].set_skin(bones, weights, nb)
    palette = K.gentle_palette(nb, 63)
    pose(gpu, gm[0], palette)
    final = [(K.skinned(meshes[0][0], bones, weights, palette), meshes[0][1]), meshes[1]]
    for sc in (a, b):
        with pytest.raises(capi.RtError, match="vertices"):
            sc.trace(*RAYS)
    gpu.set_option("verbose", 1)
    try:
        capfd.readouterr()
        a.update()
        log_a = capfd.readouterr().err
        with pytest.raises(capi.RtError, match="vertices") as e:
            b.trace(*RAYS)
        assert e.value.code == -4
        capfd.readouterr()
        b.update()
        log_b = capfd.readouterr().err
    finally:
        gpu.set_option("verbose", 0)
    assert log_a.count("BLAS arena") == 1 and "TLAS update" in log_a, log_a
    assert log_b.count("BLAS arena") == 0 and "TLAS update" in log_b, log_b
    check(capi, gpu, oracle, a, gm, final, inst_a, "shared skinned model, scene A")
    check(capi, gpu, oracle, b, gm, final, inst_b, "shared skinned model, scene B")
    a.close(); b.close()
    for m in gm:
        m.close()


# ---- the example -----------------------------------------------------------------------------------------------------------------------------
def test_skinned_example_through_the_cpp_mirror(tmp_path):
    """examples/realtime_skinned.cpp: RtModel::setSkin once, RtModel::setBones + RtScene::update per frame, end to end; bent for three frames
    the image is another than bent for one"""
    exe = os.path.join(K.ROOT, "dxrexperiments_amd", "lib", "realtime_skinned")
    images = []
    for frames in (1, 3):
        out = tmp_path / ("out%d.pfm" % frames)
        r = subprocess.run([exe, "96", "64", str(frames), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "1536 skinned vertices, 2976 triangles, 2 bones: %d frames" % frames in r.stdout and "BLAS + TLAS update" in r.stdout
        raw = out.read_bytes()
        head = b"PF\n96 64\n-1.0\n"
        assert raw.startswith(head)
        images.append(np.frombuffer(raw[len(head):], "<f4").reshape(64, 96, 3))
    assert images[0].max() > 0.1 and images[0].std() > 0.01            # an image, not a constant
    assert not np.array_equal(images[0], images[1])
