"""Morph targets (rt_model_set_morph_targets + rt_model_set_morph_weights + rt_scene_update): the vertices the device writes from a base and
a weight per target are, byte for byte, the definition of DESIGN.md section 2 restated in numpy (tests/morph_cases.py) -- both sides of a wave
and of a block, 1 to 65536 targets, every run shape of the sliced layout, host and device weights, every weight family, with and without
normal deltas; every result starts from the base; with a skin the result is the skin's rest pose; and a scene after `set_morph_weights +
update` is, array for array, the scene a fresh build over FRESH models of the morphed arrays gives, byte-equal to such a second GPU scene and
equal to the oracle's, which is built fresh.  Then traversal, a frame through a pipeline that had cached the old shape, a sequence of edits
and the states in between.  No tolerance anywhere."""
import os
import subprocess
import types

import numpy as np
import pytest

import morph_cases as M
import s2_truth as S
import skin_cases as K
from dxrexperiments_amd import rtypes as T, scenes
from test_gpu_batch import frames_of
from test_gpu_instance_transforms import two_models
from test_gpu_model_deform import RAYS, all_arrays, assert_frame, check, close_all, instances_of, own_scene, pipeline_over, stale_calls
from test_gpu_model_skin import assert_vertices, pose
from test_gpu_pipeline import make_oracle_scene
from test_gpu_scene_update import assert_bytes_equal, box_meshes, light_scene
from test_gpu_trace import compare_all
from util import Pair, random_xforms

pytestmark = pytest.mark.gpu

W, H = 96, 64


def blend(ctx, model, w, device=False):
    """set_morph_weights from a host array, or from device memory (Context.upload)"""
    if not device:
        model.set_morph_weights(w)
        return
    buf = ctx.upload(np.ascontiguousarray(w, np.float32))
    model.set_morph_weights_device(buf.ptr)
    ctx.synchronize()
    buf.close()


# ---- the definition --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normals", [False, True], ids=["positions", "normals"])
@pytest.mark.parametrize("n_targets", [1, 3, 70, M.MAX_TARGETS])
def test_morphed_vertices_are_their_definition(gpu, capi, n_targets, normals):
    """V = 1 (one lane), 63 / 64 / 65 (both sides of a wave and of a slice), 257 (both sides of a block), 901; 1, 3, 70 targets and 65536
    with entries only in targets 0, 1 and 65535; every run shape (dense; sparse with vertices nobody names and an empty target; a slice of
    width 0; one vertex named by every target beside vertices named by none); every weight family; a base with -0 coordinates; the weights
    from a host array, then from device memory on the same model (the second result starts from the base as well)"""
    seed = 100 * (n_targets % 1000) + normals
    reached = 0
    for nv in (1, 63, 64, 65, 257, 901):
        for shape in M.SHAPES:
            for family in M.FAMILIES:
                seed += 1
                base, tri, off, idx, dp, dn, w, active = M.case(shape, family, nv, n_targets, seed, normals)
                assert len(w) == n_targets == len(off) - 1 and (nv < 63 or (np.signbit(base["position"]) & (base["position"] == 0)).any())
                if n_targets == M.MAX_TARGETS:
                    assert active == [0, 1, 65535] and off[2] == off[65535], "entries elsewhere than in targets 0, 1 and 65535"
                want = M.morphed(base, off, idx, dp, dn, w)
                what = "%d targets, %d vertices, %s, %s" % (n_targets, nv, shape, family)
                if family == "nan_inf":
                    reached += int(np.isnan(want["position"]).any())
                    assert shape != "dense" or np.isnan(want["position"]).any(), what
                else:
                    assert np.isfinite(want["position"]).all() and np.isfinite(want["normal"]).all(), what
                m = capi.Model(gpu, base, tri)
                m.set_morph_targets(off, idx, dp, dn)
                assert m.morph_targets() == (n_targets, len(idx), normals)
                assert m.geometry()[0].tobytes() == base.tobytes(), what + ": set_morph_targets changed the vertices"
                for device in (False, True):
                    blend(gpu, m, w, device)
                    assert_vertices(m.geometry()[0], want, what + (", device weights" if device else ", host weights"), nans=family == "nan_inf")
                    if not device:
                        m.set_vertices(np.zeros(nv, T.VERTEX))      # (so that vertices the second result did not write show)
                assert np.array_equal(m.geometry()[1], tri)
                m.close()
    assert reached >= 6, "a NaN weight reached a vertex in %d cases only" % reached


@pytest.mark.parametrize("normals", [False, True], ids=["positions", "normals"])
def test_signed_zeros_show_evaluated_padding(gpu, capi, normals):
    """the case holds a -0 base coordinate of a vertex whose only weights are +0 (it must come out +0: every entry is evaluated) and one of a
    vertex with no entry in a slice three cells wide (it must stay -0: padding is not evaluated, and the record is copied bit for bit)"""
    base, tri, off, idx, dp, dn, w = M.signed_zero_case(normals)
    for t in range(3):                                  # what the case says of itself
        names = idx[off[t]:off[t + 1]]
        assert (5 in names) == (t < 2) and 6 not in names and 7 in names
    assert not np.signbit(w[:2]).any() and (w[:2] == 0).all() and (dp > 0).all()
    assert np.signbit(base["position"][[5, 6]]).all() and (base["position"][[5, 6]] == 0).all()
    count, slice_cell = M.pack(len(base), off, idx, dp, dn)[:2]
    assert count[5] == 2 and count[6] == 0 and count[7] == 3 and slice_cell[1] == 3 * 64
    want = M.morphed(base, off, idx, dp, dn, w)
    assert (want["position"][5] == 0).all() and not np.signbit(want["position"][5]).any(), "the restatement skips a zero weight"
    assert np.signbit(want["position"][6]).all() and want[6].tobytes() == base[6].tobytes()
    m = capi.Model(gpu, base, tri)
    m.set_morph_targets(off, idx, dp, dn)
    for device in (False, True):
        blend(gpu, m, w, device)
        got = m.geometry()[0]
        assert not np.signbit(got["position"][5]).any() and (got["position"][5] == 0).all(), "a zero weight was skipped"
        assert np.signbit(got["position"][6]).all() and got[6].tobytes() == base[6].tobytes(), "padding was evaluated"
        assert_vertices(got, want, "signed zeros")
    m.close()


# ---- the base ----------------------------------------------------------------------------------------------------------------------------
def test_every_result_starts_from_the_base(gpu, capi):
    nv, nt = 901, 5
    base, tri, off, idx, dp, dn, wa, _ = M.case("sparse", "convex", nv, nt, 77)
    wb = M.weights(nt, "wild", 78)
    m = capi.Model(gpu, base, tri)
    m.set_morph_targets(off, idx, dp, dn)
    a, b = M.morphed(base, off, idx, dp, dn, wa), M.morphed(base, off, idx, dp, dn, wb)
    assert a.tobytes() != b.tobytes() and b.tobytes() != M.morphed(a, off, idx, dp, dn, wb).tobytes()
    blend(gpu, m, wa)
    assert_vertices(m.geometry()[0], a, "weights A")
    blend(gpu, m, wb, device=True)
    assert_vertices(m.geometry()[0], b, "weights B after weights A")
    # set_vertices / set_positions in between write the current vertices and leave the base alone
    scribble = base.copy()
    scribble["position"] += np.float32(3.0)
    m.set_vertices(scribble)
    assert m.geometry()[0].tobytes() == scribble.tobytes()
    m.set_positions(base["position"][:100] * np.float32(2.0), 5)
    blend(gpu, m, wa)
    assert_vertices(m.geometry()[0], a, "weights A after set_vertices / set_positions")
    # set_morph_targets again: the vertices as they are -- A -- are the new base (and the targets are others: positions only)
    off2, idx2, dp2, _, _ = M.targets(M.runs("gap", nv, 2, 80), None, 81, normals=False)
    m.set_morph_targets(off2, idx2, dp2)
    assert m.morph_targets() == (2, len(idx2), False)
    assert_vertices(m.geometry()[0], a, "set_morph_targets again")
    blend(gpu, m, wb[:2])
    assert_vertices(m.geometry()[0], M.morphed(a, off2, idx2, dp2, None, wb[:2]), "weights B over the new base A")
    m.close()


# ---- with a skin -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["skin_first", "targets_first"])
def test_with_a_skin_the_result_is_the_rest_pose(gpu, capi, order):
    """a model in one built scene; after set_morph_weights its vertices are unchanged and the scene still traces; after set_bones the vertices
    are skinned(morphed(base)) byte for byte; after clear_skin the next morph lands in the vertices"""
    nv, nt, k, nb = 901, 4, 3, 5
    base, tri, off, idx, dp, dn, w, _ = M.case("sparse", "convex", nv, nt, 31)
    bones, sw = K.random_bones(nv, k, nb, 32), K.random_weights(nv, k, 33)
    sc, gm = own_scene(capi, gpu, [(base, tri)], [(0, None), (0, random_xforms(1, 3, spread=4.0)[0])])
    m = gm[0]
    before = sc.trace(*RAYS)
    if order == "skin_first":
        m.set_skin(bones, sw, nb)
        m.set_morph_targets(off, idx, dp, dn)           # the base: the skin's rest pose
    else:
        m.set_morph_targets(off, idx, dp, dn)           # the base: the vertices
        m.set_skin(bones, sw, nb)                       # later results go to the new rest pose
    for step, device in enumerate((False, True)):
        w = M.weights(nt, "wild", 40 + step)
        blend(gpu, m, w, device)
        if step == 0:
            assert m.geometry()[0].tobytes() == base.tobytes(), "set_morph_weights on a skinned model changed its vertices"
            after = sc.trace(*RAYS)                     # built, traceable
            assert all(np.array_equal(before[key], after[key]) for key in ("t", "prim", "inst"))
        palette = K.gentle_palette(nb, 50 + step)
        pose(gpu, m, palette, device)
        with pytest.raises(capi.RtError, match="vertices"):
            sc.trace(*RAYS)
        want = K.skinned(M.morphed(base, off, idx, dp, dn, w), bones, sw, palette)
        assert_vertices(m.geometry()[0], want, "%s, step %d: skinned(morphed(base))" % (order, step))
        sc.update()
    # no skin any more: the next result lands in the vertices, still from the morph base
    m.clear_skin()
    w = M.weights(nt, "convex", 45)
    blend(gpu, m, w)
    assert_vertices(m.geometry()[0], M.morphed(base, off, idx, dp, dn, w), order + ": after clear_skin")
    with pytest.raises(capi.RtError, match="vertices") as e:
        sc.trace(*RAYS)
    assert e.value.code == -4
    sc.update()
    sc.trace(*RAYS)
    close_all(sc, gm)


# ---- update == build ---------------------------------------------------------------------------------------------------------------------
def soup_targets(n_verts, n_targets=3, seed=60, normals=True, scale=0.3):
    """sparse targets over a mesh of n_verts vertices: (offsets, indices, dpos, dnrm)"""
    return M.targets(M.runs("sparse", n_verts, n_targets, seed), None, seed + 1, normals, scale)[:4]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_update_equals_build(gpu, capi, oracle, device):
    """the two soups of test_gpu_scene_update.py; scene A holds model 0 twice and model 1 once, scene B shares model 0; model 0 morphed
    twice, an update after each: both scenes are stale in between (RT_ERR_STATE from every call that reads them) and afterwards == a fresh
    GPU build over fresh models of the numpy vertices == the oracle's; the instance of the other model keeps its box and inverse"""
    meshes = list(box_meshes())
    xf = random_xforms(4, 17, spread=5.0)
    inst_a, inst_b = [(0, None), (1, xf[0]), (0, xf[1])], [(0, xf[2]), (1, None), (0, xf[3])]
    sc, gm = own_scene(capi, gpu, meshes, inst_a)
    other = capi.Scene(gpu)
    for mi, x in inst_b:
        other.add_model(gm[mi], x)
    other.build()
    before = all_arrays(sc, gm, inst_a)
    off, idx, dp, dn = soup_targets(len(meshes[0][0]))
    gm[0].set_morph_targets(off, idx, dp, dn)
    sc.trace(*RAYS)                                     # set_morph_targets alone: built
    for step in range(2):
        w = M.weights(3, ("convex", "wild")[step], 90 + step)
        blend(gpu, gm[0], w, device)
        for scene, n in ((sc, 2), (other, 2)):
            for call in stale_calls(scene):
                with pytest.raises(capi.RtError, match="new vertices of the models of %d instances pending" % n) as e:
                    call()
                assert e.value.code == -4
        sc.update()
        with pytest.raises(capi.RtError, match="vertices"):
            other.trace(*RAYS)
        other.update()
        new = [(M.morphed(meshes[0][0], off, idx, dp, dn, w), meshes[0][1]), meshes[1]]
        got = check(capi, gpu, oracle, sc, gm, new, inst_a, "scene A, weights %d" % step, before, deformed={0})
        check(capi, gpu, oracle, other, gm, new, inst_b, "scene B, weights %d" % step)
        assert got["model0.verts"].tobytes() != before["model0.verts"].tobytes() and sc.update_ms() > 0.0
    other.close()
    close_all(sc, gm)


def test_traversal_after_a_morph(gpu, capi, oracle):
    """13 instances of a blob and a soup, the blob morphed (three sparse targets with normal deltas): 20,000 aimed + random rays, production
    and canonical walk, closest / cull / any-hit == the oracle's BVH (built fresh over the numpy vertices) and its brute force, counters too"""
    models = two_models()
    xf = random_xforms(12, 21, spread=6.0)
    inst = [(j % 2, xf[j]) for j in range(12)] + [(0, None)]
    p = Pair(oracle, capi, gpu, models, inst)
    off, idx, dp, dn = soup_targets(len(models[0][0]), seed=40)
    w = M.weights(3, "zeros", 42)
    p.gmodels[0].set_morph_targets(off, idx, dp, dn)
    blend(gpu, p.gmodels[0], w)
    p.g.update()
    new = [(M.morphed(models[0][0], off, idx, dp, dn, w), models[0][1]), models[1]]
    assert new[0][0].tobytes() != np.ascontiguousarray(models[0][0], T.VERTEX).tobytes()
    pair = types.SimpleNamespace(g=p.g, o=make_oracle_scene(oracle, new, inst))
    sets = S.ray_sets(new, inst, None, 10000, 7)
    O = np.concatenate([sets["aimed"][0], sets["random"][0]])
    D = np.concatenate([sets["aimed"][1], sets["random"][1]])
    assert len(O) == 20000
    hit = pair.o.trace(O, D, flags=0, mode=1, nthreads=8)["inst"]
    assert len(np.unique(hit[hit != T.RT_NO_HIT])) == 13, "an instance no ray hits"
    compare_all(pair, O, D, brute=True)


def test_a_frame_through_a_pipeline_that_had_cached_the_old_shape(gpu, capi, oracle):
    """set_shadow_cache(16) and the free sphere, one frame of the base so that both are warm; then set_morph_weights -> update -> clear_output
    -> render: the 96 x 64 frame == the oracle's on a fresh scene over the numpy vertices, ray counts included, and another image than the
    same frame over the base"""
    models, inst, mats, cam = light_scene()
    env = scenes.sky_cubemap(8)
    pfcs = frames_of(capi, cam, 2, W, H)
    sc, gm = own_scene(capi, gpu, models, inst)
    off, idx, dp, dn = soup_targets(len(models[0][0]), seed=50, scale=0.6)
    gm[0].set_morph_targets(off, idx, dp, dn)
    p = pipeline_over(capi, gpu, sc, mats, env)
    p.set_depth_limits(3, 3)
    p.set_shadow_cache(16)
    old = make_oracle_scene(oracle, models, inst)
    kw = dict(env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
    p.update(pfcs[0]); p.render()
    acc, ost = old.render(np.stack(mats), pfcs[0], W, H, accum=np.zeros((H, W, 4), np.float32), **kw)
    assert_frame(p, acc, ost, "the base")
    w = M.weights(3, "convex", 55)
    blend(gpu, gm[0], w, device=True)
    with pytest.raises(capi.RtError, match="vertices") as e:
        p.render()
    assert e.value.code == -4
    sc.update()
    p.clear_output()
    blob = M.morphed(models[0][0], off, idx, dp, dn, w)
    assert gm[0].geometry()[0].tobytes() == blob.tobytes()
    osc = make_oracle_scene(oracle, [(blob, models[0][1]), models[1]], inst)
    p.update(pfcs[1]); p.render()
    acc, ost = osc.render(np.stack(mats), pfcs[1], W, H, accum=np.zeros((H, W, 4), np.float32), **kw)
    assert_frame(p, acc, ost, "the morphed blob")
    stale, _ = old.render(np.stack(mats), pfcs[1], W, H, accum=np.zeros((H, W, 4), np.float32), **kw)
    assert int((acc != stale).any(axis=2).sum()) > 50, "the same frame over the base is nearly the same image"
    p.close()
    close_all(sc, gm)


def test_deferred_frames_see_the_mesh_they_were_accepted_with(gpu, capi, oracle):
    """set_deferred(4), two frames recorded.  (a) no skin: set_morph_targets changes no vertex and renders nothing; set_morph_weights renders
    the two frames before the first byte changes (they see the base); update, two more, read: the image == the oracle's frames 1 - 2 on the
    base accumulated with 3 - 4 on the morphed blob.  (b) a skin and targets: set_morph_weights writes the rest pose only -- the recorded
    frames stay recorded, the vertices stay byte for byte -- and the next set_bones renders them and gives skinned(morphed(base))"""
    models, inst, mats, cam = light_scene()
    env = scenes.sky_cubemap(8)
    pfcs = frames_of(capi, cam, 4, W, H)
    nv = len(models[0][0])
    off, idx, dp, dn = soup_targets(nv, seed=50, scale=0.6)
    w = M.weights(3, "convex", 55)
    morphed = M.morphed(models[0][0], off, idx, dp, dn, w)
    assert morphed.tobytes() != np.ascontiguousarray(models[0][0], T.VERTEX).tobytes()

    def recording():
        sc, gm = own_scene(capi, gpu, models, inst)
        p = pipeline_over(capi, gpu, sc, mats, env)
        p.set_depth_limits(3, 3)
        p.set_deferred(4)
        return sc, gm, p

    def record(p, some):
        for pfc in some:
            p.update(pfc); p.render()
        assert p.deferred() == (4, 2)

    # (a)
    sc, gm, p = recording()
    record(p, pfcs[:2])
    gm[0].set_morph_targets(off, idx, dp, dn)
    assert p.deferred() == (4, 2), "set_morph_targets changes no vertex: nothing to render first"
    blend(gpu, gm[0], w)
    assert p.deferred() == (4, 0), "set_morph_weights did not render the recorded frames first"
    sc.update()
    record(p, pfcs[2:])
    acc = np.zeros((H, W, 4), np.float32)
    for osc, some in ((make_oracle_scene(oracle, models, inst), pfcs[:2]), (make_oracle_scene(oracle, [(morphed, models[0][1]), models[1]], inst), pfcs[2:])):
        for pfc in some:
            acc, _ = osc.render(np.stack(mats), pfc, W, H, accum=acc, env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
    got = p.read_output()
    assert np.array_equal(got, acc), "%d pixels differ" % int((got != acc).any(axis=2).sum())
    p.close()
    close_all(sc, gm)

    # (b)
    sc, gm, p = recording()
    bones, sw, nb = K.random_bones(nv, 2, 5, 50), K.random_weights(nv, 2, 51), 5
    gm[0].set_skin(bones, sw, nb)
    gm[0].set_morph_targets(off, idx, dp, dn)
    before = gm[0].geometry()[0].tobytes()
    record(p, pfcs[:2])
    blend(gpu, gm[0], w)
    assert p.deferred() == (4, 2), "set_morph_weights on a skinned model changes no vertex: nothing to render first"
    assert gm[0].geometry()[0].tobytes() == before, "set_morph_weights on a skinned model changed its vertices"
    identity = K.identity_palette(nb)
    pose(gpu, gm[0], identity)
    assert p.deferred() == (4, 0), "set_bones did not render the recorded frames first"
    sc.update()
    assert gm[0].geometry()[0].tobytes() == K.skinned(morphed, bones, sw, identity).tobytes()
    p.close()
    close_all(sc, gm)


# ---- a sequence of edits -------------------------------------------------------------------------------------------------------------------
def test_a_sequence_of_edits_equals_the_build_of_its_final_state(gpu, capi, oracle):
    """a morphed, skinned model 0 in five instances of two models: weights A + bones P, update; a transform and a hidden instance, update;
    weights B alone (the rest pose changes, no vertex: the scene stays built), a new transform, update; bones Q and the instance shown,
    update == the fresh build of skinned(morphed(base, B), Q) under the final transforms"""
    meshes = list(box_meshes())
    inst = instances_of("13")[:5]
    sc, gm = own_scene(capi, gpu, meshes, inst)
    nv = len(meshes[0][0])
    bones, sw, nb = K.random_bones(nv, 2, 4, 70), K.random_weights(nv, 2, 71), 4
    off, idx, dp, dn = soup_targets(nv, seed=72)
    gm[0].set_skin(bones, sw, nb)
    gm[0].set_morph_targets(off, idx, dp, dn)
    wa, wb = M.weights(3, "convex", 73), M.weights(3, "wild", 74)
    pp, pq = K.gentle_palette(nb, 75), K.gentle_palette(nb, 76)
    new_xf = random_xforms(5, 77, spread=6.0)
    blend(gpu, gm[0], wa)
    pose(gpu, gm[0], pp)
    sc.update()
    sc.set_transform(2, new_xf[2])
    sc.set_mask(1, 0)
    sc.update()
    blend(gpu, gm[0], wb, device=True)
    sc.trace(*RAYS)                                     # weights alone on a skinned model: nothing pending
    assert gm[0].geometry()[0].tobytes() == K.skinned(M.morphed(meshes[0][0], off, idx, dp, dn, wa), bones, sw, pp).tobytes()
    sc.set_transform(3, new_xf[3])
    sc.update()
    pose(gpu, gm[0], pq, device=True)
    sc.set_mask(1, 0xFF)
    sc.update()
    final = list(inst)
    final[2], final[3] = (inst[2][0], new_xf[2]), (inst[3][0], new_xf[3])
    new = K.skinned(M.morphed(meshes[0][0], off, idx, dp, dn, wb), bones, sw, pq)
    check(capi, gpu, oracle, sc, gm, [(new, meshes[0][1]), meshes[1]], final, "the sequence")
    close_all(sc, gm)


# ---- states ----------------------------------------------------------------------------------------------------------------------------------
def test_states_and_refusals(gpu, capi):
    """no targets: RT_ERR_STATE; the refusals (each names what it should) leave the targets, the vertices and the scene as they were;
    n_targets = 0 removes the targets; replacing them recaptures the base"""
    nv, nt = 130, 4
    base, tri = M.base(nv, 5)
    off, idx, dp, dn, _ = M.targets(M.runs("dense", nv, nt, 6), None, 7)
    w = M.weights(nt, "convex", 8)
    sc, gm = own_scene(capi, gpu, [(base, tri)], [(0, None)])
    m = gm[0]
    lib = capi.lib()
    po, pi, pp, pn, pw = off.ctypes.data, idx.ctypes.data, dp.ctypes.data, dn.ctypes.data, w.ctypes.data
    assert m.morph_targets() == (0, 0, False)
    with pytest.raises(capi.RtError, match="rt_model_set_morph_targets") as e:
        m.set_morph_weights(w)                          # never had targets
    assert e.value.code == -4
    m.set_morph_targets(off, idx, dp, dn)
    sc.trace(*RAYS)                                     # nothing changed: built
    decreasing = off.copy()
    decreasing[3] = decreasing[2] - 1
    beyond, twice = idx.copy(), idx.copy()
    beyond[2 * nv + 129] = nv
    twice[nv + 41] = twice[nv + 40]
    shifted = off + np.uint32(1)                         # (the binding itself refuses offsets that do not end at the number of indices)
    assert lib.rt_model_set_morph_targets(m.h, nt, shifted.ctypes.data, pi, pp, pn) == -1 and b"target_offsets[0]" in lib.rt_last_error()
    for o, i, words in ((decreasing, idx, "target 2"), (off, beyond, "target 2, entry %d" % (2 * nv + 129)), (off, twice, "target 1, entry %d" % (nv + 41))):
        with pytest.raises(capi.RtError, match=words) as e:
            m.set_morph_targets(o, i, dp, dn)
        assert e.value.code == -1, words
    many = np.zeros(65538, np.uint32)
    assert lib.rt_model_set_morph_targets(m.h, 65537, many.ctypes.data, pi, pp, pn) == -1 and b"65537" in lib.rt_last_error()
    for args in ((None, pi, pp, pn), (po, None, pp, pn), (po, pi, None, pn)):
        assert lib.rt_model_set_morph_targets(m.h, nt, *args) == -1 and b"null" in lib.rt_last_error()
    assert lib.rt_model_set_morph_weights(m.h, None, 0) == -1 and lib.rt_model_set_morph_weights(m.h, pw, 2) == -1
    with pytest.raises(capi.RtError, match="weights"):
        m.set_morph_weights(w[:2])
    assert m.morph_targets() == (nt, len(idx), True) and m.geometry()[0].tobytes() == base.tobytes()
    sc.trace(*RAYS)                                     # ... and still built
    blend(gpu, m, w)
    a = M.morphed(base, off, idx, dp, dn, w)
    assert_vertices(m.geometry()[0], a, "after the refusals")
    # replaced: the vertices as they are -- A -- are the base of the new targets, which have no normal deltas
    m.set_morph_targets(off[:3], idx[:off[2]], dp[:off[2]])
    assert m.morph_targets() == (2, int(off[2]), False)
    blend(gpu, m, w[:2], device=True)
    assert_vertices(m.geometry()[0], M.morphed(a, off[:3], idx[:off[2]], dp[:off[2]], None, w[:2]), "replaced targets")
    # removed: the vertices stay, set_morph_weights has nothing to work with
    last = m.geometry()[0]
    m.clear_morph_targets()
    assert m.morph_targets() == (0, 0, False)
    with pytest.raises(capi.RtError, match="rt_model_set_morph_targets") as e:
        m.set_morph_weights(w)
    assert e.value.code == -4
    buf = gpu.upload(w)
    with pytest.raises(capi.RtError, match="rt_model_set_morph_targets") as e:
        m.set_morph_weights_device(buf.ptr)
    assert e.value.code == -4
    buf.close()
    assert m.geometry()[0].tobytes() == last.tobytes()
    m.clear_morph_targets()                             # (twice is once)
    sc.update()
    sc.trace(*RAYS)
    close_all(sc, gm)


# ---- the example -----------------------------------------------------------------------------------------------------------------------------
def test_morph_example_through_the_cpp_mirror(tmp_path):
    """examples/realtime_morph.cpp: RtModel::setMorphTargets once, RtModel::setMorphWeights + RtScene::update per frame, end to end; after
    three frames the image is another than after one"""
    exe = os.path.join(M.ROOT, "dxrexperiments_amd", "lib", "realtime_morph")
    images = []
    for frames in (1, 3):
        out = tmp_path / ("out%d.pfm" % frames)
        r = subprocess.run([exe, "96", "64", str(frames), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "4096 morphed vertices, 7938 triangles, 1 target of" in r.stdout and ": %d frames" % frames in r.stdout and "BLAS + TLAS update" in r.stdout
        raw = out.read_bytes()
        head = b"PF\n96 64\n-1.0\n"
        assert raw.startswith(head)
        images.append(np.frombuffer(raw[len(head):], "<f4").reshape(64, 96, 3))
    assert images[0].max() > 0.1 and images[0].std() > 0.01            # an image, not a constant
    assert not np.array_equal(images[0], images[1])
