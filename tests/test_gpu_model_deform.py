"""Deforming meshes (rt_model_set_vertices / rt_model_set_positions / rt_model_recompute_normals + rt_scene_update): a scene after `set +
update` is, array for array, the scene a fresh build of the same instance list over FRESH models created from the final vertex arrays gives
-- every BLAS's canonical arrays, production nodes and records, reference offsets and boxes, every instance record, the TLAS -- byte-equal to
such a second GPU scene and equal to the oracle's, which is never updated: it is built fresh from the final arrays.  Then traversal, whole
frames through pipelines that had cached what the old mesh looked like, the builder options, the states in between (a scene whose model has
pending vertices is stale and nothing reads it), and recompute_normals against its definition restated in numpy.  No tolerance anywhere."""
import types

import numpy as np
import pytest

import s2_truth as S
from deform_cases import displaced, grid_mesh, index_lists, normals_of, slivers
from dxrexperiments_amd import rtypes as T, scenes
from test_gpu_batch import frames_of
from test_gpu_instance_transforms import COUNTS, two_models
from test_gpu_option_matrix import BUILD_ROWS, _case_id, context
from test_gpu_pipeline import make_oracle_scene
from test_gpu_scene_update import arrays, assert_bytes_equal, assert_equals_oracle, box_meshes, light_scene
from test_gpu_trace import compare_all
from util import ANY, Pair, assert_hits_equal, random_xforms, triangle_soup

pytestmark = pytest.mark.gpu

W, H = 96, 64
_cache = {}


def unsplit_grid():
    """29 x 29 vertices, 1,568 triangles (4,704 vertex references: two work items of the box kernels), none of them split"""
    if "grid" not in _cache:
        _cache["grid"] = scenes.displaced_grid(28, seed=7, extent=2.0)
    return _cache["grid"]


def own_scene(capi, ctx, meshes, inst):
    """(scene built over models of its own -- they are deformed in place --, the models)"""
    gm = [capi.Model(ctx, v, i) for v, i in meshes]
    sc = capi.Scene(ctx)
    for mi, x in inst:
        sc.add_model(gm[mi], x)
    sc.build()
    return sc, gm


def all_arrays(sc, gm, inst):
    """test_gpu_scene_update's arrays + for one instance of every model: bvh(k), wide_read(k), wide_counts(k), refs(k), Model.geometry()"""
    a = arrays(sc, len(inst))
    for mi in sorted(set(m for m, _ in inst)):
        k = [m for m, _ in inst].index(mi)
        nodes, keys, parents, depth = sc.bvh(k)
        wn, root, recs = sc.wide_read(k)
        off, boxes, rec_boxes = sc.refs(k)
        verts, idx = gm[mi].geometry()
        pre = "model%d." % mi
        a.update({pre + "nodes": nodes, pre + "keys": keys, pre + "parents": parents, pre + "depth": depth, pre + "wide": wn, pre + "root": root,
                  pre + "records": recs, pre + "counts": sc.wide_counts(k), pre + "ref_off": off, pre + "ref_boxes": boxes, pre + "rec_boxes": rec_boxes,
                  pre + "verts": verts, pre + "idx": idx})
    return a


def assert_blas_equals_oracle(a, osc, meshes, inst, what):
    for mi in sorted(set(m for m, _ in inst)):
        pre = "model%d." % mi
        on, ok, op, od = osc.bvh(mi)
        assert np.array_equal(a[pre + "keys"], ok) and np.array_equal(a[pre + "parents"], op) and a[pre + "depth"] == od, "%s: BLAS %d keys / parents / depth" % (what, mi)
        for f in ("left", "right"):
            assert np.array_equal(a[pre + "nodes"][f], on[f]), "%s: BLAS %d node.%s" % (what, mi, f)
        for f in ("bmin", "bmax"):
            assert np.array_equal(a[pre + "nodes"][f], on[f], equal_nan=True), "%s: BLAS %d node.%s" % (what, mi, f)
        off, boxes = osc.refs(mi, len(meshes[mi][1]))
        if off is None:
            assert a[pre + "ref_off"] is None, "%s: BLAS %d has references, the oracle's has none" % (what, mi)
        else:
            assert a[pre + "ref_off"] is not None and np.array_equal(a[pre + "ref_off"], off) and np.array_equal(a[pre + "ref_boxes"], boxes, equal_nan=True), \
                "%s: BLAS %d references" % (what, mi)
        assert a[pre + "verts"].tobytes() == np.ascontiguousarray(meshes[mi][0], T.VERTEX).tobytes(), "%s: geometry() of model %d" % (what, mi)


def check(capi, ctx, oracle, sc, gm, meshes, inst, what, before=None, deformed=()):
    """sc (already updated) against a fresh GPU scene over fresh models of the final arrays `meshes` and a fresh oracle scene; the instances
    of the models not in `deformed` as before"""
    got = all_arrays(sc, gm, inst)
    fresh, fm = own_scene(capi, ctx, meshes, inst)
    want = all_arrays(fresh, fm, inst)
    assert_bytes_equal(got, want, what + " vs a fresh GPU build over fresh models")
    osc = make_oracle_scene(oracle, meshes, inst)
    assert_equals_oracle(got, osc, len(inst), what)
    assert_blas_equals_oracle(got, osc, meshes, inst, what)
    if before is not None:
        for k, (mi, _) in enumerate(inst):
            if mi not in deformed:
                assert got["boxes"][k].tobytes() == before["boxes"][k].tobytes() and got["invs"][k].tobytes() == before["invs"][k].tobytes(), (what, k)
    fresh.close()
    for m in fm:
        m.close()
    return got


def close_all(sc, gm):
    sc.close()
    for m in gm:
        m.close()


# ---- update == build ---------------------------------------------------------------------------------------------------------------------
def instances_of(count):
    """1i: one identity instance (rays walk its BLAS directly); 1t: one transformed; 13: 12 + one identity, two models; 300: more TLAS nodes
    than the 128 of the LDS top"""
    if count == "1i":
        return [(0, None)]
    if count == "1t":
        return [(0, random_xforms(1, 9, spread=2.0)[0])]
    n = int(count)
    xf = random_xforms(n, 3, spread=6.0)
    inst = [(k % 2, xf[k]) for k in range(n)]
    if n == 13:
        inst[12] = (0, None)
    return inst


def apply(ctx, model, old, mode):
    """deforms `model` (currently `old`) by `mode`; returns the vertex array it now holds.  v / p: set_vertices / set_positions; h / d: from a
    host array / from device memory (Context.upload); sub: only the vertices from `first` > 0 to the last one"""
    first = len(old) - 901 if mode.startswith("sub") else 0
    new = displaced(old, seed=41, amount=1.0, first=first)
    kind = mode.replace("sub_", "")
    if kind[0] == "p":
        new["normal"] = old["normal"]                   # set_positions keeps the normals
    part = np.ascontiguousarray(new[first:])
    if kind == "vh":
        model.set_vertices(part, first)
    elif kind == "ph":
        model.set_positions(part["position"], first)
    elif kind == "vd":
        buf = ctx.upload(part)
        model.set_vertices_device(buf.ptr, len(part), first)
        ctx.synchronize()
        buf.close()
    else:
        buf = ctx.upload(np.ascontiguousarray(part["position"]))
        model.set_positions_device(buf.ptr, len(part), first)
        ctx.synchronize()
        buf.close()
    return new


ARRAY_CASES = [("1i", m) for m in ("vh", "ph", "vd", "pd", "sub_vh", "sub_pd")] + [("1t", "vh"), ("1t", "pd")] + \
              [("13", m) for m in ("vh", "ph", "vd", "pd", "sub_vh", "sub_pd")] + [("300", "vd"), ("300", "sub_ph")]


@pytest.mark.parametrize("count,mode", ARRAY_CASES)
def test_update_equals_build(gpu, capi, oracle, count, mode):
    """the two soups of test_gpu_scene_update.py (4,200 and 4,095 vertex references); model 0 displaced by up to 1.0 per axis in a box of
    extent 2 (another Morton order: asserted), whole or from vertex n - 901 to the last; records or positions; host or device source"""
    meshes = list(box_meshes())
    inst = instances_of(count)
    used = [m for k, m in enumerate(meshes) if k in set(mi for mi, _ in inst)]
    sc, gm = own_scene(capi, gpu, used, inst)
    before = all_arrays(sc, gm, inst)
    new = apply(gpu, gm[0], meshes[0][0], mode)
    final = [(new, meshes[0][1])] + used[1:]
    sc.update()
    got = check(capi, gpu, oracle, sc, gm, final, inst, "%s %s" % (count, mode), before, deformed={0})
    assert not np.array_equal(got["model0.keys"], before["model0.keys"]), "the deformation left the Morton order as it was: the case shows little"
    assert sc.update_ms() > 0.0
    close_all(sc, gm)


def test_transforms_and_vertices_pending_together(gpu, capi, oracle):
    """13 instances: transforms of 1, 2 and the identity instance 12 set, model 1's vertices set TWICE (all records, then the positions of a
    sub-range on top), model 0 untouched; one update()"""
    meshes = list(box_meshes())
    inst = instances_of("13")
    sc, gm = own_scene(capi, gpu, meshes, inst)
    before = all_arrays(sc, gm, inst)
    new_x = random_xforms(13, 77, spread=6.0)
    final_inst = list(inst)
    for k in (1, 2, 12):
        final_inst[k] = (inst[k][0], new_x[k])
        sc.set_transform(k, new_x[k])
    v1 = displaced(meshes[1][0], seed=5, amount=0.8)
    gm[1].set_vertices(v1)
    v2 = displaced(v1, seed=6, amount=0.5, first=2000)
    v2["normal"] = v1["normal"]
    gm[1].set_positions(v2["position"][2000:], 2000)
    sc.update()
    got = check(capi, gpu, oracle, sc, gm, [meshes[0], (v2, meshes[1][1])], final_inst, "transforms + vertices")
    for k in range(13):
        if k % 2 == 0 and k not in (2, 12):
            assert got["boxes"][k].tobytes() == before["boxes"][k].tobytes() and got["invs"][k].tobytes() == before["invs"][k].tobytes(), k
    close_all(sc, gm)


# ---- split references, degenerate structures ------------------------------------------------------------------------------------------
def test_split_references_appear_and_disappear(gpu, capi, oracle):
    """a grid none of whose triangles is split; one vertex of every 16th triangle moved by (20, 17, 13): slivers, several references each;
    every 8th: more (the buffers grow); back to 16 (they shrink); back to the grid (they vanish); and again.  n_recs, rec_boxes, ref_off and the
    record marks (wide_read's records, word 10) are among the arrays compared."""
    v, idx = unsplit_grid()
    inst = [(0, None), (0, random_xforms(2, 3, spread=30.0)[0]), (1, random_xforms(2, 3, spread=30.0)[1])]
    meshes = [(v, idx), box_meshes()[1]]
    sc, gm = own_scene(capi, gpu, meshes, inst)
    assert sc.refs(0)[0] is None, "a triangle of the undeformed grid is split: the case does not start where it says"
    n_refs = []
    for step, verts in enumerate((slivers(v, idx, 16), slivers(v, idx, 8), slivers(v, idx, 16), v, slivers(v, idx, 16))):
        gm[0].set_vertices(verts)
        sc.update()
        got = check(capi, gpu, oracle, sc, gm, [(verts, idx), meshes[1]], inst, "slivers step %d" % step)
        off = got["model0.ref_off"]
        n_refs.append(0 if off is None else int(off[-1]))
        if off is not None:
            marks = got["model0.records"][:, 10].view(np.uint32)
            assert got["model0.counts"][1] == len(marks) > len(idx) and set(marks.tolist()) == {0, 1}, "the production layout holds no triangle as several records"
    assert n_refs[0] > len(idx) and n_refs[1] > n_refs[0] and n_refs[2] == n_refs[0] and n_refs[3] == 0 and n_refs[4] == n_refs[0], n_refs
    close_all(sc, gm)


@pytest.mark.parametrize("n_tris", [1, 2])
def test_models_that_are_one_leaf(gpu, capi, oracle, n_tris):
    """a model of 1 or 2 triangles (the whole BLAS is one leaf: negative root code), alone as an identity instance and among others"""
    tiny = triangle_soup(n_tris, seed=3, extent=1.0, size=0.5)
    xf = random_xforms(3, 8, spread=4.0)
    for inst in ([(0, None)], [(0, xf[0]), (1, None), (0, None), (1, xf[1])]):
        meshes = [tiny, box_meshes()[1]][:max(m for m, _ in inst) + 1]
        sc, gm = own_scene(capi, gpu, meshes, inst)
        new = displaced(tiny[0], seed=9, amount=3.0)
        gm[0].set_vertices(new)
        sc.update()
        got = check(capi, gpu, oracle, sc, gm, [(new, tiny[1])] + meshes[1:], inst, "%d triangle(s), %d instances" % (n_tris, len(inst)))
        assert got["model0.root"] < 0 and got["model0.counts"] == (0, n_tris)
        close_all(sc, gm)


def test_not_a_number_and_back(gpu, capi, oracle):
    """a mesh gets a NaN and an inf vertex (PLOC gives up: the LBVH layout; an axis that cannot be quantised), then finite vertices again"""
    v, idx = triangle_soup(700, seed=12, extent=2.0, size=0.3)
    inst = [(0, None), (0, random_xforms(1, 4, spread=5.0)[0])]
    sc, gm = own_scene(capi, gpu, [(v, idx)], inst)
    bad = displaced(v, seed=2, amount=0.5)
    bad["position"][3, 0] = np.nan                     # (a triangle's FIRST corner: where the oracle's a < b ? a : b and the kernels' fminf agree that a NaN is ignored)
    bad["position"][1000, 1] = np.inf
    for step, verts in enumerate((bad, v, bad, displaced(v, seed=3, amount=0.5))):
        gm[0].set_vertices(verts)
        sc.update()
        check(capi, gpu, oracle, sc, gm, [(verts, idx)], inst, "NaN / inf step %d" % step)
    close_all(sc, gm)


# ---- a model shared by two scenes; states -------------------------------------------------------------------------------------------------
RAYS = (np.zeros((4, 4), np.float32), np.tile(np.array([0, 0, 1, 1e30], np.float32), (4, 1)))


def stale_calls(sc):
    """the calls test_gpu_scene_update.py lists for a stale scene"""
    O, D = RAYS
    return (lambda: sc.trace(O, D), lambda: sc.trace(O, D, canonical=True), lambda: sc.instance_info(0), lambda: sc.bvh(-1), lambda: sc.wide_read(-1),
            lambda: sc.wide_counts(0), lambda: sc.bvh(0), lambda: sc.refs(0))


def test_model_shared_by_two_scenes(gpu, capi, oracle, capfd):
    """after the set both scenes are stale; updating A leaves B stale; updating B gives B's fresh-build arrays, and builds no BLAS: the
    verbose build log shows one BLAS build in A's update and none in B's"""
    meshes = list(box_meshes())
    inst_a, inst_b = instances_of("13"), [(0, random_xforms(5, 21, spread=5.0)[k]) for k in range(4)] + [(1, None)]
    gm = [capi.Model(gpu, v, i) for v, i in meshes]
    a, b = capi.Scene(gpu), capi.Scene(gpu)
    for sc, inst in ((a, inst_a), (b, inst_b)):
        for mi, x in inst:
            sc.add_model(gm[mi], x)
        sc.build()
    new = displaced(meshes[0][0], seed=17)
    gm[0].set_vertices(new)
    final = [(new, meshes[0][1]), meshes[1]]
    for sc in (a, b):
        for call in stale_calls(sc):
            with pytest.raises(capi.RtError, match="vertices"):
                call()
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
    check(capi, gpu, oracle, a, gm, final, inst_a, "shared model, scene A")
    check(capi, gpu, oracle, b, gm, final, inst_b, "shared model, scene B")
    a.close(); b.close()
    for m in gm:
        m.close()


def test_states_and_their_messages(gpu, capi, oracle):
    meshes = list(box_meshes())
    inst = instances_of("13")[:5]
    gm = [capi.Model(gpu, v, i) for v, i in meshes]
    sc = capi.Scene(gpu)
    for mi, x in inst:
        sc.add_model(gm[mi], x)
    # never built: a set only changes the vertices, the build reads them
    v0 = displaced(meshes[0][0], seed=1)
    gm[0].set_vertices(v0)
    with pytest.raises(capi.RtError, match="rt_scene_update"):
        sc.update()
    sc.build()
    final = [(v0, meshes[0][1]), meshes[1]]
    before = check(capi, gpu, oracle, sc, gm, final, inst, "a set before the first build")
    # refused: ranges beyond the model, null sources, an unknown memory selector -- and nothing changes, the scene stays built
    nv = len(v0)
    lib, p = capi.lib(), v0.ctypes.data
    for call in (lambda: gm[0].set_vertices(v0[:2], nv - 1), lambda: gm[0].set_positions(v0["position"][:1], nv), lambda: gm[0].set_vertices(v0, 1),
                 lambda: gm[0].set_positions_device(p, 1, nv + 1), lambda: gm[0].set_vertices_device(p, 0xFFFFFFFF, 2)):
        with pytest.raises(capi.RtError, match="out of range") as e:
            call()
        assert e.value.code == -4
    assert lib.rt_model_set_vertices(gm[0].h, 0, 1, None, 0) == -1 and lib.rt_model_set_positions(gm[0].h, 0, 1, None, 1) == -1
    assert lib.rt_model_set_vertices(gm[0].h, 0, 1, p, 2) == -1 and lib.rt_model_set_positions(gm[0].h, 0, 0, p, 7) == -1
    gm[0].set_vertices(v0[:0], nv)                       # count == 0: RT_OK, nothing changes (first == n_verts is in range)
    gm[0].set_positions(np.zeros((0, 3), np.float32))
    assert lib.rt_model_set_vertices(gm[0].h, 0, 0, None, 0) == 0
    assert_bytes_equal(all_arrays(sc, gm, inst), before, "refused and empty sets")
    # stale: nothing traces or reads a scene whose model has pending vertices
    v1 = displaced(v0, seed=2)
    gm[0].set_positions(v1["position"])
    v1["normal"] = v0["normal"]
    for call in stale_calls(sc):
        with pytest.raises(capi.RtError, match="new vertices of the models of 3 instances pending") as e:
            call()
        assert e.value.code == -4
    pl = capi.Pipeline(gpu)
    pl.set_scene(sc)
    for _ in inst:
        pl.add_material(T.default_material())
    pl.set_environment_constant((0.5, 0.5, 0.5))
    pl.create_output(32, 32)
    cam = np.array([0, 2, 16, 0, 0, 0, 0, 1, 0, 0.8, 1.0], np.float32)
    pfc = frames_of(capi, cam, 1, 32, 32)[0]
    pl.update(pfc)
    for call in (pl.render, lambda: pl.render_batch([pfc])):
        with pytest.raises(capi.RtError, match="vertices"):
            call()
    # ... with a transform pending as well the message names both
    sc.set_transform(1, None)
    with pytest.raises(capi.RtError, match="vertices.*and 1 instance transform pending"):
        sc.trace(*RAYS)
    # rt_scene_build instead of rt_scene_update: the changed BLAS is rebuilt too
    sc.build()
    inst[1] = (inst[1][0], None)
    final = [(v1, meshes[0][1]), meshes[1]]
    before = check(capi, gpu, oracle, sc, gm, final, inst, "set + build")
    pl.render()
    work = pl.count_work()
    # nothing pending: no array and no generation changes
    sc.update()
    assert_bytes_equal(all_arrays(sc, gm, inst), before, "an update with nothing pending")
    assert pl.count_work() == work
    # ... while a real update is a change of scene: nothing rendered since
    gm[1].recompute_normals()
    sc.update()
    with pytest.raises(capi.RtError):
        pl.count_work()
    # instances added since the build: update refuses, build reads the vertices
    gm[0].set_vertices(v0)
    sc.add_model(gm[1], None)
    with pytest.raises(capi.RtError, match="rt_scene_update"):
        sc.update()
    sc.build()
    v_m1 = meshes[1][0].copy()
    v_m1["normal"] = normals_of(v_m1["position"], meshes[1][1])
    check(capi, gpu, oracle, sc, gm, [(v0, meshes[0][1]), (v_m1, meshes[1][1])], inst + [(1, None)], "build after a set and add_model")
    pl.close(); sc.close()
    for m in gm:
        m.close()


# ---- traversal ---------------------------------------------------------------------------------------------------------------------------
def test_traversal_after_a_deformation(gpu, capi, oracle):
    """13 instances of a blob and a soup; the soup displaced, the blob made slivers of (split references in a two-level scene): 20,000 aimed +
    random rays, production and canonical walk, closest / cull / any-hit == the oracle's BVH (built fresh) and its brute force, counters too"""
    models = two_models()
    xf = random_xforms(12, 21, spread=6.0)
    inst = [(k % 2, xf[k]) for k in range(12)] + [(0, None)]
    p = Pair(oracle, capi, gpu, models, inst)
    blob = slivers(models[0][0], models[0][1], 16)
    blob["position"] = (blob["position"] * np.float32(0.15)).astype(np.float32)        # (the slivers back into the neighbourhood of the instances)
    soup = displaced(models[1][0], seed=8, amount=0.7)
    p.gmodels[0].set_vertices(blob)
    p.gmodels[1].set_positions(soup["position"])
    soup["normal"] = models[1][0]["normal"]
    p.g.update()
    new = [(blob, models[0][1]), (soup, models[1][1])]
    assert p.g.refs(12)[0] is not None, "no split references: the case shows less than it says"
    pair = types.SimpleNamespace(g=p.g, o=make_oracle_scene(oracle, new, inst))
    sets = S.ray_sets(new, inst, None, 10000, 7)
    O = np.concatenate([sets["aimed"][0], sets["random"][0]])
    D = np.concatenate([sets["aimed"][1], sets["random"][1]])
    assert len(O) == 20000
    hit = pair.o.trace(O, D, flags=0, mode=1, nthreads=8)["inst"]
    assert len(np.unique(hit[hit != T.RT_NO_HIT])) == 13, "an instance no ray hits"
    compare_all(pair, O, D, brute=True)


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
def wave(verts, step):
    """the mesh breathing and leaning: every position scaled by 1 + 0.3 sin(step + 4 y) and pushed along x"""
    out = verts.copy()
    p = verts["position"].astype(np.float64)
    s = 1.0 + 0.3 * np.sin(0.9 * step + 4.0 * p[:, 1:2])
    out["position"] = (p * s + np.array([0.25 * np.sin(0.7 * step), 0, 0])).astype(np.float32)
    return out


def pipeline_over(capi, ctx, sc, mats, env, kind=None):
    p = capi.Pipeline(ctx) if kind is None else capi.Pipeline(ctx, kind)
    p.set_scene(sc)
    for m in mats:
        p.add_material(m)
    p.set_environment_cube(env)
    p.create_output(W, H)
    p.build_acceleration_structures()
    return p


def assert_frame(p, acc, ost, what):
    got = p.read_output()
    assert np.array_equal(got, acc), "%s: %d pixels differ" % (what, int((got != acc).any(axis=2).sum()))
    gst = p.stats()
    for key in COUNTS:
        assert gst[key] == ost[key], (what, key, gst[key], ost[key])


def test_progressive_frames_through_eight_deformations(gpu, capi, oracle):
    """set_shadow_cache(16) with per-pixel entries on and the free sphere, two frames so that all are warm; then eight steps of deform ->
    update -> clear_output -> render on ONE scene, the blob (model 0 of six instances) by set_vertices from the host on even steps and by
    set_positions from device memory + recompute_normals on odd ones: every frame == the oracle's on fresh scenes, ray counts included"""
    models, inst, mats, cam = light_scene()
    env = scenes.sky_cubemap(8)
    pfcs = frames_of(capi, cam, 10, W, H)
    gpu.set_option("shadow_cache_pixels", 1)
    try:
        sc, gm = own_scene(capi, gpu, models, inst)
        p = pipeline_over(capi, gpu, sc, mats, env)
        p.set_depth_limits(3, 3)
        p.set_shadow_cache(16)
        osc = make_oracle_scene(oracle, models, inst)
        acc = np.zeros((H, W, 4), np.float32)
        for pfc in pfcs[:2]:
            p.update(pfc); p.render()
            acc, ost = osc.render(np.stack(mats), pfc, W, H, accum=acc, env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
        assert_frame(p, acc, ost, "before any deformation")
        assert p.shadow_cache() == 16
        for step in range(8):
            blob = wave(models[0][0], step + 1)
            if step % 2 == 0:
                gm[0].set_vertices(blob)
            else:
                buf = gpu.upload(np.ascontiguousarray(blob["position"]))
                gm[0].set_positions_device(buf.ptr, len(blob))
                gm[0].recompute_normals()
                blob["normal"] = normals_of(blob["position"], models[0][1])
            sc.update()
            p.clear_output()
            assert gm[0].geometry()[0].tobytes() == blob.tobytes(), "step %d: geometry()" % step
            prev, osc = osc, make_oracle_scene(oracle, [(blob, models[0][1]), models[1]], inst)
            pfc = pfcs[2 + step]
            p.update(pfc); p.render()
            # (the oracle accumulates INTO the array it is given: an array of its own for each of the two images)
            acc, ost = osc.render(np.stack(mats), pfc, W, H, accum=np.zeros((H, W, 4), np.float32), env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
            assert_frame(p, acc, ost, "step %d" % step)
            stale, _ = prev.render(np.stack(mats), pfc, W, H, accum=np.zeros((H, W, 4), np.float32), env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
            assert int((acc != stale).any(axis=2).sum()) > 50, "step %d: the same frame over the mesh of the step before is nearly the same image" % step
        p.close()
        close_all(sc, gm)
    finally:
        gpu.set_option("shadow_cache_pixels", -1)


def test_realtime_pipeline_after_a_deformation(gpu, capi, oracle):
    """both AOVs == osc.render_realtime on the deformed mesh, ray counts included"""
    models, inst, mats, cam = light_scene()
    env = scenes.sky_cubemap(8)
    sc, gm = own_scene(capi, gpu, models, inst)
    p = pipeline_over(capi, gpu, sc, mats, env, capi.PIPELINE_REALTIME)
    host = capi.ProgressiveHost(10)
    pfc = host.update_realtime(cam, 0.0, 3, W, H)
    p.update(pfc); p.render()
    old = p.read_output(0)
    blob = wave(models[0][0], 3)
    gm[0].set_positions(blob["position"])
    gm[0].recompute_normals()
    blob["normal"] = normals_of(blob["position"], models[0][1])
    sc.update()
    pfc = host.update_realtime(cam, 0.0, 4, W, H)
    p.update(pfc); p.render()
    osc = make_oracle_scene(oracle, [(blob, models[0][1]), models[1]], inst)
    d, ind, ost = osc.render_realtime(np.stack(mats), pfc, W, H, env_faces=env, nthreads=8)
    assert np.array_equal(p.read_output(0), d), "direct-lighting AOV: %d pixels differ" % int((p.read_output(0) != d).any(axis=2).sum())
    assert np.array_equal(p.read_output(1), ind), "indirect-specular AOV: %d pixels differ" % int((p.read_output(1) != ind).any(axis=2).sum())
    gst = p.stats()
    for key in COUNTS:
        assert gst[key] == ost[key], (key, gst[key], ost[key])
    assert 0 < ost["primary_hits"] < W * H and not np.array_equal(d, old)
    p.close()
    close_all(sc, gm)


def test_deferred_frames_see_the_mesh_they_were_accepted_with(gpu, capi, oracle):
    """set_deferred(4): two frames recorded, a set (it flushes them before the first byte changes: they see the mesh as it was), update, two
    more, read: the image == the oracle's frames 1 - 2 on the old mesh accumulated with 3 - 4 on the new"""
    models, inst, mats, cam = light_scene()
    env = scenes.sky_cubemap(8)
    pfcs = frames_of(capi, cam, 4, W, H)
    sc, gm = own_scene(capi, gpu, models, inst)
    p = pipeline_over(capi, gpu, sc, mats, env)
    p.set_depth_limits(3, 3)
    p.set_deferred(4)
    for pfc in pfcs[:2]:
        p.update(pfc); p.render()
    assert p.deferred() == (4, 2)
    blob = wave(models[0][0], 2)
    buf = gpu.upload(blob)
    gm[0].set_vertices_device(buf.ptr, len(blob))
    assert p.deferred() == (4, 0), "the set did not flush the recorded frames"
    sc.update()
    for pfc in pfcs[2:]:
        p.update(pfc); p.render()
    assert p.deferred() == (4, 2)
    acc = np.zeros((H, W, 4), np.float32)
    for osc, some in ((make_oracle_scene(oracle, models, inst), pfcs[:2]), (make_oracle_scene(oracle, [(blob, models[0][1]), models[1]], inst), pfcs[2:])):
        for pfc in some:
            acc, _ = osc.render(np.stack(mats), pfc, W, H, accum=acc, env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
    got = p.read_output()
    assert np.array_equal(got, acc), "%d pixels differ" % int((got != acc).any(axis=2).sum())
    p.close()
    close_all(sc, gm)


# ---- builder options -------------------------------------------------------------------------------------------------------------------
def options_truth(oracle):
    """the oracle's side, once for all rows: five instances of the unsplit grid and a soup, the grid made slivers of (every 16th triangle) and
    displaced; 3,000 rays' closest and any hits"""
    if "options" not in _cache:
        v, idx = unsplit_grid()
        xf = random_xforms(5, 31, spread=3.0)
        inst = [(0, None), (1, xf[1]), (0, xf[2]), (1, xf[3]), (0, xf[4])]
        new = displaced(slivers(v, idx, 16), seed=23, amount=0.2)
        final = [(new, idx), box_meshes()[1]]
        osc = make_oracle_scene(oracle, final, inst)
        assert osc.refs(0, len(idx))[0] is not None
        sets = S.ray_sets(final, inst, None, 1500, 3)
        O = np.concatenate([sets["aimed"][0], sets["random"][0]])
        D = np.concatenate([sets["aimed"][1], sets["random"][1]])
        hits = {flags: osc.trace(O, D, flags=flags, mode=1, nthreads=8) for flags in (0, ANY)}
        assert int((hits[0]["inst"] != T.RT_NO_HIT).sum()) > 500
        _cache["options"] = types.SimpleNamespace(start=[(v, idx), box_meshes()[1]], final=final, inst=inst, new=new, osc=osc, O=O, D=D, hits=hits)
    return _cache["options"]


@pytest.mark.parametrize("row", range(len(BUILD_ROWS)), ids=lambda r: _case_id(BUILD_ROWS[r]))
def test_deformation_under_builder_options(oracle, capi, row):
    """one deformation per row of BUILD_ROWS (leaf sizes, the LBVH layout, the surface-area collapse, split references off, batched rounds): a
    grid that gains split references, by set_vertices + update on a context with the row's options == a fresh build on the same context,
    == the oracle's canonical arrays; closest and any hits of 3,000 rays == the oracle's"""
    opts = BUILD_ROWS[row]
    u = options_truth(oracle)
    what = "deformation under %s" % (opts,)
    ctx = context(capi, opts)
    try:
        sc, gm = own_scene(capi, ctx, u.start, u.inst)
        before = all_arrays(sc, gm, u.inst)
        gm[0].set_vertices(u.new)
        sc.update()
        got = check(capi, ctx, oracle, sc, gm, u.final, u.inst, what, before, deformed={0})
        split_layout = opts["fast_bvh"] == "ploc" and opts["split_refs"] == 1
        assert (got["model0.counts"][1] > len(u.final[0][1])) == split_layout, (what, got["model0.counts"])
        assert_hits_equal(sc.trace(u.O, u.D, flags=0), u.hits[0], what + " closest")
        assert_hits_equal(sc.trace(u.O, u.D, flags=ANY), u.hits[ANY], what + " any-hit", closest=False)
        close_all(sc, gm)
    finally:
        ctx.close()


# ---- normals -----------------------------------------------------------------------------------------------------------------------------
def normal_meshes():
    """name -> (positions, indices): the index lists of deform_cases.index_lists() with positions -- the curved 9 x 9 grid (valence 1 .. 6), a
    soup (valence 1), a vertex no triangle names, triangles naming a vertex twice and thrice, a fan of zero area (-> zeros), coordinates of
    1e20 (d overflows -> zeros)"""
    lists = index_lists()
    r = np.random.default_rng(4)
    out = {"grid": (grid_mesh()[0]["position"], lists["grid"][1])}
    for name in ("soup", "unnamed", "twice", "one"):
        nv, idx = lists[name]
        out[name] = (r.uniform(-1, 1, (nv, 3)).astype(np.float32), idx)
    nv, idx = lists["fan"]
    out["flat_fan"] = (np.outer(np.arange(nv), [0.5, 0.25, -1.0]).astype(np.float32), idx)            # every vertex on one line
    out["huge_fan"] = ((r.uniform(-1, 1, (nv, 3)) * 1e20).astype(np.float32), idx)
    return out


@pytest.mark.parametrize("name", ["grid", "soup", "unnamed", "twice", "one", "flat_fan", "huge_fan"])
def test_recompute_normals_is_its_definition(gpu, capi, name):
    pos, idx = normal_meshes()[name]
    v = np.zeros(len(pos), T.VERTEX)
    v["position"] = pos
    v["normal"] = [0.25, 0.5, -0.75]                     # (so that a normal nobody wrote shows)
    m = capi.Model(gpu, v, idx)
    m.recompute_normals()
    got, _ = m.geometry()
    want = normals_of(pos, idx)
    assert got["position"].tobytes() == pos.tobytes()
    assert got["normal"].tobytes() == want.tobytes(), "%s: %d normals differ" % (name, int((got["normal"] != want).any(axis=1).sum()))
    if name in ("flat_fan", "huge_fan"):
        assert not want.any()
    elif name == "unnamed":
        assert not want[3].any() and not want[5].any() and want[:3].any(axis=1).all()
    else:
        assert np.allclose(np.linalg.norm(want[want.any(axis=1)].astype(np.float64), axis=1), 1.0, atol=1e-6)
    # a second call on moved positions: the table made by the first call serves
    pos2 = (pos * np.float32(0.5) + np.float32(0.125)).astype(np.float32)
    m.set_positions(pos2)
    m.recompute_normals()
    assert m.geometry()[0]["normal"].tobytes() == normals_of(pos2, idx).tobytes()
    m.close()


def test_frame_shaded_with_recomputed_normals(gpu, capi, oracle):
    """the curved grid, flattened differently by set_positions, its normals recomputed: two progressive frames == the oracle's on a mesh fed
    the numpy normals"""
    v, idx = grid_mesh()
    inst = [(0, None), (0, random_xforms(1, 6, spread=1.5)[0])]
    mats = [T.default_material(), T.default_material()]
    mats[1]["type"] = 1
    env = scenes.sky_cubemap(8)
    sc, gm = own_scene(capi, gpu, [(v, idx)], inst)
    p = pipeline_over(capi, gpu, sc, mats, env)
    new = v.copy()
    new["position"][:, 1] = (0.5 * np.cos(2.0 * v["position"][:, 0]) * np.sin(1.5 * v["position"][:, 2])).astype(np.float32)
    gm[0].set_positions(new["position"])
    gm[0].recompute_normals()
    sc.update()
    new["normal"] = normals_of(new["position"], idx)
    assert not np.array_equal(new["normal"], v["normal"])
    osc = make_oracle_scene(oracle, [(new, idx)], inst)
    cam = np.array([0.5, 3.0, 3.0, 0, 0, 0, 0, 1, 0, 0.8, W / H], np.float32)
    acc = np.zeros((H, W, 4), np.float32)
    for pfc in frames_of(capi, cam, 2, W, H):
        p.update(pfc); p.render()
        acc, ost = osc.render(np.stack(mats), pfc, W, H, accum=acc, env_faces=env, nthreads=8)
    assert_frame(p, acc, ost, "recomputed normals")
    assert 0 < ost["primary_hits"] < W * H
    p.close()
    close_all(sc, gm)


def test_deforming_example_through_the_cpp_mirror(tmp_path):
    """examples/realtime_deform.cpp: RtModel::setPositions + recomputeNormals + RtScene::update per frame, end to end; waved for three frames
    the image is another than waved for one"""
    import os
    import subprocess
    from util import GOLDEN
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dxrexperiments_amd", "lib", "realtime_deform")
    images = []
    for frames in (1, 3):
        out = tmp_path / ("out%d.pfm" % frames)
        r = subprocess.run([exe, os.path.join(GOLDEN, "susanne.obj"), "96", "64", str(frames), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "waving vertices: %d frames" % frames in r.stdout and "BLAS + TLAS update" in r.stdout
        raw = out.read_bytes()
        head = b"PF\n96 64\n-1.0\n"
        assert raw.startswith(head)
        images.append(np.frombuffer(raw[len(head):], "<f4").reshape(64, 96, 3))
    assert images[0].max() > 0.1 and images[0].std() > 0.01            # an image, not a constant
    assert not np.array_equal(images[0], images[1])
