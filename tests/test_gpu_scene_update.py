"""Rigid animation (rt_scene_set_instance_transform(s) + rt_scene_update): a scene after `set transforms + update` is, array for array,
the scene a fresh build of the same instance list gives -- the TLAS' canonical arrays, its production layout and every instance record
byte-equal to a second GPU scene built from scratch with the final transforms, and equal to the oracle's, which is never updated: it is
built fresh with the new instance list.  Then traversal (production and canonical walk, closest / cull / any-hit, against the oracle's BVH
and brute force), whole frames through pipelines that had cached what the old geometry looked like (shadow cache, free sphere, deferred
frames, realtime AOVs, queues sized by count), and the states in between: a scene with pending transforms is stale and nothing reads it."""
import types

import numpy as np
import pytest

import s2_truth as S
from dxrexperiments_amd import rtypes as T, scenes
from test_gpu_batch import frames_of
from test_gpu_instance_transforms import COUNTS, frame_scene, two_models
from test_gpu_pipeline import make_gpu_pipeline, make_oracle_scene
from test_gpu_realtime_denoise import realtime_pair
from test_gpu_trace import compare_all
from util import HARD_FAMILIES, Pair, hard_xforms, random_xforms, triangle_soup, world_box_of_vertices

pytestmark = pytest.mark.gpu

W, H = 96, 64
_cache = {}


def box_meshes():
    """test_instance_world_boxes_under_hard_transforms' two meshes: 4,200 vertex references (two work items of 4,096) and 4,095 (just under one)"""
    if "meshes" not in _cache:
        _cache["meshes"] = [triangle_soup(1400, seed=31, extent=2.0, size=0.3), triangle_soup(1365, seed=32, extent=2.0, size=0.3)]
    return _cache["meshes"]


def gpu_models(capi, gpu):
    """the GPU models of those meshes, shared by every scene of this file (a built model is not built again)"""
    if "gmodels" not in _cache:
        _cache["gmodels"] = [capi.Model(gpu, v, i) for v, i in box_meshes()]
    return _cache["gmodels"]


def gpu_scene(capi, gpu, xforms):
    """instance k = mesh k % 2 under xforms[k] (None: identity), built"""
    gm = gpu_models(capi, gpu)
    sc = capi.Scene(gpu)
    for k, x in enumerate(xforms):
        sc.add_model(gm[k % 2], x)
    sc.build()
    return sc


def oracle_scene(oracle, xforms):
    return make_oracle_scene(oracle, box_meshes(), [(k % 2, x) for k, x in enumerate(xforms)])


def arrays(sc, n):
    """everything the issue's definition names: bvh(-1) (nodes, sorted keys, parents, depth), wide_read(-1), wide_counts(-1), instance_info(k)"""
    nodes, keys, parents, depth = sc.bvh(-1)
    wn, root, _ = sc.wide_read(-1)
    info = [sc.instance_info(k) for k in range(n)]
    return dict(nodes=nodes, keys=keys, parents=parents, depth=depth, wide=wn, root=root, counts=sc.wide_counts(-1),
                boxes=np.stack([b for b, _ in info]), invs=np.stack([i for _, i in info]))


def assert_bytes_equal(a, b, what):
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: %s differs" % (what, key)
        else:
            assert x == y, "%s: %s differs (%r vs %r)" % (what, key, x, y)


def assert_equals_oracle(a, osc, n, what):
    on, ok, op, od = osc.bvh(-1)
    assert np.array_equal(a["keys"], ok) and np.array_equal(a["parents"], op) and a["depth"] == od, "%s: keys / parents / depth differ from the oracle's" % what
    for f in ("left", "right"):
        assert np.array_equal(a["nodes"][f], on[f]), "%s: node.%s differs from the oracle's" % (what, f)
    for f in ("bmin", "bmax"):
        assert np.array_equal(a["nodes"][f], on[f], equal_nan=True), "%s: node.%s differs from the oracle's" % (what, f)
    for k in range(n):
        ob, oi = osc.instance_info(k)
        assert np.array_equal(a["invs"][k], oi, equal_nan=True), (what, k, a["invs"][k], oi)
        assert np.array_equal(a["boxes"][k], ob, equal_nan=True), (what, k, a["boxes"][k], ob)


def check_update(capi, gpu, oracle, sc, final, what, before=None, touched=()):
    """sc (already updated to `final`) against a fresh GPU scene and a fresh oracle scene of the final list; untouched records as before"""
    n = len(final)
    got = arrays(sc, n)
    fresh = gpu_scene(capi, gpu, final)
    assert_bytes_equal(got, arrays(fresh, n), what + " vs a fresh GPU build")
    assert_equals_oracle(got, oracle_scene(oracle, final), n, what)
    if before is not None:
        for k in range(n):
            if k not in touched:
                assert got["boxes"][k].tobytes() == before["boxes"][k].tobytes() and got["invs"][k].tobytes() == before["invs"][k].tobytes(), (what, k)
    fresh.close()
    return got


def start_xforms(n, seed=3):
    """random transforms; the scene of 13 is 12 + one identity instance"""
    xf = [x for x in random_xforms(n, seed, spread=6.0)]
    if n == 13:
        xf[12] = None
    return xf


PENDING = {
    "none": lambda n: [],
    "first": lambda n: [0],
    "last": lambda n: [n - 1],
    "all": lambda n: list(range(n)),
    "every_second": lambda n: list(range(0, n, 2)),
    "run63": lambda n: list(range(100, 163)),          # the compaction's wave edge: 63 / 64 / 65 consecutive instances, not wave aligned
    "run64": lambda n: list(range(100, 164)),
    "run65": lambda n: list(range(100, 165)),
}
ARRAY_CASES = [(n, p) for n in (1, 2, 5, 13, 300) for p in ("none", "first", "last", "all", "every_second")] + [(300, p) for p in ("run63", "run64", "run65")]


@pytest.mark.parametrize("n,pending", ARRAY_CASES)
def test_update_equals_build(gpu, capi, oracle, n, pending):
    """n = 1, 2, 5 (a partly filled wide node), 13 and 300 (more TLAS nodes than the 128 of the LDS top); pending sets none, one (first;
    last), all, every second and 63 / 64 / 65 consecutive instances: bvh(-1), wide_read(-1), wide_counts(-1) and every instance_info byte-equal
    to a fresh build, equal to the oracle's, untouched instances as they were"""
    xf = start_xforms(n)
    sc = gpu_scene(capi, gpu, xf)
    before = arrays(sc, n)
    new = random_xforms(n, 77, spread=6.0)
    which = PENDING[pending](n)
    final = list(xf)
    runs = []
    for k in which:
        final[k] = new[k]
        if runs and runs[-1][0] + len(runs[-1][1]) == k:
            runs[-1][1].append(new[k])
        else:
            runs.append((k, [new[k]]))
    for first, xs in runs:                              # one instance: the singular call; a run: the plural one
        if len(xs) == 1:
            sc.set_transform(first, xs[0])
        else:
            sc.set_transforms(first, xs)
    sc.update()
    check_update(capi, gpu, oracle, sc, final, "n=%d %s" % (n, pending), before, set(which))
    sc.close()


@pytest.mark.parametrize("family", HARD_FAMILIES + ("extreme", "degenerate"))
def test_update_to_hard_transforms_and_on(gpu, capi, oracle, family):
    """13 instances (12 + one identity): all twelve to the family's transforms (inf / NaN inverses and boxes bit for bit), == the numpy
    statement of the world box; then a second update on top of the first: the identity instance gets a transform, instance 0 becomes an
    identity instance, the odd ones go back to where they started; then a third that takes the identity -> transformed step back"""
    n = 13
    xf = start_xforms(n)
    sc = gpu_scene(capi, gpu, xf)
    hard = hard_xforms(family, 12, seed=13)
    final = [hard[k] for k in range(12)] + [None]
    sc.set_transforms(0, hard)
    sc.update()
    got = check_update(capi, gpu, oracle, sc, final, family + " first update")
    meshes = box_meshes()
    for k in range(12):
        assert np.array_equal(got["boxes"][k], world_box_of_vertices(*meshes[k % 2], hard[k]), equal_nan=True), (family, k)
    before = got
    second = list(final)
    second[12] = hard[3]
    second[0] = None
    sc.set_transform(12, hard[3])
    sc.set_transform(0, None)
    for k in range(1, 12, 2):
        second[k] = xf[k]
        sc.set_transform(k, xf[k])
    sc.update()
    before = check_update(capi, gpu, oracle, sc, second, family + " second update", before, {0, 12} | set(range(1, 12, 2)))
    third = list(second)
    third[12] = None
    third[0] = hard[0]
    sc.set_transforms(12, [None])
    sc.set_transform(0, hard[0])
    sc.update()
    check_update(capi, gpu, oracle, sc, third, family + " third update", before, {0, 12})
    sc.close()


def test_two_instances_exchange_their_transforms(gpu, capi, oracle):
    """the same boxes in another Morton order: instances 2 and 4 (the same mesh) swap places, so do 1 and 12 (mesh 1 and the identity mesh 0)"""
    n = 13
    xf = start_xforms(n)
    sc = gpu_scene(capi, gpu, xf)
    before = arrays(sc, n)
    final = list(xf)
    final[2], final[4] = xf[4], xf[2]
    final[1], final[12] = xf[12], xf[1]
    for k in (2, 4, 1, 12):
        sc.set_transform(k, final[k])
    sc.update()
    got = check_update(capi, gpu, oracle, sc, final, "exchange", before, {1, 2, 4, 12})
    assert np.array_equal(got["boxes"][2], before["boxes"][4]) and np.array_equal(got["boxes"][4], before["boxes"][2])
    assert not np.array_equal(got["keys"], before["keys"])
    sc.close()


def test_set_and_build_equals_set_and_update(gpu, capi):
    """rt_scene_build after setters keeps working (the full path, cached BLASes) and is the statement update is held to: byte for byte"""
    n = 13
    xf = start_xforms(n)
    new = hard_xforms("shear", n, seed=4)
    a, b = gpu_scene(capi, gpu, xf), gpu_scene(capi, gpu, xf)
    a.set_transforms(0, new)
    b.set_transforms(0, new)
    a.build()
    b.update()
    assert_bytes_equal(arrays(a, n), arrays(b, n), "set + build vs set + update")
    assert b.update_ms() > 0.0
    a.close(); b.close()


# ---- a fresh build is an update with every instance listed ---------------------------------------------------------------------------
FRESH_PATTERNS = {                                      # which instances carry a transform (the others are identity instances)
    "all_transformed": lambda n, k: True,
    "all_identity": lambda n, k: False,                 # the work list stays empty while the world-box grid is not
    "first_wave_identity": lambda n, k: k >= 64,        # a whole first wave of k_update_records without work items: its early return
    "alternating": lambda n, k: k % 2 == 1,
    "last_transformed": lambda n, k: k == n - 1,
}


def fresh_xforms(n, pattern):
    xf = random_xforms(n, 41, spread=6.0)
    return [xf[k] if FRESH_PATTERNS[pattern](n, k) else None for k in range(n)]


FRESH_CASES = [(n, p, 0) for n in (63, 64, 65, 130) for p in FRESH_PATTERNS] + [(130, "first_wave_identity", 64)]


@pytest.mark.parametrize("n,pattern,hidden", FRESH_CASES)
def test_fresh_build_compacts_its_work_list(gpu, capi, oracle, n, pattern, hidden):
    """no setter, no update: the build itself runs the compaction of k_update_records over all n instances -- one wave less one, one wave, one
    wave and one, three waves -- under every identity pattern: bvh(-1) and every instance_info == the oracle's.  The last case hides the
    identity wave 0..63 before the build: the TLAS, in the sub-list's numbering, == the oracle's scene of the visible instances 64..129 (as
    test_gpu_instance_masks compares it); every record, the hidden ones' too, == the oracle's scene of the full list"""
    xf = fresh_xforms(n, pattern)
    what = "fresh build n=%d %s, %d hidden" % (n, pattern, hidden)
    gm = gpu_models(capi, gpu)
    sc = capi.Scene(gpu)
    for k, x in enumerate(xf):
        sc.add_model(gm[k % 2], x)
    if hidden:
        sc.set_masks(0, np.array([0] * hidden + [0xFF] * (n - hidden), np.uint8))
    sc.build()
    got = arrays(sc, n)
    full = oracle_scene(oracle, xf)
    if not hidden:
        assert_equals_oracle(got, full, n, what)
    else:
        from test_gpu_instance_masks import unmapped    # (that module imports this one)
        assert hidden % 2 == 0                          # (the sub-list keeps "instance k = mesh k % 2")
        vis = list(range(hidden, n))
        assert got["keys"].shape[0] == len(vis)
        assert_equals_oracle(unmapped(got, vis), oracle_scene(oracle, xf[hidden:]), len(vis), what)
        for k in range(n):
            ob, oi = full.instance_info(k)
            assert np.array_equal(got["invs"][k], oi, equal_nan=True) and np.array_equal(got["boxes"][k], ob, equal_nan=True), (what, k, got["boxes"][k], ob)
    sc.close()


# ---- traversal -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("mirror", "stretch", "far"))
def test_traversal_after_an_update(gpu, capi, oracle, family):
    """from random_xforms to the family's transforms by an update: 20,000 aimed + random rays laid out over the NEW instances, production and
    canonical walk, closest / cull / any-hit == the oracle's BVH (built fresh from the new list) and its brute force, counters included"""
    models = two_models()
    start = random_xforms(12, 21, spread=6.0)
    p = Pair(oracle, capi, gpu, models, [(k % 2, start[k]) for k in range(12)] + [(0, None)])
    new = hard_xforms(family, 12, seed=5)
    inst = [(k % 2, new[k]) for k in range(12)] + [(0, None)]
    p.g.set_transforms(0, new)
    p.g.update()
    pair = types.SimpleNamespace(g=p.g, o=make_oracle_scene(oracle, models, inst))
    sets = S.ray_sets(models, inst, None, 10000, 7)
    O = np.concatenate([sets["aimed"][0], sets["random"][0]])
    D = np.concatenate([sets["aimed"][1], sets["random"][1]])
    assert len(O) == 20000
    hit = pair.o.trace(O, D, flags=0, mode=1, nthreads=8)["inst"]
    assert len(np.unique(hit[hit != T.RT_NO_HIT])) == 13, "an instance no ray hits"
    compare_all(pair, O, D, brute=True)


def test_one_instance_between_single_and_two_level(gpu, capi, oracle):
    """n = 1: an identity instance (rays walk its BLAS directly) given a transform becomes a two-level scene and traces as the oracle does; set
    back to the identity it is single-level again -- its arrays those of a fresh scene, its hits and counters the oracle's"""
    models = [two_models()[0]]
    p = Pair(oracle, capi, gpu, models, [(0, None)])
    x = random_xforms(1, 9, spread=2.0)[0]
    for step, xf in enumerate((x, None, x)):
        p.g.set_transform(0, xf)
        p.g.update()
        inst = [(0, xf)]
        fresh = Pair(oracle, capi, gpu, models, inst)
        assert_bytes_equal(arrays(p.g, 1), arrays(fresh.g, 1), "n = 1 step %d" % step)
        sets = S.ray_sets(models, inst, None, 3000, 11 + step)
        O = np.concatenate([sets["aimed"][0], sets["random"][0]])
        D = np.concatenate([sets["aimed"][1], sets["random"][1]])
        pair = types.SimpleNamespace(g=p.g, o=fresh.o)
        assert int((fresh.o.trace(O, D, flags=0, mode=1, nthreads=8)["inst"] != T.RT_NO_HIT).sum()) > 1000
        compare_all(pair, O, D, brute=True)
        # ... and by the same kernels as the fresh scene: the canonical walk's counters say which levels were walked
        a, b = p.g.trace(O, D, canonical=True), fresh.g.trace(O, D, canonical=True)
        assert np.array_equal(a["nodes"], b["nodes"]) and np.array_equal(a["tris"], b["tris"])


# ---- pipelines -----------------------------------------------------------------------------------------------------------------------
def light_scene():
    """frame_scene's models, materials (every type) and camera under ordinary transforms"""
    models, _, mats, _ = frame_scene("mirror")
    xf = random_xforms(12, seed=11, spread=6.0)
    inst = [(k % 2, xf[k]) for k in range(12)]
    cam = np.array([0, 2, 16, 0, 0, 0, 0, 1, 0, 0.8, W / H], np.float32)
    return models, inst, mats, cam


def translated(x, to):
    """the transform x with its translation replaced"""
    m = np.array(x, np.float32).reshape(3, 4).copy()
    m[:, 3] = to
    return m.reshape(12)


def oracle_frames(osc, mats, pfcs, env, acc=None):
    acc = np.zeros((H, W, 4), np.float32) if acc is None else acc
    st = None
    for pfc in pfcs:
        acc, st = osc.render(np.stack(mats), pfc, W, H, accum=acc, env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
    return acc, st


def test_shadow_cache_does_not_outlive_an_update(gpu, capi, oracle):
    """set_shadow_cache(16) with per-pixel entries on, two frames so that both are warm; the instance between the light and the others moves out
    of the light's way; update, clear_output: two frames == osc.render on the new instance list, ray counts included"""
    models, inst, mats, cam = light_scene()
    env = scenes.sky_cubemap(8)
    pfcs = frames_of(capi, cam, 4, W, H)
    lp = np.array(pfcs[0]["pointLight"]["worldPos"][:3], np.float64)
    centre = np.mean([np.asarray(x, np.float64).reshape(3, 4)[:, 3] for _, x in inst], axis=0)
    toward = (centre - lp) / np.linalg.norm(centre - lp)
    inst[0] = (0, translated(inst[0][1], lp + 1.6 * toward))          # the blob right under the light: the occluder of most shadow rays
    gpu.set_option("shadow_cache_pixels", 1)
    try:
        p = make_gpu_pipeline(capi, gpu, models, inst, mats, W, H, env=env)
        p.set_depth_limits(3, 3)
        p.set_shadow_cache(16)
        old_acc, old_st = oracle_frames(make_oracle_scene(oracle, models, inst), mats, pfcs[:2], env)
        for pfc in pfcs[:2]:
            p.update(pfc); p.render()
        assert np.array_equal(p.read_output(), old_acc) and p.shadow_cache() == 16
        sc = p._keep[0]
        new_inst = list(inst)
        new_inst[0] = (0, translated(inst[0][1], lp - 40.0 * toward))
        sc.set_transform(0, new_inst[0][1])
        sc.update()
        p.clear_output()
        osc = make_oracle_scene(oracle, models, new_inst)
        acc = np.zeros((H, W, 4), np.float32)
        for f, pfc in enumerate(pfcs[:2]):
            p.update(pfc); p.render()
            acc, ost = osc.render(np.stack(mats), pfc, W, H, accum=acc, env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
            assert np.array_equal(p.read_output(), acc), "frame %d after the update: %d pixels differ" % (f, int((p.read_output() != acc).any(axis=2).sum()))
            gst = p.stats()
            for key in COUNTS:
                assert gst[key] == ost[key], (f, key, gst[key], ost[key])
        assert not np.array_equal(acc, old_acc), "the move changed nothing: the test shows nothing"
        p.close()
    finally:
        gpu.set_option("shadow_cache_pixels", -1)


def box_distance(box, point):
    lo, hi = box[:3].astype(np.float64), box[3:].astype(np.float64)
    d = np.maximum(np.maximum(lo - point, point - hi), 0.0)
    return float(np.sqrt((d * d).sum()))


def test_free_sphere_does_not_outlive_an_update(gpu, capi, oracle):
    """an instance moves INTO the free sphere that free_sphere() reported before the update: the frames == the oracle's, and the radius reported
    afterwards is no larger than the distance to the moved instance's world box"""
    models, inst, mats, cam = light_scene()
    env = scenes.sky_cubemap(8)
    pfcs = frames_of(capi, cam, 5, W, H)
    lp = np.array(pfcs[0]["pointLight"]["worldPos"][:3], np.float64)
    p = make_gpu_pipeline(capi, gpu, models, inst, mats, W, H, env=env)
    p.set_depth_limits(3, 3)
    for pfc in pfcs[:2]:
        p.update(pfc); p.render()
    p.read_output()                                      # (waits for the stream: the radius has landed)
    r0 = p.free_sphere()
    assert r0 > 0.5, r0
    sc = p._keep[0]
    small = np.array(inst[1][1], np.float32).reshape(3, 4).copy()
    small[:, :3] *= np.float32(0.12 * r0)                # the soup (extent 1.5, triangles of 0.4, scaled by up to 1.5) shrunk to reach into the sphere
    small[:, 3] = lp + np.array([0.0, -0.55 * r0, 0.0])
    new_inst = list(inst)
    new_inst[1] = (1, small.reshape(12))
    sc.set_transform(1, new_inst[1][1])
    sc.update()
    p.clear_output()
    dist = box_distance(sc.instance_info(1)[0], lp)
    assert dist < r0, (dist, r0)
    osc = make_oracle_scene(oracle, models, new_inst)
    acc = np.zeros((H, W, 4), np.float32)
    for f, pfc in enumerate(pfcs[:3]):
        p.update(pfc); p.render()
        acc, ost = osc.render(np.stack(mats), pfc, W, H, accum=acc, env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
        assert np.array_equal(p.read_output(), acc), "frame %d after the update: %d pixels differ" % (f, int((p.read_output() != acc).any(axis=2).sum()))
        gst = p.stats()
        for key in COUNTS:
            assert gst[key] == ost[key], (f, key, gst[key], ost[key])
    assert 0.0 <= p.free_sphere() <= dist, (p.free_sphere(), dist)
    p.close()


def test_deferred_frames_see_the_scene_they_were_accepted_with(gpu, capi, oracle):
    """set_deferred(4): two frames recorded, a setter (it flushes them: they see the scene as it was), update, two more, read: the image == the
    oracle's frames 1 - 2 on the old list accumulated with 3 - 4 on the new"""
    models, inst, mats, cam = light_scene()
    env = scenes.sky_cubemap(8)
    pfcs = frames_of(capi, cam, 4, W, H)
    p = make_gpu_pipeline(capi, gpu, models, inst, mats, W, H, env=env)
    p.set_depth_limits(3, 3)
    p.set_deferred(4)
    for pfc in pfcs[:2]:
        p.update(pfc); p.render()
    assert p.deferred() == (4, 2)
    sc = p._keep[0]
    new = hard_xforms("mirror", 12, seed=5)
    new_inst = [(k % 2, new[k]) if k % 3 else inst[k] for k in range(12)]
    for k in range(12):
        if k % 3:
            sc.set_transform(k, new[k])
            assert p.deferred() == (4, 0), "the setter did not flush the recorded frames"
    sc.update()
    for pfc in pfcs[2:]:
        p.update(pfc); p.render()
    assert p.deferred() == (4, 2)
    acc, _ = oracle_frames(make_oracle_scene(oracle, models, inst), mats, pfcs[:2], env)
    acc, _ = oracle_frames(make_oracle_scene(oracle, models, new_inst), mats, pfcs[2:], env, acc)
    got = p.read_output()
    assert np.array_equal(got, acc), "%d pixels differ" % int((got != acc).any(axis=2).sum())
    p.close()


def test_realtime_pipeline_after_an_update(gpu, capi, oracle):
    """both AOVs == osc.render_realtime on the new instance list, ray counts included"""
    models, inst, mats, cam = frame_scene("shear")
    _, new_inst, _, cam = frame_scene("mirror")
    env = scenes.sky_cubemap(8)
    p, _ = realtime_pair(capi, oracle, gpu, models, inst, mats, W, H, env)
    host = capi.ProgressiveHost(10)
    pfc = host.update_realtime(cam, 0.0, 3, W, H)
    p.update(pfc); p.render()
    sc = p._keep[0]
    sc.set_transforms(0, [x for _, x in new_inst])
    sc.update()
    pfc = host.update_realtime(cam, 0.0, 4, W, H)
    p.update(pfc); p.render()
    osc = make_oracle_scene(oracle, models, new_inst)
    d, ind, ost = osc.render_realtime(np.stack(mats), pfc, W, H, env_faces=env, nthreads=8)
    assert np.array_equal(p.read_output(0), d), "direct-lighting AOV: %d pixels differ" % int((p.read_output(0) != d).any(axis=2).sum())
    assert np.array_equal(p.read_output(1), ind), "indirect-specular AOV: %d pixels differ" % int((p.read_output(1) != ind).any(axis=2).sum())
    gst = p.stats()
    for key in COUNTS:
        assert gst[key] == ost[key], (key, gst[key], ost[key])
    assert 0 < ost["primary_hits"] < W * H
    p.close()


def test_queues_sized_by_count_after_an_update(gpu, capi, oracle):
    """render_batch with set_queue_budget(1) after an update == the oracle's frames"""
    models, inst, mats, cam = frame_scene("shear")
    _, new_inst, _, cam = frame_scene("mirror")
    env = scenes.sky_cubemap(8)
    pfcs = frames_of(capi, cam, 3, W, H)
    p = make_gpu_pipeline(capi, gpu, models, inst, mats, W, H, env=env)
    p.set_depth_limits(3, 3)
    p.update(pfcs[0]); p.render()
    sc = p._keep[0]
    sc.set_transforms(0, [x for _, x in new_inst])
    sc.update()
    p.clear_output()
    p.set_queue_budget(1)
    p.render_batch(pfcs)
    acc, _ = oracle_frames(make_oracle_scene(oracle, models, new_inst), mats, pfcs, env)
    assert np.array_equal(p.read_output(), acc), "%d pixels differ" % int((p.read_output() != acc).any(axis=2).sum())
    assert p.queue_memory()[1], "the set did not size its levels by count"
    p.close()


# ---- state ---------------------------------------------------------------------------------------------------------------------------
def test_states_and_their_messages(gpu, capi):
    n = 5
    xf = start_xforms(n)
    gm = gpu_models(capi, gpu)
    sc = capi.Scene(gpu)
    for k in range(n):
        sc.add_model(gm[k % 2], xf[k])
    # never built: a setter only overwrites the stored transform, update fails (it builds no BLAS)
    new = random_xforms(n, 78, spread=6.0)
    sc.set_transform(1, new[1])
    with pytest.raises(capi.RtError, match="rt_scene_update"):
        sc.update()
    for call in (lambda: sc.set_transform(n, new[0]), lambda: sc.set_transforms(n - 1, new[:2]), lambda: sc.set_transforms(n + 1, [])):
        with pytest.raises(capi.RtError, match="out of range"):
            call()
    sc.build()
    final = list(xf)
    final[1] = new[1]
    fresh = gpu_scene(capi, gpu, final)
    assert_bytes_equal(arrays(sc, n), arrays(fresh, n), "a setter before the first build")
    # stale: nothing traces or reads a scene with pending transforms
    sc.set_transform(2, new[2])
    O = np.zeros((4, 4), np.float32); D = np.zeros((4, 4), np.float32); D[:, 2] = 1; D[:, 3] = 1e30
    for call in (lambda: sc.trace(O, D), lambda: sc.trace(O, D, canonical=True), lambda: sc.instance_info(0), lambda: sc.bvh(-1), lambda: sc.wide_read(-1),
                 lambda: sc.wide_counts(0)):
        with pytest.raises(capi.RtError, match="1 instance transform pending"):
            call()
    p = capi.Pipeline(gpu)
    p.set_scene(sc)
    for _ in range(n):
        p.add_material(T.default_material())
    p.set_environment_constant((0.5, 0.5, 0.5))
    p.create_output(32, 32)
    cam = np.array([0, 2, 16, 0, 0, 0, 0, 1, 0, 0.8, 1.0], np.float32)
    pfc = frames_of(capi, cam, 1, 32, 32)[0]
    p.update(pfc)
    with pytest.raises(capi.RtError, match="pending"):
        p.render()
    with pytest.raises(capi.RtError, match="pending"):
        p.render_batch([pfc])
    sc.update()
    final[2] = new[2]
    p.render()
    work = p.count_work()
    # nothing pending: no array and no generation changes -- count_work still answers without a new render
    before = arrays(sc, n)
    sc.update()
    assert_bytes_equal(arrays(sc, n), before, "an update with nothing pending")
    assert p.count_work() == work
    # ... while a real update is a change of scene: nothing rendered since
    sc.set_transform(0, new[0])
    sc.update()
    with pytest.raises(capi.RtError):
        p.count_work()
    # instances added since the build: update refuses, build takes the stored transforms
    sc.set_transform(3, new[3])
    sc.add_model(gm[n % 2], None)                      # (instance n of gpu_scene: mesh n % 2)
    with pytest.raises(capi.RtError, match="rt_scene_update"):
        sc.update()
    sc.build()
    final[0], final[3] = new[0], new[3]
    fresh.close()
    fresh = gpu_scene(capi, gpu, final + [None])
    assert_bytes_equal(arrays(sc, n + 1), arrays(fresh, n + 1), "build after setters and add_model")
    p.close(); fresh.close(); sc.close()


def test_animated_example_through_the_cpp_mirror(tmp_path):
    """examples/realtime_animated.cpp: RtScene::setTransform + RtScene::update per frame on a 3 x 3 grid, end to end; spun for three frames the
    image is another than spun for one"""
    import os
    import subprocess
    from util import GOLDEN
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dxrexperiments_amd", "lib", "realtime_animated")
    images = []
    for frames in (1, 3):
        out = tmp_path / ("out%d.pfm" % frames)
        r = subprocess.run([exe, os.path.join(GOLDEN, "susanne.obj"), "96", "64", str(frames), str(out), "3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "9 spinning instances: %d frames" % frames in r.stdout and "TLAS update" in r.stdout
        raw = out.read_bytes()
        head = b"PF\n96 64\n-1.0\n"
        assert raw.startswith(head)
        images.append(np.frombuffer(raw[len(head):], "<f4").reshape(64, 96, 3))
    assert images[0].max() > 0.1 and images[0].std() > 0.01            # an image, not a constant
    assert not np.array_equal(images[0], images[1])
