"""Instance masks (rt_scene_set_instance_mask(s) + rt_scene_update / rt_scene_build): "update == build, with masks" (DESIGN.md section 2).
The instance records are those of a fresh build of the FULL list; the TLAS is the TLAS of a fresh build over the VISIBLE sub-list, except that
it names every instance by its own index vis[j] where that build names the j-th of the sub-list.  So: the masked scene's arrays, taken back
to the sub-list's numbering, are byte-equal to a fresh GPU scene of the sub-list and equal to the oracle's -- which is never masked or
updated, it is built fresh from the sub-list -- and every instance_info, hidden ones included, is byte-equal to a fresh GPU build of the full
list.  Then rays (hits with `inst` mapped, canonical counters), frames through pipelines that remember the old scene, the states in between,
the builder options and the C++ mirror.  All comparisons are bit for bit."""
import os
import subprocess
import types

import numpy as np
import pytest

import s2_truth as S
from dxrexperiments_amd import rtypes as T, scenes
from test_gpu_batch import frames_of
from test_gpu_instance_transforms import COUNTS, frame_scene, two_models
from test_gpu_option_matrix import BUILD_ROWS, _case_id, context
from test_gpu_pipeline import make_gpu_pipeline, make_oracle_scene
from test_gpu_realtime_denoise import realtime_pair
from test_gpu_scene_update import arrays, assert_bytes_equal, assert_equals_oracle, box_meshes, gpu_models, start_xforms
from test_gpu_trace import compare_all
from util import GOLDEN, Pair, random_xforms

pytestmark = pytest.mark.gpu

W, H = 96, 64
_cache = {}


def scene_of(capi, ctx, gmodels, inst, masks=None):
    """instances (model, transform) on the given GPU models, built; masks (if any) set BEFORE the build"""
    sc = capi.Scene(ctx)
    for mi, x in inst:
        sc.add_model(gmodels[mi], x)
    if masks is not None:
        sc.set_masks(0, masks)
    sc.build()
    return sc


def instances(xf):
    """test_gpu_scene_update's rule: instance k = mesh k % 2 under xf[k]"""
    return [(k % 2, x) for k, x in enumerate(xf)]


def masks_of(n, hidden):
    m = np.full(n, 0xFF, np.uint8)
    m[list(hidden)] = 0
    return m


def unmapped(a, vis):
    """the arrays of a masked scene in the numbering of its visible sub-list: instance vis[j] -> j in the canonical leaves' `left`, the low words
    of the sorted keys, the wide nodes' leaf codes and (one visible instance) root_code; the records of the visible instances.  Asserts that
    the scene names visible instances only."""
    vis = np.asarray(vis, np.int64)
    pos = np.full(int(vis.max()) + 1, -1, np.int64)
    pos[vis] = np.arange(len(vis))

    def back(idx):
        idx = np.asarray(idx, np.int64)
        assert (idx <= vis.max()).all() and (pos[idx] >= 0).all(), "the TLAS names a hidden instance"
        return pos[idx]

    nodes = a["nodes"].copy()
    leaf = nodes["right"] == T.RT_LEAF
    assert int(leaf.sum()) == len(vis)
    nodes["left"][leaf] = back(nodes["left"][leaf]).astype(np.uint32)
    keys = (a["keys"] & np.uint64(0xFFFFFFFF00000000)) | back(a["keys"] & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    wide = a["wide"].copy()
    codes = wide[:, 12:16].view(np.int32)
    is_leaf = (codes < 0) & (codes != -2 ** 31)                  # (RT_NODE_NONE: an unused slot)
    codes[is_leaf] = ~back(~codes[is_leaf]).astype(np.int32)
    root = a["root"]
    if len(vis) == 1:
        assert root == ~int(vis[0]), (root, vis)
        root = -1
    return dict(nodes=nodes, keys=keys, parents=a["parents"], depth=a["depth"], wide=wide, root=root, counts=a["counts"],
                boxes=a["boxes"][vis], invs=a["invs"][vis])


def check_masked(capi, ctx, oracle, sc, gmodels, meshes, inst, vis, what, full=None):
    """sc (masked, built or updated) against: a fresh GPU scene and a fresh oracle scene of the visible sub-list (TLAS, under the index
    mapping), a fresh GPU scene of the full list (every record).  -> (arrays of sc, arrays of the fresh full scene)"""
    n = len(inst)
    got = arrays(sc, n)
    assert got["keys"].shape[0] == len(vis) and got["nodes"].shape[0] == 2 * len(vis) - 1, "%s: bvh_info(-1) does not report the visible count" % what
    sub = [inst[k] for k in vis]
    back = unmapped(got, vis)
    fresh = scene_of(capi, ctx, gmodels, sub)
    assert_bytes_equal(back, arrays(fresh, len(vis)), what + " vs a fresh GPU build of the visible sub-list")
    fresh.close()
    assert_equals_oracle(back, make_oracle_scene(oracle, meshes, sub), len(vis), what)
    if full is None:
        f = scene_of(capi, ctx, gmodels, inst)
        full = arrays(f, n)
        f.close()
    for key in ("boxes", "invs"):
        assert got[key].tobytes() == full[key].tobytes(), "%s: instance_info differs from a fresh build of the full list" % what
    return got, full


HIDDEN = {
    "first": lambda n: [0],
    "last": lambda n: [n - 1],
    "every_second": lambda n: list(range(0, n, 2)),
    "all_but_first": lambda n: list(range(1, n)),                # one visible instance: the root is a leaf
    "all_but_last": lambda n: list(range(n - 1)),
    "all_but_middle": lambda n: [k for k in range(n) if k != n // 2],
    "run63": lambda n: list(range(100, 163)),
    "run64": lambda n: list(range(100, 164)),
    "run65": lambda n: list(range(100, 165)),
    "two_of_three": lambda n: [k for k in range(n) if k % 3],    # 300 -> 100 visible: from more than 128 wide nodes to fewer
}


def array_cases():
    out, seen = [], set()
    for n in (2, 5, 13, 300):
        for name in ("first", "last", "every_second", "all_but_first", "all_but_last", "all_but_middle"):
            key = (n, tuple(HIDDEN[name](n)))
            if key not in seen:                        # (n = 2: "first" is "all but last")
                seen.add(key)
                out.append((n, name))
    return out + [(300, name) for name in ("run63", "run64", "run65", "two_of_three")]


def full_arrays(capi, gpu, n):
    """the fresh build of the full list of n, once"""
    if ("full", n) not in _cache:
        sc = scene_of(capi, gpu, gpu_models(capi, gpu), instances(start_xforms(n)))
        _cache[("full", n)] = arrays(sc, n)
        sc.close()
    return _cache[("full", n)]


@pytest.mark.parametrize("n,hidden", array_cases())
def test_update_equals_build_of_the_visible(gpu, capi, oracle, n, hidden):
    xf = start_xforms(n)
    inst = instances(xf)
    gm = gpu_models(capi, gpu)
    sc = scene_of(capi, gpu, gm, inst)
    full = full_arrays(capi, gpu, n)
    assert_bytes_equal(arrays(sc, n), full, "before any mask")
    hide = HIDDEN[hidden](n)
    vis = [k for k in range(n) if k not in set(hide)]
    m = masks_of(n, hide)
    if len(hide) == 1:
        sc.set_mask(hide[0], 0)
    else:
        sc.set_masks(0, m)
    sc.update()
    assert sc.update_ms() > 0.0
    assert np.array_equal(sc.masks(), m)
    got, _ = check_masked(capi, gpu, oracle, sc, gm, box_meshes(), inst, vis, "n=%d hidden %s" % (n, hidden), full)
    if hidden == "two_of_three":
        assert full["counts"][0] > 128 > got["counts"][0] > 0, (full["counts"], got["counts"])
    # show again: every array as before the first call
    sc.set_masks(0, np.full(n, 0xFF, np.uint8))
    sc.update()
    assert_bytes_equal(arrays(sc, n), full, "n=%d hidden %s, shown again" % (n, hidden))
    sc.close()


@pytest.mark.parametrize("n,hidden", [(13, "every_second"), (13, "all_but_middle"), (300, "run65")])
def test_build_honours_masks(gpu, capi, n, hidden):
    """masks set before the first build() == a full build followed by set_masks + update, byte for byte; and build() after masks on a built scene"""
    inst = instances(start_xforms(n))
    gm = gpu_models(capi, gpu)
    m = masks_of(n, HIDDEN[hidden](n))
    a = scene_of(capi, gpu, gm, inst, masks=m)
    b = scene_of(capi, gpu, gm, inst)
    b.set_masks(0, m)
    b.update()
    c = scene_of(capi, gpu, gm, inst)
    c.set_masks(0, m)
    c.build()
    assert_bytes_equal(arrays(a, n), arrays(b, n), "masks + build vs build + masks + update")
    assert_bytes_equal(arrays(c, n), arrays(b, n), "build + masks + build vs build + masks + update")
    assert np.array_equal(a.masks(), m)
    a.close(); b.close(); c.close()


def test_hidden_instances_follow_transforms_and_vertices(gpu, capi, oracle):
    """five instances, the two of mesh 1 hidden: a hidden instance's transform, then new positions of the model only hidden instances use, each
    with an update; then both are shown.  == a fresh build of the final list over fresh models of the final vertices, and the oracle"""
    meshes = [(v.copy(), i.copy()) for v, i in box_meshes()]
    gm = [capi.Model(gpu, v, i) for v, i in meshes]
    n = 5
    xf = start_xforms(n)
    inst = instances(xf)
    sc = scene_of(capi, gpu, gm, inst)
    sc.set_masks(0, masks_of(n, [1, 3]))
    sc.update()
    new = random_xforms(n, 78, spread=6.0)
    sc.set_transform(3, new[3])
    sc.update()
    final = list(inst)
    final[3] = (1, new[3])
    check_masked(capi, gpu, oracle, sc, gm, meshes, final, [0, 2, 4], "a hidden instance's transform")
    moved = meshes[1][0].copy()
    moved["position"] = moved["position"] * np.float32(0.75) + np.array([0.5, -0.25, 0.125], np.float32)
    gm[1].set_positions(moved["position"])
    sc.update()
    final_meshes = [meshes[0], (moved, meshes[1][1])]
    fresh_models = [capi.Model(gpu, v, i) for v, i in final_meshes]
    hidden_state = arrays(sc, n)
    f = scene_of(capi, gpu, fresh_models, final)
    full = arrays(f, n)
    f.close()
    for key in ("boxes", "invs"):
        assert hidden_state[key].tobytes() == full[key].tobytes(), "records of hidden instances after new vertices: %s" % key
    sc.set_masks(1, [0xFF, 0xFF, 0xFF])
    sc.update()
    got = arrays(sc, n)
    assert_bytes_equal(got, full, "shown after a transform and new vertices while hidden")
    assert_equals_oracle(got, make_oracle_scene(oracle, final_meshes, final), n, "shown after a transform and new vertices while hidden")
    sc.close()


# ---- rays ----------------------------------------------------------------------------------------------------------------------------
class MappedOracle:
    """an oracle scene of the visible sub-list whose hits name instance vis[j] for its j"""

    def __init__(self, osc, vis):
        self.osc, self.vis = osc, np.asarray(vis, np.uint32)

    def trace(self, O, D, **kw):
        h = dict(self.osc.trace(O, D, **kw))
        inst = h["inst"].copy()
        hit = inst != T.RT_NO_HIT
        inst[hit] = self.vis[inst[hit]]
        h["inst"] = inst
        return h


@pytest.mark.parametrize("hidden", ["every_second", "all_but_middle"])
def test_rays_pass_through_hidden_instances(gpu, capi, oracle, hidden):
    """13 instances (12 + one identity): production and canonical walk, closest / cull / any-hit == the oracle's BVH and brute force on the
    sub-list with `inst` mapped, canonical counters included; rays aimed at the triangles of ALL instances (those of the hidden ones pass
    through) and random ones"""
    models = two_models()
    xf = random_xforms(12, 21, spread=6.0)
    inst = [(k % 2, xf[k]) for k in range(12)] + [(0, None)]
    n = len(inst)
    hide = HIDDEN[hidden](n)
    vis = [k for k in range(n) if k not in set(hide)]
    p = Pair(oracle, capi, gpu, models, inst)
    sets = S.ray_sets(models, inst, None, 6000, 7)
    O = np.concatenate([sets["aimed"][0], sets["random"][0]])
    D = np.concatenate([sets["aimed"][1], sets["random"][1]])
    full_hits = p.o.trace(O, D, flags=0, mode=1, nthreads=8)["inst"]
    p.g.set_masks(0, masks_of(n, hide))
    p.g.update()
    osub = MappedOracle(make_oracle_scene(oracle, models, [inst[k] for k in vis]), vis)
    sub_hits = osub.trace(O, D, flags=0, mode=1, nthreads=8)["inst"]
    assert int(np.isin(full_hits, hide).sum()) > 1000, "few rays met a hidden instance: the test shows nothing"
    assert set(np.unique(sub_hits[sub_hits != T.RT_NO_HIT])) == set(vis), "a visible instance no ray hits"
    compare_all(types.SimpleNamespace(g=p.g, o=osub), O, D, brute=True)


# ---- pipelines -----------------------------------------------------------------------------------------------------------------------
def oracle_frames(osc, mats, pfcs, env, acc=None):
    acc = np.zeros((H, W, 4), np.float32) if acc is None else acc
    st = None
    for pfc in pfcs:
        acc, st = osc.render(np.stack(mats), pfc, W, H, accum=acc, env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
    return acc, st


def masked_frame_truth(oracle, capi):
    """frame_scene("mirror"), the odd instances hidden: the oracle's three frames of the full list and of the sub-list, and the condition that
    keeps the case from passing vacuously"""
    if "frames" not in _cache:
        models, inst, mats, cam = frame_scene("mirror")
        env = scenes.sky_cubemap(8)
        pfcs = frames_of(capi, cam, 6, W, H)
        vis = list(range(0, len(inst), 2))
        ofull = make_oracle_scene(oracle, models, inst)
        osub = make_oracle_scene(oracle, models, [inst[k] for k in vis])
        sub_mats = [mats[k] for k in vis]
        t = types.SimpleNamespace(models=models, inst=inst, mats=mats, cam=cam, env=env, pfcs=pfcs, vis=vis, ofull=ofull, osub=osub, sub_mats=sub_mats)
        t.full_acc, t.full_st = oracle_frames(ofull, mats, pfcs[:3], env)
        t.sub_acc, t.sub_st = oracle_frames(osub, sub_mats, pfcs[3:], env)
        same_frames_full, _ = oracle_frames(ofull, mats, pfcs[3:], env)
        differ = float((same_frames_full != t.sub_acc).any(axis=2).mean())
        assert differ >= 0.10, "hiding the odd instances changes %.1f %% of the pixels: the case shows nothing" % (100 * differ)
        assert 0 < t.full_st["primary_hits"] < W * H and 0 < t.sub_st["primary_hits"] < W * H
        _cache["frames"] = t
    return _cache["frames"]


def assert_frame(p, acc, st, what):
    got = p.read_output()
    assert np.array_equal(got, acc), "%s: %d pixels differ" % (what, int((got != acc).any(axis=2).sum()))
    gst = p.stats()
    for key in COUNTS:
        assert gst[key] == st[key], (what, key, gst[key], st[key])


def test_progressive_frames_across_a_mask_update(gpu, capi, oracle):
    """shadow cache on (per-pixel entries too), depth limits (3, 3): three accumulated frames of the full scene, the odd instances hidden,
    update, clear_output, three more == osc.render on the sub-list with the sub-list's materials, ray counts included.  An update that kept
    the generation would leave shadow-cache entries that name hidden instances, the old free sphere and the old primary-mode samples."""
    t = masked_frame_truth(oracle, capi)
    gpu.set_option("shadow_cache_pixels", 1)
    try:
        p = make_gpu_pipeline(capi, gpu, t.models, t.inst, t.mats, W, H, env=t.env)
        p.set_depth_limits(3, 3)
        p.set_shadow_cache(16)
        for pfc in t.pfcs[:3]:
            p.update(pfc); p.render()
        assert_frame(p, t.full_acc, t.full_st, "the full scene")
        assert p.shadow_cache() == 16
        sc = p._keep[0]
        sc.set_masks(0, masks_of(len(t.inst), range(1, len(t.inst), 2)))
        sc.update()
        p.clear_output()
        for pfc in t.pfcs[3:]:
            p.update(pfc); p.render()
        assert_frame(p, t.sub_acc, t.sub_st, "after the odd instances were hidden")
        p.close()
    finally:
        gpu.set_option("shadow_cache_pixels", -1)


def test_deferred_frames_across_a_mask_update(gpu, capi, oracle):
    """set_deferred(4): three frames recorded, the mask call flushes them (they see the full scene), update, three more on the same
    accumulation: == the oracle's frames 1 - 3 on the full list accumulated with 4 - 6 on the sub-list"""
    t = masked_frame_truth(oracle, capi)
    p = make_gpu_pipeline(capi, gpu, t.models, t.inst, t.mats, W, H, env=t.env)
    p.set_depth_limits(3, 3)
    p.set_deferred(4)
    for pfc in t.pfcs[:3]:
        p.update(pfc); p.render()
    assert p.deferred() == (4, 3)
    sc = p._keep[0]
    sc.set_masks(0, masks_of(len(t.inst), range(1, len(t.inst), 2)))
    assert p.deferred() == (4, 0), "the setter did not flush the recorded frames"
    sc.update()
    for pfc in t.pfcs[3:]:
        p.update(pfc); p.render()
    assert p.deferred() == (4, 3)
    acc, _ = oracle_frames(t.osub, t.sub_mats, t.pfcs[3:], t.env, t.full_acc.copy())
    got = p.read_output()
    assert np.array_equal(got, acc), "%d pixels differ" % int((got != acc).any(axis=2).sum())
    p.close()


def test_realtime_frame_after_a_mask_update(gpu, capi, oracle):
    """both AOVs == osc.render_realtime on the sub-list, ray counts included"""
    t = masked_frame_truth(oracle, capi)
    p, _ = realtime_pair(capi, oracle, gpu, t.models, t.inst, t.mats, W, H, t.env)
    host = capi.ProgressiveHost(10)
    pfc = host.update_realtime(t.cam, 0.0, 3, W, H)
    p.update(pfc); p.render()
    sc = p._keep[0]
    sc.set_masks(0, masks_of(len(t.inst), range(1, len(t.inst), 2)))
    sc.update()
    pfc = host.update_realtime(t.cam, 0.0, 4, W, H)
    p.update(pfc); p.render()
    d, ind, ost = t.osub.render_realtime(np.stack(t.sub_mats), pfc, W, H, env_faces=t.env, nthreads=8)
    assert np.array_equal(p.read_output(0), d), "direct-lighting AOV: %d pixels differ" % int((p.read_output(0) != d).any(axis=2).sum())
    assert np.array_equal(p.read_output(1), ind), "indirect-specular AOV: %d pixels differ" % int((p.read_output(1) != ind).any(axis=2).sum())
    gst = p.stats()
    for key in COUNTS:
        assert gst[key] == ost[key], (key, gst[key], ost[key])
    assert 0 < ost["primary_hits"] < W * H
    p.close()


# ---- states --------------------------------------------------------------------------------------------------------------------------
def test_states_and_their_messages(gpu, capi):
    n = 5
    xf = start_xforms(n)
    inst = instances(xf)
    gm = gpu_models(capi, gpu)
    sc = capi.Scene(gpu)
    for mi, x in inst:
        sc.add_model(gm[mi], x)
    assert np.array_equal(sc.masks(), np.full(n, 0xFF, np.uint8))
    # out of range is RT_ERR_STATE, an empty call is fine and changes nothing
    for call in (lambda: sc.set_mask(n, 0), lambda: sc.set_masks(n - 1, [0, 0]), lambda: sc.set_masks(n + 1, [])):
        with pytest.raises(capi.RtError, match="out of range") as e:
            call()
        assert e.value.code == -4
    sc.set_masks(n, [])
    sc.set_masks(0, [])
    # never built: a setter only stores, the build reads
    sc.set_mask(1, 0)
    sc.build()
    ref = scene_of(capi, gpu, gm, inst, masks=masks_of(n, [1]))
    assert_bytes_equal(arrays(sc, n), arrays(ref, n), "a mask before the first build")
    # the value a mask has, or one non-zero value for another: the scene stays built, nothing changes but the byte
    before = arrays(sc, n)
    O = np.zeros((4, 4), np.float32); D = np.zeros((4, 4), np.float32); D[:, 2] = 1; D[:, 3] = 1e30
    sc.set_mask(1, 0)
    sc.set_mask(0, 0x01)
    sc.set_masks(2, [0xFF, 0x80])
    sc.trace(O, D)
    assert_bytes_equal(arrays(sc, n), before, "masks that change no visibility")
    assert sc.masks().tolist() == [0x01, 0, 0xFF, 0x80, 0xFF]
    # a change of visibility: stale, and the message names the masks
    sc.set_mask(2, 0)
    for call in (lambda: sc.trace(O, D), lambda: sc.trace(O, D, canonical=True), lambda: sc.instance_info(0), lambda: sc.bvh(-1), lambda: sc.wide_read(-1),
                 lambda: sc.wide_counts(0)):
        with pytest.raises(capi.RtError, match="instance masks pending") as e:
            call()
        assert e.value.code == -4
    p = capi.Pipeline(gpu)
    p.set_scene(sc)
    for _ in range(n):
        p.add_material(T.default_material())
    p.set_environment_constant((0.5, 0.5, 0.5))
    p.create_output(32, 32)
    cam = np.array([0, 2, 16, 0, 0, 0, 0, 1, 0, 0.8, 1.0], np.float32)
    pfc = frames_of(capi, cam, 1, 32, 32)[0]
    p.update(pfc)
    with pytest.raises(capi.RtError, match="masks pending"):
        p.render()
    with pytest.raises(capi.RtError, match="masks pending"):
        p.render_batch([pfc])
    sc.update()
    p.render()
    work = p.count_work()
    # a mask that changes no visibility: no generation change either -- count_work still answers without a new render
    sc.set_mask(0, 0x7F)
    sc.update()
    assert p.count_work() == work
    # ... while a change of visibility is a change of scene: stale first, nothing rendered since afterwards
    sc.set_mask(2, 0xFF)
    with pytest.raises(capi.RtError, match="masks pending"):
        p.count_work()
    sc.update()
    with pytest.raises(capi.RtError):
        p.count_work()
    # masks together with a pending transform: the message names both
    new = random_xforms(n, 78, spread=6.0)
    sc.set_transform(4, new[4])
    sc.set_mask(4, 0)
    with pytest.raises(capi.RtError, match="1 instance transform and instance masks pending"):
        sc.bvh(-1)
    # no visible instance: update refuses, the scene stays stale, everything pending is kept
    sc.set_masks(0, np.zeros(n, np.uint8))
    for _ in range(2):
        with pytest.raises(capi.RtError, match="no instance is visible") as e:
            sc.update()
        assert e.value.code == -4
    with pytest.raises(capi.RtError, match="pending"):
        sc.trace(O, D)
    with pytest.raises(capi.RtError, match="no instance is visible"):
        sc.build()
    sc.set_mask(3, 0xFF)
    sc.update()
    final = list(inst)
    final[4] = (0, new[4])
    ref.close()
    ref = scene_of(capi, gpu, gm, final, masks=masks_of(n, [0, 1, 2, 4]))
    assert_bytes_equal(arrays(sc, n), arrays(ref, n), "one instance shown after none was visible")
    assert arrays(sc, n)["root"] == ~3
    # instances added since the build: masks are stored, update refuses as it always did, build reads them
    sc.add_model(gm[n % 2], None)
    assert sc.masks().tolist() == [0, 0, 0, 0xFF, 0, 0xFF]
    sc.set_mask(0, 0xFF)
    with pytest.raises(capi.RtError, match="rt_scene_update"):
        sc.update()
    sc.build()
    ref.close()
    ref = scene_of(capi, gpu, gm, final + [(n % 2, None)], masks=masks_of(n + 1, [1, 2, 4]))
    assert_bytes_equal(arrays(sc, n + 1), arrays(ref, n + 1), "build after masks and add_model")
    p.close(); ref.close(); sc.close()


# ---- builder options -----------------------------------------------------------------------------------------------------------------
O_N = 300
O_HIDE = list(range(0, O_N, 3))
O_MOVED = (100, 99)                 # 100 is visible, 99 hidden


def option_truth(oracle):
    if "options" not in _cache:
        xf = start_xforms(O_N)
        new = random_xforms(O_N, 91, spread=6.0)
        final = instances(xf)
        for k in O_MOVED:
            final[k] = (k % 2, new[k])
        vis = [k for k in range(O_N) if k % 3]
        _cache["options"] = types.SimpleNamespace(start=instances(xf), final=final, vis=vis, osc=make_oracle_scene(oracle, box_meshes(), [final[k] for k in vis]))
    return _cache["options"]


@pytest.mark.parametrize("row", range(len(BUILD_ROWS)), ids=lambda r: _case_id(BUILD_ROWS[r]))
def test_masked_update_under_builder_options(oracle, capi, row):
    """300 instances, every third hidden, one pending transform among the visible and one among the hidden, ONE update: against a fresh build of
    the sub-list on the same context and the oracle's; every record against a fresh build of the full list"""
    opts = BUILD_ROWS[row]
    u = option_truth(oracle)
    what = "masked update under %s" % (opts,)
    ctx = context(capi, opts)
    try:
        gm = [capi.Model(ctx, v, i) for v, i in box_meshes()]
        sc = scene_of(capi, ctx, gm, u.start)
        generation_probe = arrays(sc, O_N)
        sc.set_masks(0, masks_of(O_N, O_HIDE))
        for k in O_MOVED:
            sc.set_transform(k, u.final[k][1])
        sc.update()
        got = arrays(sc, O_N)
        back = unmapped(got, u.vis)
        fresh = scene_of(capi, ctx, gm, [u.final[k] for k in u.vis])
        assert_bytes_equal(back, arrays(fresh, len(u.vis)), what + " vs a fresh GPU build of the visible sub-list")
        fresh.close()
        assert_equals_oracle(back, u.osc, len(u.vis), what)
        full = scene_of(capi, ctx, gm, u.final)
        fa = arrays(full, O_N)
        full.close()
        for key in ("boxes", "invs"):
            assert got[key].tobytes() == fa[key].tobytes(), "%s: %s" % (what, key)
        for k in range(O_N):
            if k not in O_MOVED:
                assert got["boxes"][k].tobytes() == generation_probe["boxes"][k].tobytes(), (what, k)
        sc.close()
    finally:
        ctx.close()


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------
def test_visibility_example_through_the_cpp_mirror(gpu, capi, tmp_path):
    """examples/realtime_visibility.cpp: RtScene::setInstanceMask + RtScene::update per frame on a pool of 3 x 3, end to end; its last frame ==
    the frame the C ABI gives for a scene BUILT with the last frame's masks (realtime pipeline + denoiser, the same constants)"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dxrexperiments_amd", "lib", "realtime_visibility")
    obj = os.path.join(GOLDEN, "susanne.obj")
    side, frames = 3, 4
    out = tmp_path / "out.pfm"
    r = subprocess.run([exe, obj, str(W), str(H), str(frames), str(out), str(side)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    alive = [(k + frames) % 3 != 0 for k in range(side * side)]
    assert "a pool of 9 instances, %d alive in the last frame: %d frames" % (sum(alive), frames) in r.stdout and "TLAS update" in r.stdout
    raw = out.read_bytes()
    head = b"PF\n%d %d\n-1.0\n" % (W, H)
    assert raw.startswith(head)
    image = np.frombuffer(raw[len(head):], "<f4").reshape(H, W, 3)[::-1]       # (a PFM's rows run bottom to top)
    assert image.max() > 0.1 and image.std() > 0.01            # an image, not a constant
    # the same frame through the C ABI
    model = capi.Model(gpu, path=obj)
    sc = capi.Scene(gpu)
    p = capi.Pipeline(gpu, capi.PIPELINE_REALTIME)
    f = np.float32
    for k in range(side * side):
        x = np.array([1, 0, 0, (f(k % side) - f(0.5) * f(side - 1)) * f(3.0), 0, 1, 0, 0, 0, 0, 1, (f(k // side) - f(0.5) * f(side - 1)) * f(3.0)], np.float32)
        sc.add_model(model, x)
        m = np.zeros((), T.MATERIAL_PARAMS)
        m["albedo"] = (f(0.25) + f(0.7) * f(k % 3 == 0), f(0.25) + f(0.7) * f(k % 3 == 1), f(0.25) + f(0.7) * f(k % 3 == 2), 1.0)      # (the example's fp32 sums)
        m["specular"] = (0.58, 0.58, 0.58, 1.0)
        m["roughness"], m["reflectivity"], m["type"] = 0.5, 0.7, k % 3
        p.add_material(m)
    sc.set_masks(0, [0xFF if a else 0 for a in alive])
    p.set_scene(sc)
    p.create_output(W, H)
    p.build_acceleration_structures()
    host = capi.ProgressiveHost(1234)
    cam = capi.camera_array((0.0, f(1.2) * f(side), f(2.4) * f(side)), (0, 0, 0), (0, 1, 0), np.float32(3.14159265358979 / 4.0), np.float32(W) / np.float32(H))
    for frame in range(1, frames + 1):
        host.set_flags(True, True)
        pfc = host.update_realtime(cam, 0.0, frame, W, H)
    p.update(pfc); p.render()
    dn = capi.Denoiser(gpu)
    dn.create_output(W, H)
    dn.dispatch(p.output_device_ptr(0), p.output_device_ptr(1))
    want = dn.read_output()
    assert np.array_equal(image, want[..., :3]), "%d pixels differ" % int((image != want[..., :3]).any(axis=2).sum())
    # ... and it is not the frame of the whole pool
    sc.set_masks(0, np.full(side * side, 0xFF, np.uint8))
    sc.update()
    p.render()
    dn.dispatch(p.output_device_ptr(0), p.output_device_ptr(1))
    assert not np.array_equal(dn.read_output(), want)
    p.close(); sc.close()
