"""Every build and launch option of rt_debug_set_option (csrc/rt_api.hip), and the PLOC -> LBVH fallback, held to the CPU oracle.

DESIGN.md section 2.1 S2.7: hits and images do not depend on the traversal tree or on how a launch is shaped.  The rest of the suite
shows that for the default options; here every option of the registry (tests/option_cases.py) selects its other code path -- other leaf
sizes, another collapse, another builder, the fallback, a short LDS stack, no LDS-resident top, other persistent grids, other shadow-cache
shapes -- and the results must be the oracle's bit for bit: hits as uint32 views (util.assert_hits_equal), images with np.array_equal,
ray totals as equal integers.  The oracle does not know the options; its side of every scene is computed once and reused for every row.

  (a) FALLBACK_ROWS   the fallback (option fail_ploc_rounds=1) on every kind of mesh, one- and two-level
  (b) BUILD_ROWS      a pairwise cover of the builder options, on meshes at the builders' size thresholds
  (c) launch options  every value of the registry on its own, and LAUNCH_COMBOS, on three scenes, frame by frame and deferred

Each case creates its own context, sets its options, and closes it."""
import os

import numpy as np
import pytest

import option_cases
import wide_tree as Wt
from dxrexperiments_amd import rtypes as T, scenes
from util import ANY, CULL, assert_hits_equal, cam_array, random_rays, random_xforms, sliver_soup, triangle_soup

pytestmark = pytest.mark.gpu

CORES = max(1, len(os.sched_getaffinity(0)))
RAY_KEYS = ("rays_primary", "rays_secondary", "rays_shadow", "primary_hits", "secondary_hits")


# ---- meshes and scenes ---------------------------------------------------------------------------------------------

def clones_sheet_point():
    """the mesh of test_gpu_wide_tree.py::test_duplicates_and_flat_boxes: identical boxes and keys, zero-thickness boxes, a point, denormals"""
    v, i = triangle_soup(4096, seed=5)
    tri = v["position"].reshape(-1, 3, 3)
    tri[1:600] = tri[0]
    tri[600:700, :, 1] = 0.25
    tri[700] = tri[700, 0]
    tri[701:710] *= np.float32(1e-30)
    return v, i


MESHES = {
    "soup30000": (lambda: triangle_soup(30000, seed=51), 10.0),
    "grid": (lambda: scenes.displaced_grid(100, seed=7, extent=20.0), 10.0),
    "slivers": (lambda: sliver_soup(400, seed=21), 6.0),
    "clones": (clones_sheet_point, 10.0),
    "blob": (lambda: scenes.blob_mesh(level=2), 1.6),
    "blob4": (lambda: scenes.blob_mesh(level=4), 1.6),
}
_mesh_cache = {}


def mesh(name):
    """(verts, tris, half extent of the box rays are aimed at); "soupN": N random triangles"""
    if name not in _mesh_cache:
        if name in MESHES:
            make, ext = MESHES[name]
            v, i = make()
        else:
            n = int(name[4:])                       # (a handful of triangles: close together, so that rays find them)
            (v, i), ext = (triangle_soup(n, seed=100 + n), 10.0) if n >= 100 else (triangle_soup(n, seed=100 + n, extent=1.5, size=0.8), 2.0)
        _mesh_cache[name] = (v, i, ext)
    return _mesh_cache[name]


def instances_of(name, count, spread):
    """one identity instance (count 0), or `count` transformed ones"""
    if count == 0:
        return [(0, None)]
    return [(0, x) for x in random_xforms(count, seed=8 + count, spread=spread)]


def material(kind=1, roughness=0.4):
    m = T.default_material()
    m["type"] = kind
    m["roughness"] = roughness
    return m


def frame_constants(capi, cam, W, H, frames, lamp, seed=77):
    """`frames` progressive frames' constants: both lights on, the point light at `lamp`"""
    host = capi.ProgressiveHost(seed)
    out = []
    for f in range(frames):
        pfc = host.update(cam, 0.0, f + 1, W, H).copy()
        pfc["pointLight"]["worldPos"][:3] = lamp
        assert np.any(pfc["pointLight"]["color"][:3] > 0) and np.any(pfc["directionalLight"]["color"][:3] > 0)
        out.append(pfc)
    return out


class Truth:
    """The oracle's side of one scene, computed once: hits of all three kinds for a fixed ray set, the accumulated image and the ray totals
    after every frame."""
    cache = {}

    def __init__(self, oracle, capi, models, inst, extent, n_rays, cam, W, H, frames, lamp, mats, env):
        self.models, self.inst, self.mats, self.env, self.W, self.H = models, inst, mats, env, W, H
        osc = oracle.Scene()
        for v, i in models:
            osc.add_model(v, i)
        for mi, x in inst:
            osc.add_instance(mi, x)
        osc.build()
        self.split = [osc.refs(k, models[k][1].shape[0])[0] is not None for k in range(len(models))]
        self.O, self.D = random_rays(n_rays, 31, [-extent] * 3, [extent] * 3)
        self.hits = {flags: osc.trace(self.O, self.D, flags=flags, mode=1, nthreads=CORES) for flags in (0, CULL, ANY)}
        self.pfcs = frame_constants(capi, cam_array(cam, W / H), W, H, frames, lamp)
        self.images, self.totals = [], []
        acc = np.zeros((H, W, 4), np.float32)
        tot = dict.fromkeys(RAY_KEYS, 0)
        for pfc in self.pfcs:
            acc, st = osc.render(np.stack(mats), pfc, W, H, accum=acc, env_faces=env, nthreads=CORES)
            for k in RAY_KEYS:
                tot[k] += st[k]
            self.images.append(acc.copy())
            self.totals.append(dict(tot))

    @classmethod
    def of(cls, key, make):
        if key not in cls.cache:
            cls.cache[key] = make()
        return cls.cache[key]


def context(capi, opts):
    ctx = capi.Context(0)
    option_cases.apply(ctx, opts)
    return ctx


def gpu_scene(capi, ctx, models, inst):
    sc = capi.Scene(ctx)
    gm = [capi.Model(ctx, v, i) for v, i in models]
    for mi, x in inst:
        sc.add_model(gm[mi], x)
    sc.build()
    return sc


def check_hits(sc, truth, what, canonical=0):
    for flags in (0, CULL):
        assert_hits_equal(sc.trace(truth.O, truth.D, flags=flags), truth.hits[flags], "%s flags=%d" % (what, flags))
    assert_hits_equal(sc.trace(truth.O, truth.D, flags=ANY), truth.hits[ANY], "%s any-hit" % what, closest=False)
    if canonical:
        k = canonical
        assert_hits_equal(sc.trace(truth.O[:k], truth.D[:k], canonical=True), {n: a[:k] for n, a in truth.hits[0].items()}, "%s canonical" % what)


def check_frames(capi, ctx, sc, truth, frames, deferred, what):
    """`frames` accumulated progressive frames, one by one (deferred 0) or recorded and rendered as one deferred set, against the oracle's
    image and ray totals"""
    p = capi.Pipeline(ctx)
    p.set_scene(sc)
    for m in truth.mats:
        p.add_material(m)
    p.set_environment_cube(truth.env)
    p.create_output(truth.W, truth.H)
    p.build_acceleration_structures()
    p.set_deferred(deferred)
    p.reset_totals()
    for pfc in truth.pfcs[:frames]:
        p.update(pfc)
        p.render()
    img = p.read_output()
    want = truth.images[frames - 1]
    assert np.array_equal(img, want), "%s: %d of %d pixels differ" % (what, int((img != want).any(axis=2).sum()), truth.W * truth.H)
    tot = p.totals()
    for k in RAY_KEYS:
        assert tot[k] == truth.totals[frames - 1][k], (what, k, tot[k], truth.totals[frames - 1][k])
    p.close()


def check_trees(sc, truth, leaf_max, what):
    """every BLAS of the scene against the independent reader; no leaf above leaf_max records.  Returns {model: (stats, nodes, root)}"""
    out = {}
    for k, (mi, _) in enumerate(truth.inst):
        if mi in out:
            continue
        try:
            st, nodes, root = Wt.check_blas(sc, k, *truth.models[mi])
        except AssertionError as e:
            raise AssertionError("%s, model %d: %s" % (what, mi, e)) from None
        assert st["largest_leaf"] <= leaf_max, "%s, model %d: a leaf of %d records with leaf_max=%d" % (what, mi, st["largest_leaf"], leaf_max)
        out[mi] = (st, nodes, root)
    return out


def check_tlas(sc, n_inst, what):
    nodes, root, recs = sc.wide_read(-1)
    assert recs.shape[0] == 0
    if n_inst == 1:
        assert nodes.shape[0] == 0 and root == ~0, what
        return
    boxes = np.stack([sc.instance_info(k)[0] for k in range(n_inst)])
    try:
        Wt.check(nodes, root, boxes[:, :3], boxes[:, 3:], n_inst, blas=False)
    except AssertionError as e:
        raise AssertionError("%s, TLAS: %s" % (what, e)) from None


# ---- (a) the fallback ----------------------------------------------------------------------------------------------

# (mesh, options next to fail_ploc_rounds=1, instances: 0 = one identity instance).
# SPLIT: whether the ORACLE holds triangles of the mesh as several references (rt_refs.h), asserted per row so that a row is what it claims.
# "grid" and "blob4" (5120 triangles) have none.  Every random soup of 30000 triangles has: about 4200 of its triangles are split (the rule
# is relative to the mesh, and a soup has thin triangles), so "soup30000" is, like "slivers", a mesh that PLOC holds as several records per
# split triangle (default) or once (split_refs=0).  Before the fix of rt_model_build's fallback every row WITHOUT a re-sized record array
# -- the unsplit meshes, and the split ones under split_refs=0 -- returned wrong hits.
SPLIT = {"grid": False, "blob4": False, "soup30000": True, "slivers": True}
FALLBACK_ROWS = [
    ("soup30000", {}, 0),
    ("soup30000", {"split_refs": 0}, 0),
    ("grid", {}, 0),
    ("blob4", {}, 0),
    ("slivers", {"split_refs": 0}, 0),
    ("slivers", {}, 0),
    ("soup30000", {}, 4),
    ("soup30000", {"split_refs": 0}, 3),
    ("grid", {}, 3),
    ("blob4", {}, 5),
    ("slivers", {"split_refs": 0}, 5),
    ("slivers", {}, 4),
    ("soup30000", {"leaf_max": 1}, 0),
    ("soup30000", {"leaf_max": 8, "split_refs": 0}, 0),
    ("soup30000", {"wide_sah": 1, "split_refs": 0}, 0),
    ("grid", {"leaf_max": 1}, 0),
    ("grid", {"leaf_max": 8}, 3),
    ("grid", {"wide_sah": 1}, 0),
    ("blob4", {"leaf_max": 8, "wide_sah": 1}, 0),
    ("slivers", {"split_refs": 0, "leaf_max": 1}, 0),
    ("slivers", {"split_refs": 0, "leaf_max": 8}, 4),
    ("slivers", {"split_refs": 0, "wide_sah": 1}, 0),
    ("slivers", {"leaf_max": 8, "wide_sah": 1}, 0),
]


def fallback_truth(oracle, capi, name, count):
    def make():
        v, i, ext = mesh(name)
        spread = 0.6 * ext
        reach = ext + (spread + 0.5 * ext if count else 0.0)
        cam = dict(eye=(0.1 * reach, 0.3 * reach, 2.4 * reach), at=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=0.8)
        return Truth(oracle, capi, [(v, i)], instances_of(name, count, spread), reach, 20000, cam, 192, 108, 2, (0.2 * ext, 0.3 * ext, 0.1 * ext),
                     [material()], scenes.sky_cubemap(16))
    return Truth.of(("fallback", name, count), make)


@pytest.mark.parametrize("row", range(len(FALLBACK_ROWS)), ids=lambda r: "%s-%s-x%d" % (
    FALLBACK_ROWS[r][0], "-".join("%s=%s" % kv for kv in FALLBACK_ROWS[r][1].items()) or "default", FALLBACK_ROWS[r][2]))
def test_ploc_fallback_on_every_kind_of_mesh(oracle, capi, row):
    """rt_model_build throws the PLOC layout away (as it does when PLOC's rounds or the collapse of its tree give up) and collapses the LBVH
    instead.  PLOC had by then rewritten the triangle records in ITS order; the fallback must gather them again in LBVH order for every
    mesh, not only for one whose split references had re-sized the record array.  Checked: the layout that results is the fast_bvh=lbvh one,
    record and node arrays bit for bit, and not the default one; the tree's invariants; closest / culled / any hits and the canonical walk
    against the oracle; two accumulated progressive frames, image and ray totals.  Every check runs, so a failure lists all that is wrong."""
    name, extra, count = FALLBACK_ROWS[row]
    truth = fallback_truth(oracle, capi, name, count)
    assert truth.split[0] == SPLIT[name], "the mesh is not of the kind the row claims"
    leaf_max = extra.get("leaf_max", 2)
    what = "%s x%d %s + fail_ploc_rounds=1" % (name, count, extra)
    ctx = context(capi, dict(extra, fail_ploc_rounds=1))
    ctx_default = context(capi, extra)
    ctx_lbvh = context(capi, dict(extra, fast_bvh="lbvh"))
    problems = []

    def attempt(fn, *a, **kw):
        try:
            return fn(*a, **kw)
        except AssertionError as e:
            problems.append(str(e).split("\n")[0][:400])

    try:
        sc = gpu_scene(capi, ctx, truth.models, truth.inst)
        nodes, root, recs = sc.wide_read(0)
        dn, droot, drecs = gpu_scene(capi, ctx_default, truth.models, truth.inst).wide_read(0)
        ln, lroot, lrecs = gpu_scene(capi, ctx_lbvh, truth.models, truth.inst).wide_read(0)
        if recs.shape == drecs.shape and np.array_equal(recs.view(np.uint32), drecs.view(np.uint32)):
            problems.append("%s: the records are in the default (PLOC) build's order: the fallback did not take the LBVH layout" % what)
        if not (recs.shape == lrecs.shape and np.array_equal(recs.view(np.uint32), lrecs.view(np.uint32))):
            problems.append("%s: the records are not those of the fast_bvh=lbvh build" % what)
        if not (root == lroot and nodes.shape == ln.shape and np.array_equal(nodes, ln)):
            problems.append("%s: the nodes are not those of the fast_bvh=lbvh build" % what)
        attempt(check_trees, sc, truth, leaf_max, what)
        attempt(check_tlas, sc, len(truth.inst), what)
        for flags in (0, CULL):
            attempt(assert_hits_equal, sc.trace(truth.O, truth.D, flags=flags), truth.hits[flags], "%s flags=%d" % (what, flags))
        attempt(assert_hits_equal, sc.trace(truth.O, truth.D, flags=ANY), truth.hits[ANY], "%s any-hit" % what, closest=False)
        attempt(assert_hits_equal, sc.trace(truth.O[:3000], truth.D[:3000], canonical=True), {n: a[:3000] for n, a in truth.hits[0].items()},
                "%s canonical" % what)
        attempt(check_frames, capi, ctx, sc, truth, 2, 0, what)
    finally:
        for c in (ctx, ctx_default, ctx_lbvh):
            c.close()
    print("fallback row %d %s: %s" % (row, what, "ok" if not problems else "; ".join(problems)))
    assert not problems, "\n".join(problems)


# ---- (b) builder options -------------------------------------------------------------------------------------------

# A pairwise cover of leaf_max x fast_bvh x wide_sah x split_refs x build_batch: every value of every option, and every pair of values of
# two different options, in at least one row (tests/test_option_registry.py checks the cover on the CPU); the last row: the surface-area
# collapse with other costs than the default's.
BUILD_ROWS = [
    {"leaf_max": 1, "fast_bvh": "ploc", "wide_sah": 0, "split_refs": 0, "build_batch": 0},
    {"leaf_max": 1, "fast_bvh": "lbvh", "wide_sah": 1, "split_refs": 1, "build_batch": 1},
    {"leaf_max": 2, "fast_bvh": "ploc", "wide_sah": 0, "split_refs": 1, "build_batch": 1},
    {"leaf_max": 2, "fast_bvh": "lbvh", "wide_sah": 1, "split_refs": 0, "build_batch": 0},
    {"leaf_max": 3, "fast_bvh": "ploc", "wide_sah": 1, "split_refs": 0, "build_batch": 1},
    {"leaf_max": 3, "fast_bvh": "lbvh", "wide_sah": 0, "split_refs": 1, "build_batch": 0},
    {"leaf_max": 4, "fast_bvh": "ploc", "wide_sah": 1, "split_refs": 1, "build_batch": 0},
    {"leaf_max": 4, "fast_bvh": "lbvh", "wide_sah": 0, "split_refs": 0, "build_batch": 1},
    {"leaf_max": 8, "fast_bvh": "ploc", "wide_sah": 1, "split_refs": 1, "build_batch": 1},
    {"leaf_max": 8, "fast_bvh": "lbvh", "wide_sah": 0, "split_refs": 0, "build_batch": 0},
    {"leaf_max": 2, "fast_bvh": "ploc", "wide_sah": 1, "split_refs": 1, "build_batch": 0, "sah_node": 2.5, "sah_prim": 0.25},
]


def build_meshes(leaf_max):
    """soups at the builders' thresholds (one leaf: n <= leaf_max, rt_bvh_wide.hip; no PLOC: n < 2 leaf_max + 2, rt_bvh_ploc.hip) and well
    above them, slivers (split references), clones / sheet / point"""
    sizes = [1, 2, 3, leaf_max, leaf_max + 1, 2 * leaf_max + 1, 2 * leaf_max + 2, 2 * leaf_max + 3, 1000, 30000]
    return ["soup%d" % n for n in sorted(set(sizes))] + ["slivers", "clones"]


def build_truth(oracle, capi, name, count=0):
    def make():
        v, i, ext = mesh(name)
        n = i.shape[0]
        reach = ext + (8.0 + ext if count else 0.0)
        cam = dict(eye=(0.0, 0.3 * reach, 2.4 * reach), at=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=0.8)
        return Truth(oracle, capi, [(v, i)], instances_of(name, count, 8.0), reach, 4000 if n < 100 else 12000, cam, 64, 36, 0, (0.0, 1.0, 0.0),
                     [material()], scenes.sky_cubemap(8))
    return Truth.of(("build", name, count), make)


@pytest.mark.parametrize("row", range(len(BUILD_ROWS)), ids=lambda r: "-".join("%s=%s" % kv for kv in BUILD_ROWS[r].items()))
def test_builder_options_pairwise(gpu, oracle, capi, row):
    """One row of the pairwise cover on every mesh: the tree's invariants, no leaf above leaf_max, all three kinds of hit against the oracle;
    on 30000 triangles the options that should change the tree did; the TLAS of 150 instances under the same options."""
    opts = BUILD_ROWS[row]
    leaf_max = opts["leaf_max"]
    ctx = context(capi, opts)
    try:
        for name in build_meshes(leaf_max):
            truth = build_truth(oracle, capi, name)
            what = "%s %s" % (name, opts)
            sc = gpu_scene(capi, ctx, truth.models, truth.inst)
            trees = check_trees(sc, truth, leaf_max, what)
            check_tlas(sc, 1, what)
            check_hits(sc, truth, what)
            if name == "soup30000" and (opts["wide_sah"] or leaf_max != 2):
                d_nodes = gpu_scene(capi, gpu, truth.models, truth.inst).wide_read(0)[0]
                nodes = trees[0][1]
                assert nodes.shape != d_nodes.shape or not np.array_equal(nodes, d_nodes), "%s: the options did not change the tree" % what
        truth = build_truth(oracle, capi, "blob", 150)
        what = "150 blobs %s" % opts
        sc = gpu_scene(capi, ctx, truth.models, truth.inst)
        check_trees(sc, truth, leaf_max, what)
        check_tlas(sc, 150, what)
        check_hits(sc, truth, what)
    finally:
        ctx.close()


# ---- (c) launch options --------------------------------------------------------------------------------------------

# combinations that cross the families (kernels' stack and top, persistent grids, shadow cache, builders, the fallback)
LAUNCH_COMBOS = [
    {"lds_top": 0, "lds_stack_rows": 6, "persistent_blocks_per_cu": 1},
    {"seven_waves_always": 1, "shadow_cache_res": 16, "leaf_max": 8},
    {"fast_bvh": "lbvh", "shadow_cache_pixels": 1, "primary_persistent": 1},
    {"fail_ploc_rounds": 1, "lds_stack_rows": 6},
]
LAUNCH_CASES = [option_cases.with_needs({n: v}) for n, v in option_cases.exercised("launch")] + LAUNCH_COMBOS
TRACE_CASES = [{"lds_top": 0}, {"lds_stack_rows": 6}, {"persistent_blocks_per_cu": 1}, LAUNCH_COMBOS[0]]
LAUNCH_SCENES = ("atrium", "instances", "cables")
LAUNCH_W, LAUNCH_H, LAUNCH_FRAMES = 192, 108, 5


def instances_scene():
    """the two-level scene of the launch cases (tests/test_gpu_update_options.py animates it): a blob and a soup, 40 instances, a glossy material
    each; (models, instances, materials, camera)"""
    models = [scenes.blob_mesh(level=2), triangle_soup(500, seed=2, extent=2.0, size=0.4)]
    xf = random_xforms(40, seed=3, spread=6.0)
    inst = [(k % 2, xf[k]) for k in range(40)]
    r = np.random.default_rng(5)
    mats = []
    for k in range(40):
        m = material(1, float(r.uniform(0.1, 0.9)))
        m["albedo"][:3] = r.uniform(0.05, 0.95, 3)
        m["reflectivity"] = r.uniform(0.2, 1.0)
        mats.append(m)
    return models, inst, mats, dict(eye=(1.0, 3.0, 20.0), at=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=0.8)


def launch_truth(oracle, capi, name):
    """single-level: a reduced atrium; two-level: blobs and soups, 40 instances, a material each; split references: a hall full of cables.
    Glossy materials, both lights on, the point light INSIDE the geometry's bounds (its shadow rays end at the free sphere, the shadow
    cache is keyed by it)."""
    def make():
        env = scenes.sky_cubemap(16)
        if name == "atrium":
            models, inst, mats = [scenes.sponza_class(detail=0.3)], [(0, None)], [material()]
            cam, lamp, ext = scenes.sponza_camera(), (2.0, 0.5, 1.0), 16.0
        elif name == "instances":
            models, inst, mats, cam = instances_scene()
            lamp, ext = (0.5, 1.0, 0.5), 9.0
        else:
            models, inst, mats = [scenes.stadium_class(5, 0.25, ("hall", "cables", "slats"))], [(0, None)], [material()]
            cam, lamp, ext = scenes.stadium_camera(), (3.0, 4.0, -2.0), 30.0
        t = Truth(oracle, capi, models, inst, ext, 20000, cam, LAUNCH_W, LAUNCH_H, LAUNCH_FRAMES, lamp, mats, env)
        if name == "cables":
            assert t.split[0], "the cable mesh has no split triangle"
        return t
    return Truth.of(("launch", name), make)


def _case_id(opts):
    return "-".join("%s=%s" % kv for kv in opts.items())


@pytest.mark.parametrize("scene", LAUNCH_SCENES)
@pytest.mark.parametrize("case", range(len(LAUNCH_CASES)), ids=lambda c: _case_id(LAUNCH_CASES[c]))
def test_launch_options_render_the_oracles_image(oracle, capi, case, scene):
    """Accumulated glossy frames under one launch option (or a combination), frame by frame and as one deferred set: the oracle's image and
    ray totals.  Three frames; five where the option is about how a set is cut (batch_max)."""
    opts = LAUNCH_CASES[case]
    frames = max([option_cases.OPTIONS[n].get("frames", 3) for n in opts])
    truth = launch_truth(oracle, capi, scene)
    ctx = context(capi, opts)
    try:
        sc = gpu_scene(capi, ctx, truth.models, truth.inst)
        what = "%s %s" % (scene, opts)
        check_frames(capi, ctx, sc, truth, frames, 0, what + ", frame by frame")
        check_frames(capi, ctx, sc, truth, frames, frames, what + ", one deferred set")
    finally:
        ctx.close()


@pytest.mark.parametrize("scene", LAUNCH_SCENES)
@pytest.mark.parametrize("case", range(len(TRACE_CASES)), ids=lambda c: _case_id(TRACE_CASES[c]))
def test_launch_options_trace_the_oracles_hits(oracle, capi, case, scene):
    """Scene.trace (rt_trace_batch) under the options that change the traversal kernels or their grid: closest, culled and any hits"""
    opts = TRACE_CASES[case]
    truth = launch_truth(oracle, capi, scene)
    ctx = context(capi, opts)
    try:
        check_hits(gpu_scene(capi, ctx, truth.models, truth.inst), truth, "%s %s" % (scene, opts), canonical=2000)
    finally:
        ctx.close()
