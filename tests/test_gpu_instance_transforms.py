"""The two-level path under the instance transforms the rest of the suite never makes (util.hard_xforms): mirrored, 1000:1 stretched and
squashed, sheared, scaled by 1e-4 / 1e4 / 1e+-12 / 1e+-20, moved 40,000 units away, singular, NaN, inf.  Traversal (production and canonical
kernels, every kind of search) == oracle BVH == oracle brute force, bit for bit and counter for counter; the instance records (fp32 inverse,
world box) == the oracle's; whole frames == osc.render / osc.render_realtime.  What the fp32 definition itself loses against geometry on
these transforms is measured and bounded in tests/test_s2_truth.py and tests/test_gpu_s2_truth.py (tests/golden/s2_instance_bounds.json)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import s2_truth as S
from dxrexperiments_amd import rtypes as T, scenes
from test_gpu_batch import frames_of
from test_gpu_pipeline import make_gpu_pipeline, make_oracle_scene
from test_gpu_realtime_denoise import realtime_pair
from test_gpu_trace import compare_all
from util import ANY, CULL, HARD_FAMILIES, Pair, assert_hits_equal, cam_array, hard_xforms, random_rays, random_xforms, triangle_soup, world_box_of_vertices

pytestmark = pytest.mark.gpu

N_INST = 12
STEEP = 65536.0                      # rt_wide_step.h: a reciprocal direction component beyond it sends the lane down the exact path


def two_models():
    return [scenes.blob_mesh(level=2), triangle_soup(300, seed=2, extent=1.5, size=0.4)]


def family_instances(family, seed=5):
    """12 instances alternating the blob and the soup under the family's transforms + one identity instance (the healthy neighbour)"""
    xf = hard_xforms(family, N_INST, seed)
    return [(k % 2, xf[k]) for k in range(N_INST)] + [(0, None)], xf


def ray_source(family, models, seed=5):
    """the instances the ray sets are laid out over: the family's own where float64 can place them; the extreme and degenerate families'
    rays are laid out over the transforms they were made from (same places, healthy shapes) and the identity instance"""
    if family in ("extreme", "degenerate"):
        xf = random_xforms(N_INST, seed, spread=6.0)
    else:
        xf = hard_xforms(family, N_INST, seed)
    return [(k % 2, xf[k]) for k in range(N_INST)] + [(0, None)]


def finite_boxes(pair, n):
    b = np.stack([pair.o.instance_info(k)[0] for k in range(n)])
    return b[np.isfinite(b).all(axis=1) & (np.abs(b) < 1e30).all(axis=1)]


def plane_rays(boxes, n, seed):
    """origins ON a plane of an instance's world box (that coordinate bit for bit), elsewhere inside the face; half the rays head for a
    point inside the box, half anywhere"""
    r = np.random.default_rng(seed)
    b = boxes[r.integers(0, len(boxes), n)].astype(np.float64)
    lo, hi = b[:, :3], b[:, 3:]
    o = r.uniform(0, 1, (n, 3)) * (hi - lo) + lo
    axis, side = r.integers(0, 3, n), r.integers(0, 2, n)
    rows = np.arange(n)
    o[rows, axis] = np.where(side == 1, hi[rows, axis], lo[rows, axis])
    target = r.uniform(0, 1, (n, 3)) * (hi - lo) + lo
    d = np.where((r.uniform(size=n) < 0.5)[:, None], target - o, r.normal(size=(n, 3)))
    l = np.linalg.norm(d, axis=1, keepdims=True)
    l[l == 0] = 1
    O = np.zeros((n, 4), np.float32); D = np.zeros((n, 4), np.float32)
    O[:, :3] = o                     # (the plane coordinate is an fp32 number: the conversion keeps it)
    D[:, :3] = d / l
    D[:, 3] = 1e38
    return O, D


def small_components(r, n):
    """unit directions with one or two components of 10^U(-9, -3) (either sign) or exactly zero"""
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for _ in range(2):
        axis = r.integers(0, 3, n)
        tiny = 10.0 ** r.uniform(-9, -3, n) * np.where(r.uniform(size=n) < 0.5, 1.0, -1.0)
        tiny = np.where(r.uniform(size=n) < 0.25, 0.0, tiny)
        use = r.uniform(size=n) < (1.0 if _ == 0 else 0.5)
        d[np.nonzero(use)[0], axis[use]] = tiny[use]
    l = np.linalg.norm(d, axis=1, keepdims=True)
    l[l == 0] = 1
    return d / l


def steep_rays(lo, hi, n, seed):
    """rays through the scene's box whose WORLD direction has such components"""
    r = np.random.default_rng(seed)
    O = np.zeros((n, 4), np.float32); D = np.zeros((n, 4), np.float32)
    O[:, :3] = r.uniform(lo, hi, (n, 3))
    D[:, :3] = small_components(r, n)
    D[:, 3] = 1e38
    return O, D


def steep_object_rays(models, instances, n, seed):
    """... and rays whose direction has them in an instance's OBJECT space (the space wide_step's threshold is applied in): through a vertex of
    that instance, mapped to the world by the forward matrix in float64; the fp32 inverse brings them back to within rounding"""
    r = np.random.default_rng(seed)
    O = np.zeros((n, 4), np.float32); D = np.zeros((n, 4), np.float32)
    which = r.integers(0, N_INST, n)
    d = small_components(r, n)
    for k in range(N_INST):
        mi, x = instances[k]
        m = np.asarray(x, np.float64).reshape(3, 4)
        sel = np.nonzero(which == k)[0]
        pos = models[mi][0]["position"].astype(np.float64)
        through = pos[r.integers(0, len(pos), sel.size)] + r.normal(size=(sel.size, 3)) * 0.05
        start = through - d[sel] * r.uniform(0.5, 3.0, (sel.size, 1))
        dw = d[sel] @ m[:, :3].T
        scale = np.linalg.norm(dw, axis=1, keepdims=True)
        O[sel, :3] = start @ m[:, :3].T + m[:, 3]
        D[sel, :3] = dw / scale
    D[:, 3] = 1e38
    return O, D


def family_rays(family, pair, models, seed=7):
    src = ray_source(family, models)
    sets = S.ray_sets(models, src, None, 10000, seed)
    P, _ = S.world_triangles(models, src)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    parts = [sets["aimed"][:2], sets["random"][:2], plane_rays(finite_boxes(pair, N_INST + 1), 4000, seed + 1), steep_rays(lo, hi, 4000, seed + 2)]
    if family not in ("extreme", "degenerate"):
        parts.append(steep_object_rays(models, src, 2000, seed + 3))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def steep_pairs(pair, O, D):
    """(ray, transformed instance) pairs on either side of wide_step's threshold: the object-space direction is inv . d, not normalised"""
    steep = total = 0
    with np.errstate(all="ignore"):
        for k in range(N_INST):
            inv = pair.o.instance_info(k)[1].reshape(3, 4)[:, :3].astype(np.float32)
            d = D[:, :3]
            od = np.stack([(inv[r, 0] * d[:, 0] + inv[r, 1] * d[:, 1]) + inv[r, 2] * d[:, 2] for r in range(3)], axis=1)
            worst = np.abs(np.float32(1.0) / od).max(axis=1)
            steep += int((~(worst <= STEEP)).sum())
            total += len(worst)
    return steep, total


_pairs = {}


def family_pair(oracle, capi, gpu, family):
    """one scene per family, shared by the tests of this file (nothing changes it)"""
    if family not in _pairs:
        models = two_models()
        inst, _ = family_instances(family)
        _pairs[family] = (Pair(oracle, capi, gpu, models, inst), models)
    return _pairs[family]


@pytest.mark.parametrize("family", HARD_FAMILIES)
def test_traversal_under_hard_instance_transforms(gpu, oracle, capi, family):
    """20,000 aimed and random rays, 4,000 from the planes of the instances' world boxes, 4,000 + 2,000 with direction components of 1e-9 ...
    1e-3 and 0 in world and in object space: hits bit-equal (production and canonical walk, closest / culled / any-hit, against the oracle's
    BVH and its brute force) and the canonical walk's node and triangle counts equal.  Under stretch and squash (1000:1) the object-space
    reciprocals lie on both sides of wide_step's 65536; under small next to no ray is steep there, under large two in five are."""
    p, models = family_pair(oracle, capi, gpu, family)
    O, D = family_rays(family, p, models)
    steep, total = steep_pairs(p, O, D)
    print("%s: %d of %d (ray, instance) pairs take wide_step's exact path" % (family, steep, total))
    if family in ("stretch", "squash"):
        assert 0.001 * total < steep < 0.999 * total, (steep, total)
    if family == "small":                        # (object-space directions 1e4 long: no reciprocal comes near the threshold)
        assert steep < 0.01 * total
    if family == "large":                        # (... 1e-4 long: a component below a sixth of the length is beyond it)
        assert steep > 0.25 * total
    hit = p.o.trace(O, D, flags=0, mode=1, nthreads=8)["inst"]
    assert len(np.unique(hit[hit != T.RT_NO_HIT])) == N_INST + 1, "an instance no ray hits"
    compare_all(p, O, D, brute=True)


@pytest.mark.parametrize("family", ("extreme", "degenerate"))
def test_unusable_instance_transforms_are_traced_as_the_oracle_traces_them(gpu, oracle, capi, family):
    """A singular, NaN, inf or out-of-range instance transform is not an error (rt_scene_add_model and rt_scene_build take any twelve floats,
    as the reference's TopLevelASGenerator::AddInstance copies any matrix into the instance descriptor unchecked): the scene builds, the
    instance record holds what the fp32 adjugate / determinant gives -- inf and NaN included -- and the fp32 box of the transformed vertices,
    both as the oracle has them bit for bit, every kernel returns the hits of the oracle's brute force, and the healthy identity instance next
    to them is still hit."""
    p, models = family_pair(oracle, capi, gpu, family)
    for k in range(N_INST + 1):
        gb, gi = p.g.instance_info(k)
        ob, oi = p.o.instance_info(k)
        assert np.array_equal(gi, oi, equal_nan=True), (k, gi, oi)
        assert np.array_equal(gb, ob, equal_nan=True), (k, gb, ob)
    O, D = family_rays(family, p, models)
    for flags in (0, CULL, ANY):
        want = p.o.trace(O, D, flags=flags, mode=0, nthreads=8)
        assert_hits_equal(p.g.trace(O, D, flags=flags), want, "%s fast vs brute force flags=%d" % (family, flags), closest=flags != ANY)
        assert_hits_equal(p.g.trace(O, D, flags=flags, canonical=True), want, "%s canonical vs brute force flags=%d" % (family, flags), closest=flags != ANY)
        if flags == 0:
            assert int((want["inst"] == N_INST).sum()) > 0, "the identity instance is not hit"
            if family == "degenerate":           # (no matrix of this family maps a triangle to anything a ray can hit but the two-equal-rows one: flat, hit edge-on at most)
                assert set(np.unique(want["inst"][want["inst"] != T.RT_NO_HIT])) <= {N_INST, 4, 9}


def bad_rays(O, D):
    """4,096 ordinary rays with the rays a caller should not send spread among them, so that a bad lane shares its wave with good ones:
    every kind once in each of the 64 waves' worth of rays, at a lane that moves from wave to wave"""
    O, D = O[:4096].copy(), D[:4096].copy()
    kinds = 12
    for w in range(64):
        for kind in range(kinds):
            i = 64 * w + (5 * kind + 7 * w) % 64
            if kind == 0:
                D[i, :3] = 0.0                          # zero direction
            elif kind == 1:
                D[i, w % 3] = np.nan                    # NaN direction
            elif kind == 2:
                O[i, w % 3] = np.nan                    # NaN origin
            elif kind == 3:
                D[i, :3] = np.eye(3, dtype=np.float32)[w % 3] * (1 if w % 2 else -1)      # axis aligned: two infinite reciprocals
            elif kind == 4:
                D[i, :3] = [0, -0.0, 1]
            elif kind == 5:
                D[i, (w + 1) % 3] = -0.0
            elif kind == 6:
                D[i, 3] = -1.0                          # inverted window
            elif kind == 7:
                O[i, 3] = D[i, 3] = 2.5 + 0.25 * w      # tmin == tmax
            elif kind == 8:
                O[i, w % 3] = np.inf if w % 2 else -np.inf
            elif kind == 9:
                O[i, :3] = np.inf
            elif kind == 10:
                D[i, w % 3] = np.inf
            else:
                D[i, 3] = np.nan                        # NaN tmax
    return O, D


@pytest.mark.parametrize("scene", ("mirror", "stretch", "soup"))
def test_bad_rays_inside_waves_of_good_ones(gpu, oracle, capi, scene):
    """test_edge_cases' rays (zero / NaN / axis-aligned / -0 directions, NaN and inf origins, inverted and empty windows) against scenes with
    wide nodes, an LDS stack and instance entries -- two hard two-level scenes and a single-level soup of 20,000 triangles"""
    if scene == "soup":
        p = Pair(oracle, capi, gpu, [triangle_soup(20000, seed=7)], [(0, None)])
        O, D = random_rays(4096, 8, [-10, -10, -10], [10, 10, 10])
    else:
        p, models = family_pair(oracle, capi, gpu, scene)
        O, D, _ = S.ray_sets(models, ray_source(scene, models), None, 4096, 8)["aimed"]        # (aimed: the good lanes have work to do)
    O, D = bad_rays(O, D)
    with np.errstate(all="ignore"):
        compare_all(p, O, D, brute=True)
    good = np.isfinite(O).all(axis=1) & np.isfinite(D).all(axis=1)
    assert int((p.o.trace(O[good], D[good], flags=0, mode=1, nthreads=8)["inst"] != T.RT_NO_HIT).sum()) > 500


@pytest.mark.parametrize("family", HARD_FAMILIES + ("extreme", "degenerate"))
def test_instance_world_boxes_under_hard_transforms(gpu, oracle, capi, family):
    """k_instance_boxes under every family, on a mesh of 4,200 vertex references (two work items of 4,096) and one of 4,095 (just under
    one): GPU == oracle == the numpy statement of the definition, and the fp32 inverses equal too"""
    models = [triangle_soup(1400, seed=31, extent=2.0, size=0.3), triangle_soup(1365, seed=32, extent=2.0, size=0.3)]
    xf = hard_xforms(family, N_INST, seed=13)
    p = Pair(oracle, capi, gpu, models, [(k % 2, xf[k]) for k in range(N_INST)])
    for k in range(N_INST):
        gb, gi = p.g.instance_info(k)
        ob, oi = p.o.instance_info(k)
        want = world_box_of_vertices(*models[k % 2], xf[k])
        assert np.array_equal(gi, oi, equal_nan=True), (k, gi, oi)
        assert np.array_equal(gb, ob, equal_nan=True), (k, gb, ob)
        assert np.array_equal(gb, want, equal_nan=True), (k, gb, want)


def test_hard_transforms_with_a_small_lds_stack():
    """the stretch and mirror cases once more with 6 LDS stack rows per lane (option lds_stack_rows=6): most rays continue in the global
    rows, as in test_gpu_trace.py::test_small_lds_stack_spills_to_global_rows"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, RT_DEBUG_OPTIONS="lds_stack_rows=6")
    sel = ["test_gpu_instance_transforms.py::test_traversal_under_hard_instance_transforms[%s]" % f for f in ("stretch", "mirror")]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + [os.path.join(here, s) for s in sel],
                       env=env, cwd=os.path.dirname(here), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]


# ---- whole frames ---------------------------------------------------------------------------------------------------------------------
W, H = 96, 64
FRAME_FAMILIES = ("mirror", "stretch", "shear", "far")
COUNTS = ("rays_primary", "rays_secondary", "rays_shadow", "primary_hits", "secondary_hits")


NEAR = {"stretch": -0.9}             # (needles a thousand units long and one thick: from outside their box they are thinner than a pixel)


def frame_scene(family):
    models = two_models()
    xf = hard_xforms(family, N_INST, seed=5)
    inst = [(k % 2, xf[k]) for k in range(N_INST)]
    mats = []
    r = np.random.default_rng(1)
    for k in range(N_INST):
        m = T.default_material()
        m["albedo"][:3] = r.uniform(0.1, 0.9, 3)
        m["roughness"] = r.uniform(0.2, 0.9)
        m["type"] = k % 3
        mats.append(m)
    # the camera looks at the middle of the scene's world box from outside it, far enough to see most of it: hit and miss pixels both
    P, _ = S.world_triangles(models, inst)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    eye = c + np.array([0.1 * e[0], 0.35 * e[1], e[2] + NEAR.get(family, 1.1) * max(e[0], e[1])])
    cam = cam_array(dict(eye=tuple(eye), at=tuple(c), up=(0, 1, 0), fov=0.8), W / H)
    return models, inst, mats, cam


@pytest.mark.parametrize("family", FRAME_FAMILIES)
def test_progressive_frames_under_hard_instance_transforms(gpu, capi, oracle, family):
    """three accumulated frames at depth limits (3, 3), every material type among the instances: image and ray counts == osc.render; the
    mirror case once more in deferred mode and on queues sized by count"""
    models, inst, mats, cam = frame_scene(family)
    env = scenes.sky_cubemap(8)
    p = make_gpu_pipeline(capi, gpu, models, inst, mats, W, H, env=env)
    p.set_depth_limits(3, 3)
    osc = make_oracle_scene(oracle, models, inst)
    pfcs = frames_of(capi, cam, 3, W, H)
    acc = np.zeros((H, W, 4), np.float32)
    omats = np.stack(mats)
    for f, pfc in enumerate(pfcs):
        p.update(pfc)
        p.render()
        acc, ost = osc.render(omats, pfc, W, H, accum=acc, env_faces=env, max_radiance_depth=3, max_shadow_depth=3, nthreads=8)
        assert np.array_equal(p.read_output(), acc), "frame %d: %d pixels differ" % (f, int((p.read_output() != acc).any(axis=2).sum()))
        gst = p.stats()
        for key in COUNTS:
            assert gst[key] == ost[key], (f, key, gst[key], ost[key])
        assert 0 < ost["primary_hits"] < W * H, ost["primary_hits"]
    if family == "mirror":
        p.clear_output()
        p.set_deferred(2)
        for pfc in pfcs:
            p.update(pfc)
            p.render()
        assert p.deferred() == (2, 1)
        assert np.array_equal(p.read_output(), acc), "deferred mode"
        p.set_deferred(0)
        p.set_queue_budget(1)
        p.clear_output()
        p.render_batch(pfcs)
        assert np.array_equal(p.read_output(), acc), "counted queues"
        assert p.queue_memory()[1], "the set did not size its levels by count"
        p.set_queue_budget(0)
    p.close()


@pytest.mark.parametrize("family", FRAME_FAMILIES)
def test_realtime_frames_under_hard_instance_transforms(gpu, capi, oracle, family):
    """both AOVs of the realtime pipeline == osc.render_realtime, ray counts included"""
    models, inst, mats, cam = frame_scene(family)
    env = scenes.sky_cubemap(8)
    p, osc = realtime_pair(capi, oracle, gpu, models, inst, mats, W, H, env)
    host = capi.ProgressiveHost(10)
    pfc = host.update_realtime(cam, 0.0, 3, W, H)
    p.update(pfc)
    p.render()
    d, ind, ost = osc.render_realtime(np.stack(mats), pfc, W, H, env_faces=env, nthreads=8)
    assert np.array_equal(p.read_output(0), d), "direct-lighting AOV: %d pixels differ" % int((p.read_output(0) != d).any(axis=2).sum())
    assert np.array_equal(p.read_output(1), ind), "indirect-specular AOV: %d pixels differ" % int((p.read_output(1) != ind).any(axis=2).sum())
    gst = p.stats()
    for key in COUNTS:
        assert gst[key] == ost[key], (key, gst[key], ost[key])
    assert 0 < ost["primary_hits"] < W * H, ost["primary_hits"]
    p.close()
