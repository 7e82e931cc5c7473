"""Rigid updates (rt_scene_set_instance_transform(s) + rt_scene_update) under every build and launch option of the registry
(tests/option_cases.py), held to the CPU oracle and to a fresh GPU build bit for bit.

tests/test_gpu_option_matrix.py runs every option on scenes that are built and never updated; tests/test_gpu_scene_update.py updates scenes
on the shared context, with default options.  Here the two cross: rt_update_tlas re-runs the builders' steps (which read wide_sah, sah_node,
sah_prim and build_batch) into the scene's buffers; an update changes the scene's level (single / two), its stack need, and the generation
that the pipelines' caches -- shadow cache, free sphere, primary-mode samples, counted queues -- are keyed by.

  (a) update == build under every row of BUILD_ROWS: arrays, the independent layout reader, closest / culled / any hits
  (b) frames across an update under every entry of LAUNCH_CASES, frame by frame and with the update inside a deferred set
  (c) one instance identity -> rotated -> identity under every entry of LAUNCH_CASES, frame by frame and through render_batch, one pipeline

The oracle is never updated and does not know the options: its side is a fresh oracle.Scene of each instance list, computed once per scene
(the Truth cache of test_gpu_option_matrix.py) and reused for every row.  Each case creates its own context, sets its options, and closes it."""
import types

import numpy as np
import pytest

from dxrexperiments_amd import scenes
from test_gpu_option_matrix import (BUILD_ROWS, CORES, LAUNCH_CASES, RAY_KEYS, Truth, _case_id, check_hits, check_tlas, context, frame_constants,
                                    instances_scene, material)
from test_gpu_pipeline import make_oracle_scene
from test_gpu_scene_update import arrays, assert_bytes_equal, assert_equals_oracle, box_meshes
from util import cam_array, hard_xforms, random_xforms

pytestmark = pytest.mark.gpu


def issue(sc, final, which):
    """the setters for the instances `which`: one instance on its own by the singular call, a run of consecutive ones by the plural call"""
    runs = []
    for k in sorted(which):
        if runs and runs[-1][0] + len(runs[-1][1]) == k:
            runs[-1][1].append(final[k])
        else:
            runs.append((k, [final[k]]))
    for first, xs in runs:
        if len(xs) == 1:
            sc.set_transform(first, xs[0])
        else:
            sc.set_transforms(first, xs)
    return sum(len(xs) == 1 for _, xs in runs), sum(len(xs) > 1 for _, xs in runs)


def scene_of(capi, ctx, gmodels, inst):
    sc = capi.Scene(ctx)
    for mi, x in inst:
        sc.add_model(gmodels[mi], x)
    sc.build()
    return sc


def oracle_frames(osc, truth, pfcs, acc, tot):
    """the accumulation `acc` and the ray totals `tot` continued through `pfcs`: (image, totals), the arguments unchanged"""
    acc, tot = acc.copy(), dict(tot)
    for pfc in pfcs:
        acc, st = osc.render(np.stack(truth.mats), pfc, truth.W, truth.H, accum=acc, env_faces=truth.env, nthreads=CORES)
        for k in RAY_KEYS:
            tot[k] += st[k]
    return acc, tot


def assert_image_and_totals(p, image, totals, what):
    got = p.read_output()
    assert np.array_equal(got, image), "%s: %d of %d pixels differ" % (what, int((got != image).any(axis=2).sum()), image.shape[0] * image.shape[1])
    tot = p.totals()
    for k in RAY_KEYS:
        assert tot[k] == totals[k], (what, k, tot[k], totals[k])


def pipeline_of(capi, ctx, sc, truth):
    p = capi.Pipeline(ctx)
    p.set_scene(sc)
    for m in truth.mats:
        p.add_material(m)
    p.set_environment_cube(truth.env)
    p.create_output(truth.W, truth.H)
    p.build_acceleration_structures()
    return p


# ---- (a) update == build under the builder options -------------------------------------------------------------------------------------

A_N = 300
A_IDENTITY_AT_START = (0, 7, 102, 150, 299)             # 0, 102, 150 are in the pending set: they come FROM the identity; 7 and 299 stay
A_TO_IDENTITY = (4, 101, 164, 298)
A_PENDING = sorted(set(range(0, A_N, 2)) | set(range(100, 165)))      # every second + the 65-wide, not wave-aligned run of k_update_records


def update_lists():
    start = [x for x in random_xforms(A_N, 3, spread=6.0)]
    for k in A_IDENTITY_AT_START:
        start[k] = None
    new = random_xforms(A_N, 77, spread=6.0)
    final = list(start)
    for k in A_PENDING:
        final[k] = None if k in A_TO_IDENTITY else new[k]
    assert all(k in A_PENDING for k in A_TO_IDENTITY) and sum(k in A_PENDING for k in A_IDENTITY_AT_START) == 3
    return start, final


def update_truth(oracle, capi):
    """the oracle's side of (a): its fresh scene of the FINAL list (canonical arrays, instance records) and the hits of 12,000 rays"""
    def make():
        start, final = update_lists()
        inst = [(k % 2, x) for k, x in enumerate(final)]
        cam = dict(eye=(0.0, 3.0, 24.0), at=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=0.8)
        t = Truth(oracle, capi, box_meshes(), inst, 9.0, 12000, cam, 64, 36, 0, (0.0, 1.0, 0.0), [material()], scenes.sky_cubemap(8))
        for flags, hits in t.hits.items():
            assert int((hits["inst"] != 0xffffffff).sum()) > 2000, "too few of the rays hit anything: the hit checks show little"
        return types.SimpleNamespace(truth=t, start=start, final=final, osc=make_oracle_scene(oracle, box_meshes(), inst))
    return Truth.of(("update", "boxes300"), make)


def updated_scene(capi, ctx, gmodels, start, final):
    """(the scene built from `start` and updated to `final`, its arrays before the update)"""
    sc = scene_of(capi, ctx, gmodels, [(k % 2, x) for k, x in enumerate(start)])
    before = arrays(sc, A_N)
    singles, runs = issue(sc, final, A_PENDING)
    assert singles > 0 and runs > 0, "both setters are to be used"
    sc.update()
    return sc, before


_default_wide = {}


def default_options_wide_nodes(capi, start, final):
    """the TLAS's wide nodes after the same update on a context with default options (once)"""
    if "nodes" not in _default_wide:
        ctx = capi.Context(0)
        try:
            gm = [capi.Model(ctx, v, i) for v, i in box_meshes()]
            sc, _ = updated_scene(capi, ctx, gm, start, final)
            _default_wide["nodes"] = sc.wide_read(-1)[0]
            sc.close()
            for m in gm:
                m.close()
        finally:
            ctx.close()
    return _default_wide["nodes"]


@pytest.mark.parametrize("row", range(len(BUILD_ROWS)), ids=lambda r: _case_id(BUILD_ROWS[r]))
def test_update_equals_build_under_builder_options(oracle, capi, row):
    """300 instances of the two box meshes (more TLAS nodes than the 128 of the LDS top; 4,200 and 4,095 vertex references: two work items
    and one), five of them identity instances.  Pending: every second instance and the run 100 .. 164, some to the identity and some from
    it, by set_transform and set_transforms.  After update(): bvh(-1), wide_read(-1), wide_counts(-1) and every instance_info byte-equal to a
    fresh scene built on the same context, equal to the oracle's; untouched records as before; the independent layout reader; closest,
    culled and any hits of 12,000 rays == the oracle's.  Rows with wide_sah=1: the surface-area collapse did shape the updated TLAS."""
    opts = BUILD_ROWS[row]
    u = update_truth(oracle, capi)
    what = "update under %s" % (opts,)
    ctx = context(capi, opts)
    try:
        gm = [capi.Model(ctx, v, i) for v, i in box_meshes()]
        sc, before = updated_scene(capi, ctx, gm, u.start, u.final)
        got = arrays(sc, A_N)
        fresh = scene_of(capi, ctx, gm, u.truth.inst)
        assert_bytes_equal(got, arrays(fresh, A_N), what + " vs a fresh GPU build")
        fresh.close()
        assert_equals_oracle(got, u.osc, A_N, what)
        pending = set(A_PENDING)
        for k in range(A_N):
            if k not in pending:
                assert got["boxes"][k].tobytes() == before["boxes"][k].tobytes() and got["invs"][k].tobytes() == before["invs"][k].tobytes(), (what, k)
        assert not np.array_equal(got["keys"], before["keys"]), "%s: the update changed no key" % what
        check_tlas(sc, A_N, what)
        check_hits(sc, u.truth, what)
        if opts["wide_sah"]:
            d_nodes = default_options_wide_nodes(capi, u.start, u.final)
            assert got["wide"].shape != d_nodes.shape or not np.array_equal(got["wide"], d_nodes), "%s: wide_sah=1 did not change the updated TLAS" % what
        sc.close()
    finally:
        ctx.close()


# ---- (b) frames across an update under the launch options ------------------------------------------------------------------------------

B_W, B_H = 96, 64
B_LAMP = (-4.25, 0.75, 2.75)      # inside the scene's bounds, 1.1 from the nearest instance's world box
B_MOVED = sorted(set(range(0, 40, 3)) | {1})            # about a third of the 40; 0 and 1: a run, for the plural setter
B_OCCLUDER, B_INTO_SPHERE, B_TO_IDENTITY, B_SHEAR = 6, 9, 15, 12


def box_distance(box, point):
    lo, hi, pt = box[:3].astype(np.float64), box[3:].astype(np.float64), np.asarray(point, np.float64)
    d = np.maximum(np.maximum(lo - pt, pt - hi), 0.0)
    return float(np.sqrt((d * d).sum()))


def crossing_truth(oracle, capi):
    """the oracle's side of (b): two frames through the old scene, three through the new one, and the condition that keeps the case from
    passing vacuously: the same three frames through the OLD scene give another image (5 % of the pixels at least) and other totals"""
    def make():
        models, inst, mats, cam = instances_scene()
        lamp = np.array(B_LAMP, np.float64)
        old = make_oracle_scene(oracle, models, inst)
        sphere = min(box_distance(old.instance_info(k)[0], lamp) for k in range(len(inst)))
        assert sphere > 1.0, sphere
        new_xf = random_xforms(len(inst), seed=78, spread=6.0)
        centre = np.mean([np.asarray(x, np.float64).reshape(3, 4)[:, 3] for _, x in inst], axis=0)
        toward = (centre - lamp) / np.linalg.norm(centre - lamp)
        new = list(inst)
        for k in B_MOVED:
            new[k] = (inst[k][0], new_xf[k])
        m = np.array(inst[B_OCCLUDER][1], np.float32).reshape(3, 4).copy()           # a blob between the light and the others
        m[:, 3] = lamp + 2.6 * toward
        new[B_OCCLUDER] = (inst[B_OCCLUDER][0], m.reshape(12))
        m = np.array(inst[B_INTO_SPHERE][1], np.float32).reshape(3, 4).copy()        # a soup shrunk to reach into the empty sphere
        m[:, :3] *= np.float32(0.06 * sphere)
        m[:, 3] = lamp + np.array([0.0, -0.5 * sphere, 0.0])
        new[B_INTO_SPHERE] = (inst[B_INTO_SPHERE][0], m.reshape(12))
        new[B_TO_IDENTITY] = (inst[B_TO_IDENTITY][0], None)
        new[B_SHEAR] = (inst[B_SHEAR][0], hard_xforms("shear", len(inst), seed=4)[B_SHEAR])
        assert {B_OCCLUDER, B_INTO_SPHERE, B_TO_IDENTITY, B_SHEAR} <= set(B_MOVED) and inst[B_OCCLUDER][0] == 0 and inst[B_INTO_SPHERE][0] == 1
        t = types.SimpleNamespace(models=models, old=inst, new=new, mats=mats, env=scenes.sky_cubemap(16), W=B_W, H=B_H, sphere=sphere)
        t.pfcs = frame_constants(capi, cam_array(cam, B_W / B_H), B_W, B_H, 5, B_LAMP)
        fresh = make_oracle_scene(oracle, models, new)
        t.moved_in = box_distance(fresh.instance_info(B_INTO_SPHERE)[0], lamp)
        assert 0.0 < t.moved_in < 0.9 * sphere, (t.moved_in, sphere)
        zero = dict.fromkeys(RAY_KEYS, 0)
        acc2, tot2 = oracle_frames(old, t, t.pfcs[:2], np.zeros((B_H, B_W, 4), np.float32), zero)
        t.image, t.totals = oracle_frames(fresh, t, t.pfcs[2:], acc2, tot2)
        stay, stay_tot = oracle_frames(old, t, t.pfcs[2:], acc2, tot2)
        t.share = float((t.image != stay).any(axis=2).mean())
        print("frames 3 - 5 through the new scene instead of the old: %.1f %% of the pixels differ; rays_shadow %d vs %d, secondary_hits %d vs %d"
              % (100.0 * t.share, t.totals["rays_shadow"], stay_tot["rays_shadow"], t.totals["secondary_hits"], stay_tot["secondary_hits"]))
        assert t.share >= 0.05, "only %.2f %% of the pixels tell the new scene from the old" % (100.0 * t.share)
        assert t.totals["rays_shadow"] != stay_tot["rays_shadow"] and t.totals["secondary_hits"] != stay_tot["secondary_hits"], (t.totals, stay_tot)
        return t
    return Truth.of(("update", "crossing"), make)


@pytest.mark.parametrize("case", range(len(LAUNCH_CASES)), ids=lambda c: _case_id(LAUNCH_CASES[c]))
def test_frames_across_an_update_under_launch_options(oracle, capi, case):
    """40 instances of a blob and a soup, glossy, both lights on, the point light in an empty sphere inside the scene.  Two frames (they warm
    the shadow cache and land the free sphere), new transforms for a third of the instances -- one to between the light and the others, one
    into the free sphere reported before, one to the identity, one to a shear --, update(), three more frames into the same accumulation:
    the oracle's two frames through the old scene continued by three through the new, image and ray totals.  Then the same five frames with
    set_deferred(5), the setters and the update after two frames have been recorded: those two see the old scene, the update flushes them."""
    opts = LAUNCH_CASES[case]
    t = crossing_truth(oracle, capi)
    what = "update, %s" % (opts,)
    ctx = context(capi, opts)
    try:
        gm = [capi.Model(ctx, v, i) for v, i in t.models]
        for deferred in (0, 5):
            sc = scene_of(capi, ctx, gm, t.old)
            p = pipeline_of(capi, ctx, sc, t)
            p.set_deferred(deferred)
            p.reset_totals()
            for pfc in t.pfcs[:2]:
                p.update(pfc); p.render()
            if deferred:
                assert p.deferred() == (5, 2)
            else:
                p.read_output()                          # (waits for the stream: the radius has landed)
                r0 = p.free_sphere()
                if opts.get("free_radius", -1) != 0:
                    assert r0 > 0.9 * t.sphere, "no free sphere before the update (%r): the case shows less than it says" % r0
                assert r0 == 0.0 or t.moved_in < r0, (t.moved_in, r0)
            issue(sc, [x for _, x in t.new], B_MOVED)
            if deferred:
                assert p.deferred() == (5, 0), "the setters did not flush the recorded frames"
            sc.update()
            for pfc in t.pfcs[2:]:
                p.update(pfc); p.render()
            if deferred:
                assert p.deferred() == (5, 3)
            assert_image_and_totals(p, t.image, t.totals, what + (", deferred set" if deferred else ", frame by frame"))
            p.close(); sc.close()
    finally:
        ctx.close()


# ---- (c) one instance between single- and two-level under the launch options -----------------------------------------------------------

C_W, C_H, C_FRAMES = 64, 48, 3


def turned():
    """a rotation about the y axis and a small shift: the one instance is no identity instance, the scene two-level"""
    a = 0.35
    m = np.array([[np.cos(a), 0.0, np.sin(a), 0.3], [0.0, 1.0, 0.0, 0.1], [-np.sin(a), 0.0, np.cos(a), -0.2]])
    return m.astype(np.float32).reshape(12)


C_MESHES = {
    # the blob of test_gpu_scene_update.py::test_one_instance_between_single_and_two_level, seen from outside, and a reduced atrium seen from inside
    "blob": (lambda: scenes.blob_mesh(level=2), dict(eye=(0.5, 1.0, 4.0), at=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=0.8), (1.5, 2.0, 1.5)),
    "atrium": (lambda: scenes.sponza_class(detail=0.3), scenes.sponza_camera(), (2.0, 0.5, 1.0)),
}


def level_truth(oracle, capi, name):
    """the oracle's fresh scene of either state -- the identity instance, the turned one --: image and ray totals after three frames"""
    def make():
        make_mesh, cam, lamp = C_MESHES[name]
        t = types.SimpleNamespace(models=[make_mesh()], mats=[material()], env=scenes.sky_cubemap(16), W=C_W, H=C_H)
        t.pfcs = frame_constants(capi, cam_array(cam, C_W / C_H), C_W, C_H, C_FRAMES, lamp)
        t.states = {}
        for state, x in (("identity", None), ("turned", turned())):
            osc = make_oracle_scene(oracle, t.models, [(0, x)])
            image, totals = oracle_frames(osc, t, t.pfcs, np.zeros((C_H, C_W, 4), np.float32), dict.fromkeys(RAY_KEYS, 0))
            assert totals["primary_hits"] > C_FRAMES * C_W * C_H // 8 and totals["secondary_hits"] > 0 and totals["rays_shadow"] > 0, (name, state, totals)
            t.states[state] = (x, image, totals)
        assert not np.array_equal(t.states["identity"][1], t.states["turned"][1]), "%s: turning the instance changes nothing" % name
        return t
    return Truth.of(("update", "level", name), make)


@pytest.mark.parametrize("case", range(len(LAUNCH_CASES)), ids=lambda c: _case_id(LAUNCH_CASES[c]))
def test_one_instance_between_levels_under_launch_options(oracle, capi, case):
    """One instance, identity -> turned -> identity by two updates: the scene is single-level (rays walk the BLAS directly; the seven-wave set
    kernels), two-level, single-level again.  After each state three frames frame by frame and three through render_batch (where
    seven_waves_always and batch_max choose the kernels), each == the oracle's fresh scene of that state, image and ray totals -- through
    one pipeline object: what it carries over from the other level is the point."""
    opts = LAUNCH_CASES[case]
    ctx = context(capi, opts)
    try:
        for name in C_MESHES:
            t = level_truth(oracle, capi, name)
            sc = scene_of(capi, ctx, [capi.Model(ctx, *t.models[0])], [(0, None)])
            p = pipeline_of(capi, ctx, sc, t)
            for step, state in enumerate(("identity", "turned", "identity")):
                x, image, totals = t.states[state]
                if step:
                    sc.set_transform(0, x)
                    sc.update()
                what = "%s, step %d (%s), %s" % (name, step, state, opts)
                p.clear_output()
                p.reset_totals()
                for pfc in t.pfcs:
                    p.update(pfc); p.render()
                assert_image_and_totals(p, image, totals, what + ", frame by frame")
                p.clear_output()
                p.reset_totals()
                p.render_batch(t.pfcs)
                assert_image_and_totals(p, image, totals, what + ", render_batch")
            p.close(); sc.close()
    finally:
        ctx.close()
