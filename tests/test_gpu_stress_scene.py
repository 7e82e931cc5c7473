"""A scene with real-asset triangle statistics (round 5, VERDICT r4 task 6): scenes.stadium_class -- a hall of 16 huge triangles with dense
meshes standing on them, ~1000:1 cable slivers, 20:1 ... 60:1 slats and a debris field whose triangle areas are log-normal over four decades.
Every timed scene of rounds 1 - 4 was a uniformly tessellated procedural mesh; the reference's own default scene is a real asset
(/root/reference/src/DXRExperimentsApp.cpp:91).  The builders, the production walk and the whole progressive frame against the oracle."""
import os

import numpy as np
import pytest

from dxrexperiments_amd import rtypes as T, scenes
from util import ANY, CULL, Pair, assert_hits_equal, cam_array, nodes_equal, random_rays

pytestmark = pytest.mark.gpu


def test_stadium_statistics_are_those_of_an_asset():
    v, t = scenes.stadium_class(5, 1.0)
    assert 250_000 < t.shape[0] < 300_000
    area, aspect = scenes.triangle_statistics(v, t)
    area = area[area > 0]
    assert np.log10(np.percentile(area, 99.9) / np.percentile(area, 1.0)) > 4.0            # areas over more than four decades
    assert area.max() / np.median(area) > 1e6                                               # a few huge triangles under dense detail
    assert (aspect > 20.0).mean() > 0.05 and (aspect > 200.0).mean() > 0.02                 # slats and cables
    sv, st = scenes.sponza_class()
    sa, sasp = scenes.triangle_statistics(sv, st)
    # ... which the headline scene has not: 98 % of its triangles within 1.5 decades of area, no slivers
    assert np.log10(np.percentile(sa, 99.0) / np.percentile(sa, 1.0)) < 2.0 and (sasp > 20.0).mean() < 0.001


def test_stadium_bvh_walk_and_whole_frame_against_the_oracle(gpu, oracle, capi):
    import wide_tree as Wt
    v, t = scenes.stadium_class(5, 1.0)
    p = Pair(oracle, capi, gpu, [(v, t)], [(0, None)])
    # canonical LBVH index-exact; the production tree keeps its invariants on slivers and huge triangles
    gn, gk, gp, gd = p.g.bvh(0)
    on, ok, op, od = p.o.bvh(0)
    assert np.array_equal(gk, ok) and nodes_equal(gn, on) and np.array_equal(gp, op) and gd == od
    # split references (round 5, rt_refs.h): the builder's boxes are the oracle's, bit for bit; the production tree holds one record per
    # reference, every triangle at least once, a split one once per box, and every decoded child box contains the boxes of its subtree
    ooff, oboxes = p.o.refs(0, t.shape[0])
    goff, gboxes, grec = p.g.refs(0)
    assert ooff is not None and np.array_equal(goff, ooff) and np.array_equal(gboxes.view(np.uint32), oboxes.view(np.uint32))
    cnt = np.diff(ooff)
    assert cnt.max() <= 128 and 10000 < int((cnt > 1).sum()) < 40000 and oboxes.shape[0] > t.shape[0]
    nodes, root, recs = p.g.wide_read(0)
    assert recs.shape[0] == oboxes.shape[0]
    lo, hi, prim = Wt.record_bounds(recs)
    assert np.array_equal(np.bincount(prim, minlength=t.shape[0]), cnt)                    # a record per reference
    tri = v["position"][t[prim]]
    assert np.array_equal(recs[:, :9].reshape(-1, 3, 3), tri)
    mark = recs.view(np.uint32)[:, 10]
    assert np.array_equal(mark == 1, cnt[prim] > 1) and set(np.unique(mark)) <= {0, 1}
    # the box a record is held by: its reference box if it is one of several, else the triangle's own
    lo = np.where((mark == 1)[:, None], grec[:, :3], lo)
    hi = np.where((mark == 1)[:, None], grec[:, 3:], hi)
    for pr in np.nonzero(cnt > 1)[0][:200]:                      # every box of a split triangle sits on exactly one of its records
        mine = np.sort(grec[prim == pr].view(np.uint32).view([("", np.uint32)] * 6), axis=0)
        want = np.sort(oboxes[ooff[pr]:ooff[pr + 1]].view(np.uint32).view([("", np.uint32)] * 6), axis=0)
        assert np.array_equal(mine, want)
    st = Wt.check(nodes, root, lo, hi, recs.shape[0], blas=True)
    assert st["nodes"] >= 1
    # hits, all three kinds of search, bit for bit
    O, D = random_rays(150000, 31, [-30, -4, -20], [30, 14, 20])
    cores = max(1, len(os.sched_getaffinity(0)))
    for flags in (0, CULL):
        assert_hits_equal(p.g.trace(O, D, flags=flags), p.o.trace(O, D, flags=flags, mode=1, nthreads=cores), "stadium flags=%d" % flags)
    assert_hits_equal(p.g.trace(O, D, flags=ANY), p.o.trace(O, D, flags=ANY, mode=1, nthreads=cores), "stadium any-hit", closest=False)
    # the whole progressive frame, three accumulated frames in one deferred set, a glossy material so that the secondary rays go everywhere
    W, H = 960, 540
    pipe = capi.Pipeline(gpu)
    pipe.set_scene(p.g)
    mat = T.default_material()
    mat["type"] = 1
    mat["roughness"] = 0.4
    pipe.add_material(mat)
    env = scenes.sky_cubemap(32)
    pipe.set_environment_cube(env)
    pipe.create_output(W, H)
    pipe.build_acceleration_structures()
    host = capi.ProgressiveHost(77)
    cam = cam_array(scenes.stadium_camera(), W / H)
    pipe.set_deferred(3)
    pipe.reset_totals()
    acc = np.zeros((H, W, 4), np.float32)
    rays = {"rays_primary": 0, "rays_secondary": 0, "rays_shadow": 0, "primary_hits": 0, "secondary_hits": 0}
    for f in range(3):
        pfc = host.update(cam, 0.0, f + 1, W, H)
        pipe.update(pfc)
        pipe.render()
        acc, ost = p.o.render(mat, pfc, W, H, accum=acc, env_faces=env, nthreads=cores)
        for k in rays:
            rays[k] += ost[k]
    img = pipe.read_output()
    assert np.array_equal(img, acc), "%d of %d pixels differ" % (int((img != acc).any(axis=2).sum()), W * H)
    tot = pipe.totals()
    for k in rays:
        assert tot[k] == rays[k], (k, tot[k], rays[k])
    assert tot["primary_hits"] == 3 * W * H - (tot["rays_primary"] - tot["primary_hits"]) and tot["primary_hits"] > 0.9 * 3 * W * H


def test_references_do_not_change_a_bit_whatever_layout_holds_them(gpu, oracle, capi):
    """The candidate rule follows the split references (rt_refs.h) whether the production layout holds a long thin triangle as several
    records (default), once in a PLOC tree (option split_refs=0) or once in the LBVH layout (fast_bvh=lbvh): hits and image must be the
    oracle's -- and one another's -- bit for bit on a hall full of cables.  Two-level too: three instances of the cable mesh."""
    from util import random_xforms
    v, t = scenes.stadium_class(5, 0.25, ("hall", "cables", "slats"))
    cores = max(1, len(os.sched_getaffinity(0)))
    O, D = random_rays(60000, 41, [-30, -4, -20], [30, 14, 20])
    W, H = 320, 180
    mat = T.default_material()
    cam = cam_array(scenes.stadium_camera(), W / H)
    host = capi.ProgressiveHost(3)
    pfcs = [host.update(cam, 0.0, f + 1, W, H) for f in range(2)]
    for inst in ([(0, None)], [(0, x) for x in random_xforms(3, seed=8, spread=4.0)]):
        osc = oracle.Scene()
        osc.add_model(v, t)
        for mi, x in inst:
            osc.add_instance(mi, x)
        osc.build()
        assert osc.refs(0, t.shape[0])[0] is not None
        want = osc.trace(O, D, flags=0, mode=1, nthreads=cores)
        want_any = osc.trace(O, D, flags=ANY, mode=1, nthreads=cores)
        acc = np.zeros((H, W, 4), np.float32)
        for pfc in pfcs:
            acc, _ = osc.render(mat, pfc, W, H, accum=acc, env_faces=scenes.sky_cubemap(16), nthreads=cores)
        # (fail_ploc_rounds: the split-reference PLOC layout thrown away after it had re-sized the record array -- the path a mesh with
        # non-finite boxes takes; round 6: the records are gathered again in LBVH order before the LBVH is collapsed)
        for opts in ({}, {"split_refs": 0}, {"fast_bvh": "lbvh"}, {"fail_ploc_rounds": 1}):
            ctx = capi.Context(0)
            for k, val in opts.items():
                ctx.set_option(k, val)
            sc = capi.Scene(ctx)
            gm = capi.Model(ctx, v, t)
            for mi, x in inst:
                sc.add_model(gm, x)
            sc.build()
            n_rec = sc.wide_read(0)[2].shape[0]
            assert (n_rec > t.shape[0]) == (not opts), (opts, n_rec)
            assert_hits_equal(sc.trace(O, D, flags=0), want, "cables %s" % opts)
            assert_hits_equal(sc.trace(O, D, flags=ANY), want_any, "cables any-hit %s" % opts, closest=False)
            assert_hits_equal(sc.trace(O[:5000], D[:5000], flags=0, canonical=True), {k: a[:5000] for k, a in want.items()}, "cables canonical %s" % opts)
            p = capi.Pipeline(ctx)
            p.set_scene(sc)
            p.add_material(mat)
            p.set_environment_cube(scenes.sky_cubemap(16))
            p.create_output(W, H)
            p.build_acceleration_structures()
            for pfc in pfcs:
                p.update(pfc)
                p.render()
            assert np.array_equal(p.read_output(), acc), (opts, len(inst))


def test_a_nan_vertex_among_slivers(gpu, oracle, capi):
    """A mesh with split triangles AND a triangle with a NaN corner (which PLOC's nearest-neighbour rounds may refuse: the builder then falls
    back to the LBVH layout, after the split-reference path had already re-sized the records): whichever layout results, hits are the oracle's."""
    from util import sliver_soup
    v, t = sliver_soup(400, seed=21)
    v = v.copy()
    v["position"][t[401, 1], 0] = np.nan          # one of the small triangles
    cores = max(1, len(os.sched_getaffinity(0)))
    O, D = random_rays(50000, 43, [-6, -6, -6], [6, 6, 6])
    for opts in ({}, {"fail_ploc_rounds": 1}):
        ctx = capi.Context(0)
        for k, val in opts.items():
            ctx.set_option(k, val)
        p = Pair(oracle, capi, ctx, [(v, t)], [(0, None)])
        assert p.o.refs(0, t.shape[0])[0] is not None
        for flags in (0, CULL):
            assert_hits_equal(p.g.trace(O, D, flags=flags), p.o.trace(O, D, flags=flags, mode=1, nthreads=cores), "nan + slivers %s flags=%d" % (opts, flags))
        assert_hits_equal(p.g.trace(O, D, flags=ANY), p.o.trace(O, D, flags=ANY, mode=1, nthreads=cores), "nan + slivers any-hit", closest=False)
        ctx.close()


def test_debug_options_are_parsed_strictly(gpu, capi):
    """rt_debug_set_option: a value that is not a number is an error, not a silent 0 ('lds_top=true' used to switch the LDS top off);
    nor is one that strtod reads but that is no finite decimal number ('inf', 'nan', '0x10'); the name is judged before the value, so a
    misspelt option is reported as unknown whatever it is set to; blanks around the items of RT_DEBUG_OPTIONS are not part of them."""
    import subprocess
    import sys
    ctx = capi.Context(0)
    for name, value in (("lds_top", "true"), ("split_refs", "yes"), ("leaf_max", "4x"), ("sah_node", "one"), ("verbose", ""),
                        ("sah_node", "inf"), ("sah_node", "nan"), ("sah_node", "-inf"), ("sah_prim", "0x10"), ("sah_prim", "infinity"), ("leaf_max", "0x4")):
        with pytest.raises(capi.RtError):
            ctx.set_option(name, value)
    for name, value in (("lds_topp", "true"), ("no_such_option", "yes"), ("no_such_option", "1"), ("", "")):
        with pytest.raises(capi.RtError) as e:
            ctx.set_option(name, value)
        assert "unknown option" in str(e.value) and "not a number" not in str(e.value), str(e.value)
    with pytest.raises(capi.RtError) as e:
        ctx.set_option("leaf_max", "four")
    assert "not a number" in str(e.value), str(e.value)
    ctx.set_option("lds_top", 1)
    ctx.set_option("sah_node", "1.5")
    ctx.set_option("sah_prim", "2.5e-1")
    ctx.set_option("fast_bvh", "ploc")
    ctx.close()
    # the environment variable, read when a context is created: in a child process, with blanks around the items
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from dxrexperiments_amd import capi; c = capi.Context(0); c.close(); print('context ok')"
    for text, ok in (("lds_top=1 , leaf_max=3 ", True), (" lds_top = 1 ,, leaf_max=3", True), ("lds_top=1 , leaf_max=3 x", False), ("lds_topp=1", False)):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RT_DEBUG_OPTIONS=text), cwd=root, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        assert (r.returncode == 0 and "context ok" in r.stdout) == ok, (text, r.returncode, r.stdout[-2000:])
        if not ok:
            assert "RT_DEBUG_OPTIONS" in r.stdout, (text, r.stdout[-2000:])
