"""The production tree builder (PLOC, rt_bvh_ploc.hip; the four-wide collapse, the surface-area collapse and the byte quantiser,
rt_bvh_wide.hip) held to its numpy restatement (tests/wide_build_model.py, written from DESIGN.md section 4), node for node: the nodes
read back through rt_scene_wide_read are the model's words, the root code is the model's, the records are the model's bit for bit and in
its order.  Images cannot depend on the tree (the exactness rule), so no parity test sees the builder; the independent reader
(tests/wide_tree.py) sees whether a tree is valid and tight, not whether it is the tree the rule describes.  The input of the model is what the
C ABI reads back: the canonical tree (Morton-sorted leaves of a BLAS; the whole tree for a TLAS and for fast_bvh=lbvh) and the references
of a model with split triangles, whose keys are restated over the canonical root box."""
import numpy as np
import pytest

import wide_build_cases as C
import wide_build_model as M
import wide_tree as W
from util import hard_xforms, random_xforms

pytestmark = pytest.mark.gpu


def context(capi, opts):
    ctx = capi.Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def same_nodes(got, got_root, want, what):
    assert got_root == want["root"], "%s: root code %d, the model has %d" % (what, got_root, want["root"])
    diff = M.first_difference(got, want["nodes"])
    assert diff is None, "%s: %s" % (what, diff)


# ---- BLAS ----------------------------------------------------------------------------------------------------------

def blas_model(sc, v, i, opts):
    """the model's build of instance 0's BLAS from what the scene reads back"""
    cn = sc.bvh(0)[0]
    n = i.shape[0]
    assert cn.shape[0] == 2 * n - 1
    layout = "lbvh" if opts.get("fast_bvh") == "lbvh" else "ploc"
    sah = (opts.get("sah_node", 1.0), opts.get("sah_prim", 0.5)) if opts.get("wide_sah") else None
    off, ref_boxes, _ = sc.refs(0)
    count = None if off is None else np.diff(off).astype(np.int64)
    split_layout = off is not None and bool(opts.get("split_refs", 1)) and layout == "ploc"
    if split_layout:
        # the references by primitive, ordered by the Morton code of their centres over the canonical root box, ties by index
        prim = np.repeat(np.arange(n), count)
        order, _ = M.morton_order(ref_boxes, np.concatenate([cn["bmin"][0], cn["bmax"][0]]))
        leaves, prims = ref_boxes[order], prim[order]
    else:
        leaves = np.concatenate([cn["bmin"][n - 1:], cn["bmax"][n - 1:]], axis=1)
        prims = cn["left"][n - 1:]
    return M.build_blas(leaves, prims, opts.get("leaf_max", 2), canonical=cn, layout=layout, split_count=count, split_layout=split_layout, sah=sah)


def hold_blas(capi, name, opts, doubled=0, layout=None, split=None, model_opts=None):
    """builds mesh `name` under `opts` and holds nodes, root code and records to the model; then the independent reader, with the exact number
    of grids the quantiser had to coarsen.  model_opts: the options the model sees, where they are not the context's.  Returns the model's
    build."""
    v, i = C.mesh(name)
    ctx = context(capi, opts)
    sc = capi.Scene(ctx)
    model = capi.Model(ctx, v, i)
    sc.add_model(model)
    sc.build()
    what = "%s %s" % (name, opts)
    want = blas_model(sc, v, i, opts if model_opts is None else model_opts)
    if layout is not None:
        assert want["layout"] == layout, "%s: the case is meant for the %s layout" % (what, layout)
    if split is not None:
        assert (want["rec_boxes"] is not None) == split, "%s: the case is meant %s split references" % (what, "for" if split else "without")
    nodes, root, recs = sc.wide_read(0)
    same_nodes(nodes, root, want, what)
    want_recs = M.records(v["position"][i], want["prim"], want["mark"])
    assert np.array_equal(recs.view(np.uint32), want_recs), "%s: record %d is not the model's" % (
        what, int(np.nonzero((recs.view(np.uint32) != want_recs).any(axis=1))[0][0]) if recs.shape == want_recs.shape else -1)
    if want["rec_boxes"] is not None:
        assert np.array_equal(sc.refs(0)[2].view(np.uint32), want["rec_boxes"].view(np.uint32)), "%s: the records' boxes" % what
    assert int((want["doublings"] > 0).sum()) == doubled, "%s: the model coarsens %d grids" % (what, int((want["doublings"] > 0).sum()))
    if name != "huge":
        W.check_blas(sc, 0, v, i, doubled=doubled)
    sc.close()
    ctx.close()
    return want


@pytest.mark.parametrize("leaf_max", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [9, 64, 1000])
def test_blas_collapsed_from_the_lbvh(capi, n, leaf_max):
    hold_blas(capi, "fat_%d" % n, {"fast_bvh": "lbvh", "leaf_max": leaf_max}, layout="lbvh", split=False)


@pytest.mark.parametrize("leaf_max", [1, 2])
@pytest.mark.parametrize("n", C.PLOC_SIZES)
def test_blas_from_ploc(capi, n, leaf_max):
    """leaf_max = 1 shows the whole binary tree; 2 is the default.  Below 2 leaf_max + 2 leaves the layout is the LBVH's."""
    opts = {} if leaf_max == 2 else {"leaf_max": leaf_max}
    hold_blas(capi, "fat_%d" % n, opts, layout="ploc" if n >= 2 * leaf_max + 2 else "lbvh", split=False)


@pytest.mark.parametrize("leaf_max", [1, 2])
def test_blas_from_ploc_in_batches_of_one_round(capi, leaf_max):
    hold_blas(capi, "fat_6000", {"build_batch": 1, "leaf_max": leaf_max}, layout="ploc", split=False)


@pytest.mark.parametrize("leaf_max", [1, 2])
@pytest.mark.parametrize("name", ["clones300", "clones_in_soup", "clones2100", "flat_grid", "two_sheets"])
def test_ties(capi, name, leaf_max):
    """Where "the lowest index wins" and the halo decide the tree.  Clones merge one pair a round, always the first two clusters (DESIGN.md
    section 8), into a chain three leaves a level deep: 300 of them are 100 levels; the 600 of clones_in_soup lie across three workgroup
    edges of the rounds before the tail; 2100 of them alone would be 700 levels, which the collapse refuses (more than 254), so that mesh
    takes the LBVH layout -- by the model's rule as by the builder's."""
    hold_blas(capi, name, {"leaf_max": leaf_max}, layout="lbvh" if name == "clones2100" else "ploc", split=False)


@pytest.mark.parametrize("opts", [{}, {"leaf_max": 1}, {"split_refs": 0}, {"leaf_max": 8, "wide_sah": 1}], ids=str)
@pytest.mark.parametrize("name", ["slivers_small", "slivers_large"])
def test_split_references(capi, name, opts):
    """the leaves are the references: fewer than 2048 of them (the tail alone) and more"""
    want = hold_blas(capi, name, opts, layout="ploc", split=bool(opts.get("split_refs", 1)))
    if opts.get("split_refs", 1):
        n_refs = want["prim"].shape[0]
        assert (n_refs < 2048) == (name == "slivers_small") and n_refs > C.mesh(name)[1].shape[0], n_refs


def build_bytes(capi, name, opts):
    """what the C ABI reads back of mesh `name` built under `opts`: nodes, root code, records, then the three reference arrays (or None)"""
    v, i = C.mesh(name)
    ctx = context(capi, opts)
    sc = capi.Scene(ctx)
    sc.add_model(capi.Model(ctx, v, i))
    sc.build()
    out = [a.tobytes() if isinstance(a, np.ndarray) else a for a in sc.wide_read(0) + sc.refs(0)]
    sc.close()
    ctx.close()
    return out


@pytest.mark.parametrize("name", ["fat_6", "fat_2049", "slivers_small"])
def test_fallback_is_the_lbvh_layout(capi, name):
    """A PLOC layout that is thrown away (fail_ploc_rounds=1: what non-finite boxes do) leaves the LBVH layout and nothing else.  PLOC had
    rewritten the records in its own order -- for slivers_small one per REFERENCE, with their boxes -- and the fallback gathers them again,
    one per triangle, split ones with mark 2.  Held to the model's build of the LBVH layout, and byte for byte to a build under
    fast_bvh=lbvh.  fat_6 is the smallest mesh that runs PLOC at leaf_max 2; fat_2049 runs one multi-kernel round before the tail."""
    split = name == "slivers_small"
    want = hold_blas(capi, name, {"fail_ploc_rounds": 1}, layout="lbvh", split=False, model_opts={"fast_bvh": "lbvh"})
    assert want["prim"].shape[0] == C.mesh(name)[1].shape[0] and bool((want["mark"] == 2).any()) == split, \
        "%s: one record per triangle, the split ones (%s) marked 2" % (name, "some" if split else "none")
    fallback, lbvh = build_bytes(capi, name, {"fail_ploc_rounds": 1}), build_bytes(capi, name, {"fast_bvh": "lbvh"})
    assert (fallback[3] is not None) == split, "%s: the case is meant %s split triangles" % (name, "for" if split else "without")
    for k, what in enumerate(("nodes", "root code", "records", "reference offsets", "reference boxes", "record boxes")):
        assert fallback[k] == lbvh[k], "%s: the %s of the fallback are not those of fast_bvh=lbvh" % (name, what)


@pytest.mark.parametrize("costs", [{}, {"sah_node": 2.5, "sah_prim": 0.25}], ids=str)
@pytest.mark.parametrize("name, leaf_max", [("soup3000", 2), ("soup3000", 4), ("flat_grid", 2), ("fat_2049", 1)])
def test_surface_area_collapse(capi, name, leaf_max, costs):
    opts = dict(costs, wide_sah=1, leaf_max=leaf_max)
    want = hold_blas(capi, name, opts, layout="ploc")
    plain = blas_plain_nodes(capi, name, leaf_max)
    assert plain.shape != want["nodes"].shape or not np.array_equal(plain, want["nodes"]), "the option did not change the tree"


def blas_plain_nodes(capi, name, leaf_max):
    v, i = C.mesh(name)
    ctx = context(capi, {"leaf_max": leaf_max})
    sc = capi.Scene(ctx)
    model = capi.Model(ctx, v, i)
    sc.add_model(model)
    sc.build()
    return sc.wide_read(0)[0]


@pytest.mark.parametrize("name, doubled", [("far", 0), ("tiny", 0), ("sheet", 0), ("inexact", 0), ("tie", None), ("huge", 0)])
def test_quantiser_edges(capi, name, doubled):
    """Through real builds: 4000 units from the origin (neighbouring bytes decode to one float), extents of 1e-30, a zero-thickness sheet
    (the 2^-126 floor), an extent hi - lo that is not a float, an extent that overflows (an infinite scale, bytes 0 -- and PLOC finds no
    finite cost for the last pair, so the layout is the LBVH's).  doubled: how many grids the quantiser has to make coarser than
    255 s >= extent asks for, counted with the model on the CPU (tests/test_wide_build_model.py): none -- "inexact" included: its root takes
    the scale 64 on x, 255 * 64 is far beyond 1e4, nothing falls short -- except on "tie", which is made for it: one per node that spans the
    whole x range."""
    if name == "tie":
        want = hold_blas(capi, name, {}, doubled=TIE_DOUBLED, layout="ploc", split=False)
        d = want["doublings"]
        assert d[0, 0] == 1 and not d[:, 1:].any()
        assert (d[:, 0] > 0).sum() == TIE_DOUBLED
        return
    want = hold_blas(capi, name, {}, doubled=doubled, layout="lbvh" if name == "huge" else "ploc")
    if name == "huge":
        sc = np.stack([want["nodes"].view(np.float32)[:, k] for k in (3, 10, 11)], axis=1)
        assert np.isinf(sc[0, :2]).all() and not want["nodes"][0, 4:8].any()
    if name == "sheet":
        assert (want["nodes"].view(np.float32)[:, 10] == M.TINY).all()


TIE_DOUBLED = 1         # the nodes of "tie" that span lo = 2^-11 .. hi = 16320 + 2^-10: the root alone (the two triangles that carry the ends meet there)


# ---- TLAS ----------------------------------------------------------------------------------------------------------

def tlas_scene(capi, ctx, xf, masks=None):
    v, i = C.corner_soup(12, seed=9, extent=1.0)
    m = capi.Model(ctx, v, i)
    sc = capi.Scene(ctx)
    for x in xf:
        sc.add_model(m, x)
    if masks is not None:
        sc.set_masks(0, masks)
    sc.build()
    return sc


def hold_tlas(sc, n, what, visible=None, sah=None):
    cn = sc.bvh(-1)[0]
    visible = np.arange(n) if visible is None else visible
    assert cn.shape[0] == 2 * visible.size - 1
    assert np.array_equal(np.sort(cn["left"][visible.size - 1:]), visible), "%s: the canonical leaves do not name the visible instances" % what
    want = M.build_tlas(cn, sah=sah)
    nodes, root, recs = sc.wide_read(-1)
    assert recs.shape[0] == 0
    same_nodes(nodes, root, want, what)
    assert not (want["doublings"] > 0).any()
    boxes = np.stack([sc.instance_info(k)[0] for k in range(n)])
    if visible.size == n:
        W.check(nodes, root, boxes[:, :3], boxes[:, 3:], n, blas=False, doubled=0)
    else:
        # the reader counts items 0 .. n-1: name the visible instances by their rank
        rank = np.full(n, -1)
        rank[visible] = np.arange(visible.size)
        renamed = nodes.copy()
        code = renamed[:, 12:].view(np.int32)
        leaf = (code < 0) & (code != W.NONE)
        code[leaf] = ~rank[~code[leaf]]
        W.check(renamed, root, boxes[visible, :3], boxes[visible, 3:], visible.size, blas=False, doubled=0)
    return want


@pytest.mark.parametrize("n", [2, 3, 4, 5, 63, 64, 65, 257, 300])
def test_tlas(gpu, capi, n):
    sc = tlas_scene(capi, gpu, random_xforms(n, seed=40 + n))
    hold_tlas(sc, n, "%d instances" % n)
    sc.close()


@pytest.mark.parametrize("family", ["mirror", "stretch", "squash", "shear", "small", "large", "far"])
def test_tlas_under_hard_transforms(gpu, capi, family):
    sc = tlas_scene(capi, gpu, hard_xforms(family, 65, seed=7))
    hold_tlas(sc, 65, family)
    sc.close()


def test_tlas_with_a_third_hidden(gpu, capi):
    n = 257
    masks = np.where(np.arange(n) % 3 == 1, 0, 0xFF).astype(np.uint8)
    sc = tlas_scene(capi, gpu, random_xforms(n, seed=51), masks)
    hold_tlas(sc, n, "a third hidden", visible=np.nonzero(masks)[0])
    sc.close()


def test_tlas_after_an_update(gpu, capi):
    n = 300
    xf = random_xforms(n, seed=52)
    sc = tlas_scene(capi, gpu, xf)
    before = sc.wide_read(-1)[0]
    new = random_xforms(n, seed=53)
    sc.set_transforms(40, new[40:200])
    sc.set_mask(7, 0)
    sc.update()
    hold_tlas(sc, n, "after rt_scene_update", visible=np.delete(np.arange(n), 7))
    assert sc.wide_read(-1)[0].shape != before.shape or not np.array_equal(sc.wide_read(-1)[0], before)
    sc.close()


@pytest.mark.parametrize("costs", [{}, {"sah_node": 2.5, "sah_prim": 0.25}], ids=str)
def test_tlas_surface_area_collapse(capi, costs):
    ctx = context(capi, dict(costs, wide_sah=1))
    sc = tlas_scene(capi, ctx, random_xforms(300, seed=54))
    want = hold_tlas(sc, 300, "wide_sah %s" % costs, sah=(costs.get("sah_node", 1.0), costs.get("sah_prim", 0.5)))
    greedy = M.build_tlas(sc.bvh(-1)[0])
    assert greedy["nodes"].shape != want["nodes"].shape or not np.array_equal(greedy["nodes"], want["nodes"]), "the option did not change the tree"
    sc.close()
    ctx.close()
