"""Independent reader of the production traversal layout (rt_scene_wide_read): decodes the wide quantised nodes with
numpy, checks the invariants the traversal relies on and that every child box is as tight as its node's grid allows (check_tightness), and
prices the tree with the surface-area heuristic.

Nothing here is shared with the builder (rt_bvh_wide.hip) or the traversal (rt_trace_wave.h): the layout is taken from
the comment in include/dxr_amd.h.  Used by tests/test_gpu_wide_tree.py and tools/tree_quality.py."""
import numpy as np

NONE = -2 ** 31


def decode(nodes):
    """nodes: uint32[n, 16] (four-wide, 64 B) ->
    dict(lo float32[n, W, 3], hi float32[n, W, 3] (NaN: the axis bounds nothing), code int32[n, W], scale float32[n, 3], width W = 4).
    (The reader of round 3's eight-wide records left with that layout: dxrexperiments_amd/csrc/experiments/r03_wide8.patch.)"""
    assert nodes.shape[1] == 16, "not the four-wide layout"
    return decode4(nodes)


def decode4(nodes):
    f = nodes.view(np.float32)
    origin = f[:, 0:3]                                       # q0.xyz
    scale = np.stack([f[:, 3], f[:, 10], f[:, 11]], axis=1)  # q0.w, q2.z, q2.w
    words = {"lo": (nodes[:, 4], nodes[:, 6], nodes[:, 8]), "hi": (nodes[:, 5], nodes[:, 7], nodes[:, 9])}
    out = {"width": 4}
    for name, (wx, wy, wz) in words.items():
        planes = np.empty((nodes.shape[0], 4, 3), np.float32)
        for a, w in enumerate((wx, wy, wz)):
            for k in range(4):
                q = ((w >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.float32)
                # plane = fma(q, scale, origin); q <= 255 times a power of two is exact, so mul + add rounds once as well
                # (an unquantised axis: 0 * inf = NaN)
                with np.errstate(invalid="ignore"):
                    planes[:, k, a] = q * scale[:, a] + origin[:, a]
        out[name] = planes
    out["code"] = nodes[:, 12:16].view(np.int32).copy()
    out["scale"] = scale
    return out


def code_columns(nodes):
    """the slice of node words that holds the child codes"""
    return slice(12, 16)


def record_bounds(recs):
    """recs float32[m, 12] (p0 p1 p2 prim pad pad) -> (lo[m, 3], hi[m, 3], prim uint32[m])."""
    p = recs[:, :9].reshape(-1, 3, 3)
    return p.min(axis=1), p.max(axis=1), recs[:, 9].copy().view(np.uint32)


def levels_of(code):
    """breadth-first level of every node (root = node 0), and the parent count of every node."""
    n, WIDE = code.shape
    level = np.full(n, -1, np.int64)
    refs = np.zeros(n, np.int64)
    level[0] = 0
    frontier = np.array([0])
    while frontier.size:
        kids = code[frontier]
        lv = np.repeat(level[frontier], WIDE).reshape(-1, WIDE)
        m = kids >= 0
        ids = kids[m]
        np.add.at(refs, ids, 1)
        level[ids] = lv[m] + 1
        frontier = ids
    return level, refs


def grid_planes(origin, scale):
    """every plane fma(q, scale, origin), q = 0..255, of m grids: float32[m, 256], non-decreasing in q (the product is exact)"""
    q = np.arange(256, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (q[None, :] * scale[:, None] + origin[:, None]).astype(np.float32)


def finest_scale(ext):
    """the smallest power of two s >= 2^-126 with 255 s >= ext, for finite float32 extents; found with exact float64 products"""
    ext = ext.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(ext > 0, np.ceil(np.log2(np.where(ext > 0, ext, 1.0) / 255.0)), -126.0)
    e = np.clip(e, -126.0, 127.0)
    for _ in range(2):                                  # log2 may be one off at a power of two: settle with exact products
        e = np.where((e > -126) & (255.0 * np.exp2(e - 1) >= ext), e - 1, e)
        e = np.where((e < 127) & (255.0 * np.exp2(e) < ext), e + 1, e)
    return np.exp2(e).astype(np.float32)


def check_tightness(nodes, d, used, tlo, thi, chunk=2048):
    """Asserted for every used slot on every axis with a finite scale (tlo / thi: the true bounds of every child):
      * the decoded lo plane EQUALS the largest plane of the node's grid, fma(q, scale, origin) with q in 0..255, that is <= the child's true
        lo, and the decoded hi plane the smallest one that is >= its true hi.  In plane values, not bytes: far from the origin neighbouring
        bytes decode to the same float, and either byte is as tight;
      * the scale is the smallest power of two s >= 2^-126 with 255 s >= ext (ext = the node's hi - origin in fp32) whose last plane,
        fma(255, s, origin), reaches the node's hi.  Rounding can leave the last plane of the grid 255 s >= ext short of hi by an ulp; only
        then is the grid one power of two coarser.
    Returns the number of (node, axis) pairs on such a coarser grid."""
    n = nodes.shape[0]
    origin = nodes.view(np.float32)[:, 0:3]
    scale = d["scale"]
    doubled_axes = 0
    for at in range(0, n, chunk):
        sl = slice(at, min(n, at + chunk))
        for a in range(3):
            s, o = scale[sl, a], origin[sl, a]
            fin = np.isfinite(s)
            u = used[sl] & fin[:, None]
            planes = grid_planes(o, np.where(fin, s, np.float32(1.0)))
            for name, true, got in (("lo", tlo[sl, :, a], d["lo"][sl, :, a]), ("hi", thi[sl, :, a], d["hi"][sl, :, a])):
                with np.errstate(invalid="ignore"):
                    if name == "lo":
                        side = planes[:, None, :] <= true[:, :, None]
                        best = np.where(side, planes[:, None, :], -np.inf).max(axis=2)
                    else:
                        side = planes[:, None, :] >= true[:, :, None]
                        best = np.where(side, planes[:, None, :], np.inf).min(axis=2)
                    bad = u & np.isfinite(true) & (got != best)
                if bad.any():
                    k, slot = [int(x[0]) for x in np.nonzero(bad)]
                    raise AssertionError("node %d, slot %d, axis %d: the %s plane is %r, the grid has %r next to the child's %r" % (
                        at + k, slot, a, name, float(got[k, slot]), float(best[k, slot]), float(true[k, slot])))
            # the grid itself
            with np.errstate(invalid="ignore", over="ignore"):
                node_hi = np.where(used[sl], thi[sl, :, a], -np.inf).max(axis=1).astype(np.float32)
                ext = (node_hi - o).astype(np.float32)
                ok_ext = fin & np.isfinite(ext) & (ext < np.float32(3.0e38))
                want = finest_scale(np.where(ok_ext, ext, np.float32(0.0)))
                first = want.copy()
                for _ in range(8):
                    short = (want * np.float32(255.0) + o).astype(np.float32) < node_hi
                    want = np.where(short, want * np.float32(2.0), want)
                bad = ok_ext & (s != want)
                doubled_axes += int((ok_ext & (want != first)).sum())
            if bad.any():
                k = int(np.nonzero(bad)[0][0])
                raise AssertionError("node %d, axis %d: scale %r, the finest grid across the extent %r that reaches its end is %r" % (
                    at + k, a, float(s[k]), float(ext[k]), float(want[k])))
    return doubled_axes


def check(nodes, root_code, leaf_lo, leaf_hi, n_leaf_items, blas=True, doubled=None):
    """Invariants of a wide tree.  leaf_lo / leaf_hi: true bounds per record (BLAS) or per instance (TLAS).  doubled: if given, the exact
    number of (node, axis) grids that are coarser than their extent asks for (check_tightness).
    Returns a dict of statistics (largest_leaf: the most records any one leaf holds); raises AssertionError with a description on the first violation."""
    n = nodes.shape[0]
    if root_code < 0:
        assert n == 0, "a one-leaf structure has no nodes"
        code = ~root_code
        if blas:
            first, cnt = code >> 3, (code & 7) + 1
            assert first == 0 and cnt == n_leaf_items, "root leaf does not cover the structure"
        else:
            assert code == 0 and n_leaf_items == 1
        return {"nodes": 0, "levels": 0, "largest_leaf": int(n_leaf_items)}
    d = decode(nodes)
    code = d["code"]
    WIDE = d["width"]
    used = code != NONE
    assert np.all(used.sum(axis=1) >= 2), "a node with fewer than two children"
    assert np.all(used[:, :-1] | ~used[:, 1:]), "children not packed at the front"
    internal = used & (code >= 0)
    leaf = used & (code < 0)
    assert np.all(code[internal] < n) and np.all(code[internal] > 0), "child index out of range"
    level, refs = levels_of(code)
    assert np.all(level >= 0), "unreachable node"
    assert refs[0] == 0 and np.all(refs[1:] == 1), "a node with more than one parent"
    # breadth-first numbering: levels are contiguous and ascending (the first nodes are the LDS-resident top)
    assert np.all(np.diff(level) >= 0), "nodes are not in breadth-first order"
    # leaves cover every item exactly once
    covered = np.zeros(n_leaf_items, np.int64)
    lc = ~code[leaf]
    if blas:
        first, cnt = lc >> 3, (lc & 7) + 1
        assert np.all(first + cnt <= n_leaf_items), "leaf range out of bounds"
        for k in range(8):
            m = cnt > k
            np.add.at(covered, first[m] + k, 1)
    else:
        assert np.all(lc < n_leaf_items)
        np.add.at(covered, lc, 1)
    assert np.all(covered == 1), "%d items not covered exactly once" % int((covered != 1).sum())
    # true bounds of every child, bottom up
    inf = np.float32(np.inf)
    tlo = np.full((n, WIDE, 3), inf, np.float32)
    thi = np.full((n, WIDE, 3), -inf, np.float32)
    ni, ki = np.nonzero(leaf)
    lc = ~code[ni, ki]
    if blas:
        first, cnt = lc >> 3, (lc & 7) + 1
        for k in range(8):
            m = cnt > k
            tlo[ni[m], ki[m]] = np.minimum(tlo[ni[m], ki[m]], leaf_lo[first[m] + k])
            thi[ni[m], ki[m]] = np.maximum(thi[ni[m], ki[m]], leaf_hi[first[m] + k])
    else:
        tlo[ni, ki] = leaf_lo[lc]
        thi[ni, ki] = leaf_hi[lc]
    for lv in range(int(level.max()), -1, -1):
        at = np.nonzero(level == lv)[0]
        c = code[at]
        m = c >= 0
        a_i, k_i = np.nonzero(m)
        kid = c[m]
        tlo[at[a_i], k_i] = tlo[kid].min(axis=1)      # unused slots hold +-inf: neutral
        thi[at[a_i], k_i] = thi[kid].max(axis=1)
    # containment: the decoded box of every child holds everything below it (the exactness rule's premise)
    # (a NaN plane belongs to an axis the builder could not quantise: it bounds nothing and the traversal ignores it)
    with np.errstate(invalid="ignore"):
        ok = ((d["lo"] <= tlo) | np.isnan(d["lo"])) & ((d["hi"] >= thi) | np.isnan(d["hi"]))
    bad = used[:, :, None] & ~ok
    assert not bad.any(), "decoded child box does not contain its subtree at node %d" % int(np.nonzero(bad.any(axis=(1, 2)))[0][0])
    # quantisation grid: power-of-two scales
    sc = d["scale"]
    mant, _ = np.frexp(sc[np.isfinite(sc)])
    assert np.all(mant == 0.5), "a scale that is not a power of two"
    # tightness, whatever builder made the tree: on every finitely scaled axis each plane of a used slot is the nearest plane of the node's
    # grid on the child's side of it, and the grid is the finest power-of-two grid that reaches across the node
    doubled_axes = check_tightness(nodes, d, used, tlo, thi)
    if doubled is not None:
        assert doubled_axes == doubled, "%d axes on a grid coarser than 255 s >= extent asks for, %d expected" % (doubled_axes, doubled)
    return {"nodes": n, "levels": int(level.max()) + 1, "children_per_node": float(used.sum()) / n, "doubled_axes": doubled_axes,
            "leaf_children": int(leaf.sum()), "largest_leaf": int((((~code[leaf]) & 7) + 1).max()) if blas else 1, "decoded": d, "true_lo": tlo, "true_hi": thi, "level": level}


def check_blas(sc, which, v, i, doubled=None):
    """The BLAS of instance `which`'s model (capi.Scene.wide_read) against the mesh (v, i) it was built from: the records are the
    triangles bit for bit, every triangle -- or every reference of a split one (rt_refs.h) -- once, then check().
    Returns (statistics, nodes, root_code)."""
    nodes, root, recs = sc.wide_read(which)
    lo, hi, prim = record_bounds(recs)
    n = i.shape[0]
    off, boxes, rec_boxes = sc.refs(which)
    mark = recs.view(np.uint32)[:, 10]
    if off is None:
        assert recs.shape[0] == n and np.array_equal(np.sort(prim), np.arange(n, dtype=np.uint32)), "records are not a permutation of the triangles"
        assert not mark.any()
    else:
        # split references (round 5, rt_refs.h): a record per reference -- every triangle at least once, a split one once per box -- and a
        # record that is one of several is held by ITS box, which is what the child boxes above it must contain
        cnt = np.diff(off)
        single = recs.shape[0] == n                         # a layout that holds every triangle once (LBVH layout, option split_refs=0)
        assert np.array_equal(np.bincount(prim, minlength=n), np.ones(n, np.int64) if single else cnt), "records do not cover the references"
        assert np.array_equal(mark, np.where(cnt[prim] > 1, 2 if single else 1, 0))
        if not single:
            lo = np.where((mark == 1)[:, None], rec_boxes[:, :3], lo)
            hi = np.where((mark == 1)[:, None], rec_boxes[:, 3:], hi)
    tri = v["position"][i[prim]]                           # the record of primitive p holds p's vertices, bit for bit
    assert np.array_equal(recs[:, :9].reshape(-1, 3, 3), tri)
    st = check(nodes, root, lo, hi, recs.shape[0], blas=True, doubled=doubled)
    return st, nodes, root


def half_area(lo, hi):
    e = np.maximum(hi.astype(np.float64) - lo.astype(np.float64), 0.0)
    return e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0]


def sah(nodes, root_code, c_node=1.0, c_item=1.0):
    """Surface-area cost of the tree as the traversal sees it (decoded boxes): expected node steps and item tests of a
    random ray that hits the root box.  Returns (node_term, item_term)."""
    if root_code < 0 or nodes.shape[0] == 0:
        return 0.0, 1.0
    d = decode(nodes)
    code = d["code"]
    used = code != NONE
    area = np.where(used, half_area(d["lo"], d["hi"]), 0.0)
    root = half_area(d["lo"][0][used[0]].min(axis=0), d["hi"][0][used[0]].max(axis=0))
    internal = used & (code >= 0)
    leaf = used & (code < 0)
    cnt = np.where(leaf, ((~code) & 7) + 1, 0)
    node_term = c_node * (1.0 + float(area[internal].sum()) / root)
    item_term = c_item * float((area * cnt).sum()) / root
    return node_term, item_term
