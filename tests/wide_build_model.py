"""The production tree builder restated in numpy and plain Python (float32 throughout), written from DESIGN.md section 4
("The production tree, as a rule"): PLOC over the Morton-ordered leaves, the depth-first order of the records, the
area-greedy and the surface-area-optimal four-wide collapse, and the byte quantiser.  Nothing here is shared with
dxrexperiments_amd/csrc: the node layout is the comment in include/dxr_amd.h.  The build is compiled with -ffp-contract=off and
its only fused operation, plane = fma(q, scale, origin), has an exact product (q <= 255, power-of-two scale), so float32
numpy reproduces every bit.  Used by tests/test_wide_build_model.py (CPU) and tests/test_gpu_wide_build.py."""
import numpy as np

f32 = np.float32
NONE = np.uint32(0x80000000)            # RT_NODE_NONE: an unused slot
TINY = f32(2.0 ** -126)                 # the smallest normal number: the floor of a scale
INF = f32(np.inf)
RADIUS = 4                              # PLOC search window, either side
WIDE = 4
MAX_LEVELS = 254                        # of wide nodes: a deeper collapse is refused
FIELDS = ("origin.x", "origin.y", "origin.z", "scale.x", "lo.x bytes", "hi.x bytes", "lo.y bytes", "hi.y bytes", "lo.z bytes", "hi.z bytes",
          "scale.y", "scale.z", "code 0", "code 1", "code 2", "code 3")


class Tree:
    """A binary tree over n leaves: leaves are ids 0..n-1, internal nodes n..2n-2; left / right are indexed by id - n, box by id."""

    def __init__(self, n, left, right, box, root, instance=None):
        self.n, self.left, self.right, self.box, self.root, self.instance = n, left, right, box, root, instance
        self.size = self.offset = None


def area(lo, hi):
    """dx dy + dy dz + dz dx of boxes [..., 3], in fp32, summed left to right"""
    with np.errstate(all="ignore"):
        d = hi - lo
        return (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2]) + d[..., 2] * d[..., 0]


# ---- PLOC ----------------------------------------------------------------------------------------------------------

def _round_vectorised(b):
    """nearest neighbour of every cluster of b[c, 6]: all clusters at once, one window offset after the other"""
    c = b.shape[0]
    idx = np.arange(c)
    best = np.full(c, INF, f32)
    arg = idx.copy()
    for d in range(-RADIUS, RADIUS + 1):            # ascending j: the strictly smaller cost wins, so the lowest j wins ties
        if d == 0:
            continue
        j = idx + d
        ok = (j >= 0) & (j < c)
        jj = np.clip(j, 0, c - 1)
        cost = area(np.fmin(b[:, :3], b[jj, :3]), np.fmax(b[:, 3:], b[jj, 3:]))
        with np.errstate(invalid="ignore"):
            better = ok & (cost < best)
        best = np.where(better, cost, best)
        arg = np.where(better, jj, arg)
    return arg


def _round_one_by_one(b):
    """the same rule, cluster by cluster in plain Python (what the 'tail' of ploc() runs: a second statement of the round)"""
    c = b.shape[0]
    arg = np.arange(c)
    for i in range(c):
        best = INF
        for j in range(max(0, i - RADIUS), min(c, i + RADIUS + 1)):
            if j == i:
                continue
            cost = area(np.fmin(b[i, :3], b[j, :3]), np.fmax(b[i, 3:], b[j, 3:]))
            if cost < best:
                best, arg[i] = cost, j
    return arg


def ploc(leaf_boxes, tail=0):
    """leaf_boxes float32[n, 6] (lo, hi) in key order -> Tree.  Rounds with `tail` or fewer clusters are run by the one-by-one statement of the
    round; the result must not depend on it."""
    leaf_boxes = np.ascontiguousarray(leaf_boxes, f32)
    n = leaf_boxes.shape[0]
    assert n >= 2
    box = np.empty((2 * n - 1, 6), f32)
    box[:n] = leaf_boxes
    left = np.empty(n - 1, np.int64)
    right = np.empty(n - 1, np.int64)
    cl = np.arange(n)                               # the clusters' nodes, in order
    nxt = n
    while cl.shape[0] > 1:
        c = cl.shape[0]
        b = box[cl]
        nn = _round_one_by_one(b) if c <= tail else _round_vectorised(b)
        idx = np.arange(c)
        mutual = (nn != idx) & (nn[nn] == idx)
        lower = np.nonzero(mutual & (idx < nn))[0]  # ascending: the pairs in the order of their lower index
        if lower.size == 0:
            raise ArithmeticError("PLOC made no progress (%d clusters)" % c)
        upper = nn[lower]
        ids = nxt + np.arange(lower.size)
        left[ids - n] = cl[lower]
        right[ids - n] = cl[upper]
        box[ids, :3] = np.fmin(b[lower, :3], b[upper, :3])
        box[ids, 3:] = np.fmax(b[lower, 3:], b[upper, 3:])
        cl = cl.copy()
        cl[lower] = ids                             # the new cluster takes the lower index's place
        keep = np.ones(c, bool)
        keep[upper] = False
        cl = cl[keep]                               # survivors keep their order
        nxt += lower.size
    assert nxt == 2 * n - 1
    return Tree(n, left, right, box, 2 * n - 2)


def tree_from_canonical(nodes, tlas):
    """the canonical LBVH (rt_scene_bvh_read: internal nodes 0..n-2, leaf k at n-1+k, boxes as refitted) in the numbering above:
    leaf k -> id k, internal c -> id n + c; root = n.  A TLAS leaf names its instance in `left`."""
    n = (nodes.shape[0] + 1) // 2
    box = np.empty((2 * n - 1, 6), f32)
    ids = np.concatenate([n + np.arange(n - 1), np.arange(n)])
    box[ids, :3] = nodes["bmin"]
    box[ids, 3:] = nodes["bmax"]
    to_id = lambda c: np.where(c >= n - 1, c - (n - 1), n + c)
    left = to_id(nodes["left"][:n - 1].astype(np.int64))
    right = to_id(nodes["right"][:n - 1].astype(np.int64))
    return Tree(n, left, right, box, n, instance=nodes["left"][n - 1:].astype(np.int64) if tlas else None)


def dfs_offsets(tree):
    """(size, offset) of every node: leaves below it, and leaves before it in depth-first, left-first order"""
    n = tree.n
    size = np.ones(2 * n - 1, np.int64)
    offset = np.zeros(2 * n - 1, np.int64)
    order = []
    stack = [tree.root]
    while stack:
        v = stack.pop()
        order.append(v)
        if v >= n:
            stack.append(tree.left[v - n])
            stack.append(tree.right[v - n])
    for v in reversed(order):                       # children before parents
        if v >= n:
            size[v] = size[tree.left[v - n]] + size[tree.right[v - n]]
    for v in order:                                 # parents before children
        if v >= n:
            l = tree.left[v - n]
            offset[l] = offset[v]
            offset[tree.right[v - n]] = offset[v] + size[l]
    tree.size, tree.offset = size, offset
    return size, offset


# ---- the collapse --------------------------------------------------------------------------------------------------

def sah_table(tree, c_node, c_prim, leaf_max=2, tlas=False):
    """The bottom-up table of the surface-area-optimal collapse, per internal node: cost[i-1] of the subtree as at most i roots, pick[i-1]
    (i = 1: 0 leaf / 1 wide node; i >= 2: 0 = as with i - 1 roots, k = k roots from the left child), and spread = the k of the best split
    of all four slots.  Returns (cost float32[n-1, 4], pick int[n-1, 4], spread int[n-1])."""
    n = tree.n
    if tree.size is None:
        dfs_offsets(tree)
    c_node, c_prim = f32(c_node), f32(c_prim)
    box_a = area(tree.box[:, :3], tree.box[:, 3:])
    cost = np.full((n - 1, WIDE), INF, f32)
    pick = np.zeros((n - 1, WIDE), np.int64)
    spread = np.ones(n - 1, np.int64)

    def as_one_leaf(v):
        with np.errstate(all="ignore"):
            return box_a[v] * c_prim * f32(1 if tlas else tree.size[v])

    may_be_leaf = lambda v: v < n or (not tlas and tree.size[v] <= leaf_max)
    order = []
    stack = [tree.root]
    while stack:
        v = stack.pop()
        if v >= n:
            order.append(v)
            stack += [tree.left[v - n], tree.right[v - n]]
    with np.errstate(all="ignore"):
        for p in reversed(order):
            side = []
            for kid in (tree.left[p - n], tree.right[p - n]):
                side.append(np.full(WIDE, as_one_leaf(kid), f32) if kid < n else cost[kid - n])
            cl, cr = side
            co = np.full(WIDE, INF, f32)
            pk = [0] * WIDE
            for j in range(2, WIDE + 1):
                best, bk = INF, 1
                for k in range(1, j):
                    v = cl[k - 1] + cr[j - k - 1]
                    if v < best or k == 1:
                        best, bk = v, k
                co[j - 1], pk[j - 1] = best, bk
            spread[p - n] = pk[WIDE - 1]
            node = box_a[p] * c_node + co[WIDE - 1]
            leaf = may_be_leaf(p) and bool(as_one_leaf(p) <= node)
            co[0] = as_one_leaf(p) if leaf else node
            pk[0] = 0 if leaf else 1
            for i in range(2, WIDE + 1):            # more roots never cost more
                if not co[i - 1] < co[i - 2]:
                    co[i - 1], pk[i - 1] = co[i - 2], 0
            cost[p - n], pick[p - n] = co, pk
    return cost, pick, spread


def _sah_roots(tree, pick, v, budget):
    """the roots the subtree of v contributes with at most `budget` slots, left first"""
    n = tree.n
    if v < n:
        return [v]
    i = budget
    while i > 1 and pick[v - n, i - 1] == 0:
        i -= 1
    if i == 1:
        return [v]
    k = int(pick[v - n, i - 1])
    return _sah_roots(tree, pick, tree.left[v - n], k) + _sah_roots(tree, pick, tree.right[v - n], i - k)


def collapse(tree, leaf_max, tlas, sah=None):
    """Tree -> (kids int64[m, 4] (ids of the children in their slots, -1 unused), codes int32[m, 4], frontier int64[m] (the binary node of
    every wide node), root_code).  sah: None for the area-greedy collapse, or sah_table()'s result."""
    n = tree.n
    if tree.size is None:
        dfs_offsets(tree)
    box_a = area(tree.box[:, :3], tree.box[:, 3:])

    def is_leaf(v):
        if v < n:
            return True
        if sah is not None:
            return sah[1][v - n, 0] == 0
        return not tlas and tree.size[v] <= leaf_max

    def leaf_code(v):
        return ~int(tree.instance[v]) if tlas else ~int((int(tree.offset[v]) << 3) | (int(tree.size[v]) - 1))

    kids_out, codes_out, frontier_out = [], [], []
    frontier = [tree.root]
    base = levels = 0
    while frontier:
        levels += 1
        if levels > MAX_LEVELS:
            raise ArithmeticError("deeper than %d levels of wide nodes" % MAX_LEVELS)
        nxt_base = base + len(frontier)             # the next level starts right behind this one
        nxt = []
        for b in frontier:
            l, r = int(tree.left[b - n]), int(tree.right[b - n])
            if sah is not None:
                k = int(sah[2][b - n])
                open_ = _sah_roots(tree, sah[1], l, k) + _sah_roots(tree, sah[1], r, WIDE - k)
            else:
                open_ = [l, r]
                while len(open_) < WIDE:
                    best = -1
                    for k, v in enumerate(open_):
                        if is_leaf(v):
                            continue
                        if best < 0 or box_a[v] > box_a[open_[best]]:      # strictly larger: the first wins ties
                            best = k
                    if best < 0:
                        break
                    v = open_[best]
                    open_[best] = int(tree.left[v - n])
                    open_.append(int(tree.right[v - n]))
            slots = list(open_)
            for i in range(1, len(slots)):          # insertion sort by area, descending, stable
                j = i
                while j > 0 and box_a[slots[j]] > box_a[slots[j - 1]]:
                    slots[j], slots[j - 1] = slots[j - 1], slots[j]
                    j -= 1
            code = []
            for v in slots:
                if is_leaf(v):
                    code.append(leaf_code(v))
                else:
                    code.append(nxt_base + len(nxt))
                    nxt.append(v)
            pad = WIDE - len(slots)
            kids_out.append(slots + [-1] * pad)
            codes_out.append(code + [-2 ** 31] * pad)
            frontier_out.append(b)
        base = nxt_base
        frontier = nxt
    return (np.array(kids_out, np.int64).reshape(-1, WIDE), np.array(codes_out, np.int64).astype(np.int32).reshape(-1, WIDE),
            np.array(frontier_out, np.int64), 0)


# ---- the quantiser -------------------------------------------------------------------------------------------------

def start_scale(ext):
    """the smallest power of two s >= 2^-126 with 255 s >= ext (float32 array); 2^-126 for a zero, denormal or unusable extent"""
    ext = np.asarray(ext, f32)
    with np.errstate(all="ignore"):
        m, e = np.frexp((ext / f32(255.0)).astype(f32))
        s = np.ldexp(f32(1.0), np.where(m == 0.5, e - 1, e).astype(np.int32)).astype(f32)
        s = np.where((ext > 0) & (ext < f32(3.0e38)), s, TINY)
        return np.where(s >= TINY, s, TINY).astype(f32)


def _plane(q, s, o):
    with np.errstate(all="ignore"):
        return (q.astype(f32) * s + o).astype(f32)  # = fma(q, s, o): the product is exact


def _axis_bytes(l, h, valid, o, s):
    """one axis of m nodes: planes l, h [m, 4] of the children, origin and scale [m, 1] -> (lo bytes, hi bytes, reached [m])"""
    with np.errstate(all="ignore"):
        fl = np.floor((l - o) / s)
        fh = np.ceil((h - o) / s)
        ql = np.where(fl > 0, np.where(fl < 255, fl, f32(255)), f32(0)).astype(np.int64)       # (NaN -> 0)
        qh = np.where(fh > 0, np.where(fh < 255, fh, f32(255)), f32(0)).astype(np.int64)
        while True:
            step = valid & (ql > 0) & (_plane(ql, s, o) > l)
            if not step.any():
                break
            ql -= step
        while True:
            step = valid & (qh < 255) & (_plane(qh, s, o) < h)
            if not step.any():
                break
            qh += step
        # ... and in again, to the farther of the next two planes that still holds the child and decodes to a different float
        near2, near1 = _plane(ql + 2, s, o), _plane(ql + 1, s, o)
        two = valid & (ql + 2 <= 255) & (near2 <= l) & (near2 > _plane(ql, s, o))
        one = valid & ~two & (ql + 1 <= 255) & (near1 <= l) & (near1 > _plane(ql, s, o))
        ql = ql + 2 * two + one
        near2, near1 = _plane(qh - 2, s, o), _plane(qh - 1, s, o)
        two = valid & (qh - 2 >= 0) & (near2 >= h) & (near2 < _plane(qh, s, o))
        one = valid & ~two & (qh - 1 >= 0) & (near1 >= h) & (near1 < _plane(qh, s, o))
        qh = qh - 2 * two - one
        short = valid & ((_plane(ql, s, o) > l) | (_plane(qh, s, o) < h))
    ql = np.where(valid, ql, 255)
    qh = np.where(valid, qh, 0)
    return ql, qh, ~short.any(axis=-1)


def quantise(node_box, child_boxes, valid=None):
    """node_box float32[..., 6], child_boxes float32[..., 4, 6], valid bool[..., 4] (default: all) ->
    (scale float32[..., 3], lo bytes int[..., 4, 3], hi bytes int[..., 4, 3], doublings int[..., 3] (-1: not quantisable))"""
    node_box = np.asarray(node_box, f32)
    single = node_box.ndim == 1
    nb = node_box.reshape(-1, 6)
    cb = np.asarray(child_boxes, f32).reshape(-1, WIDE, 6)
    m = nb.shape[0]
    valid = np.ones((m, WIDE), bool) if valid is None else np.asarray(valid, bool).reshape(m, WIDE)
    scale = np.empty((m, 3), f32)
    lo8 = np.zeros((m, WIDE, 3), np.int64)
    hi8 = np.zeros((m, WIDE, 3), np.int64)
    doublings = np.zeros((m, 3), np.int64)
    for a in range(3):
        o = nb[:, a:a + 1]
        with np.errstate(all="ignore"):
            s = start_scale(nb[:, 3 + a] - nb[:, a])[:, None]
        todo = np.ones(m, bool)
        for tries in range(8):
            at = np.nonzero(todo)[0]
            if at.size == 0:
                break
            ql, qh, reached = _axis_bytes(cb[at, :, a], cb[at, :, 3 + a], valid[at], o[at], s[at])
            ok = reached & (s[at, 0] < f32(1.0e38))
            done = at[ok]
            lo8[done, :, a], hi8[done, :, a] = ql[ok], qh[ok]
            doublings[done, a] = tries
            todo[done] = False
            with np.errstate(over="ignore"):
                s[at[~ok]] = s[at[~ok]] * f32(2.0)  # the last step fell short: a coarser grid
        scale[:, a] = np.where(todo, INF, s[:, 0])  # not quantisable: an infinite scale, all bytes 0
        doublings[todo, a] = -1
    if single:
        return scale[0], lo8[0], hi8[0], doublings[0]
    return scale, lo8, hi8, doublings


# ---- whole builds ----------------------------------------------------------------------------------------------------

def emit(tree, kids, codes, frontier):
    """the nodes as uint32[m, 16] in the layout of include/dxr_amd.h, and the quantiser's doublings per node and axis"""
    m = kids.shape[0]
    valid = kids >= 0
    cb = tree.box[np.where(valid, kids, 0)]
    nb = tree.box[frontier]
    scale, lo8, hi8, doublings = quantise(nb, cb, valid)
    out = np.zeros((m, 16), np.uint32)
    fl = out.view(f32)
    fl[:, 0:3] = nb[:, :3]
    fl[:, 3], fl[:, 10], fl[:, 11] = scale[:, 0], scale[:, 1], scale[:, 2]
    shifts = (np.arange(WIDE) * 8)[None, :]
    for a in range(3):
        out[:, 4 + 2 * a] = (lo8[:, :, a] << shifts).sum(axis=1).astype(np.uint32)
        out[:, 5 + 2 * a] = (hi8[:, :, a] << shifts).sum(axis=1).astype(np.uint32)
    out[:, 12:16] = codes.view(np.uint32)
    return out, doublings


def _wide(tree, leaf_max, tlas, sah_costs):
    dfs_offsets(tree)
    sah = None if sah_costs is None else sah_table(tree, sah_costs[0], sah_costs[1], leaf_max, tlas)
    kids, codes, frontier, root = collapse(tree, leaf_max, tlas, sah)
    nodes, doublings = emit(tree, kids, codes, frontier)
    return nodes, root, doublings


def build_blas(leaf_boxes, leaf_prim, leaf_max, canonical=None, layout="ploc", split_count=None, split_layout=False, sah=None, tail=0):
    """A BLAS.  leaf_boxes float32[n, 6] / leaf_prim[n]: the leaves in key order (the canonical leaves, or the references of a model with
    split triangles: split_layout); canonical: the canonical nodes (the LBVH layout, which a BLAS of n < 2 leaf_max + 2 leaves takes);
    split_count[prim]: references of every primitive (None: no triangle is split); sah: None or (c_node, c_prim).
    Returns dict(nodes, root, prim (of every record, in order), mark, rec_boxes (split layout: the box of every record), doublings, layout)."""
    n = leaf_boxes.shape[0]
    leaf_prim = np.asarray(leaf_prim, np.int64)
    use_ploc = layout == "ploc" and n >= 2 * leaf_max + 2
    if use_ploc:
        try:
            tree = ploc(leaf_boxes, tail)
            wide = _wide(tree, leaf_max, False, sah)
        except ArithmeticError:                     # no pair with a finite cost, or a tree too deep to collapse: such a mesh keeps the LBVH layout
            use_ploc = False
    out = {"layout": "ploc" if use_ploc else "lbvh", "rec_boxes": None}
    if use_ploc:
        size, offset = dfs_offsets(tree)
        order = np.empty(n, np.int64)
        order[offset[:n]] = np.arange(n)            # record r holds leaf order[r]
        out["prim"] = leaf_prim[order]
        if split_layout:
            out["mark"] = np.where(split_count[out["prim"]] > 1, 1, 0)
            out["rec_boxes"] = np.asarray(leaf_boxes, f32)[order]
        else:
            out["mark"] = np.zeros(n, np.int64) if split_count is None else np.where(split_count[out["prim"]] > 1, 2, 0)
        out["nodes"], out["root"], out["doublings"] = wide
        out["tree"] = tree
        return out
    # the LBVH layout: one record per triangle in key order, whatever the references
    cn = canonical
    n = (cn.shape[0] + 1) // 2
    out["prim"] = cn["left"][n - 1:].astype(np.int64)
    out["mark"] = np.zeros(n, np.int64) if split_count is None else np.where(split_count[out["prim"]] > 1, 2, 0)
    if n <= leaf_max:                               # the whole structure is one leaf
        out["nodes"], out["root"], out["doublings"] = np.zeros((0, 16), np.uint32), ~(n - 1), np.zeros((0, 3), np.int64)
        return out
    tree = tree_from_canonical(cn, False)
    out["nodes"], out["root"], out["doublings"] = _wide(tree, leaf_max, False, sah)
    out["tree"] = tree
    return out


def build_tlas(canonical_nodes, sah=None):
    """A TLAS from the canonical tree over the visible instances (a leaf names its instance in `left`)."""
    n = (canonical_nodes.shape[0] + 1) // 2
    if n == 1:
        return {"nodes": np.zeros((0, 16), np.uint32), "root": ~0, "doublings": np.zeros((0, 3), np.int64)}
    tree = tree_from_canonical(canonical_nodes, True)
    nodes, root, doublings = _wide(tree, 1, True, sah)
    return {"nodes": nodes, "root": root, "doublings": doublings, "tree": tree}


def records(positions, prim, mark):
    """the 48-B records: p0 p1 p2 of the primitive bit for bit, its index, the mark, a zero word"""
    out = np.zeros((prim.shape[0], 12), np.uint32)
    out[:, :9] = np.ascontiguousarray(positions, f32).reshape(-1, 9).view(np.uint32)[prim]
    out[:, 9] = prim
    out[:, 10] = mark
    return out


# ---- keys of the references ----------------------------------------------------------------------------------------

def _spread10(v):
    v = v.astype(np.uint64) & np.uint64(0x3FF)
    out = np.zeros_like(v)
    for bit in range(10):
        out |= ((v >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit)
    return out


def morton_order(boxes, bounds):
    """The order of boxes[m, 6] by the 30-bit Morton code of their centres over bounds[6] (x in the highest bit of every triple), ties by
    index: centre = (lo + hi) * 0.5, cell = (centre - lo_b) / ext_b * 1024 clamped to [0, 1023] and truncated (0 for an extent that is not
    positive).  Returns (order, codes)."""
    boxes = np.asarray(boxes, f32)
    bounds = np.asarray(bounds, f32)
    code = np.zeros(boxes.shape[0], np.uint64)
    with np.errstate(all="ignore"):
        for c in range(3):
            ctr = (boxes[:, c] + boxes[:, 3 + c]) * f32(0.5)
            ext = bounds[3 + c] - bounds[c]
            if ext > 0:
                q = (ctr - bounds[c]) / ext * f32(1024.0)
                q = np.fmin(np.fmax(q, f32(0.0)), f32(1023.0))
                cell = q.astype(np.int64)
            else:
                cell = np.zeros(boxes.shape[0], np.int64)
            code |= _spread10(cell) << np.uint64(2 - c)
    return np.argsort(code, kind="stable"), code


# ---- comparison ----------------------------------------------------------------------------------------------------

def first_difference(got, want):
    """None if two node arrays are the same words, else a sentence that names the first node, slot and field that differ"""
    if got.shape != want.shape:
        return "%d nodes, the model has %d" % (got.shape[0], want.shape[0])
    bad = np.nonzero(got != want)
    if bad[0].size == 0:
        return None
    node, word = int(bad[0][0]), int(bad[1][0])
    g, w = got[node, word], want[node, word]
    if word in (0, 1, 2, 3, 10, 11):
        return "node %d, %s: %r, the model has %r" % (node, FIELDS[word], float(got.view(f32)[node, word]), float(want.view(f32)[node, word]))
    if word >= 12:
        return "node %d, slot %d, code: %d, the model has %d (codes %s / %s)" % (
            node, word - 12, int(np.int32(g)), int(np.int32(w)), got[node, 12:].view(np.int32).tolist(), want[node, 12:].view(np.int32).tolist())
    slot = next(k for k in range(WIDE) if ((int(g) ^ int(w)) >> (8 * k)) & 0xFF)
    return "node %d, slot %d, %s: %d, the model has %d" % (node, slot, FIELDS[word], (int(g) >> (8 * slot)) & 0xFF, (int(w) >> (8 * slot)) & 0xFF)
