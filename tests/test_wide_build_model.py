"""The numpy restatement of the production tree builder (tests/wide_build_model.py) held to what it claims, without a GPU and without
the library: its trees are valid and tight by the independent reader (tests/wide_tree.py), its binary trees are trees, the result does not
depend on where the one-by-one 'tail' statement of a PLOC round takes over, and small inputs give answers worked out by hand.  The
builder itself is held to this model by tests/test_gpu_wide_build.py, on the same meshes (tests/wide_build_cases.py)."""
import itertools

import numpy as np
import pytest

import wide_build_cases as C
import wide_build_model as M
import wide_tree as W

f32 = np.float32


def cpu_leaves(v, i):
    """the leaves of a mesh without split triangles, as the canonical builder orders them: triangle boxes by the Morton code of their centres"""
    boxes = C.triangle_boxes(v, i)
    bounds = np.concatenate([np.fmin.reduce(boxes[:, :3], axis=0), np.fmax.reduce(boxes[:, 3:], axis=0)])
    order, _ = M.morton_order(boxes, bounds)
    return boxes[order], order


def slab_references(v, i, pieces=6):
    """references of the model's own making: the box of every triangle whose longest side is over a tenth of the mesh cut into slabs"""
    boxes = C.triangle_boxes(v, i)
    whole = np.fmax.reduce(boxes[:, 3:], axis=0) - np.fmin.reduce(boxes[:, :3], axis=0)
    out, prim = [], []
    for p, b in enumerate(boxes):
        ext = b[3:] - b[:3]
        a = int(np.argmax(ext))
        k = pieces if ext[a] > 0.1 * whole.max() else 1
        cuts = np.linspace(b[a], b[3 + a], k + 1).astype(f32)
        for j in range(k):
            r = b.copy()
            r[a], r[3 + a] = cuts[j], cuts[j + 1]
            out.append(r)
            prim.append(p)
    return np.array(out, f32), np.array(prim)


def check_binary_tree(tree, leaf_boxes):
    n = tree.n
    assert tree.left.shape[0] == n - 1 and tree.box.shape[0] == 2 * n - 1 and tree.root == 2 * n - 2
    assert np.array_equal(tree.box[:n], leaf_boxes)
    kids = np.concatenate([tree.left, tree.right])
    assert np.array_equal(np.sort(kids), np.arange(2 * n - 2)), "a node that is not the child of exactly one node"
    assert np.all(tree.left < n + np.arange(n - 1)) and np.all(tree.right < n + np.arange(n - 1)), "a child created after its parent"
    l, r = tree.box[tree.left], tree.box[tree.right]
    assert np.array_equal(tree.box[n:, :3], np.fmin(l[:, :3], r[:, :3])) and np.array_equal(tree.box[n:, 3:], np.fmax(l[:, 3:], r[:, 3:]))
    size, offset = M.dfs_offsets(tree)
    assert size[tree.root] == n and np.array_equal(np.sort(offset[:n]), np.arange(n)), "leaves not covered once"


def check_build(out, bounds_lo, bounds_hi, leaf_max):
    n_rec = out["prim"].shape[0]
    st = W.check(out["nodes"], out["root"], bounds_lo, bounds_hi, n_rec, blas=True, doubled=int((out["doublings"] > 0).sum()))
    assert st["largest_leaf"] <= leaf_max
    return st


BLAS_CASES = ["fat_%d" % n for n in C.PLOC_SIZES] + ["clones300", "flat_grid", "two_sheets", "far", "tiny", "sheet", "inexact", "tie"]


def takes_ploc(name, leaf_max):
    return not name.startswith("fat_") or int(name[4:]) >= 2 * leaf_max + 2      # (smaller: the LBVH layout, whose input is the canonical tree)


@pytest.mark.parametrize("name, leaf_max", [(n, l) for n in BLAS_CASES for l in (1, 2) if takes_ploc(n, l)])
def test_the_models_trees_are_valid_and_tight(name, leaf_max):
    v, i = C.mesh(name)
    boxes, order = cpu_leaves(v, i)
    out = M.build_blas(boxes, order, leaf_max)
    assert out["layout"] == "ploc"
    check_binary_tree(out["tree"], boxes)
    assert np.array_equal(np.sort(out["prim"]), np.arange(i.shape[0]))
    tri = C.triangle_boxes(v, i)[out["prim"]]
    check_build(out, tri[:, :3], tri[:, 3:], leaf_max)


def test_doublings_of_the_quantiser_on_these_meshes():
    """How often the quantiser has to take a coarser grid than the extent asks for, counted here so that the GPU test can name the number:
    nowhere, except on the mesh made for it."""
    for name in BLAS_CASES:
        v, i = C.mesh(name)
        boxes, order = cpu_leaves(v, i)
        for leaf_max in (1, 2):
            if not takes_ploc(name, leaf_max):
                continue
            d = M.build_blas(boxes, order, leaf_max)["doublings"]
            assert (d >= 0).all()
            if name == "tie":
                assert (d[:, 0] > 0).sum() >= 1 and d[0, 0] == 1 and not d[:, 1:].any()
            else:
                assert not d.any(), name


@pytest.mark.parametrize("sah", [None, (1.0, 0.5), (2.5, 0.25)])
def test_split_references_and_both_collapses(sah):
    v, i = C.mesh("slivers_small")
    ref_boxes, ref_prim = slab_references(v, i)
    assert ref_boxes.shape[0] > i.shape[0]
    whole = np.concatenate([np.fmin.reduce(ref_boxes[:, :3], axis=0), np.fmax.reduce(ref_boxes[:, 3:], axis=0)])
    order, _ = M.morton_order(ref_boxes, whole)
    count = np.bincount(ref_prim, minlength=i.shape[0])
    for leaf_max in (1, 2, 8):
        out = M.build_blas(ref_boxes[order], ref_prim[order], leaf_max, split_count=count, split_layout=True, sah=sah)
        assert np.array_equal(np.bincount(out["prim"], minlength=i.shape[0]), count)
        assert np.array_equal(out["mark"], (count[out["prim"]] > 1).astype(np.int64))
        check_build(out, out["rec_boxes"][:, :3], out["rec_boxes"][:, 3:], leaf_max)


def test_the_sah_collapse_is_never_costlier_than_the_greedy_one():
    """the table's own claim: cost[0] of the root is the cheapest forest, so the tree it picks costs no more under its own measure than
    the area-greedy tree over the same binary tree"""
    v, i = C.mesh("fat_2049")
    boxes, order = cpu_leaves(v, i)
    tree = M.ploc(boxes)
    M.dfs_offsets(tree)
    box_a = M.area(tree.box[:, :3], tree.box[:, 3:]).astype(np.float64)

    def price(kids, frontier, c_node, c_prim):
        total = c_node * box_a[frontier].sum()
        leaves = [k for row, _ in zip(kids, frontier) for k in row if k >= 0]
        internal = set(frontier.tolist())
        return total + sum(c_prim * box_a[k] * tree.size[k] for k in leaves if k not in internal)

    for c_node, c_prim in ((1.0, 0.5), (2.5, 0.25)):
        table = M.sah_table(tree, c_node, c_prim, leaf_max=2)
        ks, _, fs, _ = M.collapse(tree, 2, False, table)
        kg, _, fg, _ = M.collapse(tree, 2, False, None)
        best = price(ks, fs, c_node, c_prim)
        assert best <= price(kg, fg, c_node, c_prim) * (1 + 1e-6)
        assert abs(best - float(table[0][tree.root - tree.n, 0])) <= 1e-4 * best, "the table's cost of the root is not the cost of its tree"


@pytest.mark.parametrize("name, tails", [("fat_257", (0, 64, 2048)), ("fat_2049", (0, 64, 2048)), ("clones300", (0, 64)), ("two_sheets", (0, 64))])
def test_where_the_tail_takes_over_does_not_show(name, tails):
    v, i = C.mesh(name)
    boxes, _ = cpu_leaves(v, i)
    trees = [M.ploc(boxes, tail=t) for t in tails]
    for t in trees[1:]:
        assert np.array_equal(t.left, trees[0].left) and np.array_equal(t.right, trees[0].right)
        assert np.array_equal(t.box.view(np.uint32), trees[0].box.view(np.uint32))


@pytest.mark.parametrize("n", [2, 5, 9, 40])
def test_identical_boxes_merge_the_first_pair_every_round(n):
    """All costs tie, so every cluster picks the lowest index in its window: cluster 0 picks 1, cluster 1 picks 0, everyone else somebody
    lower who does not pick them back.  One merge per round, always (0, 1): a caterpillar, written out here."""
    box = np.tile(np.array([1, 2, 3, 4, 6, 8], f32), (n, 1))
    for tail in (0, 64):
        t = M.ploc(box, tail=tail)
        assert t.left.tolist() == [0] + [n + k for k in range(n - 2)]
        assert t.right.tolist() == list(range(1, n))
        assert np.array_equal(t.box, np.tile(box[0], (2 * n - 1, 1)))
    size, offset = M.dfs_offsets(t)
    assert offset[:n].tolist() == list(range(n))


CUBES = {k: np.array([10 * k, 0, 0, 10 * k + k + 1, k + 1, k + 1], f32) for k in range(4)}       # cube k: edge k + 1 at x = 10 k; surface 3 (k + 1)^2


@pytest.mark.parametrize("order", list(itertools.permutations(range(4))))
def test_four_boxes_in_a_row_in_every_order(order):
    """Four cubes of edge 1, 2, 3, 4 as the instances 0..3 of a TLAS, in all 24 leaf orders.  Whatever binary tree the order gives, the root
    opens until it holds all four, and the slots go larger surface first: instance 3, 2, 1, 0."""
    n = 4
    tree = M.ploc(np.stack([CUBES[k] for k in order]))
    tree.instance = np.array(list(order) + [0] * (n - 1))
    out, _ = M.emit(tree, *M.collapse(tree, 1, True)[:3])
    assert out.shape == (1, 16)
    assert out[0, 12:].view(np.int32).tolist() == [~3, ~2, ~1, ~0]
    # the root box is 0..34 x 0..4 x 0..4: 34 / 255 = 0.133 -> scale 1/4 on x; 4 / 255 = 0.0157 -> 1/32 on y and z (255 / 64 < 4)
    assert out.view(f32)[0, [0, 1, 2, 3, 10, 11]].tolist() == [0.0, 0.0, 0.0, 0.25, 0.03125, 0.03125]
    word = lambda bytes4: sum(b << (8 * k) for k, b in enumerate(bytes4))
    assert out[0, 4:10].tolist() == [word([120, 80, 40, 0]), word([136, 92, 48, 4]),            # x: lo = 40 k, hi = 40 k + 4 (k + 1)
                                     0, word([128, 96, 64, 32]), 0, word([128, 96, 64, 32])]   # y, z: lo = 0, hi = 32 (k + 1)


def test_four_boxes_as_a_blas_by_hand():
    """The same cubes in the order 0 1 2 3 as a BLAS with leaf_max = 1.  Merged surfaces: (0,1) 52, (1,2) 87, (2,3) 128, (0,2) 147, (1,3) 208,
    (0,3) 288.  Round 1: 0 <-> 1 are mutual (2 wants 1, 3 wants 2): node 4 = (0, 1).  Round 2 over [4, 2, 3]: (4,2) 147, (2,3) 128, (4,3) 288:
    2 <-> 3: node 5 = (2, 3).  Round 3: node 6 = (4, 5).  Depth first the leaves are 0 1 2 3.  The root opens node 5 first (surface 128
    against 52): [4, 2, 3], then node 4 in place: [0, 2, 3, 1]; sorted by surface: 3, 2, 1, 0, each a leaf of one record at its offset."""
    tree = M.ploc(np.stack([CUBES[k] for k in range(4)]))
    assert tree.left.tolist() == [0, 2, 4] and tree.right.tolist() == [1, 3, 5]
    out = M.build_blas(np.stack([CUBES[k] for k in range(4)]), np.arange(4), 1)
    assert out["prim"].tolist() == [0, 1, 2, 3] and out["root"] == 0
    assert out["nodes"][0, 12:].view(np.int32).tolist() == [~(3 << 3), ~(2 << 3), ~(1 << 3), ~0]


def test_the_quantiser_by_hand():
    """origin 1, extent 255 exactly: frexp(255 / 255) has the mantissa 0.5, so the scale is 1, not 2; planes land on the integers.
    An extent of zero takes 2^-126; an extent that overflows an infinite scale and bytes 0."""
    node = np.array([1, 0, -3.0e38, 256, 0, 3.0e38], f32)
    kids = np.zeros((4, 6), f32)
    kids[:, 0], kids[:, 3] = [1, 1.5, 100, 255.5], [1, 2.5, 101, 256]
    kids[:, 2], kids[:, 5] = -3.0e38, 3.0e38
    scale, lo, hi, doublings = M.quantise(node, kids, np.array([True, True, True, False]))
    assert scale.tolist() == [1.0, float(M.TINY), np.inf]
    assert lo[:, 0].tolist() == [0, 0, 99, 255] and hi[:, 0].tolist() == [0, 2, 100, 0]
    assert lo[:, 1].tolist() == [0, 0, 0, 255] and hi[:, 1].tolist() == [0, 0, 0, 0]
    assert not lo[:, 2].any() and not hi[:, 2].any() and doublings.tolist() == [0, 0, -1]


def test_first_difference_names_node_slot_and_field():
    a = np.zeros((3, 16), np.uint32)
    b = a.copy()
    assert M.first_difference(a, b) is None
    b[2, 7] = 5 << 16
    assert M.first_difference(a, b) == "node 2, slot 2, hi.y bytes: 0, the model has 5"
    b[1, 13] = 7
    assert M.first_difference(a, b).startswith("node 1, slot 1, code: 0, the model has 7")
    assert "nodes" in M.first_difference(a[:2], b)
