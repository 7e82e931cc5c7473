"""Morph targets, weights and the numpy restatement shared by tests/test_model_morph_abi.py (CPU) and tests/test_gpu_model_morph.py: the
definition of DESIGN.md section 2 "Morphed vertices" (include/dxr_amd.h, "Morph targets") in fp32, in the stated order -- written from that
text, not from the kernel --, the SELL-64 packing of dxrexperiments_amd/csrc/rt_morph.h restated, and the case generators: run shapes, the
weight families, bases."""
import numpy as np

import skin_cases as K
from dxrexperiments_amd import rtypes as T

ROOT = K.ROOT
FAMILIES = ("one_hot", "convex", "zeros", "wild", "nan_inf")
SHAPES = ("dense", "sparse", "gap", "spike")
MAX_TARGETS = 65536
canonical_nans = K.canonical_nans


def morphed(base, offsets, indices, dpos, dnrm, weights):
    """base T.VERTEX[V], offsets [n_targets + 1], indices [E], dpos float32[E, 3], dnrm float32[E, 3] or None, weights float32[n_targets]
    -> T.VERTEX[V].  Every operation is one fp32 operation on fp32 operands (numpy's float32 arrays round each product and each sum, and
    fuse nothing).  The targets are visited in ascending order, so every vertex sees its entries in ascending target order; a target names
    a vertex at most once, so the vertices of one target are taken together.  A target without entries has nothing to evaluate; a target
    with entries is evaluated whatever its weight."""
    base = np.ascontiguousarray(base, T.VERTEX)
    off = np.asarray(offsets, np.int64).reshape(-1)
    idx = np.asarray(indices, np.int64).reshape(-1)
    dp = np.asarray(dpos, np.float32).reshape(-1, 3)
    dn = None if dnrm is None else np.asarray(dnrm, np.float32).reshape(-1, 3)
    w = np.asarray(weights, np.float32).reshape(-1)
    assert len(w) == len(off) - 1 and off[0] == 0 and off[-1] == len(idx) == len(dp)
    p = base["position"].copy()
    s = base["normal"].copy()
    named = np.zeros(len(base), bool)
    with np.errstate(all="ignore"):
        for t in np.flatnonzero(off[1:] > off[:-1]):
            e = slice(off[t], off[t + 1])
            v = idx[e]
            assert (np.diff(v) > 0).all() and v[-1] < len(base)
            named[v] = True
            for c in range(3):
                p[v, c] = p[v, c] + (w[t] * dp[e, c])
                if dn is not None:
                    s[v, c] = s[v, c] + (w[t] * dn[e, c])
        out = base.copy()                                   # a vertex that no target names: its base record, bit for bit
        out["position"][named] = p[named]
        if dn is not None:
            d = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
            ok = (d > 0) & np.isfinite(d)
            inv = np.float32(1.0) / np.sqrt(d)
            assert d.dtype == inv.dtype == np.float32
            for c in range(3):
                out["normal"][named, c] = np.where(ok, s[:, c] * inv, np.float32(0.0))[named]
    assert p.dtype == s.dtype == np.float32
    return out


def pack(n_verts, offsets, indices, dpos, dnrm):
    """the layout rt_morph.h packs targets into: (count uint32[V], slice_cell uint32[S + 1], target uint16[cells], dpos float32[3 cells],
    dnrm float32[3 cells] or None).  The j-th entry of vertex v in ascending target order sits in cell slice_cell[v >> 6] + 64 j + (v & 63);
    unused cells hold target 0 and +0 deltas."""
    off = np.asarray(offsets, np.int64).reshape(-1)
    idx = np.asarray(indices, np.int64).reshape(-1)
    dp = np.asarray(dpos, np.float32).reshape(-1, 3)
    count = np.bincount(idx, minlength=n_verts).astype(np.uint32)
    slices = (n_verts + 63) // 64
    padded = np.zeros(slices * 64, np.uint32)
    padded[:n_verts] = count
    slice_cell = np.zeros(slices + 1, np.uint32)
    slice_cell[1:] = np.cumsum(64 * padded.reshape(slices, 64).max(axis=1).astype(np.int64))
    cells = int(slice_cell[-1])
    # the entries in (vertex, target) order: the target-major list, sorted by vertex, stably; j = the place within the vertex's run
    of_target = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order = np.argsort(idx, kind="stable")
    v = idx[order]
    first = np.zeros(n_verts + 1, np.int64)
    first[1:] = np.cumsum(count)
    j = np.arange(len(v)) - first[v]
    cell = slice_cell[v >> 6].astype(np.int64) + 64 * j + (v & 63)
    assert len(np.unique(cell)) == len(cell) and (len(cell) == 0 or cell.max() < cells)
    target = np.zeros(cells, np.uint16)
    target[cell] = of_target[order]
    out_dp = np.zeros((cells, 3), np.float32)
    out_dp.view(np.uint32)[cell] = dp.view(np.uint32)[order]                   # (bit for bit)
    out_dn = None
    if dnrm is not None:
        out_dn = np.zeros((cells, 3), np.float32)
        out_dn.view(np.uint32)[cell] = np.asarray(dnrm, np.float32).reshape(-1, 3).view(np.uint32)[order]
    return count, slice_cell, target, out_dp.reshape(-1), None if out_dn is None else out_dn.reshape(-1)


def runs(shape, n_verts, n_active, seed):
    """the sorted vertex lists of n_active targets.  dense: every target lists every vertex; sparse: about a third of the vertices each,
    a quarter of the vertices named by nobody, and with three targets or more the last but one empty; gap: about half of the vertices
    each but none of 64 .. 127, a slice of width 0 (between two others from 129 vertices on); spike: every target names the middle vertex
    and nothing else"""
    rng = np.random.default_rng(seed)
    every = np.arange(n_verts, dtype=np.uint32)
    if shape == "dense":
        return [every.copy() for _ in range(n_active)]
    if shape == "spike":
        return [np.array([n_verts // 2], np.uint32) for _ in range(n_active)]
    out = []
    nobody = rng.uniform(size=n_verts) < 0.25
    for t in range(n_active):
        if shape == "sparse":
            take = (rng.uniform(size=n_verts) < 0.33) & ~nobody
            if n_active >= 3 and t == n_active - 2:
                take[:] = False
        else:
            take = (rng.uniform(size=n_verts) < 0.5) & ((every < 64) | (every >= 128))
        out.append(every[take])
    if shape == "sparse" and not any(len(r) for r in out):
        out[0] = every[:1].copy()
    return out


def targets(lists, n_targets=None, seed=0, normals=True, scale=0.5):
    """(offsets, indices, dpos, dnrm or None, active) of the vertex lists.  n_targets == MAX_TARGETS: three lists at the most, which become
    targets 0, 1 and 65535, every other target empty"""
    rng = np.random.default_rng(seed)
    n_targets = len(lists) if n_targets is None else n_targets
    if n_targets == len(lists):
        active = list(range(n_targets))
    else:
        assert n_targets == MAX_TARGETS and len(lists) <= 3
        active = [0, 1, MAX_TARGETS - 1][3 - len(lists):] if len(lists) < 3 else [0, 1, MAX_TARGETS - 1]
    sizes = np.zeros(n_targets, np.int64)
    sizes[active] = [len(r) for r in lists]
    offsets = np.zeros(n_targets + 1, np.uint32)
    offsets[1:] = np.cumsum(sizes)
    indices = np.concatenate([np.asarray(r, np.uint32) for r in lists]) if lists else np.zeros(0, np.uint32)
    dpos = rng.uniform(-scale, scale, (len(indices), 3)).astype(np.float32)
    dnrm = rng.uniform(-scale, scale, (len(indices), 3)).astype(np.float32) if normals else None
    return offsets, indices, dpos, dnrm, active


def weights(n_targets, family, seed, active=None):
    """float32[n_targets].  one_hot: one target in use 1, the others 0; convex: non-negative, summing to 1 up to rounding; zeros: convex
    with exact zeros (+0 and -0) in about a third of the targets; wild: -2 .. 2; nan_inf: convex with a NaN at the first target in use and
    an inf at the last (if that is another)"""
    rng = np.random.default_rng(seed)
    active = list(range(n_targets)) if active is None else active
    if family == "one_hot":
        w = np.zeros(n_targets, np.float32)
        w[active[rng.integers(0, len(active))]] = 1.0
        return w
    if family == "wild":
        return rng.uniform(-2.0, 2.0, n_targets).astype(np.float32)
    w = rng.uniform(0.05, 1.0, n_targets)
    if family == "zeros":
        w[rng.uniform(size=n_targets) < 0.33] = 0.0
        w[active[0]] += w[active].sum() == 0               # (no division by zero)
    w = (w / w[active].sum()).astype(np.float32)
    if family == "zeros":
        w[(w == 0) & (rng.uniform(size=n_targets) < 0.5)] = -0.0
    if family == "nan_inf":
        w[active[0]] = np.nan
        if active[-1] != active[0]:
            w[active[-1]] = np.inf
    return w


def base(n_verts, seed):
    """(T.VERTEX[V], indices[n, 3]): skin_cases.rest_pose with -0 (and +0) coordinates among positions and normals"""
    return K.rest_pose(n_verts, seed, neg_zero=True)


def case(shape, family, n_verts, n_targets, seed, normals=True):
    """(base, triangle indices, offsets, vertex indices, dpos, dnrm, weights, active targets)"""
    b, tri = base(n_verts, seed)
    lists = runs(shape, n_verts, min(n_targets, 3) if n_targets == MAX_TARGETS else n_targets, seed + 1)
    off, idx, dp, dn, active = targets(lists, n_targets, seed + 2, normals)
    return b, tri, off, idx, dp, dn, weights(n_targets, family, seed + 3, active), active


def signed_zero_case(normals):
    """130 vertices, three targets, weights (+0, +0, 1.5).  Vertex 5: a base of -0 throughout, named by targets 0 and 1 with positive
    deltas -- its only weights are +0, and -0 + (+0 * d) is +0.  Vertex 6: a base of -0, named by nobody -- it stays -0, unless the padding
    of its slice (three cells wide because of vertex 7, which every target names) is evaluated: -0 + (w[0] * +0) would be +0."""
    b, tri = base(130, 11)
    for v in (5, 6):
        b["position"][v] = -0.0
        b["normal"][v] = -0.0
    lists = [np.array([5, 7, 100], np.uint32), np.array([5, 7], np.uint32), np.array([7, 129], np.uint32)]
    off, idx, dp, dn, _ = targets(lists, None, 12, normals)
    dp[:] = np.abs(dp) + np.float32(0.125)
    if dn is not None:
        dn[:] = np.abs(dn) + np.float32(0.125)
    return b, tri, off, idx, dp, dn, np.array([0.0, 0.0, 1.5], np.float32)
