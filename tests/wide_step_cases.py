"""The enumerated inputs of tests/test_wide_step_edges.py (CPU: the model of oracle/wide_step_model.h against the canonical box test) and
tests/test_gpu_wide_step.py (GPU: rt_debug_wide_step against the model): four-wide nodes and (node, ray) items placed where one step of
the traversal engine (csrc/rt_wide_step.h) decides -- at the threshold of the box test, at the steep threshold, at the floor of the margin.

The independent side is the canonical test: slab() of oracle/oracle_bvh.h (pyoracle.slab_batch) on the planes
fma(byte, scale, origin) that tests/wide_tree.py decodes.  Everything is deterministic (seeded); `python tests/wide_step_cases.py --write`
measures the looseness of family (a) and writes tests/golden/wide_step_bounds.json.

A SWEEP is one ray of which one float (an origin coordinate; in family (c) a direction component) is stepped ulp by ulp, HALF ulps either
side of the point where a verdict on one child flips; the flip is found by bisection over the float's ordinal, between a value at which
the verdict is "kept" and one at which it is "culled" (the bracket, from the geometry in float64)."""
import json
import os
import sys

import numpy as np

import wide_tree as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_step_bounds.json")
NONE, EMPTY = -2 ** 31, 0x7FFFFFFE
HALF = 64                       # ulps either side of the canonical threshold
HALF_MODEL = 4                  # ... of the model's own threshold
SLACK = 1.0 + 2.0 ** -16
BIG = np.float32(3.0e38)
# brackets tried, as relative distances from the threshold computed in float64: the kept side first in the middle of the band that the slack
# leaves a box without extent (a point, a flat box: kept only while all its planes are within 2^-16 of one another), then farther out
KEEP_WIDTHS = (2.0 ** -17, 2.0 ** -11, 2.0 ** -7, 2.0 ** -3, 0.75, 0.75, 0.75)
WIDTHS = (2.0 ** -11, 2.0 ** -11, 2.0 ** -7, 2.0 ** -3, 0.75, 8.0, 64.0)


def make_node(origin, scale, lo, hi, codes):
    """one 64-B record (include/dxr_amd.h): origin[3], scale[3], lo / hi bytes [4 children][3 axes], codes[4]"""
    w = np.zeros(16, np.uint32)
    f = w.view(np.float32)
    f[0:3] = origin
    f[3], f[10], f[11] = scale
    lo = np.asarray(lo, np.uint32).reshape(4, 3)
    hi = np.asarray(hi, np.uint32).reshape(4, 3)
    for a, (wl, wh) in enumerate(((4, 5), (6, 7), (8, 9))):
        w[wl] = sum(int(lo[k, a]) << (8 * k) for k in range(4))
        w[wh] = sum(int(hi[k, a]) << (8 * k) for k in range(4))
    w[12:16] = np.asarray(codes, np.int64).astype(np.int32).view(np.uint32)
    return w


def ordinal(x):
    """float32 -> int64, monotone in the value (-0 and +0 share 0)"""
    b = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def from_ordinal(o):
    o = np.asarray(o, np.int64)
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(np.float32)


def canonical(oracle, dec, index, O, D):
    """the canonical verdict of every slot: bool[n, 4] (unused slots included: what their bytes decode to)"""
    out = np.empty((index.size, 4), bool)
    for k in range(4):
        out[:, k] = oracle.slab_batch(O, D, dec["lo"][index, k], dec["hi"][index, k])[0]
    return out


def truth64(dec, index, O, D):
    """the same test on the same decoded planes in float64 with the same slack: bool[n, 4]"""
    with np.errstate(all="ignore"):
        o = O[:, None, :3].astype(np.float64)
        inv = 1.0 / D[:, None, :3].astype(np.float64)
        a = (dec["lo"][index].astype(np.float64) - o) * inv
        b = (dec["hi"][index].astype(np.float64) - o) * inv
        lo = np.fmax(np.fmax.reduce(np.fmin(a, b), axis=2), O[:, None, 3].astype(np.float64))
        hi = np.fmin(np.fmin.reduce(np.fmax(a, b), axis=2), D[:, None, 3].astype(np.float64))
        return lo <= hi * SLACK


class Specs:
    """sweeps to be placed: node, child, the ray (8 floats: origin tmin direction tbest), the swept float's column, and per bracket width a
    value at which the child is kept and one at which it is culled"""

    def __init__(self):
        self.node, self.child, self.row, self.coord, self.keep, self.cull, self.labels = [], [], [], [], [], [], []

    def add(self, node, child, row, coord, keep, cull, labels):
        self.node.append(node); self.child.append(child); self.row.append(np.asarray(row, np.float32)); self.coord.append(coord)
        self.keep.append(np.asarray(keep, np.float32)); self.cull.append(np.asarray(cull, np.float32)); self.labels.append(tuple(labels))

    def graze(self, dec, node, k, a, b, d, binding, t0, labels):
        """a ray along d (float32[3], no zero on a or b) that enters child k through its near plane on axis a as it leaves through the
        far plane on axis b, at distance t0; binding: which pair decides -- 'planes' (near plane a against far plane b), 'tbest' (near
        plane a against the far end of the window), 'tmin' (the near end of the window against far plane b)"""
        with np.errstate(all="ignore"):
            L, H = dec["lo"][node, k].astype(np.float64), dec["hi"][node, k].astype(np.float64)
            d = np.asarray(d, np.float32)
            dd = d.astype(np.float64)
            near, far = np.where(dd > 0, L, H), np.where(dd > 0, H, L)
            P = 0.5 * (L + H)
            P = np.where(np.isfinite(P), P, dec["origin"][node].astype(np.float64))
            if not (np.isfinite(near[a]) and np.isfinite(far[b])):
                return
            tmin, tbest = 0.0, float(BIG)
            if binding != "tmin":
                P[a] = near[a]
            if binding != "tbest":
                P[b] = far[b]
            if binding == "tbest":
                tbest = t0
            if binding == "tmin":
                tmin = t0 * SLACK
            o = P - t0 * dd
            o = np.where(dd == 0, P, o)
            row = np.array([o[0], o[1], o[2], tmin, d[0], d[1], d[2], tbest], np.float64)
            if binding == "tmin":       # kept while far plane b is beyond t0
                keep = [far[b] - t0 * (1 + w) * dd[b] for w in KEEP_WIDTHS]
                cull = [far[b] - t0 * (1 - w) * dd[b] for w in WIDTHS]            # (beyond w = 1: the plane is behind the origin)
                coord = b
            else:                        # kept while near plane a is before t0 (1 + 2^-16)
                keep = [near[a] - t0 * SLACK * (1 - w) * dd[a] for w in KEEP_WIDTHS]
                cull = [near[a] - t0 * SLACK * (1 + w) * dd[a] for w in WIDTHS]
                coord = a
            if not (np.all(np.isfinite(row[:7])) and np.all(np.abs(row[:3]) < 1e37)):
                return
            self.add(node, k, row, coord, keep, cull, labels)


def place_sweeps(specs, verdict, half):
    """-> dict(index, O, D, sweep (id per item), labels (per sweep), child (per sweep)): the sweeps of `specs` whose bracket the verdict
    function (node[m], child[m], O[m, 4], D[m, 4]) -> bool[m] confirms, HALF ulps either side of the flip"""
    m = len(specs.node)
    node, child = np.array(specs.node, np.int32), np.array(specs.child, np.int64)
    rows, coord = np.stack(specs.row), np.array(specs.coord, np.int64)
    keep, cull = np.stack(specs.keep), np.stack(specs.cull)
    ar = np.arange(m)

    def at(x):
        r = rows.copy()
        r[ar, coord] = from_ordinal(x)
        return verdict(node, child, np.ascontiguousarray(r[:, :4]), np.ascontiguousarray(r[:, 4:]))

    a, b, ok = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, bool)
    for w in range(keep.shape[1]):
        ka, cb = ordinal(keep[:, w]), ordinal(cull[:, w])
        good = at(ka) & ~at(cb) & ~ok
        a, b, ok = np.where(good, ka, a), np.where(good, cb, b), ok | good
    for _ in range(34):
        mid = (a + b) >> 1
        h = at(mid)
        a, b = np.where(h, mid, a), np.where(h, b, mid)
    sel = np.nonzero(ok)[0]
    steps = np.arange(-half, half + 1, dtype=np.int64)
    x = from_ordinal(np.clip(a[sel, None] + steps[None, :], -0x7F7FFFFF, 0x7F7FFFFF))           # [s, 2 half + 1]
    r = np.repeat(rows[sel], steps.size, axis=0)
    r[np.arange(r.shape[0]), np.repeat(coord[sel], steps.size)] = x.reshape(-1)
    return dict(index=np.repeat(node[sel], steps.size), O=np.ascontiguousarray(r[:, :4]), D=np.ascontiguousarray(r[:, 4:]),
                sweep=np.repeat(np.arange(sel.size), steps.size), labels=[specs.labels[i] for i in sel], child=child[sel], placed=sel.size, asked=m)


def canonical_verdict(oracle, dec):
    return lambda node, child, O, D: oracle.slab_batch(O, D, dec["lo"][node, child], dec["hi"][node, child])[0]


def model_verdict(oracle, nodes):
    return lambda node, child, O, D: ((oracle.wide_step_model(nodes, node, O, D)["mask"] >> child) & 1) != 0


def decode(nodes):
    d = W.decode4(nodes)
    d["origin"] = nodes.view(np.float32)[:, 0:3].copy()
    return d


def random_children(r, flat_axis=None):
    lo = r.integers(0, 200, (4, 3))
    hi = lo + r.integers(1, 56, (4, 3))
    if flat_axis is not None:
        hi[:, flat_axis] = lo[:, flat_axis]
    return lo, hi


def octant_signs(octant):
    return np.array([-1.0 if octant >> a & 1 else 1.0 for a in range(3)], np.float32)


AXIS_PAIRS = ((0, 1), (1, 2), (2, 0), (1, 0), (2, 1), (0, 2))
A_ORIGINS = (0.0, 4000.0, -4000.0, 1.0e6, -1.0e6)
A_SCALES = (-126, -20, -4, 3, 100)


def graze_specs_for(dec, node_ids, r, specs, labels_of, per_node, far_of=None):
    """family (a) against the children of the nodes node_ids: per node `per_node` sweeps that go round the octants, the three bindings,
    near and far origins, the ordered axis pairs and the used children"""
    for ni in node_ids:
        used = np.nonzero(dec["code"][ni] != NONE)[0]
        for j in range(per_node):
            octant, binding, far = j % 8, ("planes", "tmin", "tbest")[(j // 8) % 3], (j // 24) % 2
            k = int(used[(j + ni) % used.size])
            a, b = AXIS_PAIRS[(j + j // 6 + ni) % 6]
            d = octant_signs(octant) * r.uniform(0.35, 1.0, 3).astype(np.float32)
            with np.errstate(all="ignore"):
                ext = dec["hi"][ni, k].astype(np.float64) - dec["lo"][ni, k].astype(np.float64)
            ext = float(np.nanmax(np.where(np.isfinite(ext), ext, 0.0)))
            # (a box that its node's origin all but swallows -- a point in float32 -- is seen from a distance at which a ray's own rounding
            # is small against 2^-16, not from a few of its extents away)
            far_off = float(np.abs(dec["origin"][ni]).max())
            ext = max(0.25 * far_off if ext < 2.0 ** -12 * far_off else ext, 1.0e-37)
            t0 = ext * r.uniform(0.5, 3.0)
            if far:
                t0 = max(float(r.choice((far_of(ni) if far_of else None) or [1.0e3, 1.0e5, 1.0e7])), ext * float(r.choice([1.0e1, 1.0e3])))
            specs.graze(dec, ni, k, a, b, d, binding, t0, labels_of(ni) + ("oct%d" % octant, binding, "far" if far else "near"))


def family_a_nodes(r):
    nodes, tags = [], []
    for og in A_ORIGINS:
        for e in A_SCALES:
            lo, hi = random_children(r)
            origin = np.float32(og) * (1 + r.uniform(0, 1e-3, 3)).astype(np.float32)
            codes = [len(nodes) * 4 + k + 1 for k in range(4)]
            nodes.append(make_node(origin, [np.float32(2.0) ** e] * 3, lo, hi, codes))
            tags.append(("origin%g" % abs(og), "scale2^%d" % e))
    return np.stack(nodes), tags


def build(oracle):
    """-> dict(nodes uint32[N, 16], families {name: dict(index, O, D, ...)})"""
    r = np.random.default_rng(20261)
    fam = {}
    nodes_a, tags = family_a_nodes(r)
    all_nodes = [nodes_a]

    # ---- (a) threshold sweeps, and the same rays at the model's own threshold --------------------------------------------------------
    dec = decode(nodes_a)
    sp = Specs()
    # (far origins of the smallest nodes at the origin: where 1e-37 is about an ulp of the distances -- nearer it is a margin of its own,
    # farther it is nothing and the step's arithmetic is the canonical test's, bit for bit -- and far as everywhere else)
    graze_specs_for(dec, range(nodes_a.shape[0]), r, sp, lambda ni: tags[ni], 48,
                    far_of=lambda ni: [1.0e-31, 1.0e-30, 3.0e-30, 1.0e-29, 1.0e3] if tags[ni] == ("origin0", "scale2^-126") else None)
    fam["a"] = place_sweeps(sp, canonical_verdict(oracle, dec), HALF)
    fam["a_model_edge"] = place_sweeps(sp, model_verdict(oracle, nodes_a), HALF_MODEL)
    n_nodes = nodes_a.shape[0]

    def new_family(name, nodes, items):
        nonlocal n_nodes
        items["index"] = (items["index"] + n_nodes).astype(np.int32)
        all_nodes.append(nodes)
        n_nodes += nodes.shape[0]
        fam[name] = items

    # ---- (b) both sides of the steep threshold: |1 / d| at 65536, the nearest reciprocals either side, 1e5, 1e9, on one to three axes; a zero
    #      component (+0, -0: reciprocal +-inf) with the origin stepped across the planes of that axis ---------------------------------
    nb = np.stack([make_node([0.25, -0.5, 0.125], [np.float32(2.0) ** -4] * 3, *random_children(r), [11, 12, 13, 14]),
                   make_node([4000.0, -2500.0, 3000.0], [np.float32(2.0) ** -2] * 3, *random_children(r), [21, 22, 23, 24])])
    decb = decode(nb)
    sp = Specs()
    tiny16 = np.float32(2.0 ** -16)
    steep_d = (("at65536", tiny16), ("above", np.nextafter(tiny16, np.float32(0))), ("below", np.nextafter(tiny16, np.float32(1))),
               ("1e5", np.float32(1e-5)), ("1e9", np.float32(1e-9)))
    j = 0
    for ni in range(2):
        for name, val in steep_d:
            for nsteep in (1, 2, 3):
                for rep in range(3):
                    octant, binding = (j * 5 + rep) % 8, ("planes", "tmin", "tbest")[rep % 3]
                    a, b = AXIS_PAIRS[(j + rep) % 6]
                    mag = r.uniform(0.35, 1.0, 3).astype(np.float32)
                    for s in range(nsteep):
                        mag[(a + s) % 3 if rep % 2 else (b + s) % 3] = val
                    ext = float((decb["hi"][ni, rep % 4] - decb["lo"][ni, rep % 4]).max())
                    sp.graze(decb, ni, rep % 4, a, b, octant_signs(octant) * mag, binding, ext * r.uniform(0.5, 3.0) / float(mag.min()) * 0.35,
                             (name, "steep%d" % nsteep))
                    j += 1
        for zero in (np.float32(0.0), np.float32(-0.0)):
            for nzero in (1, 2, 3):
                for rep in range(6):
                    k, c = rep % 4, rep % 3
                    d = octant_signs(rep % 8) * r.uniform(0.35, 1.0, 3).astype(np.float32)
                    for s in range(nzero):
                        d[(c + s) % 3] = zero
                    L, H = decb["lo"][ni, k].astype(np.float64), decb["hi"][ni, k].astype(np.float64)
                    P = L + (H - L) * r.uniform(0.2, 0.8, 3)
                    o = np.where(d == 0, P, P - 0.7 * d.astype(np.float64))
                    plane, out = (L[c], L[c] - (H[c] - L[c])) if rep % 2 else (H[c], H[c] + (H[c] - L[c]))
                    sp.add(ni, k, [o[0], o[1], o[2], 0.0, d[0], d[1], d[2], float(BIG)], c, [P[c]] * len(WIDTHS), [out] * len(WIDTHS),
                           ("zero" if not np.signbit(zero) else "negzero", "steep%d" % nzero))
    new_family("b", nb, place_sweeps(sp, canonical_verdict(oracle, decb), HALF))

    # ---- (c) the floor of the margin: node origin 0, the smallest scale, ray origin 0 or denormal, and a direction component stepped across
    #      the threshold; direction lengths from 1 to 10^5 (nothing normalises a ray's direction) ------------------------------------------
    nc = np.stack([make_node([0, 0, 0], [np.float32(2.0) ** -126] * 3, *random_children(r), [31 + 4 * i, 32 + 4 * i, 33 + 4 * i, 34 + 4 * i]) for i in range(4)])
    decc = decode(nc)
    sp = Specs()
    for ni in range(4):
        for rep in range(24):
            k = rep % 4
            a, b = AXIS_PAIRS[rep % 6]
            c = 3 - a - b
            length = (1.0, 37.0, 1.0e3, 1.0e5)[(rep // 2) % 4]
            L, H = decc["lo"][ni, k].astype(np.float64), decc["hi"][ni, k].astype(np.float64)
            o = np.zeros(3)
            if rep % 2:
                o = r.integers(-40, 41, 3) * 2.0 ** -149
            da = length * r.uniform(0.35, 1.0)
            ta = (L[a] - o[a]) / da                                      # the ray goes (+,+,+) from the corner the node hangs on
            db = (H[b] - o[b]) * SLACK / ta                             # ... and leaves through far plane b where near plane a / (1 + 2^-16) is
            dc = 0.5 * (L[c] + H[c]) / ta
            if not (ta > 0 and np.isfinite(db) and db > 0 and dc > 0):
                continue
            sp.add(ni, k, [o[0], o[1], o[2], 0.0] + [[da, db, dc][[a, b, c].index(x)] for x in range(3)] + [float(BIG)], 4 + b,
                   [db * (1 - w) for w in KEEP_WIDTHS], [db * (1 + w) for w in WIDTHS], ("len%g" % length, "denormal" if rep % 2 else "zero"))
    new_family("c", nc, place_sweeps(sp, canonical_verdict(oracle, decc), HALF))

    # ---- (d) axes the builder could not quantise: scale +inf, bytes 0, on one to three axes ------------------------------------------------------
    nd = []
    for nq in (1, 2, 3):
        for first in range(3):
            lo, hi = random_children(r)
            scale = [np.float32(0.5)] * 3
            for s in range(nq):
                scale[(first + s) % 3] = np.float32(np.inf)
                lo[:, (first + s) % 3] = 0
                hi[:, (first + s) % 3] = 0
            nd.append(make_node([3.0, -7.0, 11.0], scale, lo, hi, [41 + 4 * len(nd) + k for k in range(4)]))
    nd = np.stack(nd)
    decd = decode(nd)
    sp = Specs()
    for ni in range(nd.shape[0]):
        fin = [a for a in range(3) if np.isfinite(decd["scale"][ni, a])]
        for rep in range(12):
            d = octant_signs(rep % 8) * r.uniform(0.35, 1.0, 3).astype(np.float32)
            if len(fin) == 2:
                a, b = fin if rep % 2 else fin[::-1]
                sp.graze(decd, ni, rep % 4, a, b, d, ("planes", "tmin", "tbest")[rep % 3], 40.0 * r.uniform(0.5, 3.0), ("unquantised1",))
            elif len(fin) == 1:
                a = fin[0]
                sp.graze(decd, ni, rep % 4, a, a, d, ("tmin", "tbest")[rep % 2], 40.0 * r.uniform(0.5, 3.0), ("unquantised2",))
    items = place_sweeps(sp, canonical_verdict(oracle, decd), HALF)
    # ... and rays of every kind at all of them: with three such axes only the window and the slot's use decide
    m = 64 * nd.shape[0]
    O = np.concatenate([r.uniform(-60, 60, (m, 3)), r.choice([0.0, 1.0, 5.0], (m, 1))], 1).astype(np.float32)
    D = np.concatenate([r.uniform(-1, 1, (m, 3)), r.choice([0.5, 1.0, 5.0, 5.00001, 1e30], (m, 1))], 1).astype(np.float32)
    items = dict(items, index=np.concatenate([items["index"], np.repeat(np.arange(nd.shape[0], dtype=np.int32), 64)]),
                 O=np.concatenate([items["O"], O]), D=np.concatenate([items["D"], D]))
    new_family("d", nd, items)

    # ---- (e) unused slots inside a node far smaller than the margin; duplicate children (equal entry distances); flat boxes ------------------
    ne = []
    for i, (og, e) in enumerate(((1000.0, -126), (0.5, -60), (-4000.0, -40))):
        for n_used in (2, 3):
            lo, hi = random_children(r)
            codes = [51 + 8 * len(ne) + k for k in range(4)]
            for k in range(n_used, 4):
                lo[k], hi[k], codes[k] = 255, 0, NONE
            ne.append(make_node([og, og * 0.5, -og], [np.float32(2.0) ** e] * 3, lo, hi, codes))
    n_micro = len(ne)
    for i in range(6):
        lo, hi = random_children(r)
        lo[[1, 3]], hi[[1, 3]] = lo[[0, 2]], hi[[0, 2]]                                    # slots 0 = 1 and 2 = 3: every distance comes twice
        if i >= 3:
            lo[:], hi[:] = lo[0], hi[0]                                                     # ... four times
        ne.append(make_node([1.0, 2.0, 3.0], [np.float32(0.125)] * 3, lo, hi, [51 + 8 * len(ne) + k for k in range(4)]))
    n_dup = len(ne)
    for axis in range(3):
        lo, hi = random_children(r, flat_axis=axis)
        ne.append(make_node([-3.0, 0.5, 2.0], [np.float32(0.0625)] * 3, lo, hi, [51 + 8 * len(ne) + k for k in range(4)]))
    ne = np.stack(ne)
    dece = decode(ne)
    sp = Specs()
    for ni in range(n_dup, ne.shape[0]):                                                   # flat boxes: grazing sweeps that enter / leave through the flat axis
        axis = ni - n_dup
        for rep in range(24):
            other = (axis + 1 + rep % 2) % 3
            a, b = (axis, other) if (rep // 2) % 2 else (other, axis)
            d = octant_signs(rep % 8) * r.uniform(0.35, 1.0, 3).astype(np.float32)
            sp.graze(dece, ni, rep % 4, a, b, d, ("planes", "tmin", "tbest")[rep % 3], r.uniform(0.5, 6.0), ("flat",))
    items = place_sweeps(sp, canonical_verdict(oracle, dece), HALF)
    # rays through and around the microscopic and the duplicate nodes: aimed at a point within a few ulps of the node
    m = 96 * n_dup
    idx = np.repeat(np.arange(n_dup, dtype=np.int32), 96)
    mid = np.where(np.isfinite(dece["lo"][idx, 0]), 0.5 * (dece["lo"][idx, 0].astype(np.float64) + dece["hi"][idx, 0]), 0.0)
    aim = from_ordinal(ordinal(mid.astype(np.float32)) + r.integers(-3, 4, (m, 3))).astype(np.float64)
    aim = np.where(idx[:, None] >= n_micro, mid + r.uniform(-0.6, 0.6, (m, 3)), aim)
    d = r.uniform(-1, 1, (m, 3))
    t0 = r.choice([0.5, 3.0, 100.0], (m, 1))
    O = np.concatenate([aim - t0 * d, np.zeros((m, 1))], 1).astype(np.float32)
    D = np.concatenate([d, np.full((m, 1), float(BIG))], 1).astype(np.float32)
    items = dict(items, index=np.concatenate([items["index"], idx]), O=np.concatenate([items["O"], O]), D=np.concatenate([items["D"], D]))
    new_family("e", ne, items)

    # ---- (f) NaN / inf in the ray, inverted windows, windows one ulp either side of empty ------------------------------------------------------
    nf = np.stack([make_node([0.0, 0.0, 0.0], [np.float32(0.25)] * 3, *random_children(r), [91, 92, 93, 94]),
                   make_node([4000.0, 1.0, -2.0], [np.float32(1.0)] * 3, *random_children(r), [95, 96, 97, 98])])
    decf = decode(nf)
    O, D, idx = [], [], []
    for ni in range(2):
        for rep in range(24):
            k = rep % 4
            P = 0.5 * (decf["lo"][ni, k].astype(np.float64) + decf["hi"][ni, k])
            d = octant_signs(rep % 8) * r.uniform(0.35, 1.0, 3)
            t0 = r.uniform(20.0, 90.0)
            row = np.array([*(P - t0 * d), 0.0, *d, float(BIG)], np.float32)
            rows = [row]
            for col in range(8):
                for v in (np.nan, np.inf, -np.inf):
                    x = row.copy(); x[col] = v; rows.append(x)
            for tmin, tbest in ((2.0 * t0, t0), (t0, 0.5 * t0), (t0, -1.0), (-1.0, -2.0), (np.inf, np.inf), (0.0, 0.0)):
                x = row.copy(); x[3], x[7] = tmin, tbest; rows.append(x)
            tb = np.float32(t0)
            edge = np.float32(tb * np.float32(SLACK))
            for s in range(-4, 5):                                                              # tmin around tbest * (1 + 2^-16): the window's own slack
                x = row.copy(); x[3], x[7] = from_ordinal(ordinal(edge) + s).reshape(-1)[0], tb; rows.append(x)
            O += [x[:4] for x in rows]; D += [x[4:] for x in rows]; idx += [ni] * len(rows)
    new_family("f", nf, dict(index=np.array(idx, np.int32), O=np.array(O, np.float32), D=np.array(D, np.float32)))

    # ---- the order of the hit children: four boxes in a row, in every assignment to the slots, rays from every octant, windows that end
    #      after one, two, three of them --------------------------------------------------------------------------------------------------
    import itertools
    ns, O, D, idx = [], [], [], []
    for perm in itertools.permutations(range(4)):
        lo = np.array([[10 + 60 * perm[k], 10 + 60 * perm[k], 10 + 60 * perm[k]] for k in range(4)])
        ns.append(make_node([-5.0, -5.0, -5.0], [np.float32(0.03125)] * 3, lo, lo + 40, [101 + 4 * len(ns) + k for k in range(4)]))
        for octant in range(8):
            s = octant_signs(octant).astype(np.float64)
            c = -5.0 + 0.03125 * 140.0                                                          # the middle of the row
            for cut in (0.9, 1.5, 2.6, 4.2, 1e30):
                O.append([*(c - s * 5.0), 0.0]); D.append([*s, cut * 0.03125 * 60.0 + 0.9]); idx.append(len(ns) - 1)
    new_family("order", np.stack(ns), dict(index=np.array(idx, np.int32), O=np.array(O, np.float32), D=np.array(D, np.float32)))

    return dict(nodes=np.concatenate(all_nodes), families=fam)


def evaluate(oracle, cases, **model_args):
    """per family: the canonical verdicts, the used slots and the model's answer"""
    nodes = cases["nodes"]
    dec = decode(nodes)
    out = {}
    for name, f in cases["families"].items():
        m = oracle.wide_step_model(nodes, f["index"], f["O"], f["D"], **model_args)
        out[name] = dict(model=m, kept=(m["mask"][:, None] >> np.arange(4)) & 1 != 0, used=dec["code"][f["index"]] != NONE,
                         canonical=canonical(oracle, dec, f["index"], f["O"], f["D"]))
    return out


def looseness(oracle, nodes, fam, **model_args):
    """(slots the model keeps although the float64 evaluation of the same decoded box rejects them, used slots tested)"""
    dec = decode(nodes)
    m = oracle.wide_step_model(nodes, fam["index"], fam["O"], fam["D"], **model_args)
    kept = (m["mask"][:, None] >> np.arange(4)) & 1 != 0
    used = dec["code"][fam["index"]] != NONE
    return int((kept & used & ~truth64(dec, fam["index"], fam["O"], fam["D"])).sum()), int(used.sum())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import pyoracle
    pyoracle.build()
    cases = build(pyoracle)
    loose, slots = looseness(pyoracle, cases["nodes"], cases["families"]["a"])
    doc = {"what": "family (a) of tests/wide_step_cases.py: used slots the step of oracle/wide_step_model.h (= csrc/rt_wide_step.h) keeps although the "
                   "float64 evaluation of the decoded box with the same slack rejects them; an upper bound held by tests/test_wide_step_edges.py; "
                   "written by python tests/wide_step_cases.py --write",
           "family_a": {"items": int(cases["families"]["a"]["index"].size), "slots": slots, "kept_but_rejected_in_float64": loose}}
    print(json.dumps(doc, indent=1))
    for name, f in cases["families"].items():
        print(name, f["index"].size, "items", f.get("placed"), "of", f.get("asked"), "sweeps placed")
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
