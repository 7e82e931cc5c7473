"""Binary FBX files with node hierarchies for the tests: a WRITER (tests/fbx_tools.py's record and property encoders, reused by
import) that emits Models with arbitrary Properties70, Model -> Model connections, non-mesh Models and several Geometry ->
Model connections, and an independent EVALUATOR (numpy float64, written from the FBX definition below, not from
dxrexperiments_amd/csrc/rt_fbx.cpp) that flattens such a file the way the reference's importer does
(aiProcess_PreTransformVertices, libs/DXRFramework/RtModel.cpp:26).

Per node:   L = T . Roff . Rp . Rpre . R . Rpost^-1 . Rp^-1 . Soff . Sp . S . Sp^-1
            (Lcl Translation, RotationOffset, RotationPivot, PreRotation, Lcl Rotation, PostRotation, ScalingOffset, ScalingPivot,
            Lcl Scaling; degrees; Rpre / Rpost in XYZ order = Rz.Ry.Rx; R by RotationOrder)
World     = L(root-most ancestor) . ... . L(parent) . L(node) over the "OO" Model -> Model connections
vertex    = World . G . v,  G = GT . GR . GS (GeometricTranslation / Rotation / Scaling, XYZ order) of the mesh's own Model only
normal    = inverse transpose of the linear part of World . G, normalised
A Geometry connected to k Models is emitted k times, in Connections order; Geometry objects in file order."""
import struct

import numpy as np

import fbx_tools as F

VECTORS = ("Lcl Translation", "Lcl Rotation", "Lcl Scaling", "PreRotation", "PostRotation", "RotationPivot", "ScalingPivot", "RotationOffset",
           "ScalingOffset", "GeometricTranslation", "GeometricRotation", "GeometricScaling")
ENUMS = ("RotationOrder", "InheritType", "RotationActive")


# ---- writer -----------------------------------------------------------------------------------------------------

def _geometry(gid, m):
    pvi = []
    for poly in m["polygons"]:
        pvi += list(poly[:-1]) + [~int(poly[-1])]
    ln = [("Version", [101], []), ("Name", [b""], []), ("MappingInformationType", [m.get("mapping", "ByPolygonVertex").encode()], []),
          ("ReferenceInformationType", [b"Direct"], []), ("Normals", [np.asarray(m["normals"], np.float64).reshape(-1)], [])]
    return ("Geometry", [gid, b"\x00\x01Geometry", b"Mesh"],
            [("Vertices", [np.asarray(m["positions"], np.float64).reshape(-1)], []), ("PolygonVertexIndex", [np.asarray(pvi, np.int32)], []),
             ("LayerElementNormal", [0], ln)])


def _p70(props):
    out = []
    for key, val in props.items():
        if key in ENUMS:
            out.append(("P", [key.encode(), b"enum", b"", b"", int(val)], []))
        else:
            assert key in VECTORS, key
            out.append(("P", [key.encode(), key.encode(), b"", b"A"] + [float(x) for x in val], []))
    return out


def gid(k):
    return 1000 + k


def mid(k):
    return 200000 + k


def write(path, geoms, models, version=7500, compress=True):
    """geoms: mesh dicts as fbx_tools.write takes them (positions, polygons, normals, mapping); geometry k gets id gid(k).
    models: dicts with  cls     "Mesh", "Null", "LimbNode", ... (the Model's class string),
                        parent  index of the parent Model, None for the scene root, or a list of indices (several parents: hostile),
                        geoms   indices of the geometries connected to it, in this order,
                        props   {Properties70 name: 3 floats, or an int for RotationOrder / InheritType}.
    Connections are written Model by Model in list order, a Model's own parent connection(s) first, then its geometries."""
    wide = version >= 7500
    objs = [_geometry(gid(k), g) for k, g in enumerate(geoms)]
    conns = []
    for k, m in enumerate(models):
        cls = m.get("cls", "Mesh")
        objs.append(("Model", [mid(k), b"Node%d\x00\x01Model" % k, cls.encode()], [("Version", [232], []), ("Properties70", [], _p70(m.get("props", {})))]))
        parents = m.get("parent")
        for p in (parents if isinstance(parents, (list, tuple)) else [parents]):
            conns.append(("C", [b"OO", mid(k), 0 if p is None else mid(p)], []))
        for g in m.get("geoms", ()):
            conns.append(("C", [b"OO", gid(g), mid(k)], []))
    top = [("FBXHeaderExtension", [], [("FBXVersion", [version], [])]), ("Objects", [], objs), ("Connections", [], conns)]
    out = b"Kaydara FBX Binary  \x00\x1a\x00" + struct.pack("<I", version)
    for t in top:
        out += F._record(t[0], t[1], t[2], len(out), wide, compress)
    out += b"\0" * (25 if wide else 13)
    with open(path, "wb") as f:
        f.write(out)


def combine(*scenes):
    """Several (geoms, models) scenes in one file: indices rebased, order kept."""
    geoms, models = [], []
    for g, m in scenes:
        go, mo = len(geoms), len(models)
        geoms += g
        for x in m:
            y = dict(x, geoms=[go + k for k in x.get("geoms", ())])
            if y.get("parent") is not None:
                y["parent"] = mo + y["parent"]
            models.append(y)
    return geoms, models


# ---- independent evaluator --------------------------------------------------------------------------------------

def _axis(axis, deg):
    a = np.radians(np.float64(deg))
    c, s = np.cos(a), np.sin(a)
    return {0: np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), 1: np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            2: np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


# RotationOrder -> the axes of the product, leftmost factor first ("XYZ": X is applied first, so it stands rightmost)
ORDERS = {0: (2, 1, 0), 1: (1, 2, 0), 2: (0, 2, 1), 3: (2, 0, 1), 4: (1, 0, 2), 5: (0, 1, 2)}


def _rot(deg, order=0):
    a, b, c = ORDERS[order]
    return _h(_axis(a, deg[a]) @ _axis(b, deg[b]) @ _axis(c, deg[c]))


def _h(lin=None, t=None):
    M = np.eye(4)
    if lin is not None:
        M[:3, :3] = lin
    if t is not None:
        M[:3, 3] = t
    return M


def _values(model):
    v = {k: np.zeros(3) for k in VECTORS}
    v["Lcl Scaling"] = np.ones(3)
    v["GeometricScaling"] = np.ones(3)
    v["RotationOrder"] = 0
    p70 = F._kid(model, "Properties70")
    for p in (p70["kids"] if p70 else []):
        key = p["props"][0].decode()
        if key in VECTORS:
            v[key] = np.array(p["props"][4:7], np.float64)
        elif key in ENUMS:
            v[key] = int(p["props"][4])
    return v


def local_matrix(v):
    T, Roff, Rp, Soff, Sp = (_h(t=v[k]) for k in ("Lcl Translation", "RotationOffset", "RotationPivot", "ScalingOffset", "ScalingPivot"))
    Rpre, Rpost, R = _rot(v["PreRotation"]), _rot(v["PostRotation"]), _rot(v["Lcl Rotation"], v["RotationOrder"])
    S = _h(np.diag(v["Lcl Scaling"]))
    inv = np.linalg.inv
    return T @ Roff @ Rp @ Rpre @ R @ inv(Rpost) @ inv(Rp) @ Soff @ Sp @ S @ inv(Sp)


def geometric_matrix(v):
    return _h(t=v["GeometricTranslation"]) @ _rot(v["GeometricRotation"]) @ _h(np.diag(v["GeometricScaling"]))


def evaluate(path):
    """(pos+normal float32[n, 6], uint32[m, 3]): the file flattened by the formulas in this module's docstring, with
    fbx_tools.ingest's corner, joining and normal rules (polygons fanned from their first corner, one vertex per distinct
    (position index, float32 normal value) per emitted mesh in first-use order)."""
    _, top = F.parse(path)
    objects = next(n for n in top if n["name"] == "Objects")
    conns = next(n for n in top if n["name"] == "Connections")
    models = {m["props"][0]: _values(m) for m in objects["kids"] if m["name"] == "Model"}
    parent, owners = {}, {}
    for c in conns["kids"]:
        if c["name"] != "C" or c["props"][0] != b"OO" or c["props"][2] not in models:
            continue
        child, par = c["props"][1], c["props"][2]
        if child in models:
            assert child not in parent, "the evaluator takes well-formed hierarchies only"
            parent[child] = par
        else:
            owners.setdefault(child, []).append(par)

    def world(m):
        M, k = local_matrix(models[m]), parent.get(m)
        while k is not None:
            M = local_matrix(models[k]) @ M
            k = parent.get(k)
        return M

    verts, idx = [], []
    for g in objects["kids"]:
        if g["name"] != "Geometry" or g["props"][2] != b"Mesh":
            continue
        P = np.asarray(F._kid(g, "Vertices")["props"][0], np.float64).reshape(-1, 3)
        pv = np.asarray(F._kid(g, "PolygonVertexIndex")["props"][0], np.int64)
        ln = F._kid(g, "LayerElementNormal")
        N = np.asarray(F._kid(ln, "Normals")["props"][0], np.float64).reshape(-1, 3)
        by_pv = F._kid(ln, "MappingInformationType")["props"][0] == b"ByPolygonVertex"
        assert F._kid(ln, "ReferenceInformationType")["props"][0] == b"Direct"
        corners, poly = [], []
        for k, v in enumerate(pv):
            last = v < 0
            poly.append((int(~v if last else v), k))
            if last:
                for j in range(1, len(poly) - 1):
                    corners += [poly[0], poly[j], poly[j + 1]]
                poly = []
        for m in owners.get(g["props"][0], [None]):
            M = np.eye(4) if m is None else world(m) @ geometric_matrix(models[m])
            Pw = P @ M[:3, :3].T + M[:3, 3]
            it = np.linalg.inv(M[:3, :3]).T
            seen = {}
            for p, k in corners:
                n = it @ N[k if by_pv else p]
                n32 = (n / np.linalg.norm(n)).astype(np.float32)
                key = (p, n32.tobytes())
                if key not in seen:
                    seen[key] = len(verts)
                    verts.append(np.concatenate([Pw[p].astype(np.float32), n32]))
                idx.append(seen[key])
    return np.array(verts, np.float32).reshape(-1, 6), np.array(idx, np.uint32).reshape(-1, 3)


# ---- the cases of tests/test_fbx_hierarchy.py (shared with the sanitizer and GPU tests) -------------------------

def box(offset=(0.0, 0.0, 0.0), size=(1.0, 0.75, 0.5)):
    """A box of 6 quads = 12 triangles with per-polygon-vertex normals: each face's normal bent a little towards its corner, so that
    a vertex's three corners keep three different normals and a non-uniform scaling shows in them."""
    s = np.asarray(size, np.float64)
    P = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64) * s + np.asarray(offset, np.float64)
    quads = [[0, 2, 3, 1], [4, 5, 7, 6], [0, 1, 5, 4], [2, 6, 7, 3], [0, 4, 6, 2], [1, 3, 7, 5]]
    N = []
    for q in quads:
        fn = np.cross(P[q[1]] - P[q[0]], P[q[2]] - P[q[0]])
        fn /= np.linalg.norm(fn)
        c = P[q].mean(axis=0)
        for k in q:
            n = fn + 0.25 * (P[k] - c) / np.linalg.norm(P[k] - c)
            N.append(n / np.linalg.norm(n))
    return dict(positions=P, polygons=quads, normals=np.array(N))


def cases():
    """name -> (geoms, models), the hierarchies (a) ... (h); coordinates stay O(1 - 10)."""
    c = {}
    c["a_three_levels"] = ([box()], [
        dict(cls="Null", parent=None, props={"PreRotation": (-90.0, 0.0, 0.0), "InheritType": 1}),
        dict(cls="Null", parent=0, props={"Lcl Translation": (1.5, -2.0, 0.75), "Lcl Scaling": (2.0, 0.5, 1.25), "InheritType": 1}),
        dict(parent=1, geoms=[0], props={"Lcl Rotation": (30.0, -45.0, 10.0), "InheritType": 1})])
    c["b_pivots_and_offsets"] = ([box()], [
        dict(parent=None, geoms=[0], props={"Lcl Translation": (0.5, 1.0, -1.5), "Lcl Rotation": (20.0, 35.0, -50.0), "Lcl Scaling": (1.5, 0.75, 2.0),
                                            "RotationPivot": (0.5, -1.0, 0.25), "ScalingPivot": (-0.75, 0.5, 1.0), "RotationOffset": (0.25, 0.5, -0.5),
                                            "ScalingOffset": (1.0, -0.25, 0.5)})])
    c["c_post_rotation"] = ([box()], [
        dict(parent=None, geoms=[0], props={"Lcl Translation": (1.0, 2.0, 3.0), "Lcl Rotation": (15.0, 25.0, 35.0), "PostRotation": (40.0, -20.0, 70.0),
                                            "PreRotation": (0.0, 90.0, 0.0), "Lcl Scaling": (1.0, 2.0, 0.5)})])
    for order in range(6):
        c["d_rotation_order_%d" % order] = ([box()], [
            dict(parent=None, geoms=[0], props={"RotationOrder": order, "Lcl Rotation": (25.0, -40.0, 65.0), "Lcl Translation": (0.5, 0.25, -1.0),
                                                "Lcl Scaling": (1.25, 1.0, 0.75)})])
    c["e_geometric_not_inherited"] = ([box(), box(offset=(0.5, 0.0, 0.0), size=(0.5, 0.5, 0.5))], [
        dict(parent=None, geoms=[0], props={"Lcl Translation": (2.0, 0.0, 0.0), "Lcl Rotation": (0.0, 30.0, 0.0), "GeometricTranslation": (0.0, 1.5, 0.0),
                                            "GeometricRotation": (45.0, 10.0, -30.0), "GeometricScaling": (0.5, 2.0, 1.5)}),
        dict(parent=0, geoms=[1], props={"Lcl Translation": (0.0, 0.0, 3.0), "Lcl Scaling": (1.0, 1.5, 1.0)})])
    c["f_null_in_chain"] = ([box()], [
        dict(parent=None, cls="Mesh", props={"Lcl Translation": (1.0, 0.0, 0.0)}),
        dict(parent=0, cls="Null", props={"Lcl Rotation": (0.0, 0.0, 90.0), "Lcl Scaling": (2.0, 2.0, 2.0)}),
        dict(parent=1, cls="LimbNode", props={"Lcl Translation": (0.0, 1.0, 0.0), "PreRotation": (10.0, 20.0, 30.0)}),
        dict(parent=2, geoms=[0], props={"Lcl Translation": (0.0, 0.0, 1.0)})])
    c["g_instanced_geometry"] = ([box()], [
        dict(parent=None, geoms=[0], props={"Lcl Translation": (-3.0, 0.5, 0.0), "Lcl Rotation": (0.0, 20.0, 0.0)}),
        dict(parent=None, geoms=[0], props={"Lcl Translation": (3.0, 1.0, 0.5), "Lcl Scaling": (0.5, 1.5, 1.0), "PreRotation": (-90.0, 0.0, 0.0)})])
    for inherit in (0, 2):
        c["h_inherit_type_%d" % inherit] = ([box()], [
            dict(parent=None, cls="Null", props={"Lcl Rotation": (10.0, 50.0, -20.0), "Lcl Translation": (1.0, 1.0, 1.0), "InheritType": inherit}),
            dict(parent=0, geoms=[0], props={"Lcl Scaling": (2.0, 1.0, 0.5), "Lcl Rotation": (-35.0, 15.0, 5.0), "InheritType": inherit})])
    return c
