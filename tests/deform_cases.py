"""Meshes and the numpy restatements shared by tests/test_model_deform_abi.py (CPU) and tests/test_gpu_model_deform.py: the index lists
rt_model_recompute_normals' adjacency is held to, its CSR, and the normals of include/dxr_amd.h's definition in scalar fp32 order."""
import numpy as np

from dxrexperiments_amd import rtypes as T


def grid_mesh(side=9):
    """an indexed grid of side x side vertices over a gently curved sheet: valences 1 .. 6"""
    ys, xs = np.mgrid[0:side, 0:side]
    pos = np.stack([xs.ravel() * 0.25 - 1.0, 0.3 * np.sin(xs.ravel() * 0.7) * np.cos(ys.ravel() * 0.5), ys.ravel() * 0.25 - 1.0], axis=1).astype(np.float32)
    idx = []
    for y in range(side - 1):
        for x in range(side - 1):
            a = y * side + x
            idx += [[a, a + side, a + 1], [a + 1, a + side, a + side + 1]]
    v = np.zeros(side * side, T.VERTEX)
    v["position"] = pos
    v["normal"] = [0, 1, 0]
    return v, np.array(idx, np.uint32)


def index_lists():
    """name -> (n_verts, indices[n, 3]): the grid, a soup (valence 1), a vertex no triangle names, a triangle naming a vertex twice (and
    thrice), a fan, one triangle"""
    _, grid = grid_mesh()
    soup = np.arange(3 * 40, dtype=np.uint32).reshape(-1, 3)
    unnamed = np.array([[0, 1, 2], [2, 1, 4]], np.uint32)                       # vertex 3 of 6 and vertex 5: no triangle
    twice = np.array([[0, 1, 1], [2, 2, 2], [3, 0, 3], [0, 1, 2]], np.uint32)
    fan = np.array([[0, k, k + 1] for k in range(1, 7)], np.uint32)
    return {"grid": (81, grid), "soup": (120, soup), "unnamed": (6, unnamed), "twice": (4, twice), "fan": (8, fan),
            "one": (3, np.array([[0, 1, 2]], np.uint32))}


def csr_of(n_verts, idx):
    """the definition: the triangles naming v at any corner, ascending, each once"""
    runs = [[] for _ in range(n_verts)]
    for t, tri in enumerate(np.asarray(idx).reshape(-1, 3)):
        for v in sorted(set(int(x) for x in tri)):
            runs[v].append(t)
    off = np.zeros(n_verts + 1, np.uint32)
    off[1:] = np.cumsum([len(r) for r in runs])
    return off, np.array([t for r in runs for t in r], np.uint32)


def normals_of(pos, idx):
    """include/dxr_amd.h rt_model_recompute_normals, scalar fp32 in the stated order: s += cross(p1 - p0, p2 - p0) over the ascending
    triangles of v; d = ((x x) + y y) + z z; s * (1 / sqrt(d)) if 0 < d < inf else 0"""
    f = np.float32
    pos = np.asarray(pos, np.float32)
    idx = np.asarray(idx).reshape(-1, 3)
    off, tris = csr_of(len(pos), idx)
    out = np.zeros((len(pos), 3), np.float32)
    with np.errstate(all="ignore"):
        e1 = pos[idx[:, 1]] - pos[idx[:, 0]]
        e2 = pos[idx[:, 2]] - pos[idx[:, 0]]
        face = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]],
                        axis=1).astype(np.float32)     # (each product and each difference rounded to fp32: the arrays are fp32)
        for v in range(len(pos)):
            s = np.zeros(3, np.float32)
            for t in tris[off[v]:off[v + 1]]:
                s = s + face[t]
            d = f(s[0] * s[0])
            d = f(d + f(s[1] * s[1]))
            d = f(d + f(s[2] * s[2]))
            if d > 0 and np.isfinite(d):
                out[v] = s * f(f(1.0) / np.sqrt(d))
    return out


def displaced(verts, seed, amount=1.0, first=0):
    """the vertices from `first` on moved by up to `amount` per axis (seeded) and their normals turned over: another Morton order, other
    normal records"""
    r = np.random.default_rng(seed)
    out = verts.copy()
    n = len(verts) - first
    out["position"][first:] += r.uniform(-amount, amount, (n, 3)).astype(np.float32)
    out["normal"][first:] = -out["normal"][first:]
    return out


def slivers(verts, idx, step):
    """one vertex of every step-th triangle moved by (20, 17, 13): long diagonal slivers, held as several references each (rt_refs.h)"""
    out = verts.copy()
    t = np.arange(0, len(idx), step)
    out["position"][idx[t, 0]] += np.array([20, 17, 13], np.float32)
    return out
