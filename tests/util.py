"""Shared helpers for the parity tests: scene construction on both sides, ray sets."""
import os

import numpy as np

from dxrexperiments_amd import rtypes as T
from dxrexperiments_amd import scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CORNELL_OBJ = os.path.join(GOLDEN, "cornell.obj")

CULL = T.RAY_FLAG_CULL_BACK_FACING_TRIANGLES
ANY = T.RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH | T.RAY_FLAG_SKIP_CLOSEST_HIT_SHADER


def rng(seed):
    return np.random.default_rng(seed)


def triangle_soup(n, seed, extent=10.0, size=0.6):
    """n random triangles (own vertices, flat normals)."""
    r = rng(seed)
    c = r.uniform(-extent, extent, (n, 1, 3))
    p = (c + r.uniform(-size, size, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    v = np.zeros(3 * n, T.VERTEX)
    v["position"] = p
    fn = np.cross(p[1::3] - p[0::3], p[2::3] - p[0::3])
    l = np.linalg.norm(fn, axis=1, keepdims=True)
    l[l == 0] = 1
    v["normal"] = np.repeat((fn / l).astype(np.float32), 3, axis=0)
    return v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def sliver_soup(n, seed, extent=4.0):
    """n long thin triangles in random directions (length 0.5 ... 2 x extent, width 1/30 ... 1/3000 of it) among n small ones: what the
    builder holds as several references each (rt_refs.h)."""
    r = rng(seed)
    c = r.uniform(-extent, extent, (n, 3))
    d = r.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    w = np.cross(d, r.normal(size=(n, 3))); w /= np.linalg.norm(w, axis=1, keepdims=True)
    L = r.uniform(0.5, 2.0, n) * extent
    wd = L / np.exp(r.uniform(np.log(30.0), np.log(3000.0), n))
    p = np.stack([c - 0.5 * L[:, None] * d, c + 0.5 * L[:, None] * d, c + r.uniform(-0.5, 0.5, n)[:, None] * L[:, None] * d + wd[:, None] * w], 1)
    sv, si = triangle_soup(n, seed + 1, extent=extent, size=0.3)
    pos = np.concatenate([np.clip(p, -1.5 * extent, 1.5 * extent).reshape(-1, 3).astype(np.float32), sv["position"]])
    v = np.zeros(pos.shape[0], T.VERTEX)
    v["position"] = pos
    fn = np.cross(pos[1::3] - pos[0::3], pos[2::3] - pos[0::3])
    l = np.linalg.norm(fn, axis=1, keepdims=True)
    l[l == 0] = 1
    v["normal"] = np.repeat((fn / l).astype(np.float32), 3, axis=0)
    return v, np.arange(pos.shape[0], dtype=np.uint32).reshape(-1, 3)


def random_xforms(n, seed, spread=8.0):
    r = rng(seed)
    out = np.zeros((n, 12), np.float32)
    for i in range(n):
        a, b, c = r.uniform(0, 2 * np.pi, 3)
        rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
        s = np.diag(r.uniform(0.5, 1.5, 3))
        m = np.zeros((3, 4))
        m[:, :3] = rz @ ry @ rx @ s
        m[:, 3] = r.uniform(-spread, spread, 3)
        out[i] = m.astype(np.float32).reshape(12)
    return out


HARD_FAMILIES = ("mirror", "stretch", "squash", "shear", "small", "large", "far")       # ... whose distance from geometry is bounded (s2_truth.py)
FAR_SHIFT = (40000.0, -25000.0, 30000.0)


def hard_xforms(family, n, seed):
    """Instance transforms random_xforms never makes: random_xforms(n, seed, spread=6) changed in float64, returned as fp32 [n, 12].
    mirror (negative determinant), stretch / squash (1000:1 anisotropy either way), shear, small / large (uniform scale 1e-4 / 1e4, the
    latter with its translation), far (translation 4 - 5 orders above the mesh's size), extreme (linear part x 1e12, 1e-12, 1e20, 1e-20 in
    turn: the adjugate or the determinant leaves fp32's range) and degenerate (index k takes case k % 5: a zero column, a zero linear
    part, one NaN entry, one +inf translation entry, two equal rows)."""
    m = random_xforms(n, seed, spread=6.0).astype(np.float64).reshape(n, 3, 4)
    L, t = m[:, :, :3], m[:, :, 3]
    with np.errstate(over="ignore"):
        if family == "mirror":
            L[:, :, 0] = -L[:, :, 0]
        elif family == "stretch":
            L[:] = L @ np.diag([1000.0, 1.0, 1.0])
        elif family == "squash":
            L[:] = L @ np.diag([1.0, 1e-3, 1.0])
        elif family == "shear":
            L[:] = L @ np.array([[1.0, 30.0, 0.0], [0.0, 1.0, -20.0], [0.0, 0.0, 1.0]])
        elif family == "small":
            L *= 1e-4
        elif family == "large":
            L *= 1e4
            t *= 1e4
        elif family == "far":
            t += np.array(FAR_SHIFT)
        elif family == "extreme":
            for k in range(n):
                L[k] *= (1e12, 1e-12, 1e20, 1e-20)[k % 4]
        elif family == "degenerate":
            for k in range(n):
                case = k % 5
                if case == 0:
                    L[k, :, 1] = 0.0
                elif case == 1:
                    L[k] = 0.0
                elif case == 2:
                    L[k, 1, 2] = np.nan
                elif case == 3:
                    t[k, 2] = np.inf
                else:
                    L[k, 2] = L[k, 0]
        else:
            raise KeyError(family)
        return m.reshape(n, 12).astype(np.float32)


def world_box_of_vertices(v, idx, m):
    """the definition (oracle_bvh.h scene_build): the box of the triangles' transformed vertices, x' = ((m0 x + m1 y) + m2 z) + m3 in fp32,
    by min / max that start from the empty box and pass over a NaN"""
    p = v["position"][np.asarray(idx).reshape(-1)].astype(np.float32)
    m = np.asarray(m, np.float32).reshape(3, 4)
    with np.errstate(all="ignore"):
        w = np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], axis=1)
    inf = np.float32(np.inf)
    return np.concatenate([np.fmin.reduce(w, axis=0, initial=inf), np.fmax.reduce(w, axis=0, initial=-inf)])


class Pair:
    """The same scene on the oracle and on the GPU."""

    def __init__(self, oracle, capi, ctx, models, instances):
        """models: list of (verts, idx), or of file paths the PRODUCT ingests (rt_model_create_from_file: .obj / .fbx) -- the
        oracle then gets the arrays the product read; instances: list of (model_index, xform or None)."""
        self.o = oracle.Scene()
        self.g = capi.Scene(ctx)
        self.gmodels = []
        for m in models:
            if isinstance(m, str):
                gm = capi.Model(ctx, path=m)
                v, i = gm.geometry()
            else:
                v, i = m
                gm = capi.Model(ctx, v, i)
            self.o.add_model(v, i)
            self.gmodels.append(gm)
        for mi, x in instances:
            self.o.add_instance(mi, x)
            self.g.add_model(self.gmodels[mi], x)
        self.o.build()
        self.g.build()
        self.n_instances = len(instances)


def random_rays(n, seed, lo, hi, tmin=0.0, tmax=1e38):
    """Rays with origins in a box grown around [lo,hi] aimed at random points inside it."""
    r = rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    o = c + r.uniform(-1.6, 1.6, (n, 3)) * e
    t = c + r.uniform(-1.0, 1.0, (n, 3)) * e
    d = t - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    O = np.zeros((n, 4), np.float32); D = np.zeros((n, 4), np.float32)
    O[:, :3] = o; O[:, 3] = tmin
    D[:, :3] = d; D[:, 3] = tmax
    return O, D


def primary_rays(pf, W, H):
    """RayGen's ray set-up in numpy fp32 (same operation order as the kernels)."""
    cp = pf["cameraParams"]
    f = np.float32
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    dx = ((xs + f(0.5)) / f(W)) * f(2.0) - f(1.0)
    dy = ((ys + f(0.5)) / f(H)) * f(2.0) - f(1.0)
    d = dx[..., None] * cp["U"][:3] + (-dy)[..., None] * cp["V"][:3]
    d = d + cp["W"][:3]
    dot = d[..., 0] * d[..., 0]
    dot = dot + d[..., 1] * d[..., 1]
    dot = dot + d[..., 2] * d[..., 2]
    d = d * (f(1.0) / np.sqrt(dot))[..., None]
    n = W * H
    o = np.zeros((n, 4), np.float32)
    j = cp["jitters"] * f(30.0)
    o[:, 0] = cp["worldEyePos"][0] + j[0]
    o[:, 1] = cp["worldEyePos"][1] + j[1]
    o[:, 2] = cp["worldEyePos"][2] + f(0.0)
    dd = np.zeros((n, 4), np.float32)
    dd[:, :3] = d.reshape(-1, 3)
    dd[:, 3] = f(1.0e38)
    return o, dd


def assert_hits_equal(a, b, what="", closest=True):
    """Bit-exact comparison of two hit dictionaries (miss t = -1 on both sides)."""
    hit_a = a["inst"] != T.RT_NO_HIT
    hit_b = b["inst"] != T.RT_NO_HIT
    assert np.array_equal(hit_a, hit_b), "%s: hit/miss differs on %d rays" % (what, int((hit_a != hit_b).sum()))
    if not closest:
        return
    for k in ("inst", "prim"):
        bad = np.nonzero(a[k] != b[k])[0]
        assert bad.size == 0, "%s: %s differs on %d rays, first %d: %s vs %s" % (what, k, bad.size, bad[0], a[k][bad[0]], b[k][bad[0]])
    for k in ("t", "u", "v"):
        x, y = a[k][hit_a], b[k][hit_a]
        bad = np.nonzero(x.view(np.uint32) != y.view(np.uint32))[0]
        bad = bad[x[bad] != y[bad]]        # +0 / -0 compare equal
        assert bad.size == 0, "%s: %s differs on %d rays (first: %r vs %r)" % (what, k, bad.size, x[bad[0]], y[bad[0]])


def nodes_equal(a, b):
    """Canonical node arrays equal (floats by value so that -0 == +0)."""
    return (np.array_equal(a["left"], b["left"]) and np.array_equal(a["right"], b["right"])
            and np.array_equal(a["bmin"], b["bmin"]) and np.array_equal(a["bmax"], b["bmax"]))


def cam_array(cam, aspect):
    return np.array([*cam["eye"], *cam["at"], *cam["up"], cam["fov"], aspect], np.float32)


REFERENCE_ASSETS = os.path.join(GOLDEN, "reference_assets")


def reference_asset(name, directory):
    """The reference checkout's asset file `name` as tests/golden/make_reference_copies.py stored it: the committed copy of a mesh
    (cornell.obj, susanne.obj, ground.fbx), or a cube map written out into `directory` -- CathedralIrradiance.dds byte for byte;
    CathedralRadiance.dds with its own header and level 0 (what the readers return) and levels 1 - 6, which the readers skip,
    made again by a 2x2 box filter (the file's layout and size are the original's)."""
    import lzma
    if not name.endswith(".dds"):
        return os.path.join(REFERENCE_ASSETS, name)
    path = os.path.join(str(directory), name)
    if name == "CathedralIrradiance.dds":
        with open(os.path.join(REFERENCE_ASSETS, name + ".xz"), "rb") as f:
            data = lzma.decompress(f.read())
    else:
        with open(os.path.join(REFERENCE_ASSETS, "CathedralRadiance.mip0.xz"), "rb") as f:
            raw = lzma.decompress(f.read())
        header, body = raw[:148], np.frombuffer(raw, np.uint8, offset=148)
        size, mips = int(np.frombuffer(header, np.uint32, 1, 12)[0]), int(np.frombuffer(header, np.uint32, 1, 28)[0])
        delta = np.stack([body[:body.size // 2], body[body.size // 2:]], 1).copy().view(np.uint16).reshape(3, 6, size, size)
        planes = np.cumsum(delta, axis=-1, dtype=np.uint16)                       # (wraps mod 2^16 as the deltas did)
        level = np.full((6, size, size, 4), 0x3C00, np.uint16)
        level[..., :3] = np.moveaxis(planes, 0, 3)
        faces = [[level[f]] for f in range(6)]
        lv = level.view(np.float16).astype(np.float32)
        for m in range(1, mips):
            lv = 0.25 * (lv[:, 0::2, 0::2] + lv[:, 1::2, 0::2] + lv[:, 0::2, 1::2] + lv[:, 1::2, 1::2])
            for f in range(6):
                faces[f].append(lv[f].astype(np.float16).view(np.uint16))
        data = header + b"".join(m.tobytes() for face in faces for m in face)
    with open(path, "wb") as f:
        f.write(data)
    return path
