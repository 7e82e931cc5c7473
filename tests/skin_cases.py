"""Skins, palettes and the numpy restatement shared by tests/test_model_skin_abi.py (CPU) and tests/test_gpu_model_skin.py: the definition of
DESIGN.md section 2 "Skinned vertices" (include/dxr_amd.h, "Skeletal animation") in fp32, in the stated order -- written from that text, not
from the kernel -- and the case generators: palettes, the weight families, rest poses."""
import os
import re

import numpy as np

from dxrexperiments_amd import rtypes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("one_hot", "convex", "zeros", "wild", "nan_inf", "neg_zero")


def lds_bones():
    """RT_SKIN_LDS_BONES as dxrexperiments_amd/csrc/rt_skin.h defines it"""
    text = open(os.path.join(ROOT, "dxrexperiments_amd", "csrc", "rt_skin.h")).read()
    return int(re.search(r"^#define RT_SKIN_LDS_BONES (\d+)u?\s*$", text, flags=re.M).group(1))


def skinned(rest, bones_idx, weights, palette):
    """rest T.VERTEX[V], bones_idx [V, K], weights float32[V, K], palette float32[n_bones, 12] -> T.VERTEX[V].  Every operation is one fp32
    operation on fp32 operands (numpy's float32 arrays round each product and each sum, and fuse nothing), in the order of the definition,
    entry by entry and slot by slot; only the vertices are taken together."""
    rest = np.ascontiguousarray(rest, T.VERTEX)
    idx = np.asarray(bones_idx).reshape(len(rest), -1)
    w = np.asarray(weights, np.float32).reshape(idx.shape)
    pal = np.asarray(palette, np.float32).reshape(-1, 12)
    assert idx.max() < len(pal)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        B = []
        for e in range(12):                                # blend: B[e] = w[0] M[0][e]; then B[e] = B[e] + w[k] M[k][e], every slot
            b = w[:, 0] * pal[idx[:, 0], e]
            for k in range(1, idx.shape[1]):
                b = b + w[:, k] * pal[idx[:, k], e]
            B.append(b)
        out = np.zeros(len(rest), T.VERTEX)
        x, y, z = (np.ascontiguousarray(rest["position"][:, c]) for c in range(3))
        nx, ny, nz = (np.ascontiguousarray(rest["normal"][:, c]) for c in range(3))
        s = []
        for r in range(3):
            out["position"][:, r] = ((B[4 * r] * x + B[4 * r + 1] * y) + B[4 * r + 2] * z) + B[4 * r + 3]
            s.append((B[4 * r] * nx + B[4 * r + 1] * ny) + B[4 * r + 2] * nz)
        d = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
        ok = (d > 0) & np.isfinite(d)
        inv = one / np.sqrt(d)
        for r in range(3):
            out["normal"][:, r] = np.where(ok, s[r] * inv, np.float32(0.0))
    for a in B + s + [d, inv]:
        assert a.dtype == np.float32
    return out


def rotations(n, rng):
    """n proper rotations (float64), uniformly enough: QR of a Gaussian matrix, the determinant made +1"""
    out = np.empty((n, 3, 3))
    for k in range(n):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out[k] = q
    return out


def random_palette(n_bones, seed, spread=1.0):
    """rotations x uniform scales 0.5 .. 1.5 + translations of up to `spread` per axis: float32[n_bones, 12]"""
    rng = np.random.default_rng(seed)
    m = np.zeros((n_bones, 3, 4))
    m[:, :, :3] = rotations(n_bones, rng) * rng.uniform(0.5, 1.5, (n_bones, 1, 1))
    m[:, :, 3] = rng.uniform(-spread, spread, (n_bones, 3))
    return m.reshape(n_bones, 12).astype(np.float32)


def gentle_palette(n_bones, seed, angle=0.5, spread=0.3):
    """rotations by up to `angle` radians about random axes x scales 0.8 .. 1.25 + small translations: a pose that keeps a mesh in its
    neighbourhood (for scenes and frames)"""
    rng = np.random.default_rng(seed)
    m = np.zeros((n_bones, 3, 4))
    for b in range(n_bones):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        a = rng.uniform(-angle, angle)
        k = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
        m[b, :, :3] = (np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * (k @ k)) * rng.uniform(0.8, 1.25)
    m[:, :, 3] = rng.uniform(-spread, spread, (n_bones, 3))
    return m.reshape(n_bones, 12).astype(np.float32)


def identity_palette(n_bones):
    return np.tile(np.asarray(T.IDENTITY_3X4, np.float32).reshape(1, 12), (n_bones, 1))


def random_bones(n_verts, k, n_bones, seed):
    """uint32[V, K], any bone in any slot (a bone may repeat within a vertex); the largest index is in use"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, n_bones, (n_verts, k)).astype(np.uint32)
    b[rng.integers(0, n_verts), rng.integers(0, k)] = n_bones - 1
    return b


def random_weights(n_verts, k, seed, family="convex"):
    """float32[V, K].  one_hot: one slot 1, the others 0; convex: non-negative, summing to 1 up to rounding; zeros: convex with exact zeros
    (+0 and -0) in about a third of the slots; wild: -2 .. 2, summing to anything"""
    rng = np.random.default_rng(seed)
    if family == "one_hot":
        w = np.zeros((n_verts, k), np.float32)
        w[np.arange(n_verts), rng.integers(0, k, n_verts)] = 1.0
        return w
    if family == "wild":
        return rng.uniform(-2.0, 2.0, (n_verts, k)).astype(np.float32)
    w = rng.uniform(0.05, 1.0, (n_verts, k))
    if family == "zeros":
        w[rng.uniform(size=w.shape) < 0.33] = 0.0
        w[:, 0] += (w.sum(axis=1) == 0)                     # (no vertex without any weight)
    w = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    if family == "zeros":
        w[(w == 0) & (rng.uniform(size=w.shape) < 0.5)] = -0.0
    return w


def rest_pose(n_verts, seed, neg_zero=False):
    """(T.VERTEX[V], indices[n, 3]): random positions in a box of extent 2, random unit normals; neg_zero: about a quarter of the rest
    coordinates, positions and normals, are -0 (and some +0)"""
    rng = np.random.default_rng(seed)
    v = np.zeros(n_verts, T.VERTEX)
    v["position"] = rng.uniform(-2, 2, (n_verts, 3)).astype(np.float32)
    n = rng.normal(size=(n_verts, 3))
    v["normal"] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    if neg_zero:
        for field in ("position", "normal"):
            u = rng.uniform(size=(n_verts, 3))
            v[field][u < 0.25] = -0.0
            v[field][u > 0.9] = 0.0
    idx = np.array([[t, (t + 1) % n_verts, (t + 2) % n_verts] for t in range(max(1, n_verts // 3))], np.uint32)
    return v, idx


def case(family, n_verts, k, n_bones, seed):
    """(rest, indices, bones, weights, palette) of one of FAMILIES.  nan_inf: convex weights, one NaN and one inf entry in the palette, in
    bones and entries that are in use (a translation entry and an entry of the linear part); neg_zero: a rest pose with -0 coordinates"""
    rest, idx = rest_pose(n_verts, seed, neg_zero=family == "neg_zero")
    bones = random_bones(n_verts, k, n_bones, seed + 1)
    weights = random_weights(n_verts, k, seed + 2, family if family in ("one_hot", "convex", "zeros", "wild") else "convex")
    palette = random_palette(n_bones, seed + 3)
    if family == "nan_inf":
        palette[bones[0, 0], 3] = np.nan
        palette[bones[-1, -1], 5] = np.inf
    return rest, idx, bones, weights, palette


def pack(bones, weights):
    """the layout rt_skin.h packs a skin into: slot major, 16-bit indices"""
    return np.ascontiguousarray(np.asarray(bones).T.astype(np.uint16)), np.ascontiguousarray(np.asarray(weights, np.float32).T)


def canonical_nans(a):
    """float32 array with every NaN replaced by one NaN: sign and payload of a NaN that an operation produces are what IEEE 754 leaves to
    the hardware (x86 gives the negative default NaN, the GPU the positive one); WHERE a NaN stands is not"""
    out = np.array(a, np.float32, copy=True)
    out[np.isnan(out)] = np.float32(np.nan)
    return out
