"""Hierarchies, poses, clips and the numpy restatement shared by tests/test_skeleton_abi.py (CPU) and tests/test_gpu_skeleton.py: the
definition of DESIGN.md section 2 "Posed skeletons" (include/dxr_amd.h, "Posed skeletons") in fp32, in the stated order -- written from that
text, not from the kernel -- and the case generators: the hierarchy families, the pose families, clips."""
import os
import re

import numpy as np

from skin_cases import ROOT, canonical_nans  # noqa: F401  (canonical_nans: reused by the tests)

HIERARCHIES = ("forest", "chain", "star", "random", "roots")
POSES = ("unit", "raw", "mirror", "neg_zero", "nan_inf")
F = np.float32


def lds_joints():
    """RT_SKELETON_LDS_JOINTS as dxrexperiments_amd/csrc/rt_skeleton.h defines it"""
    text = open(os.path.join(ROOT, "dxrexperiments_amd", "csrc", "rt_skeleton.h")).read()
    return int(re.search(r"^#define RT_SKELETON_LDS_JOINTS (\d+)u?\s*$", text, flags=re.M).group(1))


# ---- the definition --------------------------------------------------------------------------------------------------------------------
def local_of(trs):
    """float32[n, 10] -> float32[n, 12]: L = T.R.S, the quaternion as given.  Every operation is one fp32 operation on fp32 operands."""
    p = np.ascontiguousarray(trs, F).reshape(-1, 10)
    t, s = p[:, 0:3], p[:, 7:10]
    x, y, z, w = (np.ascontiguousarray(p[:, 3 + c]) for c in range(4))
    one, two = F(1.0), F(2.0)
    with np.errstate(all="ignore"):
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        R = [[one - two * (yy + zz), two * (xy - wz), two * (xz + wy)],
             [two * (xy + wz), one - two * (xx + zz), two * (yz - wx)],
             [two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]]
        L = np.empty((len(p), 12), F)
        for r in range(3):
            for c in range(3):
                assert R[r][c].dtype == F
                L[:, 4 * r + c] = R[r][c] * s[:, c]
            L[:, 4 * r + 3] = t[:, r]
    return L


def compose(A, B):
    """C = A o B of float32[n, 12] 3x4 affine matrices, grouped as the header groups it"""
    A, B = np.asarray(A, F).reshape(-1, 12), np.asarray(B, F).reshape(-1, 12)
    C = np.empty(np.broadcast_shapes(A.shape, B.shape), F)
    with np.errstate(all="ignore"):
        for r in range(3):
            a0, a1, a2, a3 = (A[:, 4 * r + k] for k in range(4))
            for c in range(3):
                C[:, 4 * r + c] = (a0 * B[:, c] + a1 * B[:, 4 + c]) + a2 * B[:, 8 + c]
            C[:, 4 * r + 3] = ((a0 * B[:, 3] + a1 * B[:, 7]) + a2 * B[:, 11]) + a3
    return C


def levels_of(parents):
    """(order, level_offsets): the joints in level order, ascending by index within a level"""
    parents = np.asarray(parents, np.int64)
    level = np.zeros(len(parents), np.int64)
    for j in range(len(parents)):
        if parents[j] >= 0:
            level[j] = level[parents[j]] + 1
    order = np.argsort(level, kind="stable").astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(level))]).astype(np.uint32)
    return order, offsets


def posed(parents, inverse_bind, trs):
    """(W float32[n, 12], M float32[n, 12]): W_j = L_j for a root, else W_parent o L_j; M_j = W_j o inverse_bind_j.  Level by level: the
    recursion fixes the association, so the order of evaluation changes no bit."""
    parents = np.asarray(parents, np.int64)
    W = local_of(trs)                                    # (a root's W is its L, bit for bit)
    order, offsets = levels_of(parents)
    for l in range(1, len(offsets) - 1):
        js = order[offsets[l]:offsets[l + 1]].astype(np.int64)
        W[js] = compose(W[parents[js]], W[js])
    return W, compose(W, np.asarray(inverse_bind, F).reshape(-1, 12))


def segment(times, t):
    """(i, a) of the definition: fp32 differences, an fp32 quotient"""
    times = np.asarray(times, F)
    t = F(t)
    K = len(times)
    if K == 1 or t <= times[0]:
        return 0, F(0.0)
    if t >= times[-1]:
        return K - 2, F(1.0)
    i = int(np.searchsorted(times, t, side="right")) - 1
    return i, F(F(t - times[i]) / F(times[i + 1] - times[i]))


def sampled(times, keys, t):
    """the local pose float32[n, 10] of the clip (times float32[K], keys float32[K, n, 10]) at t"""
    keys = np.asarray(keys, F)
    i, a = segment(times, t)
    A = keys[i]
    B = (keys[i + 1] if len(keys) > 1 else keys[i]).copy()
    out = np.empty_like(A)
    with np.errstate(all="ignore"):
        d = ((A[:, 3] * B[:, 3] + A[:, 4] * B[:, 4]) + A[:, 5] * B[:, 5]) + A[:, 6] * B[:, 6]
        B[d < 0, 3:7] = -B[d < 0, 3:7]                   # (a NaN d compares false: nothing is negated)
        for c in range(10):
            out[:, c] = A[:, c] + (a * (B[:, c] - A[:, c]))
        q = out[:, 3:7].copy()
        n = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        ok = (n > 0) & np.isfinite(n)
        inv = F(1.0) / np.sqrt(n)
        assert d.dtype == n.dtype == inv.dtype == F
        for c in range(4):
            out[:, 3 + c] = np.where(ok, q[:, c] * inv, F(1.0 if c == 3 else 0.0))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def hierarchy(family, n, seed=0):
    """int32[n] parents.  forest: roots only; chain: j - 1; star: one root, every other joint its child; random: parent[j] uniform in
    [-1, j); roots: a random tree under each of several roots (every eighth joint is a root)"""
    rng = np.random.default_rng(seed)
    j = np.arange(n, dtype=np.int64)
    if family == "forest":
        p = np.full(n, -1)
    elif family == "chain":
        p = j - 1
    elif family == "star":
        p = np.where(j == 0, -1, 0)
    elif family == "random":
        p = np.floor(rng.uniform(size=n) * (j + 1)).astype(np.int64) - 1       # uniform in [-1, j)
        p = np.minimum(p, j - 1)
    elif family == "roots":
        p = np.floor(rng.uniform(size=n) * j).astype(np.int64)                 # uniform in [0, j) ...
        p = np.minimum(p, j - 1)
        p[::8] = -1                                                            # ... and every eighth a root
    else:
        raise ValueError(family)
    p[0] = -1
    return p.astype(np.int32)


def descendants(parents, joints):
    """bool[n]: the joints named and everything below them"""
    hit = np.zeros(len(parents), bool)
    hit[list(joints)] = True
    for j in range(len(parents)):
        if parents[j] >= 0 and hit[parents[j]]:
            hit[j] = True
    return hit


def with_children(parents):
    """the joints that are some joint's parent, ascending"""
    return np.unique(parents[parents >= 0])


def unit_quaternions(n, rng):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)


def pose(family, parents, seed):
    """float32[n, 10] of one of POSES.  unit: unit quaternions, scales 0.5 .. 1.5; raw: quaternions of lengths 0.8 .. 1.2, a fifth of them zero; mirror:
    negative and zero scales; neg_zero: -0 (and +0) in about a third of all components; nan_inf: a unit pose with one NaN (a translation) and
    one inf (a scale) in joints that have descendants, if the hierarchy has any -- else in joints 0 and n - 1"""
    n = len(parents)
    rng = np.random.default_rng(seed)
    p = np.empty((n, 10), F)
    p[:, 0:3] = rng.uniform(-1, 1, (n, 3))
    p[:, 3:7] = unit_quaternions(n, rng)
    p[:, 7:10] = rng.uniform(0.5, 1.5, (n, 3))
    if family == "raw":
        p[:, 3:7] *= rng.uniform(0.8, 1.2, (n, 1)).astype(F)     # (lengths about 1: a chain of a thousand such joints stays finite)
        p[rng.uniform(size=n) < 0.2, 3:7] = 0.0
        p[0, 3:7] = 0.0
    elif family == "mirror":
        p[:, 7:10] *= np.where(rng.uniform(size=(n, 3)) < 0.4, -1.0, 1.0).astype(F)
        p[:, 7:10][rng.uniform(size=(n, 3)) < 0.1] = 0.0
        p[0, 7], p[n - 1, 9] = -1.25, 0.0
    elif family == "neg_zero":
        u = rng.uniform(size=(n, 10))
        p[u < 0.25] = -0.0
        p[u > 0.92] = 0.0
        p[0, 0] = -0.0
    elif family == "nan_inf":
        inner = with_children(parents)
        a, b = (int(inner[0]), int(inner[-1])) if len(inner) else (0, n - 1)
        p[a, 1] = np.nan
        p[b, 8] = np.inf
    elif family != "unit":
        raise ValueError(family)
    return p


def poisoned(parents, family="nan_inf"):
    """the joints of pose("nan_inf", parents, ...) that hold the NaN and the inf"""
    inner = with_children(parents)
    return (int(inner[0]), int(inner[-1])) if len(inner) else (0, len(parents) - 1)


def inverse_binds(n, seed, identity_every=5):
    """float32[n, 12]: rotations x scales + translations (skin_cases.random_palette), every fifth an exact identity (multiplied all the same)"""
    from skin_cases import identity_palette, random_palette
    b = random_palette(n, seed)
    b[::identity_every] = identity_palette(len(b[::identity_every]))
    return b


def clip(parents, n_keys, seed, family="unit"):
    """(times float32[K] ascending strictly with uneven steps, keys float32[K, n, 10])"""
    rng = np.random.default_rng(seed)
    times = np.cumsum(rng.uniform(0.1, 1.0, n_keys)).astype(F) - F(0.5)
    assert (np.diff(times) > 0).all()
    return times, np.stack([pose(family, parents, seed + 1 + k) for k in range(n_keys)])


def sample_times(times):
    """t below the first key, on every key, inside every segment (two places), beyond the last key, and -inf / +inf"""
    times = np.asarray(times, F)
    out = [F(times[0] - F(1.0)), F(-np.inf)]
    for k in range(len(times)):
        out.append(times[k])
        if k + 1 < len(times):
            out.append(F(times[k] + F(0.25) * (times[k + 1] - times[k])))
            out.append(np.nextafter(times[k + 1], F(-np.inf), dtype=F))
    out += [F(times[-1] + F(2.0)), F(np.inf)]
    return out
