"""Two-bone reach and aim constraints (rt_skeleton_solve_ik): the numpy restatement shared by tests/test_skeleton_ik_abi.py (CPU) and
tests/test_gpu_skeleton_ik.py -- the definition of include/dxr_amd.h "Posed skeletons", "inverse kinematics", in fp32, in the stated order,
written from that text and not from dxrexperiments_amd/csrc/rt_ik.h, on top of skeleton_cases.local_of / posed and
skeleton_blend_cases.normalised / hamilton / conj, with NaNs made canonical at the write -- the host's check of a constraint list restated,
and the case generators.  A BATCH is a dict of arrays, one row per constraint: kind uint32[n], has_parent uint32[n], tip / mid / root
float32[n, 10] (the joints c, b, a; an aim reads tip alone), W float32[n, 12] (the parent's world matrix), target, pole float32[n, 3],
weight float32[n]."""
import numpy as np

import skeleton_blend_cases as B
import skeleton_cases as S
import util

F = np.float32
TWO_BONE, AIM = 0, 1
MAX_IK = 32
WEIGHTS = B.WEIGHTS
INF = F(np.inf)


# ---- the definition --------------------------------------------------------------------------------------------------------------------
def dot3(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def cross3(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def unit(v):
    """(v * (1 / sqrt(v.v)) where 0 < v.v < inf, else zero; whether there is an answer)"""
    d = dot3(v, v)
    ok = (d > 0) & (d < INF)
    inv = F(1.0) / np.sqrt(d)
    out = np.where(ok[:, None], v * inv[:, None], F(0.0))
    assert out.dtype == F
    return out, ok


def rot(q, v):
    t = F(2.0) * cross3(q[:, 0:3], v)
    return (v + q[:, 3:4] * t) + cross3(q[:, 0:3], t)


def perp(u):
    a = np.abs(u)
    y = a[:, 1] < a[:, 0]
    least = np.where(y, a[:, 1], a[:, 0])
    z = a[:, 2] < least
    e = np.stack([~y & ~z, y & ~z, z], axis=1).astype(F)
    return unit(cross3(u, e))[0]


def between(u, v):
    s = u + v
    ss = dot3(s, s)
    h, ok = unit(s)
    x = B.normalised(np.concatenate([cross3(u, h), dot3(u, h)[:, None]], axis=1))
    half = (ss < F(1e-6)) | ~ok
    p = np.concatenate([perp(u), np.zeros((len(u), 1), F)], axis=1)
    return np.where(half[:, None], p, x)


def turn(a, b):
    u, ok_u = unit(a)
    v, ok_v = unit(b)
    return np.where((ok_u & ok_v)[:, None], between(u, v), B.IDENTITY_Q[None, :])


def point(M, p):
    return np.stack([((M[:, 4 * r] * p[:, 0] + M[:, 4 * r + 1] * p[:, 1]) + M[:, 4 * r + 2] * p[:, 2]) + M[:, 4 * r + 3] for r in range(3)], axis=1)


def invert3x4(m):
    """the adjugate / determinant inverse of the instance transforms (DESIGN.md "Instances"), every NaN the quiet NaN"""
    m = np.ascontiguousarray(m, F).reshape(-1, 12)
    a, b, c, d, e, f, g, h, i = (m[:, k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    A, Bc, Cc = e * i - f * h, f * g - d * i, d * h - e * g
    det = a * A
    det = det + b * Bc
    det = det + c * Cc
    inv = F(1.0) / det
    o = np.empty_like(m)
    o[:, 0], o[:, 1], o[:, 2] = A * inv, (c * h - b * i) * inv, (b * f - c * e) * inv
    o[:, 4], o[:, 5], o[:, 6] = Bc * inv, (a * i - c * g) * inv, (c * d - a * f) * inv
    o[:, 8], o[:, 9], o[:, 10] = Cc * inv, (b * g - a * h) * inv, (a * e - b * d) * inv
    for r in range(3):
        s = o[:, 4 * r] * m[:, 3]
        s = s + o[:, 4 * r + 1] * m[:, 7]
        s = s + o[:, 4 * r + 2] * m[:, 11]
        o[:, 4 * r + 3] = -s
    return S.canonical_nans(o)


def weigh(A, X, w):
    d = ((A[:, 0] * X[:, 0] + A[:, 1] * X[:, 1]) + A[:, 2] * X[:, 2]) + A[:, 3] * X[:, 3]
    X = np.where((d < 0)[:, None], -X, X)
    q = A + (w[:, None] * (X - A))
    assert q.dtype == F
    return S.canonical_nans(B.normalised(q))


def local(t, q, s):
    return S.local_of(np.concatenate([t, q, s], axis=1))


def solve_batch(b, trace=None):
    """(q_root, q_mid) float32[n, 4]: what the constraints of a batch store in a and b; an aim stores q_root in its joint, its q_mid is zero.
    trace: a dict that receives the path every constraint took -- solve (step 5 passed), pole (0 the pole, 1 the middle joint, 2 perp),
    clamp (-1 raised to |l1 - l2|, 1 cut to l1 + l2, 0 neither), aim (both directions had an answer), half (the aim's turn is the half turn)"""
    with np.errstate(all="ignore"):
        kind = np.asarray(b["kind"])
        tip, mid, root = (np.ascontiguousarray(b[k], F) for k in ("tip", "mid", "root"))
        T, P, w = np.array(b["target"], F), np.array(b["pole"], F), np.ascontiguousarray(b["weight"], F)
        has = np.asarray(b["has_parent"]).astype(bool)
        two = kind == TWO_BONE
        I = invert3x4(b["W"])
        T = np.where(has[:, None], point(I, T), T)
        P = np.where((has & two)[:, None], point(I, P), P)
        # aim
        Q = B.normalised(tip[:, 3:7])
        v, ok_v = unit(rot(Q, P))
        ww, ok_w = unit(T - tip[:, 0:3])
        Q2 = np.where((ok_v & ok_w)[:, None], B.normalised(B.hamilton(between(v, ww), Q)), Q)
        if trace is not None:
            trace.update(aim=ok_v & ok_w, half=(dot3(v + ww, v + ww) < F(1e-6)) | ~unit(v + ww)[1])
        aim = weigh(Q, Q2, w)
        # two-bone
        A, Bq = B.normalised(root[:, 3:7]), B.normalised(mid[:, 3:7])
        La, Lb = local(root[:, 0:3], A, root[:, 7:10]), local(mid[:, 0:3], Bq, mid[:, 7:10])
        pa = root[:, 0:3]
        pb = point(La, mid[:, 0:3])
        pc = point(La, point(Lb, tip[:, 0:3]))
        e1, e2, g = pb - pa, pc - pb, T - pa
        l1, l2 = np.sqrt(dot3(e1, e1)), np.sqrt(dot3(e2, e2))
        n, ok_n = unit(g)
        d = np.sqrt(dot3(g, g))
        lo, hi = np.abs(l1 - l2), l1 + l2
        if trace is not None:
            trace.update(clamp=np.where(d < lo, -1, np.where(d > hi, 1, 0)))
        d = np.where(d < lo, lo, d)
        d = np.where(d > hi, hi, d)
        solve = ok_n & (d > 0) & (l1 > 0) & (l2 > 0)
        x = ((l1 * l1 - l2 * l2) + d * d) / (F(2.0) * d)
        hh = l1 * l1 - x * x
        h = np.sqrt(np.where(hh > 0, hh, F(0.0)))
        k = P - pa
        m0, ok0 = unit(k - n * dot3(k, n)[:, None])
        m1, ok1 = unit(e1 - n * dot3(e1, n)[:, None])
        m = np.where(ok0[:, None], m0, np.where(ok1[:, None], m1, perp(n)))
        if trace is not None:
            trace.update(solve=solve, pole=np.where(ok0, 0, np.where(ok1, 1, 2)))
        pb2 = (pa + n * x[:, None]) + m * h[:, None]
        pc2 = pa + n * d[:, None]
        Da = turn(e1, pb2 - pa)
        A2 = B.normalised(B.hamilton(Da, A))
        b1 = pa + rot(Da, e1)
        c1 = pa + rot(Da, pc - pa)
        Db = turn(c1 - b1, pc2 - b1)
        B2 = B.normalised(B.hamilton(B.hamilton(B.conj(A2), B.hamilton(Db, A2)), Bq))
        A2 = np.where(solve[:, None], A2, A)
        B2 = np.where(solve[:, None], B2, Bq)
        qa, qb = weigh(A, A2, w), weigh(Bq, B2, w)
        for a in (T, P, Q2, pb, pc, l1, d, x, h, m, pb2, Da, A2, Db, B2, qa, qb, aim):
            assert a.dtype == F
        return np.where(two[:, None], qa, aim), np.where(two[:, None], qb, F(0.0))


def chain_of(parents, kind, joint):
    """(c, b, a, p): the joints a constraint reads poses of, and the parent whose space it is solved in (-1: none)"""
    c = int(joint)
    b, a = (int(parents[c]), int(parents[parents[c]])) if kind == TWO_BONE else (c, c)
    return c, b, a, int(parents[a])


def batch_of(parents, pose, joints, constraints):
    """the batch of a list of (kind, joint, target, pole, weight) against a skeleton's local pose float32[n, 10] and joints float32[n, 12]"""
    pose, joints = np.asarray(pose, F).reshape(-1, 10), np.asarray(joints, F).reshape(-1, 12)
    chains = [chain_of(parents, c[0], c[1]) for c in constraints]
    return {"kind": np.array([c[0] for c in constraints], np.uint32), "has_parent": np.array([ch[3] >= 0 for ch in chains], np.uint32),
            "tip": pose[[ch[0] for ch in chains]], "mid": pose[[ch[1] for ch in chains]], "root": pose[[ch[2] for ch in chains]],
            "W": joints[[max(ch[3], 0) for ch in chains]], "target": np.array([c[2] for c in constraints], F).reshape(-1, 3),
            "pole": np.array([c[3] for c in constraints], F).reshape(-1, 3), "weight": np.array([c[4] for c in constraints], F)}, chains


def solved(parents, pose, joints, constraints):
    """the local pose float32[n, 10] a solve leaves: every constraint from the same input, only quaternions written"""
    batch, chains = batch_of(parents, pose, joints, constraints)
    qa, qb = solve_batch(batch)
    out = np.array(pose, F, copy=True).reshape(-1, 10)
    for k, (c, b, a, p) in enumerate(chains):
        out[a, 3:7] = qa[k]
        if constraints[k][0] == TWO_BONE:
            out[b, 3:7] = qb[k]
    return out


def solved_and_posed(parents, inverse_bind, pose, constraints):
    """(pose, W, M) after a solve of a skeleton that holds `pose`"""
    W, _ = S.posed(parents, inverse_bind, pose)
    out = solved(parents, pose, W, constraints)
    return (out,) + S.posed(parents, inverse_bind, out)


# ---- the host's check of a constraint list (dxrexperiments_amd/csrc/rt_skeleton.h: rt_skeleton_validate_ik) --------------------------------
def validate(records, parents, posed):
    """(what, (writer or constraint, reader, joint)) for raw records (kind, joint, target, pole, weight): 0 fine, 2 n outside 1 .. 32, 3 an
    unknown kind, 4 a joint >= n_joints, 5 a two-bone tip with fewer than two ancestors, 6 a NaN weight -- every constraint is held to these
    first, in this order --, 7 a constraint writes what another reads (readers in order, each walked from its joint up; the lowest
    writer), 8 no pose yet.  2 .. 7 are RT_ERR_INVALID_ARG, 8 is RT_ERR_STATE."""
    n_joints = len(parents)
    if not 1 <= len(records) <= MAX_IK:
        return 2, (0, 0, 0)
    for k, (kind, joint, target, pole, weight) in enumerate(records):
        if kind not in (TWO_BONE, AIM):
            return 3, (k, 0, 0)
        if joint >= n_joints:
            return 4, (k, 0, joint)
        if kind == TWO_BONE and (parents[joint] < 0 or parents[parents[joint]] < 0):
            return 5, (k, 0, joint)
        if np.isnan(weight):
            return 6, (k, 0, 0)
    writes = []
    for kind, joint, *_ in records:
        writes.append({int(parents[joint]), int(parents[parents[joint]])} if kind == TWO_BONE else {int(joint)})
    for k, (kind, joint, *_) in enumerate(records):
        j = int(joint)
        while j >= 0:
            for other in range(len(records)):
                if other != k and j in writes[other]:
                    return 7, (other, k, j)
            j = int(parents[j])
    return (0 if posed else 8), (0, 0, 0)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def comb(n_limbs=16, n_teeth=16):
    """parents of a comb: joint 0 is the root; limb l owns the chain 1 + 3 l (child of 0), 2 + 3 l, 3 + 3 l; after the limbs, n_teeth single
    joints hang off the root.  16 limbs and 16 teeth are 65 joints that take 32 independent constraints: a two-bone constraint on each
    limb's last joint writes the limb's first two joints, an aim on a tooth writes the tooth, and nothing reads either but its own
    constraint (all read the root, which nothing writes)."""
    p = [-1]
    for l in range(n_limbs):
        p += [0, 1 + 3 * l, 2 + 3 * l]
    return np.array(p + [0] * n_teeth, np.int32)


def comb_constraints(n, seed, n_limbs=16, n_teeth=16):
    """n <= n_limbs + n_teeth independent constraints on comb(): two-bone and aim in turn, targets and poles 0.5 .. 3 from the origin, weights
    walking through WEIGHTS"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        kind = (TWO_BONE, AIM)[k % 2] if k // 2 < min(n_limbs, n_teeth) else (TWO_BONE if n_limbs > n_teeth else AIM)
        joint = 3 + 3 * (k // 2) if kind == TWO_BONE else 1 + 3 * n_limbs + k // 2
        if k // 2 >= min(n_limbs, n_teeth):
            rest = k - 2 * min(n_limbs, n_teeth)
            joint = 3 + 3 * (n_teeth + rest) if kind == TWO_BONE else 1 + 3 * n_limbs + n_limbs + rest
        target = _units(1, rng)[0] * rng.uniform(0.5, 3.0)
        pole = _units(1, rng)[0] * rng.uniform(0.5, 3.0)
        out.append((kind, int(joint), tuple(float(F(x)) for x in target), tuple(float(F(x)) for x in pole), WEIGHTS[k % len(WEIGHTS)]))
    return out


def _units(n, rng):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def fk64(b, qa=None, qb=None):
    """float64 forward kinematics of a batch in parent space, quaternions as stored (or qa, qb in their place): pa, pb, pc"""
    root, mid, tip = (np.asarray(b[k], np.float64) for k in ("root", "mid", "tip"))
    A = np.asarray(root[:, 3:7] if qa is None else qa, np.float64)
    Bq = np.asarray(mid[:, 3:7] if qb is None else qb, np.float64)
    La, Lb = _local64(root[:, 0:3], A, root[:, 7:10]), _local64(mid[:, 0:3], Bq, mid[:, 7:10])
    return root[:, 0:3], point64(La, mid[:, 0:3]), point64(La, point64(Lb, tip[:, 0:3]))


def _local64(t, q, s):
    x, y, z, w = q.T
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)
    M = np.empty((len(t), 3, 4))
    M[:, :, :3] = R * s[:, None, :]
    M[:, :, 3] = t
    return M


def point64(M, p):
    M = np.asarray(M, np.float64).reshape(-1, 3, 4)
    return np.einsum("nrc,nc->nr", M[:, :, :3], p) + M[:, :, 3]


def inverse64(W):
    W = np.asarray(W, np.float64).reshape(-1, 3, 4)
    Li = np.linalg.inv(W[:, :, :3])
    out = np.empty_like(W)
    out[:, :, :3] = Li
    out[:, :, 3] = -np.einsum("nrc,nc->nr", Li, W[:, :, 3])
    return out


REGIMES = ("reachable", "out_of_reach", "nearly_straight", "too_close")


def chains(regime, n, seed, parent="xforms", uniform=True, unit_quats=True):
    """a batch of n two-bone constraints of weight 1.  Bones 0.3 .. 1.2 long, l1 and l2 at least 5 % of the chain apart; the target at a
    distance from a, in the space of a's parent, of: reachable |l1 - l2| + 5 % .. 95 % of l1 + l2; out_of_reach 1.1 .. 3 x (l1 + l2);
    nearly_straight (l1 + l2) x (1 - 1e-6 .. 1e-4); too_close 5 .. 90 % of |l1 - l2|.  The pole stands 0.1 .. 1 chain lengths off the axis
    from a to the target.  parent: None (a is a root: W is not read), "xforms" (util.random_xforms) or a family of util.hard_xforms.
    uniform: a and b carry uniform scale 0.5 .. 1.5 (the RIGID families: the tip reaches the target); else three scales each."""
    rng = np.random.default_rng(seed)
    b = {"kind": np.full(n, TWO_BONE, np.uint32), "has_parent": np.full(n, 0 if parent is None else 1, np.uint32), "weight": np.ones(n, F)}
    for name in ("tip", "mid", "root"):
        j = np.empty((n, 10))
        j[:, 0:3] = _units(n, rng) * rng.uniform(0.3, 1.2, (n, 1))
        q = rng.normal(size=(n, 4))
        j[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
        if not unit_quats:
            j[:, 3:7] *= rng.uniform(0.5, 2.0, (n, 1))
        j[:, 7:10] = rng.uniform(0.5, 1.5, (n, 1)) if uniform else rng.uniform(0.5, 1.5, (n, 3))
        b[name] = j.astype(F)
    if parent is None:
        b["W"] = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (n, 1))
    elif parent == "xforms":
        b["W"] = util.random_xforms(n, seed + 1)
    else:
        b["W"] = util.hard_xforms(parent, n, seed + 1)
    # lengths as float64 sees the normalised input; keep l1 and l2 apart
    norm = {k: np.asarray(b[k], np.float64) for k in ("root", "mid")}
    qa = norm["root"][:, 3:7] / np.linalg.norm(norm["root"][:, 3:7], axis=1, keepdims=True)
    qb = norm["mid"][:, 3:7] / np.linalg.norm(norm["mid"][:, 3:7], axis=1, keepdims=True)
    pa, pb, pc = fk64(b, qa, qb)
    l1, l2 = np.linalg.norm(pb - pa, axis=1), np.linalg.norm(pc - pb, axis=1)
    close = np.abs(l1 - l2) < 0.05 * (l1 + l2)
    b["tip"][close, 0:3] *= F(0.5)
    pa, pb, pc = fk64(b, qa, qb)
    l1, l2 = np.linalg.norm(pb - pa, axis=1), np.linalg.norm(pc - pb, axis=1)
    L, gap = l1 + l2, np.abs(l1 - l2)
    u = rng.uniform(size=n)
    dist = {"reachable": gap + 0.05 * L + u * (0.95 * L - gap - 0.05 * L), "out_of_reach": (1.1 + 1.9 * u) * L,
            "nearly_straight": L * (1 - 10.0 ** (-6 + 2 * u)), "too_close": (0.05 + 0.85 * u) * gap}[regime]
    axis = _units(n, rng)
    side = np.cross(axis, _units(n, rng))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    target = pa + axis * dist[:, None]
    pole = pa + axis * rng.uniform(-1, 2, (n, 1)) * L[:, None] + side * (rng.uniform(0.1, 1.0, n) * L)[:, None]
    W = np.asarray(b["W"], np.float64)
    b["target"] = (point64(W, target) if parent is not None else target).astype(F)
    b["pole"] = (point64(W, pole) if parent is not None else pole).astype(F)
    return b


def aims(n, seed, parent="xforms", antiparallel_every=10):
    """a batch of n aims of weight 1: a random joint, a random axis of length 0.5 .. 2, a target 0.5 .. 5 away in the parent's space; every
    tenth target stands opposite the axis as the pose has it, to fp32 rounding"""
    rng = np.random.default_rng(seed)
    b = chains("reachable", n, seed + 7, parent=parent)
    b["kind"] = np.full(n, AIM, np.uint32)
    axis = _units(n, rng) * rng.uniform(0.5, 2.0, (n, 1))
    direction = _units(n, rng)
    q = np.asarray(b["tip"][:, 3:7], np.float64)
    R = _local64(np.zeros((n, 3)), q / np.linalg.norm(q, axis=1, keepdims=True), np.ones((n, 3)))[:, :, :3]
    now = np.einsum("nrc,nc->nr", R, axis)
    anti = np.arange(n) % antiparallel_every == 0
    direction[anti] = -now[anti] / np.linalg.norm(now[anti], axis=1, keepdims=True)
    target = np.asarray(b["tip"][:, 0:3], np.float64) + direction * rng.uniform(0.5, 5.0, (n, 1))
    W = np.asarray(b["W"], np.float64)
    b["target"] = (point64(W, target) if parent is not None else target).astype(F)
    b["pole"] = axis.astype(F)
    return b


def concat(batches):
    return {k: np.concatenate([np.asarray(b[k]) for b in batches]) for k in batches[0]}


def at_weights(b):
    """the batch at each of WEIGHTS"""
    out = []
    for w in WEIGHTS:
        c = {k: np.array(v, copy=True) for k, v in b.items()}
        c["weight"] = np.full(len(c["kind"]), w, F)
        out.append(c)
    return concat(out)


def _axis_chain(n=1, l1=1.0, l2=0.75, target=(1.25, 0, 0), pole=(0.5, 1.0, 0), kind=TWO_BONE, along=0):
    """exact chains along a coordinate axis (+x) from the origin without a parent: identity rotations, unit scales"""
    b = {"kind": np.full(n, kind, np.uint32), "has_parent": np.zeros(n, np.uint32), "weight": np.ones(n, F),
         "W": np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (n, 1))}
    ident = [0, 0, 0, 1, 1, 1, 1]
    b["root"] = np.tile(np.array([0, 0, 0] + ident, F), (n, 1))
    b["mid"] = np.tile(np.array([l1 * (along == c) for c in range(3)] + ident, F), (n, 1))
    b["tip"] = np.tile(np.array([l2 * (along == c) for c in range(3)] + ident, F), (n, 1))
    b["target"] = np.tile(np.array(target, F), (n, 1))
    b["pole"] = np.tile(np.array(pole, F), (n, 1))
    return b


def degenerate():
    """name -> a small batch of weight 1: the places where the definition takes another path"""
    out = {}
    on_a = chains("reachable", 16, 21, parent=None)
    on_a["target"] = on_a["root"][:, 0:3].copy()
    out["target_on_a"] = on_a
    out["pole_on_axis"] = _axis_chain(target=(1.25, 0, 0), pole=(0.5, 0, 0))
    bent = _axis_chain(target=(1.25, 0, 0), pole=(3.0, 0, 0))
    h = F(np.sqrt(0.5))
    bent["root"][:, 3:7] = (0, 0, h, h)                                                       # a quarter turn about z: pb = (0, 1, 0), off the axis
    out["pole_on_axis_first_fallback"] = bent
    out["pole_and_middle_on_axis_perp"] = concat([_axis_chain(target=t, pole=p, along=a) for a, t, p in ((0, (1.25, 0, 0), (0.5, 0, 0)), (1, (0, 1.5, 0), (0, -2, 0)), (2, (0, 0, 1.0), (0, 0, 0)))])
    out["zero_first_bone"] = _axis_chain(l1=0.0)
    out["zero_second_bone"] = _axis_chain(l2=0.0)
    out["equal_bones_target_on_a"] = _axis_chain(l1=1.0, l2=1.0, target=(0, 0, 0))
    out["equal_bones_target_near_a"] = _axis_chain(l1=1.0, l2=1.0, target=(1e-3, 2e-3, 0))
    par = _axis_chain(n=4, kind=AIM)
    par["pole"] = np.array([[1, 0, 0], [0, 2, 0], [0, 0, 0.5], [1, 1, 0]], F)
    par["target"] = par["pole"] * F(3.0)
    out["aim_parallel"] = par
    anti = _axis_chain(n=4, kind=AIM)
    anti["pole"] = np.array([[0, 1, 0], [1, 0, 0], [1, 1, 0], [0, 0, 1]], F)                  # e = x, y, z and x again
    anti["target"] = -anti["pole"] * F(2.0)
    anti["tip"][:, 0:3] = 0.0
    par["tip"][:, 0:3] = 0.0
    out["aim_antiparallel"] = anti
    zero = aims(8, 31)
    zero["pole"][:] = 0.0
    out["aim_zero_axis"] = zero
    on = aims(8, 32, parent=None)
    on["target"] = on["tip"][:, 0:3].copy()
    out["aim_target_on_joint"] = on
    return out


def non_finite(seed=41):
    """two-bone chains and aims with a NaN, +inf or -inf in one float of the target, the pole, a pose or W, and zero quaternions"""
    rng = np.random.default_rng(seed)
    b = concat([chains("reachable", 96, seed), aims(96, seed + 1)])
    n = len(b["kind"])
    values = np.array([np.nan, np.inf, -np.inf], F)
    for k in range(n):
        name = ("target", "pole", "tip", "mid", "root", "W")[k % 6]
        b[name][k, int(rng.integers(0, b[name].shape[1]))] = values[(k // 6) % 3]
    zero = concat([chains("reachable", 6, seed + 2), aims(3, seed + 3)])
    zero["root"][0:2, 3:7] = 0.0
    zero["mid"][2:4, 3:7] = 0.0
    zero["tip"][6:9, 3:7] = 0.0
    return concat([b, zero])


def bitwise_families():
    """name -> batch, each at every weight of WEIGHTS: what the solver under the sanitizers, and the kernel, are held to bit for bit"""
    out = {}
    for regime in REGIMES:
        out[regime] = chains(regime, 48, 100 + REGIMES.index(regime))
        out[regime + "_root"] = chains(regime, 16, 110 + REGIMES.index(regime), parent=None)
    for k, family in enumerate(("mirror", "shear", "stretch", "squash")):
        out["parent_" + family] = concat([chains("reachable", 16, 120 + k, parent=family), aims(16, 130 + k, parent=family)])
    out["aims"] = aims(64, 140)
    out["aims_root"] = aims(32, 141, parent=None)
    out["non_unit_quaternions"] = concat([chains("reachable", 32, 150, unit_quats=False), chains("too_close", 16, 151, unit_quats=False)])
    out["non_uniform_scales"] = concat([chains(r, 16, 160 + k, uniform=False) for k, r in enumerate(REGIMES)])
    out.update(degenerate())
    out["non_finite"] = non_finite()
    return {name: at_weights(b) for name, b in out.items()}


def rigid_families():
    """name -> batch of weight 1 that the geometry holds for: uniform scale on a and b, ancestors from util.random_xforms (or none)"""
    out = {}
    for k, regime in enumerate(REGIMES):
        out[regime] = concat([chains(regime, 1000, 200 + k), chains(regime, 200, 210 + k, parent=None)])
    out["aim"] = concat([aims(1000, 220), aims(200, 221, parent=None)])
    return out


def geometry_errors(b, qa, qb):
    """of a rigid batch and its solved quaternions, in float64 and in the space of the chain root's parent.  Two-bone: (the distance of the
    tip from the clamped target over l1 + l2, the middle joint's offset from the axis towards the pole's side over l1 + l2 -- negative: the wrong
    side).  Aim: (|unit(R(Q') axis) - unit(T - t_j)|, None)."""
    has = np.asarray(b["has_parent"]).astype(bool)
    I = inverse64(b["W"])
    T = np.where(has[:, None], point64(I, np.asarray(b["target"], np.float64)), b["target"])
    if b["kind"][0] == AIM:
        R = _local64(np.zeros((len(T), 3)), np.asarray(qa, np.float64), np.ones((len(T), 3)))[:, :, :3]
        v = np.einsum("nrc,nc->nr", R, np.asarray(b["pole"], np.float64))
        w = T - np.asarray(b["tip"][:, 0:3], np.float64)
        return np.linalg.norm(v / np.linalg.norm(v, axis=1, keepdims=True) - w / np.linalg.norm(w, axis=1, keepdims=True), axis=1), None
    P = np.where(has[:, None], point64(I, np.asarray(b["pole"], np.float64)), b["pole"])
    norm = lambda q: np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64), axis=1, keepdims=True)
    pa, pb, pc = fk64(b, norm(b["root"][:, 3:7]), norm(b["mid"][:, 3:7]))
    l1, l2 = np.linalg.norm(pb - pa, axis=1), np.linalg.norm(pc - pb, axis=1)
    g = T - pa
    d = np.linalg.norm(g, axis=1)
    n = g / d[:, None]
    clamped = pa + n * np.clip(d, np.abs(l1 - l2), l1 + l2)[:, None]
    _, pb2, pc2 = fk64(b, qa, qb)
    k = P - pa
    off = k - n * (k * n).sum(axis=1, keepdims=True)
    assert (np.linalg.norm(off, axis=1) >= 1e-3 * (l1 + l2)).all(), "a rigid family keeps its pole off the axis by construction"
    side = off / np.linalg.norm(off, axis=1, keepdims=True)
    e = pb2 - pa
    return np.linalg.norm(pc2 - clamped, axis=1) / (l1 + l2), ((e - n * (e * n).sum(axis=1, keepdims=True)) * side).sum(axis=1) / (l1 + l2)
