"""Inverse kinematics for crowds (rt_crowd_set_ik_chains, rt_crowd_solve_ik; include/dxr_amd.h "Posed skeletons", crowds) for the tests:
the restatement of what the host packs and checks (dxrexperiments_amd/csrc/rt_skeleton.h: rt_skeleton_pack_ik; rt_crowd_ik.h), the rigs,
chain lists and per-actor values the GPU tests solve, and the families of ik_cases dealt to (actor, chain).  The arithmetic of a solve is not
restated here: actor a of a crowd is a skeleton given rt_skeleton_solve_ik with its own values, so the numpy statement is tests/ik_cases.py,
by import."""
import numpy as np

import crowd_cases as CC
import ik_cases as IK
import skeleton_cases as S

F = np.float32
NAN = float("nan")
LDS = S.lds_joints()
MAX_IK = IK.MAX_IK


# ---- what the host packs and checks --------------------------------------------------------------------------------------------------------
def packed_table(records, parents):
    """uint32[n, 12]: the entries rt_skeleton_pack_ik makes of a crowd's chain list -- kind, c, b, a, p, the target (0, 0, 0: a chain has
    none), the default pole and the default weight"""
    out = np.zeros((len(records), 12), np.uint32)
    for k, (kind, joint, target, pole, weight) in enumerate(records):
        c, b, a, p = IK.chain_of(parents, kind, joint)
        out[k, 0:4] = (kind, c, b, a)
        out[k, 4] = np.array([p], np.int32).view(np.uint32)[0]
        out[k, 8:11] = np.array(pole, F).view(np.uint32)
        out[k, 11] = np.array([weight], F).view(np.uint32)[0]
    return out


def check_values(weights):
    """(what, actor, constraint) of host weights float32[n_actors, n], or None: 6 and the first NaN weight, the first bad actor first; else
    (0, 0, 0)"""
    if weights is None:
        return 0, 0, 0
    bad = np.argwhere(np.isnan(np.asarray(weights, F)))
    return (6, int(bad[0][0]), int(bad[0][1])) if len(bad) else (0, 0, 0)


def value_block(targets, poles, weights):
    """(offset of the poles, offset of the weights, floats, the block) of a host call's one upload: the arrays it brings, one behind another"""
    parts, at = [np.asarray(targets, F).reshape(-1)], {}
    for name, a in (("poles", poles), ("weights", weights)):
        at[name] = sum(len(p) for p in parts) if a is not None else 0
        if a is not None:
            parts.append(np.asarray(a, F).reshape(-1))
    block = np.concatenate(parts)
    return at["poles"], at["weights"], len(block), block


def value_cases():
    """(n_actors, n, targets, poles or None, weights or None): no NaN weight, one in the first, a middle and the last entry, two of them (the
    first is named), every float of targets and poles a NaN (no refusal: the host does not look), with and without each optional array"""
    rng = np.random.default_rng(17)
    out = []
    for n_actors, n in ((1, 1), (1, 32), (3, 2), (7, 5), (300, 3)):
        e = n_actors * n
        for has_poles in (True, False):
            targets = rng.uniform(-3, 3, (n_actors, n, 3)).astype(F)
            poles = rng.uniform(-3, 3, (n_actors, n, 3)).astype(F) if has_poles else None
            out.append((n_actors, n, targets, poles, None))
            fine = rng.choice(np.array(IK.WEIGHTS + (np.inf, -np.inf), F), (n_actors, n)).astype(F)
            out.append((n_actors, n, targets, poles, fine))
            for at in sorted({0, e // 2, e - 1}):
                w = fine.copy()
                w.reshape(-1)[at] = np.nan
                out.append((n_actors, n, targets, poles, w))
            w = fine.copy()
            w.reshape(-1)[[e - 1, e // 3]] = np.nan
            out.append((n_actors, n, targets, poles, w))
            out.append((n_actors, n, np.full_like(targets, np.nan), None if poles is None else np.full_like(poles, np.nan), fine))
    return out


# ---- what the GPU tests solve --------------------------------------------------------------------------------------------------------------
def independent_chains(parents, n, seed):
    """n chains of both kinds on random joints that pass the host's check, default poles random, default weights walking through WEIGHTS"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(100000):
        if len(out) == n:
            break
        c = (int(rng.integers(0, 2)), int(rng.integers(0, len(parents))), (0.0, 0.0, 0.0), tuple(float(F(x)) for x in rng.uniform(-3, 3, 3)), IK.WEIGHTS[len(out) % len(IK.WEIGHTS)])
        if IK.validate(out + [c], parents, True)[0] == 0:
            out.append(c)
    assert len(out) == n
    return out


def rigs():
    """(name, parents, chain lists): a chain of 3 (the chain's root is a root of the skeleton: no W_p) and of 4; the 65-joint comb with 1, 31
    and 32 chains of both kinds (two waves: solved quaternions cross the barrier to another wave); a random tree of 257 joints with an
    independent list (the block of 256 with the strided loop); a chain of RT_SKELETON_LDS_JOINTS joints with a two-bone chain on its last"""
    z = (0.0, 0.0, 0.0)
    out = []
    for n in (3, 4):
        out.append(("chain %d" % n, S.hierarchy("chain", n, 0), [[(IK.TWO_BONE, n - 1, z, (0.0, 2.0, 1.0), 0.75)], [(IK.AIM, n - 1, z, (1.0, 0.5, 0.0), 0.25)], [(IK.AIM, 0, z, (0.0, 1.0, 0.0), 1.0)]]))
    comb = IK.comb()
    lists = [IK.comb_constraints(k, 10 + k) for k in (1, 31, 32)]
    assert {c[0] for c in lists[2]} == {IK.TWO_BONE, IK.AIM}
    out.append(("comb 65", comb, lists))
    tree = S.hierarchy("random", 257, 300)
    out.append(("random 257", tree, [independent_chains(tree, 9, 311)]))
    out.append(("chain %d" % LDS, S.hierarchy("chain", LDS, 0), [[(IK.TWO_BONE, LDS - 1, z, (0.0, 2.0, 1.0), 1.0)]]))
    return out


def values(n_actors, n, seed):
    """(targets float32[n_actors, n, 3], poles likewise, weights float32[n_actors, n]): every actor's own, weights walking through WEIGHTS
    from an actor's own start"""
    rng = np.random.default_rng(seed)
    targets = rng.uniform(-3, 3, (n_actors, n, 3)).astype(F)
    poles = rng.uniform(-3, 3, (n_actors, n, 3)).astype(F)
    weights = np.array([[IK.WEIGHTS[(a + k) % len(IK.WEIGHTS)] for k in range(n)] for a in range(n_actors)], F)
    return targets, poles, weights


def constraints_of(chains, targets, poles, weights, a):
    """the constraints rt_skeleton_solve_ik takes for actor a: the chains' kinds and joints with the actor's values, or the chains' own
    pole and weight where the call brings none"""
    return [(kind, joint, tuple(float(x) for x in targets[a, k]), pole if poles is None else tuple(float(x) for x in poles[a, k]), weight if weights is None else float(weights[a, k]))
            for k, (kind, joint, _, pole, weight) in enumerate(chains)]


def prior_poses(parents, n_actors, seed):
    """float32[n_actors, n, 10]: unit poses and raw ones (quaternions that are not unit, a fifth of them zero) in turn"""
    return np.stack([S.pose(("unit", "raw")[a % 2], parents, seed + a) for a in range(n_actors)])


def checked_actors(n_actors, n_levels):
    """all of a small case, else the first, a middle and the last"""
    return CC.numpy_actors(n_actors, n_levels)


# ---- the families of ik_cases, dealt to (actor, chain) ---------------------------------------------------------------------------------------
def family(name):
    if name == "degenerate":
        return IK.at_weights(IK.concat(list(IK.degenerate().values())))
    if name == "non_finite":
        return IK.at_weights(IK.non_finite())
    return IK.at_weights(IK.concat([IK.chains(r, 8, 400 + k, uniform=False, unit_quats=False, parent=None if k % 2 else "xforms") for k, r in enumerate(IK.REGIMES)] + [IK.aims(16, 410)]))


def groups(batch, seed):
    """the rows of a batch grouped by (kind, has_parent); each group becomes crowds of one rig of up to 32 trees p, a, b, c (a is p's child
    where the rows have a parent; a two-bone chain is solved on c, an aim on a) whose row (actor, chain) is row actor * n + chain of the
    group.  Yields (parents, chains, poses float32[n_actors, 4 n, 10], targets, poles, weights): the rig, its chain list with zero default
    poles and weights, and every actor's pose and values.  p's pose is random with three scales, and takes a NaN or an inf where the row's W
    has one, as test_gpu_skeleton_ik.forest_of builds it."""
    rng = np.random.default_rng(seed)
    kinds, has = np.asarray(batch["kind"]), np.asarray(batch["has_parent"]).astype(bool)
    for kind in (IK.TWO_BONE, IK.AIM):
        for parent in (False, True):
            rows = np.flatnonzero((kinds == kind) & (has == parent))
            if len(rows) == 0:
                continue
            n = min(MAX_IK, len(rows))
            n_actors = -(-len(rows) // n)
            rows = np.concatenate([rows, rows[:n_actors * n - len(rows)]])           # (the last actor is filled up from the first rows)
            parents = np.empty(4 * n, np.int32)
            for k in range(n):
                parents[4 * k:4 * k + 4] = (-1, 4 * k if parent else -1, 4 * k + 1, 4 * k + 2)
            z = (0.0, 0.0, 0.0)
            chains = [(int(kind), 4 * k + 3 if kind == IK.TWO_BONE else 4 * k + 1, z, z, 0.0) for k in range(n)]
            poses = np.empty((n_actors, 4 * n, 10), F)
            for a in range(n_actors):
                for k in range(n):
                    r, p = rows[a * n + k], 4 * k
                    poses[a, p] = S.pose("unit", np.array([-1], np.int32), int(rng.integers(0, 1 << 30)))[0]
                    W = batch["W"][r]
                    if not np.isfinite(W).all():
                        poses[a, p, 1 if np.isnan(W).any() else 8] = W[~np.isfinite(W)][0]
                    poses[a, p + 1] = batch["root"][r] if kind == IK.TWO_BONE else batch["tip"][r]
                    poses[a, p + 2], poses[a, p + 3] = batch["mid"][r], batch["tip"][r]
            pick = rows.reshape(n_actors, n)
            yield parents, chains, poses, np.asarray(batch["target"], F)[pick], np.asarray(batch["pole"], F)[pick], np.asarray(batch["weight"], F)[pick]
