"""Ordered groups of IK constraints (rt_skeleton_solve_ik_groups, rt_crowd_set_ik_chain_groups; include/dxr_amd.h "Posed skeletons", inverse
kinematics, GROUPS) for the tests: the numpy statement of a grouped solve -- ik_cases.solved_and_posed applied group after group to the pose
the previous group left --, the restatement of the host's check (dxrexperiments_amd/csrc/rt_ik_groups.h) on top of ik_cases.validate, of the
group ends and of the refusals' text, and the rigs and grouped lists the GPU tests solve.  A group is a list of (kind, joint, target, pole,
weight) records as ik_cases takes them; a grouped list is a list of groups."""
import numpy as np

import crowd_ik_cases as CI
import ik_cases as IK
import skeleton_cases as S

F = np.float32
MAX_GROUPS = 8
Z = (0.0, 0.0, 0.0)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------------
def flat(groups):
    return [c for g in groups for c in g]


def sizes_of(groups):
    return [len(g) for g in groups]


def split(records, sizes):
    out, first = [], 0
    for s in sizes:
        out.append(list(records[first:first + s]))
        first += s
    return out


def solved_and_posed(parents, inverse_bind, pose, groups):
    """(pose, W, M) after the groups, in order: each group is one ik_cases.solved_and_posed on the pose the group before it left"""
    out = (np.array(pose, F, copy=True).reshape(-1, 10),) + S.posed(parents, inverse_bind, pose)
    for g in groups:
        out = IK.solved_and_posed(parents, inverse_bind, out[0], g)
    return out


def side_by_side(parents, inverse_bind, pose, groups):
    """the pose a kernel would leave that forgot the walk between its stages: the whole list solved from the ONE input pose"""
    W, _ = S.posed(parents, inverse_bind, pose)
    return IK.solved(parents, pose, W, flat(groups))


def is_dependent(parents, inverse_bind, pose, groups):
    """the condition on a dependent case: the joined list is refused as one group (code 7), and the grouped result differs in bits from
    side_by_side"""
    return IK.validate(flat(groups), parents, True)[0] == 7 and solved_and_posed(parents, inverse_bind, pose, groups)[0].tobytes() != side_by_side(parents, inverse_bind, pose, groups).tobytes()


# ---- the host's check (rt_ik_groups.h: rt_ik_groups_validate, rt_ik_group_ends, rt_ik_groups_refusal) ----------------------------------------
def validate(sizes, records, parents, posed, null=False):
    """(what, (writer or constraint, reader, joint, group)) in the order of the header: 1 a null array, 9 the number of groups outside
    1 .. 8, 10 an empty group, 2 the total outside 1 .. 32, 3 .. 6 of ik_cases.validate over the whole list, 11 a dependent pair inside one
    group (list indices), 8 no pose"""
    none = (0, 0, 0, 0)
    if null:
        return 1, none
    if not 1 <= len(sizes) <= MAX_GROUPS:
        return 9, none
    for g, s in enumerate(sizes):
        if s == 0:
            return 10, (0, 0, 0, g)
    if sum(sizes) > IK.MAX_IK:
        return 2, none
    assert len(records) == sum(sizes)
    what, bad = IK.validate(records, parents, True)
    if 3 <= what <= 6:
        return what, tuple(bad) + (0,)
    first = 0
    for g, s in enumerate(sizes):
        what, bad = IK.validate(records[first:first + s], parents, True)
        if what == 7:
            return 11, (first + bad[0], first + bad[1], bad[2], g)
        first += s
    return (0 if posed else 8), none


def group_ends(sizes):
    """the 64 bits that travel beside the table: byte g is where group g ends; the bytes behind the last group repeat the total"""
    ends, end = 0, 0
    for g in range(MAX_GROUPS):
        if g < len(sizes):
            end += sizes[g]
        ends |= end << (8 * g)
    return ends


def refusal(who, what, bad, n_groups, total):
    """the text of the codes this check adds; None for the codes whose text is rt_skeleton_ik_refusal's"""
    if what == 9:
        return "%s: %d groups: 1 .. 8 are supported" % (who, n_groups)
    if what == 10:
        return "%s: group %d is empty: every group holds at least one constraint" % (who, bad[3])
    if what == 11:
        return ("%s: constraints %d and %d of group %d depend on one another: constraint %d writes joint %d, which constraint %d reads (its joint or an ancestor of it); "
                "put the reader in a later group" % (who, bad[0], bad[1], bad[3], bad[0], bad[2], bad[1]))
    if what == 2:
        return "%s: %d constraints: 1 .. 32 are supported" % (who, total)
    return None


def check_cases():
    """(sizes, n_groups, records, parents, posed, null_sizes, null_records): grouped lists that reach every code -- 0, 1, 2, 3 - 6, 8, 9, 10,
    11 --, among them lists whose sizes or whose records must not be read (n_groups 0, 9 and 2^32 - 1 with no size behind the pointer;
    totals of 33 and of 8 x (2^32 - 1) with no record behind it), and 200 generated ones.  n_groups is what the call is told; len(sizes)
    what stands behind the pointer."""
    N, NAN = 0xFFFFFFFF, float("nan")
    x = (1.0, 0.0, 0.0)
    chain, comb = S.hierarchy("chain", 8, 0), IK.comb()
    reach, aim = (IK.TWO_BONE, 3, Z, x, 1.0), (IK.AIM, 3, Z, x, 0.5)
    out = []

    def add(sizes, records, parents, posed=True, n_groups=None, null_sizes=False, null_records=False):
        out.append((list(sizes), len(sizes) if n_groups is None else n_groups, list(records), parents, posed, null_sizes, null_records))

    add([1, 1], [reach, aim], chain)                                  # 0: the pair one list refuses
    add([1, 1], [reach, aim], chain, posed=False)                     # 8
    add([2], [reach, aim], chain)                                     # 11: as one group
    add([2], [aim, reach], chain)                                     # 11: the other order
    add([1, 2, 1], [(IK.AIM, 7, Z, x, 1.0), reach, aim, reach], chain)        # 11 in a middle group: list indices 1 and 2
    add([1, 1, 2], [reach, aim, (IK.AIM, 5, Z, x, 1.0), (IK.AIM, 6, Z, x, 1.0)], chain)      # 11 in the last group: 2 writes 5, which 3 reads
    add([1, 1], [reach, aim], chain, null_sizes=True)                 # 1
    add([1, 1], [reach, aim], chain, null_records=True)               # 1
    add([1, 1], [reach, aim], chain, null_sizes=True, null_records=True)
    for n_groups in (0, 9, N):                                        # 9: no size is read
        add([], [], chain, n_groups=n_groups)
    add([], [reach], chain, n_groups=0, null_records=True)            # 1 before 9
    add([1, 0], [reach], chain)                                       # 10
    add([0], [], chain)
    add([1, 1, 1, 1, 1, 1, 1, 0], [(IK.AIM, j, Z, x, 1.0) for j in range(7)], chain)
    add([0, N], [], chain)                                            # 10 before 2
    add([33], [], comb)                                               # 2: no record is read
    add([32, 1], [], comb)
    add([N] * 8, [], comb)                                            # (the sum does not wrap)
    add([N, 1], [], comb)                                             # (2^32: a 32-bit sum would say 0)
    add([25, 1, 1, 1, 1, 1, 1, 1], [(IK.AIM, 0, Z, x, 1.0)] * 32, chain)     # 11: the first group writes joint 0 twenty-five times
    for at in (0, 2, 3):                                              # 3 .. 6 on the first, a middle and the last constraint, before any pair
        for bad in ((2, 3, Z, x, 1.0), (IK.AIM, 8, Z, x, 1.0), (IK.TWO_BONE, N, Z, x, 1.0), (IK.TWO_BONE, 1, Z, x, 1.0), (IK.AIM, 3, Z, x, NAN)):
            records = [reach, aim, aim, reach]
            records[at] = bad
            add([2, 2], records, chain)                               # (both groups are dependent inside: 3 .. 6 come first)
            add([1, 1, 1, 1], records, chain, posed=False)            # (... and before the state)
    add([16, 16], [(IK.TWO_BONE, 3 + 3 * l, Z, x, 1.0) for l in range(16)] + [(IK.AIM, 3 + 3 * l, Z, x, 1.0) for l in range(16)], comb)      # 0: 32 in two groups
    add([4] * 8, IK.comb_constraints(32, 5), comb)                    # 0: 8 x 4
    rng = np.random.default_rng(23)
    for k in range(200):
        parents = S.hierarchy(("random", "chain", "roots")[k % 3], int(rng.integers(3, 40)), 1000 + k)
        sizes = [int(s) for s in rng.integers(1, 5, int(rng.integers(1, 9)))]
        records = [(int(rng.integers(0, 2)), int(rng.integers(0, len(parents))), Z, x, 1.0) for _ in range(sum(sizes))]
        add(sizes, records, parents, posed=bool(k % 4))
    return out


# ---- what the GPU tests solve ----------------------------------------------------------------------------------------------------------------
def deepest(parents):
    depth = np.zeros(len(parents), np.int64)
    for j, p in enumerate(parents):
        depth[j] = 0 if p < 0 else depth[p] + 1
    return int(np.argmax(depth)), depth


def reach_then_aim(parents, seed, extra=0):
    """three groups on any rig with a joint two levels down: group 0 a reach on the deepest joint t beside `extra` chains that are
    independent of it, group 1 an aim of t (it reads what the reach wrote and writes what the reach read), group 2 an aim of the reach's
    root (it rewrites a joint of group 0 once more)"""
    rng = np.random.default_rng(seed)
    t, depth = deepest(parents)
    assert depth[t] >= 2
    vec = lambda: tuple(float(F(v)) for v in rng.uniform(-2, 2, 3))
    first = [(IK.TWO_BONE, t, vec(), vec(), 1.0)]
    for _ in range(10000):
        if len(first) == 1 + extra:
            break
        c = (int(rng.integers(0, 2)), int(rng.integers(0, len(parents))), vec(), vec(), IK.WEIGHTS[len(first) % len(IK.WEIGHTS)])
        if IK.validate(first + [c], parents, True)[0] == 0:
            first.append(c)
    a = int(parents[parents[t]])
    return [first, [(IK.AIM, t, vec(), vec(), 0.75)], [(IK.AIM, a, vec(), vec(), 1.0)]]


def comb_reach_then_aim(seed, sizes=(16, 16)):
    """the 65-joint comb: a reach on every limb, then an aim of every limb's tip -- 32 constraints, cut into groups of `sizes`: any cut that
    keeps a limb's aim in a later group than its reach passes the check"""
    rng = np.random.default_rng(seed)
    vec = lambda lo, hi: tuple(float(F(v)) for v in rng.uniform(lo, hi, 3))
    records = [(IK.TWO_BONE, 3 + 3 * l, vec(-3, 3), vec(-3, 3), IK.WEIGHTS[l % len(IK.WEIGHTS)]) for l in range(16)]
    records += [(IK.AIM, 3 + 3 * l, vec(-3, 3), vec(-1, 1), IK.WEIGHTS[(l + 2) % len(IK.WEIGHTS)]) for l in range(16)]
    return split(records, sizes)


def comb_25_and_seven(seed):
    """(25, 1, 1, 1, 1, 1, 1, 1): sixteen reaches and nine aims of teeth side by side, then seven aims of limb tips one after another"""
    rng = np.random.default_rng(seed)
    vec = lambda: tuple(float(F(v)) for v in rng.uniform(-3, 3, 3))
    first = [(IK.TWO_BONE, 3 + 3 * l, vec(), vec(), 1.0) for l in range(16)] + [(IK.AIM, 49 + k, vec(), vec(), 0.5) for k in range(9)]
    return [first] + [[(IK.AIM, 3 + 3 * l, vec(), vec(), 1.0)] for l in range(7)]


def aims_down_a_chain(seed, n=8):
    """n single aims down an n-joint chain, joint 0 first: each reads the W its parent got one stage earlier"""
    rng = np.random.default_rng(seed)
    vec = lambda: tuple(float(F(v)) for v in rng.uniform(-3, 3, 3))
    return S.hierarchy("chain", n, 0), [[(IK.AIM, j, vec(), vec(), 1.0)] for j in range(n)]


def two_reaches(seed):
    """two groups that write the same joints of the four-joint chain: the second reach starts from the first's result"""
    rng = np.random.default_rng(seed)
    vec = lambda: tuple(float(F(v)) for v in rng.uniform(-2, 2, 3))
    return S.hierarchy("chain", 4, 0), [[(IK.TWO_BONE, 3, vec(), vec(), 0.5)], [(IK.TWO_BONE, 3, vec(), vec(), 0.75)]]


def skeleton_rigs():
    """(name, parents, grouped list): the four-joint chain, reach then aim; the comb; random trees at the edges of rt_crowd_block (64, 65,
    128, 129, 256, 257), at RT_SKELETON_LDS_JOINTS and one joint above it, where the call falls back to the loop"""
    x = (1.0, 0.5, 0.0)
    out = [("chain 4", S.hierarchy("chain", 4, 0), [[(IK.TWO_BONE, 3, (0.9, 0.4, -0.3), (0.0, 2.0, 1.0), 1.0)], [(IK.AIM, 3, (0.2, -1.0, 0.7), x, 1.0)]]),
           ("comb 65", IK.comb(), comb_reach_then_aim(41))]
    for n in (64, 65, 128, 129, 256, 257, CI.LDS, CI.LDS + 1):
        parents = S.hierarchy("random", n, 500 + n)
        out.append(("random %d" % n, parents, reach_then_aim(parents, 600 + n, extra=5)))
    return out


def values(n_actors, n, seed):
    """crowd_ik_cases.values with every actor's weights started two steps further into WEIGHTS: actor 0's first constraint has weight 1,
    not 0 -- a reach of weight 0 on a unit pose writes what it read, and the groups behind it would be the only ones"""
    targets, poles, _ = CI.values(n_actors, n, seed)
    weights = np.array([[IK.WEIGHTS[(a + k + 2) % len(IK.WEIGHTS)] for k in range(n)] for a in range(n_actors)], F)
    return targets, poles, weights


def actor_groups(groups, targets, poles, weights, a):
    """the grouped list rt_skeleton_solve_ik_groups takes for actor a of a crowd: crowd_ik_cases.constraints_of over the whole list, cut as
    the crowd's list is"""
    return split(CI.constraints_of(flat(groups), targets, poles, weights, a), sizes_of(groups))
