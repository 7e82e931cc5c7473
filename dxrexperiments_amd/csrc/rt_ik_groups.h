// rt_ik_groups.h -- the host side of an ordered list of IK groups (rt_skeleton_solve_ik_groups, rt_crowd_set_ik_chain_groups; include/dxr_amd.h
// "Posed skeletons", inverse kinematics, groups): the check of a grouped list, the text of the refusals it adds and the group ends that
// travel by value beside the packed table.  A grouped list is n_groups groups in order over ONE array of constraints: within a group the
// constraints are independent by the rule of rt_skeleton_validate_ik, across groups anything goes.  The check of a constraint, the walk that
// finds a dependent pair, the text of codes 1 .. 8 and the packed table are rt_skeleton.h's, reused unchanged.  Host code without HIP, as
// rt_crowd_ik.h is: tests/cpp/ik_groups_sanitized.cpp compiles it alone.
#pragma once

#include "rt_skeleton.h"

// 0: the groups describe one solve of a skeleton of n_joints joints with these parents, posed or not.  Else what is wrong, in this order:
//   1  a null array
//   9  n_groups outside 1 .. RT_SKELETON_MAX_IK_GROUPS (group_sizes is not read)
//   10 a group of size 0 (bad[3]: the group)
//   2  the total outside 1 .. RT_SKELETON_MAX_IK (no constraint is read)
//   3 .. 6 of rt_skeleton_validate_ik, every constraint of the whole list held to them in list order (bad[0]: its list index; bad[2]: the
//      joint of 4 and 5)
//   11 two constraints of ONE group of which one writes a joint the other reads: the groups in order, within a group the walk of
//      rt_skeleton_validate_ik's code 7 (bad[0]: the writer, bad[1]: the reader, both list indices; bad[2]: the joint; bad[3]: the group)
//   8  a skeleton without a pose (a crowd's list needs none: `posed` is then taken as true)
// 1, 2, 9, 10, 11 and 3 .. 6 are the caller's arguments (RT_ERR_INVALID_ARG), 8 the skeleton's state (RT_ERR_STATE).  *total (may be null)
// is the sum of the sizes once 9 and 10 have passed, saturated at 2^32 - 1.  Reads n_groups entries of `group_sizes` and `total` entries of
// `constraints`; `bad` may be null.
static inline int rt_ik_groups_validate(uint32_t n_groups, const uint32_t *group_sizes, const rt_skeleton_ik *constraints, uint32_t n_joints, const int32_t *parents,
                                        bool posed, uint32_t *total, uint32_t bad[4])
{
    uint32_t none[4], sum;
    if (!bad) bad = none;
    if (!total) total = &sum;
    bad[0] = bad[1] = bad[2] = bad[3] = 0u;
    *total = 0u;
    if (!group_sizes || !constraints || !parents) return 1;
    if (n_groups < 1u || n_groups > RT_SKELETON_MAX_IK_GROUPS) return 9;
    uint64_t n = 0;
    for (uint32_t g = 0; g < n_groups; g++) {
        if (group_sizes[g] == 0u) {
            bad[3] = g;
            return 10;
        }
        n += group_sizes[g];
    }
    *total = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
    if (n > RT_SKELETON_MAX_IK) return 2;                // (n >= 1: no group is empty)
    // the whole list: 3 .. 6 come before any pair; what it says of pairs (7) and of the pose (8) is not this list's answer
    const int each = rt_skeleton_validate_ik((uint32_t)n, constraints, n_joints, parents, true, bad);
    if (each >= 3 && each <= 6) return each;
    bad[0] = bad[1] = bad[2] = 0u;
    uint32_t first = 0;
    for (uint32_t g = 0; g < n_groups; g++) {            // a group's own sub-list: the independence walk, its indices shifted back
        uint32_t pair[3];
        if (rt_skeleton_validate_ik(group_sizes[g], constraints + first, n_joints, parents, true, pair) == 7) {
            bad[0] = first + pair[0]; bad[1] = first + pair[1]; bad[2] = pair[2]; bad[3] = g;
            return 11;
        }
        first += group_sizes[g];
    }
    return posed ? 0 : 8;
}

// The refusal behind a code of rt_ik_groups_validate under the name `who` of the call that asked, written into out[size]: 9 .. 11 in the
// text below, every other code in rt_skeleton_ik_refusal's with `total` for the count.  `constraints` is the list the check read (entry
// bad[0] is read for 3 only).  Returns the error class.
static inline int rt_ik_groups_refusal(int what, const char *who, uint32_t n_groups, uint32_t total, const rt_skeleton_ik *constraints, const uint32_t bad[4],
                                       uint32_t n_joints, const char *noun, const char *hint, char *out, size_t size)
{
    switch (what) {
    case 9: snprintf(out, size, "%s: %u groups: 1 .. %u are supported", who, n_groups, RT_SKELETON_MAX_IK_GROUPS); break;
    case 10: snprintf(out, size, "%s: group %u is empty: every group holds at least one constraint", who, bad[3]); break;
    case 11:
        snprintf(out, size, "%s: constraints %u and %u of group %u depend on one another: constraint %u writes joint %u, which constraint %u reads (its joint or an ancestor of it); put the reader in a later group",
                 who, bad[0], bad[1], bad[3], bad[0], bad[2], bad[1]);
        break;
    default: return rt_skeleton_ik_refusal(what, who, total, constraints, bad, n_joints, noun, hint, out, size);
    }
    return RT_ERR_INVALID_ARG;
}

// Where the groups of a checked list end, as the kernel takes them: byte g of the result is the list index one past group g's last
// constraint (at most RT_SKELETON_MAX_IK = 32, so a byte holds it); the bytes behind the last group repeat the total.  Eight groups are
// eight bytes: one 64-bit kernel argument beside the table.
static inline uint64_t rt_ik_group_ends(uint32_t n_groups, const uint32_t *group_sizes)
{
    uint64_t ends = 0, end = 0;
    for (uint32_t g = 0; g < RT_SKELETON_MAX_IK_GROUPS; g++) {
        if (g < n_groups) end += group_sizes[g];
        ends |= end << (8u * g);
    }
    return ends;
}

// ... and back: the sizes of the n_groups groups whose ends these are
static inline void rt_ik_group_sizes(uint64_t ends, uint32_t n_groups, uint32_t *group_sizes)
{
    uint32_t before = 0;
    for (uint32_t g = 0; g < n_groups; g++) {
        const uint32_t end = (uint32_t)(ends >> (8u * g)) & 0xFFu;
        group_sizes[g] = end - before;
        before = end;
    }
}
