// rt_attach.h -- the host side of attached instances (rt_scene_attach_instances, include/dxr_amd.h "Attached instances"): validation of the
// caller's arrays, the word a binding is kept in on the device, and the search of a range for an attached instance that the transform setters
// refuse by.  Host code without HIP, as rt_skeleton.h is: tests/cpp/attach_sanitized.cpp compiles it alone.
#pragma once

#include <stddef.h>
#include <stdint.h>

// A binding as k_gather_transforms reads it, one word per instance: the joint in the low 16 bits (a joint is below RT_SKELETON_MAX_JOINTS =
// 65536), RT_ATTACH_BOUND for an attached instance, RT_ATTACH_LOCAL for one whose local matrix is multiplied in.  0: not attached.
#define RT_ATTACH_JOINT_MASK 0xFFFFu
#define RT_ATTACH_BOUND 0x40000000u
#define RT_ATTACH_LOCAL 0x80000000u

// 0: instances first .. first + count - 1 of a scene of n_instances may be attached to `joints` of a skeleton of n_joints.  Else what is
// wrong: 1 a null array (joints; a null `local3x4` is legal), 2 a range beyond the instances, 3 a joint >= n_joints -- then *bad_entry names
// the first such entry of `joints`.  A count of 0 reads nothing and is 0, or 2 when `first` lies beyond the instances.
static inline int rt_attach_validate(uint32_t n_instances, uint32_t first, uint32_t count, uint32_t n_joints, const uint32_t *joints, uint32_t *bad_entry)
{
    if (!joints && count != 0u) return 1;
    if (first > n_instances || count > n_instances - first) return 2;
    for (uint32_t k = 0; k < count; k++)
        if (joints[k] >= n_joints) {
            if (bad_entry) *bad_entry = k;
            return 3;
        }
    return 0;
}

// the words of `count` validated bindings
static inline void rt_attach_pack(uint32_t count, const uint32_t *joints, bool has_local, uint32_t *words)
{
    for (uint32_t k = 0; k < count; k++) words[k] = (joints[k] & RT_ATTACH_JOINT_MASK) | RT_ATTACH_BOUND | (has_local ? RT_ATTACH_LOCAL : 0u);
}

// true, and *which the first of them, if some instance of first .. first + count - 1 (a validated range) is attached; `words` may be null or
// hold fewer than first + count entries: instances added after the last attachment have none
static inline bool rt_attach_range_holds(const uint32_t *words, size_t n_words, uint32_t first, uint32_t count, uint32_t *which)
{
    for (uint32_t k = 0; k < count; k++) {
        const size_t i = (size_t)first + k;
        if (words && i < n_words && (words[i] & RT_ATTACH_BOUND)) {
            if (which) *which = (uint32_t)i;
            return true;
        }
    }
    return false;
}
