// rt_crowd_ik.h -- the host side of a crowd's inverse kinematics (rt_crowd_set_ik_chains, rt_crowd_solve_ik; include/dxr_amd.h "Posed
// skeletons", crowds): the copy of the caller's chain list that the check and the packing read, the check of an actor-major array of host
// weights, and the ONE block in which a host call's targets, poles and weights cross to the device.  The check of the list itself, the text
// of its refusals and the packed table are rt_skeleton.h's, shared with rt_skeleton_solve_ik.  Host code without HIP, as rt_crowd.h is:
// tests/cpp/crowd_ik_sanitized.cpp compiles it alone.
#pragma once

#include <string.h>

#include "rt_crowd.h"

// rt_crowd_set_ik_chains' copy of the caller's list: kind and joint of every entry, its pole and weight -- the defaults of a call that
// brings no poles or no weights -- and every target 0: the caller's `target` is not read (a chain has none; an actor brings its own).
static inline void rt_crowd_ik_chains(uint32_t n, const rt_skeleton_ik *chains, rt_skeleton_ik *out)
{
    for (uint32_t k = 0; k < n; k++) {
        out[k].kind = chains[k].kind;
        out[k].joint = chains[k].joint;
        for (int i = 0; i < 3; i++) {
            out[k].target[i] = 0.0f;
            out[k].pole[i] = chains[k].pole[i];
        }
        out[k].weight = chains[k].weight;
    }
}

// 0: no weight of `weights` (n_actors x n, actor major; null: none are brought, and nothing is read) is NaN.  Else 6, the code
// rt_skeleton_validate_ik gives a NaN weight, and *bad_actor and *bad_constraint name the first such entry, the first bad actor first.
// Targets and poles are taken as given, as on a skeleton: nothing looks at them.
static inline int rt_crowd_ik_check_values(uint32_t n_actors, uint32_t n, const float *weights, uint32_t *bad_actor, uint32_t *bad_constraint)
{
    uint32_t none;
    if (!bad_actor) bad_actor = &none;
    if (!bad_constraint) bad_constraint = &none;
    *bad_actor = *bad_constraint = 0u;
    if (!weights) return 0;
    for (size_t e = 0; e < (size_t)n_actors * n; e++)
        if (isnan(weights[e])) {
            *bad_actor = (uint32_t)(e / n);
            *bad_constraint = (uint32_t)(e % n);
            return 6;
        }
    return 0;
}

// Where the arrays of a host call stand in the one block that carries them, in floats from its base: the targets first (n_actors x n x 3),
// then the poles (as many; absent when the call brings none), then the weights (n_actors x n; likewise).  An absent array has offset 0 and
// `has` false: the kernel is then given a null pointer and takes the chain's default.
struct rt_crowd_ik_block {
    size_t poles, weights, floats;       // offsets of the two optional arrays, and the length of the block
    bool has_poles, has_weights;
};
static inline rt_crowd_ik_block rt_crowd_ik_layout(uint32_t n_actors, uint32_t n, bool has_poles, bool has_weights)
{
    const size_t e = (size_t)n_actors * n;
    rt_crowd_ik_block b;
    b.has_poles = has_poles;
    b.has_weights = has_weights;
    b.floats = 3u * e;
    b.poles = has_poles ? b.floats : 0u;
    if (has_poles) b.floats += 3u * e;
    b.weights = has_weights ? b.floats : 0u;
    if (has_weights) b.floats += e;
    return b;
}

// The block filled: `out` has b.floats floats.  Reads all of `targets`, and of `poles` and `weights` where the layout has them.
static inline void rt_crowd_ik_pack_values(uint32_t n_actors, uint32_t n, const rt_crowd_ik_block &b, const float *targets, const float *poles, const float *weights,
                                           float *out)
{
    const size_t e = (size_t)n_actors * n;
    memcpy(out, targets, sizeof(float) * 3u * e);
    if (b.has_poles) memcpy(out + b.poles, poles, sizeof(float) * 3u * e);
    if (b.has_weights) memcpy(out + b.weights, weights, sizeof(float) * e);
}
