// rt_skeleton.h -- the host side of a skeleton (rt_skeleton_create, rt_skeleton_add_clip, rt_skeleton_set_time, rt_skeleton_set_blend):
// validation of the caller's arrays, the level table k_skeleton_pose walks, the segment search of a clip, the check of a layer list and the
// text of its refusals (a skeleton's and a crowd's alike: tests/cpp/layer_refusals_sanitized.cpp holds it to what both used to say), the
// record a validated layer is packed into (shared with rt_crowd.h), the check of a list of IK constraints (rt_skeleton_solve_ik,
// rt_crowd_set_ik_chains), the text of its refusals and the table a checked list is packed into, which both IK kernels take by value.  Host
// code without HIP, as rt_skin.h is: tests/cpp/skeleton_sanitized.cpp, tests/cpp/skeleton_blend_sanitized.cpp, tests/cpp/ik_sanitized.cpp
// and tests/cpp/crowd_ik_sanitized.cpp compile it alone.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../include/dxr_amd_types.h"     // rt_skeleton_layer, rt_skeleton_ik and their constants
#include "rt_xform.h"                        // RT_HOST_DEVICE: the segment and the layer record are found by ONE text, on the host and in k_crowd_pose

#define RT_SKELETON_MAX_JOINTS 65536u    // the skin's bone limit (RT_SKIN_MAX_BONES): a joint is a bone, and fits 16 bits
#define RT_SKELETON_POSE_FLOATS 10u      // a joint of a pose: tx ty tz  qx qy qz qw  sx sy sz
#define RT_SKELETON_BLOCK 256u           // lanes of the one block that poses a skeleton

// Skeletons of up to this many joints are posed with the world matrices W in LDS: 48 B per joint, component major (12 rows of this many
// floats, so that the lanes of a wave that read their parents' entries read 64 different banks on a chain and one broadcast word on a star),
// and beside them the level table and the level offsets, 4 B per joint each.  1024 joints take 48 KiB + 8 KiB = 56 KiB, inside the 64 KiB a
// block may declare on every CDNA part and about a third of the 160 KiB of an MI355X CU: the one block of the pose kernel leaves room for the
// skin kernel's blocks of 12 KiB that run on the same CU behind it.  A character has 50 - 300 joints and a crowd rig that shares one skeleton a few times that; what is
// above 1024 is a stress case, and it keeps W in the joints' global array (L2 resident: 3 MiB at 65536 joints), at a global round trip per
// level instead of an LDS one.
#define RT_SKELETON_LDS_JOINTS 1024u

// 0: the arguments describe a hierarchy.  Else what is wrong: 1 a null array, 2 n_joints outside 1 .. 65536, 3 a parent that is neither -1
// nor < its joint (parents come before children) -- then *bad_joint names the first such joint.  Reads n_joints entries of `parents`.
static inline int rt_skeleton_validate(uint32_t n_joints, const int32_t *parents, const float *inverse_bind, uint32_t *bad_joint)
{
    if (!parents || !inverse_bind) return 1;
    if (n_joints < 1u || n_joints > RT_SKELETON_MAX_JOINTS) return 2;
    for (uint32_t j = 0; j < n_joints; j++)
        if (parents[j] < -1 || (int64_t)parents[j] >= (int64_t)j) {
            if (bad_joint) *bad_joint = j;
            return 3;
        }
    return 0;
}

// The level table of a validated hierarchy.  The level of a root is 0, of any other joint its parent's + 1.  `order`: the joints in level
// order, ascending by index within a level (n_joints entries); `level_offsets`: level l owns order[level_offsets[l]] ..
// order[level_offsets[l + 1] - 1] (levels + 1 entries, the last one n_joints).  Returns the number of levels.
static inline uint32_t rt_skeleton_levels(uint32_t n_joints, const int32_t *parents, std::vector<uint32_t> &order, std::vector<uint32_t> &level_offsets)
{
    std::vector<uint32_t> level(n_joints, 0u);
    uint32_t n_levels = 0;
    for (uint32_t j = 0; j < n_joints; j++) {           // (parents come first: one pass)
        level[j] = parents[j] < 0 ? 0u : level[(uint32_t)parents[j]] + 1u;
        if (level[j] + 1u > n_levels) n_levels = level[j] + 1u;
    }
    level_offsets.assign((size_t)n_levels + 1u, 0u);
    for (uint32_t j = 0; j < n_joints; j++) level_offsets[level[j] + 1u]++;
    for (uint32_t l = 0; l < n_levels; l++) level_offsets[l + 1u] += level_offsets[l];
    std::vector<uint32_t> at(level_offsets.begin(), level_offsets.end() - 1);
    order.assign(n_joints, 0u);
    for (uint32_t j = 0; j < n_joints; j++) order[at[level[j]]++] = j;       // (ascending j: stable within a level)
    return n_levels;
}

// The table as k_skeleton_pose reads it: entry k = order[k] | parent << 16 (a joint and its parent both fit 16 bits; a root's parent field
// is 0xFFFF, which no joint can have for a parent: parent < joint <= 65535).
static inline void rt_skeleton_pack_table(const int32_t *parents, const std::vector<uint32_t> &order, std::vector<uint32_t> &table)
{
    table.resize(order.size());
    for (size_t k = 0; k < order.size(); k++) {
        const int32_t p = parents[order[k]];
        table[k] = order[k] | ((p < 0 ? 0xFFFFu : (uint32_t)p) << 16);
    }
}

// 0: the key times of a clip.  Else: 1 a null array, 2 n_keys == 0, 3 a time that is not finite, 4 a time that is not above the one before
// it (the times ascend strictly) -- for 3 and 4 *bad_key names the first such key.
static inline int rt_skeleton_validate_times(uint32_t n_keys, const float *times, uint32_t *bad_key)
{
    if (!times) return 1;
    if (n_keys == 0u) return 2;
    for (uint32_t k = 0; k < n_keys; k++) {
        if (!isfinite(times[k])) {
            if (bad_key) *bad_key = k;
            return 3;
        }
        if (k > 0u && !(times[k] > times[k - 1u])) {
            if (bad_key) *bad_key = k;
            return 4;
        }
    }
    return 0;
}

// The segment of validated key times that holds t (not NaN), and where t stands in it: one key, or t at or before the first, gives (0, 0);
// t at or beyond the last (n_keys - 2, 1); otherwise i is the largest key with times[i] <= t and a = (t - times[i]) / (times[i + 1] -
// times[i]), two fp32 differences and one fp32 quotient.
// The host never hands it a NaN (every host call refuses one), but rt_crowd_set_blend_device reads its times from device memory unseen, so
// what a NaN does is part of the statement: with one key, (0, 0); otherwise both range tests are false, every comparison of the search is
// false, so hi comes down to 1 and lo stays 0: (0, NaN).  Whatever the 32 bits of t, every read is times[0 .. n_keys - 1] and i <= n_keys - 2
// (0 with one key): the two keys a record names exist.
RT_HOST_DEVICE static inline void rt_skeleton_segment(uint32_t n_keys, const float *times, float t, uint32_t *i_out, float *a_out)
{
    if (n_keys == 1u || t <= times[0]) { *i_out = 0u; *a_out = 0.0f; return; }
    if (t >= times[n_keys - 1u]) { *i_out = n_keys - 2u; *a_out = 1.0f; return; }
    uint32_t lo = 0u, hi = n_keys - 1u;                  // times[lo] <= t < times[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (times[mid] <= t) lo = mid; else hi = mid;
    }
    const float num = t - times[lo], den = times[lo + 1u] - times[lo];
    *i_out = lo;
    *a_out = num / den;
}

// 0: the layers describe a blend of a skeleton with n_clips clips and n_masks masks that is posed or not.  Else what is wrong, and
// *bad_layer names the first such layer (0 for 1 and 2): 1 a null array, 2 n_layers outside 1 .. RT_SKELETON_MAX_LAYERS, 3 an unknown mode,
// 4 an additive layer 0, 5 RT_SKELETON_CURRENT_POSE on a layer other than 0, 6 a NaN time on a layer that samples, 7 an unknown clip,
// 8 an unknown mask (the base layer's mask is not read, and not checked), 9 RT_SKELETON_CURRENT_POSE on a skeleton without a pose.  1 .. 6
// are the caller's arguments (RT_ERR_INVALID_ARG), 7 .. 9 the skeleton's state (RT_ERR_STATE); every layer is held to 3 .. 6 before any
// layer is held to 7 .. 9.  Reads n_layers entries of `layers`, and nothing when it says 1 or 2.
static inline int rt_skeleton_validate_layers(uint32_t n_layers, const rt_skeleton_layer *layers, uint32_t n_clips, uint32_t n_masks, bool posed,
                                              uint32_t *bad_layer)
{
    if (bad_layer) *bad_layer = 0u;
    if (!layers) return 1;
    if (n_layers < 1u || n_layers > RT_SKELETON_MAX_LAYERS) return 2;
    for (uint32_t k = 0; k < n_layers; k++) {
        const rt_skeleton_layer &l = layers[k];
        int what = 0;
        if (l.mode != RT_LAYER_BLEND && l.mode != RT_LAYER_ADDITIVE) what = 3;
        else if (k == 0u && l.mode != RT_LAYER_BLEND) what = 4;
        else if (k > 0u && l.clip == RT_SKELETON_CURRENT_POSE) what = 5;
        else if (l.clip != RT_SKELETON_CURRENT_POSE && isnan(l.time)) what = 6;
        if (what) {
            if (bad_layer) *bad_layer = k;
            return what;
        }
    }
    for (uint32_t k = 0; k < n_layers; k++) {
        const rt_skeleton_layer &l = layers[k];
        int what = 0;
        if (l.clip == RT_SKELETON_CURRENT_POSE) what = posed ? 0 : 9;
        else if (l.clip >= n_clips) what = 7;
        if (!what && k > 0u && l.mask != RT_SKELETON_NO_MASK && l.mask >= n_masks) what = 8;
        if (what) {
            if (bad_layer) *bad_layer = k;
            return what;
        }
    }
    return 0;
}

// The refusal behind a code 1 .. 9 of rt_skeleton_validate_layers, in the ONE text that rt_skeleton_set_blend, rt_crowd_set_blend and
// rt_crowd_set_layout answer with: written into out[size] under the name `who` of the call that asked.  `actor`: null for a skeleton, else the
// bad actor of a crowd, named in front of what is wrong with a layer (3 .. 9; 1 and 2 name none).  `bad` is the bad layer and `l` its record (read for 3, 7 and
// 8 only).  `noun` and `hint` are the pose source's own (rt_pose_source, rt_internal.h).  Returns the error class: RT_ERR_INVALID_ARG for
// 1 .. 6, RT_ERR_STATE for 7 .. 9.
static inline int rt_skeleton_layers_refusal(int what, const char *who, const uint32_t *actor, uint32_t bad, const rt_skeleton_layer *l, uint32_t n_layers,
                                             uint32_t n_clips, uint32_t n_masks, const char *noun, const char *hint, char *out, size_t size)
{
    char at[24] = "";                                    // "actor 4294967295: " is 18
    if (actor) snprintf(at, sizeof at, "actor %u: ", *actor);
    switch (what) {
    case 1: snprintf(out, size, "%s: null argument", who); break;
    case 2: snprintf(out, size, "%s: %u layers: 1 .. %u are supported", who, n_layers, RT_SKELETON_MAX_LAYERS); break;
    case 3: snprintf(out, size, "%s: %slayer %u has mode %u: RT_LAYER_BLEND (0) or RT_LAYER_ADDITIVE (1)", who, at, bad, l->mode); break;
    case 4: snprintf(out, size, "%s: %slayer 0 is additive: the base layer is RT_LAYER_BLEND", who, at); break;
    case 5: snprintf(out, size, "%s: %slayer %u names RT_SKELETON_CURRENT_POSE: only layer 0 may", who, at, bad); break;
    case 6: snprintf(out, size, "%s: %sthe time of layer %u is NaN", who, at, bad); break;
    case 7: snprintf(out, size, "%s: %slayer %u names clip %u: the skeleton has %u (rt_skeleton_add_clip adds one)", who, at, bad, l->clip, n_clips); break;
    case 8: snprintf(out, size, "%s: %slayer %u names mask %u: the skeleton has %u (rt_skeleton_add_mask adds one)", who, at, bad, l->mask, n_masks); break;
    default: snprintf(out, size, "%s: %slayer %u names RT_SKELETON_CURRENT_POSE: the %s has no pose yet (%s)", who, at, bad, noun, hint); break;
    }
    return what <= 6 ? RT_ERR_INVALID_ARG : RT_ERR_STATE;
}

// A validated layer as the kernels read it (rt_pose_device.h: blend_joint, blend_layer).  k_skeleton_blend takes up to
// RT_SKELETON_MAX_LAYERS of them by value, as its argument; k_crowd_pose reads n_layers of them per actor from a table in device memory,
// through addresses that are uniform over the block.  Either way they come by scalar loads.
struct rt_blend_layer {
    const float *key_a, *key_b;          // the two keys about the layer's time (layer 0: nullptr = the pose that is held) ...
    const float *ref_a, *ref_b;          // ... and the clip's first two keys: the reference pose of an additive layer is sampled from them at a = 0
    const float *mask;                   // float[n_joints], or nullptr: none
    float a, weight;
    uint32_t mode, pad;
};

// The sampling half of a layer record: the segment of `t` in the clip's `times` (n_keys of them; read HERE, so host memory for a host
// caller and the clip's device copy inside k_crowd_pose), the two keys about it and the clip's first two in `keys` (device memory,
// float[n_keys][10][n_joints], never dereferenced), weight, mode and mask.  keys == nullptr is RT_SKELETON_CURRENT_POSE: key_a stays null and
// nothing is read.  ONE text for rt_skeleton_pack_layer, whose times the host validated, and for the kernel, whose times and weights are
// any 32 bits (rt_skeleton_segment says what a NaN does).
RT_HOST_DEVICE static inline void rt_skeleton_sample_layer(uint32_t n_joints, uint32_t n_keys, const float *times, const float *keys, float t, float weight,
                                                           uint32_t mode, const float *mask, rt_blend_layer &b)
{
    const size_t per_key = RT_SKELETON_POSE_FLOATS * (size_t)n_joints;
    b = rt_blend_layer();
    b.weight = weight;
    b.mode = mode;
    if (!keys) return;                                   // (layer 0 only: the kernel starts from the pose that is held)
    uint32_t i = 0;
    rt_skeleton_segment(n_keys, times, t, &i, &b.a);
    b.ref_a = keys;
    b.ref_b = n_keys == 1u ? b.ref_a : b.ref_a + per_key;
    b.key_a = b.ref_a + per_key * i;
    b.key_b = n_keys == 1u ? b.key_a : b.key_a + per_key;
    b.mask = mask;
}

// Layer k of a validated list, packed.  `times` (n_keys of them) and `keys` (device memory, float[n_keys][10][n_joints]) are the layer's
// clip -- not read for RT_SKELETON_CURRENT_POSE, where key_a stays null -- and `mask` the layer's mask in device memory or nullptr; the base
// layer's mask is dropped.  The segment (i, a) is found here, on the host, by rt_skeleton_sample_layer; no pointer is dereferenced but `times`.
static inline void rt_skeleton_pack_layer(const rt_skeleton_layer &l, uint32_t k, uint32_t n_joints, uint32_t n_keys, const float *times, const float *keys,
                                          const float *mask, rt_blend_layer &b)
{
    const bool held = l.clip == RT_SKELETON_CURRENT_POSE;
    rt_skeleton_sample_layer(n_joints, n_keys, times, held ? nullptr : keys, l.time, l.weight, l.mode, k > 0u && l.mask != RT_SKELETON_NO_MASK ? mask : nullptr, b);
}

// 0: the constraints describe one solve of a skeleton of n_joints joints with these parents, posed or not.  Else what is wrong, and bad[0]
// names the first such constraint (0 for 1 and 2): 1 a null array, 2 n outside 1 .. RT_SKELETON_MAX_IK, 3 an unknown kind, 4 a joint
// >= n_joints, 5 a two-bone tip with fewer than two ancestors (bad[2]: the joint), 6 a NaN weight, 7 two constraints that are not
// independent, 8 a skeleton without a pose.  1 .. 7 are the caller's arguments (RT_ERR_INVALID_ARG), 8 the skeleton's state (RT_ERR_STATE);
// every constraint is held to 3 .. 6, in that order, before any pair is held to 7, and 7 before 8.
// Independence: a two-bone constraint WRITES the parent b of its tip and b's parent a, an aim its joint; every constraint READS its joint and
// all of that joint's ancestors.  For 7 the readers are walked in order, each from its joint up to its root; the first joint met that another
// constraint writes is bad[2], the reader bad[1], the lowest such writer bad[0].  (Two constraints that write the same joint are caught by
// this: a constraint reads what it writes.)  Reads n entries of `constraints`, and nothing when it says 1 or 2; `bad` may be null.
static inline int rt_skeleton_validate_ik(uint32_t n, const rt_skeleton_ik *constraints, uint32_t n_joints, const int32_t *parents, bool posed, uint32_t bad[3])
{
    uint32_t none[3];
    if (!bad) bad = none;
    bad[0] = bad[1] = bad[2] = 0u;
    if (!constraints || !parents) return 1;
    if (n < 1u || n > RT_SKELETON_MAX_IK) return 2;
    for (uint32_t k = 0; k < n; k++) {
        const rt_skeleton_ik &c = constraints[k];
        int what = 0;
        if (c.kind != RT_IK_TWO_BONE && c.kind != RT_IK_AIM) what = 3;
        else if (c.joint >= n_joints) what = 4;
        else if (c.kind == RT_IK_TWO_BONE && (parents[c.joint] < 0 || parents[parents[c.joint]] < 0)) what = 5;
        else if (isnan(c.weight)) what = 6;
        if (what) {
            bad[0] = k;
            if (what == 4 || what == 5) bad[2] = c.joint;
            return what;
        }
    }
    uint32_t written[2u * RT_SKELETON_MAX_IK], writer[2u * RT_SKELETON_MAX_IK], n_written = 0;
    for (uint32_t k = 0; k < n; k++) {
        const rt_skeleton_ik &c = constraints[k];
        if (c.kind == RT_IK_TWO_BONE) {
            const uint32_t b = (uint32_t)parents[c.joint];
            written[n_written] = (uint32_t)parents[b]; writer[n_written++] = k;
            written[n_written] = b; writer[n_written++] = k;
        } else {
            written[n_written] = c.joint; writer[n_written++] = k;
        }
    }
    for (uint32_t k = 0; k < n; k++)
        for (int32_t j = (int32_t)constraints[k].joint; j >= 0; j = parents[j])
            for (uint32_t e = 0; e < n_written; e++)     // (ascending by writer)
                if (written[e] == (uint32_t)j && writer[e] != k) {
                    bad[0] = writer[e]; bad[1] = k; bad[2] = (uint32_t)j;
                    return 7;
                }
    return posed ? 0 : 8;
}

// The refusal behind a code 1 .. 8 of rt_skeleton_validate_ik, in the ONE text that rt_skeleton_solve_ik and rt_crowd_set_ik_chains answer
// with: written into out[size] under the name `who` of the call that asked.  `bad` is what the check filled in, `constraints` the list it
// read (entry bad[0] is read for 3 only).  `noun` and `hint` are the pose source's own (rt_pose_source, rt_internal.h; 8 only).  Returns the
// error class: RT_ERR_INVALID_ARG for 1 .. 7, RT_ERR_STATE for 8.
static inline int rt_skeleton_ik_refusal(int what, const char *who, uint32_t n, const rt_skeleton_ik *constraints, const uint32_t bad[3], uint32_t n_joints,
                                         const char *noun, const char *hint, char *out, size_t size)
{
    switch (what) {
    case 1: snprintf(out, size, "%s: null argument", who); break;
    case 2: snprintf(out, size, "%s: %u constraints: 1 .. %u are supported", who, n, RT_SKELETON_MAX_IK); break;
    case 3: snprintf(out, size, "%s: constraint %u has kind %u: RT_IK_TWO_BONE (0) or RT_IK_AIM (1)", who, bad[0], constraints[bad[0]].kind); break;
    case 4: snprintf(out, size, "%s: constraint %u names joint %u: the skeleton has %u", who, bad[0], bad[2], n_joints); break;
    case 5:
        snprintf(out, size, "%s: constraint %u names joint %u for the tip of a two-bone chain: it has fewer than two ancestors (the tip's parent is the middle joint, that joint's parent the chain's root)",
                 who, bad[0], bad[2]);
        break;
    case 6: snprintf(out, size, "%s: the weight of constraint %u is NaN", who, bad[0]); break;
    case 7:
        snprintf(out, size, "%s: constraints %u and %u are not independent: constraint %u writes joint %u, which constraint %u reads (its joint or an ancestor of it); solve them in two calls",
                 who, bad[0], bad[1], bad[0], bad[2], bad[1]);
        break;
    default: snprintf(out, size, "%s: the %s has no pose yet (%s)", who, noun, hint); break;
    }
    return what <= 7 ? RT_ERR_INVALID_ARG : RT_ERR_STATE;
}

// A constraint of a solve as the kernels read it -- the host has found the chain: tip c, middle b, root a of a two-bone reach (an aim: c is
// its joint; b and a repeat it) and the parent p of the joint whose space the target is carried into, -1 for a root of the skeleton -- and
// the table of them that travels by value as the kernel's argument, as k_skeleton_blend's table of layers does.  k_skeleton_ik reads all of
// an entry; k_crowd_ik reads the chain, and target, pole and weight from the actor's own values (pole and weight here are the defaults of
// rt_crowd_set_ik_chains, for a call that brings none).
struct IkEntry {
    uint32_t kind, c, b, a;
    int32_t p;
    float target[3], pole[3], weight;
};
struct IkTable {
    IkEntry e[RT_SKELETON_MAX_IK];
};

// The table of a list that rt_skeleton_validate_ik passed (codes 0 and 8: the pose is not its business), over the parents the check read:
// entries 0 .. n - 1; the rest of `table` is left as it is.
static inline void rt_skeleton_pack_ik(uint32_t n, const rt_skeleton_ik *constraints, const int32_t *parents, IkTable &table)
{
    for (uint32_t k = 0; k < n; k++) {
        const rt_skeleton_ik &c = constraints[k];
        IkEntry &e = table.e[k];
        e.kind = c.kind;
        e.c = e.b = e.a = c.joint;
        if (c.kind == RT_IK_TWO_BONE) {
            e.b = (uint32_t)parents[c.joint];
            e.a = (uint32_t)parents[e.b];
        }
        e.p = parents[e.a];
        for (int i = 0; i < 3; i++) {
            e.target[i] = c.target[i];
            e.pole[i] = c.pole[i];
        }
        e.weight = c.weight;
    }
}
