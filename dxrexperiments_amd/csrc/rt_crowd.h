// rt_crowd.h -- the host side of a crowd (rt_crowd_create, rt_crowd_set_times, rt_crowd_set_blend, rt_crowd_set_layout; include/dxr_amd.h
// "Posed skeletons", crowds): the check of every actor's layer list, the table of layer records that one upload carries to k_crowd_pose, the
// slots of a layout (rt_crowd_set_layout) from which k_crowd_pose makes the same records itself, and the block width and LDS a rig needs.
// Host code without HIP, as rt_skeleton.h is: tests/cpp/crowd_sanitized.cpp and tests/cpp/crowd_layout_sanitized.cpp compile it alone.
#pragma once

#include "rt_skeleton.h"

// LDS of k_crowd_pose, sized by the rig: W component major, 12 rows of n_joints floats, the level table (n_joints words) and the level
// offsets (at most n_joints + 1 words): 56 B a joint + 4 -- 3.5 KiB for 64 joints, so that some forty blocks of small actors share the
// 160 KiB of a CU, where the 56 KiB that k_skeleton_pose declares for any rig would admit two.
static inline size_t rt_crowd_lds_bytes(uint32_t n_joints) { return 56u * (size_t)n_joints + 4u; }

// ... and of its device form (rt_crowd_set_blend_device), where the actor's n_layers layer records (56 B each: five pointers, so 8-byte
// aligned) stand in LDS too.  They stand FIRST, at the base of the block's LDS, and the layout above follows them at a multiple of 8 bytes:
// behind it they would start at 56 n_joints + 4, which no rig aligns.  At most 448 B more: 64 joints and 8 layers take 4036 B, still forty
// blocks to a CU, and the waves of a CU run out before its LDS does.
static inline size_t rt_crowd_lds_bytes_device(uint32_t n_joints, uint32_t n_layers) { return 56u * (size_t)n_layers + rt_crowd_lds_bytes(n_joints); }

// Lanes of the block that poses one actor: the smallest of 64, 128 and 256 that covers the JOINT COUNT (phases 0 and 2 stride over all the
// joints, whatever the widest level is; DESIGN.md section 7 has the three widths side by side: at 64 joints they cannot be told apart).  A block of one wave meets at barriers that cost it
// nothing; the barriers stay, so that the three widths run the same statements.
// -DRT_CROWD_BLOCK=64, 128 or 256 forces one width whatever the rig (measurements only; the bytes are the same).
#ifndef RT_CROWD_BLOCK
#define RT_CROWD_BLOCK 0u
#endif
static inline uint32_t rt_crowd_block(uint32_t n_joints)
{
    if (RT_CROWD_BLOCK == 64u || RT_CROWD_BLOCK == 128u || RT_CROWD_BLOCK == 256u) return RT_CROWD_BLOCK;
    return n_joints <= 64u ? 64u : n_joints <= 128u ? 128u : 256u;
}

// A clip and the masks of the crowd's skeleton as the packing reads them: host times, device keys
struct rt_crowd_clip {
    uint32_t n_keys;
    const float *times;          // host, n_keys
    const float *keys;           // device, float[n_keys][10][n_joints]
    const float *d_times;        // device, n_keys: the copy a layout's slots name (rt_crowd_pack_slots alone reads this member)
};

// 0: `layers` (n_actors x n_layers, actor major) describes a blend of every actor of a crowd whose skeleton has n_clips clips and n_masks
// masks, posed or not.  Else the code of rt_skeleton_validate_layers, to which every actor's list is held UNCHANGED, and *bad_actor and
// *bad_layer name where (0 and 0 for 1 and 2).  Every actor is held to 3 .. 6, the caller's arguments, before any actor is held to 7 .. 9,
// the skeleton's and the crowd's state: the first pass asks with limits nothing can exceed and a pose, so only 1 .. 6 can answer; within a
// pass the first bad actor wins.  Reads n_actors * n_layers entries, and nothing when it says 1 or 2.
static inline int rt_crowd_validate_layers(uint32_t n_actors, uint32_t n_layers, const rt_skeleton_layer *layers, uint32_t n_clips, uint32_t n_masks, bool posed,
                                           uint32_t *bad_actor, uint32_t *bad_layer)
{
    uint32_t none;
    if (!bad_actor) bad_actor = &none;
    if (!bad_layer) bad_layer = &none;
    *bad_actor = *bad_layer = 0u;
    for (int pass = 0; pass < 2; pass++)
        for (uint32_t a = 0; a < n_actors; a++) {
            const rt_skeleton_layer *mine = layers ? layers + (size_t)a * n_layers : nullptr;
            const int what = pass == 0 ? rt_skeleton_validate_layers(n_layers, mine, 0xFFFFFFFFu, 0xFFFFFFFFu, true, bad_layer)
                                       : rt_skeleton_validate_layers(n_layers, mine, n_clips, n_masks, posed, bad_layer);
            if (what) {
                *bad_actor = what <= 2 ? 0u : a;
                return what;
            }
        }
    return 0;
}

// The table of a validated call: out[a * n_layers + k] is layer k of actor a (rt_skeleton_pack_layer: the segment of every sampled layer is
// found here, on the host, with rt_skeleton_segment).  `clips` has an entry per clip of the skeleton, `masks` a device pointer per mask.
static inline void rt_crowd_pack_layers(uint32_t n_actors, uint32_t n_layers, const rt_skeleton_layer *layers, uint32_t n_joints, const rt_crowd_clip *clips,
                                        const float *const *masks, rt_blend_layer *out)
{
    for (size_t e = 0; e < (size_t)n_actors * n_layers; e++) {
        const rt_skeleton_layer &l = layers[e];
        const uint32_t k = (uint32_t)(e % n_layers);
        const rt_crowd_clip *c = l.clip == RT_SKELETON_CURRENT_POSE ? nullptr : &clips[l.clip];
        const float *mask = k > 0u && l.mask != RT_SKELETON_NO_MASK ? masks[l.mask] : nullptr;
        rt_skeleton_pack_layer(l, k, n_joints, c ? c->n_keys : 0u, c ? c->times : nullptr, c ? c->keys : nullptr, mask, out[e]);
    }
}

// rt_crowd_set_times as rt_crowd_set_blend takes it: one layer per actor, without a mask ("one layer without a mask is rt_skeleton_set_time,
// bit for bit").  The base layer's weight is not read.
static inline void rt_crowd_layers_of_times(uint32_t n_actors, const uint32_t *clips, const float *times, rt_skeleton_layer *out)
{
    for (uint32_t a = 0; a < n_actors; a++) {
        out[a].clip = clips[a];
        out[a].time = times[a];
        out[a].weight = 1.0f;
        out[a].mask = RT_SKELETON_NO_MASK;
        out[a].mode = RT_LAYER_BLEND;
    }
}

// ---- layouts (rt_crowd_set_layout, rt_crowd_set_blend_device) ---------------------------------------------------------------------------------
// What the HOST decides of layer k of actor a, checked once and kept on the device: which clip (where its keys and its key times stand, and
// how many), which mask, which mode, and a weight for calls that bring none.  Every member that becomes an address is here; what a posing call
// then reads from the caller's device memory -- a time and a weight -- is arithmetic only.
struct rt_crowd_slot {
    const float *keys;           // device, float[n_keys][10][n_joints]; nullptr: RT_SKELETON_CURRENT_POSE (layer 0 only)
    const float *times;          // device, n_keys (nullptr with keys)
    const float *mask;           // device, float[n_joints], or nullptr: none (the base layer's mask is dropped)
    uint32_t n_keys, mode;
    float weight;                // the layout's: taken when rt_crowd_set_blend_device is given no weights
    uint32_t pad;
};

// rt_crowd_set_layout's copy of the caller's list: clip, weight, mask and mode of every entry, and every time 0 -- the caller's `time` is
// not read (a layout has none; rt_crowd_validate_layers then cannot say 6)
static inline void rt_crowd_layout_layers(size_t n, const rt_skeleton_layer *layers, rt_skeleton_layer *out)
{
    for (size_t e = 0; e < n; e++) {
        out[e].clip = layers[e].clip;
        out[e].time = 0.0f;
        out[e].weight = layers[e].weight;
        out[e].mask = layers[e].mask;
        out[e].mode = layers[e].mode;
    }
}

// The slots of a validated layout: out[a * n_layers + k] is layer k of actor a.  Reads clip, weight, mask and mode of every entry, never time.
static inline void rt_crowd_pack_slots(uint32_t n_actors, uint32_t n_layers, const rt_skeleton_layer *layers, const rt_crowd_clip *clips, const float *const *masks,
                                       rt_crowd_slot *out)
{
    for (size_t e = 0; e < (size_t)n_actors * n_layers; e++) {
        const rt_skeleton_layer &l = layers[e];
        const rt_crowd_clip *c = l.clip == RT_SKELETON_CURRENT_POSE ? nullptr : &clips[l.clip];
        rt_crowd_slot s = rt_crowd_slot();
        s.keys = c ? c->keys : nullptr;
        s.times = c ? c->d_times : nullptr;
        s.n_keys = c ? c->n_keys : 0u;
        s.mask = e % n_layers > 0u && l.mask != RT_SKELETON_NO_MASK ? masks[l.mask] : nullptr;
        s.mode = l.mode;
        s.weight = l.weight;
        out[e] = s;
    }
}

// The record of a slot at time t with weight w: rt_skeleton_pack_layer of the layer the slot was packed from, with that time and weight,
// word for word -- both are rt_skeleton_sample_layer.  Reads s.times (n_keys of them) where the slot samples: device memory in k_crowd_pose.
RT_HOST_DEVICE static inline void rt_crowd_layer_of_slot(const rt_crowd_slot &s, uint32_t n_joints, float t, float w, rt_blend_layer &b)
{
    rt_skeleton_sample_layer(n_joints, s.n_keys, s.times, s.keys, t, w, s.mode, s.mask, b);
}
