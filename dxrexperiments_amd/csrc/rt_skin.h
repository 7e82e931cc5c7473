// rt_skin.h -- the skin of a model (rt_model_set_skin): validation of the caller's arrays and their packing into the layout k_skin_vertices
// (rt_model.hip) reads.  Host code without HIP, as rt_adjacency.h is: tests/cpp/skin_sanitized.cpp compiles it alone.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <vector>

#define RT_SKIN_MAX_INFLUENCES 8u
#define RT_SKIN_MAX_BONES 65536u         // a bone index is stored in 16 bits

// Palettes of up to this many bones are staged into LDS by every block of k_skin_vertices; larger ones are gathered from global memory.
// Two bounds, and the smaller one is taken.  Occupancy: a CU holds 32 waves, eight blocks of 256 lanes, and 160 KiB of LDS, so a block may take
// 20 KiB (426 bones of 48 B) before the LDS, and not the wave slots, decides how many blocks are resident -- and the kernel is a stream of
// loads that wants every wave it can get.  Traffic: a block of 256 vertices reads and writes 256 x 24 B each way, 12 KiB, and staging costs it
// another 48 B per bone from L2; at 256 bones the staging is as large as the block's own vertex traffic, and beyond that a block would move
// more palette than mesh in order to use, with K influences, at most 256 K entries of it.  256 bones = 12 KiB per block, 96 KiB for the eight
// blocks of a CU.
#define RT_SKIN_LDS_BONES 256u

// 0: the arguments describe a skin.  Else what is wrong: 1 a null array, 2 influences outside 1 .. 8, 3 n_bones outside 1 .. 65536,
// 4 an index >= n_bones -- then *bad_vertex / *bad_slot name the first such entry in vertex-major order.  Reads n_verts x influences
// entries of bone_indices and nothing else.
static inline int rt_skin_validate(uint32_t n_verts, uint32_t influences, uint32_t n_bones, const uint32_t *bone_indices, const float *weights,
                                   uint32_t *bad_vertex, uint32_t *bad_slot)
{
    if (!bone_indices || !weights) return 1;
    if (influences < 1u || influences > RT_SKIN_MAX_INFLUENCES) return 2;
    if (n_bones < 1u || n_bones > RT_SKIN_MAX_BONES) return 3;
    for (size_t v = 0; v < n_verts; v++)
        for (uint32_t k = 0; k < influences; k++)
            if (bone_indices[v * influences + k] >= n_bones) {
                if (bad_vertex) *bad_vertex = (uint32_t)v;
                if (bad_slot) *bad_slot = k;
                return 4;
            }
    return 0;
}

// The caller's vertex-major arrays (entry [v][k] at v * influences + k) as the kernel reads them, slot major: bone[k * n_verts + v] in 16 bits
// and weight[k * n_verts + v], so that the 64 lanes of a wave load 64 consecutive entries of one slot.  The arrays must have passed
// rt_skin_validate (every index < n_bones <= 65536 fits 16 bits).  The weights are copied bit for bit.
static inline void rt_skin_pack(uint32_t n_verts, uint32_t influences, const uint32_t *bone_indices, const float *weights,
                                std::vector<uint16_t> &bone, std::vector<float> &weight)
{
    const size_t n = (size_t)n_verts * influences;
    bone.assign(n, (uint16_t)0);
    weight.assign(n, 0.0f);
    for (size_t v = 0; v < n_verts; v++)
        for (uint32_t k = 0; k < influences; k++) {
            bone[(size_t)k * n_verts + v] = (uint16_t)bone_indices[v * influences + k];
            weight[(size_t)k * n_verts + v] = weights[v * influences + k];
        }
}
