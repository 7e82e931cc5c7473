// The host side of a crowd's layout (dxrexperiments_amd/csrc/rt_crowd.h: rt_crowd_layout_layers, rt_crowd_pack_slots,
// rt_crowd_layer_of_slot; host code without HIP) as a CPU program of its own, for g++ -fsanitize=address,undefined
// (tests/test_crowd_device_abi.py).  IN has two parts.
//   Part 1: uint32 n_cases, then per case eight uint32 -- n_actors, n_layers, n_records, n_clips, n_masks, posed, null (1: the list is passed
//     as a null pointer), n_joints -- and n_records records of 20 bytes (rt_skeleton_layer), as tests/cpp/crowd_sanitized.cpp takes them.
//     The list is checked the way rt_crowd_set_layout checks it: copied without its times, then rt_crowd_validate_layers.  OUT per case:
//     uint32 what it says, the actor and the layer it names; and, where it says 0, per slot seven uint32: the clip whose keys the slot names
//     and the clip whose device key times it names (0xFFFFFFFF: null), n_keys, the mask + 1 (0: none), the mode, the bits of the weight, the
//     pad.  Clip k of a case has k + 1 keys and made-up device addresses that are never followed.
//   Part 2: uint32 n_clips, then per clip uint32 n_keys, n_keys floats (the key times), uint32 n_queries and n_queries floats (times, NaN
//     among them).  For every query, on layers 0 and 1, masked and not, in both modes: the record rt_crowd_layer_of_slot makes of the slot
//     that rt_crowd_pack_slots packed must equal the record rt_skeleton_pack_layer makes of the layer, all 56 bytes.  OUT per query: uint32 i
//     (where key_a stands, in keys from the clip's base) and the bits of `a`.
// Every list, table and array of key times lives in a heap block of exactly its size, so that a read or write past either end is a report.
//   crowd_layout_sanitized IN OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../dxrexperiments_amd/csrc/rt_crowd.h"

static const float *clip_base(uint32_t k) { return (const float *)(uintptr_t)(0x10000000u * (uint64_t)(k + 1u)); }
static const float *times_base(uint32_t k) { return (const float *)(uintptr_t)(0x100000u * (uint64_t)(k + 1u)); }
static const float *mask_base(uint32_t m) { return (const float *)(uintptr_t)(0x1000u * (uint64_t)(m + 1u)); }

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    static_assert(sizeof(rt_skeleton_layer) == 20, "a layer is 20 B");
    static_assert(sizeof(rt_blend_layer) == 56, "a layer record is five pointers, two floats and two words");
    static_assert(sizeof(rt_crowd_slot) == 40 && alignof(rt_crowd_slot) == 8, "a slot is three pointers, two words, a float and a pad");
    static_assert(sizeof(rt_blend_layer) % alignof(rt_blend_layer) == 0 && alignof(rt_blend_layer) == 8, "records stand 8-byte aligned at the base of the block's LDS");

    // ---- part 1: layouts ----
    uint32_t n_cases = 0;
    if (fread(&n_cases, sizeof(uint32_t), 1, f) != 1) return 3;
    size_t cases = 0, queries = 0;
    for (uint32_t c = 0; c < n_cases; c++) {
        uint32_t head[8];
        if (fread(head, sizeof(uint32_t), 8, f) != 8) return 3;
        const uint32_t n_actors = head[0], n_layers = head[1], n_records = head[2], n_clips = head[3], n_masks = head[4];
        rt_skeleton_layer *layers = (rt_skeleton_layer *)malloc(n_records ? n_records * sizeof(rt_skeleton_layer) : 1);
        rt_skeleton_layer *mine = (rt_skeleton_layer *)malloc(n_records ? n_records * sizeof(rt_skeleton_layer) : 1);
        if (!layers || !mine || fread(layers, sizeof(rt_skeleton_layer), n_records, f) != n_records) return 3;
        // (as rt_crowd_set_layout: a null list and a layer count out of range are refused before anything is copied or read)
        const bool readable = !head[6] && n_layers >= 1u && n_layers <= RT_SKELETON_MAX_LAYERS;
        if (readable) {
            if ((size_t)n_actors * n_layers != n_records) return 4;
            rt_crowd_layout_layers(n_records, layers, mine);
            for (uint32_t e = 0; e < n_records; e++)
                if (bits(mine[e].time) != 0u || mine[e].clip != layers[e].clip || bits(mine[e].weight) != bits(layers[e].weight) || mine[e].mask != layers[e].mask ||
                    mine[e].mode != layers[e].mode)
                    return 5;
        }
        uint32_t res[3] = {0, 0xFFFFFFFFu, 0xFFFFFFFFu};
        res[0] = (uint32_t)rt_crowd_validate_layers(n_actors, n_layers, head[6] ? nullptr : readable ? mine : layers, n_clips, n_masks, head[5] != 0, &res[1], &res[2]);
        if (res[0] == 6u) return 5;                      // (a layout has no times: nothing to be NaN)
        if (fwrite(res, sizeof(uint32_t), 3, g) != 3) return 3;
        if (res[0] == 0u) {
            rt_crowd_clip *clips = (rt_crowd_clip *)malloc(n_clips ? n_clips * sizeof(rt_crowd_clip) : 1);
            const float **masks = (const float **)malloc(n_masks ? n_masks * sizeof(const float *) : 1);
            rt_crowd_slot *slots = (rt_crowd_slot *)malloc(n_records * sizeof(rt_crowd_slot));
            if (!clips || !masks || !slots) return 3;
            for (uint32_t k = 0; k < n_clips; k++) {
                clips[k].n_keys = k + 1u;
                clips[k].times = nullptr;                // (the host's times: a layout has no use for them)
                clips[k].keys = clip_base(k);
                clips[k].d_times = times_base(k);
            }
            for (uint32_t m = 0; m < n_masks; m++) masks[m] = mask_base(m);
            rt_crowd_pack_slots(n_actors, n_layers, mine, clips, masks, slots);
            for (uint32_t e = 0; e < n_records; e++) {
                const rt_crowd_slot &s = slots[e];
                uint32_t out[7] = {0xFFFFFFFFu, 0xFFFFFFFFu, s.n_keys, 0u, s.mode, bits(s.weight), s.pad};
                for (uint32_t k = 0; k < n_clips; k++) {
                    if (s.keys == clip_base(k)) out[0] = k;
                    if (s.times == times_base(k)) out[1] = k;
                }
                if ((s.keys && out[0] == 0xFFFFFFFFu) || (s.times && out[1] == 0xFFFFFFFFu)) return 6;
                for (uint32_t m = 0; m < n_masks; m++)
                    if (s.mask == mask_base(m)) out[3] = m + 1u;
                if (s.mask && !out[3]) return 6;
                if (fwrite(out, sizeof(uint32_t), 7, g) != 7) return 3;
            }
            free(clips); free(masks); free(slots);
        }
        free(layers); free(mine);
        cases++;
    }

    // ---- part 2: the record of a slot == the record of its layer ----
    uint32_t n_clips = 0;
    if (fread(&n_clips, sizeof(uint32_t), 1, f) != 1) return 3;
    const uint32_t n_joints = 65u;
    const size_t per_key = RT_SKELETON_POSE_FLOATS * (size_t)n_joints;
    for (uint32_t c = 0; c < n_clips; c++) {
        uint32_t n_keys = 0, n_queries = 0;
        if (fread(&n_keys, sizeof(uint32_t), 1, f) != 1 || n_keys == 0u) return 3;
        float *times = (float *)malloc(n_keys * sizeof(float));
        if (!times || fread(times, sizeof(float), n_keys, f) != n_keys) return 3;
        if (fread(&n_queries, sizeof(uint32_t), 1, f) != 1) return 3;
        float *ts = (float *)malloc(n_queries ? n_queries * sizeof(float) : 1);
        if (!ts || fread(ts, sizeof(float), n_queries, f) != n_queries) return 3;
        const rt_crowd_clip clip = {n_keys, times, clip_base(c), times};      // (the slot's times are read: here they are the host's block)
        const float *masks[1] = {mask_base(0)};
        for (uint32_t q = 0; q < n_queries; q++) {
            uint32_t out[2] = {0u, 0u};
            for (uint32_t variant = 0; variant < 8u; variant++) {
                const uint32_t k = variant & 1u, masked = (variant >> 1) & 1u, mode = k ? (variant >> 2) & 1u : RT_LAYER_BLEND;
                // two layers, so that layer 1 exists; the one under test is layer k, and actor 0 is the only actor
                rt_skeleton_layer *list = (rt_skeleton_layer *)malloc(2 * sizeof(rt_skeleton_layer));
                rt_skeleton_layer *mine = (rt_skeleton_layer *)malloc(2 * sizeof(rt_skeleton_layer));
                rt_crowd_slot *slots = (rt_crowd_slot *)malloc(2 * sizeof(rt_crowd_slot));
                if (!list || !mine || !slots) return 3;
                for (uint32_t e = 0; e < 2u; e++) {
                    list[e].clip = 0u;
                    list[e].time = ts[q];
                    list[e].weight = 0.25f + 0.5f * (float)variant;
                    list[e].mask = masked ? 0u : RT_SKELETON_NO_MASK;
                    list[e].mode = e == k ? mode : RT_LAYER_BLEND;
                }
                rt_crowd_layout_layers(2, list, mine);
                if (rt_crowd_validate_layers(1u, 2u, mine, 1u, 1u, false, nullptr, nullptr) != 0) return 7;     // (a NaN time is accepted)
                rt_crowd_pack_slots(1u, 2u, mine, &clip, masks, slots);
                rt_blend_layer of_slot, of_layer;
                memset(&of_slot, 0xAB, sizeof of_slot);
                memset(&of_layer, 0xCD, sizeof of_layer);
                rt_crowd_layer_of_slot(slots[k], n_joints, ts[q], list[k].weight, of_slot);
                rt_skeleton_pack_layer(list[k], k, n_joints, n_keys, times, clip_base(c), masks[0], of_layer);
                if (memcmp(&of_slot, &of_layer, sizeof of_slot) != 0) return 8;
                if (of_slot.mask != (k && masked ? masks[0] : nullptr) || of_slot.mode != list[k].mode || bits(of_slot.weight) != bits(list[k].weight)) return 8;
                if (of_slot.ref_a != clip_base(c) || of_slot.ref_b != clip_base(c) + (n_keys == 1u ? 0u : per_key) || of_slot.key_b != of_slot.key_a + (n_keys == 1u ? 0u : per_key))
                    return 8;
                const size_t i = (size_t)(of_slot.key_a - clip_base(c)) / per_key;
                if (of_slot.key_a != clip_base(c) + per_key * i || i + (n_keys == 1u ? 1u : 2u) > n_keys) return 9;      // (both keys are keys of the clip)
                if (variant && (out[0] != (uint32_t)i || out[1] != bits(of_slot.a))) return 8;
                out[0] = (uint32_t)i;
                out[1] = bits(of_slot.a);
                free(list); free(mine); free(slots);
            }
            if (fwrite(out, sizeof(uint32_t), 2, g) != 2) return 3;
            queries++;
        }
        free(times); free(ts);
    }
    fclose(f);
    fclose(g);
    printf("%zu cases, %zu queries, 0 sanitizer reports\n", cases, queries);
    return 0;
}
