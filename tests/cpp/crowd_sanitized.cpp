// The host side of a crowd (dxrexperiments_amd/csrc/rt_crowd.h: rt_crowd_validate_layers, rt_crowd_pack_layers, rt_crowd_layers_of_times;
// host code without HIP) as a CPU program of its own, for g++ -fsanitize=address,undefined (tests/test_crowd_abi.py).  IN: any number of
// cases, each eight uint32 -- n_actors, n_layers, n_records, n_clips, n_masks, posed, null (1: the list is passed as a null pointer),
// n_joints -- and n_records records of 20 bytes (rt_skeleton_layer): n_actors * n_layers of them where the validator may read the list, 0
// where it must not.  OUT per case: uint32 what rt_crowd_validate_layers says, the actor and the layer it names; and, where it says 0, per
// record nine uint32: where key_a, key_b, ref_a and ref_b stand, in floats from the base of the layer's clip (0xFFFFFFFF: null), the clip the
// base belongs to, the bits of `a` and of the weight, the mask + 1 (0: none) and the mode.
// Clip k of a case has k + 1 keys at times 0, 1 .. k and a made-up device address that is never followed; mask m likewise.  The list and
// the table live in heap blocks of exactly their sizes, so that a read or write past either end is a report.
//   crowd_sanitized IN OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../dxrexperiments_amd/csrc/rt_crowd.h"

static const float *clip_base(uint32_t k) { return (const float *)(uintptr_t)(0x10000000u * (uint64_t)(k + 1u)); }
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
    uint32_t head[8];
    size_t cases = 0;
    while (fread(head, sizeof(uint32_t), 8, f) == 8) {
        const uint32_t n_actors = head[0], n_layers = head[1], n_records = head[2], n_clips = head[3], n_masks = head[4], n_joints = head[7];
        rt_skeleton_layer *layers = (rt_skeleton_layer *)malloc(n_records ? n_records * sizeof(rt_skeleton_layer) : 1);
        if (!layers || fread(layers, sizeof(rt_skeleton_layer), n_records, f) != n_records) return 3;
        uint32_t res[3] = {0, 0xFFFFFFFFu, 0xFFFFFFFFu};
        res[0] = (uint32_t)rt_crowd_validate_layers(n_actors, n_layers, head[6] ? nullptr : layers, n_clips, n_masks, head[5] != 0, &res[1], &res[2]);
        if (fwrite(res, sizeof(uint32_t), 3, g) != 3) return 3;
        // the actor and the layer are optional, and it says the same without them
        if ((uint32_t)rt_crowd_validate_layers(n_actors, n_layers, head[6] ? nullptr : layers, n_clips, n_masks, head[5] != 0, nullptr, nullptr) != res[0]) return 5;
        if (res[0] == 0u) {
            rt_crowd_clip *clips = (rt_crowd_clip *)malloc(n_clips ? n_clips * sizeof(rt_crowd_clip) : 1);
            const float **masks = (const float **)malloc(n_masks ? n_masks * sizeof(const float *) : 1);
            float **times = (float **)malloc(n_clips ? n_clips * sizeof(float *) : 1);
            rt_blend_layer *table = (rt_blend_layer *)malloc(n_records * sizeof(rt_blend_layer));
            if (!clips || !masks || !times || !table) return 3;
            for (uint32_t k = 0; k < n_clips; k++) {
                times[k] = (float *)malloc((k + 1u) * sizeof(float));
                if (!times[k]) return 3;
                for (uint32_t i = 0; i <= k; i++) times[k][i] = (float)i;
                clips[k].n_keys = k + 1u;
                clips[k].times = times[k];
                clips[k].keys = clip_base(k);
            }
            for (uint32_t m = 0; m < n_masks; m++) masks[m] = mask_base(m);
            rt_crowd_pack_layers(n_actors, n_layers, layers, n_joints, clips, masks, table);
            for (uint32_t e = 0; e < n_records; e++) {
                const rt_blend_layer &b = table[e];
                uint32_t out[9] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, bits(b.a), bits(b.weight), 0u, b.mode};
                if (b.key_a) {
                    const uint32_t clip = layers[e].clip;
                    out[0] = (uint32_t)(b.key_a - clip_base(clip));
                    out[1] = (uint32_t)(b.key_b - clip_base(clip));
                    out[2] = (uint32_t)(b.ref_a - clip_base(clip));
                    out[3] = (uint32_t)(b.ref_b - clip_base(clip));
                    out[4] = clip;
                } else if (b.key_b || b.ref_a || b.ref_b) return 6;
                for (uint32_t m = 0; m < n_masks; m++)
                    if (b.mask == mask_base(m)) out[7] = m + 1u;
                if (b.mask && !out[7]) return 6;
                if (b.pad != 0u) return 6;
                if (fwrite(out, sizeof(uint32_t), 9, g) != 9) return 3;
            }
            // rt_crowd_set_times's layers: one per actor, exactly n_actors records written
            if (n_layers == 1u) {
                uint32_t *c = (uint32_t *)malloc(n_actors * sizeof(uint32_t));
                float *t = (float *)malloc(n_actors * sizeof(float));
                rt_skeleton_layer *made = (rt_skeleton_layer *)malloc(n_actors * sizeof(rt_skeleton_layer));
                if (!c || !t || !made) return 3;
                for (uint32_t a = 0; a < n_actors; a++) { c[a] = layers[a].clip; t[a] = layers[a].time; }
                rt_crowd_layers_of_times(n_actors, c, t, made);
                for (uint32_t a = 0; a < n_actors; a++)
                    if (made[a].clip != c[a] || bits(made[a].time) != bits(t[a]) || made[a].mask != RT_SKELETON_NO_MASK || made[a].mode != RT_LAYER_BLEND) return 7;
                free(c); free(t); free(made);
            }
            for (uint32_t k = 0; k < n_clips; k++) free(times[k]);
            free(clips); free(masks); free(times); free(table);
        }
        free(layers);
        cases++;
    }
    fclose(f);
    fclose(g);
    printf("%zu cases, 0 sanitizer reports\n", cases);
    return 0;
}
