// The host's check of a layer list (dxrexperiments_amd/csrc/rt_skeleton.h: rt_skeleton_validate_layers; host code without HIP) as a CPU
// program of its own, for g++ -fsanitize=address,undefined (tests/test_skeleton_blend_abi.py).  IN: any number of cases, each six uint32 --
// n_layers, n_records, n_clips, n_masks, posed, null (1: the list is passed as a null pointer) -- and n_records records of 20 bytes
// (rt_skeleton_layer).  n_records is n_layers where the validator may read the list, and 0 where it must not (n_layers outside 1 .. 8).
// OUT per case: uint32 what rt_skeleton_validate_layers says and the layer it names.
// The list lives in a heap block of exactly its size, so that a read past either end is a report.
//   skeleton_blend_sanitized IN OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../dxrexperiments_amd/csrc/rt_skeleton.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    static_assert(sizeof(rt_skeleton_layer) == 20, "a layer is 20 B");
    uint32_t head[6];
    size_t cases = 0;
    while (fread(head, sizeof(uint32_t), 6, f) == 6) {
        const uint32_t n_layers = head[0], n_records = head[1], n_clips = head[2], n_masks = head[3];
        rt_skeleton_layer *layers = (rt_skeleton_layer *)malloc(n_records ? n_records * sizeof(rt_skeleton_layer) : 1);
        if (!layers || fread(layers, sizeof(rt_skeleton_layer), n_records, f) != n_records) return 3;
        uint32_t res[2] = {0, 0xFFFFFFFFu};
        res[0] = (uint32_t)rt_skeleton_validate_layers(n_layers, head[5] ? nullptr : layers, n_clips, n_masks, head[4] != 0, &res[1]);
        if (fwrite(res, sizeof(uint32_t), 2, g) != 2) return 3;
        // the layer is optional, and says the same without it
        if ((uint32_t)rt_skeleton_validate_layers(n_layers, head[5] ? nullptr : layers, n_clips, n_masks, head[4] != 0, nullptr) != res[0]) return 5;
        free(layers);
        cases++;
    }
    fclose(f);
    fclose(g);
    printf("%zu cases, 0 sanitizer reports\n", cases);
    return 0;
}
