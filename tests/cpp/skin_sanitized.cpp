// The host side of rt_model_set_skin (dxrexperiments_amd/csrc/rt_skin.h: validation and slot-major 16-bit packing, host code without HIP) as
// a CPU program of its own, for g++ -fsanitize=address,undefined (tests/test_model_skin_abi.py).  IN: any number of cases, each uint32
// n_verts, influences, n_bones, then n_verts x influences uint32 bone indices and as many float weights, vertex major; OUT per case: uint32
// what rt_skin_validate says, the vertex and the slot it names (0, 0 unless it says 4), and if it says 0 the packed uint16 indices and the
// packed weights.  Every array lives in a heap block of exactly its size, so that a read or write past either end is a report.
//   skin_sanitized IN OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dxrexperiments_amd/csrc/rt_skin.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    uint32_t head[3];
    size_t cases = 0;
    while (fread(head, sizeof(uint32_t), 3, f) == 3) {
        const size_t n = (size_t)head[0] * head[1];
        uint32_t *bones = (uint32_t *)malloc(n ? n * sizeof(uint32_t) : 1);
        float *weights = (float *)malloc(n ? n * sizeof(float) : 1);
        if (!bones || !weights || fread(bones, sizeof(uint32_t), n, f) != n || fread(weights, sizeof(float), n, f) != n) return 3;
        uint32_t res[3] = {0, 0, 0};
        res[0] = (uint32_t)rt_skin_validate(head[0], head[1], head[2], bones, weights, &res[1], &res[2]);
        if (fwrite(res, sizeof(uint32_t), 3, g) != 3) return 3;
        if (res[0] == 0) {
            std::vector<uint16_t> pb;
            std::vector<float> pw;
            rt_skin_pack(head[0], head[1], bones, weights, pb, pw);
            if (pb.size() != n || pw.size() != n) return 4;
            if (n && (fwrite(pb.data(), sizeof(uint16_t), n, g) != n || fwrite(pw.data(), sizeof(float), n, g) != n)) return 3;
        }
        // null arrays are refused before anything is read
        if (rt_skin_validate(head[0], head[1], head[2], nullptr, weights, nullptr, nullptr) != 1 ||
            rt_skin_validate(head[0], head[1], head[2], bones, nullptr, nullptr, nullptr) != 1) return 5;
        free(bones);
        free(weights);
        cases++;
    }
    fclose(f);
    fclose(g);
    printf("%zu skins, 0 sanitizer reports\n", cases);
    return 0;
}
