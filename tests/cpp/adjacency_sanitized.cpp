// The vertex -> triangle CSR builder of rt_model_recompute_normals (dxrexperiments_amd/csrc/rt_adjacency.h: host code without HIP) as a CPU
// program of its own, for g++ -fsanitize=address,undefined (tests/test_model_deform_abi.py).  IN: any number of cases, each
// uint32 n_verts, n_tris and 3 n_tris indices; OUT per case: uint32 ok (0: an index out of range, nothing follows), then off[n_verts + 1]
// and tris[off[n_verts]].  Every index list lives in a heap block of exactly its size, so that a read past either end is a report.
//   adjacency_sanitized IN OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dxrexperiments_amd/csrc/rt_adjacency.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    uint32_t head[2];
    size_t cases = 0;
    while (fread(head, sizeof(uint32_t), 2, f) == 2) {
        const size_t n_idx = 3 * (size_t)head[1];
        uint32_t *idx = (uint32_t *)malloc(n_idx ? n_idx * sizeof(uint32_t) : 1);
        if (!idx || fread(idx, sizeof(uint32_t), n_idx, f) != n_idx) return 3;
        std::vector<uint32_t> off, tris;
        const uint32_t ok = rt_build_adjacency(idx, head[1], head[0], off, tris) ? 1u : 0u;
        if (fwrite(&ok, sizeof ok, 1, g) != 1) return 3;
        if (ok && (fwrite(off.data(), sizeof(uint32_t), off.size(), g) != off.size() ||
                   (tris.size() && fwrite(tris.data(), sizeof(uint32_t), tris.size(), g) != tris.size()))) return 3;
        free(idx);
        cases++;
    }
    fclose(f);
    fclose(g);
    printf("%zu index lists, 0 sanitizer reports\n", cases);
    return 0;
}
