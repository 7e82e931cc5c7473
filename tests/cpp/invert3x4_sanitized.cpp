// The instance transform's text (dxrexperiments_amd/csrc/rt_xform.h: device code, kept host-compilable) as a CPU program of its own, for
// g++ -fsanitize=address,undefined (tests/test_scene_update_abi.py): reads n x 12 floats, writes n x 13 -- the fp32 adjugate / determinant
// inverse of every matrix and whether it is the identity.  Every matrix lives in a heap block of exactly twelve floats, so that a read or
// write past either end is a report.
//   invert3x4_sanitized IN OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dxrexperiments_amd/csrc/rt_xform.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> in;
    float row[12];
    while (fread(row, sizeof(float), 12, f) == 12) in.insert(in.end(), row, row + 12);
    fclose(f);
    const size_t n = in.size() / 12;
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    for (size_t k = 0; k < n; k++) {
        float *m = (float *)malloc(12 * sizeof(float)), *o = (float *)malloc(12 * sizeof(float));
        if (!m || !o) return 3;
        memcpy(m, &in[12 * k], 12 * sizeof(float));
        invert3x4(m, o);
        const float identity = is_identity3x4(m) ? 1.0f : 0.0f;
        if (fwrite(o, sizeof(float), 12, g) != 12 || fwrite(&identity, sizeof(float), 1, g) != 1) return 3;
        free(m);
        free(o);
    }
    fclose(g);
    printf("%zu matrices, 0 sanitizer reports\n", n);
    return 0;
}
