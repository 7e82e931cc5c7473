// The host side of attached instances (dxrexperiments_amd/csrc/rt_attach.h: validation of a binding, its device word, the search of a range
// for an attached instance; host code without HIP) as a CPU program of its own, for g++ -fsanitize=address,undefined
// (tests/test_instance_attach_abi.py).  IN: any number of cases, each eight uint32 -- n_instances, first, count, n_joints, has_joints,
// has_local, n_words, n_read -- then n_read uint32 joints (n_read is `count`, or fewer when the range is one the validation must refuse before
// it reads any), then n_words uint32 words of a scene.  OUT per case: uint32 what rt_attach_validate says and the entry it names (0 unless it
// says 3); if it says 0, the `count` packed words; then uint32 whether rt_attach_range_holds finds an attached instance in first .. first +
// count - 1 of the scene's words (asked only of ranges the validation accepts) and which.
// Every array lives in a heap block of exactly its size, so that a read or write past either end is a report.
//   attach_sanitized IN OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../dxrexperiments_amd/csrc/rt_attach.h"

template <class T> static T *block(size_t n) { return (T *)malloc(n ? n * sizeof(T) : 1); }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    uint32_t head[8];
    size_t cases = 0;
    while (fread(head, sizeof(uint32_t), 8, f) == 8) {
        const uint32_t n_instances = head[0], first = head[1], count = head[2], n_joints = head[3], n_words = head[6], n_read = head[7];
        const bool has_joints = head[4] != 0, has_local = head[5] != 0;
        uint32_t *joints = block<uint32_t>(n_read), *words = block<uint32_t>(n_words);
        if (!joints || !words || fread(joints, sizeof(uint32_t), n_read, f) != n_read || fread(words, sizeof(uint32_t), n_words, f) != n_words) return 3;
        uint32_t res[2] = {0, 0};
        res[0] = (uint32_t)rt_attach_validate(n_instances, first, count, n_joints, has_joints ? joints : nullptr, &res[1]);
        if (fwrite(res, sizeof(uint32_t), 2, g) != 2) return 3;
        if (res[0] == 0) {
            uint32_t *packed = block<uint32_t>(count);
            if (!packed) return 3;
            rt_attach_pack(count, joints, has_local, packed);
            if (fwrite(packed, sizeof(uint32_t), count, g) != count) return 3;
            free(packed);
            uint32_t held[2] = {0, 0};
            held[0] = rt_attach_range_holds(n_words ? words : nullptr, n_words, first, count, &held[1]) ? 1u : 0u;
            if (fwrite(held, sizeof(uint32_t), 2, g) != 2) return 3;
        }
        free(joints);
        free(words);
        cases++;
    }
    fclose(f);
    if (fclose(g) != 0) return 3;
    printf("%zu cases, 0 sanitizer reports\n", cases);
    return 0;
}
