// The host side of a skeleton (dxrexperiments_amd/csrc/rt_skeleton.h: validation, the level table, the segment search of a clip; host code
// without HIP) as a CPU program of its own, for g++ -fsanitize=address,undefined (tests/test_skeleton_abi.py).  IN: any number of cases, each
// starting with a uint32 kind.
//   kind 0, a hierarchy: uint32 n_joints, then n_joints int32 parents.  OUT: uint32 what rt_skeleton_validate says and the joint it names (0
//   unless it says 3); if it says 0: uint32 n_levels, the n_joints uint32 of the level order, the n_levels + 1 level offsets, the n_joints
//   packed table entries.
//   kind 1, key times: uint32 n_keys, n_keys floats, uint32 n_queries, n_queries floats t.  OUT: uint32 what rt_skeleton_validate_times says
//   and the key it names (0 unless it says 3 or 4); if it says 0: per query uint32 i and float a of rt_skeleton_segment.
// Every array lives in a heap block of exactly its size, so that a read or write past either end is a report.
//   skeleton_sanitized IN OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dxrexperiments_amd/csrc/rt_skeleton.h"

template <class T> static T *block(size_t n) { return (T *)malloc(n ? n * sizeof(T) : 1); }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    uint32_t head[2];
    size_t cases = 0;
    float *some = block<float>(1);                        // (the inverse bind matrices: only ever compared with null)
    if (!some) return 3;
    while (fread(head, sizeof(uint32_t), 2, f) == 2) {
        const uint32_t kind = head[0], n = head[1];
        uint32_t res[2] = {0, 0};
        if (kind == 0) {
            int32_t *parents = block<int32_t>(n);
            if (!parents || fread(parents, sizeof(int32_t), n, f) != n) return 3;
            res[0] = (uint32_t)rt_skeleton_validate(n, parents, some, &res[1]);
            if (fwrite(res, sizeof(uint32_t), 2, g) != 2) return 3;
            if (res[0] == 0) {
                std::vector<uint32_t> order, offsets, table;
                const uint32_t n_levels = rt_skeleton_levels(n, parents, order, offsets);
                rt_skeleton_pack_table(parents, order, table);
                if (order.size() != n || table.size() != n || offsets.size() != (size_t)n_levels + 1) return 4;
                if (fwrite(&n_levels, sizeof(uint32_t), 1, g) != 1 || fwrite(order.data(), sizeof(uint32_t), n, g) != n ||
                    fwrite(offsets.data(), sizeof(uint32_t), offsets.size(), g) != offsets.size() || fwrite(table.data(), sizeof(uint32_t), n, g) != n)
                    return 3;
            }
            // null arrays are refused before anything is read
            if (rt_skeleton_validate(n, nullptr, some, nullptr) != 1 || rt_skeleton_validate(n, parents, nullptr, nullptr) != 1) return 5;
            free(parents);
        } else if (kind == 1) {
            float *times = block<float>(n);
            uint32_t n_queries = 0;
            if (!times || fread(times, sizeof(float), n, f) != n || fread(&n_queries, sizeof(uint32_t), 1, f) != 1) return 3;
            float *ts = block<float>(n_queries);
            if (!ts || fread(ts, sizeof(float), n_queries, f) != n_queries) return 3;
            res[0] = (uint32_t)rt_skeleton_validate_times(n, times, &res[1]);
            if (fwrite(res, sizeof(uint32_t), 2, g) != 2) return 3;
            if (res[0] == 0)
                for (uint32_t q = 0; q < n_queries; q++) {
                    uint32_t i = 0xFFFFFFFFu;
                    float a = -1.0f;
                    rt_skeleton_segment(n, times, ts[q], &i, &a);
                    if (fwrite(&i, sizeof(uint32_t), 1, g) != 1 || fwrite(&a, sizeof(float), 1, g) != 1) return 3;
                }
            if (rt_skeleton_validate_times(n, nullptr, nullptr) != 1) return 5;
            free(times);
            free(ts);
        } else return 6;
        cases++;
    }
    free(some);
    fclose(f);
    fclose(g);
    printf("%zu cases, 0 sanitizer reports\n", cases);
    return 0;
}
