// The host side of ordered IK groups (dxrexperiments_amd/csrc/rt_ik_groups.h: rt_ik_groups_validate, rt_ik_groups_refusal, rt_ik_group_ends,
// rt_ik_group_sizes; rt_skeleton.h: rt_skeleton_pack_ik; host code without HIP) as a CPU program of its own, for
// g++ -fsanitize=address,undefined (tests/test_ik_groups_abi.py).
//   IN: uint32 n_cases, then per case seven uint32 -- n_groups (what the call is told), n_sizes (how many sizes stand behind the pointer),
//     n_records, n_joints, posed, null_sizes, null_records (1: passed as a null pointer) --, n_sizes uint32 sizes, n_records records of 36
//     bytes (rt_skeleton_ik) and n_joints int32 parents.
//   OUT per case: uint32 what the check says, the four indices it names and the total it found; 256 bytes of the refusal's text under the
//     name "who" (zeros where the check says 0) and uint32 its class; and, where the check says 0 or 8, the n entries of the packed table,
//     48 bytes each, and the two halves of the 64 bits of group ends.
// Every array lives in a heap block of exactly its size, so that a read past either end is a report: a list whose sizes or records must not
// be read has no size, or no record, behind its pointer.
//   ik_groups_sanitized IN OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../dxrexperiments_amd/csrc/rt_ik_groups.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    static_assert(sizeof(rt_skeleton_ik) == 36, "a constraint is 36 B");
    static_assert(sizeof(IkEntry) == 48, "an entry is 48 B");
    static_assert(RT_SKELETON_MAX_IK_GROUPS == 8u && RT_SKELETON_MAX_IK <= 255u, "eight ends of one byte each");
    uint32_t n_cases = 0;
    if (fread(&n_cases, sizeof(uint32_t), 1, f) != 1) return 3;
    size_t lists = 0;
    for (uint32_t c = 0; c < n_cases; c++) {
        uint32_t head[7];
        if (fread(head, sizeof(uint32_t), 7, f) != 7) return 3;
        const uint32_t n_groups = head[0], n_sizes = head[1], n_records = head[2], n_joints = head[3];
        uint32_t *sizes = (uint32_t *)malloc(n_sizes ? n_sizes * sizeof(uint32_t) : 1);
        rt_skeleton_ik *records = (rt_skeleton_ik *)malloc(n_records ? n_records * sizeof(rt_skeleton_ik) : 1);
        int32_t *parents = (int32_t *)malloc(n_joints ? n_joints * sizeof(int32_t) : 1);
        if (!sizes || !records || !parents || fread(sizes, sizeof(uint32_t), n_sizes, f) != n_sizes || fread(records, sizeof(rt_skeleton_ik), n_records, f) != n_records ||
            fread(parents, sizeof(int32_t), n_joints, f) != n_joints)
            return 3;
        uint32_t res[6] = {0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        res[0] = (uint32_t)rt_ik_groups_validate(n_groups, head[5] ? nullptr : sizes, head[6] ? nullptr : records, n_joints, parents, head[4] != 0, &res[5], &res[1]);
        if (rt_ik_groups_validate(n_groups, head[5] ? nullptr : sizes, head[6] ? nullptr : records, n_joints, parents, head[4] != 0, nullptr, nullptr) != (int)res[0]) return 4;      // (both outputs may be null)
        if (fwrite(res, sizeof(uint32_t), 6, g) != 6) return 3;
        char msg[256];
        memset(msg, 0, sizeof msg);
        uint32_t rc = 0;
        if (res[0]) rc = (uint32_t)rt_ik_groups_refusal((int)res[0], "who", n_groups, res[5], records, &res[1], n_joints, "skeleton", "a hint", msg, sizeof msg);
        if (fwrite(msg, 1, sizeof msg, g) != sizeof msg || fwrite(&rc, sizeof(uint32_t), 1, g) != 1) return 3;
        if (res[0] == 0u || res[0] == 8u) {
            const uint32_t n = res[5];
            if (n != n_records || n_groups != n_sizes) return 5;
            IkTable *table = (IkTable *)malloc(sizeof(IkTable));
            if (!table) return 3;
            memset(table, 0xAB, sizeof(IkTable));
            rt_skeleton_pack_ik(n, records, parents, *table);
            for (uint32_t k = n; k < RT_SKELETON_MAX_IK; k++)
                for (size_t b = 0; b < sizeof(IkEntry); b++)
                    if (((const unsigned char *)&table->e[k])[b] != 0xABu) return 6;      // (the entries behind the list are left alone)
            const uint64_t ends = rt_ik_group_ends(n_groups, sizes);
            const uint32_t halves[2] = {(uint32_t)ends, (uint32_t)(ends >> 32)};
            uint32_t back[RT_SKELETON_MAX_IK_GROUPS];
            rt_ik_group_sizes(ends, n_groups, back);
            if (memcmp(back, sizes, n_groups * sizeof(uint32_t)) != 0) return 7;          // (the ends give the sizes back)
            if (fwrite(table->e, sizeof(IkEntry), n, g) != n || fwrite(halves, sizeof(uint32_t), 2, g) != 2) return 3;
            free(table);
        }
        free(sizes); free(records); free(parents);
        lists++;
    }
    fclose(f);
    fclose(g);
    printf("%zu lists, 0 sanitizer reports\n", lists);
    return 0;
}
