// The host side of rt_model_set_morph_targets (dxrexperiments_amd/csrc/rt_morph.h: validation and SELL-64 packing, host code without HIP) as
// a CPU program of its own, for g++ -fsanitize=address,undefined (tests/test_model_morph_abi.py).  IN: any number of cases, each uint32
// n_verts, n_targets, n_entries, has_normals, then n_targets + 1 uint32 offsets, n_entries uint32 vertex indices, 3 n_entries float position
// deltas and, with has_normals, as many normal deltas; OUT per case: uint32 what rt_morph_validate says, the target and the entry it names
// (0, 0 unless it names them), and if it says 0 the packed count, slice_cell, target, dpos and (with has_normals) dnrm.  Every array lives in
// a heap block of exactly its size, so that a read or write past either end is a report.  At the end, from arrays made here: the layout of
// exactly 2^32 cells is refused and the one a target smaller is not.
//   morph_sanitized IN OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dxrexperiments_amd/csrc/rt_morph.h"

template <class T>
static T *read_block(FILE *f, size_t n)
{
    T *p = (T *)malloc(n ? n * sizeof(T) : 1);
    if (!p || fread(p, sizeof(T), n, f) != n) exit(3);
    return p;
}

template <class T>
static void write_block(FILE *g, const std::vector<T> &v)
{
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), g) != v.size()) exit(3);
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    uint32_t head[4];
    size_t cases = 0;
    while (fread(head, sizeof(uint32_t), 4, f) == 4) {
        const uint32_t nv = head[0], nt = head[1];
        const size_t ne = head[2];
        uint32_t *off = read_block<uint32_t>(f, (size_t)nt + 1);
        uint32_t *idx = read_block<uint32_t>(f, ne);
        float *dp = read_block<float>(f, 3 * ne);
        float *dn = head[3] ? read_block<float>(f, 3 * ne) : nullptr;
        uint32_t res[3] = {0, 0, 0};
        res[0] = (uint32_t)rt_morph_validate(nv, nt, off, idx, dp, &res[1], &res[2]);
        if (fwrite(res, sizeof(uint32_t), 3, g) != 3) return 3;
        if (res[0] == 0) {
            rt_morph_packed pk;
            rt_morph_pack(nv, nt, off, idx, dp, dn, pk);
            const size_t slices = ((size_t)nv + 63) / 64;
            if (pk.count.size() != nv || pk.slice_cell.size() != slices + 1) return 4;
            const size_t cells = pk.slice_cell[slices];
            if (pk.target.size() != cells || pk.dpos.size() != 3 * cells || pk.dnrm.size() != (dn ? 3 * cells : 0)) return 4;
            write_block(g, pk.count); write_block(g, pk.slice_cell); write_block(g, pk.target); write_block(g, pk.dpos); write_block(g, pk.dnrm);
        }
        // null arrays are refused before anything is read
        if (rt_morph_validate(nv, nt, nullptr, idx, dp, nullptr, nullptr) != 1 || rt_morph_validate(nv, nt, off, nullptr, dp, nullptr, nullptr) != 1 ||
            rt_morph_validate(nv, nt, off, idx, nullptr, nullptr, nullptr) != 1) return 5;
        free(off); free(idx); free(dp); free(dn);
        cases++;
    }
    fclose(f);
    fclose(g);
    {   // 65536 vertices, 1024 slices; every target names the first vertex of every slice: 64 cells per slice and target.  65536 targets are
        // 2^32 cells, refused; 65535 targets pass (and are not packed here).  The deltas are only asked to be there.
        const uint32_t nv = 65536, nt = 65536, per = 1024;
        uint32_t *off = (uint32_t *)malloc(((size_t)nt + 1) * sizeof(uint32_t));
        uint32_t *idx = (uint32_t *)malloc((size_t)nt * per * sizeof(uint32_t));
        float *dp = (float *)malloc(sizeof(float));
        if (!off || !idx || !dp) return 3;
        for (uint32_t t = 0; t <= nt; t++) off[t] = t * per;
        for (size_t e = 0; e < (size_t)nt * per; e++) idx[e] = 64u * (uint32_t)(e % per);
        if (rt_morph_validate(nv, nt, off, idx, dp, nullptr, nullptr) != 7) return 6;
        if (rt_morph_validate(nv, nt - 1, off, idx, dp, nullptr, nullptr) != 0) return 6;
        free(off); free(idx); free(dp);
    }
    printf("%zu target sets, 0 sanitizer reports\n", cases);
    return 0;
}
