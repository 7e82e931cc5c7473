// rt_adjacency.h -- the vertex -> triangle adjacency of an index list, as CSR.  Host code without HIP: rt_model_recompute_normals builds it
// once per model and uploads it; tests/cpp/adjacency_sanitized.cpp compiles it alone.
#pragma once

#include <stdint.h>
#include <vector>

// off[n_verts + 1], tris[off[n_verts]]: tris[off[v] .. off[v + 1]) are the triangles that name vertex v at any corner, in ASCENDING order, a
// triangle that names v more than once listed once.  A vertex no triangle names has an empty run.  The order is the definition of
// rt_model_recompute_normals' sum (include/dxr_amd.h).  false: an index >= n_verts (nothing is written past the arrays either way).
static inline bool rt_build_adjacency(const uint32_t *idx, uint32_t n_tris, uint32_t n_verts, std::vector<uint32_t> &off, std::vector<uint32_t> &tris)
{
    off.assign((size_t)n_verts + 1, 0u);
    tris.clear();
    // the corners of triangle t that count: each distinct vertex once
    auto corners = [idx](uint32_t t, uint32_t out[3]) {
        const uint32_t a = idx[3 * (size_t)t], b = idx[3 * (size_t)t + 1], c = idx[3 * (size_t)t + 2];
        int n = 0;
        out[n++] = a;
        if (b != a) out[n++] = b;
        if (c != a && c != b) out[n++] = c;
        return n;
    };
    for (uint32_t t = 0; t < n_tris; t++) {
        uint32_t v[3];
        const int n = corners(t, v);
        for (int k = 0; k < n; k++) {
            if (v[k] >= n_verts) return false;
            off[(size_t)v[k] + 1]++;
        }
    }
    for (size_t v = 0; v < n_verts; v++) off[v + 1] += off[v];
    tris.assign(off[n_verts], 0u);
    std::vector<uint32_t> at(off.begin(), off.end() - 1);      // next free slot of every vertex's run
    for (uint32_t t = 0; t < n_tris; t++) {                    // triangles in ascending order: so is every run
        uint32_t v[3];
        const int n = corners(t, v);
        for (int k = 0; k < n; k++) tris[at[v[k]]++] = t;
    }
    return true;
}
