// rt_morph.h -- the morph targets of a model (rt_model_set_morph_targets): validation of the caller's sparse lists and their packing into the
// layout k_morph_vertices (rt_model.hip) reads.  Host code without HIP, as rt_skin.h and rt_adjacency.h are: tests/cpp/morph_sanitized.cpp compiles it alone.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#define RT_MORPH_MAX_TARGETS 65536u      // a target index is stored in 16 bits
#define RT_MORPH_SLICE 64u               // vertices per slice: one wavefront

// The packed layout, sliced ELL with slices of one wavefront (SELL-64).  Slice s covers vertices 64 s .. 64 s + 63 and is as wide as the
// longest run of entries among them; the j-th entry of vertex v, in ascending target order, sits in cell
//   slice_cell[v >> 6] + 64 j + (v & 63)
// so that at step j the 64 lanes of a wave read 64 consecutive targets and 64 consecutive 12-byte deltas, every lane gathers its own vertex
// in order and nothing needs an atomic.  Cells beyond a vertex's count hold target 0 and +0 deltas and are never evaluated: a lane loops to
// its own count.
struct rt_morph_packed {
    std::vector<uint32_t> count;         // [V]: entries of each vertex
    std::vector<uint32_t> slice_cell;    // [S + 1], S = ceil(V / 64): the first cell of each slice; slice_cell[S] = number of cells
    std::vector<uint16_t> target;        // [cells]
    std::vector<float> dpos;             // [3 cells]: the position delta of cell c at 3 c
    std::vector<float> dnrm;             // [3 cells] with normal deltas, else empty
};

// 0: the arguments describe n_targets >= 1 morph targets of a model with n_verts vertices.  Else what is wrong: 1 a null array,
// 2 n_targets > 65536, 3 target_offsets[0] != 0, 4 target_offsets[t + 1] < target_offsets[t] (*bad_target = t), 5 a vertex index >= n_verts,
// 6 an index not above the one before it in the same target -- for 5 and 6 *bad_target / *bad_entry name the first such entry, the entry
// as its place in vertex_indices -- and 7 a packed layout of 2^32 cells or more.  Reads n_targets + 1 offsets and target_offsets[n_targets]
// indices and nothing else; the deltas are only asked to be there.
static inline int rt_morph_validate(uint32_t n_verts, uint32_t n_targets, const uint32_t *target_offsets, const uint32_t *vertex_indices,
                                    const float *position_deltas, uint32_t *bad_target, uint32_t *bad_entry)
{
    if (!target_offsets || !vertex_indices || !position_deltas) return 1;
    if (n_targets > RT_MORPH_MAX_TARGETS) return 2;
    if (target_offsets[0] != 0u) return 3;
    for (uint32_t t = 0; t < n_targets; t++)
        if (target_offsets[t + 1] < target_offsets[t]) {
            if (bad_target) *bad_target = t;
            return 4;
        }
    std::vector<uint32_t> count(n_verts, 0u);
    for (uint32_t t = 0; t < n_targets; t++)
        for (uint32_t e = target_offsets[t]; e < target_offsets[t + 1]; e++) {
            const uint32_t v = vertex_indices[e];
            const int what = v >= n_verts ? 5 : (e > target_offsets[t] && v <= vertex_indices[e - 1]) ? 6 : 0;
            if (what) {
                if (bad_target) *bad_target = t;
                if (bad_entry) *bad_entry = e;
                return what;
            }
            count[v]++;
        }
    uint64_t cells = 0;
    for (size_t first = 0; first < n_verts; first += RT_MORPH_SLICE) {
        uint32_t width = 0;
        for (size_t v = first; v < n_verts && v < first + RT_MORPH_SLICE; v++)
            if (count[v] > width) width = count[v];
        cells += (uint64_t)RT_MORPH_SLICE * width;
    }
    return cells >> 32 ? 7 : 0;
}

// The caller's target-major lists as the kernel reads them (above).  The arguments must have passed rt_morph_validate.  normal_deltas may
// be null: positions only, and dnrm stays empty.  The deltas are copied bit for bit.
static inline void rt_morph_pack(uint32_t n_verts, uint32_t n_targets, const uint32_t *target_offsets, const uint32_t *vertex_indices,
                                 const float *position_deltas, const float *normal_deltas, rt_morph_packed &out)
{
    const size_t slices = ((size_t)n_verts + RT_MORPH_SLICE - 1u) / RT_MORPH_SLICE;
    out.count.assign(n_verts, 0u);
    for (uint32_t e = 0; e < target_offsets[n_targets]; e++) out.count[vertex_indices[e]]++;
    out.slice_cell.assign(slices + 1u, 0u);
    for (size_t s = 0; s < slices; s++) {
        uint32_t width = 0;
        for (size_t v = s * RT_MORPH_SLICE; v < n_verts && v < (s + 1u) * RT_MORPH_SLICE; v++)
            if (out.count[v] > width) width = out.count[v];
        out.slice_cell[s + 1u] = out.slice_cell[s] + RT_MORPH_SLICE * width;
    }
    const size_t cells = out.slice_cell[slices];
    out.target.assign(cells, (uint16_t)0);
    out.dpos.assign(3u * cells, 0.0f);
    out.dnrm.assign(normal_deltas ? 3u * cells : 0u, 0.0f);
    std::vector<uint32_t> filled(n_verts, 0u);
    for (uint32_t t = 0; t < n_targets; t++)            // ascending targets: a vertex's cells fill in the order they are evaluated in
        for (uint32_t e = target_offsets[t]; e < target_offsets[t + 1]; e++) {
            const uint32_t v = vertex_indices[e];
            const size_t cell = (size_t)out.slice_cell[v / RT_MORPH_SLICE] + (size_t)RT_MORPH_SLICE * filled[v]++ + v % RT_MORPH_SLICE;
            out.target[cell] = (uint16_t)t;
            memcpy(&out.dpos[3u * cell], position_deltas + 3u * (size_t)e, 12);
            if (normal_deltas) memcpy(&out.dnrm[3u * cell], normal_deltas + 3u * (size_t)e, 12);
        }
}
