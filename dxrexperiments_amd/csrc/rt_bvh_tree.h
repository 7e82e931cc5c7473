// rt_bvh_tree.h -- what the tree builders share, each thing once: rt_bvh_build.hip (LBVH, BLAS), rt_bvh_ploc.hip (the production binary tree),
// rt_bvh_wide.hip (its collapse) and the TLAS update of rt_scene.hip.  A header of its own beside rt_lbvh.h, which includes it: rt_lbvh.h is the
// LBVH builder's interface (temporaries, host entry points), of which PLOC and the collapse use nothing; this is the vocabulary of all four.
#pragma once

#include "rt_internal.h"

inline unsigned grid_for(size_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }
struct Box6 { float lo[3]; float hi[3]; };
// (half) surface area: of a box, and of the union of two without forming it
__device__ __forceinline__ float box_area(const Box6 &b)
{
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return dx * dy + dy * dz + dz * dx;
}
__device__ __forceinline__ float merged_area(const Box6 &a, const Box6 &b)
{
    const float dx = fmaxf(a.hi[0], b.hi[0]) - fminf(a.lo[0], b.lo[0]);
    const float dy = fmaxf(a.hi[1], b.hi[1]) - fminf(a.lo[1], b.lo[1]);
    const float dz = fmaxf(a.hi[2], b.hi[2]) - fminf(a.lo[2], b.lo[2]);
    return dx * dy + dy * dz + dz * dx;
}
__device__ __forceinline__ Box6 box_union(const Box6 &a, const Box6 &b)
{
    Box6 u;
    for (int k = 0; k < 3; k++) { u.lo[k] = fminf(a.lo[k], b.lo[k]); u.hi[k] = fmaxf(a.hi[k], b.hi[k]); }
    return u;
}

// The binary tree in CLUSTER NUMBERING, what one builder hands the next: PLOC and the conversion of the canonical LBVH (k_lbvh_to_tree,
// rt_bvh_wide.hip) make one, the collapse (rt_build_wide_layout) takes one.  The n leaves have the ids 0 .. n-1, in sorted-key order; the
// internal nodes n .. 2n-2 (PLOC: in creation order, the root last; from the LBVH: n + canonical index, the root first).  left / right are
// indexed by id - n, everything else by id.  A view of arena slices, passed to kernels by value.
struct BinTree {
    uint32_t *left, *right;      // [id - n] the children of an internal node
    Box6 *box;                   // [id]
    uint32_t *size, *offset;     // [id] leaves below; leaves before, depth first: a subtree's records are offset .. offset + size - 1
    uint32_t *leaf_prim;         // [id < n] TLAS: the instance of a leaf; nullptr for a BLAS, whose leaves are records
    uint32_t *parent;            // [id] 0xFFFFFFFF for the root
    uint32_t n;
};

// a triangle's three positions; from them its own box (exact min / max) and its 48-byte record with its primitive and mark (rt_refs.h:
// 0; 1: a reference of a split triangle, whose box stands beside the record; 2: a split triangle held once, validated by primitive)
__device__ __forceinline__ void tri_positions(const rt_vertex *__restrict__ verts, const uint32_t *__restrict__ idx, uint32_t prim, float p[3][3])
{
    for (int k = 0; k < 3; k++) {
        const rt_float3 v = verts[idx[3 * prim + k]].position;
        p[k][0] = v.x; p[k][1] = v.y; p[k][2] = v.z;
    }
}
__device__ __forceinline__ Box6 tri_box(const float p[3][3])
{
    Box6 b;
    for (int q = 0; q < 3; q++) { b.lo[q] = fminf(fminf(p[0][q], p[1][q]), p[2][q]); b.hi[q] = fmaxf(fmaxf(p[0][q], p[1][q]), p[2][q]); }
    return b;
}
__device__ __forceinline__ TriRec tri_record(const float p[3][3], uint32_t prim, uint32_t mark)
{
    TriRec t;
    t.a = make_float4(p[0][0], p[0][1], p[0][2], p[1][0]);
    t.b = make_float4(p[1][1], p[1][2], p[2][0], p[2][1]);
    t.c = make_float4(p[2][2], __uint_as_float(prim), __uint_as_float(mark), 0.0f);
    return t;
}

__device__ __forceinline__ uint32_t expand10(uint32_t v)
{
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ __forceinline__ uint32_t quant10(float c, float lo, float ext)
{
    if (!(ext > 0.0f)) return 0;
    float q = (c - lo) / ext * 1024.0f;
    q = fminf(fmaxf(q, 0.0f), 1023.0f);
    return (uint32_t)q;
}
// the 30-bit Morton code of the centre of the box lo[3] .. hi[3] within the structure bounds (lo[3], hi[3])
__device__ __forceinline__ uint32_t morton30(const float *lo, const float *hi, const float *__restrict__ bounds)
{
    uint32_t m = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) m |= expand10(quant10((lo[c] + hi[c]) * 0.5f, bounds[c], bounds[3 + c] - bounds[c])) << (2 - c);
    return m;
}

// THE ORDERING OF A BOTTOM-UP CLIMB.  Two kernels climb a binary tree from its leaves, every internal node visited once (Karras 2012):
// k_refit (rt_bvh_build.hip) unites boxes, k_wide_sah (rt_bvh_wide.hip) fills cost records.  At a parent a thread bumps an arrival counter;
// the first arriver stops, the second -- who knows by the counter that the sibling's subtree is complete -- reads what the sibling's
// climber published and goes on.  The two may run on different XCDs, whose L2s are not coherent with each other.  A release / acquire
// pair at agent scope would be correct and would write back and invalidate the WHOLE local L2 once per node; the climbs order exactly
// the words they exchange, by hand:
//   publish            what a climber hands over is stored at AGENT scope: written through the local L2.
//   wait_acknowledged  every such store has been ACKNOWLEDGED before the arrival is counted.  Inline asm: the compiler drops a wait it
//                      believes redundant (after a waited load or a returned atomic its counter reads "empty": MI355X_MICROARCH.md,
//                      "Compiler hazard") and does not look into asm, whose "memory" clobber also keeps the stores in front of it.
//   arrive             a RELAXED agent-scope fetch_add, executed at the memory side: one read-modify-write per node and no cache
//                      maintenance.  The hardware is ordered by the wait before it and the scope of the loads after it; the two signal
//                      fences emit nothing and keep the COMPILER from moving a relaxed store or load across it.
//   load               the sibling's words are loaded at AGENT scope: past the local L2, which may hold a stale line.
// The second arriver's loads follow its own arrival, which follows the first's, which follows the acknowledgement of the first's stores.
namespace climb {
__device__ __forceinline__ uint64_t pair(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }
template <class T> __device__ __forceinline__ void publish(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void wait_acknowledged() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ uint32_t arrive(uint32_t *counter)      // returns how many had arrived before
{
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const uint32_t before = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    return before;
}
template <class T> __device__ __forceinline__ T load(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
}  // namespace climb
