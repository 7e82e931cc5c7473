// rt_bvh_build.hip -- the LBVH builder, which the TLAS shares (rt_lbvh.h, rt_scene.hip), and BLAS construction on the GPU.
//
// Stands in for what the reference enqueues through the Fallback Layer:
//   RtModel::build  -> BottomLevelASGenerator::Generate -> BuildRaytracingAccelerationStructure
//       (libs/DXRFramework/RtModel.cpp:86-118, Helpers/BottomLevelASGenerator.cpp:279-343)
// The builder itself (source absent from the reference checkout) is this engine's
// own: an LBVH whose every integer step is fully determined, so the CPU oracle and
// these kernels produce identical node arrays:
//   1. primitive AABBs + structure AABB           (exact float min/max)
//   2. key = morton30(centre of AABB) << 32 | primitive index   (unique keys)
//   3. ascending radix sort of the 62-bit keys
//   4. Karras 2012 binary radix tree over the sorted keys (integer only)
//   5. bottom-up AABB union (exact float min/max; order independent)
//   6. traversal layout (rt_bvh_ploc.hip, rt_bvh_wide.hip): a better binary tree over the same leaves,
//      collapsed into four-wide 64-B nodes; subtrees of <= leaf_max primitives become leaves.
#include "rt_lbvh.h"

#include <chrono>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "rt_refs.h"

namespace {

__device__ __forceinline__ float wave_min(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ void k_init_bounds(uint32_t *enc)
{
    if (threadIdx.x < 3) enc[threadIdx.x] = ENC_POS_INF;
    else if (threadIdx.x < 6) enc[threadIdx.x] = ENC_NEG_INF;
}

// Structure bounds: wave reduction, then the block's waves meet in LDS and ONE wave issues the six atomics (same-address
// returning atomics serialise at ~11 ns each: six per WAVE cost 0.28 ms on 262 k triangles, six per 1024-thread block 0.02).
constexpr unsigned BOUNDS_BLOCK = 1024;
__device__ __forceinline__ void reduce_bounds(const Box6 &b, bool valid, uint32_t *enc)
{
    __shared__ float part[BOUNDS_BLOCK / 64][6];
    const float inf = __uint_as_float(0x7f800000u);
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, n_waves = (blockDim.x + 63u) >> 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float lo = wave_min(valid ? b.lo[c] : inf);
        const float hi = wave_max(valid ? b.hi[c] : -inf);
        if (lane == 0) { part[wave][c] = lo; part[wave][3 + c] = hi; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const bool is_lo = threadIdx.x < 3;
        float v = part[0][threadIdx.x];
        for (unsigned w = 1; w < n_waves; w++) v = is_lo ? fminf(v, part[w][threadIdx.x]) : fmaxf(v, part[w][threadIdx.x]);
        if (is_lo) atomicMin(&enc[threadIdx.x], f_enc(v));
        else atomicMax(&enc[threadIdx.x], f_enc(v));
    }
}

__global__ void k_tri_boxes(const rt_vertex *__restrict__ verts, const uint32_t *__restrict__ idx, uint32_t n,
                            Box6 *__restrict__ boxes, uint32_t *enc)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Box6 b;
    bool valid = i < n;
    if (valid) {
        float p[3][3];
        tri_positions(verts, idx, i, p);
        b = tri_box(p);
        boxes[i] = b;
    }
    reduce_bounds(b, valid, enc);
}

__global__ void k_box_bounds(const Box6 *__restrict__ boxes, uint32_t n, uint32_t *enc)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Box6 b;
    bool valid = i < n;
    if (valid) {
        // the structure's box holds BOTH corners of every primitive box (oracle_bvh.h box_merge): the same thing unless a box is the
        // empty, inverted one -- an instance none of whose vertices has a number in some axis -- whose corners then reach to both infinities
        b = boxes[i];
        for (int c = 0; c < 3; c++) {
            const float lo = b.lo[c], hi = b.hi[c];
            b.lo[c] = fminf(lo, hi);
            b.hi[c] = fmaxf(lo, hi);
        }
    }
    reduce_bounds(b, valid, enc);
}

__global__ void k_decode_bounds(const uint32_t *enc, float *out)
{
    if (threadIdx.x < 6) out[threadIdx.x] = f_dec(enc[threadIdx.x]);
}

// The world box of a transformed instance: the exact box of its triangles' transformed vertices (oracle_bvh.h
// scene_build; the box of the BLAS box's eight transformed corners is up to 1.6x wider in footprint for a rotated mesh, and a third
// of all instance entries of the 4096-instance frame were false ones, profiles/r04/tight_boxes.txt).  One block per work item =
// (slot of the list, chunk of INST_BOX_REFS vertex references); x' = ((m0 x + m1 y) + m2 z) + m3 as the oracle's xform_point; min / max
// are order free, so the atomics cannot change a bit.  The transform and the encoded box go by slot.  The grid is the host's bound; blocks
// beyond the list's count have nothing to do.  (The scene's kernel, rt_scene.hip: here for the sake of its instructions, rt_lbvh.h.)
__global__ void __launch_bounds__(BOUNDS_BLOCK) k_instance_boxes(const InstanceRec *__restrict__ inst, const uint32_t *__restrict__ pend_idx,
                                                                const float *__restrict__ pend_xf, const uint2 *__restrict__ items,
                                                                const uint32_t *__restrict__ n_items, uint32_t *__restrict__ enc)
{
    if (blockIdx.x >= *n_items) return;                // (block-uniform)
    const uint2 it = items[blockIdx.x];
    const InstanceRec &in = inst[pend_idx[it.x]];
    const float *m = pend_xf + 12u * (size_t)it.x;
    const uint32_t refs = 3u * in.n_prims;
    const float inf = __uint_as_float(0x7f800000u);
    Box6 b;
    for (int c = 0; c < 3; c++) { b.lo[c] = inf; b.hi[c] = -inf; }
    for (uint32_t k = it.y * INST_BOX_REFS + threadIdx.x; k < refs && k < (it.y + 1u) * INST_BOX_REFS; k += BOUNDS_BLOCK) {
        const rt_float3 p = in.verts[in.indices[k]].position;
        for (int r = 0; r < 3; r++) {
            float w = m[4 * r + 0] * p.x;
            w = w + m[4 * r + 1] * p.y;
            w = w + m[4 * r + 2] * p.z;
            w = w + m[4 * r + 3];
            b.lo[r] = fminf(b.lo[r], w);
            b.hi[r] = fmaxf(b.hi[r], w);
        }
    }
    reduce_bounds(b, true, enc + 6u * (size_t)it.x);
}

__global__ void k_morton(const Box6 *__restrict__ boxes, uint32_t n, const float *__restrict__ bounds, uint64_t *__restrict__ keys)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Box6 b = boxes[i];
    keys[i] = ((uint64_t)morton30(b.lo, b.hi, bounds) << 32) | i;
}

__global__ void k_leaves(const uint64_t *__restrict__ keys, const Box6 *__restrict__ boxes, uint32_t n,
                         rt_bvh_node *__restrict__ nodes, uint32_t *__restrict__ parents)
{
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint32_t prim = (uint32_t)(keys[k] & 0xFFFFFFFFull);
    Box6 b = boxes[prim];
    rt_bvh_node nd;
    nd.bmin[0] = b.lo[0]; nd.bmin[1] = b.lo[1]; nd.bmin[2] = b.lo[2];
    nd.bmax[0] = b.hi[0]; nd.bmax[1] = b.hi[1]; nd.bmax[2] = b.hi[2];
    nd.left = prim;
    nd.right = RT_LEAF;
    nodes[n - 1 + k] = nd;
    if (n == 1) parents[0] = 0xFFFFFFFFu;
}

__device__ __forceinline__ int key_delta(const uint64_t *__restrict__ k, int n, int i, int j)
{
    if (j < 0 || j >= n) return -1;
    return __clzll((long long)(k[i] ^ k[j]));
}

// Karras, "Maximizing parallelism in the construction of BVHs, octrees, and k-d trees", HPG 2012.
__global__ void k_karras(const uint64_t *__restrict__ keys, int n, rt_bvh_node *__restrict__ nodes,
                         uint32_t *__restrict__ parents, uint2 *__restrict__ ranges)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    int d = (key_delta(keys, n, i, i + 1) - key_delta(keys, n, i, i - 1)) > 0 ? 1 : -1;
    int dmin = key_delta(keys, n, i, i - d);
    int lmax = 2;
    while (key_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (key_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    int j = i + l * d;
    int dnode = key_delta(keys, n, i, j);
    int s = 0;
    int t = l;
    do {
        t = (t + 1) >> 1;
        if (key_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    int gamma = i + s * d + min(d, 0);
    int first = min(i, j), last = max(i, j);
    uint32_t leaf0 = (uint32_t)(n - 1);
    uint32_t left = (first == gamma) ? leaf0 + (uint32_t)gamma : (uint32_t)gamma;
    uint32_t right = (last == gamma + 1) ? leaf0 + (uint32_t)(gamma + 1) : (uint32_t)(gamma + 1);
    nodes[i].left = left;
    nodes[i].right = right;
    parents[left] = (uint32_t)i;
    parents[right] = (uint32_t)i;
    if (i == 0) parents[0] = 0xFFFFFFFFu;
    ranges[i] = make_uint2((uint32_t)first, (uint32_t)last);
}

// Bottom-up union, every internal node visited ONCE: the climb of rt_bvh_tree.h ("the ordering of a bottom-up climb"), in the shape
// publish, then arrive.  A thread publishes its node's box and depth, waits until the stores are acknowledged, only then bumps the parent's
// arrival counter; the second arriver reads the sibling's words and unites.  One read-modify-write per node; the first round-2 version
// exchanged every word with one (14 per node, 0.15 ms for 262 k triangles), round 1's min/max climb issued ~180 per leaf.  min / max are
// exact and order independent, so the boxes are the oracle's bit for bit.  Scratch per node: 6 box words + depth + arrival counter = 8
// words (three 64-bit pairs and two words), zero-initialised.
__global__ void k_refit(const rt_bvh_node *__restrict__ nodes, const uint32_t *__restrict__ parents, uint32_t n,
                        uint32_t *__restrict__ scratch, uint32_t *__restrict__ max_depth)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const rt_bvh_node nd = nodes[n - 1 + k];
    float lo[3] = {nd.bmin[0], nd.bmin[1], nd.bmin[2]}, hi[3] = {nd.bmax[0], nd.bmax[1], nd.bmax[2]};
    uint32_t depth = 0, cur = n - 1 + k;
    for (;;) {
        const uint32_t parent = parents[cur];
        if (parent == 0xFFFFFFFFu) { atomicMax(max_depth, depth); return; }       // cur is the root
        // publish this node (leaves too: the sibling's climber reads them the same way), then arrive
        uint64_t *mine = reinterpret_cast<uint64_t *>(scratch + (size_t)cur * 8);
        climb::publish(&mine[0], climb::pair(__float_as_uint(lo[0]), __float_as_uint(lo[1])));
        climb::publish(&mine[1], climb::pair(__float_as_uint(lo[2]), __float_as_uint(hi[0])));
        climb::publish(&mine[2], climb::pair(__float_as_uint(hi[1]), __float_as_uint(hi[2])));
        // (word 7 of a node is its arrival counter: the depth is published as a 32-bit store so that it is left alone)
        climb::publish(scratch + (size_t)cur * 8 + 6, depth);
        climb::wait_acknowledged();
        if (climb::arrive(&scratch[(size_t)parent * 8 + 7]) == 0u) return;       // the sibling's climber will take over from here
        const rt_bvh_node pn = nodes[parent];
        const uint32_t sib = pn.left == cur ? pn.right : pn.left;
        const uint64_t *other = reinterpret_cast<const uint64_t *>(scratch + (size_t)sib * 8);
        const uint64_t o0 = climb::load(&other[0]), o1 = climb::load(&other[1]), o2 = climb::load(&other[2]);
        const uint32_t od = climb::load(scratch + (size_t)sib * 8 + 6);
        lo[0] = fminf(lo[0], __uint_as_float((uint32_t)o0));
        lo[1] = fminf(lo[1], __uint_as_float((uint32_t)(o0 >> 32)));
        lo[2] = fminf(lo[2], __uint_as_float((uint32_t)o1));
        hi[0] = fmaxf(hi[0], __uint_as_float((uint32_t)(o1 >> 32)));
        hi[1] = fmaxf(hi[1], __uint_as_float((uint32_t)o2));
        hi[2] = fmaxf(hi[2], __uint_as_float((uint32_t)(o2 >> 32)));
        depth = (depth > od ? depth : od) + 1u;
        cur = parent;
    }
}

// the boxes the climbers left in the scratch -> the internal nodes (the root's, which nobody published, is the union of
// its children's)
__global__ void k_refit_decode(const uint32_t *__restrict__ scratch, rt_bvh_node *__restrict__ nodes, uint32_t n_internal)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_internal) return;
    if (i == 0) {
        const uint32_t *a = scratch + (size_t)nodes[0].left * 8, *b = scratch + (size_t)nodes[0].right * 8;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            nodes[0].bmin[c] = fminf(__uint_as_float(a[c]), __uint_as_float(b[c]));
            nodes[0].bmax[c] = fmaxf(__uint_as_float(a[3 + c]), __uint_as_float(b[3 + c]));
        }
        return;
    }
    const uint32_t *p = scratch + (size_t)i * 8;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        nodes[i].bmin[c] = __uint_as_float(p[c]);
        nodes[i].bmax[c] = __uint_as_float(p[3 + c]);
    }
}

__global__ void k_gather_tris(const uint64_t *__restrict__ keys, const rt_vertex *__restrict__ verts, const uint32_t *__restrict__ idx, uint32_t n, TriRec *__restrict__ tris)
{
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint32_t prim = (uint32_t)(keys[k] & 0xFFFFFFFFull);
    float p[3][3];
    tri_positions(verts, idx, prim, p);
    tris[k] = tri_record(p, prim, 0u);
}

// the vertex normals of every primitive, gathered once per build into one record per primitive (shading reads them per hit)
__global__ void k_normal_records(const rt_vertex *__restrict__ verts, const uint32_t *__restrict__ idx, uint32_t n, TriRec *__restrict__ out)
{
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const rt_float3 n0 = verts[idx[3 * p + 0]].normal;
    const rt_float3 n1 = verts[idx[3 * p + 1]].normal;
    const rt_float3 n2 = verts[idx[3 * p + 2]].normal;
    TriRec t;
    t.a = make_float4(n0.x, n0.y, n0.z, n1.x);
    t.b = make_float4(n1.y, n1.z, n2.x, n2.y);
    t.c = make_float4(n2.z, 0.0f, 0.0f, 0.0f);
    out[p] = t;
}

// 64-bit sum of n 32-bit counts (grid-stride; one atomic per wave)
__global__ void k_sum64(const uint32_t *__restrict__ v, uint32_t n, unsigned long long *__restrict__ out)
{
    unsigned long long s = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) s += v[i];
    for (int o = 32; o > 0; o >>= 1) s += (unsigned long long)__shfl_xor((long long)s, o, 64);
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(out, s);
}

// ---- split references (rt_refs.h): count the pieces of every triangle, then (after a scan) write their boxes ----
__device__ __forceinline__ float ref_min_len(const float *__restrict__ bounds)
{
    const float ex = bounds[3] - bounds[0], ey = bounds[4] - bounds[1], ez = bounds[5] - bounds[2];
    return rtd::ref_max2(rtd::ref_max2(ex, ey), ez) * 0.001953125f;          // the model's longest extent / 512
}
__global__ void k_ref_count(const rt_vertex *__restrict__ verts, const uint32_t *__restrict__ idx, uint32_t n, const float *__restrict__ bounds,
                            uint32_t *__restrict__ count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { count[n] = 0u; return; }           // (the scan's last element: the total)
    float p[3][3];
    tri_positions(verts, idx, i, p);
    int axis;
    count[i] = rtd::ref_pieces(p, ref_min_len(bounds), axis);
}
__global__ void k_ref_emit(const rt_vertex *__restrict__ verts, const uint32_t *__restrict__ idx, uint32_t n, const float *__restrict__ bounds,
                           const uint32_t *__restrict__ off, float *__restrict__ ref_boxes, uint32_t *__restrict__ ref_prim)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float p[3][3];
    tri_positions(verts, idx, i, p);
    const uint32_t first = off[i], k = off[i + 1] - first;
    if (k == 1u) {                                     // not split: its own box
        const Box6 own = tri_box(p);
        float *b = ref_boxes + 6 * (size_t)first;
        for (int q = 0; q < 3; q++) { b[q] = own.lo[q]; b[3 + q] = own.hi[q]; }
        ref_prim[first] = i;
        return;
    }
    int axis;
    (void)rtd::ref_pieces(p, ref_min_len(bounds), axis);
    for (uint32_t j = 0; j < k; j++) {
        float b[6];
        rtd::ref_box(p, axis, k, j, b);
        for (int q = 0; q < 6; q++) ref_boxes[6 * (size_t)(first + j) + q] = b[q];
        ref_prim[first + j] = i;
    }
}
// Morton keys of the references (the LBVH's codes, over the same bounds) and, after the sort, the leaves PLOC starts from
__global__ void k_ref_keys(const float *__restrict__ ref_boxes, uint32_t m, const float *__restrict__ bounds, uint64_t *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const float *b = ref_boxes + 6 * (size_t)i;
    keys[i] = ((uint64_t)morton30(b, b + 3, bounds) << 32) | i;
}
__global__ void k_ref_leaves(const uint64_t *__restrict__ keys, uint32_t m, const float *__restrict__ ref_boxes, const uint32_t *__restrict__ ref_prim,
                             float *__restrict__ leaf_box, uint32_t *__restrict__ leaf_prim)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const uint32_t r = (uint32_t)(keys[k] & 0xFFFFFFFFull);
    for (int q = 0; q < 6; q++) leaf_box[6 * (size_t)k + q] = ref_boxes[6 * (size_t)r + q];
    leaf_prim[k] = ref_prim[r];
}
// a model with split triangles in a layout that holds every triangle once (LBVH layout): its records say "validate by primitive"
__global__ void k_ref_mark_records(TriRec *__restrict__ tris, uint32_t n, const uint32_t *__restrict__ off)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t prim = __float_as_uint(tris[k].c.y);
    if (off[prim + 1] - off[prim] > 1u) tris[k].c.z = __uint_as_float(2u);
}

// the temporaries of a BLAS build: the LBVH's (rt_lbvh.h) + the reference count of every triangle, its scan and the scan's scratch
struct BlasTemps : LbvhTemps {
    uint32_t *ref_count, *ref_off;      // n + 1 each
    void *scan; size_t scan_bytes;
};
void carve_blas(Carver &c, uint32_t n, BlasTemps &t)
{
    carve_lbvh(c, n, t);
    t.ref_count = c.take<uint32_t>((size_t)n + 1);
    t.ref_off = c.take<uint32_t>((size_t)n + 1);
    t.scan_bytes = (size_t)1 << 20;
    t.scan = c.take<char>(t.scan_bytes);
}
// A rocPRIM call with its temporary storage: call(storage, bytes) asks for the size when storage is null and queues the work otherwise.
// tmp adopts the arena's slice (nullptr: none) or, if the library asks for more, becomes an allocation of its own: the caller says where it lives.
template <class Call> int rocprim_with_temp(DevBuf &tmp, void *slice, size_t slice_bytes, Call call)
{
    size_t bytes = 0;
    HIP_TRY(call(nullptr, bytes));
    tmp.adopt(slice, slice_bytes);
    RT_TRY(tmp.reserve(bytes));
    HIP_TRY(call(tmp.p, bytes));
    return RT_OK;
}
int sort_by_morton_code(DevBuf &tmp, void *slice, size_t slice_bytes, uint64_t *keys, uint64_t *sorted, uint32_t n, hipStream_t st)
{
    return rocprim_with_temp(tmp, slice, slice_bytes, [&](void *storage, size_t &bytes) { return rocprim::radix_sort_keys(storage, bytes, keys, sorted, n, 32, 62, st); });
}
void drop_build_arena_if_large(rt_context *ctx)
{
    if (ctx->build_arena.bytes > ((size_t)256 << 20)) ctx->build_arena.release();      // keep small arenas for the next build
}

}  // namespace

// ---- the builder's host entry points (rt_lbvh.h) ----

void lbvh_queue_box_bounds(rt_context *ctx, uint32_t n, const LbvhTemps &t)
{
    k_init_bounds<<<1, 64, 0, ctx->stream>>>(t.enc);
    k_box_bounds<<<grid_for(n, BOUNDS_BLOCK), BOUNDS_BLOCK, 0, ctx->stream>>>(t.boxes, n, t.enc);
    k_decode_bounds<<<1, 64, 0, ctx->stream>>>(t.enc, t.bounds);
}

void lbvh_queue_instance_boxes(rt_context *ctx, uint32_t max_items, const InstanceRec *inst, const uint32_t *pend_idx, const float *pend_xf, const uint2 *items,
                               const uint32_t *n_items, uint32_t *enc)
{
    k_instance_boxes<<<max_items, BOUNDS_BLOCK, 0, ctx->stream>>>(inst, pend_idx, pend_xf, items, n_items, enc);
}

int lbvh_from_boxes(rt_context *ctx, BvhDev &bv, uint32_t n, const LbvhTemps &t)
{
    hipStream_t st = ctx->stream;
    const unsigned B = 256;
    // the traversal addresses a node as base + (index << RT_NODE_SHIFT) with a 32-bit byte offset (rt_trace_wave.h): 64-B nodes
    // leave room for 2^26 of them
    constexpr uint32_t kMaxPrims = 1u << (32 - RT_NODE_SHIFT);
    if (n > kMaxPrims) { rt_set_error("acceleration structure over %u primitives: the limit is 2^%d (%u)", n, 32 - RT_NODE_SHIFT, kMaxPrims); return RT_ERR_UNSUPPORTED; }
    bv.n = n;
    RT_TRY(bv.nodes.reserve(sizeof(rt_bvh_node) * (2 * (size_t)n - 1)));
    RT_TRY(bv.keys.reserve(sizeof(uint64_t) * n));
    RT_TRY(bv.parents.reserve(sizeof(uint32_t) * (2 * (size_t)n - 1)));
    RT_TRY(bv.ranges.reserve(sizeof(uint2) * (n > 1 ? n - 1 : 1)));

    k_morton<<<grid_for(n, B), B, 0, st>>>(t.boxes, n, t.bounds, t.keys);
    // keys are (30-bit Morton code << 32) | index with the indices ascending on input: a STABLE sort of the code bits alone
    // gives the order of the full 64-bit keys (the oracle's) with half the radix passes
    DevBuf sort_tmp;
    RT_TRY(sort_by_morton_code(sort_tmp, t.sort, t.sort_bytes, t.keys, bv.keys.as<uint64_t>(), n, st));

    rt_bvh_node *nodes = bv.nodes.as<rt_bvh_node>();
    uint32_t *parents = bv.parents.as<uint32_t>();
    k_leaves<<<grid_for(n, B), B, 0, st>>>(bv.keys.as<uint64_t>(), t.boxes, n, nodes, parents);
    HIP_TRY(hipMemsetAsync(t.depth, 0, sizeof(uint32_t), st));
    if (n > 1) {
        k_karras<<<grid_for(n - 1, B), B, 0, st>>>(bv.keys.as<uint64_t>(), (int)n, nodes, parents, bv.ranges.as<uint2>());
        HIP_TRY(hipMemsetAsync(t.refit_enc, 0, sizeof(uint32_t) * 8 * (2 * (size_t)n - 1), st));
        k_refit<<<grid_for(n, B), B, 0, st>>>(nodes, parents, n, t.refit_enc, t.depth);
        k_refit_decode<<<grid_for(n - 1, B), B, 0, st>>>(t.refit_enc, nodes, n - 1);
    }
    HIP_TRY(hipGetLastError());
    // depth and bounds come back through page-locked memory and are picked up by lbvh_collect() once the caller has queued
    // the rest of the build: no host round trip in the middle of it
    uint32_t *back = ctx->pinned ? ctx->pinned + RT_PINNED_LBVH : nullptr;
    HIP_TRY(hipMemcpyAsync(back ? (void *)back : (void *)&bv.max_depth, t.depth, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(back ? (void *)(back + 1) : (void *)bv.bounds, t.bounds, 6 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (!back) HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

int lbvh_collect(rt_context *ctx, BvhDev &bv)
{
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->pinned) {
        bv.max_depth = ctx->pinned[RT_PINNED_LBVH];
        memcpy(bv.bounds, ctx->pinned + RT_PINNED_LBVH + 1, 6 * sizeof(float));
    }
    return RT_OK;
}

// ---- the steps of a BLAS build (rt_build_blas) ----

namespace {

constexpr unsigned BB = 256;

// option verbose=1: wall time of each build phase on stderr (synchronises: diagnostics only)
struct PhaseClock {
    rt_context *ctx;
    std::chrono::steady_clock::time_point prev = std::chrono::steady_clock::now();
    void mark(const char *what)
    {
        if (!ctx->verbose) return;
        (void)hipStreamSynchronize(ctx->stream);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[dxr_amd]   BLAS %-18s %7.3f ms\n", what, std::chrono::duration<double, std::milli>(now - prev).count());
        prev = now;
    }
};

// The references of a model with split triangles (rt_refs.h), from their count to the leaves the production tree is built from.  The
// buffers live until the build's last step has been queued and joined: freeing one earlier would wait for the device in mid-build.
struct RefLeaves {
    uint32_t n_refs = 0;         // boxes all triangles together are validated against: n_tris when none is split
    bool split_layout = false;   // the production tree gets one leaf per reference
    DevBuf prim, keys, sorted, sort_tmp, leaf_box, leaf_prim;
};

int blas_boxes_and_bounds(rt_context *ctx, rt_model *m, const BlasTemps &t, PhaseClock &clock)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = m->n_tris;
    RT_TRY(m->tris.reserve(sizeof(TriRec) * (size_t)n));
    RT_TRY(m->normals.reserve(sizeof(TriRec) * (size_t)n));
    clock.mark("tris alloc");
    k_init_bounds<<<1, 64, 0, st>>>(t.enc);
    k_tri_boxes<<<grid_for(n, BOUNDS_BLOCK), BOUNDS_BLOCK, 0, st>>>(m->d_verts.as<rt_vertex>(), m->d_idx.as<uint32_t>(), n, t.boxes, t.enc);
    k_decode_bounds<<<1, 64, 0, st>>>(t.enc, t.bounds);
    clock.mark("alloc + boxes");
    return RT_OK;
}

int blas_records(rt_context *ctx, rt_model *m)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = m->n_tris;
    k_gather_tris<<<grid_for(n, BB), BB, 0, st>>>(m->blas.keys.as<uint64_t>(), m->d_verts.as<rt_vertex>(), m->d_idx.as<uint32_t>(), n, m->tris.as<TriRec>());
    k_normal_records<<<grid_for(n, BB), BB, 0, st>>>(m->d_verts.as<rt_vertex>(), m->d_idx.as<uint32_t>(), n, m->normals.as<TriRec>());
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// Split references (rt_refs.h): how many boxes every triangle is validated against.  One each leaves the model as it was; otherwise the
// boxes by primitive (the canonical walk validates against them) and the primitive of every reference.
int blas_split_refs(rt_context *ctx, rt_model *m, const BlasTemps &t, RefLeaves &r)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = m->n_tris;
    m->n_recs = n;
    m->rec_boxes.release(); m->ref_off.release(); m->ref_boxes.release();      // (a rebuild starts from a model without references)
    k_ref_count<<<grid_for(n + 1, BB), BB, 0, st>>>(m->d_verts.as<rt_vertex>(), m->d_idx.as<uint32_t>(), n, t.bounds, t.ref_count);
    DevBuf scan_tmp;
    RT_TRY(rocprim_with_temp(scan_tmp, t.scan, t.scan_bytes, [&](void *storage, size_t &bytes) {
        return rocprim::exclusive_scan(storage, bytes, t.ref_count, t.ref_off, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st);
    }));
    r.n_refs = n;
    uint32_t *back = ctx->pinned ? ctx->pinned : &r.n_refs;
    HIP_TRY(hipMemcpyAsync(back, t.ref_off + n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    r.n_refs = *back;
    // up to RT_REF_MAX_PIECES references per triangle: beyond 2^32 / 128 triangles the 32-bit scan can wrap past a plausible
    // total, so such a mesh has its counts summed again in 64 bits
    if ((uint64_t)n * RT_REF_MAX_PIECES > 0xFFFFFFFFull) {
        DevBuf sum64;
        unsigned long long total64 = 0;
        RT_TRY(sum64.reserve(8));
        HIP_TRY(hipMemsetAsync(sum64.p, 0, 8, st));
        k_sum64<<<1024, BB, 0, st>>>(t.ref_count, n, sum64.as<unsigned long long>());
        HIP_TRY(hipMemcpyAsync(&total64, sum64.p, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (total64 != (unsigned long long)r.n_refs) { rt_set_error("split references: %llu for %u triangles", total64, n); return RT_ERR_UNSUPPORTED; }
    }
    if (r.n_refs == n) return RT_OK;
    if (r.n_refs < n || r.n_refs > (1u << (32 - RT_NODE_SHIFT))) { rt_set_error("split references: %u for %u triangles", r.n_refs, n); return RT_ERR_UNSUPPORTED; }
    RT_TRY(m->ref_off.reserve(4 * ((size_t)n + 1)));
    HIP_TRY(hipMemcpyAsync(m->ref_off.p, t.ref_off, 4 * ((size_t)n + 1), hipMemcpyDeviceToDevice, st));
    RT_TRY(m->ref_boxes.reserve(24 * (size_t)r.n_refs));
    RT_TRY(r.prim.reserve(4 * (size_t)r.n_refs));
    k_ref_emit<<<grid_for(n, BB), BB, 0, st>>>(m->d_verts.as<rt_vertex>(), m->d_idx.as<uint32_t>(), n, t.bounds, m->ref_off.as<uint32_t>(),
                                             m->ref_boxes.as<float>(), r.prim.as<uint32_t>());
    if (ctx->verbose) fprintf(stderr, "[dxr_amd]   BLAS %u triangles -> %u references\n", n, r.n_refs);
    return RT_OK;
}

// the references in Morton order: the leaves of the production tree
int blas_ref_leaves(rt_context *ctx, rt_model *m, const BlasTemps &t, RefLeaves &r)
{
    hipStream_t st = ctx->stream;
    const uint32_t n_refs = r.n_refs;
    RT_TRY(r.keys.reserve(8 * (size_t)n_refs));
    RT_TRY(r.sorted.reserve(8 * (size_t)n_refs));
    RT_TRY(r.leaf_box.reserve(24 * (size_t)n_refs));
    RT_TRY(r.leaf_prim.reserve(4 * (size_t)n_refs));
    k_ref_keys<<<grid_for(n_refs, BB), BB, 0, st>>>(m->ref_boxes.as<float>(), n_refs, t.bounds, r.keys.as<uint64_t>());
    RT_TRY(sort_by_morton_code(r.sort_tmp, nullptr, 0, r.keys.as<uint64_t>(), r.sorted.as<uint64_t>(), n_refs, st));
    k_ref_leaves<<<grid_for(n_refs, BB), BB, 0, st>>>(r.sorted.as<uint64_t>(), n_refs, m->ref_boxes.as<float>(), r.prim.as<uint32_t>(),
                                                    r.leaf_box.as<float>(), r.leaf_prim.as<uint32_t>());
    return RT_OK;
}

// production traversal layout: re-cluster the same leaves with PLOC (rt_bvh_ploc.hip), then collapse the binary
// tree into wide quantised nodes (rt_bvh_wide.hip); tiny meshes and option fast_bvh=lbvh collapse the LBVH itself
int blas_layout(rt_context *ctx, rt_model *m, const RefLeaves &r, PhaseClock &clock)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = m->n_tris;
    bool ploc_done = false;
    if (ctx->use_ploc) {
        const PlocLeaves leaves = r.split_layout ? PlocLeaves{r.n_refs, r.leaf_box.as<float>(), r.leaf_prim.as<uint32_t>()} : PlocLeaves{};
        const int rc = rt_build_ploc_layout(ctx, m, &ploc_done, leaves);
        // PLOC's nearest-neighbour rounds make no progress on boxes whose surface is not finite (NaN / inf vertices,
        // extents that overflow): such a mesh keeps the LBVH as its traversal layout.  rt_build_ploc_layout may give up AFTER k_ploc_tris
        // had rewritten m->tris in PLOC order (the collapse that follows it can refuse a tree too), so the records are gathered again
        // in LBVH order whatever the mesh: that is the order the collapse below and k_ref_mark_records index
        if (rc == RT_ERR_STATE || (rc == RT_OK && ctx->opt_fail_ploc_rounds)) {      // (the option: tests force this path)
            ploc_done = false;
            if (r.split_layout) {
                // the split-reference path had grown m->tris for one record per REFERENCE (DevBuf::reserve keeps no contents):
                // back to one record per triangle
                m->rec_boxes.release();
                m->n_recs = n;
                RT_TRY(m->tris.reserve(sizeof(TriRec) * (size_t)n));
            }
            k_gather_tris<<<grid_for(n, BB), BB, 0, st>>>(m->blas.keys.as<uint64_t>(), m->d_verts.as<rt_vertex>(),
                                                        m->d_idx.as<uint32_t>(), n, m->tris.as<TriRec>());
        } else RT_TRY(rc);
    }
    clock.mark("PLOC + wide layout");
    if (!ploc_done) RT_TRY(rt_build_wide_from_lbvh(ctx, m->blas, false, ctx->leaf_max));
    if (r.n_refs > n && !(ploc_done && r.split_layout)) {
        // a layout with one record per triangle (LBVH; PLOC with the option split_refs=0): split triangles are validated by primitive
        m->n_recs = n;
        k_ref_mark_records<<<grid_for(n, BB), BB, 0, st>>>(m->tris.as<TriRec>(), n, m->ref_off.as<uint32_t>());
    }
    clock.mark("wide layout (LBVH)");
    return RT_OK;
}

int blas_steps(rt_context *ctx, rt_model *m, PhaseClock &clock)
{
    const uint32_t n = m->n_tris;
    BlasTemps t;
    RefLeaves refs;
    RT_TRY(take_build_temps(ctx, n, t, [n](Carver &c, BlasTemps &bt) { carve_blas(c, n, bt); }));
    clock.mark("arena");
    RT_TRY(blas_boxes_and_bounds(ctx, m, t, clock));
    RT_TRY(lbvh_from_boxes(ctx, m->blas, n, t));
    clock.mark("LBVH");
    RT_TRY(blas_records(ctx, m));
    RT_TRY(blas_split_refs(ctx, m, t, refs));
    refs.split_layout = refs.n_refs > n && ctx->opt_split_refs && ctx->use_ploc;
    if (refs.split_layout) RT_TRY(blas_ref_leaves(ctx, m, t, refs));
    clock.mark("gather");
    RT_TRY(blas_layout(ctx, m, refs, clock));
    RT_TRY(lbvh_collect(ctx, m->blas));
    m->built = true;
    return RT_OK;
}

}  // namespace

int rt_build_blas(rt_context *ctx, rt_model *m)
{
    if (m->built) return RT_OK;
    PhaseClock clock{ctx};
    const int rc = blas_steps(ctx, m, clock);          // (its buffers are gone when it returns, whichever way)
    drop_build_arena_if_large(ctx);
    clock.mark("free");
    return rc;
}
