// rt_bvh_ploc.hip -- traversal-layout optimiser for a BLAS.
//
// The canonical acceleration structure (rt_bvh_build.hip) is an LBVH: fully determined,
// index-exact against the oracle, but only spatial-median quality (~95 box tests per primary
// ray on the Sponza-class scene).  Results do not depend on the tree that is walked (DESIGN.md
// "Exactness rule"), so the PRODUCTION traversal is free to use a better hierarchy over the
// same triangles.  This file builds one with PLOC (parallel locally-ordered clustering,
// Meister & Bittner 2018): clusters start as the Morton-sorted leaves of the canonical tree;
// every round each cluster finds, inside a window of +-RADIUS neighbours, the partner that
// minimises the surface area of the merged box; mutual pairs merge; the cluster array is
// compacted in order (prefix sums by workgroup index, rt_level_scan.h), until one cluster is left.
// Node ids come from those prefix sums, so the build is run-to-run deterministic.  A round is two
// launches; its cluster count lives in device memory and the host launches a batch of rounds blind.
//
// Output: triangles re-gathered in the depth-first order of the new tree, so that every subtree is a
// contiguous triangle range and subtrees of <= leaf_max triangles collapse to leaves, and the binary
// tree itself, which rt_bvh_wide.hip collapses into the four-wide 64-B nodes the traversal walks.
#include "rt_bvh_tree.h"

#include "rt_level_scan.h"

#include <cstring>

namespace {

// Search window.  Measured on the three bench scenes, frame ms (1080p 262 k triangles / 4K 10 M triangles, 4 bounces / 4K 4096
// instances): radius 2: 2.75 / 16.3 / 6.28, 3: 2.70 / 15.9, 4: 2.64 / 15.4 / 6.20, 6: 2.83 / 15.6, 8: 2.76 / 15.4 / 6.24,
// 12: 2.82 / 15.9 / 6.17, 16: 2.87 / 16.3 -- a few per cent of tree-quality noise, no trend towards wide windows once the
// binary tree is collapsed four wide; 4 is also the cheapest to build.
#ifndef RT_PLOC_RADIUS
#define RT_PLOC_RADIUS 4
#endif
constexpr int PLOC_RADIUS = RT_PLOC_RADIUS;
#ifndef RT_PLOC_TAIL_RADIUS
#define RT_PLOC_TAIL_RADIUS RT_PLOC_RADIUS
#endif
constexpr int PLOC_TAIL_RADIUS = RT_PLOC_TAIL_RADIUS;       // window of the single-workgroup rounds at the top of the tree
constexpr unsigned PB = 256;

// where the clustering stands before round r (device memory, one entry per round of a batch)
struct PlocRound { uint32_t c, next_node, cur, error; };
constexpr uint32_t PLOC_TAIL = 2048, TAIL_BLOCK = 1024, PLOC_MAX_BATCH = 64;   // (tail at 4096: 0.20 ms in the one workgroup; a multi-kernel round costs ~12 us)

// the arrays the PLOC rounds read and write
struct PlocArrays {
    uint32_t *nn, *flags;
    uint64_t *tally;                   // per workgroup: clusters kept (low word) and nodes created (high word)
    uint32_t *arrivals;
    PlocRound *round;                  // PLOC_MAX_BATCH + 1 entries
    uint32_t *cl_node[2];
    Box6 *cl_box[2];
    BinTree tree;                      // what the rounds build (its offsets: k_ploc_offsets, once the tree stands)
};

// ---- the steps of a round, each written once: taken by the multi-kernel rounds (k_ploc_pair, k_ploc_apply) and by the tail (k_ploc_tail) ----
// The nearest neighbour of cluster i of c inside the window of R either side: smallest merged area, ties -> lower index (itself, if it has
// no neighbour).  box_at(j): the box of cluster j.
template <int R, class BoxAt> __device__ __forceinline__ uint32_t ploc_nearest(int i, int c, BoxAt box_at)
{
    const Box6 me = box_at(i);
    float best = __uint_as_float(0x7f800000u);
    uint32_t arg = (uint32_t)i;
    for (int d = -R; d <= R; d++) {
        const int j = i + d;
        if (d == 0 || j < 0 || j >= c) continue;
        const float ar = merged_area(me, box_at(j));
        if (ar < best) { best = ar; arg = (uint32_t)j; }
    }
    return arg;
}
// What becomes of cluster i whose nearest neighbour is j (nn_at(j): j's own): of a mutual pair the lower index creates the node and the
// higher one disappears; every other cluster is kept as it is.
template <class NnAt> __device__ __forceinline__ void ploc_flags(uint32_t i, uint32_t j, NnAt nn_at, uint32_t &kept, uint32_t &created)
{
    const bool mutual = j != i && nn_at(j) == i;
    created = (mutual && i < j) ? 1u : 0u;
    kept = (mutual && i > j) ? 0u : 1u;
}
// Node m from the clusters with the ids na, nb and the boxes ba, bb: its children, box and size, the three parents; returns the box.
// size_sum(): the leaves below the two (the rounds read them from the tree, the tail keeps them in LDS), asked for where the rounds always
// read them: behind the stores of the children and the box.
template <class SizeSum> __device__ __forceinline__ Box6 ploc_merge(const BinTree &t, uint32_t m, uint32_t na, uint32_t nb, const Box6 &ba, const Box6 &bb,
                                                                    SizeSum size_sum, uint32_t &size)
{
    const Box6 u = box_union(ba, bb);
    t.left[m - t.n] = na; t.right[m - t.n] = nb;
    t.box[m] = u;
    t.size[m] = size = size_sum();
    t.parent[na] = m; t.parent[nb] = m; t.parent[m] = 0xFFFFFFFFu;
    return u;
}

// clusters start as the canonical leaves, in key order
// (leaf_box6 != nullptr: the leaves are the references of a model with split triangles, rt_refs.h -- 6 floats each, in Morton order)
__global__ void k_ploc_init(const rt_bvh_node *__restrict__ nodes, const float *__restrict__ leaf_box6, uint32_t n, uint32_t *__restrict__ cl_node, Box6 *__restrict__ cl_box,
                            uint32_t *__restrict__ size, uint32_t *__restrict__ parent, PlocRound *__restrict__ round0, uint32_t *__restrict__ arrivals)
{
    const uint32_t k = blockIdx.x * PB + threadIdx.x;
    if (k == 0) { const PlocRound r0 = {n, n, 0u, 0u}; *round0 = r0; *arrivals = 0; }
    if (k >= n) return;
    Box6 b;
    if (leaf_box6) {
        for (int c = 0; c < 3; c++) { b.lo[c] = leaf_box6[6 * (size_t)k + c]; b.hi[c] = leaf_box6[6 * (size_t)k + 3 + c]; }
    } else {
        const rt_bvh_node nd = nodes[n - 1 + k];
        for (int c = 0; c < 3; c++) { b.lo[c] = nd.bmin[c]; b.hi[c] = nd.bmax[c]; }
    }
    cl_node[k] = k;                 // node ids: leaves 0..n-1 (key order), internal n..2n-2 (creation order)
    cl_box[k] = b;
    size[k] = 1;
    parent[k] = 0xFFFFFFFFu;
}

// First half of a round.  Nearest neighbour inside the window (smallest merged area, ties -> lower index) for the
// workgroup's clusters and a halo of RADIUS either side, so that "is the choice mutual" needs no second launch; then the
// flags (bit 0: the cluster survives, bit 1: it creates a node), the workgroup's tally, and -- in the last workgroup to
// arrive -- the offsets of all workgroups and the size of the next round.
__global__ void __launch_bounds__(PB) k_ploc_pair(PlocArrays a, uint32_t r)
{
    constexpr int R = PLOC_RADIUS;
    __shared__ Box6 tile[PB + 4 * R];
    __shared__ uint32_t near[PB + 2 * R];
    __shared__ uint64_t lds64[PB];
    __shared__ uint32_t lds[PB / 64];
    __shared__ uint32_t lds_flag;
    const PlocRound s = a.round[r];
    if (s.c <= PLOC_TAIL || s.error) {                 // the tail kernel's share, or a failed round: hand the state on
        if (blockIdx.x == 0 && threadIdx.x == 0) a.round[r + 1] = s;
        return;
    }
    const uint32_t c = s.c, nblocks = (c + PB - 1) / PB;
    if (blockIdx.x >= nblocks) return;
    const Box6 *cl_box = a.cl_box[s.cur];
    const int base = (int)(blockIdx.x * PB) - 2 * R;    // tile[t] = cluster base + t
    for (int t = threadIdx.x; t < (int)PB + 4 * R; t += PB) {
        const int g = base + t;
        if (g >= 0 && g < (int)c) tile[t] = cl_box[g];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < (int)PB + 2 * R; t += PB) {       // near[t] = nn of cluster base + R + t
        const int i = base + R + t;
        if (i < 0 || i >= (int)c) continue;
        near[t] = ploc_nearest<R>(i, (int)c, [&](int j) -> const Box6 & { return tile[j - base]; });
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * PB + threadIdx.x;
    uint32_t packed = 0;                                // kept | created << 16
    if (i < c) {
        const uint32_t j = near[threadIdx.x + R];
        uint32_t kp, mg;
        ploc_flags(i, j, [&](uint32_t o) { return near[(int)o - base - R]; }, kp, mg);
        a.nn[i] = j;
        a.flags[i] = kp | (mg << 1);
        packed = kp | (mg << 16);
    }
    uint32_t block_total;
    (void)rt_scan::block_exclusive<PB>(packed, lds, block_total);
    const uint64_t mine = (uint64_t)(block_total & 0xFFFFu) | ((uint64_t)(block_total >> 16) << 32);
    if (!rt_scan::publish_and_arrive(a.tally, mine, a.arrivals, nblocks, &lds_flag)) return;
    const uint64_t total = rt_scan::scan_tallies<uint64_t, PB>(a.tally, nblocks, lds64);
    if (threadIdx.x == 0) {
        const uint32_t kept = (uint32_t)total, created = (uint32_t)(total >> 32);
        PlocRound nx = {kept, s.next_node + created, s.cur ^ 1u, 0u};
        if (created == 0 || kept != c - created) { nx = s; nx.error = 1; }      // no progress: reported by the host
        a.round[r + 1] = nx;
        *a.arrivals = 0;
    }
}

// Second half: every surviving cluster moves to its place in the other cluster array; the lower index of a mutual pair
// becomes the new node.
__global__ void __launch_bounds__(PB) k_ploc_apply(PlocArrays a, uint32_t r)
{
    __shared__ uint32_t lds[PB / 64];
    const PlocRound s = a.round[r];
    if (s.c <= PLOC_TAIL || s.error || a.round[r + 1].error) return;
    const uint32_t c = s.c;
    if (blockIdx.x * PB >= c) return;
    const uint32_t i = blockIdx.x * PB + threadIdx.x;
    const uint32_t fl = i < c ? a.flags[i] : 0u;
    uint32_t block_total;
    const uint32_t before = rt_scan::block_exclusive<PB>((fl & 1u) | ((fl >> 1) << 16), lds, block_total);
    if (!(fl & 1u)) return;
    const uint64_t off = a.tally[blockIdx.x];
    const uint32_t pos = (uint32_t)off + (before & 0xFFFFu);
    const uint32_t *cl_node = a.cl_node[s.cur];
    const Box6 *cl_box = a.cl_box[s.cur];
    uint32_t *out_node = a.cl_node[s.cur ^ 1u];
    Box6 *out_box = a.cl_box[s.cur ^ 1u];
    if (fl & 2u) {
        const uint32_t j = a.nn[i];
        const uint32_t m = s.next_node + (uint32_t)(off >> 32) + (before >> 16);
        const uint32_t na = cl_node[i], nb = cl_node[j];
        uint32_t sz;
        const Box6 u = ploc_merge(a.tree, m, na, nb, cl_box[i], cl_box[j], [&] { return a.tree.size[na] + a.tree.size[nb]; }, sz);
        out_node[pos] = m;
        out_box[pos] = u;
    } else {
        out_node[pos] = cl_node[i];
        out_box[pos] = cl_box[i];
    }
}

// The tail of the clustering: once PLOC_TAIL or fewer clusters are left, ONE workgroup runs all the remaining rounds
// (nearest neighbour, mutual-pair flags, the two prefix sums, merge: the steps above) back to back with barriers in between,
// without ~40 rounds of launches and host round trips for a handful of clusters each.  The cluster array (boxes, node ids, sizes) lives in LDS for the whole tail: 2048 x 34 B
// = 68 KiB of the CU's 160; the first version kept it in global memory and spent 0.36 ms of a 2.5 ms build on round trips.
struct TailLds {
    Box6 box[PLOC_TAIL];
    uint32_t node[PLOC_TAIL], size[PLOC_TAIL];
    uint16_t nn[PLOC_TAIL];
    uint32_t scan[TAIL_BLOCK / 64];
};
__global__ void __launch_bounds__(TAIL_BLOCK) k_ploc_tail(PlocArrays a, uint32_t r, PlocRound *__restrict__ result)
{
    const PlocRound s = a.round[r];
    if (s.c > PLOC_TAIL || s.error) {                  // the batch of rounds fell short (or failed): the host decides
        if (threadIdx.x == 0) *result = s;
        return;
    }
    uint32_t c = s.c, next_node = s.next_node;
    const uint32_t cur = s.cur;
    extern __shared__ __align__(16) unsigned char tail_smem[];
    TailLds &L = *reinterpret_cast<TailLds *>(tail_smem);
    constexpr uint32_t PER = PLOC_TAIL / TAIL_BLOCK;
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < c; i += TAIL_BLOCK) {
        const uint32_t id = a.cl_node[cur][i];
        L.box[i] = a.cl_box[cur][i];
        L.node[i] = id;
        L.size[i] = a.tree.size[id];
    }
    __syncthreads();
    while (c > 1) {
        for (uint32_t i = t; i < c; i += TAIL_BLOCK)
            L.nn[i] = (uint16_t)ploc_nearest<PLOC_TAIL_RADIUS>((int)i, (int)c, [&](int j) -> const Box6 & { return L.box[j]; });
        __syncthreads();
        // flags, PER consecutive clusters per thread, kept in registers; tallies packed kept | created << 16
        uint32_t mine = 0, keep_bits = 0, merge_bits = 0;
        for (uint32_t e = 0; e < PER; e++) {
            const uint32_t i = t * PER + e;
            if (i >= c) break;
            const uint32_t j = L.nn[i];
            uint32_t kp, mg;
            ploc_flags(i, j, [&](uint32_t o) -> uint32_t { return L.nn[o]; }, kp, mg);
            merge_bits |= mg << e;
            keep_bits |= kp << e;
            mine += kp | (mg << 16);
        }
        uint32_t total;
        const uint32_t before = rt_scan::block_exclusive<TAIL_BLOCK>(mine, L.scan, total);
        uint32_t k_run = before & 0xFFFFu, m_run = before >> 16;
        const uint32_t kept = total & 0xFFFFu, merged = total >> 16;
        if (merged == 0 || kept != c - merged) break;                 // no progress: reported by the host (block-uniform)
        // what this thread's clusters become, computed into registers before anybody overwrites the array
        Box6 out_box[PER];
        uint32_t out_node[PER], out_size[PER], out_pos[PER];
        for (uint32_t e = 0; e < PER; e++) {
            const uint32_t i = t * PER + e;
            out_pos[e] = 0xFFFFFFFFu;
            if (i >= c || !((keep_bits >> e) & 1u)) continue;
            out_pos[e] = k_run;
            if ((merge_bits >> e) & 1u) {
                const uint32_t j = L.nn[i], m = next_node + m_run;
                out_box[e] = ploc_merge(a.tree, m, L.node[i], L.node[j], L.box[i], L.box[j], [&] { return L.size[i] + L.size[j]; }, out_size[e]);
                out_node[e] = m;
                m_run++;
            } else {
                out_node[e] = L.node[i];
                out_box[e] = L.box[i];
                out_size[e] = L.size[i];
            }
            k_run++;
        }
        __syncthreads();
        for (uint32_t e = 0; e < PER; e++)
            if (out_pos[e] != 0xFFFFFFFFu) { L.box[out_pos[e]] = out_box[e]; L.node[out_pos[e]] = out_node[e]; L.size[out_pos[e]] = out_size[e]; }
        __syncthreads();
        c = kept;
        next_node += merged;
    }
    if (t == 0) { const PlocRound out = {c, next_node, cur, 0u}; *result = out; }
}

// leaf boxes into node_box[0..n-1] so every node id indexes one box array
__global__ void k_ploc_leaf_boxes(const Box6 *__restrict__ cl_box, uint32_t n, Box6 *__restrict__ node_box)
{
    const uint32_t k = blockIdx.x * PB + threadIdx.x;
    if (k < n) node_box[k] = cl_box[k];
}

// depth-first offset of every node = number of leaves before it
__global__ void k_ploc_offsets(BinTree t)
{
    const uint32_t id = blockIdx.x * PB + threadIdx.x, n = t.n;
    if (id >= 2 * n - 1) return;
    uint32_t off = 0, cur = id;
    for (uint32_t p = t.parent[cur]; p != 0xFFFFFFFFu; p = t.parent[cur]) {
        if (t.right[p - n] == cur) off += t.size[t.left[p - n]];
        cur = p;
    }
    t.offset[id] = off;
}

// (leaf_prim != nullptr: leaf k is a reference of primitive leaf_prim[k] with the box leaf_box6[k]; the record of a split triangle's reference
// says so and its box goes to rec_boxes beside it)
__global__ void k_ploc_tris(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ leaf_prim, const float *__restrict__ leaf_box6,
                            const uint32_t *__restrict__ ref_off, const rt_vertex *__restrict__ verts, const uint32_t *__restrict__ idx,
                            const uint32_t *__restrict__ offset, uint32_t n, TriRec *__restrict__ tris, float *__restrict__ rec_boxes)
{
    const uint32_t k = blockIdx.x * PB + threadIdx.x;
    if (k >= n) return;
    const uint32_t prim = leaf_prim ? leaf_prim[k] : (uint32_t)(keys[k] & 0xFFFFFFFFull);
    float p[3][3];
    tri_positions(verts, idx, prim, p);
    const bool split = leaf_prim && ref_off[prim + 1] - ref_off[prim] > 1u;
    tris[offset[k]] = tri_record(p, prim, split ? 1u : 0u);
    if (rec_boxes)
        for (int q = 0; q < 6; q++) rec_boxes[6 * (size_t)offset[k] + q] = leaf_box6[6 * (size_t)k + q];
}

// Every temporary of the build is carved out of ONE allocation, the context's build arena (hipMalloc / hipFree synchronise the
// device and cost more than the kernels of a small build).  The cluster arrays of the rounds, up to `left`, are free once the tree
// stands and serve the collapse into wide nodes as its scratch.
struct PlocTemps {
    PlocArrays pa;
    PlocRound *result;           // where a batch of rounds stopped: the entry behind pa.round's PLOC_MAX_BATCH + 1
    size_t scratch_bytes;        // from pa.cl_node[0]
};
void carve_ploc(Carver &c, uint32_t n, PlocTemps &t)
{
    const size_t nn2 = 2 * (size_t)n - 1, scratch_from = c.offset;
    PlocArrays &pa = t.pa;
    BinTree &tree = pa.tree;
    for (int k = 0; k < 2; k++) pa.cl_node[k] = c.take<uint32_t>(n);
    for (int k = 0; k < 2; k++) pa.cl_box[k] = c.take<Box6>(n);
    pa.nn = c.take<uint32_t>(n);
    pa.flags = c.take<uint32_t>(n);
    pa.tally = c.take<uint64_t>(grid_for(n, PB));
    (void)c.take<char>(64 * (size_t)n);          // (only widens what the collapse uses as its scratch: rt_wide_temp_bytes)
    t.scratch_bytes = c.offset - scratch_from;
    tree.left = c.take<uint32_t>(n - 1); tree.right = c.take<uint32_t>(n - 1);
    tree.box = c.take<Box6>(nn2);
    tree.size = c.take<uint32_t>(nn2); tree.parent = c.take<uint32_t>(nn2); tree.offset = c.take<uint32_t>(nn2);
    tree.leaf_prim = nullptr; tree.n = n;      // (a BLAS)
    pa.round = c.take<PlocRound>(PLOC_MAX_BATCH + 2);
    t.result = pa.round ? pa.round + PLOC_MAX_BATCH + 1 : nullptr;
    pa.arrivals = c.take<uint32_t>(1);
}

}  // namespace

// bytes of temporaries rt_build_ploc_layout slices out of the context's build arena
size_t rt_ploc_temp_bytes(uint32_t n)
{
    Carver sizing(nullptr);
    PlocTemps t;
    carve_ploc(sizing, n, t);
    return sizing.offset;
}

// Rebuilds m->tris and m->blas.wide / root_code / fast_depth from a PLOC tree.  The canonical arrays
// (nodes, keys, parents) are left untouched.  Returns RT_OK with *done = false for meshes too small to bother.
int rt_build_ploc_layout(rt_context *ctx, rt_model *m, bool *done, const PlocLeaves &leaves)
{
    const float *leaf_box6 = leaves.box6;
    const uint32_t n = leaf_box6 ? leaves.n : m->n_tris;          // leaves of the tree: triangles, or the references of a model with split ones
    *done = false;
    if (n < 2 * ctx->leaf_max + 2) return RT_OK;          // tiny meshes: the LBVH layout is as good as any
    hipStream_t st = ctx->stream;
    RT_TRY(ctx->build_arena.reserve(rt_ploc_temp_bytes(n)));      // normally already there (take_build_temps)
    Carver arena(ctx->build_arena.p);
    PlocTemps t;
    carve_ploc(arena, n, t);
    const PlocArrays &pa = t.pa;
    // 68 KiB of dynamic LDS: above the default 64 KiB limit of a launch (the attribute is per device, set every build)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_ploc_tail), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(TailLds)));

    if (leaf_box6) {          // records and their boxes for every reference
        RT_TRY(m->tris.reserve(sizeof(TriRec) * (size_t)n));
        RT_TRY(m->rec_boxes.reserve(24 * (size_t)n));
    }
    k_ploc_init<<<grid_for(n, PB), PB, 0, st>>>(m->blas.nodes.as<rt_bvh_node>(), leaf_box6, n, pa.cl_node[0], pa.cl_box[0], pa.tree.size, pa.tree.parent, pa.round, pa.arrivals);
    k_ploc_leaf_boxes<<<grid_for(n, PB), PB, 0, st>>>(pa.cl_box[0], n, pa.tree.box);
    // Rounds are launched in batches without looking at the cluster count: every launch covers the count the batch
    // started with (workgroups past the live count leave at once), a round past the tail threshold costs two empty
    // launches, and the tail kernel closes the batch.  A round keeps ~0.76 of its clusters on the scenes measured;
    // the estimate below assumes 0.78 and a batch that falls short is simply followed by another.
    PlocRound res = {n, n, 0u, 0u};
    for (int batchno = 0; batchno < 4096; batchno++) {
        uint32_t rounds = 0;
        for (double x = (double)res.c; x > (double)PLOC_TAIL && rounds < PLOC_MAX_BATCH; x *= 0.78) rounds++;
        if (rounds > 0 && rounds < PLOC_MAX_BATCH) rounds++;
        if (ctx->build_batch && rounds > ctx->build_batch) rounds = ctx->build_batch;      // (tests: force short batches)
        for (uint32_t r = 0; r < rounds; r++) {
            k_ploc_pair<<<grid_for(res.c, PB), PB, 0, st>>>(pa, r);
            k_ploc_apply<<<grid_for(res.c, PB), PB, 0, st>>>(pa, r);
        }
        k_ploc_tail<<<1, TAIL_BLOCK, sizeof(TailLds), st>>>(pa, rounds, t.result);
        PlocRound *host = ctx->pinned ? (PlocRound *)ctx->pinned : &res;      // page-locked: no staging copy
        HIP_TRY(hipMemcpyAsync(host, t.result, sizeof(PlocRound), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipGetLastError());
        const uint32_t before = res.c;
        res = *host;
        if (res.error || (res.c > PLOC_TAIL && res.c >= before)) {
            rt_set_error("PLOC made no progress (%u clusters)", res.c);
            return RT_ERR_STATE;
        }
        if (res.c <= PLOC_TAIL) break;
        // short of the tail: the next batch starts from where this one stopped
        HIP_TRY(hipMemcpyAsync(pa.round, t.result, sizeof(PlocRound), hipMemcpyDeviceToDevice, st));
    }
    if (res.c != 1 || res.next_node != 2 * n - 1) {
        rt_set_error("PLOC did not converge (%u clusters, %u nodes)", res.c, res.next_node);
        return RT_ERR_STATE;
    }
    k_ploc_offsets<<<grid_for(2 * (size_t)n - 1, PB), PB, 0, st>>>(pa.tree);
    k_ploc_tris<<<grid_for(n, PB), PB, 0, st>>>(m->blas.keys.as<uint64_t>(), leaves.prim, leaf_box6, leaf_box6 ? m->ref_off.as<uint32_t>() : nullptr,
                                     m->d_verts.as<rt_vertex>(), m->d_idx.as<uint32_t>(), pa.tree.offset, n, m->tris.as<TriRec>(),
                                     leaf_box6 ? m->rec_boxes.as<float>() : nullptr);
    HIP_TRY(hipGetLastError());
    // four-wide nodes from the binary tree (root = the last node created); the cluster arrays of the rounds are free now
    // and serve as its scratch
    RT_TRY(rt_build_wide_layout(ctx, m->blas, pa.tree, 2 * n - 2, ctx->leaf_max, pa.cl_node[0], t.scratch_bytes));
    if (leaf_box6) m->n_recs = n;
    *done = true;
    return RT_OK;
}
