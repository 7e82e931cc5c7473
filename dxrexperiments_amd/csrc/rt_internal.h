// rt_internal.h -- objects behind the opaque C-ABI handles (include/dxr_amd.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/dxr_amd.h"
#include "rt_skeleton.h"                     // RT_SKELETON_POSE_FLOATS: what rt_pose_source holds per joint
#include "rt_ik_groups.h"                    // the group ends of a crowd's chain list

void rt_set_error(const char *fmt, ...);

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            rt_set_error("%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return RT_ERR_HIP;                                                                \
        }                                                                                     \
    } while (0)

#define RT_TRY(expr)              \
    do {                          \
        int r_ = (expr);          \
        if (r_ != RT_OK) return r_; \
    } while (0)

#define RT_REQUIRE(cond, msg)                        \
    do {                                             \
        if (!(cond)) {                               \
            rt_set_error("%s: %s", __func__, msg);   \
            return RT_ERR_INVALID_ARG;               \
        }                                            \
    } while (0)

// Test hook (rt_debug_set_alloc_limit): device allocations above this many bytes fail with RT_ERR_OOM as if the device were
// full, so that the out-of-memory paths can be exercised on a 288 GB part.  Default: no limit.
size_t &rt_alloc_limit_ref();
static inline size_t rt_alloc_limit() { return rt_alloc_limit_ref(); }

// Owning device allocation; grows on demand, never shrinks.  Frees itself when it goes out of scope and moves, never copies: an owner
// lists no buffers to release, and rt_release (below, with rt_handle) selects the device before its members die.  None has static or thread storage
// duration: a hipFree after the runtime has shut down is not acceptable.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    bool borrowed = false;       // p points into somebody else's allocation (adopt): never freed here
    DevBuf() = default;
    ~DevBuf() { release(); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes), borrowed(o.borrowed) { o.p = nullptr; o.bytes = 0; o.borrowed = false; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p; bytes = o.bytes; borrowed = o.borrowed;
            o.p = nullptr; o.bytes = 0; o.borrowed = false;
        }
        return *this;
    }
    // use a slice of another allocation; a later reserve() beyond it falls back to an allocation of its own
    void adopt(void *ptr, size_t n) { release(); p = ptr; bytes = n; borrowed = ptr != nullptr; }
    // Grows to at least n bytes (contents are NOT kept).  The new block is allocated BEFORE the old one is freed, so a
    // growth that fails leaves the buffer as it was; only when old + new do not fit together is the old block given up
    // first -- and then a second failure leaves an EMPTY buffer (p = nullptr, bytes = 0), never a stale pointer.  Callers
    // keep no capacities of their own: what a buffer can hold is `bytes`.
    int reserve(size_t n)
    {
        if (n <= bytes) return RT_OK;
        const size_t want = n ? n : 16;
        void *q = nullptr;
        hipError_t e = want > rt_alloc_limit() ? hipErrorOutOfMemory : hipMalloc(&q, want);
        if (e == hipErrorOutOfMemory && p && !borrowed && want <= rt_alloc_limit()) {
            (void)hipGetLastError();
            (void)hipFree(p);
            p = nullptr; bytes = 0;
            q = nullptr;
            e = hipMalloc(&q, want);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rt_set_error("hipMalloc(%zu): %s", n, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP;
        }
        if (p && !borrowed) (void)hipFree(p);
        p = q; bytes = want; borrowed = false;
        return RT_OK;
    }
    void release()
    {
        if (p && !borrowed) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        borrowed = false;
    }
    template <class T> T *as() const { return (T *)p; }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a DevBuf has one owner");

// An event a function creates and also destroys (an owner's own events are its destructor's business).
struct ScopedEvent {
    hipEvent_t e = nullptr;
    ScopedEvent() = default;
    ScopedEvent(const ScopedEvent &) = delete;
    ScopedEvent &operator=(const ScopedEvent &) = delete;
    ~ScopedEvent() { if (e) (void)hipEventDestroy(e); }
};

// A scalar on its way back from the device that nobody waits for: a page-locked block of 64 bytes and the event that says when a copy into
// it has landed.  Made on first use, both or neither (a creation that failed is tried again by the next call); moves, never copies.  The
// destructor frees both and reads neither: the owner has selected the device and joined the stream before its members die.
struct PinnedReadback {
    void *block = nullptr;
    hipEvent_t event = nullptr;
    bool in_flight = false;      // a copy has been sent and landed() has not said so yet
    PinnedReadback() = default;
    ~PinnedReadback() { release(); }
    PinnedReadback(PinnedReadback &&o) noexcept { *this = std::move(o); }      // (and so no copies)
    PinnedReadback &operator=(PinnedReadback &&o) noexcept
    {
        if (this != &o) {
            release();
            block = o.block; event = o.event; in_flight = o.in_flight;
            o.block = nullptr; o.event = nullptr; o.in_flight = false;
        }
        return *this;
    }
    void release() { if (event) (void)hipEventDestroy(event); if (block) (void)hipHostFree(block); block = nullptr; event = nullptr; in_flight = false; }
    bool ready()
    {
        if (block) return true;
        void *b = nullptr;
        if (hipHostMalloc(&b, 64, hipHostMallocDefault) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&event, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(b); event = nullptr; return false; }
        block = b;
        return true;
    }
    // `bytes` of device memory into the block, behind what the stream holds; true: a copy is in flight
    bool send(const void *src, size_t bytes, hipStream_t st)
    {
        return in_flight = ready() && bytes <= 64 && hipMemcpyAsync(block, src, bytes, hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(event, st) == hipSuccess;
    }
    // true once per flight: the first time the event says that the copy is there (never waits)
    bool landed() { const bool now = in_flight && hipEventQuery(event) == hipSuccess; in_flight = in_flight && !now; return now; }
    template <class T> T read() const { T v; static_assert(sizeof v <= 64, "the block holds 64 bytes"); memcpy(&v, block, sizeof v); return v; }
};

// Slices of one allocation, each 256-byte aligned.  A builder describes its temporaries ONCE, as a function that takes a carver and
// fills a struct of typed pointers; with a null base the same calls only add up the bytes the allocation must hold.
struct Carver {
    char *base = nullptr;
    size_t offset = 0;
    explicit Carver(void *b) : base((char *)b) {}
    template <class T> T *take(size_t count)
    {
        const size_t at = offset;
        offset += (sizeof(T) * count + 255) & ~(size_t)255;
        return base ? (T *)(base + at) : nullptr;
    }
};

// ---- device-visible records -------------------------------------------------

// One traversal node = FOUR children in one 64-B line (fetched as 4 x dwordx4).  Child boxes are quantised to 8 bits per plane
// on a power-of-two grid anchored at the node's own box: plane = fma(q, scale, origin), the builder rounds lo planes down and
// hi planes up WITH THIS SAME EXPRESSION until the decoded box contains the child's true box, so culling against it is
// conservative and the candidate validation of rt_trace_device.h keeps every result bit-identical to the canonical definition.
//   q0 = origin.x origin.y origin.z scale.x
//   q1 = lo.x[4] hi.x[4] lo.y[4] hi.y[4]        (one byte per child, child k in bits 8k..8k+7)
//   q2 = lo.z[4] hi.z[4] scale.y scale.z
//   q3 = code[4]
// Child code: >= 0 index of an internal node of the same array; < 0 leaf: ~code = (first << 3) | (count-1) for a BLAS
// (triangles first..first+count-1 of the sorted triangle array), or the instance index for the TLAS; RT_NODE_NONE for an
// unused slot.  Nodes are numbered breadth first, so the first top_n nodes ARE the top of the tree (LDS resident in the
// traversal kernels).  Children are packed at the front, larger surface first (any-hit rays walk unordered and try the
// likelier occluder first); closest-hit rays sort the hit children by entry distance.  A scale of +inf (with q = 0 planes)
// marks an axis the builder could not quantise: its planes decode to NaN and never cull.
#define RT_WIDE 4                     // children of a node (the eight-wide layout of round 3, measured slower: experiments/r03_wide8.patch)
struct WNode { float4 q0, q1, q2, q3; };
#define RT_NODE_SHIFT 6               // log2(sizeof(WNode))
#define RT_TOP_WORDS 16               // ints of a node kept in LDS: all of it
#define RT_NODE_NONE ((int)0x80000000)

// One triangle in leaf order: the three ORIGINAL vertex positions (so that the
// Moller-Trumbore edges and the triangle's own AABB are recomputed from the same
// floats the canonical BVH was built from) plus the primitive id.  48 B.
struct TriRec { float4 a, b, c; };   // a = v0.xyz v1.x ; b = v1.yz v2.xy ; c = v2.z prim ref 0
                                     // ref (bits of c.z, round 5, rt_refs.h): 0 = the triangle is validated against its own AABB (every triangle of rounds 1 - 4);
                                     //   1 = this record is ONE reference of a split triangle, its box is InstanceRec::rec_boxes[record index];
                                     //   2 = a split triangle in a layout that holds it once (LBVH layout): validated against all its boxes, by primitive
                                     // (padding a record to one 64-B line so that none straddles two: measured, no change)

#define RT_INST_IDENTITY 1u

struct InstanceRec {
    float inv[12];              // world-to-object, 3x4 row-major
    float wlo[3]; int root_code;
    float whi[3]; uint32_t flags;
    const WNode *wide;
    const TriRec *tris;
    const rt_bvh_node *cnodes;  // canonical nodes of the BLAS
    const rt_vertex *verts;
    const uint32_t *indices;
    const TriRec *normals;      // the three vertex normals of primitive p in ONE 48-B record (n0.xyz n1.x | n1.yz n2.xy | n2.z):
                                //   a shaded hit fetches one record instead of three indices and three scattered vertices
    uint32_t n_prims;           // triangles of the model
    uint32_t material;
    // split references (rt_refs.h): nullptr when no triangle of the model is split
    const float *rec_boxes;     // 6 floats per record of `tris` (meaningful where the record says ref = 1)
    const uint32_t *ref_off;    // per primitive: its boxes are ref_boxes[6 * ref_off[p] .. 6 * ref_off[p + 1])
    const float *ref_boxes;
    uint32_t n_recs;            // records of `tris`: n_prims, or more when some triangles are held as several references
    uint32_t pad_;
};

struct SceneDev {
    const InstanceRec *inst;
    const WNode *tlas_wide;
    const rt_bvh_node *tlas_cnodes;
    uint32_t n_inst;
    int tlas_root_code;
    int *deep_stack;             // global stack rows beyond the LDS rows (rt_trace_wave.h); nullptr: never needed
    uint32_t top_n;              // nodes 0..top_n-1 of the structure a ray starts in (single-level: the BLAS, two-level: the
                                 //   TLAS) are copied into LDS by every traversal workgroup
};

#ifndef RT_TOP_NODES
#define RT_TOP_NODES  128             // nodes of the LDS-resident top: 8 KiB per 256-thread block (the size hardly matters: 32 .. 192 nodes all within 1 %)
#endif
#define RT_TOP_ROWS(BLOCK) ((RT_TOP_NODES * RT_TOP_WORDS + (BLOCK) - 1) / (BLOCK))      // LDS rows (of BLOCK ints) the top table takes


// ---- host objects --------------------------------------------------------------

#define RT_PINNED_WORDS 128
#define RT_PINNED_LBVH 64
struct rt_context {
    int refs = 1;                // handle + every object created on it (rt_handle); touched by rt_context_retain / _release only
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_trace_ms = 0.0f;
    uint32_t leaf_max = 2;       // triangles per collapsed leaf in the traversal layout (option leaf_max; 2 measured best: 1 4.05, 2 3.69, 3 3.80, 4 3.87, 8 4.23 ms/frame)
    bool use_ploc = true;        // option fast_bvh=lbvh keeps the canonical LBVH as the traversal layout
    bool wide_sah = false;       // option wide_sah=1: the collapse into wide nodes minimises the surface-area cost (rt_bvh_wide.hip); default: area-greedy
                                 //   (measured, profiles/r03/wide8_experiment.md: no faster on either layout)
    float sah_node = 1.0f, sah_prim = 0.5f;     // cost of one wide-node step / one triangle test (options sah_node, sah_prim)
    uint32_t cu_count = 256;     // compute units of the device
    size_t device_mem_total = 0; // bytes of device memory (asked once, when a pipeline first sizes its queues)
    uint32_t blocks_per_cu_override = 0;    // option persistent_blocks_per_cu: 0 = ask the occupancy API per kernel
    bool lds_top = true;                    // option lds_top=0: every node comes from global memory
    uint32_t lds_stack_rows = 0;            // option lds_stack_rows=6: the small-stack instantiation (tests of the deep-stack path)
    DevBuf pool;                 // ray-pool counters of rt_trace_batch
    DevBuf deep_stack;           // global stack rows of the traversal kernels (rt_scene_dev_for_launch)
    uint32_t build_batch = 0;    // test hook (option build_batch): PLOC rounds / collapse levels launched between two looks at the
                                 //   device-side state; 0 = the builders' own estimates
    uint32_t *pinned = nullptr;  // RT_PINNED_WORDS of page-locked host memory: small device-to-host read-backs without staging
                                 // (words 0..63: whoever synchronises next; RT_PINNED_LBVH..+6: depth and bounds of an LBVH in flight)
    DevBuf build_arena;          // temporaries of the acceleration-structure builds: one allocation, sliced (hipMalloc
                                 // and hipFree synchronise the device and cost more than the kernels of a small build)
    DevBuf scratch[8];           // staging for host-pointer batch calls
    // Experiment / test knobs (rt_debug_set_option, include/dxr_amd.h; the one environment variable RT_DEBUG_OPTIONS="name=value,..." is
    // applied once, when the context is created).  Nothing else in the library reads the environment for its behaviour.
    bool verbose = false;                   // verbose=1: build phases and structure depths on stderr
    int opt_shadow_cache_res = -1;          // shadow_cache_res: cells per side for pipelines that have not been told (-1: by triangle count, 0: off)
    int opt_shadow_cache_pixels = -1;       // shadow_cache_pixels: per-pixel entries (-1: two-level scenes only)
    int opt_primary_persistent = -1;        // primary_persistent: the primary stage as a persistent launch (-1: two-level scenes only)
    bool opt_seven_waves_always = false;    // seven_waves_always=1: single frames on the sets' kernels
    bool opt_free_radius = true;            // free_radius=0: no free sphere around the point light
    uint32_t opt_batch_max = 0;             // batch_max: frames per set of launches (0: RT_MAX_BATCH)
    bool opt_fail_ploc_rounds = false;      // fail_ploc_rounds=1 (tests): the PLOC layout is thrown away as if its rounds had made no progress (non-finite boxes): the LBVH fallback
    bool opt_split_refs = true;             // split_refs=0: no triangle is held as several references (the builder of rounds 1 - 4; the CANDIDATE RULE still
                                            //   follows rt_refs.h -- results do not depend on this option)
    uint32_t opt_primary_retry_cap = 0;     // primary_retry_cap: entries of the primary launch's retry list (0: 2^20; tests: a few, so that the list overflows)
    int opt_primary_entries = -1;           // primary_entries: primary rays start from per-tile entry lists (-1: sets of 4 frames or more of single-level scenes with an LDS top whose primary launch is not persistent)
    uint32_t opt_primary_entries_cut = 0;   // primary_entries_cut: the lists cut the tree below its first n nodes (0: RT_TOP_NODES)
    uint32_t opt_primary_entries_cap = 0;   // primary_entries_cap: entries a list may hold before it falls back to a coarser cut (0: RT_ENTRY_CAP; tests: 1)
    size_t opt_queue_budget_mb = 0;         // queue_budget_mb: worst-case queue bytes a set may reserve up front (0: a quarter of the device)
    double opt_dist_check_seconds = 5.0;    // dist_check_seconds: how long rt_dist_create waits for the other ranks' device ids
    std::vector<struct rt_pipeline *> deferred;      // pipelines holding frames that render() has accepted and not rendered yet
                                 //   (rt_pipeline_set_deferred): whatever changes what those frames would see flushes them first
    ~rt_context();               // (rt_api.hip) selects the device and joins the stream; pinned memory, events, an owned stream; then the buffers
};

static inline int rt_use_device(const rt_context *ctx) { HIP_TRY(hipSetDevice(ctx->device)); return RT_OK; }

// The context lives until its handle AND every object created on it are gone.
static inline void rt_context_retain(rt_context *ctx) { if (ctx) ctx->refs++; }
static inline void rt_context_release(rt_context *ctx) { if (ctx && --ctx->refs == 0) delete ctx; }

// What every host object but the context is: made on a context, which it retains until its OWN members are gone (a base's destructor runs
// after the derived members'), and counted: its handle + whoever rt_retain()s it.  A type says with `joins_stream` whether its last
// release waits for the context's stream (queued work may still read its buffers) before the object dies.
struct rt_handle {
    rt_context *const ctx;
    int refs = 1;
    explicit rt_handle(rt_context *c) : ctx(c) { rt_context_retain(c); }
    rt_handle(const rt_handle &) = delete;
    rt_handle &operator=(const rt_handle &) = delete;
protected:
    ~rt_handle() { rt_context_release(ctx); }
};

template <class T> void rt_retain(T *x) { x->refs++; }
// every *_destroy, and the one way out of a *_create that fails: the last reference selects the device, joins, deletes
template <class T> int rt_release(T *x)
{
    if (!x || --x->refs > 0) return RT_OK;
    (void)hipSetDevice(x->ctx->device);
    if (T::joins_stream) (void)hipStreamSynchronize(x->ctx->stream);
    delete x;
    return RT_OK;
}
// an object between `new` and `*out = x.release()`
struct rt_releaser { template <class T> void operator()(T *x) const { (void)rt_release(x); } };
template <class T> using rt_made = std::unique_ptr<T, rt_releaser>;
template <class T> int rt_make(rt_context *ctx, rt_made<T> &x)
{
    x.reset(new (std::nothrow) T(ctx));
    if (!x) { rt_set_error("out of host memory"); return RT_ERR_OOM; }
    return RT_OK;
}
// `bytes` of a host array into a buffer grown to hold them, queued on the context's stream
static inline int rt_upload(rt_context *ctx, DevBuf &b, const void *host, size_t bytes)
{
    RT_TRY(b.reserve(bytes));
    if (bytes) HIP_TRY(hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return RT_OK;
}

struct BvhDev {
    uint32_t n = 0;              // primitives
    uint32_t max_depth = 0;
    float bounds[6] = {0, 0, 0, 0, 0, 0};
    DevBuf nodes;                // rt_bvh_node[2n-1]   canonical
    DevBuf keys;                 // uint64[n]           sorted morton keys
    DevBuf parents;              // uint32[2n-1]
    DevBuf ranges;               // uint2[n-1]          leaf range of every internal node
    DevBuf wide;                 // WNode[wide_n]       traversal layout, breadth first
    uint32_t wide_n = 0;
    int root_code = -1;
    uint32_t fast_depth = 0;     // stack entries the traversal layout can need
};

// rt_model_set_skin / rt_model_set_bones: k == 0: no skin.  (An empty one assigned over it frees every buffer: nothing lists them.)
struct ModelSkin {
    uint32_t k = 0, bones = 0;   // influences per vertex, bones of a palette
    DevBuf bone, weight;         // uint16[k][n_verts], float[k][n_verts]: slot major (rt_skin.h)
    DevBuf rest;                 // rt_vertex[n_verts]: the rest pose, d_verts as they were when the skin was set
};

// rt_model_set_morph_targets / rt_model_set_morph_weights: targets == 0: no targets
struct ModelMorph {
    uint32_t targets = 0, entries = 0;
    bool normals = false;        // the targets carry normal deltas (dnrm is filled)
    DevBuf count, slice;         // uint32[n_verts], uint32[ceil(n_verts / 64) + 1]: SELL-64 (rt_morph.h)
    DevBuf target, dpos, dnrm;   // uint16[cells], float[3 cells], float[3 cells]
    DevBuf base;                 // rt_vertex[n_verts]: the base, captured when the targets were set
};

struct rt_model : rt_handle {
    using rt_handle::rt_handle;  // refs: handle + rt_model_retain + every instance of a scene
    static constexpr bool joins_stream = false;
    uint32_t n_verts = 0, n_tris = 0;
    std::vector<rt_vertex> h_verts;
    std::vector<uint32_t> h_idx;
    DevBuf d_verts, d_idx;
    DevBuf tris;                 // TriRec[n_recs] in sorted order
    DevBuf normals;              // TriRec[n_tris] in primitive order: the vertex normals (InstanceRec::normals)
    uint32_t n_recs = 0;         // records of `tris`: n_tris, or more when long thin triangles are held as several references (rt_refs.h)
    DevBuf rec_boxes;            // float[6 n_recs]: the reference box of every record (split models only)
    DevBuf ref_off, ref_boxes;   // uint32[n_tris + 1], float[6 refs]: the same boxes by primitive (canonical walk, LBVH layout)
    BvhDev blas;
    bool built = false;
    // rt_model_set_vertices / _set_positions / _recompute_normals: a mesh that changes shape (never its counts or its index list)
    uint64_t geom_gen = 0;       // bumped by every successful set: a scene records it per instance at build / update (SceneInstance::seen_geom)
    bool h_verts_stale = false;  // d_verts was written from device memory: rt_model_read_geometry downloads before it answers
    std::vector<struct rt_scene *> scenes;   // the scenes that hold the model in some instance (each once): a set leaves the built ones stale
    DevBuf adj_off, adj_tris;    // vertex -> triangle CSR of the index list (rt_adjacency.h), made by the first rt_model_recompute_normals
    bool adj_ready = false;
    ModelSkin skin;
    ModelMorph morph;
};

// rt_skeleton_create (rt_skeleton.hip): a joint hierarchy, its current pose and the palette a skin reads
struct SkeletonClip {
    std::vector<float> times;    // n_keys, ascending strictly
    DevBuf d_times;              // ... and their copy on the device, which the slots of a crowd's layout name (k_crowd_pose searches it)
    DevBuf keys;                 // float[n_keys][10][n_joints]: component major within a key, so that the lanes of a wave read 64 consecutive floats
};

// What an attached instance follows, and what a skeleton and a crowd both are: n_poses poses of n_joints joints whose world matrices W stand
// in `joints`, pose after pose, beside the local poses they came from and the palettes made of them.  A scene holds, retains and releases
// its pose sources through this type alone (rt_scene::sources), so the pending rule, the refusals and the lifetime of attachments are
// written once for both; the destructor is virtual for that release.  What a skeleton and a crowd do alike with these members is written
// once too (below: rt_skeleton.hip), and this is the one place that knows what either is called and how it comes by a pose.
struct rt_pose_source : rt_handle {
    using rt_handle::rt_handle;  // refs: handle + every scene that has instances attached to it (once per scene) (+ a skeleton: every crowd made of it)
    static constexpr bool joins_stream = true;       // a skin kernel that reads the palette, or a pose kernel, may still be queued
    uint64_t pose_count = 0;     // bumped by every posing call: a scene records it per attached instance at build / update (SceneInstance::seen_pose)
    uint32_t n_joints = 0;
    uint32_t n_poses = 1;        // a skeleton: 1; a crowd: its actors
    DevBuf pose;                 // float[n_poses][n_joints][10]: the local pose last set, sampled or blended
    DevBuf joints;               // float[n_poses][n_joints][12]: W_j
    DevBuf palette;              // float[n_poses][n_joints][12]: M_j = W_j o inverse_bind_j, what rt_model_set_bones_from_skeleton / _from_crowd hand to the skin kernel
    bool posed = false;          // a pose has been set or sampled: joints (and the palette) hold something
    bool is_crowd = false;       // the object is an rt_crowd, else an rt_skeleton
    float *pose_of(uint32_t i) const { return pose.as<float>() + RT_SKELETON_POSE_FLOATS * (size_t)n_joints * i; }
    const float *w_of(uint32_t i) const { return joints.as<float>() + 12u * (size_t)n_joints * i; }
    const float *palette_of(uint32_t i) const { return palette.as<float>() + 12u * (size_t)n_joints * i; }
    void queued() { posed = true; pose_count++; }     // a posing launch has been queued: one count per call, whatever n_poses
    const char *noun() const { return is_crowd ? "crowd" : "skeleton"; }
    // ... and how "the <noun> has no pose yet (<hint>)" ends
    const char *pose_hint() const { return is_crowd ? "rt_crowd_set_poses or rt_crowd_set_times gives it one" : "rt_skeleton_set_pose or rt_skeleton_set_time gives it one"; }
    virtual ~rt_pose_source() = default;
};

struct rt_skeleton : rt_pose_source {
    using rt_pose_source::rt_pose_source;
    uint32_t n_levels = 0;
    std::vector<uint32_t> level_offsets;     // n_levels + 1 (rt_skeleton.h)
    std::vector<int32_t> parents;            // n_joints, as rt_skeleton_create took them: rt_skeleton_solve_ik finds a constraint's chain and checks independence with them
    DevBuf table;                // uint32[n_joints]: joint | parent << 16 in level order (rt_skeleton_pack_table)
    DevBuf d_level_offsets;      // uint32[n_levels + 1]
    DevBuf inverse_bind;         // float[n_joints][12]
    std::vector<SkeletonClip> clips;
    std::vector<DevBuf> masks;   // rt_skeleton_add_mask: float[n_joints] each, one weight per joint of a blend layer (rt_skeleton_set_blend)
    uint64_t clip_gen = 0, mask_gen = 0;     // bumped by rt_skeleton_clear_clips / _clear_masks when they free something: a crowd's layout holds device addresses of clips and masks and records both (adding keeps every address, and bumps nothing)
};

// rt_crowd_create (rt_crowd.hip): n_poses = n_actors poses of one skeleton, which it retains and whose hierarchy, inverse binds, clips and
// masks it reads where they live.  Every posing call is one upload of the actors' layer records and one launch of k_crowd_pose, or
// (rt_crowd_set_blend_device) the launch alone, over the slots of a layout uploaded once.  rt_crowd_solve_ik (rt_crowd_ik.hip) is one
// launch of k_crowd_ik over the chains the crowd holds, after one upload of the actors' values where they are the host's.
struct CrowdStage {              // one slot of page-locked staging for that upload, and the event behind the copy out of it
    void *block = nullptr;
    size_t bytes = 0;
    hipEvent_t event = nullptr;
    bool in_flight = false;
};
struct rt_crowd : rt_pose_source {
    using rt_pose_source::rt_pose_source;
    rt_skeleton *sk = nullptr;   // retained
    DevBuf layers;               // rt_blend_layer[n_actors][n_layers] of the call last queued (rt_skeleton.h)
    CrowdStage stage[2];         // written in turn: a slot is the host's again once its own event has passed (rt_crowd.hip: crowd_stage)
    uint32_t next_stage = 0;
    DevBuf slots;                // rt_crowd_slot[n_actors][layout_layers] of rt_crowd_set_layout (rt_crowd.h)
    uint32_t layout_layers = 0;  // 0: no layout
    uint64_t layout_clip_gen = 0, layout_mask_gen = 0;   // the skeleton's generations when the layout was packed: it is stale once either has moved
    IkTable ik_chains = {};      // rt_crowd_set_ik_chains: the one list every actor solves, packed (rt_skeleton_pack_ik); it travels by value to k_crowd_ik
    uint32_t n_ik_chains = 0;    // 0: no chains
    uint64_t ik_group_ends = 0;  // rt_crowd_set_ik_chain_groups: where the ordered groups of that list end (rt_ik_group_ends, rt_ik_groups.h); rt_crowd_set_ik_chains: one group
    uint32_t n_ik_groups = 0;    // 0: no chains; 1: rt_crowd_solve_ik launches k_crowd_ik; more: k_ik_groups (rt_ik_groups.hip)
    DevBuf ik_values;            // rt_crowd_solve_ik(RT_MEM_HOST): the targets, poles and weights of the call last queued, one behind another (rt_crowd_ik.h)
    ~rt_crowd() override;        // (rt_crowd.hip) the staging, then the skeleton; the caller has selected the device and joined the stream
};

// Where an instance's transform comes from.  Host: SceneInstance::xform is the truth.  Device: set from device memory, rt_scene::d_xf holds it and
// xform is older until an update's join or a build's.  Joint: attached, every update or build that lists it composes it from its skeleton's W
enum class XfSource : uint8_t { Host, Device, Joint };

// THE host-side statement about one instance; what the device reads of it stands in rt_scene's contiguous arrays, one entry per instance
struct SceneInstance {
    rt_model *model = nullptr;   // retained by the scene
    float xform[12];
    uint8_t mask = 0xFF;         // the InstanceMask byte, as given (0xFF from rt_scene_add_model): visible iff non-zero
    bool pending = false;        // listed in rt_scene::pending
    XfSource source = XfSource::Host;
    uint64_t seen_geom = 0;      // its model's geom_gen when its record was last written (build / update); another value now: the model's
                                 //   vertices changed since, the scene is STALE as with a pending transform
    rt_pose_source *src = nullptr;       // source == Joint: the skeleton or crowd, retained by the scene once (rt_scene::sources); else nullptr
    uint32_t actor = 0;          // ... and which of its poses: a crowd's actor, 0 for a skeleton
    uint64_t seen_pose = 0;      // src->pose_count when the scene last applied a pose to this instance (0: never)
};

// The records and the binding mirrors (inst, att_words, att_local) have exactly inst.size() entries at every entry point: rt_scene_add_model
// lengthens them together and nothing else does.  h_inst and h_blas_bounds are a build's output, one entry per instance of an updatable scene;
// the device arrays are sized for all instances at once (rt_scene.hip).
struct rt_scene : rt_handle {
    using rt_handle::rt_handle;  // refs: handle + every pipeline it is set on
    static constexpr bool joins_stream = false;
    std::vector<SceneInstance> inst;
    std::vector<InstanceRec> h_inst;
    DevBuf d_inst;
    BvhDev tlas;
    bool built = false;
    uint32_t generation = 0;     // bumped by every add_model / build / update: device pointers cached from an older one are stale
    float build_ms = 0.0f;
    uint32_t stack_need = 0;     // traversal stack entries a ray can hold at once
    bool two_level = true;       // false: one identity instance, rays walk its BLAS directly
    bool has_refs = false;       // some model of the scene holds triangles as several references (rt_refs.h)
    // rt_scene_set_instance_transform(s) / rt_scene_update: rigid animation without a rebuild of the instance list
    bool updatable = false;      // the TLAS stands for THIS instance list (built, and no rt_scene_add_model since): an update can apply transforms
    std::vector<uint32_t> pending;       // instances whose transform a setter has changed since the last build / update (each once:
                                         //   SceneInstance::pending); while there are any the scene is STALE: built == false, nothing traces or reads it
    std::vector<float> h_blas_bounds;    // float[6 n]: the BLAS box of every instance's model, as uploaded to ...
    DevBuf blas_bounds;          // ... the box an instance set (back) to the identity takes (written by every build)
    DevBuf update_back;          // the first 20 words (inv, world box, flags) of the records rt_update_tlas rewrote, on their way to h_inst
    float update_ms = 0.0f;
    // rt_scene_set_instance_mask(s): every ray carries the reference's inclusion mask 0xFF, so an instance is VISIBLE iff its mask byte is
    // non-zero.  Masks never touch a record: the TLAS is the one of the visible sub-list, whose leaves name the instances' own indices
    bool masks_dirty = false;            // a setter has changed some instance's visibility on an updatable scene: STALE, as with a pending transform
    std::vector<uint32_t> vis;           // the visible instances, ascending, as the TLAS stands for them (written by a build / update)
    DevBuf d_vis;                        // ... on the device: uploaded only by a build or update at which some visibility changed
    uint32_t n_vis = 0;                  // how many; == inst.size(): nothing hidden, d_vis is not read and the builders launch what they always did
    // rt_scene_set_instance_transforms_mem(RT_MEM_DEVICE) / rt_scene_attach_instances: transforms that come from device memory
    DevBuf d_xf;                         // float[12 n]: the transform of every instance whose source is Device or Joint (the latter: as last composed)
    DevBuf xf_back;                      // the device-sourced transforms an update listed, slot by slot, on their way to SceneInstance::xform
    std::vector<uint32_t> att_words;     // per instance: the binding as the device reads it (rt_attach.h), 0: not attached ...
    std::vector<float> att_local;        // ... its local matrix, float[12] per instance ...
    DevBuf d_att_words, d_att_local, d_att_w;    // ... and both on the device, with the W array (const float *: its skeleton's, or its actor's slice of its crowd's) of every attached instance
    std::vector<rt_pose_source *> sources;       // the skeletons and crowds the scene retains: every one some instance is or was attached to, each once
    SceneDev dev() const
    {
        SceneDev s;
        s.inst = d_inst.as<InstanceRec>();
        s.tlas_wide = tlas.wide.as<WNode>();
        s.tlas_cnodes = tlas.nodes.as<rt_bvh_node>();
        s.n_inst = (uint32_t)inst.size();
        s.tlas_root_code = tlas.root_code;
        s.deep_stack = nullptr;
        s.top_n = 0;
        return s;
    }
    ~rt_scene();                 // (rt_scene.hip) lets go of the models and pose sources it retains; then the buffers
};

// ---- internal entry points shared between translation units ---------------------

// rt_bvh_build.hip
int rt_build_blas(rt_context *ctx, rt_model *m);

// rt_scene.hip
// new vertices of one of the scene's models have been queued (rt_model.hip): a fresh scene is stale until its update or build applies them
void rt_scene_model_changed(rt_scene *s);
// RT_OK for a built scene.  Otherwise RT_ERR_STATE and its message: what is pending -- transforms, instance masks, models' vertices -- or, if
// nothing is, `not_built`, a format that may name `who` once
int rt_scene_require_built(const rt_scene *s, const char *who, const char *not_built);

// rt_skeleton.hip: what a skeleton and a crowd do alike with the record they share
// RT_OK for a source that has a pose; else RT_ERR_STATE and "<who>: the <noun> has no pose yet (<hint>)"
int rt_pose_require(const rt_pose_source *src, const char *who);
// the refusal behind code `what` of rt_skeleton_validate_layers (rt_skeleton_layers_refusal, rt_skeleton.h, with the source's noun and hint) as the last error; its class
int rt_pose_refuse_layers(const rt_pose_source *src, const char *who, int what, const uint32_t *actor, uint32_t bad, const rt_skeleton_layer *l, uint32_t n_layers,
                          uint32_t n_clips, uint32_t n_masks);
// `count` poses from `first` on out of `from` (pose, joints or palette: floats_per_joint 10 or 12), joined.  A skeleton asks for (0, 1)
int rt_pose_read_back(rt_pose_source *src, const char *who, const DevBuf &from, size_t floats_per_joint, uint32_t first, uint32_t count, float *to);
// the refusal behind code `what` of rt_skeleton_validate_ik (rt_skeleton_ik_refusal, rt_skeleton.h, with the source's joints, noun and hint) as the last error; its class
int rt_pose_refuse_ik(const rt_pose_source *src, const char *who, int what, uint32_t n, const rt_skeleton_ik *constraints, const uint32_t bad[3]);
// the caller's n_poses local poses (`mem`: RT_MEM_HOST or RT_MEM_DEVICE, else the refusal under `who`) queued into src->pose; the type's own
// launch follows, and then the join that makes a host array the caller's own again
int rt_pose_copy_in(rt_pose_source *src, const char *who, const float *trs, uint32_t mem);
static inline int rt_pose_join_host(rt_pose_source *src, uint32_t mem) { if (mem == RT_MEM_HOST) HIP_TRY(hipStreamSynchronize(src->ctx->stream)); return RT_OK; }
// pose `actor`'s palette handed to the model's skin (rt_model_set_bones, RT_MEM_DEVICE), or the refusal under `who`
int rt_pose_set_bones(rt_model *m, rt_pose_source *src, uint32_t actor, const char *who);
// the device address of `which` (joints or palette) of a source that has a pose
int rt_pose_device_ptr(const rt_pose_source *src, const char *who, const DevBuf &which, void **ptr);
// rt_crowd.hip: the crowd's next staging slot, the host's to write `bytes` into (what every upload of a crowd call goes through: rt_crowd.hip, rt_crowd_ik.hip)
int crowd_stage(rt_crowd *c, size_t bytes, CrowdStage **out);
// rt_ik_groups.hip: the ONE launch of k_ik_groups over the grouped list a crowd holds, every actor's values in device memory (what rt_crowd_solve_ik ends in when the list has more than one group)
int rt_ik_groups_solve_crowd(rt_crowd *c, const float *targets, const float *poles, const float *weights);

// rt_bvh_ploc.hip.  The leaves PLOC clusters, in Morton order.  Empty: the canonical leaves, one per triangle; otherwise the references of a
// model with split triangles (rt_refs.h): their count, 6 floats and a primitive id per leaf
struct PlocLeaves {
    uint32_t n = 0;
    const float *box6 = nullptr;
    const uint32_t *prim = nullptr;
};
size_t rt_ploc_temp_bytes(uint32_t n);
int rt_build_ploc_layout(rt_context *ctx, rt_model *m, bool *done, const PlocLeaves &leaves);

// rt_bvh_wide.hip: collapses a binary tree (BinTree, rt_bvh_tree.h: the numbering is stated there) into the four-wide traversal layout
// (bv.wide, wide_n, fast_depth, root_code); subtrees of at most leaf_max leaves become leaves (a TLAS: 1).  Temporaries come from the arena
// slice [scratch, scratch + scratch_bytes), or from an allocation of the collapse's own if that is too small.
struct BinTree;
size_t rt_wide_temp_bytes(uint32_t n);
size_t rt_wide_lbvh_temp_bytes(uint32_t n);
int rt_build_wide_layout(rt_context *ctx, BvhDev &bv, const BinTree &tree, uint32_t root, uint32_t leaf_max, void *scratch, size_t scratch_bytes);
// the same from the canonical LBVH arrays of bv (TLAS, tiny meshes, option fast_bvh=lbvh)
int rt_build_wide_from_lbvh(rt_context *ctx, BvhDev &bv, bool tlas, uint32_t leaf_max);

// rt_trace.hip
struct TraceOut {
    float *t, *u, *v;
    uint32_t *prim, *inst, *cnt_nodes, *cnt_tris;
};
int rt_launch_trace(rt_context *ctx, const rt_scene *s, const float4 *origin_tmin, const float4 *dir_tmax, size_t n,
                    uint32_t ray_flags, uint32_t kernel, const TraceOut &out);

// Grid of a persistent traversal kernel: exactly the blocks that are resident at once (the static
// chunk interleaving gives every launched wave its share of the queue, so a block that has to wait
// for a slot would run its share as a serial tail).
#define RT_RESIDENT_BLOCKS_PER_CU 8
template <class K>
static inline unsigned rt_persistent_grid(const rt_context *ctx, K kernel, int block, size_t rays)
{
    int per_cu = (int)ctx->blocks_per_cu_override;
    if (per_cu <= 0 && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess) per_cu = 4;
    if (per_cu < 1) per_cu = 1;
    // the global stack rows behind the LDS ones are sized for RT_RESIDENT_BLOCKS_PER_CU 256-thread workgroups per CU (or the option's count, if larger:
    // scene_for_set): a launch may not have more threads than that, whatever the occupancy query says for a kernel with little LDS
    const int row_cap = ((int)ctx->blocks_per_cu_override > RT_RESIDENT_BLOCKS_PER_CU ? (int)ctx->blocks_per_cu_override : RT_RESIDENT_BLOCKS_PER_CU) * 256 / block;
    if (per_cu > row_cap) per_cu = row_cap;
    const size_t want = (rays + (size_t)block - 1) / (size_t)block;
    const size_t cap = (size_t)ctx->cu_count * (size_t)per_cu;
    return (unsigned)(want < cap ? (want ? want : 1) : cap);
}

#ifndef RT_LDS_STACK_ROWS
#define RT_LDS_STACK_ROWS 18            // LDS stack rows of the traversal kernels; with the 8-row top table (top of the BLAS for
#endif                                  // single-level walks, top of the TLAS for two-level ones) 26 KiB per 256-thread block = 6 blocks per CU.
                                        // Bench-scene rays: 98.1 % never hold more than 8 entries, 99.97 % not more than 12, none more than 17.
// The traversal kernels' STACK template argument is the number of LDS stack rows, + RT_STACK_REFS for the instantiations that walk scenes
// with split references (rt_refs.h; trace_wave's REFS): one argument, so that every launch site picks both at once
#define RT_STACK_REFS 100
#define RT_ROWS(S) ((S) % RT_STACK_REFS)
#define RT_REFS(S) ((S) >= RT_STACK_REFS)
#define RT_LDS_STACK_ROWS_TEST 6        // second instantiation (option lds_stack_rows=6): tests force rays onto the global rows
// Sets of frames (rt_pipeline_render_batch) run long launches whose ramp and drain no longer matter, and there a seventh wave
// per SIMD pays (-3.5 % on the bench scene; frame by frame it costs 2 %, the drain grows with the resident waves:
// profiles/r03/seven_waves.txt): their single-level kernels keep 14 stack rows in LDS (22 KiB per block = 7 blocks per CU) and
// are compiled for seven waves (72 VGPRs; the 74 - 78 of the 18-row kernels shed two to six into scratch, off the step).
#ifndef RT_LDS_STACK_ROWS_SETS
#define RT_LDS_STACK_ROWS_SETS 14
#endif

// The scene as the traversal kernels see it, with the global stack rows a PERSISTENT launch of `threads` threads whose
// kernels keep `lds_rows` rows in LDS may need: the tree bounds a walk to stack_need (+1 speculative) entries.  (Round 5: the only launch
// that is not persistent, the one-tile-per-wave primary stage -- one thread per pixel slot: 224 MB of rows per 1080p frame of a set in
// rounds 1 - 4 -- keeps none: rt_trace_wave.h NO_DEEP.)
static inline int rt_scene_dev_for_launch(rt_context *ctx, const rt_scene *s, uint32_t lds_rows, size_t threads, SceneDev *out)
{
    *out = s->dev();
    if (ctx->lds_top) {          // one identity instance: rays walk its BLAS directly; otherwise the top of the TLAS
        const BvhDev &bv = s->two_level ? s->tlas : s->inst[0].model->blas;
        out->top_n = bv.wide_n < RT_TOP_NODES ? bv.wide_n : RT_TOP_NODES;
    }
    const uint32_t bound = s->stack_need + 2;
    if (bound <= lds_rows) return RT_OK;
    RT_TRY(ctx->deep_stack.reserve((size_t)(bound - lds_rows) * threads * sizeof(int)));
    out->deep_stack = ctx->deep_stack.as<int>();
    return RT_OK;
}
static inline uint32_t rt_lds_stack_rows(const rt_context *ctx)
{
    return ctx->lds_stack_rows == RT_LDS_STACK_ROWS_TEST ? RT_LDS_STACK_ROWS_TEST : RT_LDS_STACK_ROWS;
}

// rt_pipeline_render.hip: renders the frames every deferred pipeline of the context still holds (rt_pipeline_set_deferred)
int rt_context_flush_deferred(rt_context *ctx);

// rt_obj.cpp, rt_fbx.cpp
int rt_obj_parse(const char *path, std::vector<rt_vertex> &verts, std::vector<uint32_t> &idx);
int rt_fbx_parse(const char *path, std::vector<rt_vertex> &verts, std::vector<uint32_t> &idx);
