// rt_pipeline_inspect.hip -- the calls that look at a pipeline without rendering: the two counting passes over the queues the last
// frame left behind (rt_pipeline_count_work: every ray again in canonical order; rt_pipeline_count_walk: the production walk with
// tallies), the read-backs of its primary hits and of a secondary ray, and the cube-map sampler on its own.  Entry points, launches
// and kernels in one place; the sources the kernels read through are the frame's own (rt_pipeline_rays.h).
#include "rt_pipeline_rays.h"

namespace {

// ---- walk counting (rt_pipeline_count_walk): the production walk over the last frame's queues with per-lane
// tallies of what it fetches; results are not stored (the frame already holds them)
template <bool TWO_LEVEL>
__global__ void __launch_bounds__(PBLOCK) k_walk_primary(PipeDev pd, unsigned long long *walk)
{
    __shared__ int smem[walk_lds_words(RT_LDS_STACK_ROWS)];
    PrimarySrc src = {pd};
    NullSink sink;
    trace_wave<RT_LDS_STACK_ROWS, PBLOCK, TWO_LEVEL, 64u, false, true, false, true>(pd.sc, src, sink, nullptr, smem, nullptr, walk);
}
// (... of a primary stage that started from entry lists: the same lists, the same walk.  As k_walk_primary does for the walk from the root, it
// keeps rows beyond LDS and walks a deep ray on from where it stands, where the timed launch hands it to k_primary_retry, which starts at the
// root again: on a tree deeper than the LDS rows the tally leaves out the retried rays' second walk, with lists as without)
template <bool BATCH>
__global__ void __launch_bounds__(PBLOCK) k_walk_primary_from_entries(PipeDev pd, const uint2 *__restrict__ entries, uint32_t frames_magic, uint32_t tiles_x_magic, unsigned long long *walk)
{
    __shared__ int smem[walk_lds_words(RT_LDS_STACK_ROWS, true)];
    PrimaryEntrySrcT<BATCH> src = {{pd}, entries, frames_magic, tiles_x_magic};
    NullSink sink;
    trace_wave<RT_LDS_STACK_ROWS, PBLOCK, false, 64u, false, true, false, true>(pd.sc, src, sink, nullptr, smem, nullptr, walk);
}
template <bool TWO_LEVEL>
__global__ void __launch_bounds__(PBLOCK) k_walk_queue(SceneDev sc, QueueSrc src, unsigned long long *walk)
{
    __shared__ int smem[walk_lds_words(RT_LDS_STACK_ROWS)];
    NullSink sink;
    trace_wave<RT_LDS_STACK_ROWS, PBLOCK, TWO_LEVEL, RT_POOL_CHUNK, false, true, false, true>(sc, src, sink, nullptr, smem, nullptr, walk);
}
template <bool TWO_LEVEL>
__global__ void __launch_bounds__(PBLOCK) k_walk_shadow(SceneDev sc, ShadowQueue queue, unsigned long long *walk)
{
    __shared__ int smem[walk_lds_words(RT_LDS_STACK_ROWS)];
    ShadowSrcN<true> src;
    static_cast<ShadowQueue &>(src) = queue;
    NullSink sink;
    trace_wave<RT_LDS_STACK_ROWS, PBLOCK, TWO_LEVEL, RT_POOL_CHUNK, true, true, false, true>(sc, src, sink, nullptr, smem, nullptr, walk);
}

// every lane of the wave must call this (no early exits before it)
RT_DEV void wave_add64(unsigned long long v, unsigned long long *counter)
{
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
    if ((threadIdx.x & 63u) == 0u && v) atomicAdd(counter, v);
}

// canonical-order re-trace of a queue: sums rays / nodes / triangles into out[0..2]
template <class Src>
__global__ void __launch_bounds__(PBLOCK)
k_count_queue(SceneDev sc, Src src, unsigned long long *__restrict__ out)
{
    const uint32_t idx = blockIdx.x * PBLOCK + threadIdx.x;
    unsigned long long rays = 0, nodes = 0, tris = 0;
    if (idx < src.count()) {
        RayD r;
        uint32_t ticket;
        if (load_ray_of(src, idx, r, ticket, 0)) {
            uint32_t cn, ct;
            (void)trace_canonical(sc, r, src.flags(), cn, ct);
            rays = 1; nodes = cn; tris = ct;
        }
    }
    wave_add64(rays, &out[0]);
    wave_add64(nodes, &out[1]);
    wave_add64(tris, &out[2]);
}

__global__ void k_debug_cube(PipeDev pd, const float *__restrict__ dirs, float *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3 c = sample_cube(pd, mk3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
    out[3 * i] = c.x; out[3 * i + 1] = c.y; out[3 * i + 2] = c.z;
}

// ---- the queues the last frame left behind --------------------------------------------------------------------------------
// Every queue of the frame pd describes, in the order the two passes have always launched them: visit(stage row, source, upper bound of
// its rays).  The primary rays (a source that holds the frame by value), the shadow rays of the primary hits, the radiance rays of
// levels 1 .. frame_levels (all in the row of the secondary stage; level 1 has two batches rstride apart, a deeper level one ray per hit
// slot of the level before), then the shadow rays of all deeper levels that cast any, as one queue.
template <class Visit>
void for_each_queue(const PipeDev &pd, Visit &&visit)
{
    visit(RT_STAGE_PRIMARY, PrimarySrcByValue{pd}, (size_t)pd.cap);
    visit(RT_STAGE_SHADOW0, shadow_queue(pd, 0, 1), (size_t)pd.lv[0].hstride << pd.sh_log2);
    size_t deeper = 0;
    for (uint32_t l = 1; l <= frame_levels(pd.max_rad); l++) {
        visit(RT_STAGE_SECONDARY, level_rays(pd, l), l == 1 ? 2 * (size_t)pd.lv[1].rstride : (size_t)pd.lv[l - 1].hstride);
        if (l < pd.sh_levels) deeper += pd.lv[l].hstride;
    }
    if (pd.sh_levels > 1u) visit(RT_STAGE_SHADOW1, shadow_queue(pd, 1, pd.sh_levels - 1u), deeper << pd.sh_log2);
}

// count_work: one thread per ray of the bound
struct CountPass {
    hipStream_t st;
    const SceneDev &sc;
    unsigned long long *w;       // [RT_STAGE_COUNT][3]
    template <class Src>
    void operator()(int stage, const Src &src, size_t rays) const { k_count_queue<<<blocks(rays), PBLOCK, 0, st>>>(sc, src, w + 3 * stage); }
    void operator()(int stage, const ShadowQueue &queue, size_t rays) const
    {
        ShadowSrcN<true> src;
        static_cast<ShadowQueue &>(src) = queue;
        k_count_queue<<<blocks(rays), PBLOCK, 0, st>>>(sc, src, w + 3 * stage);
    }
};

// count_walk: persistent launches, which deal a queue of any length to the grid they get -- the queues' grids are sized for two rays per
// pixel slot of the set whatever the queue's own bound, and the tallies come out the same from one call to the next
template <bool TWO_LEVEL>
struct WalkPass {
    const rt_pipeline *p;
    unsigned long long *w;       // [RT_STAGE_COUNT][RT_WALK_WORDS]
    const rt_context *ctx = p->ctx;
    hipStream_t st = ctx->stream;
    const PipeDev &pd = p->last_pd;
    const unsigned gq = rt_persistent_grid(ctx, k_walk_queue<TWO_LEVEL>, PBLOCK, (size_t)pd.cap * 2);
    const unsigned gs = rt_persistent_grid(ctx, k_walk_shadow<TWO_LEVEL>, PBLOCK, (size_t)pd.cap * 2);
    void operator()(int stage, const PrimarySrcByValue &, size_t rays) const      // (the walk builds its source inside the kernel, from lists if the frame did)
    {
        unsigned long long *ws = w + RT_WALK_WORDS * stage;
        if (!TWO_LEVEL && p->primary_entries.on) {
            const uint2 *lists = p->primary_entries.lists.as<uint2>();
            const uint32_t fm = recip32(pd.n_frames), tm = recip32(pd.tiles_x);
            if (pd.n_frames > 1u) k_walk_primary_from_entries<true><<<rt_persistent_grid(ctx, k_walk_primary_from_entries<true>, PBLOCK, rays), PBLOCK, 0, st>>>(pd, lists, fm, tm, ws);
            else k_walk_primary_from_entries<false><<<rt_persistent_grid(ctx, k_walk_primary_from_entries<false>, PBLOCK, rays), PBLOCK, 0, st>>>(pd, lists, fm, tm, ws);
        } else
            k_walk_primary<TWO_LEVEL><<<rt_persistent_grid(ctx, k_walk_primary<TWO_LEVEL>, PBLOCK, rays), PBLOCK, 0, st>>>(pd, ws);
    }
    void operator()(int stage, const QueueSrc &src, size_t) const { k_walk_queue<TWO_LEVEL><<<gq, PBLOCK, 0, st>>>(pd.sc, src, w + RT_WALK_WORDS * stage); }
    void operator()(int stage, const ShadowQueue &src, size_t) const { k_walk_shadow<TWO_LEVEL><<<gs, PBLOCK, 0, st>>>(pd.sc, src, w + RT_WALK_WORDS * stage); }
};

// The head and the tail of the two counting calls (`who`): the last frame's queues must still stand and `words` counters are cleared
// (*w: where the launches put them); the launches' first error, and the counters brought back into h.
int replay_begin(rt_pipeline *p, const char *who, size_t words, unsigned long long **w)
{
    RT_TRY(rt_pipeline_flush_pending(p));
    const char *nothing = "%s: nothing rendered since the last change of scene, materials or output";
    if (p->rendered) RT_TRY(rt_scene_require_built(p->scene, who, nothing));       // (transforms, masks or vertices pending: the message names them)
    if (!p->rendered || p->scene->generation != p->last_scene_gen) { rt_set_error(nothing, who); return RT_ERR_STATE; }
    RT_TRY(rt_use_device(p->ctx));
    RT_TRY(p->work.reserve(RT_STAGE_COUNT * RT_WALK_WORDS * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(p->work.p, 0, words * sizeof(unsigned long long), p->ctx->stream));
    *w = p->work.as<unsigned long long>();
    return RT_OK;
}
int replay_end(rt_pipeline *p, unsigned long long *h, size_t words)
{
    hipStream_t st = p->ctx->stream;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, p->work.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_pipeline_count_work(rt_pipeline *p, rt_stage_work *out)
{
    RT_REQUIRE(p && out, "null argument");
    unsigned long long h[RT_STAGE_COUNT * 3], *w;
    RT_TRY(replay_begin(p, "count_work", RT_STAGE_COUNT * 3, &w));
    for_each_queue(p->last_pd, CountPass{p->ctx->stream, p->last_pd.sc, w});
    RT_TRY(replay_end(p, h, RT_STAGE_COUNT * 3));
    for (int k = 0; k < RT_STAGE_COUNT; k++) { out[k].rays = h[3 * k]; out[k].nodes = h[3 * k + 1]; out[k].tris = h[3 * k + 2]; }
    return RT_OK;
}

int rt_pipeline_count_walk(rt_pipeline *p, rt_stage_walk *out)
{
    RT_REQUIRE(p && out, "null argument");
    unsigned long long h[RT_STAGE_COUNT * RT_WALK_WORDS], *w;
    RT_TRY(replay_begin(p, "count_walk", RT_STAGE_COUNT * RT_WALK_WORDS, &w));
    if (p->scene->two_level) for_each_queue(p->last_pd, WalkPass<true>{p, w});
    else for_each_queue(p->last_pd, WalkPass<false>{p, w});
    RT_TRY(replay_end(p, h, RT_STAGE_COUNT * RT_WALK_WORDS));
    for (int k = 0; k < RT_STAGE_COUNT; k++) {
        const unsigned long long *hk = h + RT_WALK_WORDS * k;
        out[k].rays = hk[0]; out[k].nodes_global = hk[1]; out[k].nodes_lds = hk[2];
        out[k].tris = hk[3]; out[k].instance_entries = hk[4]; out[k].lines = hk[5];
        out[k].longest_walk = hk[6] >> 32;
        out[k].longest_walk_ray = (uint32_t)hk[6];
        out[k].wave_node_steps = hk[7]; out[k].wave_leaf_phases = hk[8]; out[k].wave_tri_steps = hk[9]; out[k].node_lines = hk[10];
    }
    return RT_OK;
}

// debugging aid for rt_stage_walk.longest_walk_ray: ray `index` of the level-1 radiance queue (diffuse batch, then specular batch)
int rt_debug_read_secondary_ray(rt_pipeline *p, uint32_t index, float origin_tmin[4], float dir_tmax[4])
{
    RT_REQUIRE(p && origin_tmin && dir_tmax, "null argument");
    RT_TRY(rt_pipeline_flush_pending(p));
    if (!p->rendered) { rt_set_error("nothing rendered yet"); return RT_ERR_STATE; }
    RT_TRY(rt_use_device(p->ctx));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    uint32_t n = 0;
    HIP_TRY(hipMemcpy(&n, p->last_pd.counters + C_NHIT, 4, hipMemcpyDeviceToHost));
    RT_REQUIRE(n > 0 && index < 2 * n, "ray index out of range");
    const size_t slot = (size_t)(index / n) * p->last_pd.lv[1].rstride + index % n;
    HIP_TRY(hipMemcpy(origin_tmin, p->last_pd.lv[1].O + slot, 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dir_tmax, p->last_pd.lv[1].D + slot, 16, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_pipeline_read_primary_hits(rt_pipeline *p, float *t, uint32_t *prim, uint32_t *inst)
{
    RT_REQUIRE(p, "null pipeline");
    RT_TRY(rt_pipeline_flush_pending(p));
    if (!p->rendered) { rt_set_error("nothing rendered yet"); return RT_ERR_STATE; }
    RT_TRY(rt_use_device(p->ctx));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    const PipeDev &pd = p->last_pd;
    const size_t cap = pd.cap;
    std::vector<float4> h(cap);
    std::vector<uint32_t> hi(cap);
    HIP_TRY(hipMemcpy(h.data(), p->lv[0].hit.p, cap * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hi.data(), p->lv[0].inst.p, cap * 4, hipMemcpyDeviceToHost));
    for (size_t q = 0; q < cap; q++) {          // slots are 8x8-tiled: scatter back to scanline order
        const uint32_t tl = (uint32_t)(q >> 6), w = (uint32_t)(q & 63u);
        const uint32_t lx = (tl % pd.tiles_x) * 8u + (w & 7u), ly = (tl / pd.tiles_x) * 8u + (w >> 3);
        if (lx >= pd.tw || ly >= pd.th) continue;
        const size_t i = (size_t)ly * pd.tw + lx;
        if (t) t[i] = h[q].x;
        if (prim) memcpy(&prim[i], &h[q].w, 4);
        if (inst) inst[i] = hi[q];
    }
    return RT_OK;
}

int rt_debug_sample_cube(rt_context *ctx, const float *faces, uint32_t size, uint32_t filter, const float *dirs, float *out, size_t n)
{
    RT_REQUIRE(ctx && faces && dirs && out && size > 0, "bad argument");
    RT_REQUIRE(filter == RT_CUBE_SEAMLESS || filter == RT_CUBE_FACE_CLAMP, "unknown cube-map filter");
    if (n == 0) return RT_OK;
    RT_TRY(rt_use_device(ctx));
    DevBuf *sb = ctx->scratch;
    const size_t fb = (size_t)6 * size * size * 16;
    RT_TRY(sb[0].reserve(fb)); RT_TRY(sb[1].reserve(n * 12)); RT_TRY(sb[2].reserve(n * 12));
    HIP_TRY(hipMemcpyAsync(sb[0].p, faces, fb, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(sb[1].p, dirs, n * 12, hipMemcpyHostToDevice, ctx->stream));
    PipeDev pd;
    memset(&pd, 0, sizeof pd);
    pd.env = sb[0].as<float4>();
    pd.env_size = size;
    pd.env_filter = filter;
    k_debug_cube<<<blocks(n), PBLOCK, 0, ctx->stream>>>(pd, sb[1].as<float>(), sb[2].as<float>(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, sb[2].p, n * 12, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

}  // extern "C"
