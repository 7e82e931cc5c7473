// rt_pipeline_render.hip -- the render calls of the pipeline: one frame over a region (tile, bands), sets of frames
// (rt_pipeline_render_batch, rt_pipeline_render_bands_batch), deferred mode behind update() + render(), queue-memory
// reservation and reporting, and the host side of the shadow cache and of the free sphere around the point light.  The stage kernels
// and their launch sequence: rt_pipeline.hip.  The entry lists' policy: rt_pipeline_entries.hip.  The exports that replay the last
// frame's queues (work counting, primary hits): rt_pipeline_inspect.hip.
#include <hip/hip_fp16.h>

#include <utility>

#include "rt_pipeline_queues.h"

using namespace rtd;

namespace {

// How far from a point light the scene certainly is empty: its shadow rays may stop that far short of the light (QueueSrc::load_lit) --
// nothing can occlude them inside that sphere, and all of them would otherwise walk the nodes around the light, where they converge.
// A lower bound is enough: the least distance from the light to the bounding box of any triangle (single-level scenes; to the world box
// of any instance otherwise), times 0.99, minus RAY_EPSILON.  One device pass over the triangle records per (scene, light position),
// queued behind the frame that first sees the pair and read back through page-locked memory: the frames until it has landed run
// with no sphere (a scene that changes every frame never gets one, and never waits for one).  Bench scene: 3.3 of a 32 x 11 x 14
// atrium, shadow stage -3 % (profiles/r03/free_radius.txt).
__global__ void __launch_bounds__(PBLOCK) k_free_sphere(SceneDev sc, uint32_t two_level, uint32_t n, float lx, float ly, float lz, uint32_t *out_bits)
{
    const uint32_t i = blockIdx.x * PBLOCK + threadIdx.x;
    float d2 = __uint_as_float(0x7f800000u);
    if (i < n) {
        float lo[3], hi[3];
        if (two_level) {
            const InstanceRec &in = sc.inst[i];
            for (int c = 0; c < 3; c++) { lo[c] = in.wlo[c]; hi[c] = in.whi[c]; }
        } else {
            const TriRec t = sc.inst[0].tris[i];
            const float vx[3] = {t.a.x, t.a.w, t.b.z}, vy[3] = {t.a.y, t.b.x, t.b.w}, vz[3] = {t.a.z, t.b.y, t.c.x};
            lo[0] = fminf(vx[0], fminf(vx[1], vx[2])); hi[0] = fmaxf(vx[0], fmaxf(vx[1], vx[2]));
            lo[1] = fminf(vy[0], fminf(vy[1], vy[2])); hi[1] = fmaxf(vy[0], fmaxf(vy[1], vy[2]));
            lo[2] = fminf(vz[0], fminf(vz[1], vz[2])); hi[2] = fmaxf(vz[0], fmaxf(vz[1], vz[2]));
        }
        const float l[3] = {lx, ly, lz};
        float s = 0.0f;
        bool known = true;
        for (int c = 0; c < 3; c++) {
            const float d = l[c] < lo[c] ? lo[c] - l[c] : l[c] > hi[c] ? l[c] - hi[c] : 0.0f;
            known = known && lo[c] == lo[c] && hi[c] == hi[c];
            s += d * d;
        }
        // (a box with a NaN in it says nothing about where its triangle is: the sphere has no room then.  A triangle with a NaN
        // CORNER meets no ray, but fminf / fmaxf may have hidden the NaN: not worth telling apart)
        d2 = known ? s : 0.0f;
    }
    for (int o = 32; o > 0; o >>= 1) d2 = fminf(d2, __shfl_xor(d2, o, 64));
    if ((threadIdx.x & 63u) == 0u) atomicMin(out_bits, __float_as_uint(d2));          // (non-negative floats order like their bits)
}

// a pass that has landed becomes what is known
void free_sphere_poll(rt_pipeline::FreeSphere &f)
{
    if (f.back.landed()) {
        f.known_gen = f.asked_gen;
        memcpy(f.known_lp, f.asked_lp, sizeof f.known_lp);
        // (0.99 and the term in the coordinates' size -- 32 units in the last place of the largest one -- cover the rounding of
        // the rays' own arithmetic: a ray's parameter at a triangle is exact to a few ulps of the coordinates, not of the radius)
        double size = 0.0;
        for (int c = 0; c < 3; c++) size = fmax(size, fmax(fabs((double)f.asked_lp[c]), (double)f.asked_size));
        const double r = sqrt((double)f.back.read<float>()) * 0.99 - (double)RAY_EPSILON - size * 4e-6;
        f.known_radius = r > 0.0 && r < 1e30 ? (float)r : 0.0f;
    }
}

float free_radius(rt_pipeline *p, const PipeDev &pd, const float lp[3])
{
    rt_pipeline::FreeSphere &f = p->free_sphere;
    const rt_scene *s = p->scene;
    hipStream_t st = p->ctx->stream;
    if (!(lp[0] == lp[0] && lp[1] == lp[1] && lp[2] == lp[2])) return 0.0f;
    if (!f.back.ready() || f.d_min.reserve(64) != RT_OK) return 0.0f;
    free_sphere_poll(f);
    const bool known = f.known_gen == s->generation && memcmp(f.known_lp, lp, sizeof f.known_lp) == 0;
    if (!known && !f.back.in_flight) {
        const uint32_t n = s->two_level ? (uint32_t)s->inst.size() : (s->inst.empty() || !s->inst[0].model ? 0u : s->inst[0].model->n_recs);
        if (n == 0u) return 0.0f;
        if (hipMemsetD32Async((hipDeviceptr_t)f.d_min.p, 0x7f800000, 1, st) != hipSuccess) return 0.0f;      // +inf
        k_free_sphere<<<(n + PBLOCK - 1) / PBLOCK, PBLOCK, 0, st>>>(pd.sc, s->two_level ? 1u : 0u, n, lp[0], lp[1], lp[2], f.d_min.as<uint32_t>());
        if (!f.back.send(f.d_min.p, 4, st)) return 0.0f;
        f.asked_gen = s->generation;
        const float *bb = s->two_level ? s->tlas.bounds : s->inst[0].model->blas.bounds;
        f.asked_size = 0.0f;
        for (int c = 0; c < 6; c++) f.asked_size = bb[c] == bb[c] ? fmaxf(f.asked_size, fabsf(bb[c])) : __builtin_inff();
        memcpy(f.asked_lp, lp, sizeof f.asked_lp);
    }
    return known ? f.known_radius : 0.0f;
}

// The shadow cache of the coming launches (ShadowCacheDev): single-level scenes only (an entry is an index into the one sorted
// triangle array); the table is cleared when the scene has changed (an index must stay inside the array), its directional cells
// span the bounding sphere of the model, its basis follows the frame's light (entries of another direction are merely stale).
int prepare_shadow_cache(rt_pipeline *p, const LightRays *lr)
{
    rt_pipeline::ShadowCache &sc = p->shadow_cache;
    sc.dev = ShadowCacheDev{};
    const rt_scene *s = p->scene;
    if (sc.res == 0 || s->inst.empty()) return RT_OK;
    size_t n_tris_all = 0;
    for (const SceneInstance &si : s->inst) {
        if (!si.model || si.model->n_tris >= (1u << 28)) return RT_OK;
        n_tris_all += si.model->n_tris;
    }
    int want = sc.res;
    if (want < 0) {                         // not set through the API: the context's option, else by the size of the triangles
        want = p->ctx->opt_shadow_cache_res;
        if (want == 0) return RT_OK;
    }
    if (want < 0) {
        // cells well below the triangles' size: 8 per sqrt(triangle count) across the scene, a power of two in [1024, 8192]
        // (bench scene, 262 k triangles: 1024 / 2048 / 4096 / 8192 cells -> 1.80 / 1.74 / 1.70 / 1.72 ms per frame, off 1.87;
        //  10 M triangles: 2048 -> 11.9, 8192 -> 10.9 ms, off 12.0; profiles/r03/shadow_cache*.txt)
        const double target = 8.0 * sqrt((double)n_tris_all);
        want = 1024;
        while (want < 8192 && (double)want < target) want *= 2;
    }
    if (want > 8192) want = 8192;
    if (want < 16) want = 16;
    const uint32_t res = (uint32_t)want & ~1u;
    // (+ two entries per pixel slot of the output for the primary hits' rays: ShadowCacheDev::px_base.  Measured, profiles/r04/
    // shadow_cache_pixels.txt: two-level scenes -7 % on the any-hit stage (4096 instances: 4.52 -> 4.40 ms); single-level scenes +3 % --
    // their primary hits' rays no longer seed the light-space cells the secondary hits' rays read.  So: on for two-level scenes;
    // the option shadow_cache_pixels = 0 / 1 overrides)
    const int per_pixel_opt = p->ctx->opt_shadow_cache_pixels;
    const bool per_pixel = per_pixel_opt < 0 ? s->two_level : per_pixel_opt != 0;
    const size_t cells = (size_t)res * res + 6u * (size_t)(res / 2) * (res / 2);
    const size_t px_slots = per_pixel ? (size_t)((p->width + 7u) / 8u) * ((p->height + 7u) / 8u) * 64u : 0;
    const size_t entries = cells + 2 * px_slots, entry_bytes = s->two_level ? 8 : 4;
    if (entries >= 0xffffffffull) return RT_OK;
    if (sc.table.bytes < entries * entry_bytes) { RT_TRY(sc.table.reserve(entries * entry_bytes)); sc.invalidate(); }
    if (!lr) return RT_OK;                             // (rt_pipeline_reserve_batch: the allocation only)
    if (sc.gen != s->generation) {
        HIP_TRY(hipMemsetAsync(sc.table.p, 0xff, entries * entry_bytes, p->ctx->stream));
        // the world bounds: what the builds brought back (the model's own box for one identity instance, the TLAS's otherwise)
        const float *bb = s->two_level ? s->tlas.bounds : s->inst[0].model->blas.bounds;
        float lo[3], hi[3];
        for (int c = 0; c < 3; c++) {
            lo[c] = bb[c]; hi[c] = bb[3 + c];
            if (!(lo[c] > -1e30f && hi[c] < 1e30f && lo[c] <= hi[c])) { lo[c] = -1.0f; hi[c] = 1.0f; }      // (any cell size is legal)
        }
        float r2 = 0.0f;
        for (int c = 0; c < 3; c++) { sc.centre[c] = 0.5f * (lo[c] + hi[c]); const float h = 0.5f * (hi[c] - lo[c]); r2 += h * h; }
        sc.radius = r2 > 0.0f && r2 < 1e30f ? sqrtf(r2) : 1.0f;
        sc.gen = s->generation;
    }
    ShadowCacheDev c = {};
    c.table = sc.table.as<uint32_t>();
    c.res = res; c.res_f = (float)res;
    c.two_level = s->two_level ? 1u : 0u;
    c.n_tris = s->two_level ? 0u : s->inst[0].model->n_recs;
    c.entries = (uint32_t)entries;
    c.px_base = px_slots ? (uint32_t)cells : 0u;
    c.px_slots = (uint32_t)px_slots;                 // (launch_frame fills in what belongs to the launch: jlist0, hstride0, the set's frames)
    // two unit vectors across the direction to the light
    const float d[3] = {lr->dir_to_light[0], lr->dir_to_light[1], lr->dir_to_light[2]};
    const float ref[3] = {fabsf(d[1]) < 0.9f ? 0.0f : 1.0f, fabsf(d[1]) < 0.9f ? 1.0f : 0.0f, 0.0f};
    float a[3] = {d[1] * ref[2] - d[2] * ref[1], d[2] * ref[0] - d[0] * ref[2], d[0] * ref[1] - d[1] * ref[0]};
    const float al = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (!(al > 1e-6f)) { a[0] = 1.0f; a[1] = 0.0f; a[2] = 0.0f; } else { a[0] /= al; a[1] /= al; a[2] /= al; }
    const float b[3] = {d[1] * a[2] - d[2] * a[1], d[2] * a[0] - d[0] * a[2], d[0] * a[1] - d[1] * a[0]};
    const float k = 0.5f * (float)res / sc.radius;
    c.ua[3] = 0.5f * (float)res; c.va[3] = 0.5f * (float)res;
    for (int i = 0; i < 3; i++) {
        c.ua[i] = a[i] * k; c.va[i] = b[i] * k;
        c.ua[3] -= sc.centre[i] * c.ua[i];
        c.va[3] -= sc.centre[i] * c.va[i];
        c.lp[i] = lr->point_pos[i];
    }
    sc.dev = c;
    return RT_OK;
}

// The scene as a set of n_frames frames walks it: which kernels (LDS stack rows) and the global stack rows
// behind them -- (tree bound - LDS rows) x 4 B per thread of the largest launch, and the primary stage of a single-level scene runs
// one thread per pixel slot: 4.3 GB for 20 frames of 1080p.  Insurance that is never touched on the bench scene, but an allocation:
// rt_pipeline_reserve_batch makes it too (round 4: on some boxes that hipMalloc took 126 ms of the first set's render() call).
int scene_for_set(rt_pipeline *p, uint32_t n_frames, SceneDev *out, bool *sets_kernels = nullptr)
{
    rt_context *ctx = p->ctx;
    const bool seven_waves_always = ctx->opt_seven_waves_always;      // (experiment: single frames on the sets' kernels)
    // (a scene with split triangles keeps the 18-row kernels in sets too: rt_frame_launch)
    const bool set_rows = (n_frames > 1 || seven_waves_always) && !p->scene->two_level && !p->scene->has_refs && ctx->lds_stack_rows != RT_LDS_STACK_ROWS_TEST && RT_LDS_STACK_ROWS_SETS != RT_LDS_STACK_ROWS;
    // (round 5: rows for the threads of the PERSISTENT launches only -- at most eight 256-thread workgroups per CU fit their LDS, sixteen
    // is the option's limit; the one-tile-per-wave primary launch, one thread per pixel slot, keeps none: PipeDev::retry)
    const size_t resident = (size_t)ctx->cu_count * (ctx->blocks_per_cu_override > (uint32_t)RT_RESIDENT_BLOCKS_PER_CU ? ctx->blocks_per_cu_override : (uint32_t)RT_RESIDENT_BLOCKS_PER_CU) * PBLOCK;      // (rt_persistent_grid clamps its launches to the same count)
    if (sets_kernels) *sets_kernels = set_rows;
    return rt_scene_dev_for_launch(ctx, p->scene, set_rows ? RT_LDS_STACK_ROWS_SETS : rt_lds_stack_rows(ctx), resident, out);
}

// what every render call needs before it may record or render a frame (`own_frame`: the last update()'s); `who`: the entry point, as its messages name it
int check_renderable(const rt_pipeline *p, uint32_t width, uint32_t height, bool own_frame, const char *who)
{
    RT_TRY(rt_scene_require_built(p->scene, "render", "%s: acceleration structures not built"));
    if (!p->accum) { rt_set_error("render: no output resource"); return RT_ERR_STATE; }
    if (own_frame && !p->have_pfc) { rt_set_error("render: update() has not been called"); return RT_ERR_STATE; }
    if (p->mats.empty()) { rt_set_error("render: no material"); return RT_ERR_STATE; }
    if (width != p->width || height != p->height) { rt_set_error("%s: width/height differ from the output resource", who); return RT_ERR_INVALID_ARG; }
    return RT_OK;
}

int upload_materials(rt_pipeline *p)
{
    if (!p->mats_dirty) return RT_OK;
    RT_TRY(p->d_mats.reserve(sizeof(rt_material_params) * p->mats.size()));
    HIP_TRY(hipMemcpyAsync(p->d_mats.p, p->mats.data(), sizeof(rt_material_params) * p->mats.size(), hipMemcpyHostToDevice, p->ctx->stream));
    p->mats_dirty = false;
    return RT_OK;
}

// the set's lights: the free sphere around the first frame's point light, and the shadow cache of the coming launches
int prepare_lights(rt_pipeline *p, PipeDev &pd, const SetPlan &plan, const rt_per_frame_constants &first)
{
    pd.point_free = p->ctx->opt_free_radius ? free_radius(p, pd, &first.pointLight.worldPos.x) : 0.0f;
    const LightRays lr = light_rays(1u, first);
    if (plan.ao_view) p->shadow_cache.dev = ShadowCacheDev{};      // (the light buffer is keyed by the two lights: the AO view's random rays do not use it)
    else RT_TRY(prepare_shadow_cache(p, &lr));
    return RT_OK;
}

// the constants and light rays of a set's frames go to device memory: kernels index them by the frame of a slot
int stage_set_constants(rt_pipeline *p, PipeDev &pd, const rt_per_frame_constants *frames)
{
    pd.pfc = frames[0]; pd.pfcs = nullptr; pd.frame_lights = nullptr;
    if (pd.n_frames <= 1) return RT_OK;
    std::vector<unsigned char> stage(BATCH_PFC_BYTES + BATCH_LIGHT_BYTES, 0);
    for (uint32_t f = 0; f < pd.n_frames; f++) {
        memcpy(&stage[sizeof(rt_per_frame_constants) * f], &frames[f], sizeof(rt_per_frame_constants));
        LightRays lr = light_rays(pd.shadow_compact, frames[f]);
        // (frames whose point light is where the first frame's is share its sphere; a frame with another light gets none)
        lr.point_free = memcmp(lr.point_pos, &frames[0].pointLight.worldPos, 3 * sizeof(float)) == 0 ? pd.point_free : 0.0f;
        memcpy(&stage[BATCH_PFC_BYTES + sizeof(LightRays) * f], &lr, sizeof lr);
    }
    HIP_TRY(hipMemcpyAsync(p->batch_consts.p, stage.data(), stage.size(), hipMemcpyHostToDevice, p->ctx->stream));     // (pageable source: staged before the call returns)
    pd.pfcs = p->batch_consts.as<rt_per_frame_constants>();
    pd.frame_lights = (const LightRays *)((const char *)p->batch_consts.p + BATCH_PFC_BYTES);
    return RT_OK;
}

// the rectangle [x0,x1) x [y0,y1) of the image a set of launches covers; band_rows != 0: the interleaved bands {b : b mod band_world == band_rank}
// of band_rows rows each (the rectangle then spans the full width and the rank's rows, packed)
struct Region { uint32_t x0, y0, x1, y1, band_rows, band_rank, band_world; };

// everything of PipeDev that the pipeline's state, the plan and the region decide (the scene, the lights and the constants are in already;
// the primary stage's choice follows)
void fill_pipe_dev(const rt_pipeline *p, PipeDev &pd, const SetPlan &plan, const Region &r)
{
    const uint32_t tw = r.x1 - r.x0, th = r.y1 - r.y0, cap = plan.cap;
    pd.mats = p->d_mats.as<rt_material_params>(); pd.nmats = (uint32_t)p->mats.size();
    pd.env = p->d_env.as<float4>(); pd.env_size = p->env_size; pd.env_filter = p->env_filter;
    for (int k = 0; k < 3; k++) pd.env_const[k] = p->env_const[k];
    pd.width = p->width; pd.height = p->height;
    pd.x0 = r.x0; pd.y0 = r.y0; pd.tw = tw; pd.th = th; pd.cap = cap; pd.tiles_x = (tw + 7u) / 8u;
    pd.band_rows = r.band_rows; pd.band_rank = r.band_rank; pd.band_world = r.band_world;
    uint32_t owned_rows = th;
    if (r.band_rows) {          // rows of the rank's bands that lie inside the image (the last band may be short)
        owned_rows = 0;
        for (uint32_t b = r.band_rank; (uint64_t)b * r.band_rows < p->height; b += r.band_world)
            owned_rows += (uint64_t)(b + 1) * r.band_rows <= p->height ? r.band_rows : p->height - b * r.band_rows;
    }
    pd.n_pixels = tw * owned_rows;                  // (per frame)
    pd.max_rad = p->max_rad; pd.max_shadow = p->max_shadow;
    pd.sh_log2 = plan.sh_log2;
    pd.sh_levels = shadow_levels(plan.levels, p->max_shadow);
    for (int k = 0; k <= MAXD; k++) pd.sh_cbase[k] = 0;
    pd.accum_mode = p->accum_mode; pd.accum_f16 = p->accum_f16; pd.skip_unlit = p->skip_unlit; pd.kind = p->kind;
    pd.accum = p->accum;
    pd.aov_direct = p->accum; pd.aov_indirect = p->aov_own.as<float4>();      // realtime: output 0 = direct lighting, output 1 = indirect specular
    pd.counters = p->counters.as<uint32_t>();
    for (int l = 0; l <= MAXD; l++) {          // (counted queues: launch_frame binds a level again once it has sized it)
        bind_level(p, pd, l);
        pd.lv[l].rstride = cap;
        pd.lv[l].hstride = l == 0 ? cap : 2u * cap;
    }
    static_assert(C_COUNT <= POOL_OFFSET_WORDS, "scalar counters overlap the chunk pools");
    pd.pools = pd.counters + POOL_OFFSET_WORDS;
    pd.totals = p->totals.as<unsigned long long>();
}

// how the primary stage of this set runs, and -- one tile per wave on a tree deeper than the LDS rows -- its retry list
int choose_primary_stage(rt_pipeline *p, PipeDev &pd, const rt_per_frame_constants *frames)
{
    rt_context *ctx = p->ctx;
    pd.primary_persistent = p->primary_mode.choose(ctx, p->scene) ? 1u : 0u;
    RT_TRY(rt_entries_choose(p, pd, frames));      // from per-tile entry lists or from the root
    pd.retry = nullptr; pd.retry_cap = 0;
    if (pd.sc.deep_stack && !pd.primary_persistent) {      // the primary launch keeps no rows beyond LDS: the list of the rays that would need one
        const uint32_t want = ctx->opt_primary_retry_cap ? ctx->opt_primary_retry_cap : (1u << 20);
        if (p->retry.bytes < (2 + (size_t)want) * 4) {
            RT_TRY(p->retry.reserve((2 + (size_t)want) * 4));
            HIP_TRY(hipMemsetAsync(p->retry.p, 0, 8, ctx->stream));
        }
        pd.retry = p->retry.as<uint32_t>();
        pd.retry_cap = want;
    }
    return RT_OK;
}

// one frame, or one set of n_frames frames (frames == nullptr: the frame of the last rt_pipeline_update), over a region of the image
int render_region(rt_pipeline *p, uint32_t width, uint32_t height, Region r, const rt_per_frame_constants *frames = nullptr, uint32_t n_frames = 1)
{
    RT_REQUIRE(p, "null pipeline");
    RT_TRY(check_renderable(p, width, height, !frames, __func__));
    if (!frames) { frames = &p->pfc; n_frames = 1; }
    RT_REQUIRE(n_frames >= 1 && n_frames <= RT_MAX_BATCH, "batch size");
    if (r.x1 > width) r.x1 = width;
    if (!r.band_rows && r.y1 > height) r.y1 = height;      // (band mode: y counts the rank's packed rows, checked per pixel)
    RT_REQUIRE(r.x0 < r.x1 && r.y0 < r.y1, "empty tile");
    RT_TRY(rt_use_device(p->ctx));
    p->rendered = false;
    // RayGen early-out (ProgressiveRaytracing.hlsl:14-16): nothing is traced or written (batches: the caller has dropped such frames)
    if (p->kind == RT_PIPELINE_PROGRESSIVE && frames[0].cameraParams.accumCount >= frames[0].options.maxIterations) {
        memset(&p->stats, 0, sizeof p->stats);
        return RT_OK;
    }
    RT_TRY(upload_materials(p));
    SetPlan plan;
    RT_TRY(plan_set(p, r.x1 - r.x0, r.y1 - r.y0, n_frames, p->kind == RT_PIPELINE_PROGRESSIVE && frames[0].options.showAmbientOcclusionOnly, __func__, &plan));
    RT_TRY(reserve_set(p, plan));
    p->counted_queues = plan.counted;
    PipeDev pd;
    bool set_rows = false;
    RT_TRY(scene_for_set(p, n_frames, &pd.sc, &set_rows));
    pd.n_frames = n_frames; pd.fcap = plan.fcap;
    pd.shadow_compact = plan.compact ? 1u : 0u;
    RT_TRY(prepare_lights(p, pd, plan, frames[0]));
    RT_TRY(stage_set_constants(p, pd, frames));
    fill_pipe_dev(p, pd, plan, r);
    RT_TRY(choose_primary_stage(p, pd, frames));
    RT_TRY(rt_frame_launch(p, pd, plan, set_rows));
    HIP_TRY(hipGetLastError());
    if (pd.retry) p->primary_mode.sample(p->ctx, pd.retry + 1, plan.cap, p->ctx->stream);      // this set's retry count, for the next sets' choice of primary launch
    p->last_pd = pd;
    p->last_scene_gen = p->scene->generation;
    p->last_tile[0] = r.x0; p->last_tile[1] = r.y0; p->last_tile[2] = r.x1; p->last_tile[3] = r.y1;
    p->last_pixels = pd.n_pixels * n_frames;
    p->rendered = true;
    return RT_OK;
}

// n frames through shared sets of launches; band_rows != 0: only the rank's interleaved bands of every frame
int render_frames(rt_pipeline *p, uint32_t width, uint32_t height, const rt_per_frame_constants *constants, uint32_t n,
                  uint32_t band_rows, uint32_t band_rank, uint32_t band_world)
{
    uint32_t band_count = 0;
    if (band_rows) {
        RT_TRY(rt_tile_bands(height, band_rows, band_rank, band_world, nullptr, nullptr, 0, &band_count));
        if (band_count == 0) n = 0;             // more ranks than bands: nothing to render here (the constants still become current)
    }
    const Region region = band_rows ? Region{0, 0, width, band_count * band_rows, band_rows, band_rank, band_world} : Region{0, 0, width, height, 0, 0, 1};
    uint32_t batch_max = RT_MAX_BATCH;
    if (p->ctx->opt_batch_max >= 1 && p->ctx->opt_batch_max <= RT_MAX_BATCH) batch_max = p->ctx->opt_batch_max;
    // frames RayGen would leave at once (accumCount >= maxIterations, ProgressiveRaytracing.hlsl:14-16) are dropped here;
    // frames that disagree on what sizes the queues (the ambient-occlusion view) do not share a set of launches
    std::vector<rt_per_frame_constants> run;
    auto flush = [&]() -> int {
        // the queues grow with the batch: when the device cannot hold them, the same frames go through in smaller sets
        for (size_t at = 0; at < run.size();) {
            const size_t n_now = run.size() - at < batch_max ? run.size() - at : batch_max;
            const int rc = render_region(p, width, height, region, run.data() + at, (uint32_t)n_now);
            if (rc == RT_ERR_OOM && n_now > 1) { batch_max = (uint32_t)(n_now / 2); continue; }
            if (rc != RT_OK) { run.clear(); return rc; }
            at += n_now;
        }
        run.clear();
        return RT_OK;
    };
    for (uint32_t i = 0; i < n; i++) {
        const rt_per_frame_constants &c = constants[i];
        if (c.cameraParams.accumCount >= c.options.maxIterations) continue;
        if (!run.empty() && (run.size() >= batch_max || (run[0].options.showAmbientOcclusionOnly != 0) != (c.options.showAmbientOcclusionOnly != 0))) RT_TRY(flush());
        run.push_back(c);
    }
    return flush();
}

int flush_pending_now(rt_pipeline *p)
{
    if (p->pending.empty()) return RT_OK;
    std::vector<rt_per_frame_constants> frames;
    frames.swap(p->pending);                    // (whatever happens, the frames are not rendered twice)
    std::vector<rt_pipeline *> &reg = p->ctx->deferred;
    for (size_t k = 0; k < reg.size(); k++) if (reg[k] == p) { reg.erase(reg.begin() + (long)k); break; }
    const rt_per_frame_constants keep = p->pfc;              // the constants of the last update(): a frame may have been updated and not rendered yet
    const int rc = render_frames(p, p->width, p->height, frames.data(), (uint32_t)frames.size(), 0, 0, 1);
    p->pfc = keep;
    return rc;
}

}  // namespace

// The primary stage as a persistent launch that refills its lanes from a pool of tiles (instead of one tile per wave, dealt by the
// hardware): pays where the rays of a tile part ways early -- two-level scenes, whose primary waves run at 0.48 of their lanes
// (4096 instances at 4K: 1.39 -> 1.31 ms) -- and costs 13 % where they stay together (the single-level bench scene: 0.69 of the lanes
// as it is).  The option primary_persistent = 0 / 1 overrides.  profiles/r04/c4_variants.txt, primary_persistent.txt
// (single-level scenes: one tile per wave, unless this scene's retry lists said otherwise -- rt_pipeline::PrimaryMode)
bool rt_pipeline::PrimaryMode::choose(const rt_context *ctx, const rt_scene *scene)
{
    if (gen != scene->generation) { gen = scene->generation; samples = 0; persistent = false; back.in_flight = false; }
    if (back.landed()) {
        samples++;
        if ((double)back.read<uint32_t>() > 0.002 * (double)asked_slots) persistent = true;       // more than 0.2 % of the primary rays
    }
    return ctx->opt_primary_persistent < 0 ? (scene->two_level || persistent) : ctx->opt_primary_persistent != 0;
}

// (the set's compaction has cleared retry[0] and left the count in retry[1]: d_count)
void rt_pipeline::PrimaryMode::sample(const rt_context *ctx, const uint32_t *d_count, uint32_t slots, hipStream_t st)
{
    if (back.in_flight || samples >= 8 || ctx->opt_primary_persistent >= 0) return;
    if (back.send(d_count, 4, st)) asked_slots = slots;
}

// every entry point of the pipeline that renders, reads or changes what recorded frames would see calls this first
int rt_pipeline_flush_pending(rt_pipeline *p)
{
    if (!p) return RT_OK;
    if (p->deferred_error != RT_OK) {           // a flush behind somebody else's call failed: this pipeline's caller hears of it here, once
        const int rc = p->deferred_error;
        rt_set_error("deferred frames were lost: %s", p->deferred_error_msg.c_str());
        p->deferred_error = RT_OK;
        p->deferred_error_msg.clear();
        return rc;
    }
    return flush_pending_now(p);
}

// Calls that are not about one pipeline (scene changes, rt_context_synchronize, the collectives) render what every deferred
// pipeline of the context still holds.  A failure there belongs to the pipeline, not to the caller's own work: it is parked on
// the pipeline (see deferred_error) and the call goes on.
int rt_context_flush_deferred(rt_context *ctx)
{
    if (!ctx) return RT_OK;
    while (!ctx->deferred.empty()) {
        rt_pipeline *p = ctx->deferred.back();
        const int rc = flush_pending_now(p);      // (a flush takes the pipeline off the list)
        if (rc != RT_OK && p->deferred_error == RT_OK) { p->deferred_error = rc; p->deferred_error_msg = rt_last_error(); }
    }
    return RT_OK;
}

extern "C" {

int rt_pipeline_flush(rt_pipeline *p)
{
    RT_REQUIRE(p, "null pipeline");
    return rt_pipeline_flush_pending(p);
}

int rt_pipeline_set_deferred(rt_pipeline *p, uint32_t max_frames)
{
    RT_REQUIRE(p, "null pipeline");
    RT_REQUIRE(max_frames <= RT_MAX_BATCH, "set_deferred: at most 32 frames share a set of launches");
    RT_REQUIRE(p->kind == RT_PIPELINE_PROGRESSIVE || max_frames <= 1, "set_deferred: only the progressive pipeline accumulates frames");
    RT_TRY(rt_pipeline_flush_pending(p));
    p->deferred_max = max_frames;
    return RT_OK;
}

int rt_pipeline_get_deferred(const rt_pipeline *p, uint32_t *max_frames, uint32_t *pending)
{
    RT_REQUIRE(p, "null pipeline");
    if (max_frames) *max_frames = p->deferred_max;
    if (pending) *pending = (uint32_t)p->pending.size();
    return RT_OK;
}

int rt_pipeline_render_tile(rt_pipeline *p, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
{
    RT_TRY(rt_pipeline_flush_pending(p));
    return render_region(p, width, height, Region{x0, y0, x1, y1, 0, 0, 1});
}

int rt_pipeline_render_bands(rt_pipeline *p, uint32_t width, uint32_t height, uint32_t band_rows, uint32_t rank, uint32_t world)
{
    RT_REQUIRE(world > 0 && rank < world, "rank outside [0, world)");
    RT_REQUIRE(band_rows > 0 && band_rows % 8 == 0, "band_rows must be a positive multiple of 8 (pixel slots are 8x8 tiles)");
    RT_TRY(rt_pipeline_flush_pending(p));
    uint32_t n = 0;
    RT_TRY(rt_tile_bands(height, band_rows, rank, world, nullptr, nullptr, 0, &n));
    if (n == 0) return RT_OK;                   // more ranks than bands: nothing to render here
    return render_region(p, width, height, Region{0, 0, width, n * band_rows, band_rows, rank, world});
}

int rt_pipeline_render(rt_pipeline *p, uint32_t width, uint32_t height)
{
    RT_REQUIRE(p, "null pipeline");
    if (p->deferred_max > 1 && p->kind == RT_PIPELINE_PROGRESSIVE) {
        RT_TRY(check_renderable(p, width, height, true, __func__));      // a bad call fails where it is made and not at some later flush
        if (p->pending.empty()) p->ctx->deferred.push_back(p);
        p->pending.push_back(p->pfc);
        p->rendered = false;                    // (nothing of the LAST frame is on the device yet: count_work / stats flush first)
        if (p->pending.size() >= p->deferred_max) return rt_pipeline_flush_pending(p);
        return RT_OK;
    }
    return rt_pipeline_render_tile(p, width, height, 0, 0, width, height);
}

int rt_pipeline_render_batch(rt_pipeline *p, uint32_t width, uint32_t height, const rt_per_frame_constants *constants, uint32_t n)
{
    RT_REQUIRE(p && (constants || n == 0), "null argument");
    RT_REQUIRE(p->kind == RT_PIPELINE_PROGRESSIVE, "render_batch: only the progressive pipeline accumulates frames");
    RT_TRY(rt_pipeline_flush_pending(p));
    RT_TRY(render_frames(p, width, height, constants, n, 0, 0, 1));
    if (n) { p->pfc = constants[n - 1]; p->have_pfc = true; }     // as after n x (update, render)
    return RT_OK;
}

int rt_pipeline_render_bands_batch(rt_pipeline *p, uint32_t width, uint32_t height, uint32_t band_rows, uint32_t rank, uint32_t world,
                                   const rt_per_frame_constants *constants, uint32_t n)
{
    RT_REQUIRE(p && (constants || n == 0), "null argument");
    RT_REQUIRE(p->kind == RT_PIPELINE_PROGRESSIVE, "render_bands_batch: only the progressive pipeline accumulates frames");
    RT_REQUIRE(world > 0 && rank < world, "rank outside [0, world)");
    RT_REQUIRE(band_rows > 0 && band_rows % 8 == 0, "band_rows must be a positive multiple of 8 (pixel slots are 8x8 tiles)");
    RT_TRY(rt_pipeline_flush_pending(p));
    RT_TRY(render_frames(p, width, height, constants, n, band_rows, rank, world));
    if (n) { p->pfc = constants[n - 1]; p->have_pfc = true; }
    return RT_OK;
}

int rt_pipeline_set_queue_budget(rt_pipeline *p, size_t bytes)
{
    RT_REQUIRE(p, "null pipeline");
    p->queue_budget = bytes;
    return RT_OK;
}

int rt_pipeline_get_queue_memory(rt_pipeline *p, size_t *bytes_reserved, uint32_t *sized_by_count)
{
    RT_REQUIRE(p, "null pipeline");
    size_t total = p->counters.bytes + p->batch_consts.bytes + p->sh_hits.bytes + p->sh_O.bytes + p->sh_D.bytes + p->sh_vis.bytes;
    for (const rt_pipeline::LevelBuf &l : p->lv) {
        const DevBuf *lb[] = {&l.O, &l.D, &l.hit, &l.inst, &l.slot_j, &l.jlist, &l.pix, &l.color};
        for (const DevBuf *b : lb) total += b->bytes;
    }
    if (bytes_reserved) *bytes_reserved = total;
    if (sized_by_count) *sized_by_count = p->counted_queues ? 1u : 0u;
    return RT_OK;
}

int rt_pipeline_reserve_batch(rt_pipeline *p, uint32_t width, uint32_t height, uint32_t frames)
{
    RT_REQUIRE(p && width > 0 && height > 0 && frames >= 1 && frames <= RT_MAX_BATCH, "reserve_batch: bad argument");
    RT_TRY(rt_use_device(p->ctx));
    // (a set whose worst case is over the budget sizes its levels by count as it goes: only the pixel slots are known now)
    SetPlan plan;
    RT_TRY(plan_set(p, width, height, frames, p->have_pfc && p->pfc.options.showAmbientOcclusionOnly != 0, __func__, &plan));
    // Any buffer this call grows is a buffer the last frame's replay calls (count_work, count_walk, read_primary_hits, ...) still hold
    // pointers to in last_pd: a reservation therefore ends what was "rendered" (the calls then refuse instead of
    // launching on freed memory).  Frames a deferred pipeline still holds are rendered first: they own the queues as they are.
    RT_TRY(rt_pipeline_flush_pending(p));
    p->rendered = false;
    RT_TRY(reserve_set(p, plan));
    if (p->scene && p->scene->built) {                 // the traversal kernels' global stack rows and the shadow cache's table as well
        SceneDev sc;
        RT_TRY(scene_for_set(p, frames, &sc));
        RT_TRY(prepare_shadow_cache(p, nullptr));
        p->shadow_cache.dev = ShadowCacheDev{};
    }
    return RT_OK;
}

int rt_pipeline_get_free_sphere(rt_pipeline *p, float *radius)
{
    RT_REQUIRE(p && radius, "get_free_sphere: null argument");
    *radius = 0.0f;
    rt_pipeline::FreeSphere &f = p->free_sphere;
    if (!p->scene || !p->have_pfc || !f.back.block) return RT_OK;
    RT_TRY(rt_use_device(p->ctx));
    free_sphere_poll(f);
    const float *lp = &p->pfc.pointLight.worldPos.x;
    if (f.known_gen == p->scene->generation && memcmp(f.known_lp, lp, sizeof f.known_lp) == 0) *radius = f.known_radius;
    return RT_OK;
}

}  // extern "C"
