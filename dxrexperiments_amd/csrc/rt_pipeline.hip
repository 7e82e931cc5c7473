// rt_pipeline.hip -- the ProgressiveRaytracingPipeline on gfx950.
//
// The reference renders a frame with ONE DispatchRays whose raygen shader recurses
// through TraceRay (src/ProgressiveRaytracingPipeline.cpp:215-247 ->
// assets/shaders/ProgressiveRaytracing.hlsl).  Here the same per-pixel recursion
// (reference limits: depth <= 1 radiance, <= 2 shadow, RaytracingCommon.hlsli:11-12;
// this engine: radiance depth <= MAXD = 4) becomes a wavefront DAG of ray queues in
// HBM, one kernel per stage:
//
//   primary        raygen + closest-hit traversal (cull back faces) -> level-0 hits, compaction
//   shade 0 / emit PrimaryClosestHit -> shade(): emits 2 (AO: 4) shadow rays + the diffuse and
//                  the specular ray of level 1
//   for l = 1..max radiance depth:
//     trace l      closest-hit over the ray queue of level l, compaction of its hits
//     shade l/emit closest-hit shading of those hits: 2 shadow rays each + the specular ray of l+1
//   shadow         any-hit over the shadow queues of ALL levels in one persistent launch
//   resolve        re-runs shade() with every TraceRay replaced by its stored result, then
//                  gOutput = (n*prev + cur)/(n+1)                      (ProgressiveRaytracing.hlsl:36-38)
//
// shade() is ONE template used in both the emit and the resolve stage, so the
// arithmetic (and the RNG draw order) of both passes is identical by construction.
// Queues are SoA float4 arrays (origin|tmin, direction|tmax) so a wave reads 1 KiB
// per instruction; hits are compacted with __ballot + popcount prefix sums and one
// atomic per 1024-thread block; diffuse and specular secondaries sit in separate
// batches so waves stay as coherent as the sampling allows.
//
// This file: the stage kernels and the launch sequence of a frame (or of a set of frames).
// rt_pipeline_rays.h: the ray sources and sinks of the stages.  rt_shade.h: the shaders as device functions.
// rt_pipeline_dev.h: PipeDev and the host object.  rt_pipeline_queues.h: queue memory.
// rt_pipeline_entries.hip: the primary stage's entry lists (policy, kernel, launch, read-back).
// rt_pipeline_render.hip: the render calls (regions, sets of frames, deferred mode), the shadow cache's and the free sphere's host side.
// rt_pipeline_inspect.hip: the calls that replay the last frame's queues (work and walk counting, read-backs).
// rt_pipeline_host.hip: creation, setters, outputs, checkpoints, timing and statistics.
#include <hip/hip_fp16.h>

#include "rt_pipeline_rays.h"

using namespace rtd;

namespace {

// ---- compaction ----------------------------------------------------------------------
constexpr int CBLOCK = 1024;

// ---- kernels -------------------------------------------------------------------------

// (see RT_LDS_STACK_ROWS_SETS: the single-level instantiations with that many stack rows are compiled for seven waves per SIMD,
// the 18-row ones for the six their LDS allows (the any-hit kernel with the shadow cache would take 81 registers otherwise);
// the two-level ones for five -- they take 88 - 96 registers by themselves, except the primary stage of a set (99: a fourth wave lost
// for three registers; capped it fits 96 without scratch))
#ifndef RT_WAVES_PER_EU
#define RT_WAVES_PER_EU __attribute__((amdgpu_waves_per_eu(TWO_LEVEL ? 5 : RT_ROWS(STACK) == RT_LDS_STACK_ROWS_SETS ? 7 : RT_ROWS(STACK) == RT_LDS_STACK_ROWS ? 6 : 1)))
#endif
// the frame's counters and chunk pools start at zero: its first kernel clears them (nothing there uses them, every later
// kernel of the frame does) instead of a 20-KB fill launch of its own
RT_DEV void clear_frame_counters(const PipeDev &pd)
{
    if (blockIdx.x == 0)
        for (uint32_t i = threadIdx.x; i < (uint32_t)(POOL_OFFSET_WORDS + POOL_BYTES / 4); i += PBLOCK) pd.counters[i] = 0u;
}
// rays a wave of a persistent launch takes from its queue at a time: the long launches of a set of frames (the seven-wave single-level
// kernels) take more, its any-hit launch more still (RT_POOL_CHUNK*, rt_trace_wave.h)
constexpr uint32_t pool_chunk(int stack, bool two_level, bool anyhit)
{
    return !two_level && RT_ROWS(stack) == RT_LDS_STACK_ROWS_SETS ? (anyhit ? RT_POOL_CHUNK_SETS_ANYHIT : RT_POOL_CHUNK_SETS) : RT_POOL_CHUNK;
}

// PERSIST = false: one 8x8 tile per wave, dealt by the hardware dispatcher -- one thread per pixel slot, so this launch keeps NO stack rows
// beyond LDS (NO_DEEP: a ray that would need one goes to PipeDev::retry and k_primary_retry walks it); true: a persistent launch that refills
// its lanes from a pool of tiles (two-level scenes), with rows by resident thread like the other persistent launches
template <int STACK, bool TWO_LEVEL, bool BATCH, bool PERSIST>
__global__ void __launch_bounds__(PBLOCK) RT_WAVES_PER_EU k_primary(PipeDev pd)
{
    __shared__ int smem[walk_lds_words(RT_ROWS(STACK))];
    clear_frame_counters(pd);
    PrimarySrcT<BATCH> src = {pd};
    PrimarySink sink = {pd};
    if (PERSIST) trace_wave<RT_ROWS(STACK), PBLOCK, TWO_LEVEL, 64u, false, false, false, RT_REFS(STACK)>(pd.sc, src, sink, pd.pools + POOL_BYTES / 4, smem, nullptr);
    else trace_wave<RT_ROWS(STACK), PBLOCK, TWO_LEVEL, 64u, false, false, true, RT_REFS(STACK)>(pd.sc, src, sink, nullptr, smem, nullptr);
}

// the pixel slots k_primary<.., PERSIST = false> gave up, walked from the start by a persistent launch with rows beyond LDS (static deal of
// the list: there is next to nothing on it -- on the bench scenes nothing: the launch returns before it touches its LDS)
template <int STACK, bool TWO_LEVEL>
__global__ void __launch_bounds__(PBLOCK) RT_WAVES_PER_EU k_primary_retry(PipeDev pd)
{
    __shared__ int smem[walk_lds_words(RT_ROWS(STACK))];
    if (pd.retry[0] == 0u) return;
    PrimaryRetrySrc src = {pd};
    PrimarySink sink = {pd};
    trace_wave<RT_ROWS(STACK), PBLOCK, TWO_LEVEL, 64u, false, false, false, RT_REFS(STACK)>(pd.sc, src, sink, nullptr, smem, nullptr);
}

// k_primary<.., false, BATCH, false> whose rays start from their tile's entry list instead of the root (single-level scenes; the rays it gives
// up go to k_primary_retry like the others', which walks them from the root).  No table of the top in LDS: one row behind the stack rows
// holds the lanes' places in their lists.
template <int STACK, bool BATCH, bool TWO_LEVEL = false>
__global__ void __launch_bounds__(PBLOCK) RT_WAVES_PER_EU k_primary_from_entries(PipeDev pd, const uint2 *__restrict__ entries, uint32_t frames_magic, uint32_t tiles_x_magic)
{
    __shared__ int smem[walk_lds_words(RT_ROWS(STACK), true)];
    clear_frame_counters(pd);
    PrimaryEntrySrcT<BATCH> src = {{pd}, entries, frames_magic, tiles_x_magic};
    PrimarySink sink = {pd};
    trace_wave<RT_ROWS(STACK), PBLOCK, false, 64u, false, false, true, RT_REFS(STACK)>(pd.sc, src, sink, nullptr, smem, nullptr);
}

// Compaction of the hits of level L (they get shaded).  Level 0 runs over the pixel slots, level 1 over its two batches,
// deeper levels over one batch.  A block owns CTILES consecutive tiles of CBLOCK slots: it first counts its hits (each
// thread remembers its CTILES flags in a bit mask), reserves its output range with ONE atomic, then writes tile after
// tile in slot order -- same-address returning atomics serialise at ~11 ns, and one per 1024 slots (2,000 - 4,000 per
// launch at 1080p) was most of this kernel's 36 us.
constexpr int CTILES = 8;            // (tiles per workgroup 4 / 8 / 16: 41 / 40 / 45 us for the frame's two compactions)
__global__ void __launch_bounds__(CBLOCK) k_compact_level(PipeDev pd, int L)
{
    __shared__ uint32_t wave_total[CBLOCK / 64];
    __shared__ uint32_t block_base;
    uint32_t total_items, n = 0;
    if (L == 0) total_items = pd.cap;
    else { n = pd.counters[C_NHIT + L - 1]; total_items = (L == 1 ? 2u : 1u) * n; }
    if (L == 0 && pd.retry && blockIdx.x == 0 && threadIdx.x == 0) { pd.retry[1] = pd.retry[0]; pd.retry[0] = 0u; }      // (the retry launch in front of this one has used it;
                                                                                                                           //  [1]: the set's count, for the host's choice of primary launch)
    const uint32_t first = blockIdx.x * (uint32_t)(CTILES * CBLOCK);
    if (first >= total_items) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    auto slot_of = [&](uint32_t idx) -> size_t { return L == 1 ? (size_t)(idx / n) * pd.lv[1].rstride + idx % n : (size_t)idx; };
    uint32_t flags = 0, mine = 0;
#pragma unroll 4
    for (int t = 0; t < CTILES; t++) {
        const uint32_t idx = first + (uint32_t)t * CBLOCK + threadIdx.x;
        const bool hit = idx < total_items && pd.lv[L].hit[slot_of(idx)].x >= 0.0f;
        flags |= (hit ? 1u : 0u) << t;
        mine += hit ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o, 64);
    if (lane == 0) wave_total[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < CBLOCK / 64; w++) sum += wave_total[w];
        block_base = sum ? atomicAdd(&pd.counters[C_NHIT + L], sum) : 0u;
    }
    __syncthreads();
    uint32_t running = block_base;
    for (int t = 0; t < CTILES; t++) {
        const uint32_t idx = first + (uint32_t)t * CBLOCK + threadIdx.x;
        if (first + (uint32_t)t * CBLOCK >= total_items) break;          // (block-uniform)
        const bool hit = (flags >> t) & 1u;
        const unsigned long long mask = __ballot(hit);
        __syncthreads();                                                 // wave_total is reused tile after tile
        if (lane == 0) wave_total[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, tile_total = 0;
        for (int w = 0; w < CBLOCK / 64; w++) { const uint32_t c = wave_total[w]; before += w < (int)wave ? c : 0u; tile_total += c; }
        const uint32_t j = running + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (idx < total_items) {
            const size_t slot = slot_of(idx);
            pd.lv[L].slot_j[slot] = hit ? j : RT_NO_HIT;
            if (hit) pd.lv[L].jlist[j] = (uint32_t)slot;
        }
        running += tile_total;
    }
}

// closest-hit shading of the compacted hits of level L in emit mode: writes their shadow rays and the rays
// of level L+1; slots a hit does not use are marked "not traced"
// BATCH: the launch covers several frames; a hit takes the constants of the frame its pixel slot lies in
// (LC >= 0: the level as a compile-time constant, from the time when the batch kernels replaced pfc in a per-thread copy of the arguments
// and a run-time index into the copy's lv[] put it into scratch memory.  Since round 17 they copy the frame's constants alone -- fc,
// rt_shade.h -- and the compiler makes the same code of it.)
template <bool PRIMARY, bool BATCH, int LC>
RT_DEV void shade_emit_body(const PipeDev &pd, int level, uint32_t shadow_slots, uint32_t emit_next)
{
    const int L = PRIMARY ? 0 : (LC >= 0 ? LC : level);          // (depth 0 compiles to its own kernel: it alone samples indirect diffuse)
    __builtin_assume(PRIMARY || L >= 1);
    const uint32_t idx = blockIdx.x * PBLOCK + threadIdx.x;
    if (idx >= pd.counters[C_NHIT + L]) return;
    const uint32_t slot = pd.lv[L].jlist[idx];
    const uint32_t q = L == 0 ? slot : pd.lv[L].pix[slot];
    uint32_t px, py, ql = q, frame = 0;
    // (the hits of a wave come from several frames: a thread takes its frame's constants in one go, 188 B that arrive together --
    //  read field by field where they are used they cost this memory-bound kernel 14 %)
    rt_per_frame_constants own;
    if (BATCH) { frame = slot_frame(pd, q, ql); own = pd.pfcs[frame]; }
    const rt_per_frame_constants &fc = BATCH ? own : pd.pfc;
    (void)pix_xy(pd, ql, px, py);
    const RayD r = L == 0 ? primary_ray(pd, fc.cameraParams, px, py) : load_ray(pd.lv[L].O, pd.lv[L].D, slot);
    const float4 h = pd.lv[L].hit[slot];
    if (!PRIMARY && !emit_next && pd.shadow_compact && !pd.skip_unlit) {
        // The LAST radiance level (round 4): its hits spawn nothing, so all the emit pass has to leave is where their two light
        // rays start -- P = O + t D, the expression of closest_hit_aov -- and which of the two exist: both
        // (RaytracingCommon.hlsli:126-147 trace them whatever N.L is), or the one shade() draws in the one-light view
        // (ProgressiveRaytracing.hlsl:92-97: the first number of the pixel's sequence).  No normals record, no material, no
        // lobe sample: the resolve pass shades these hits anyway.  (With the reference's depth limits this is every secondary
        // hit: 3.7 M per 1080p frame, the emit kernel 0.065 -> 0.02 ms.)
        const f3 P = r.o + r.d * h.x;
        uint32_t mask = 3u;
        if (pd.kind != RT_PIPELINE_REALTIME && fc.options.debug == 2) {
            uint32_t seed = init_rand(px + py * pd.width, fc.cameraParams.frameCount);
            mask = next_rand(seed) < 0.5f ? 1u : 2u;
        }
        if ((uint32_t)L < pd.sh_levels) pd.sh_hits[pd.sh_cbase[L] + idx] = make_float4(P.x, P.y, P.z, __uint_as_float(mask | (frame << 8)));
        return;
    }
    EmitIO io(pd, fc, L, idx, q, frame);
    (void)closest_hit(pd, fc, io, r, h.x, h.y, h.z, __float_as_uint(h.w), pd.lv[L].inst[slot], (uint32_t)L, px + py * pd.width);
    io.finish_shadows(shadow_slots);
    if (emit_next) {
        if (L == 0) {
            for (uint32_t w = 0; w < 2; w++)
                if (!(io.sec_mask & (1u << w))) store_invalid(pd.lv[1].O, pd.lv[1].D, (size_t)w * pd.lv[1].rstride + idx);
        } else if (L < MAXD && !io.sec_mask) store_invalid(pd.lv[L < MAXD ? L + 1 : MAXD].O, pd.lv[L < MAXD ? L + 1 : MAXD].D, idx);
    }
}
template <bool PRIMARY, bool BATCH>
__global__ void __launch_bounds__(PBLOCK) k_shade_emit(PipeDev pd, int level, uint32_t shadow_slots, uint32_t emit_next)
{
    if (PRIMARY || !BATCH) shade_emit_body<PRIMARY, BATCH, -1>(pd, level, shadow_slots, emit_next);
    else if (level == 1) shade_emit_body<PRIMARY, BATCH, 1>(pd, level, shadow_slots, emit_next);
    else if (level == 2) shade_emit_body<PRIMARY, BATCH, 2>(pd, level, shadow_slots, emit_next);
    else if (level == 3) shade_emit_body<PRIMARY, BATCH, 3>(pd, level, shadow_slots, emit_next);
    else shade_emit_body<PRIMARY, BATCH, MAXD>(pd, level, shadow_slots, emit_next);
}

template <int STACK, bool TWO_LEVEL, bool BATCH>
__global__ void __launch_bounds__(PBLOCK) RT_WAVES_PER_EU k_trace_shadow(SceneDev sc, ShadowQueue queues, uint32_t *pool, uint32_t *stat)
{
    __shared__ int smem[walk_lds_words(RT_ROWS(STACK))];
    ShadowSrcN<BATCH> src;
    static_cast<ShadowQueue &>(src) = queues;
    ShadowSinkN sink = {queues};
    trace_wave<RT_ROWS(STACK), PBLOCK, TWO_LEVEL, pool_chunk(STACK, TWO_LEVEL, true), true, false, false, RT_REFS(STACK)>(sc, src, sink, pool, smem, stat);
}

template <int STACK, bool TWO_LEVEL>
__global__ void __launch_bounds__(PBLOCK) RT_WAVES_PER_EU k_trace_secondary(SceneDev sc, QueueSrc src, float4 *hit1, uint32_t *inst1, uint32_t *pool, uint32_t *stat)
{
    __shared__ int smem[walk_lds_words(RT_ROWS(STACK))];
    SecondarySink sink = {src, hit1, inst1};
    trace_wave<RT_ROWS(STACK), PBLOCK, TWO_LEVEL, pool_chunk(STACK, TWO_LEVEL, false), false, false, false, RT_REFS(STACK)>(sc, src, sink, pool, smem, stat);
}

// the frame's ray / hit counts into the running totals (one thread, once per frame)
RT_DEV void add_totals(const uint32_t *__restrict__ counters, unsigned long long *__restrict__ totals, uint32_t pixels, uint32_t frames)
{
    totals[0] += (unsigned long long)pixels * frames;
    totals[1] += counters[C_SECONDARY];
    totals[2] += counters[C_SHADOW] + counters[C_SHADOW_SKIPPED];
    totals[6] += counters[C_SHADOW_SKIPPED];
    totals[3] += counters[C_NHIT + 0];
    for (int l = 1; l <= MAXD; l++) totals[4] += counters[C_NHIT + l];
    totals[5] += frames;
}

// what the frame's last kernel does with the colour of pixel slot q (RayGen's tail, ProgressiveRaytracing.hlsl:36-38 /
// RealtimeRaytracing.hlsl:44-45)
RT_DEV float4 accumulate(const PipeDev &pd, const rt_per_frame_constants &fc, const float4 prev, const Shaded &sh)
{
    const f3 c = sh.color;
    const float4 cur = make_float4(fmax2(c.x, 0.0f), fmax2(c.y, 0.0f), fmax2(c.z, 0.0f), 1.0f);
    if (pd.accum_mode == RT_ACCUM_SUM) return make_float4(prev.x + cur.x, prev.y + cur.y, prev.z + cur.z, prev.w + cur.w);
    const float n = (float)fc.cameraParams.accumCount;
    const float n1 = (float)(fc.cameraParams.accumCount + 1u);
    float4 m = make_float4((n * prev.x + cur.x) / n1, (n * prev.y + cur.y) / n1, (n * prev.z + cur.z) / n1, (n * prev.w + cur.w) / n1);
    // the reference's RGBA16F texture (src/DXRExperimentsApp.cpp:28): what the next frame reads back is this mean rounded to fp16
    if (pd.accum_f16 == 1u) m = make_float4(__half2float(__float2half_rn(m.x)), __half2float(__float2half_rn(m.y)), __half2float(__float2half_rn(m.z)), __half2float(__float2half_rn(m.w)));
    else if (pd.accum_f16 == 2u) m = make_float4(__half2float(__float2half_rz(m.x)), __half2float(__float2half_rz(m.y)), __half2float(__float2half_rz(m.z)), __half2float(__float2half_rz(m.w)));
    return m;
}
RT_DEV void write_aovs(const PipeDev &pd, size_t pixel, const Shaded &sh)          // two AOVs, no accumulation
{
    pd.aov_direct[pixel] = make_float4(fmax2(sh.aov_direct.x, 0.0f), fmax2(sh.aov_direct.y, 0.0f), fmax2(sh.aov_direct.z, 0.0f), 1.0f);
    pd.aov_indirect[pixel] = make_float4(fmax2(sh.aov_indirect.x, 0.0f), fmax2(sh.aov_indirect.y, 0.0f), fmax2(sh.aov_indirect.z, 0.0f), 1.0f);
}

// FLAT = false: one bounce at most, the secondary hits are shaded inline (ResolveIO<0, 1>); FLAT = true: their colours
// come from k_shade_level (LevelResolveIO)
// pfcs: the constants of the set's frames (PipeDev::pfcs once more, as an argument of its own: `const __restrict__` tells the compiler that no
// store of this kernel reaches them, and with the frame the same for the whole wave every field of frame f is then fetched by a scalar load
// where it is used.  Until round 17 each thread replaced pfc in a copy of the arguments: the frame's 47 dwords came by vector loads and
// stayed in vector registers for as long as shade() needed them.)
// Registers (round 17, profiles/r17/resolve_sets.txt): the set form of the one-bounce kernel took 116 VGPRs = four waves per SIMD against the
// single-frame form's 88 = five.  Reading the constants in place leaves 101; the rest is what a pixel carries from frame to frame -- the
// running value (4), its index (2), the parts of the primary ray that do not depend on the frame, its slot.  Capped at five waves (96) the
// allocator then spills 12 B; with the pixel's index worked out again behind the loop it fits 96 with no scratch.  The other three forms
// keep the occupancy they had (the cap is the number of waves they reached by themselves).
template <bool FLAT, bool BATCH>
__global__ void __launch_bounds__(PBLOCK) __attribute__((amdgpu_waves_per_eu(FLAT && !BATCH ? 6 : 5))) k_resolve(PipeDev pd, const rt_per_frame_constants *__restrict__ pfcs)
{
    const uint32_t ql = blockIdx.x * PBLOCK + threadIdx.x;
    if (ql == 0) add_totals(pd.counters, pd.totals, pd.n_pixels, pd.n_frames);      // every counter of the frame is final when this kernel starts
    if (ql >= pd.fcap) return;
    uint32_t px, py;
    if (!pix_xy(pd, ql, px, py)) return;
    // a batch: the frames of a pixel one after the other, in frame order, so that the running mean is the one S single
    // frames would have left (each frame with its own accumCount)
    // (one bounce: the pixel's running value stays in registers from the first frame of the set to the last, resolve -4 %:
    //  profiles/r03/resolve_registers.txt; the level-by-level form reads and writes it frame by frame)
    const size_t pixel = (size_t)py * pd.width + px;
    const bool progressive = pd.kind != RT_PIPELINE_REALTIME;
    constexpr bool KEEP = BATCH && !FLAT;
    float4 acc = KEEP && progressive ? pd.accum[pixel] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // (KEEP: the two registers of `pixel` are not carried through the frames -- the store behind them works the index out again from the
    //  thread's slot, through a register the optimiser cannot see through, or it would keep the first computation alive)
    auto pixel_again = [&]() -> size_t {
        uint32_t slot = blockIdx.x * PBLOCK + threadIdx.x, x, y;
        asm volatile("" : "+v"(slot));
        (void)pix_xy(pd, slot, x, y);
        return (size_t)y * pd.width + x;
    };
    for (uint32_t f = 0; f < (BATCH ? pd.n_frames : 1u); f++) {
        const rt_per_frame_constants &fc = BATCH ? pfcs[f] : pd.pfc;
        const uint32_t q = frame_slot(pd, f, ql);
        const RayD r = primary_ray(pd, fc.cameraParams, px, py);
        const float4 h = pd.lv[0].hit[q];
        Shaded sh;
        if (h.x == HIT_MISS) {
            sh.color = sample_environment(pd, fc, r.d);         // PrimaryMiss
            sh.aov_direct = sh.color;                           // RealtimeRaytracing.hlsl:119-126
            sh.aov_indirect = mk3(0.0f, 0.0f, 0.0f);
        } else if (FLAT) {
            LevelResolveIO io(pd, fc, 0, pd.lv[0].slot_j[q]);
            sh = closest_hit_aov(pd, fc, io, r, h.x, h.y, h.z, __float_as_uint(h.w), pd.lv[0].inst[q], 0u, px + py * pd.width);
        } else {
            ResolveIO<0, 1> io(pd, fc, pd.lv[0].slot_j[q], px + py * pd.width);
            sh = closest_hit_aov(pd, fc, io, r, h.x, h.y, h.z, __float_as_uint(h.w), pd.lv[0].inst[q], 0u, px + py * pd.width);
        }
        if (progressive) { acc = accumulate(pd, fc, KEEP ? acc : pd.accum[pixel], sh); if (!KEEP) pd.accum[pixel] = acc; }
        else write_aovs(pd, KEEP ? pixel_again() : pixel, sh);
    }
    if (KEEP && progressive) pd.accum[pixel_again()] = acc;
}

// deep paths: the colour of every hit of level L >= 1 (its shadow rays are traced, the hits of level L + 1 already shaded)
template <bool BATCH, int LC>
RT_DEV void shade_level_body(const PipeDev &pd, int level)
{
    const int L = LC >= 0 ? LC : level;
    const uint32_t idx = blockIdx.x * PBLOCK + threadIdx.x;
    if (idx >= pd.counters[C_NHIT + L]) return;
    const uint32_t slot = pd.lv[L].jlist[idx];
    const uint32_t q = pd.lv[L].pix[slot];
    uint32_t px, py, ql = q;
    rt_per_frame_constants own;
    if (BATCH) own = pd.pfcs[slot_frame(pd, q, ql)];
    const rt_per_frame_constants &fc = BATCH ? own : pd.pfc;
    (void)pix_xy(pd, ql, px, py);
    const RayD r = load_ray(pd.lv[L].O, pd.lv[L].D, slot);
    const float4 h = pd.lv[L].hit[slot];
    LevelResolveIO io(pd, fc, L, idx);
    const f3 c = closest_hit(pd, fc, io, r, h.x, h.y, h.z, __float_as_uint(h.w), pd.lv[L].inst[slot], (uint32_t)L, px + py * pd.width);
    pd.lv[L].color[slot] = make_float4(c.x, c.y, c.z, 0.0f);
}
template <bool BATCH>
__global__ void __launch_bounds__(PBLOCK) k_shade_level(PipeDev pd, int L)
{
    if (!BATCH) shade_level_body<BATCH, -1>(pd, L);
    else if (L == 1) shade_level_body<BATCH, 1>(pd, L);
    else if (L == 2) shade_level_body<BATCH, 2>(pd, L);
    else if (L == 3) shade_level_body<BATCH, 3>(pd, L);
    else shade_level_body<BATCH, MAXD>(pd, L);
}

// The launches of one frame (BATCH = false), or of one set of frames: the shading kernels then pick the constants of every hit's frame.
// plan.counted: the levels beyond the pixel slots are sized by what the compaction before them has counted ("queue memory",
// rt_pipeline_queues.h); otherwise the caller has reserved the worst case and set the strides.  pd is updated as the levels are bound
// and is what the counting passes replay (rt_pipeline::last_pd, rt_pipeline_inspect.hip).
template <int STACK, bool TWO_LEVEL, bool BATCH>
int launch_frame(rt_pipeline *p, PipeDev &pd, const SetPlan &plan)
{
    hipError_t first_error = hipSuccess;
    auto record = [&](hipEvent_t e, hipStream_t s) { const hipError_t rc = hipEventRecord(e, s); if (first_error == hipSuccess) first_error = rc; };
    hipStream_t st = p->ctx->stream;
    const bool T = p->ring_frames > 0;
    const size_t ring_slot = T ? (size_t)(p->ring_pos % (uint64_t)p->ring_frames) : 0;
    hipEvent_t *ev = T ? &p->ring[ring_slot * EV_COUNT] : nullptr;
    const uint32_t cap = pd.cap;
    rt_context *ctx = p->ctx;
    const uint32_t levels = plan.levels;
    const bool deep = levels > 1, counted = plan.counted;
    // counted queues: the hits the compaction of level l has just produced -> the shadow queue of level l and the ray queue of
    // level l + 1 get their sizes; `slots` = ray slots of the level whose launches come next (level 1: two batches)
    size_t hits_l = cap, slots = cap;
    size_t sh_total = 0;                        // entries of the shared shadow queue taken by the levels sized so far
    auto size_next = [&](uint32_t l, bool casts_shadows, bool spawns) -> int {
        if (counted) {
            HIP_TRY(hipMemcpyAsync(ctx->pinned, &pd.counters[C_NHIT + l], 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            hits_l = round64((size_t)ctx->pinned[0]);
            if (hits_l == 0) hits_l = 64;
        } else hits_l = l == 0 ? (size_t)cap : 2 * (size_t)cap;
        if (hits_l > 0xffffffc0ull / 2) { rt_set_error("render: more than 2^31 hits at radiance level %u", l); return RT_ERR_UNSUPPORTED; }
        pd.lv[l].hstride = (uint32_t)hits_l;
        if (casts_shadows) {
            if (((sh_total + hits_l) << plan.sh_log2) >= 0xffffffc0ull) { rt_set_error("render: more than 2^32 shadow rays in one set of launches"); return RT_ERR_UNSUPPORTED; }
            if (counted) RT_TRY(reserve_shadows(p, sh_total + hits_l, plan.sh_log2, plan.compact, sh_total));
            pd.sh_cbase[l] = (uint32_t)sh_total;
            sh_total += hits_l;
        }
        bind_level(p, pd, (int)l);
        if (spawns) {
            slots = (l == 0 ? 2 : 1) * hits_l;
            if (l == 0) pd.lv[1].rstride = (uint32_t)hits_l;
            if (counted) RT_TRY(reserve_level_rays(p, l + 1, slots, deep));
            bind_level(p, pd, (int)l + 1);
        }
        return RT_OK;
    };
    if (T) record(ev[0], st);
    if (pd.primary_persistent) {
        HIP_TRY(hipMemsetAsync(pd.pools + POOL_BYTES / 4, 0, PRIMARY_POOL_WORDS * 4, st));      // (its own first block cannot clear it: the others already draw from it)
        k_primary<STACK, TWO_LEVEL, BATCH, true><<<rt_persistent_grid(ctx, k_primary<STACK, TWO_LEVEL, BATCH, true>, PBLOCK, cap), PBLOCK, 0, st>>>(pd);
    } else {
        // primary rays are coherent: one 8x8 tile per wave, scheduled by the hardware dispatcher -- from the tile's entry list, made here
        // once for the frames of the set (inside the stage's time), or from the root
        bool from_entries = false;
        if constexpr (!TWO_LEVEL) {
            if (p->primary_entries.on) {
                const uint2 *lists = rt_entries_launch(p, pd);
                k_primary_from_entries<STACK, BATCH><<<blocks(cap), PBLOCK, 0, st>>>(pd, lists, recip32(pd.n_frames), recip32(pd.tiles_x));
                from_entries = true;
            }
        }
        if (!from_entries) k_primary<STACK, TWO_LEVEL, BATCH, false><<<blocks(cap), PBLOCK, 0, st>>>(pd);
        // the rays that would have needed a stack row beyond LDS (none on the bench scenes: the launch returns at once)
        if (pd.retry) k_primary_retry<STACK, TWO_LEVEL><<<rt_persistent_grid(ctx, k_primary_retry<STACK, TWO_LEVEL>, PBLOCK, cap), PBLOCK, 0, st>>>(pd);
    }
    k_compact_level<<<(cap + CTILES * CBLOCK - 1) / (CTILES * CBLOCK), CBLOCK, 0, st>>>(pd, 0);
    if (T) record(ev[1], st);
    RT_TRY(size_next(0, true, levels >= 1));
    k_shade_emit<true, BATCH><<<blocks(hits_l), PBLOCK, 0, st>>>(pd, 0, plan.shadow_slots, levels >= 1 ? 1u : 0u);
    if (T) record(ev[2], st);
    for (uint32_t l = 1; l <= levels; l++) {
        const QueueSrc rays = level_rays(pd, l);
        k_trace_secondary<STACK, TWO_LEVEL><<<rt_persistent_grid(ctx, k_trace_secondary<STACK, TWO_LEVEL>, PBLOCK, slots), PBLOCK, 0, st>>>(
            pd.sc, rays, pd.lv[l].hit, pd.lv[l].inst, pd.pools + (size_t)l * RT_POOL_GROUPS * RT_POOL_STRIDE, &pd.counters[C_SECONDARY]);
        k_compact_level<<<(unsigned)((slots + CTILES * CBLOCK - 1) / (CTILES * CBLOCK)), CBLOCK, 0, st>>>(pd, (int)l);
        if (T) record(ev[3 + 2 * (l - 1)], st);
        const bool casts_shadows = l < pd.sh_levels, spawns = l < levels;
        RT_TRY(size_next(l, casts_shadows, spawns));
        if (casts_shadows || spawns) k_shade_emit<false, BATCH><<<blocks(hits_l), PBLOCK, 0, st>>>(pd, (int)l, 2u, spawns ? 1u : 0u);
        if (T) record(ev[4 + 2 * (l - 1)], st);
    }
    {   // every shadow ray of the frame (or set) in ONE persistent any-hit launch over the shared queue
        ShadowQueue sq = shadow_queue(pd, 0, pd.sh_levels);
        sq.cache = p->shadow_cache.dev;
        sq.cache.jlist0 = pd.lv[0].jlist;
        sq.cache.hstride0 = pd.lv[0].hstride;
        sq.cache.n_frames = pd.n_frames;
        sq.cache.frames_magic = recip32(pd.n_frames);
        if (sq.cache.px_slots > pd.fcap) sq.cache.px_slots = pd.fcap;
        const size_t rays_max = sh_total << pd.sh_log2;
        HIP_TRY(hipMemsetAsync(pd.sh_vis, 0, ((rays_max + 31) / 32) * 4, st));      // the visibility bits: set by the rays that reach their light
        k_trace_shadow<STACK, TWO_LEVEL, BATCH><<<rt_persistent_grid(ctx, k_trace_shadow<STACK, TWO_LEVEL, BATCH>, PBLOCK, rays_max), PBLOCK, 0, st>>>(
            pd.sc, sq, pd.pools, &pd.counters[C_SHADOW]);
    }
    if (T) record(ev[EV_SHADOW], st);
    // (resolve: one thread per pixel slot of ONE frame; a batch's frames are accumulated in order inside the thread)
    if (levels <= 1) k_resolve<false, BATCH><<<blocks(pd.fcap), PBLOCK, 0, st>>>(pd, pd.pfcs);      // (level by level is slower here: 0.143 vs 0.118 ms at 1080p)
    else {
        for (uint32_t l = levels; l >= 1; l--) k_shade_level<BATCH><<<blocks(pd.lv[l].hstride), PBLOCK, 0, st>>>(pd, (int)l);      // (one thread per hit of the level)
        k_resolve<true, BATCH><<<blocks(pd.fcap), PBLOCK, 0, st>>>(pd, pd.pfcs);
    }
    if (T) { record(ev[EV_RESOLVE], st); p->ring_levels[ring_slot] = (uint8_t)levels; p->ring_nframes[ring_slot] = (uint8_t)pd.n_frames; p->ring_pos++; }
    HIP_TRY(first_error);
    return RT_OK;
}

template <int STACK, bool TWO_LEVEL>
int launch_frame_sized(rt_pipeline *p, PipeDev &pd, const SetPlan &plan)
{
    return pd.n_frames > 1u ? launch_frame<STACK, TWO_LEVEL, true>(p, pd, plan) : launch_frame<STACK, TWO_LEVEL, false>(p, pd, plan);
}
// (+ RT_STACK_REFS: the instantiations that look references up, for scenes that hold split triangles)
template <int STACK>
int launch_frame_any(rt_pipeline *p, PipeDev &pd, const SetPlan &plan)
{
    if (p->scene->has_refs) return p->scene->two_level ? launch_frame_sized<STACK + RT_STACK_REFS, true>(p, pd, plan) : launch_frame_sized<STACK + RT_STACK_REFS, false>(p, pd, plan);
    return p->scene->two_level ? launch_frame_sized<STACK, true>(p, pd, plan) : launch_frame_sized<STACK, false>(p, pd, plan);
}

}  // namespace

int rt_frame_launch(rt_pipeline *p, PipeDev &pd, const SetPlan &plan, bool set_rows)
{
    // 18 LDS stack rows + the 8-row top table = 26 KiB per 256-thread block = 6 resident blocks per CU, whatever
    // the depth of the tree; the rare deeper walk continues in global rows (rt_trace_wave.h)
    if (p->ctx->lds_stack_rows == RT_LDS_STACK_ROWS_TEST) return launch_frame_any<RT_LDS_STACK_ROWS_TEST>(p, pd, plan);
    // (scene_for_set never asks for the sets' rows on a scene with split triangles: there the 18-row six-wave kernels are the faster ones --
    // 2.2 M-triangle stress scene 5.63 -> 4.89 ms per frame, 272 k 4.88 -> 4.86: profiles/r05/ref_rule.txt -- and the reference-aware
    // seven-wave instantiations, which spilled 36 - 72 B, are not compiled)
    if (set_rows) return launch_frame_sized<RT_LDS_STACK_ROWS_SETS, false>(p, pd, plan);
    return launch_frame_any<RT_LDS_STACK_ROWS>(p, pd, plan);
}
