/*
 * harness.cpp -- TEST INFRASTRUCTURE ONLY (oracle/refshade): the DXR machinery that the reference's shading text calls into.
 *
 * The text itself is included below from oracle/_ref/gen/ (translate.py's output, never committed) and runs as written.  What this
 * file adds is what the D3D12 runtime and the reference's host code provide around it:
 *
 *   - the system values (DispatchRaysIndex, WorldRayOrigin, RayTCurrent, PrimitiveIndex, ...), one ray state per TraceRay nesting level;
 *   - the shader table, as the reference's pipelines set it up:
 *       hit group 0 = PrimaryClosestHit, miss 0 = PrimaryMiss     src/ProgressiveRaytracingPipeline.cpp:38, src/RealtimeRaytracingPipeline.cpp:37
 *       hit group 1 = ShadowClosestHit + ShadowAnyHit, miss 1 = ShadowMiss            ...Pipeline.cpp:39,                        ...:38
 *       one hit record per (instance, ray type), record = instance * hitProgramCount + ray type
 *                                                                  libs/DXRFramework/RtScene.cpp:29, RtBindings.cpp:158-164
 *       record (instance, ray type) binds that instance's vertex buffer, index buffer and mMaterials[instance]
 *                                                                  src/ProgressiveRaytracingPipeline.cpp:220-227, src/RealtimeRaytracingPipeline.cpp:206-213
 *       payload sizes 20 and 60 bytes                              src/ProgressiveRaytracingPipeline.cpp:72, src/RealtimeRaytracingPipeline.cpp:71
 *   - TraceRay: the hit is found by the oracle's tracer (orc_trace; its semantics have their own truth test), then the closest-hit
 *     shader of record  RayContributionToHitGroupIndex + multiplier * geometry index (0) + instance * hitProgramCount  runs, or the
 *     miss shader MissShaderIndex; RAY_FLAG_SKIP_CLOSEST_HIT_SHADER is honoured.  ShadowAnyHit is a no-op in the text and is not run;
 *   - the resources: gOutput as an fp32 image or one stored as RGBA16F (orc_round_to_half), the cube map (orc_sample_cube).
 *
 * Single-threaded: the state below is global.
 */
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../oracle.h"
#include "hlsl_shim.h"

namespace hlsl {

/* ---- state behind the system values ---- */

struct RayState { float3 origin, direction; float t; uint prim; };
static RayState g_ray;
static uint3 g_index, g_dims;

uint3 DispatchRaysIndex() { return g_index; }
uint3 DispatchRaysDimensions() { return g_dims; }
float3 WorldRayOrigin() { return g_ray.origin; }
float3 WorldRayDirection() { return g_ray.direction; }
float RayTCurrent() { return g_ray.t; }
uint PrimitiveIndex() { return g_ray.prim; }

}  // namespace hlsl

/* ---- the reference's text ---- */

namespace hlsl {
#include "RaytracingCommon.h"
#include "shim_selftest.h"
namespace progressive {
#include "ProgressiveRaytracing.h"
}
namespace realtime {
#include "RealtimeRaytracing.h"
}
}  // namespace hlsl

namespace hlsl {

static_assert(sizeof(progressive::SimplePayload) == 20, "setMaxPayloadSize(20), src/ProgressiveRaytracingPipeline.cpp:72");
static_assert(sizeof(realtime::RealtimePayload) == 60, "setMaxPayloadSize(60), src/RealtimeRaytracingPipeline.cpp:71");

/* ---- shader table ---- */

enum { HIT_PROGRAM_COUNT = 2, MISS_PROGRAM_COUNT = 2 };
typedef void (*ClosestHitFn)(void *payload, Attributes attrib);
typedef void (*MissFn)(void *payload);

struct HitRecord {                       /* program + local root arguments */
    ClosestHitFn closestHit;
    const rt_vertex *vertices;
    const uint32_t *indices;
    MaterialParams material;
};

struct Pipeline {
    void (*rayGen)();
    ClosestHitFn hitGroup[HIT_PROGRAM_COUNT];
    MissFn miss[MISS_PROGRAM_COUNT];
};

static const Pipeline PROGRESSIVE = {
    [] { progressive::RayGen(); },
    { [](void *p, Attributes a) { progressive::PrimaryClosestHit(*(progressive::SimplePayload *)p, a); },      /* addHitGroup(0, ...) */
      [](void *p, Attributes a) { progressive::ShadowClosestHit(*(ShadowPayload *)p, a); } },                  /* addHitGroup(1, ...) */
    { [](void *p) { progressive::PrimaryMiss(*(progressive::SimplePayload *)p); },                             /* addMiss(0, ...) */
      [](void *p) { progressive::ShadowMiss(*(ShadowPayload *)p); } },                                         /* addMiss(1, ...) */
};

static const Pipeline REALTIME = {
    [] { realtime::RayGen(); },
    { [](void *p, Attributes a) { realtime::PrimaryClosestHit(*(realtime::RealtimePayload *)p, a); },
      [](void *p, Attributes a) { realtime::ShadowClosestHit(*(ShadowPayload *)p, a); } },
    { [](void *p) { realtime::PrimaryMiss(*(realtime::RealtimePayload *)p); },
      [](void *p) { realtime::ShadowMiss(*(ShadowPayload *)p); } },
};

struct Launch {
    const orc_scene *scene;
    int trace_mode;                      /* orc_trace: 1 = BVH traversal, 0 = the brute-force loop */
    const Pipeline *pipeline;
    std::vector<HitRecord> hitRecords;   /* [instance * HIT_PROGRAM_COUNT + ray type] */
    int depth;                           /* TraceRay nesting level: 0 while RayGen's own ray is in flight */
    orc_render_stats stats;
};
static Launch g_launch;

void trace_ray(uint flags, uint, uint rayContribution, uint geometryMultiplier, uint missShaderIndex, const RayDesc &ray, void *payload)
{
    const float o[4] = {ray.Origin.x, ray.Origin.y, ray.Origin.z, ray.TMin};
    const float d[4] = {ray.Direction.x, ray.Direction.y, ray.Direction.z, ray.TMax};
    float t = 0.0f, u = 0.0f, v = 0.0f;
    uint32_t prim = 0, inst = RT_NO_HIT;
    if (orc_trace(g_launch.scene, o, d, 1, flags, g_launch.trace_mode, &t, &u, &v, &prim, &inst, NULL, NULL, 1) != 0) abort();
    const bool hit = inst != RT_NO_HIT;
    orc_render_stats &st = g_launch.stats;
    if (rayContribution == 1) st.rays_shadow++;
    else if (g_launch.depth == 0) { st.rays_primary++; if (hit) { st.primary_hits++; st.shaded_hits++; } }
    else { st.rays_secondary++; if (hit) { st.secondary_hits++; st.shaded_hits++; } }

    /* the callee's system values and local root arguments; the caller's come back when it returns */
    const RayState savedRay = g_ray;
    const Buffer<float3> savedVertexBuffer = vertexBuffer;
    const ByteAddressBuffer savedIndexBuffer = indexBuffer;
    const MaterialParams savedMaterial = materialParams;
    g_ray.origin = ray.Origin;
    g_ray.direction = ray.Direction;
    g_launch.depth++;
    if (!hit) {
        if (missShaderIndex >= MISS_PROGRAM_COUNT) abort();
        g_launch.pipeline->miss[missShaderIndex](payload);
    } else if (!(flags & RAY_FLAG_SKIP_CLOSEST_HIT_SHADER)) {
        const size_t record = (size_t)rayContribution + (size_t)geometryMultiplier * 0u + (size_t)inst * HIT_PROGRAM_COUNT;
        if (record >= g_launch.hitRecords.size()) abort();
        const HitRecord &r = g_launch.hitRecords[record];
        vertexBuffer.data = &r.vertices[0].position.x;
        indexBuffer.bytes = (const uint8_t *)r.indices;
        materialParams = r.material;
        g_ray.t = t;
        g_ray.prim = prim;
        Attributes attrib;
        attrib.bary = float2{u, v};
        r.closestHit(payload, attrib);
    }
    g_launch.depth--;
    g_ray = savedRay;
    vertexBuffer = savedVertexBuffer;
    indexBuffer = savedIndexBuffer;
    materialParams = savedMaterial;
}

/* ---- resources ---- */

float4 TextureCube::SampleLevel(SamplerState, float3 dir, float) const
{
    if (!faces) return float4{constant[0], constant[1], constant[2], 1.0f};
    const float din[3] = {dir.x, dir.y, dir.z};
    float out[3];
    orc_sample_cube(faces, size, din, out, 1);
    return float4{out[0], out[1], out[2], 1.0f};
}

template <> void RWTexture2D<float4>::store(uint2 at, float4 v) const
{
    float px[4] = {v.x, v.y, v.z, v.w};
    if (f16) { float r[4]; orc_round_to_half(px, r, 4, f16 == 1); memcpy(px, r, sizeof px); }
    memcpy(texels + ((size_t)at.y * width + at.x) * 4, px, sizeof px);
}

/* ---- one DispatchRays ---- */

static int launch(const Pipeline &pipeline, const orc_scene *sc, const rt_material_params *mats, uint32_t nmats,
                  const float *env_faces, int env_size, const float env_constant[3], const rt_per_frame_constants *pfc,
                  uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, int trace_mode,
                  orc_render_stats *stats_out)
{
    static_assert(sizeof(PerFrameConstants) == sizeof(rt_per_frame_constants) && sizeof(MaterialParams) == sizeof(rt_material_params), "records");
    uint32_t ninst = 0;
    orc_scene_instance_geometry(sc, 0, NULL, NULL, NULL, NULL, &ninst);
    if (ninst == 0 || nmats < ninst) return -1;             /* mMaterials[instance]: one material per instance */
    g_launch.scene = sc;
    g_launch.trace_mode = trace_mode;
    g_launch.pipeline = &pipeline;
    g_launch.depth = 0;
    memset(&g_launch.stats, 0, sizeof g_launch.stats);
    g_launch.hitRecords.clear();
    for (uint32_t inst = 0; inst < ninst; inst++)
        for (int rayType = 0; rayType < HIT_PROGRAM_COUNT; rayType++) {
            HitRecord r;
            r.closestHit = pipeline.hitGroup[rayType];
            if (orc_scene_instance_geometry(sc, inst, &r.vertices, NULL, &r.indices, NULL, NULL) != 0) return -1;
            memcpy((void *)&r.material, &mats[inst], sizeof r.material);
            g_launch.hitRecords.push_back(r);
        }
    memcpy((void *)static_cast<PerFrameConstants *>(&perFrameConstants), pfc, sizeof(PerFrameConstants));
    envCubemap.faces = env_faces;
    envCubemap.size = env_size;
    for (int k = 0; k < 3; k++) envCubemap.constant[k] = env_constant ? env_constant[k] : 0.0f;
    g_dims = uint3{width, height, 1};
    if (x1 > width) x1 = width;
    if (y1 > height) y1 = height;
    for (uint32_t y = y0; y < y1; y++)
        for (uint32_t x = x0; x < x1; x++) {
            g_index = uint3{x, y, 0};
            pipeline.rayGen();
        }
    if (stats_out) *stats_out = g_launch.stats;
    return 0;
}

}  // namespace hlsl

using namespace hlsl;

extern "C" {

/* ---- unit entry points: the text's own functions over arrays ---- */

/* seed = initRand(v0, v1); rand = nextRand(seed) (state = the seed after the draw) */
void ref_rng_batch(const uint32_t *v0, const uint32_t *v1, uint32_t *seed, uint32_t *state, float *rand, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        uint s = initRand(v0[i], v1[i]);
        seed[i] = s;
        rand[i] = nextRand(s);
        state[i] = s;
    }
}

/* kinds as ORC_SAMPLE_*; same arguments as orc_sample_batch */
void ref_sample_batch(int kind, const uint32_t *seeds, const float *vec3_in, float exponent,
                      float *vec3_out, float *pdf_brdf, uint32_t *seeds_out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        uint s = seeds[i];
        const float3 in = float3{vec3_in[3 * i], vec3_in[3 * i + 1], vec3_in[3 * i + 2]};
        float3 o;
        float pdf = 0.0f, brdf = 0.0f;
        switch (kind) {
        case ORC_SAMPLE_COS:     o = getCosHemisphereSample(s, in); break;
        case ORC_SAMPLE_UNIFORM: o = getUniformHemisphereSample(s, in); break;
        case ORC_SAMPLE_PHONG:   o = samplePhongLobe(s, in, exponent, pdf, brdf); break;
        case ORC_SAMPLE_PERP:    o = getPerpendicularVector(in); break;
        default: break;
        }
        vec3_out[3 * i] = o.x; vec3_out[3 * i + 1] = o.y; vec3_out[3 * i + 2] = o.z;
        if (pdf_brdf) { pdf_brdf[2 * i] = pdf; pdf_brdf[2 * i + 1] = brdf; }
        if (seeds_out) seeds_out[i] = s;
    }
}

void ref_fresnel_batch(const float *I, const float *N, const float *f0, float *out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        const float3 r = FresnelReflectanceSchlick(float3{I[3 * i], I[3 * i + 1], I[3 * i + 2]}, float3{N[3 * i], N[3 * i + 1], N[3 * i + 2]},
                                                   float3{f0[3 * i], f0[3 * i + 1], f0[3 * i + 2]});
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
    }
}

/* the exponent the text derives from a roughness (shade(): exp((1.0 - roughness) * 12.0)) */
float ref_phong_exponent(float roughness) { return hlsl::exp((1.0f - roughness) * 12.0f); }

/* ---- the shim's self-tests (translate.py SELFTEST) ---- */

void ref_selftest_two_draws(uint32_t *seed, float out[2])
{
    uint s = *seed;
    const float2 r = shimTwoDraws(s);
    *seed = s;
    out[0] = r.x; out[1] = r.y;
}

float ref_selftest_float_only(float x) { return shimFloatOnly(x); }

/* rows of { size or offset in the translated compat header (HLSL defined), the same in include/dxr_amd_types.h }; returns the row count */
int ref_layout(uint32_t *rows, int max_rows)
{
    std::vector<uint32_t> t;
#define SIZE_ROW(H, R) do { t.push_back((uint32_t)sizeof(H)); t.push_back((uint32_t)sizeof(R)); } while (0)
#define FIELD_ROW(H, R, f) do { t.push_back((uint32_t)offsetof(H, f)); t.push_back((uint32_t)offsetof(R, f)); \
                                t.push_back((uint32_t)sizeof(((H *)0)->f)); t.push_back((uint32_t)sizeof(((R *)0)->f)); } while (0)
    struct rt_shadow_payload { float lightVisibility; };           /* no record in dxr_amd_types.h: stated here */
    struct rt_attributes { rt_float2 bary; };
    SIZE_ROW(ShadowPayload, rt_shadow_payload); FIELD_ROW(ShadowPayload, rt_shadow_payload, lightVisibility);
    SIZE_ROW(Attributes, rt_attributes); FIELD_ROW(Attributes, rt_attributes, bary);
    SIZE_ROW(Vertex, rt_vertex); FIELD_ROW(Vertex, rt_vertex, position); FIELD_ROW(Vertex, rt_vertex, normal);
    SIZE_ROW(CameraParams, rt_camera_params);
    FIELD_ROW(CameraParams, rt_camera_params, worldEyePos); FIELD_ROW(CameraParams, rt_camera_params, U);
    FIELD_ROW(CameraParams, rt_camera_params, V); FIELD_ROW(CameraParams, rt_camera_params, W);
    FIELD_ROW(CameraParams, rt_camera_params, jitters); FIELD_ROW(CameraParams, rt_camera_params, frameCount);
    FIELD_ROW(CameraParams, rt_camera_params, accumCount);
    SIZE_ROW(DirectionalLightParams, rt_directional_light_params);
    FIELD_ROW(DirectionalLightParams, rt_directional_light_params, forwardDir); FIELD_ROW(DirectionalLightParams, rt_directional_light_params, color);
    SIZE_ROW(PointLightParams, rt_point_light_params);
    FIELD_ROW(PointLightParams, rt_point_light_params, worldPos); FIELD_ROW(PointLightParams, rt_point_light_params, color);
    SIZE_ROW(DebugOptions, rt_debug_options);
    FIELD_ROW(DebugOptions, rt_debug_options, maxIterations); FIELD_ROW(DebugOptions, rt_debug_options, cosineHemisphereSampling);
    FIELD_ROW(DebugOptions, rt_debug_options, showIndirectDiffuseOnly); FIELD_ROW(DebugOptions, rt_debug_options, showIndirectSpecularOnly);
    FIELD_ROW(DebugOptions, rt_debug_options, showAmbientOcclusionOnly); FIELD_ROW(DebugOptions, rt_debug_options, showGBufferAlbedoOnly);
    FIELD_ROW(DebugOptions, rt_debug_options, showDirectLightingOnly); FIELD_ROW(DebugOptions, rt_debug_options, showFresnelTerm);
    FIELD_ROW(DebugOptions, rt_debug_options, noIndirectDiffuse); FIELD_ROW(DebugOptions, rt_debug_options, environmentStrength);
    FIELD_ROW(DebugOptions, rt_debug_options, debug);
    SIZE_ROW(PerFrameConstants, rt_per_frame_constants);
    FIELD_ROW(PerFrameConstants, rt_per_frame_constants, cameraParams); FIELD_ROW(PerFrameConstants, rt_per_frame_constants, directionalLight);
    FIELD_ROW(PerFrameConstants, rt_per_frame_constants, pointLight); FIELD_ROW(PerFrameConstants, rt_per_frame_constants, options);
    SIZE_ROW(MaterialParams, rt_material_params);
    FIELD_ROW(MaterialParams, rt_material_params, albedo); FIELD_ROW(MaterialParams, rt_material_params, specular);
    FIELD_ROW(MaterialParams, rt_material_params, emissive); FIELD_ROW(MaterialParams, rt_material_params, reflectivity);
    FIELD_ROW(MaterialParams, rt_material_params, roughness); FIELD_ROW(MaterialParams, rt_material_params, IoR);
    FIELD_ROW(MaterialParams, rt_material_params, type);
#undef SIZE_ROW
#undef FIELD_ROW
    const int n = (int)(t.size() / 2);
    for (int i = 0; i < n && i < max_rows; i++) { rows[2 * i] = t[2 * i]; rows[2 * i + 1] = t[2 * i + 1]; }
    return n;
}

/* ---- frames ---- */

/* One ProgressiveRaytracing.hlsl DispatchRays over the pixels [x0, x1) x [y0, y1) of a width x height launch; the arguments of
 * orc_render without its depth overrides (the text compiles MAX_RADIANCE_RAY_DEPTH 1 and MAX_SHADOW_RAY_DEPTH 2 in).
 * accum_mode: RT_ACCUM_RUNNING_MEAN only (the text has no other); bits 8-9 = gOutput is stored as RGBA16F, 1: rounded to nearest even,
 * 2: toward zero.  use_brute: 0 / 1 as orc_render.  nthreads is ignored.  stats: ray and hit counts (nodes, tris = 0). */
int ref_render_progressive(const orc_scene *s, const rt_material_params *mats, uint32_t nmats,
                           const float *env_faces, int env_size, const float env_constant[3],
                           const rt_per_frame_constants *pfc, uint32_t width, uint32_t height,
                           uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                           uint32_t accum_mode, int use_brute, float *accum, int nthreads, orc_render_stats *stats)
{
    (void)nthreads;
    if ((accum_mode & 0xFFu) != RT_ACCUM_RUNNING_MEAN || (accum_mode >> 10) != 0 || ((accum_mode >> 8) & 3u) == 3u) return -1;
    if (use_brute != 0 && use_brute != 1) return -1;
    progressive::gOutput.texels = accum;
    progressive::gOutput.width = width;
    progressive::gOutput.f16 = (int)((accum_mode >> 8) & 3u);
    return launch(PROGRESSIVE, s, mats, nmats, env_faces, env_size, env_constant, pfc, width, height, x0, y0, x1, y1, use_brute ? 0 : 1, stats);
}

/* One RealtimeRaytracing.hlsl DispatchRays; the arguments of orc_render_realtime without its depth overrides. */
int ref_render_realtime(const orc_scene *s, const rt_material_params *mats, uint32_t nmats,
                        const float *env_faces, int env_size, const float env_constant[3],
                        const rt_per_frame_constants *pfc, uint32_t width, uint32_t height,
                        float *direct, float *indirect, int nthreads, orc_render_stats *stats)
{
    (void)nthreads;
    realtime::gDirectLightingOutput.texels = direct;
    realtime::gDirectLightingOutput.width = width;
    realtime::gDirectLightingOutput.f16 = 0;
    realtime::gIndirectSpecularOutput.texels = indirect;
    realtime::gIndirectSpecularOutput.width = width;
    realtime::gIndirectSpecularOutput.f16 = 0;
    return launch(REALTIME, s, mats, nmats, env_faces, env_size, env_constant, pfc, width, height, 0, 0, width, height, 1, stats);
}

}  // extern "C"
