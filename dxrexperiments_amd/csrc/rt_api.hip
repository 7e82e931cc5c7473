// rt_api.hip -- C-ABI entry points for context, model, scene and batch TraceRay
// (include/dxr_amd.h).  Stand-ins for libs/DXRFramework/Rt{Context,Model,Scene}.
#include <cmath>
#include <cstring>
#include <new>

#include "rt_adjacency.h"
#include "rt_morph.h"
#include "rt_skin.h"
#include "rt_trace_device.h"

static thread_local std::string g_last_error;

void rt_set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

size_t &rt_alloc_limit_ref()
{
    static size_t limit = ~(size_t)0;
    return limit;
}

extern "C" int rt_debug_set_alloc_limit(size_t bytes)
{
    rt_alloc_limit_ref() = bytes ? bytes : ~(size_t)0;
    return RT_OK;
}

namespace {

using namespace rtd;

// ---- device math probes ------------------------------------------------------

__global__ void k_debug_math(int fn, const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s, c, r = 0.0f;
    switch (fn) {
    case 0: sincos_det(x[i], s, c); r = s; break;
    case 1: sincos_det(x[i], s, c); r = c; break;
    case 2: r = exp_det(x[i]); break;
    case 3: r = log_det(x[i]); break;
    case 4: r = pow_det(x[i], y[i]); break;
    case 5: r = __builtin_sqrtf(x[i]); break;
    case 6: r = x[i] / y[i]; break;
    case 7: r = fmin2(x[i], y[i]); break;
    case 8: r = fmax2(x[i], y[i]); break;
    default: break;
    }
    out[i] = r;
}

__global__ void k_debug_sample(int kind, const uint32_t *__restrict__ seeds, const float *__restrict__ vin, float exponent,
                               float *__restrict__ vout, float *__restrict__ pdf_brdf, uint32_t *__restrict__ seeds_out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s = seeds[i];
    const f3 in = mk3(vin[3 * i], vin[3 * i + 1], vin[3 * i + 2]);
    f3 o = mk3(0.0f, 0.0f, 0.0f);
    float pdf = 0.0f, brdf = 0.0f;
    switch (kind) {
    case 0: o = cos_hemisphere(s, in); break;
    case 1: o = uniform_hemisphere(s, in); break;
    case 2: o = phong_lobe(s, in, exponent, pdf, brdf); break;
    case 3: o = perpendicular(in); break;
    default: break;
    }
    vout[3 * i] = o.x; vout[3 * i + 1] = o.y; vout[3 * i + 2] = o.z;
    if (pdf_brdf) { pdf_brdf[2 * i] = pdf; pdf_brdf[2 * i + 1] = brdf; }
    if (seeds_out) seeds_out[i] = s;
}

// ---- deforming meshes: new vertices for a model (rt_model_set_positions, rt_model_recompute_normals) ----

// count x 3 floats into the positions of the 24-byte vertex records first .. first + count - 1; the normals stay
__global__ void k_set_positions(rt_vertex *__restrict__ verts, uint32_t first, uint32_t count, const float *__restrict__ xyz)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    rt_float3 p;
    p.x = xyz[3 * (size_t)k]; p.y = xyz[3 * (size_t)k + 1]; p.z = xyz[3 * (size_t)k + 2];
    verts[(size_t)first + k].position = p;
}

// One lane per vertex: the sum of cross(p1 - p0, p2 - p0) over the triangles of its CSR run (rt_adjacency.h: ascending, each once), in that
// order, normalised; a sum whose squared length is 0, inf or NaN gives (0, 0, 0).  No atomics: the order of an fp32 sum is part of the result.
__global__ void k_vertex_normals(rt_vertex *__restrict__ verts, uint32_t n_verts, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ off,
                                 const uint32_t *__restrict__ tris)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_verts) return;
    f3 s = mk3(0.0f, 0.0f, 0.0f);
    for (uint32_t e = off[v]; e < off[v + 1]; e++) {
        const size_t t = tris[e];
        const rt_float3 a = verts[idx[3 * t]].position, b = verts[idx[3 * t + 1]].position, c = verts[idx[3 * t + 2]].position;
        const f3 p0 = mk3(a.x, a.y, a.z);
        s = s + cross(mk3(b.x, b.y, b.z) - p0, mk3(c.x, c.y, c.z) - p0);
    }
    const float d = dot(s, s);
    const f3 n = (d > 0.0f && d < __uint_as_float(0x7f800000u)) ? normalize(s) : mk3(0.0f, 0.0f, 0.0f);
    rt_float3 out;
    out.x = n.x; out.y = n.y; out.z = n.z;
    verts[v].normal = out;
}

// ---- skeletal animation: a model's vertices from its rest pose and a bone palette (rt_model_set_bones) ----

// One lane per vertex; a wave reads and writes 64 consecutive 24-byte records and, per slot, 64 consecutive indices and weights (the skin is
// slot major: rt_skin.h).  The 12 entries of the blended matrix are weight[0] * M[bone[0]], then + weight[k] * M[bone[k]] in slot order, every
// slot evaluated; position and normal as include/dxr_amd.h states them, no FMA.  K is a template parameter: the slot loop is unrolled and B
// lives in registers.  LDS: the palette (n_bones <= RT_SKIN_LDS_BONES) is copied into LDS by the whole block, coalesced, and gathered from
// there; else the lanes gather it from global memory.  The arithmetic is the same statements either way: the same bytes.
template <int K, bool LDS>
__global__ void __launch_bounds__(256) k_skin_vertices(rt_vertex *__restrict__ verts, const rt_vertex *__restrict__ rest, uint32_t n_verts,
                                                       const uint16_t *__restrict__ bone, const float *__restrict__ weight,
                                                       const float *__restrict__ palette, uint32_t n_bones)
{
    __shared__ float s_palette[LDS ? 12u * RT_SKIN_LDS_BONES : 1u];
    if (LDS) {
        for (uint32_t e = threadIdx.x; e < 12u * n_bones; e += 256u) s_palette[e] = palette[e];
        __syncthreads();
    }
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n_verts) return;
    const float *pal = LDS ? s_palette : palette;
    float B[12];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const size_t at = (size_t)k * n_verts + v;
        const float w = weight[at];
        const float *M = pal + 12u * (uint32_t)bone[at];
#pragma unroll
        for (int e = 0; e < 12; e++) {
            const float t = w * M[e];
            B[e] = k == 0 ? t : B[e] + t;
        }
    }
    const rt_vertex r = rest[v];
    const float x = r.position.x, y = r.position.y, z = r.position.z;
    rt_vertex o;
    o.position.x = ((B[0] * x + B[1] * y) + B[2] * z) + B[3];
    o.position.y = ((B[4] * x + B[5] * y) + B[6] * z) + B[7];
    o.position.z = ((B[8] * x + B[9] * y) + B[10] * z) + B[11];
    const float nx = r.normal.x, ny = r.normal.y, nz = r.normal.z;
    const f3 s = mk3((B[0] * nx + B[1] * ny) + B[2] * nz, (B[4] * nx + B[5] * ny) + B[6] * nz, (B[8] * nx + B[9] * ny) + B[10] * nz);
    const float d = dot(s, s);
    const f3 n = (d > 0.0f && d < __uint_as_float(0x7f800000u)) ? normalize(s) : mk3(0.0f, 0.0f, 0.0f);
    o.normal.x = n.x; o.normal.y = n.y; o.normal.z = n.z;
    verts[v] = o;
}

template <int K>
void launch_skin(hipStream_t st, bool lds, rt_vertex *verts, const rt_vertex *rest, uint32_t n_verts, const uint16_t *bone, const float *weight,
                 const float *palette, uint32_t n_bones)
{
    const uint32_t blocks = (n_verts + 255u) / 256u;
    if (lds) k_skin_vertices<K, true><<<blocks, 256, 0, st>>>(verts, rest, n_verts, bone, weight, palette, n_bones);
    else k_skin_vertices<K, false><<<blocks, 256, 0, st>>>(verts, rest, n_verts, bone, weight, palette, n_bones);
}

// ---- morph targets: a model's vertices from its base and a weight per target (rt_model_set_morph_weights) ----

// One lane per vertex, a block of 256 is four whole slices of the SELL-64 layout (rt_morph.h).  A lane walks its own `count` cells, 64 apart:
// at step j the lanes of a wave that still run read 64 consecutive 16-bit targets and 64 consecutive 12-byte deltas, and lanes whose run is
// shorter sit masked until the widest lane of the wave is through (the padding of a slice is never read).  The weights are gathered from
// global memory, 4 B per target and cache resident; no LDS staging -- the skin kernel's LDS palette was the slower path at its edge (DESIGN.md
// section 7, round 9), and nobody has measured this kernel with one.  The sums are include/dxr_amd.h's: p = p + (w * dp) per component in
// ascending target order, every entry evaluated, no FMA.  A vertex without entries is copied, all 24 bytes; without NORMALS so is every normal.
// `dst` is the model's vertices or its skin's rest pose (the host chooses); `base` is never either.
template <bool NORMALS>
__global__ void __launch_bounds__(256) k_morph_vertices(rt_vertex *__restrict__ dst, const rt_vertex *__restrict__ base, uint32_t n_verts,
                                                        const uint32_t *__restrict__ count, const uint32_t *__restrict__ slice_cell,
                                                        const uint16_t *__restrict__ target, const float *__restrict__ dpos,
                                                        const float *__restrict__ dnrm, const float *__restrict__ weights)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n_verts) return;
    rt_vertex o = base[v];
    const uint32_t n = count[v];
    if (n != 0u) {
        size_t cell = (size_t)slice_cell[v >> 6] + (v & 63u);
        f3 s = mk3(o.normal.x, o.normal.y, o.normal.z);
        for (uint32_t j = 0; j < n; j++, cell += 64u) {
            const float w = weights[target[cell]];
            const float *dp = dpos + 3u * cell;
            o.position.x = o.position.x + w * dp[0];
            o.position.y = o.position.y + w * dp[1];
            o.position.z = o.position.z + w * dp[2];
            if (NORMALS) {
                const float *dn = dnrm + 3u * cell;
                s = mk3(s.x + w * dn[0], s.y + w * dn[1], s.z + w * dn[2]);
            }
        }
        if (NORMALS) {
            const float d = dot(s, s);
            const f3 nn = (d > 0.0f && d < __uint_as_float(0x7f800000u)) ? normalize(s) : mk3(0.0f, 0.0f, 0.0f);
            o.normal.x = nn.x; o.normal.y = nn.y; o.normal.z = nn.z;
        }
    }
    dst[v] = o;
}

int upload(rt_context *ctx, DevBuf &b, const void *host, size_t bytes)
{
    RT_TRY(b.reserve(bytes));
    if (bytes) HIP_TRY(hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return RT_OK;
}

int use_device(const rt_context *ctx)
{
    HIP_TRY(hipSetDevice(ctx->device));
    return RT_OK;
}

}  // namespace

extern "C" {

const char *rt_version(void) { return "dxrexperiments_amd 0.1 (gfx950)"; }

const char *rt_last_error(void) { return g_last_error.c_str(); }

int rt_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        rt_set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
        return RT_ERR_HIP;
    }
    return n;
}

// ---- experiment / test knobs ------------------------------------------------------

extern "C" int rt_debug_set_option(rt_context *c, const char *name, const char *value)
{
    RT_REQUIRE(c && name && value, "null argument");
    const std::string n(name);
    // every option but fast_bvh takes a number: the whole of `value` must be one, decimal and finite ('true', 'on', '4x' used to read as 0 and
    // quietly switch things off; strtod also reads 'inf', 'nan' and '0x10').  The name is matched first, so that a misspelt option is reported as
    // unknown whatever its value: is() notes that the name exists and lets its branch run only with a well-formed value.
    char *end_i = nullptr, *end_f = nullptr;
    const long iv = strtol(value, &end_i, 10);
    const double fv = strtod(value, &end_f);
    auto bad = [&]() { rt_set_error("rt_debug_set_option: value '%s' out of range for '%s'", value, name); return RT_ERR_INVALID_ARG; };
    const bool is_int = *value != '\0' && end_i && *end_i == '\0';
    const bool is_num = *value != '\0' && end_f && *end_f == '\0' && std::isfinite(fv) && !strpbrk(value, "xX");
    const bool wants_float = n == "sah_node" || n == "sah_prim" || n == "dist_check_seconds";
    const bool value_ok = n == "fast_bvh" || (wants_float ? is_num : is_int);
    bool known = false;
    auto is = [&](bool match) { known = known || match; return match && value_ok; };
    if (is(n == "lds_top")) c->lds_top = iv != 0;
    else if (is(n == "lds_stack_rows")) { if (iv != 0 && iv != RT_LDS_STACK_ROWS && iv != RT_LDS_STACK_ROWS_TEST) return bad(); c->lds_stack_rows = (uint32_t)iv; }
    else if (is(n == "persistent_blocks_per_cu")) { if (iv < 0 || iv > 16) return bad(); c->blocks_per_cu_override = (uint32_t)iv; }
    else if (is(n == "fast_bvh")) { if (strcmp(value, "lbvh") != 0 && strcmp(value, "ploc") != 0) return bad(); c->use_ploc = strcmp(value, "ploc") == 0; }
    else if (is(n == "build_batch")) { if (iv < 0 || iv > 64) return bad(); c->build_batch = (uint32_t)iv; }
    else if (is(n == "leaf_max")) { if (iv < 1 || iv > 8) return bad(); c->leaf_max = (uint32_t)iv; }
    else if (is(n == "wide_sah")) c->wide_sah = iv != 0;
    else if (is(n == "sah_node")) { if (!(fv > 0.0)) return bad(); c->sah_node = (float)fv; }
    else if (is(n == "sah_prim")) { if (!(fv > 0.0)) return bad(); c->sah_prim = (float)fv; }
    else if (is(n == "verbose")) c->verbose = iv != 0;
    else if (is(n == "shadow_cache_res")) { if (iv < -1 || iv > 8192) return bad(); c->opt_shadow_cache_res = (int)iv; }
    else if (is(n == "shadow_cache_pixels")) { if (iv < -1 || iv > 1) return bad(); c->opt_shadow_cache_pixels = (int)iv; }
    else if (is(n == "primary_persistent")) { if (iv < -1 || iv > 1) return bad(); c->opt_primary_persistent = (int)iv; }
    else if (is(n == "seven_waves_always")) c->opt_seven_waves_always = iv != 0;
    else if (is(n == "free_radius")) c->opt_free_radius = iv != 0;
    else if (is(n == "split_refs")) c->opt_split_refs = iv != 0;
    else if (is(n == "fail_ploc_rounds")) c->opt_fail_ploc_rounds = iv != 0;
    else if (is(n == "primary_retry_cap")) { if (iv < 0 || iv > (1 << 24)) return bad(); c->opt_primary_retry_cap = (uint32_t)iv; }
    else if (is(n == "batch_max")) { if (iv < 0 || iv > 32) return bad(); c->opt_batch_max = (uint32_t)iv; }
    else if (is(n == "queue_budget_mb")) { if (iv < 0) return bad(); c->opt_queue_budget_mb = (size_t)iv; }
    else if (is(n == "dist_check_seconds")) { if (!(fv >= 0.0)) return bad(); c->opt_dist_check_seconds = fv; }
    else if (known) { rt_set_error("rt_debug_set_option: '%s' is not a number (option '%s')", value, name); return RT_ERR_INVALID_ARG; }
    else { rt_set_error("rt_debug_set_option: unknown option '%s'", name); return RT_ERR_INVALID_ARG; }
    return RT_OK;
}

// ---- context -------------------------------------------------------------------

static int context_create(int device, void *stream, bool own, rt_context **out)
{
    RT_REQUIRE(out, "null argument");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) {
        rt_set_error("rt_context_create: device %d not present (%d HIP devices visible)", device, n);
        return RT_ERR_HIP;
    }
    HIP_TRY(hipSetDevice(device));
    rt_context *c = new (std::nothrow) rt_context();
    if (!c) { rt_set_error("out of host memory"); return RT_ERR_OOM; }
    c->device = device;
    c->own_stream = own;
    if (own) {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { rt_set_error("hipStreamCreate: %s", hipGetErrorString(e)); delete c; return RT_ERR_HIP; }
    } else c->stream = (hipStream_t)stream;
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
        rt_set_error("hipEventCreate failed");
        delete c;          // (the stream and the first event go with it)
        return RT_ERR_HIP;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        c->cu_count = (uint32_t)prop.multiProcessorCount;
    if (hipHostMalloc((void **)&c->pinned, RT_PINNED_WORDS * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) c->pinned = nullptr;
    // the one environment variable the library reads for its behaviour: RT_DEBUG_OPTIONS="name=value,name=value" 
    if (const char *env = getenv("RT_DEBUG_OPTIONS")) {
        std::string all(env);
        size_t at = 0;
        while (at < all.size()) {
            size_t end = all.find(',', at);
            if (end == std::string::npos) end = all.size();
            auto trim = [](const std::string &t) {          // blanks around an item, a name or a value are not part of it
                const size_t a = t.find_first_not_of(" \t"), b = t.find_last_not_of(" \t");
                return a == std::string::npos ? std::string() : t.substr(a, b - a + 1);
            };
            const std::string item = trim(all.substr(at, end - at));
            const size_t eq = item.find('=');
            if (item.empty()) { at = end + 1; continue; }
            if (eq == std::string::npos) {
                rt_set_error("RT_DEBUG_OPTIONS: '%s' is not name=value", item.c_str());
                rt_context_release(c);
                return RT_ERR_INVALID_ARG;
            }
            if (rt_debug_set_option(c, trim(item.substr(0, eq)).c_str(), trim(item.substr(eq + 1)).c_str()) != RT_OK) {
                const std::string why = rt_last_error();
                rt_set_error("RT_DEBUG_OPTIONS: %s", why.c_str());
                rt_context_release(c);
                return RT_ERR_INVALID_ARG;
            }
            at = end + 1;
        }
    }
    // the RT_* variables the library read one by one until round 4 are no longer looked at: say so once instead of quietly running the defaults
    {
        static const char *const legacy[] = {"RT_BATCH_MAX", "RT_BUILD_BATCH", "RT_DIST_CHECK_SECONDS", "RT_FAST_BVH", "RT_FREE_RADIUS", "RT_LDS_STACK_ROWS", "RT_LDS_TOP",
                                             "RT_LEAF_MAX", "RT_PERSISTENT_BLOCKS_PER_CU", "RT_PRIMARY_PERSISTENT", "RT_QUEUE_BUDGET_MB", "RT_SAH_NODE", "RT_SAH_PRIM",
                                             "RT_SEVEN_WAVES_ALWAYS", "RT_SHADOW_CACHE_PIXELS", "RT_SHADOW_CACHE_RES", "RT_VERBOSE", "RT_WIDE_SAH"};
        static bool warned = false;
        for (const char *v : legacy)
            if (!warned && getenv(v)) {
                fprintf(stderr, "[dxr_amd] %s is set but no longer read: use RT_DEBUG_OPTIONS=\"name=value,...\" or rt_debug_set_option (INTEGRATION.md)\n", v);
                warned = true;
            }
    }
    *out = c;
    return RT_OK;
}

int rt_context_create(int device, rt_context **out) { return context_create(device, nullptr, true, out); }

int rt_context_create_on_stream(int device, void *hip_stream, rt_context **out)
{
    return context_create(device, hip_stream, false, out);
}

int rt_context_destroy(rt_context *ctx)
{
    rt_context_release(ctx);
    return RT_OK;
}

}  // extern "C"

void rt_context_retain(rt_context *ctx) { if (ctx) ctx->refs++; }

void rt_scene_retain(rt_scene *s) { if (s) s->refs++; }

// The context lives until its handle AND every object created on it are gone.
void rt_context_release(rt_context *ctx)
{
    if (!ctx || --ctx->refs > 0) return;
    delete ctx;
}

rt_context::~rt_context()
{
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
    if (pinned) (void)hipHostFree(pinned);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

rt_model::~rt_model()
{
    if (ctx) (void)hipSetDevice(ctx->device);
}

rt_scene::~rt_scene()
{
    (void)hipSetDevice(ctx->device);
    for (SceneInstance &in : inst) {
        std::vector<rt_scene *> &held = in.model->scenes;      // (the model outlives this: the scene retains it)
        for (size_t k = 0; k < held.size(); k++)
            if (held[k] == this) { held.erase(held.begin() + k); break; }
        rt_model_destroy(in.model);
    }
}

extern "C" {

int rt_context_synchronize(rt_context *ctx)
{
    RT_REQUIRE(ctx, "null context");
    RT_TRY(use_device(ctx));
    RT_TRY(rt_context_flush_deferred(ctx));          // frames a deferred pipeline still holds are part of "everything submitted"
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_context_get_stack_memory(rt_context *ctx, size_t *bytes)
{
    RT_REQUIRE(ctx && bytes, "null argument");
    *bytes = ctx->deep_stack.bytes;
    return RT_OK;
}

int rt_context_get_stream(rt_context *ctx, void **hip_stream_out)
{
    RT_REQUIRE(ctx && hip_stream_out, "null argument");
    // (a caller that asks for the stream is about to order its own work behind "everything submitted": the frames a deferred
    // pipeline still holds go onto the stream first -- ADVICE r4)
    *hip_stream_out = (void *)ctx->stream;
    if (!ctx->deferred.empty()) { RT_TRY(use_device(ctx)); RT_TRY(rt_context_flush_deferred(ctx)); }
    return RT_OK;
}

int rt_context_get_device(rt_context *ctx, int *device_out)
{
    RT_REQUIRE(ctx && device_out, "null argument");
    *device_out = ctx->device;
    return RT_OK;
}

int rt_device_alloc(rt_context *ctx, size_t bytes, void **device_ptr)
{
    RT_REQUIRE(ctx && device_ptr, "null argument");
    RT_TRY(use_device(ctx));
    hipError_t e = hipMalloc(device_ptr, bytes ? bytes : 16);
    if (e != hipSuccess) {
        rt_set_error("hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP;
    }
    return RT_OK;
}

int rt_device_free(rt_context *ctx, void *device_ptr)
{
    RT_REQUIRE(ctx, "null context");
    RT_TRY(use_device(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (device_ptr) HIP_TRY(hipFree(device_ptr));
    return RT_OK;
}

int rt_device_upload(rt_context *ctx, void *device_dst, const void *host_src, size_t bytes)
{
    RT_REQUIRE(ctx && (bytes == 0 || (device_dst && host_src)), "null argument");
    RT_TRY(use_device(ctx));
    if (bytes) HIP_TRY(hipMemcpyAsync(device_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_device_download(rt_context *ctx, void *host_dst, const void *device_src, size_t bytes)
{
    RT_REQUIRE(ctx && (bytes == 0 || (host_dst && device_src)), "null argument");
    RT_TRY(use_device(ctx));
    RT_TRY(rt_context_flush_deferred(ctx));          // (device_src may be an output a deferred pipeline still owes frames to)
    if (bytes) HIP_TRY(hipMemcpyAsync(host_dst, device_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

// ---- model -----------------------------------------------------------------------

static int model_finish(rt_context *ctx, rt_model *m, rt_model **out)
{
    m->ctx = ctx;
    rt_context_retain(ctx);
    m->n_verts = (uint32_t)m->h_verts.size();
    m->n_tris = (uint32_t)(m->h_idx.size() / 3);
    for (uint32_t i : m->h_idx)
        if (i >= m->n_verts) {
            rt_set_error("index %u out of range (%u vertices)", i, m->n_verts);
            delete m;
            rt_context_release(ctx);
            return RT_ERR_INVALID_ARG;
        }
    int rc = use_device(ctx);
    if (rc == RT_OK) rc = upload(ctx, m->d_verts, m->h_verts.data(), sizeof(rt_vertex) * m->h_verts.size());
    if (rc == RT_OK) rc = upload(ctx, m->d_idx, m->h_idx.data(), sizeof(uint32_t) * m->h_idx.size());
    if (rc == RT_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) { rt_set_error("geometry upload failed"); rc = RT_ERR_HIP; }
    if (rc != RT_OK) {
        delete m;
        rt_context_release(ctx);
        return rc;
    }
    *out = m;
    return RT_OK;
}

int rt_model_create_from_arrays(rt_context *ctx, const rt_vertex *verts, uint32_t n_verts, const uint32_t *indices,
                                uint32_t n_tris, rt_model **out)
{
    RT_REQUIRE(ctx && verts && indices && out, "null argument");
    RT_REQUIRE(n_verts > 0 && n_tris > 0, "a model needs at least one triangle");
    rt_model *m = new (std::nothrow) rt_model();
    if (!m) { rt_set_error("out of host memory"); return RT_ERR_OOM; }
    m->h_verts.assign(verts, verts + n_verts);
    m->h_idx.assign(indices, indices + 3 * (size_t)n_tris);
    return model_finish(ctx, m, out);
}

int rt_model_create_from_obj(rt_context *ctx, const char *path, rt_model **out)
{
    RT_REQUIRE(ctx && path && out, "null argument");
    rt_model *m = new (std::nothrow) rt_model();
    if (!m) { rt_set_error("out of host memory"); return RT_ERR_OOM; }
    int rc = rt_obj_parse(path, m->h_verts, m->h_idx);
    if (rc != RT_OK) { delete m; return rc; }
    return model_finish(ctx, m, out);
}

int rt_model_create_from_file(rt_context *ctx, const char *path, rt_model **out)
{
    RT_REQUIRE(ctx && path && out, "null argument");
    const size_t n = strlen(path);
    const bool fbx = n >= 4 && path[n - 4] == '.' && (path[n - 3] | 0x20) == 'f' && (path[n - 2] | 0x20) == 'b' && (path[n - 1] | 0x20) == 'x';
    if (!fbx) return rt_model_create_from_obj(ctx, path, out);
    rt_model *m = new (std::nothrow) rt_model();
    if (!m) { rt_set_error("out of host memory"); return RT_ERR_OOM; }
    int rc = rt_fbx_parse(path, m->h_verts, m->h_idx);
    if (rc != RT_OK) { delete m; return rc; }
    return model_finish(ctx, m, out);
}

int rt_model_get_counts(const rt_model *m, uint32_t *n_verts, uint32_t *n_tris)
{
    RT_REQUIRE(m, "null model");
    if (n_verts) *n_verts = m->n_verts;
    if (n_tris) *n_tris = m->n_tris;
    return RT_OK;
}

// A set has gone through its checks and is about to write d_verts: frames a deferred pipeline holds are rendered first (they see the
// mesh as it was).
static int model_before_set(rt_model *m)
{
    RT_TRY(use_device(m->ctx));
    return rt_context_flush_deferred(m->ctx);
}

// ... and has been queued: the BLAS is older than the vertices, every built scene that holds the model is stale.
static void model_changed(rt_model *m)
{
    m->geom_gen++;
    m->built = false;         // rt_scene_update and rt_scene_build rebuild the BLAS (rt_build_blas)
    for (rt_scene *s : m->scenes)
        if (s->updatable) s->built = false;            // (never built, or instances added since: the next build reads the new vertices anyway)
}

static int model_set_range_check(const rt_model *m, const char *who, uint32_t first, uint32_t count)
{
    if (first > m->n_verts || count > m->n_verts - first) {
        rt_set_error("%s: vertices %u .. %llu out of range: the model has %u", who, first, (unsigned long long)first + count, m->n_verts);
        return RT_ERR_STATE;
    }
    return RT_OK;
}

int rt_model_set_vertices(rt_model *m, uint32_t first, uint32_t count, const rt_vertex *verts, uint32_t mem)
{
    RT_REQUIRE(m && (verts || count == 0), "null argument");
    RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, "unknown memory selector");
    RT_TRY(model_set_range_check(m, "rt_model_set_vertices", first, count));
    if (count == 0) return RT_OK;
    RT_TRY(model_before_set(m));
    hipStream_t st = m->ctx->stream;
    rt_vertex *dst = m->d_verts.as<rt_vertex>() + first;
    const size_t bytes = sizeof(rt_vertex) * (size_t)count;
    if (mem == RT_MEM_DEVICE) {
        HIP_TRY(hipMemcpyAsync(dst, verts, bytes, hipMemcpyDeviceToDevice, st));
        m->h_verts_stale = true;
    } else {
        HIP_TRY(hipMemcpyAsync(dst, verts, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));             // (the caller's array is its own again when the call returns)
        if (!m->h_verts_stale) memcpy(m->h_verts.data() + first, verts, bytes);
    }
    model_changed(m);
    return RT_OK;
}

int rt_model_set_positions(rt_model *m, uint32_t first, uint32_t count, const float *xyz, uint32_t mem)
{
    RT_REQUIRE(m && (xyz || count == 0), "null argument");
    RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, "unknown memory selector");
    RT_TRY(model_set_range_check(m, "rt_model_set_positions", first, count));
    if (count == 0) return RT_OK;
    rt_context *ctx = m->ctx;
    RT_TRY(model_before_set(m));
    const float *src = xyz;
    if (mem == RT_MEM_HOST) {
        RT_TRY(upload(ctx, ctx->scratch[0], xyz, 12 * (size_t)count));
        src = ctx->scratch[0].as<float>();
    }
    k_set_positions<<<(count + 255u) / 256u, 256, 0, ctx->stream>>>(m->d_verts.as<rt_vertex>(), first, count, src);
    HIP_TRY(hipGetLastError());
    if (mem == RT_MEM_HOST) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (!m->h_verts_stale)
            for (uint32_t k = 0; k < count; k++) memcpy(&m->h_verts[(size_t)first + k].position, xyz + 3 * (size_t)k, 12);
    } else m->h_verts_stale = true;
    model_changed(m);
    return RT_OK;
}

int rt_model_recompute_normals(rt_model *m)
{
    RT_REQUIRE(m, "null model");
    rt_context *ctx = m->ctx;
    RT_TRY(model_before_set(m));
    if (!m->adj_ready) {      // once per model: the index list never changes
        std::vector<uint32_t> off, tris;
        if (m->n_tris > 0x55555555u || !rt_build_adjacency(m->h_idx.data(), m->n_tris, m->n_verts, off, tris)) {
            rt_set_error("rt_model_recompute_normals: no adjacency for %u triangles over %u vertices", m->n_tris, m->n_verts);
            return RT_ERR_UNSUPPORTED;
        }
        RT_TRY(upload(ctx, m->adj_off, off.data(), 4 * off.size()));
        RT_TRY(upload(ctx, m->adj_tris, tris.data(), 4 * tris.size()));
        HIP_TRY(hipStreamSynchronize(ctx->stream));    // (the vectors go out of scope)
        m->adj_ready = true;
    }
    k_vertex_normals<<<(m->n_verts + 255u) / 256u, 256, 0, ctx->stream>>>(m->d_verts.as<rt_vertex>(), m->n_verts, m->d_idx.as<uint32_t>(),
                                                                          m->adj_off.as<uint32_t>(), m->adj_tris.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    m->h_verts_stale = true;
    model_changed(m);
    return RT_OK;
}

int rt_model_set_skin(rt_model *m, uint32_t influences, uint32_t n_bones, const uint32_t *bone_indices, const float *weights)
{
    RT_REQUIRE(m, "null model");
    rt_context *ctx = m->ctx;
    if (influences == 0) {    // no skin: the vertices stay as the last pose left them
        RT_TRY(use_device(ctx));
        HIP_TRY(hipStreamSynchronize(ctx->stream));     // (a kernel that reads the buffers may still be queued)
        m->skin_k = m->skin_bones = 0;
        m->skin_bone.release(); m->skin_weight.release(); m->skin_rest.release();
        return RT_OK;
    }
    uint32_t bad_v = 0, bad_k = 0;
    switch (rt_skin_validate(m->n_verts, influences, n_bones, bone_indices, weights, &bad_v, &bad_k)) {
    case 0: break;
    case 1: rt_set_error("rt_model_set_skin: null argument"); return RT_ERR_INVALID_ARG;
    case 2: rt_set_error("rt_model_set_skin: %u influences per vertex: 1 .. %u are supported (0 removes the skin)", influences, RT_SKIN_MAX_INFLUENCES); return RT_ERR_INVALID_ARG;
    case 3: rt_set_error("rt_model_set_skin: %u bones: 1 .. %u are supported", n_bones, RT_SKIN_MAX_BONES); return RT_ERR_INVALID_ARG;
    default:
        rt_set_error("rt_model_set_skin: vertex %u, slot %u names bone %u of %u", bad_v, bad_k, bone_indices[(size_t)bad_v * influences + bad_k], n_bones);
        return RT_ERR_INVALID_ARG;
    }
    std::vector<uint16_t> bone;
    std::vector<float> weight;
    rt_skin_pack(m->n_verts, influences, bone_indices, weights, bone, weight);
    RT_TRY(use_device(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));         // (a skin that is replaced: a kernel that reads the old one may still be queued)
    m->skin_k = m->skin_bones = 0;                      // (no skin until all of the new one is there)
    RT_TRY(upload(ctx, m->skin_bone, bone.data(), sizeof(uint16_t) * bone.size()));
    RT_TRY(upload(ctx, m->skin_weight, weight.data(), sizeof(float) * weight.size()));
    const size_t bytes = sizeof(rt_vertex) * (size_t)m->n_verts;
    RT_TRY(m->skin_rest.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(m->skin_rest.p, m->d_verts.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));       // the rest pose: the vertices as they are
    HIP_TRY(hipStreamSynchronize(ctx->stream));         // (the vectors go out of scope)
    m->skin_k = influences;
    m->skin_bones = n_bones;
    return RT_OK;             // the vertices are what they were: nothing changed, built scenes stay built
}

int rt_model_get_skin(const rt_model *m, uint32_t *influences, uint32_t *n_bones)
{
    RT_REQUIRE(m, "null model");
    if (influences) *influences = m->skin_k;
    if (n_bones) *n_bones = m->skin_bones;
    return RT_OK;
}

int rt_model_set_bones(rt_model *m, const float *bones3x4, uint32_t mem)
{
    RT_REQUIRE(m && bones3x4, "null argument");
    RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, "unknown memory selector");
    if (m->skin_k == 0) {
        rt_set_error("rt_model_set_bones: the model has no skin (rt_model_set_skin gives it one)");
        return RT_ERR_STATE;
    }
    rt_context *ctx = m->ctx;
    RT_TRY(model_before_set(m));
    const float *palette = bones3x4;
    if (mem == RT_MEM_HOST) {
        RT_TRY(upload(ctx, ctx->scratch[0], bones3x4, 48 * (size_t)m->skin_bones));
        palette = ctx->scratch[0].as<float>();
    }
    const bool lds = m->skin_bones <= RT_SKIN_LDS_BONES;
    rt_vertex *verts = m->d_verts.as<rt_vertex>();
    const rt_vertex *rest = m->skin_rest.as<rt_vertex>();
    const uint16_t *bone = m->skin_bone.as<uint16_t>();
    const float *weight = m->skin_weight.as<float>();
    switch (m->skin_k) {      // (every pose from the rest pose, the whole mesh)
#define RT_SKIN_CASE(K) case K: launch_skin<K>(ctx->stream, lds, verts, rest, m->n_verts, bone, weight, palette, m->skin_bones); break
    RT_SKIN_CASE(1); RT_SKIN_CASE(2); RT_SKIN_CASE(3); RT_SKIN_CASE(4); RT_SKIN_CASE(5); RT_SKIN_CASE(6); RT_SKIN_CASE(7); RT_SKIN_CASE(8);
#undef RT_SKIN_CASE
    default: rt_set_error("rt_model_set_bones: %u influences", m->skin_k); return RT_ERR_STATE;
    }
    HIP_TRY(hipGetLastError());
    if (mem == RT_MEM_HOST) HIP_TRY(hipStreamSynchronize(ctx->stream));      // (the caller's array is its own again, and the scratch buffer anybody's)
    m->h_verts_stale = true;
    model_changed(m);
    return RT_OK;
}

int rt_model_set_morph_targets(rt_model *m, uint32_t n_targets, const uint32_t *target_offsets, const uint32_t *vertex_indices,
                               const float *position_deltas, const float *normal_deltas)
{
    RT_REQUIRE(m, "null model");
    rt_context *ctx = m->ctx;
    if (n_targets == 0) {     // no targets: the vertices stay as the last weights left them
        RT_TRY(use_device(ctx));
        HIP_TRY(hipStreamSynchronize(ctx->stream));     // (a kernel that reads the buffers may still be queued)
        m->morph_targets = m->morph_entries = 0;
        m->morph_normals = false;
        m->morph_count.release(); m->morph_slice.release(); m->morph_target.release();
        m->morph_dpos.release(); m->morph_dnrm.release(); m->morph_base.release();
        return RT_OK;
    }
    uint32_t bad_t = 0, bad_e = 0;
    switch (rt_morph_validate(m->n_verts, n_targets, target_offsets, vertex_indices, position_deltas, &bad_t, &bad_e)) {
    case 0: break;
    case 1: rt_set_error("rt_model_set_morph_targets: null argument"); return RT_ERR_INVALID_ARG;
    case 2: rt_set_error("rt_model_set_morph_targets: %u targets: up to %u are supported (0 removes them)", n_targets, RT_MORPH_MAX_TARGETS); return RT_ERR_INVALID_ARG;
    case 3: rt_set_error("rt_model_set_morph_targets: target_offsets[0] is %u, not 0", target_offsets[0]); return RT_ERR_INVALID_ARG;
    case 4:
        rt_set_error("rt_model_set_morph_targets: target %u: its offsets decrease, %u to %u", bad_t, target_offsets[bad_t], target_offsets[bad_t + 1]);
        return RT_ERR_INVALID_ARG;
    case 5:
        rt_set_error("rt_model_set_morph_targets: target %u, entry %u names vertex %u of %u", bad_t, bad_e, vertex_indices[bad_e], m->n_verts);
        return RT_ERR_INVALID_ARG;
    case 6:
        rt_set_error("rt_model_set_morph_targets: target %u, entry %u names vertex %u after vertex %u: the indices of a target ascend strictly", bad_t,
                     bad_e, vertex_indices[bad_e], vertex_indices[bad_e - 1]);
        return RT_ERR_INVALID_ARG;
    default:
        rt_set_error("rt_model_set_morph_targets: the packed targets would take 2^32 cells or more");
        return RT_ERR_UNSUPPORTED;
    }
    rt_morph_packed pk;
    rt_morph_pack(m->n_verts, n_targets, target_offsets, vertex_indices, position_deltas, normal_deltas, pk);
    RT_TRY(use_device(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));         // (targets that are replaced: a kernel that reads the old ones may still be queued)
    m->morph_targets = m->morph_entries = 0;            // (no targets until all of the new ones are there)
    RT_TRY(upload(ctx, m->morph_count, pk.count.data(), sizeof(uint32_t) * pk.count.size()));
    RT_TRY(upload(ctx, m->morph_slice, pk.slice_cell.data(), sizeof(uint32_t) * pk.slice_cell.size()));
    RT_TRY(upload(ctx, m->morph_target, pk.target.data(), sizeof(uint16_t) * pk.target.size()));
    RT_TRY(upload(ctx, m->morph_dpos, pk.dpos.data(), sizeof(float) * pk.dpos.size()));
    RT_TRY(upload(ctx, m->morph_dnrm, pk.dnrm.data(), sizeof(float) * pk.dnrm.size()));
    const size_t bytes = sizeof(rt_vertex) * (size_t)m->n_verts;
    RT_TRY(m->morph_base.reserve(bytes));
    const void *from = m->skin_k ? m->skin_rest.p : m->d_verts.p;            // the base: the skin's rest pose, or the vertices as they are
    HIP_TRY(hipMemcpyAsync(m->morph_base.p, from, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));         // (the vectors go out of scope)
    m->morph_targets = n_targets;
    m->morph_entries = target_offsets[n_targets];
    m->morph_normals = normal_deltas != nullptr;
    return RT_OK;             // the vertices are what they were: nothing changed, built scenes stay built
}

int rt_model_get_morph_targets(const rt_model *m, uint32_t *n_targets, uint32_t *n_entries, uint32_t *has_normals)
{
    RT_REQUIRE(m, "null model");
    if (n_targets) *n_targets = m->morph_targets;
    if (n_entries) *n_entries = m->morph_entries;
    if (has_normals) *has_normals = m->morph_normals ? 1u : 0u;
    return RT_OK;
}

int rt_model_set_morph_weights(rt_model *m, const float *weights, uint32_t mem)
{
    RT_REQUIRE(m && weights, "null argument");
    RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, "unknown memory selector");
    if (m->morph_targets == 0) {
        rt_set_error("rt_model_set_morph_weights: the model has no morph targets (rt_model_set_morph_targets gives it some)");
        return RT_ERR_STATE;
    }
    rt_context *ctx = m->ctx;
    const bool skinned = m->skin_k != 0;                // the result is the skin's rest pose: no vertex changes before the next rt_model_set_bones
    if (skinned) RT_TRY(use_device(ctx));
    else RT_TRY(model_before_set(m));
    const float *w = weights;
    if (mem == RT_MEM_HOST) {
        RT_TRY(upload(ctx, ctx->scratch[0], weights, sizeof(float) * (size_t)m->morph_targets));
        w = ctx->scratch[0].as<float>();
    }
    rt_vertex *dst = skinned ? m->skin_rest.as<rt_vertex>() : m->d_verts.as<rt_vertex>();
    const rt_vertex *base = m->morph_base.as<rt_vertex>();
    const uint32_t blocks = (m->n_verts + 255u) / 256u;
    if (m->morph_normals)     // (every result from the base, the whole mesh)
        k_morph_vertices<true><<<blocks, 256, 0, ctx->stream>>>(dst, base, m->n_verts, m->morph_count.as<uint32_t>(), m->morph_slice.as<uint32_t>(),
                                                                m->morph_target.as<uint16_t>(), m->morph_dpos.as<float>(), m->morph_dnrm.as<float>(), w);
    else
        k_morph_vertices<false><<<blocks, 256, 0, ctx->stream>>>(dst, base, m->n_verts, m->morph_count.as<uint32_t>(), m->morph_slice.as<uint32_t>(),
                                                                 m->morph_target.as<uint16_t>(), m->morph_dpos.as<float>(), nullptr, w);
    HIP_TRY(hipGetLastError());
    if (mem == RT_MEM_HOST) HIP_TRY(hipStreamSynchronize(ctx->stream));      // (the caller's array is its own again, and the scratch buffer anybody's)
    if (skinned) return RT_OK;
    m->h_verts_stale = true;
    model_changed(m);
    return RT_OK;
}

int rt_model_read_geometry(const rt_model *m, rt_vertex *verts, uint32_t *indices)
{
    RT_REQUIRE(m, "null model");
    if (verts && m->h_verts_stale) {                   // vertices set from device memory: the host mirror follows on demand
        rt_model *w = const_cast<rt_model *>(m);
        RT_TRY(use_device(m->ctx));
        HIP_TRY(hipMemcpyAsync(w->h_verts.data(), m->d_verts.p, sizeof(rt_vertex) * m->h_verts.size(), hipMemcpyDeviceToHost, m->ctx->stream));
        HIP_TRY(hipStreamSynchronize(m->ctx->stream));
        w->h_verts_stale = false;
    }
    if (verts) memcpy(verts, m->h_verts.data(), sizeof(rt_vertex) * m->h_verts.size());
    if (indices) memcpy(indices, m->h_idx.data(), sizeof(uint32_t) * m->h_idx.size());
    return RT_OK;
}

int rt_model_retain(rt_model *m)
{
    RT_REQUIRE(m, "null model");
    m->refs++;
    return RT_OK;
}

int rt_model_destroy(rt_model *m)
{
    if (!m) return RT_OK;
    if (--m->refs > 0) return RT_OK;
    rt_context *ctx = m->ctx;
    delete m;
    rt_context_release(ctx);
    return RT_OK;
}

// ---- scene -----------------------------------------------------------------------

int rt_scene_create(rt_context *ctx, rt_scene **out)
{
    RT_REQUIRE(ctx && out, "null argument");
    rt_scene *s = new (std::nothrow) rt_scene();
    if (!s) { rt_set_error("out of host memory"); return RT_ERR_OOM; }
    s->ctx = ctx;
    rt_context_retain(ctx);
    *out = s;
    return RT_OK;
}

int rt_scene_add_model(rt_scene *s, rt_model *m, const float transform3x4[12])
{
    RT_REQUIRE(s && m && transform3x4, "null argument");
    RT_REQUIRE(m->ctx == s->ctx, "model and scene belong to different contexts");
    RT_TRY(rt_context_flush_deferred(s->ctx));       // frames accepted before this change see the scene as it was
    SceneInstance in;
    in.model = m;
    memcpy(in.xform, transform3x4, sizeof in.xform);
    m->refs++;
    s->inst.push_back(in);
    s->masks.push_back(0xFF);  // InstanceMask of the reference's descriptors (TopLevelASGenerator.cpp:361)
    bool held = false;
    for (rt_scene *o : m->scenes) held = held || o == s;
    if (!held) m->scenes.push_back(s);
    s->built = false;
    s->updatable = false;     // the TLAS no longer stands for this instance list: only rt_scene_build brings the scene back
    s->generation++;
    return RT_OK;
}

static int scene_range_check(const rt_scene *s, const char *who, uint32_t first, uint32_t count)
{
    const size_t n = s->inst.size();
    if (first > n || count > n - first) {
        rt_set_error("%s: instances %u .. %llu out of range: the scene has %zu", who, first, (unsigned long long)first + count, n);
        return RT_ERR_STATE;
    }
    return RT_OK;
}

// instance i joins the list the next update rewrites (once)
static void scene_mark_pending(rt_scene *s, uint32_t i)
{
    s->is_pending.resize(s->inst.size(), 0);
    if (!s->is_pending[i]) { s->is_pending[i] = 1; s->pending.push_back(i); }
}

// A build or an update has succeeded: every stored transform and mask has been read, and the vertices of the models of `changed` (an
// update: exactly the instances whose generation differed; nullptr, a build: of every instance).  Nothing is pending, the scene is fresh.
static void scene_applied(rt_scene *s, const std::vector<uint32_t> *changed)
{
    const size_t n = s->inst.size();
    if (changed) {
        for (uint32_t i : s->pending) s->is_pending[i] = 0;
        for (uint32_t i : *changed) s->seen_geom[i] = s->inst[i].model->geom_gen;
    } else {
        s->is_pending.assign(n, 0);
        s->seen_geom.resize(n);
        for (size_t i = 0; i < n; i++) s->seen_geom[i] = s->inst[i].model->geom_gen;
    }
    s->pending.clear();
    s->masks_dirty = false;
    s->built = true;
}

int rt_scene_set_instance_transforms(rt_scene *s, uint32_t first, uint32_t count, const float *transforms3x4)
{
    RT_REQUIRE(s && (transforms3x4 || count == 0), "null argument");
    RT_TRY(scene_range_check(s, "rt_scene_set_instance_transforms", first, count));
    if (count == 0) return RT_OK;
    RT_TRY(rt_context_flush_deferred(s->ctx));       // frames accepted before this change see the scene as it was
    for (uint32_t k = 0; k < count; k++) memcpy(s->inst[first + k].xform, transforms3x4 + 12 * (size_t)k, sizeof s->inst[0].xform);
    if (!s->updatable) return RT_OK;                  // never built (or instances added since): the next build reads the stored transforms
    for (uint32_t i = first; i < first + count; i++) scene_mark_pending(s, i);
    s->built = false;         // stale until rt_scene_update or rt_scene_build: nothing traces a half-applied state
    return RT_OK;
}

int rt_scene_set_instance_transform(rt_scene *s, uint32_t instance, const float transform3x4[12])
{
    RT_REQUIRE(s && transform3x4, "null argument");
    if (instance >= s->inst.size()) {
        rt_set_error("rt_scene_set_instance_transform: instance %u out of range: the scene has %zu", instance, s->inst.size());
        return RT_ERR_STATE;
    }
    return rt_scene_set_instance_transforms(s, instance, 1, transform3x4);
}

// EXTENSION: the InstanceMask member of the instance descriptors (TopLevelASGenerator.cpp:344-362), which the reference fills with 0xFF, under the
// inclusion mask 0xFF of its every TraceRay (ProgressiveRaytracing.hlsl:34,53, RaytracingCommon.hlsli:94, RealtimeRaytracing.hlsl:42,61)
int rt_scene_set_instance_masks(rt_scene *s, uint32_t first, uint32_t count, const uint8_t *masks)
{
    RT_REQUIRE(s && (masks || count == 0), "null argument");
    RT_TRY(scene_range_check(s, "rt_scene_set_instance_masks", first, count));
    if (count == 0) return RT_OK;
    RT_TRY(rt_context_flush_deferred(s->ctx));       // frames accepted before this change see the scene as it was
    bool visibility = false;
    for (uint32_t k = 0; k < count; k++) {
        visibility = visibility || ((s->masks[first + k] != 0) != (masks[k] != 0));
        s->masks[first + k] = masks[k];
    }
    if (!s->updatable || !visibility) return RT_OK;   // not built: the next build reads the stored masks; the same visibility: only the bytes change
    s->masks_dirty = true;
    s->built = false;         // stale until rt_scene_update or rt_scene_build, as with a pending transform
    return RT_OK;
}

int rt_scene_set_instance_mask(rt_scene *s, uint32_t instance, uint8_t mask)
{
    RT_REQUIRE(s, "null scene");
    if (instance >= s->inst.size()) {
        rt_set_error("rt_scene_set_instance_mask: instance %u out of range: the scene has %zu", instance, s->inst.size());
        return RT_ERR_STATE;
    }
    return rt_scene_set_instance_masks(s, instance, 1, &mask);
}

int rt_scene_get_instance_masks(const rt_scene *s, uint32_t first, uint32_t count, uint8_t *masks)
{
    RT_REQUIRE(s && (masks || count == 0), "null argument");
    RT_TRY(scene_range_check(s, "rt_scene_get_instance_masks", first, count));
    if (count) memcpy(masks, s->masks.data() + first, count);
    return RT_OK;
}

int rt_scene_update(rt_scene *s)
{
    RT_REQUIRE(s, "null scene");
    if (!s->updatable) {
        rt_set_error("rt_scene_update: the scene has not been built since its last rt_scene_add_model (an update builds no BLAS: rt_scene_build)");
        return RT_ERR_STATE;
    }
    std::vector<uint32_t> changed;                    // instances whose model's vertices were set since their records were written
    rt_scene_changed_instances(s, &changed);
    if (s->pending.empty() && changed.empty() && !s->masks_dirty) return RT_OK;      // nothing to apply: nothing launched, the generation stays
    rt_context *ctx = s->ctx;
    RT_TRY(use_device(ctx));
    RT_TRY(rt_context_flush_deferred(ctx));
    // pending masks: the visible sub-list goes up if it differs from the one the TLAS stands for (no visible instance: refused here, with every
    // pending thing kept -- showing one and updating again succeeds)
    if (s->masks_dirty) RT_TRY(rt_scene_apply_masks(ctx, s, "rt_scene_update", false));
    s->generation++;          // pipelines drop what they cached from the old geometry: shadow-cache occluders, per-pixel entries, the free sphere, the primary-mode samples
    ScopedEvent e0, e1;
    HIP_TRY(hipEventCreate(&e0.e));
    HIP_TRY(hipEventCreate(&e1.e));
    HIP_TRY(hipEventRecord(e0.e, ctx->stream));
    if (!changed.empty()) {
        // a changed model whose BLAS is older than its vertices: rebuilt by the build's own steps into the model's own buffers (one that
        // another scene's update or build has rebuilt already is built: rt_build_blas returns at once)
        for (uint32_t i : changed) RT_TRY(rt_build_blas(ctx, s->inst[i].model));
        RT_TRY(rt_update_model_records(ctx, s, changed));
        for (uint32_t i : changed) scene_mark_pending(s, i);      // ... and take their world boxes over the new vertices, with the transforms they have
    }
    // (a failure leaves the scene stale, the transforms and the models pending); e1: behind the wide collapse, in front of the read-back
    RT_TRY(rt_update_tlas(ctx, s, s->pending, "rt_scene_update", e1.e));
    HIP_TRY(hipEventElapsedTime(&s->update_ms, e0.e, e1.e));
    scene_applied(s, &changed);
    return RT_OK;
}

int rt_scene_update_ms(const rt_scene *s, float *ms)
{
    RT_REQUIRE(s && ms, "null argument");
    *ms = s->update_ms;
    return RT_OK;
}

int rt_scene_get_num_instances(const rt_scene *s, uint32_t *n)
{
    RT_REQUIRE(s && n, "null argument");
    *n = (uint32_t)s->inst.size();
    return RT_OK;
}

int rt_scene_build(rt_scene *s, uint32_t hit_group_count)
{
    (void)hit_group_count;   // hit-group stride of the reference's shader table; material = f(instance) here
    RT_REQUIRE(s, "null scene");
    RT_REQUIRE(!s->inst.empty(), "scene has no instances");
    rt_context *ctx = s->ctx;
    RT_TRY(use_device(ctx));
    RT_TRY(rt_context_flush_deferred(ctx));
    RT_TRY(rt_scene_apply_masks(ctx, s, "rt_scene_build", true));     // (no visible instance: refused as a scene without instances is)
    ScopedEvent e0, e1;
    HIP_TRY(hipEventCreate(&e0.e));
    HIP_TRY(hipEventCreate(&e1.e));
    HIP_TRY(hipEventRecord(e0.e, ctx->stream));
    s->generation++;          // device arrays are about to be reallocated: pipelines drop what they cached
    for (SceneInstance &in : s->inst) RT_TRY(rt_build_blas(ctx, in.model));
    s->updatable = false;
    RT_TRY(rt_build_tlas(ctx, s));
    HIP_TRY(hipEventRecord(e1.e, ctx->stream));
    HIP_TRY(hipEventSynchronize(e1.e));
    HIP_TRY(hipEventElapsedTime(&s->build_ms, e0.e, e1.e));
    s->updatable = true;
    scene_applied(s, nullptr);
    return RT_OK;
}

int rt_scene_destroy(rt_scene *s)
{
    if (!s) return RT_OK;
    if (--s->refs > 0) return RT_OK;
    rt_context *ctx = s->ctx;
    delete s;
    rt_context_release(ctx);
    return RT_OK;
}

static const BvhDev *pick_bvh(const rt_scene *s, int which)
{
    if (!s || !s->built) return nullptr;
    if (which < 0) return &s->tlas;
    if ((size_t)which >= s->inst.size()) return nullptr;
    return &s->inst[which].model->blas;
}

int rt_scene_bvh_info(const rt_scene *s, int which, uint32_t *n_prims, uint32_t *n_nodes, uint32_t *max_depth)
{
    const BvhDev *b = pick_bvh(s, which);
    if (!b) { if (!rt_scene_stale_error(s, "rt_scene_bvh_info")) rt_set_error("rt_scene_bvh_info: scene not built or index out of range"); return RT_ERR_STATE; }
    if (n_prims) *n_prims = b->n;
    if (n_nodes) *n_nodes = 2 * b->n - 1;
    if (max_depth) *max_depth = b->max_depth;
    return RT_OK;
}

int rt_scene_bvh_read(const rt_scene *s, int which, rt_bvh_node *nodes, uint64_t *sorted_keys, uint32_t *parents)
{
    const BvhDev *b = pick_bvh(s, which);
    if (!b) { if (!rt_scene_stale_error(s, "rt_scene_bvh_read")) rt_set_error("rt_scene_bvh_read: scene not built or index out of range"); return RT_ERR_STATE; }
    RT_TRY(use_device(s->ctx));
    const size_t nn = 2 * (size_t)b->n - 1;
    if (nodes) HIP_TRY(hipMemcpy(nodes, b->nodes.p, sizeof(rt_bvh_node) * nn, hipMemcpyDeviceToHost));
    if (sorted_keys) HIP_TRY(hipMemcpy(sorted_keys, b->keys.p, sizeof(uint64_t) * b->n, hipMemcpyDeviceToHost));
    if (parents) HIP_TRY(hipMemcpy(parents, b->parents.p, sizeof(uint32_t) * nn, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_scene_wide_info(const rt_scene *s, int which, uint32_t *n_nodes, int32_t *root_code, uint32_t *n_records)
{
    const BvhDev *b = pick_bvh(s, which);
    if (!b) { if (!rt_scene_stale_error(s, "rt_scene_wide_info")) rt_set_error("rt_scene_wide_info: scene not built or index out of range"); return RT_ERR_STATE; }
    if (n_nodes) *n_nodes = b->wide_n;
    if (root_code) *root_code = b->root_code;
    if (n_records) *n_records = which < 0 ? 0u : s->inst[which].model->n_recs;
    return RT_OK;
}

int rt_wide_layout_info(uint32_t *width, uint32_t *node_bytes)
{
    if (width) *width = RT_WIDE;
    if (node_bytes) *node_bytes = (uint32_t)sizeof(WNode);
    return RT_OK;
}

int rt_scene_wide_read(const rt_scene *s, int which, void *nodes, void *records)
{
    const BvhDev *b = pick_bvh(s, which);
    if (!b) { if (!rt_scene_stale_error(s, "rt_scene_wide_read")) rt_set_error("rt_scene_wide_read: scene not built or index out of range"); return RT_ERR_STATE; }
    RT_TRY(use_device(s->ctx));
    if (nodes && b->wide_n) HIP_TRY(hipMemcpy(nodes, b->wide.p, sizeof(WNode) * (size_t)b->wide_n, hipMemcpyDeviceToHost));
    if (records && which >= 0) HIP_TRY(hipMemcpy(records, s->inst[which].model->tris.p, sizeof(TriRec) * (size_t)s->inst[which].model->n_recs, hipMemcpyDeviceToHost));
    return RT_OK;
}

/* the validation boxes of an instance's model (rt_refs.h): *n_refs = 0 when none of its triangles is split */
int rt_scene_refs_info(const rt_scene *s, int which, uint32_t *n_tris, uint32_t *n_refs)
{
    const BvhDev *b = pick_bvh(s, which);
    if (!b || which < 0) { if (!rt_scene_stale_error(s, "rt_scene_refs_info")) rt_set_error("rt_scene_refs_info: scene not built or index out of range"); return RT_ERR_STATE; }
    const rt_model *m = s->inst[which].model;
    if (n_tris) *n_tris = m->n_tris;
    if (n_refs) *n_refs = m->ref_off.p ? (uint32_t)(m->ref_boxes.bytes / 24) : 0u;
    return RT_OK;
}

int rt_scene_refs_read(const rt_scene *s, int which, uint32_t *ref_off, float *ref_boxes, float *record_boxes)
{
    const BvhDev *b = pick_bvh(s, which);
    if (!b || which < 0) { if (!rt_scene_stale_error(s, "rt_scene_refs_read")) rt_set_error("rt_scene_refs_read: scene not built or index out of range"); return RT_ERR_STATE; }
    const rt_model *m = s->inst[which].model;
    if (!m->ref_off.p) { rt_set_error("rt_scene_refs_read: no triangle of this model is split"); return RT_ERR_STATE; }
    RT_TRY(use_device(s->ctx));
    uint32_t total = 0;
    HIP_TRY(hipMemcpy(&total, m->ref_off.as<uint32_t>() + m->n_tris, 4, hipMemcpyDeviceToHost));
    if (ref_off) HIP_TRY(hipMemcpy(ref_off, m->ref_off.p, 4 * ((size_t)m->n_tris + 1), hipMemcpyDeviceToHost));
    if (ref_boxes) HIP_TRY(hipMemcpy(ref_boxes, m->ref_boxes.p, 24 * (size_t)total, hipMemcpyDeviceToHost));
    if (record_boxes && m->rec_boxes.p) HIP_TRY(hipMemcpy(record_boxes, m->rec_boxes.p, 24 * (size_t)m->n_recs, hipMemcpyDeviceToHost));
    return RT_OK;
}

/* layout experiments (tools/layout_estimate.py): replaces the node array by a renumbering of itself */
int rt_debug_wide_write(rt_scene *s, int which, const void *nodes, uint32_t n_nodes)
{
    const BvhDev *b = pick_bvh(s, which);
    if (!b || !nodes || n_nodes != b->wide_n) { rt_set_error("rt_debug_wide_write: scene not built, or a different node count"); return RT_ERR_STATE; }
    RT_TRY(use_device(s->ctx));
    HIP_TRY(hipMemcpy(b->wide.p, nodes, sizeof(WNode) * (size_t)n_nodes, hipMemcpyHostToDevice));
    return RT_OK;                                      // (same device pointers, same node count: nothing cached goes stale)
}

int rt_scene_instance_info(const rt_scene *s, uint32_t instance, float world_box[6], float world_to_object[12])
{
    RT_REQUIRE(s, "null scene");
    if (!s->built || instance >= s->h_inst.size()) {
        if (!rt_scene_stale_error(s, "rt_scene_instance_info")) rt_set_error("scene not built or instance out of range");
        return RT_ERR_STATE;
    }
    const InstanceRec &r = s->h_inst[instance];
    if (world_box) for (int c = 0; c < 3; c++) { world_box[c] = r.wlo[c]; world_box[3 + c] = r.whi[c]; }
    if (world_to_object) memcpy(world_to_object, r.inv, sizeof r.inv);
    return RT_OK;
}

int rt_scene_build_ms(const rt_scene *s, float *ms)
{
    RT_REQUIRE(s && ms, "null argument");
    *ms = s->build_ms;
    return RT_OK;
}

// ---- batch TraceRay ---------------------------------------------------------------

int rt_trace_batch(rt_context *ctx, const rt_scene *s, const float *origin_tmin, const float *dir_tmax, size_t n,
                   uint32_t ray_flags, uint32_t kernel, uint32_t mem, float *t, float *u, float *v, uint32_t *prim,
                   uint32_t *inst, uint32_t *cnt_nodes, uint32_t *cnt_tris)
{
    RT_REQUIRE(ctx && s, "null argument");
    if (!s->built) { if (!rt_scene_stale_error(s, "rt_trace_batch")) rt_set_error("rt_trace_batch: scene not built"); return RT_ERR_STATE; }
    RT_REQUIRE(kernel == RT_TRACE_FAST || kernel == RT_TRACE_CANONICAL, "unknown kernel selector");
    if (n == 0) return RT_OK;
    RT_REQUIRE(origin_tmin && dir_tmax, "null ray arrays");
    RT_TRY(use_device(ctx));
    if (mem == RT_MEM_DEVICE) {
        TraceOut out = {t, u, v, prim, inst, cnt_nodes, cnt_tris};
        return rt_launch_trace(ctx, s, (const float4 *)origin_tmin, (const float4 *)dir_tmax, n, ray_flags, kernel, out);
    }
    RT_REQUIRE(mem == RT_MEM_HOST, "unknown memory selector");
    DevBuf *sb = ctx->scratch;
    RT_TRY(upload(ctx, sb[0], origin_tmin, n * 16));
    RT_TRY(upload(ctx, sb[1], dir_tmax, n * 16));
    void *host_out[7] = {t, u, v, prim, inst, cnt_nodes, cnt_tris};
    RT_TRY(sb[2].reserve(n * 4 * 7));
    char *base = sb[2].as<char>();
    void *dev_out[7];
    for (int k = 0; k < 7; k++) dev_out[k] = host_out[k] ? base + (size_t)k * n * 4 : nullptr;
    TraceOut out = {(float *)dev_out[0], (float *)dev_out[1], (float *)dev_out[2], (uint32_t *)dev_out[3],
                    (uint32_t *)dev_out[4], (uint32_t *)dev_out[5], (uint32_t *)dev_out[6]};
    if (kernel != RT_TRACE_CANONICAL) { out.cnt_nodes = nullptr; out.cnt_tris = nullptr; }
    RT_TRY(rt_launch_trace(ctx, s, sb[0].as<float4>(), sb[1].as<float4>(), n, ray_flags, kernel, out));
    for (int k = 0; k < 7; k++)
        if (host_out[k] && dev_out[k] && !((k >= 5) && kernel != RT_TRACE_CANONICAL))
            HIP_TRY(hipMemcpyAsync(host_out[k], dev_out[k], n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_trace_last_ms(rt_context *ctx, float *ms)
{
    RT_REQUIRE(ctx && ms, "null argument");
    RT_TRY(use_device(ctx));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    HIP_TRY(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return RT_OK;
}

// ---- device math probes -------------------------------------------------------------

int rt_debug_math(rt_context *ctx, int fn, const float *x, const float *y, float *out, size_t n)
{
    RT_REQUIRE(ctx && x && out, "null argument");
    if (n == 0) return RT_OK;
    RT_TRY(use_device(ctx));
    DevBuf *sb = ctx->scratch;
    RT_TRY(upload(ctx, sb[0], x, n * 4));
    RT_TRY(upload(ctx, sb[1], y ? y : x, n * 4));
    RT_TRY(sb[2].reserve(n * 4));
    k_debug_math<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(fn, sb[0].as<float>(), sb[1].as<float>(), sb[2].as<float>(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, sb[2].p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_debug_sample(rt_context *ctx, int kind, const uint32_t *seeds, const float *vec3_in, float exponent, float *vec3_out,
                    float *pdf_brdf, uint32_t *seeds_out, size_t n)
{
    RT_REQUIRE(ctx && seeds && vec3_in && vec3_out, "null argument");
    if (n == 0) return RT_OK;
    RT_TRY(use_device(ctx));
    DevBuf *sb = ctx->scratch;
    RT_TRY(upload(ctx, sb[0], seeds, n * 4));
    RT_TRY(upload(ctx, sb[1], vec3_in, n * 12));
    RT_TRY(sb[2].reserve(n * 12));
    RT_TRY(sb[3].reserve(n * 8));
    RT_TRY(sb[4].reserve(n * 4));
    k_debug_sample<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(kind, sb[0].as<uint32_t>(), sb[1].as<float>(), exponent,
                                                                         sb[2].as<float>(), sb[3].as<float>(), sb[4].as<uint32_t>(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(vec3_out, sb[2].p, n * 12, hipMemcpyDeviceToHost, ctx->stream));
    if (pdf_brdf) HIP_TRY(hipMemcpyAsync(pdf_brdf, sb[3].p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (seeds_out) HIP_TRY(hipMemcpyAsync(seeds_out, sb[4].p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

}  // extern "C"
