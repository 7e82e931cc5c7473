// rt_api.hip -- C-ABI entry points for error state, debug options, context, device memory and batch TraceRay, and the device
// math probes (include/dxr_amd.h).  Stand-in for libs/DXRFramework/RtContext; the model is rt_model.hip, the scene rt_scene.hip.
#include <cmath>
#include <cstring>
#include <new>

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

// The options of the primary stage's entry lists (rt_pipeline_entries.hip: k_primary_entries and its policy).  Their tests are tests/test_gpu_primary_entries.py,
// which runs every value of each against primary_entries=0 bit for bit.  1: the name is one of them (*rc: the result).
static bool entry_list_option(rt_context *c, const std::string &name, bool is_int, long iv, int *rc)
{
    const bool which[3] = {name == "primary_entries", name == "primary_entries_cut", name == "primary_entries_cap"};
    if (!which[0] && !which[1] && !which[2]) return false;
    *rc = RT_ERR_INVALID_ARG;
    if (!is_int) { rt_set_error("rt_debug_set_option: option '%s' takes a whole number", name.c_str()); return true; }
    if ((which[0] && (iv < -1 || iv > 1)) || (which[1] && (iv < 0 || iv > 128)) || (which[2] && (iv < 0 || iv > 32))) {
        rt_set_error("rt_debug_set_option: value %ld out of range for '%s'", iv, name.c_str());
        return true;
    }
    if (which[0]) c->opt_primary_entries = (int)iv;
    else if (which[1]) c->opt_primary_entries_cut = (uint32_t)iv;
    else c->opt_primary_entries_cap = (uint32_t)iv;
    *rc = RT_OK;
    return true;
}

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
    int rc_entries = RT_OK;
    if (entry_list_option(c, n, is_int, iv, &rc_entries)) return rc_entries;
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
        if (e != hipSuccess) { rt_set_error("hipStreamCreate: %s", hipGetErrorString(e)); rt_context_release(c); return RT_ERR_HIP; }
    } else c->stream = (hipStream_t)stream;
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
        rt_set_error("hipEventCreate failed");
        rt_context_release(c);         // (the stream and the first event go with it)
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

rt_context::~rt_context()
{
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
    if (pinned) (void)hipHostFree(pinned);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

extern "C" {

int rt_context_synchronize(rt_context *ctx)
{
    RT_REQUIRE(ctx, "null context");
    RT_TRY(rt_use_device(ctx));
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
    if (!ctx->deferred.empty()) { RT_TRY(rt_use_device(ctx)); RT_TRY(rt_context_flush_deferred(ctx)); }
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
    RT_TRY(rt_use_device(ctx));
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
    RT_TRY(rt_use_device(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (device_ptr) HIP_TRY(hipFree(device_ptr));
    return RT_OK;
}

int rt_device_upload(rt_context *ctx, void *device_dst, const void *host_src, size_t bytes)
{
    RT_REQUIRE(ctx && (bytes == 0 || (device_dst && host_src)), "null argument");
    RT_TRY(rt_use_device(ctx));
    if (bytes) HIP_TRY(hipMemcpyAsync(device_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_device_download(rt_context *ctx, void *host_dst, const void *device_src, size_t bytes)
{
    RT_REQUIRE(ctx && (bytes == 0 || (host_dst && device_src)), "null argument");
    RT_TRY(rt_use_device(ctx));
    RT_TRY(rt_context_flush_deferred(ctx));          // (device_src may be an output a deferred pipeline still owes frames to)
    if (bytes) HIP_TRY(hipMemcpyAsync(host_dst, device_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

// ---- batch TraceRay ---------------------------------------------------------------

int rt_trace_batch(rt_context *ctx, const rt_scene *s, const float *origin_tmin, const float *dir_tmax, size_t n,
                   uint32_t ray_flags, uint32_t kernel, uint32_t mem, float *t, float *u, float *v, uint32_t *prim,
                   uint32_t *inst, uint32_t *cnt_nodes, uint32_t *cnt_tris)
{
    RT_REQUIRE(ctx && s, "null argument");
    RT_TRY(rt_scene_require_built(s, "rt_trace_batch", "%s: scene not built"));
    RT_REQUIRE(kernel == RT_TRACE_FAST || kernel == RT_TRACE_CANONICAL, "unknown kernel selector");
    if (n == 0) return RT_OK;
    RT_REQUIRE(origin_tmin && dir_tmax, "null ray arrays");
    RT_TRY(rt_use_device(ctx));
    if (mem == RT_MEM_DEVICE) {
        TraceOut out = {t, u, v, prim, inst, cnt_nodes, cnt_tris};
        return rt_launch_trace(ctx, s, (const float4 *)origin_tmin, (const float4 *)dir_tmax, n, ray_flags, kernel, out);
    }
    RT_REQUIRE(mem == RT_MEM_HOST, "unknown memory selector");
    DevBuf *sb = ctx->scratch;
    RT_TRY(rt_upload(ctx, sb[0], origin_tmin, n * 16));
    RT_TRY(rt_upload(ctx, sb[1], dir_tmax, n * 16));
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
    RT_TRY(rt_use_device(ctx));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    HIP_TRY(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return RT_OK;
}

// ---- device math probes -------------------------------------------------------------

int rt_debug_math(rt_context *ctx, int fn, const float *x, const float *y, float *out, size_t n)
{
    RT_REQUIRE(ctx && x && out, "null argument");
    if (n == 0) return RT_OK;
    RT_TRY(rt_use_device(ctx));
    DevBuf *sb = ctx->scratch;
    RT_TRY(rt_upload(ctx, sb[0], x, n * 4));
    RT_TRY(rt_upload(ctx, sb[1], y ? y : x, n * 4));
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
    RT_TRY(rt_use_device(ctx));
    DevBuf *sb = ctx->scratch;
    RT_TRY(rt_upload(ctx, sb[0], seeds, n * 4));
    RT_TRY(rt_upload(ctx, sb[1], vec3_in, n * 12));
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
