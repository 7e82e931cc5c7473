// rt_trace.hip -- batch TraceRay kernels behind rt_trace_batch().
#include "rt_trace_wave.h"

using namespace rtd;

namespace {

constexpr int TRACE_BLOCK = 256;

RT_DEV void store_hit(const TraceOut &out, size_t i, const HitD &h)
{
    const bool miss = h.inst == RT_NO_HIT;
    if (out.t) out.t[i] = miss ? -1.0f : h.t;
    if (out.u) out.u[i] = h.u;
    if (out.v) out.v[i] = h.v;
    if (out.prim) out.prim[i] = h.prim;
    if (out.inst) out.inst[i] = h.inst;
}

RT_DEV RayD load_ray(const float4 *__restrict__ o, const float4 *__restrict__ d, size_t i)
{
    const v4f a = ldg16(o, i * 16), b = ldg16(d, i * 16);
    RayD r;
    r.o = mk3(a.x, a.y, a.z); r.tmin = a.w;
    r.d = mk3(b.x, b.y, b.z); r.tmax = b.w;
    return r;
}

__global__ void __launch_bounds__(TRACE_BLOCK)
k_trace_canonical(SceneDev sc, const float4 *__restrict__ o, const float4 *__restrict__ d, size_t n, uint32_t flags, TraceOut out)
{
    const size_t i = (size_t)blockIdx.x * TRACE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const RayD r = load_ray(o, d, i);
    uint32_t cn, ct;
    const HitD h = trace_canonical(sc, r, flags, cn, ct);
    store_hit(out, i, h);
    if (out.cnt_nodes) out.cnt_nodes[i] = cn;
    if (out.cnt_tris) out.cnt_tris[i] = ct;
}

struct BatchSrc {
    const float4 *o, *d;
    uint32_t n, fl;
    RT_DEV uint32_t count() const { return n; }
    RT_DEV uint32_t flags() const { return fl; }
    RT_DEV bool load(uint32_t i, RayD &r) const { r = load_ray(o, d, i); return true; }
};

struct BatchSink {
    TraceOut out;
    RT_DEV void store(uint32_t i, const HitD &h, bool) const { store_hit(out, i, h); }
};

template <int STACK, bool TWO_LEVEL>
__global__ void __launch_bounds__(TRACE_BLOCK) k_trace_fast(SceneDev sc, BatchSrc src, BatchSink sink, uint32_t *pool)
{
    __shared__ int smem[(RT_ROWS(STACK) + RT_TOP_ROWS(TRACE_BLOCK)) * TRACE_BLOCK];
    trace_wave<RT_ROWS(STACK), TRACE_BLOCK, TWO_LEVEL, RT_POOL_CHUNK, false, false, false, RT_REFS(STACK)>(sc, src, sink, pool, smem, nullptr);
}

template <int STACK>
void launch_fast(const rt_context *ctx, bool two_level, hipStream_t st, const SceneDev &sc, const BatchSrc &src, const BatchSink &sink, uint32_t *pool)
{
    if (two_level)
        k_trace_fast<STACK, true><<<rt_persistent_grid(ctx, k_trace_fast<STACK, true>, TRACE_BLOCK, src.n), TRACE_BLOCK, 0, st>>>(sc, src, sink, pool);
    else
        k_trace_fast<STACK, false><<<rt_persistent_grid(ctx, k_trace_fast<STACK, false>, TRACE_BLOCK, src.n), TRACE_BLOCK, 0, st>>>(sc, src, sink, pool);
}

// rt_debug_wide_step: ONE call of the engine's wide_step per lane, on caller-supplied nodes, from an empty stack (sp = 0, where the pure-LDS
// instantiation is legal too) -- the production STACK / BLOCK, the engine's make_inv and its prologue's copy of the nodes to LDS.
// out: five ints per item -- the node entered (RT_NODE_EMPTY: every child culled), the new sp, the rows pushed in stack order
// (RT_NODE_NONE in the rows above sp).
template <bool DEEP, bool ANYHIT>
__global__ void __launch_bounds__(TRACE_BLOCK)
k_debug_wide_step(const WNode *nodes, uint32_t top_n, const int *__restrict__ index, const float4 *__restrict__ o, const float4 *__restrict__ d,
                  uint32_t n, int *deep, int *__restrict__ out)
{
    constexpr int STACK = RT_LDS_STACK_ROWS;
    __shared__ int smem[(STACK + RT_TOP_ROWS(TRACE_BLOCK)) * TRACE_BLOCK];
    LaneStack<STACK, TRACE_BLOCK> st;
    st.lds = smem + threadIdx.x;
    st.threads = gridDim.x * TRACE_BLOCK;
    st.deep = deep + (size_t)blockIdx.x * TRACE_BLOCK + threadIdx.x;
    int *topl = smem + STACK * TRACE_BLOCK;
    if (top_n != 0) {
        const int *src_top = (const int *)nodes;
        for (uint32_t i = threadIdx.x; i < top_n * RT_TOP_WORDS; i += TRACE_BLOCK) topl[i] = src_top[(i / RT_TOP_WORDS) * (uint32_t)(sizeof(WNode) / 4) + i % RT_TOP_WORDS];
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * TRACE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const RayD r = load_ray(o, d, i);
    const RayInv ri = make_inv(r.o, r.d);
    for (int row = 0; row < 3; row++) st.lds[row * TRACE_BLOCK] = RT_NODE_NONE;
    int node = index[i], sp = 0;
    wide_step<DEEP, ANYHIT>(nodes, topl, top_n, ri, r.tmin, r.tmax, st, node, sp);
    out[5 * (size_t)i] = node;
    out[5 * (size_t)i + 1] = sp;
    for (int row = 0; row < 3; row++) out[5 * (size_t)i + 2 + row] = row < sp ? st.read(row) : RT_NODE_NONE;
}

}  // namespace

extern "C" int rt_debug_wide_step(rt_context *ctx, const void *nodes, uint32_t n_nodes, const int32_t *node_index, const float *origin_tmin,
                                  const float *dir_tbest, size_t n, uint32_t variant, int32_t *out)
{
    RT_REQUIRE(ctx && nodes && node_index && origin_tmin && dir_tbest && out, "null argument");
    RT_REQUIRE(variant < 8u, "unknown variant bits");
    RT_REQUIRE(n_nodes > 0 && n_nodes < (1u << 24) && n < (1u << 24), "too many nodes or items");
    const bool lds_top = (variant & RT_WIDE_STEP_LDS_TOP) != 0;
    if (lds_top) RT_REQUIRE(n_nodes <= RT_TOP_NODES, "the LDS-resident top holds RT_TOP_NODES nodes at most");
    for (size_t i = 0; i < n; i++) RT_REQUIRE(node_index[i] >= 0 && (uint32_t)node_index[i] < n_nodes, "node index out of range");
    if (n == 0) return RT_OK;
    RT_TRY(rt_use_device(ctx));
    hipStream_t st = ctx->stream;
    DevBuf *sb = ctx->scratch;
    const unsigned grid = (unsigned)((n + TRACE_BLOCK - 1) / TRACE_BLOCK);
    RT_TRY(sb[0].reserve(sizeof(WNode) * (size_t)n_nodes));
    RT_TRY(sb[1].reserve(n * 4));
    RT_TRY(sb[2].reserve(n * 16));
    RT_TRY(sb[3].reserve(n * 16));
    RT_TRY(sb[4].reserve(n * 20));
    RT_TRY(sb[5].reserve((size_t)grid * TRACE_BLOCK * 4));          // one global stack row: a step from sp = 0 reaches none
    HIP_TRY(hipMemcpyAsync(sb[0].p, nodes, sizeof(WNode) * (size_t)n_nodes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(sb[1].p, node_index, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(sb[2].p, origin_tmin, n * 16, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(sb[3].p, dir_tbest, n * 16, hipMemcpyHostToDevice, st));
    const WNode *nd = sb[0].as<WNode>();
    const uint32_t top_n = lds_top ? n_nodes : 0u;
    const int *ix = sb[1].as<int>();
    const float4 *o = sb[2].as<float4>(), *d = sb[3].as<float4>();
    int *deep = sb[5].as<int>(), *res = sb[4].as<int>();
    switch (variant & (RT_WIDE_STEP_ANYHIT | RT_WIDE_STEP_DEEP)) {
    case 0: k_debug_wide_step<false, false><<<grid, TRACE_BLOCK, 0, st>>>(nd, top_n, ix, o, d, (uint32_t)n, deep, res); break;
    case RT_WIDE_STEP_ANYHIT: k_debug_wide_step<false, true><<<grid, TRACE_BLOCK, 0, st>>>(nd, top_n, ix, o, d, (uint32_t)n, deep, res); break;
    case RT_WIDE_STEP_DEEP: k_debug_wide_step<true, false><<<grid, TRACE_BLOCK, 0, st>>>(nd, top_n, ix, o, d, (uint32_t)n, deep, res); break;
    default: k_debug_wide_step<true, true><<<grid, TRACE_BLOCK, 0, st>>>(nd, top_n, ix, o, d, (uint32_t)n, deep, res); break;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, sb[4].p, n * 20, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_launch_trace(rt_context *ctx, const rt_scene *s, const float4 *o, const float4 *d, size_t n, uint32_t ray_flags,
                    uint32_t kernel, const TraceOut &out)
{
    if (n == 0) return RT_OK;
    SceneDev sc = s->dev();
    hipStream_t st = ctx->stream;
    if (kernel == RT_TRACE_CANONICAL) {
        const unsigned grid = (unsigned)((n + TRACE_BLOCK - 1) / TRACE_BLOCK);
        HIP_TRY(hipEventRecord(ctx->ev0, st));
        k_trace_canonical<<<grid, TRACE_BLOCK, 0, st>>>(sc, o, d, n, ray_flags, out);
    } else {
        if (n > 0xFFFFFF00ull) { rt_set_error("rt_trace_batch: more than 2^32 rays in one batch"); return RT_ERR_INVALID_ARG; }
        RT_TRY(ctx->pool.reserve(RT_POOL_GROUPS * RT_POOL_STRIDE * 4));
        HIP_TRY(hipMemsetAsync(ctx->pool.p, 0, RT_POOL_GROUPS * RT_POOL_STRIDE * 4, st));
        BatchSrc src = {o, d, (uint32_t)n, ray_flags};
        BatchSink sink = {out};
        HIP_TRY(hipEventRecord(ctx->ev0, st));
        uint32_t *pool = ctx->pool.as<uint32_t>();
        // a fixed number of LDS stack rows whatever the depth of the tree: deeper walks continue in global rows
        RT_TRY(rt_scene_dev_for_launch(ctx, s, rt_lds_stack_rows(ctx), (size_t)ctx->cu_count * 16 * TRACE_BLOCK, &sc));
        if (s->has_refs) {
            if (ctx->lds_stack_rows == RT_LDS_STACK_ROWS_TEST) launch_fast<RT_LDS_STACK_ROWS_TEST + RT_STACK_REFS>(ctx, s->two_level, st, sc, src, sink, pool);
            else launch_fast<RT_LDS_STACK_ROWS + RT_STACK_REFS>(ctx, s->two_level, st, sc, src, sink, pool);
        } else if (ctx->lds_stack_rows == RT_LDS_STACK_ROWS_TEST) launch_fast<RT_LDS_STACK_ROWS_TEST>(ctx, s->two_level, st, sc, src, sink, pool);
        else launch_fast<RT_LDS_STACK_ROWS>(ctx, s->two_level, st, sc, src, sink, pool);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->ev1, st));
    return RT_OK;
}
