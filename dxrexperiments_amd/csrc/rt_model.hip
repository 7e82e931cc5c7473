// rt_model.hip -- the model behind rt_model_* (include/dxr_amd.h): creation, read-back, and every VERTEX PRODUCER with its kernel -- deforming
// meshes, skins, morph targets.  Stand-in for libs/DXRFramework/RtModel.  What a producer owes the scenes that hold the model is written once
// here: "the producer sequence" below; what a skin and a set of morph targets have in common when they are set: "the attachment sequence".
#include <cstring>
#include <initializer_list>
#include <new>

#include "rt_adjacency.h"
#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_morph.h"
#include "rt_skin.h"

namespace {

using namespace rtd;

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
    const f3 n = unit_or_zero(s);
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
    const f3 n = unit_or_zero(mk3((B[0] * nx + B[1] * ny) + B[2] * nz, (B[4] * nx + B[5] * ny) + B[6] * nz, (B[8] * nx + B[9] * ny) + B[10] * nz));
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
            const f3 nn = unit_or_zero(s);
            o.normal.x = nn.x; o.normal.y = nn.y; o.normal.z = nn.z;
        }
    }
    dst[v] = o;
}

int model_finish(rt_made<rt_model> &m, rt_model **out)
{
    rt_context *ctx = m->ctx;
    m->n_verts = (uint32_t)m->h_verts.size();
    m->n_tris = (uint32_t)(m->h_idx.size() / 3);
    for (uint32_t i : m->h_idx)
        if (i >= m->n_verts) { rt_set_error("index %u out of range (%u vertices)", i, m->n_verts); return RT_ERR_INVALID_ARG; }
    RT_TRY(rt_use_device(ctx));
    RT_TRY(rt_upload(ctx, m->d_verts, m->h_verts.data(), sizeof(rt_vertex) * m->h_verts.size()));
    RT_TRY(rt_upload(ctx, m->d_idx, m->h_idx.data(), sizeof(uint32_t) * m->h_idx.size()));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { rt_set_error("geometry upload failed"); return RT_ERR_HIP; }
    *out = m.release();
    return RT_OK;
}

// ---- the producer sequence ---------------------------------------------------------------
// A vertex producer writes the model's device vertices and leaves its BLAS, and every built scene that holds the model, stale.  Each runs its
// own checks and then produce(), which is all it owes the scenes and the pipelines ("The producer contract").  It writes:
enum Writes {
    WRITES_VERTS,             // d_verts, by a kernel or from device memory: the host mirror is stale
    WRITES_VERTS_MIRRORED,    // d_verts, the bytes of a HOST array: the caller copies them into h_verts too while that is current, and it stays so
    WRITES_REST_POSE          // morph weights on a skinned model: skin.rest only, no vertex changes before the next rt_model_set_bones
};

// New vertices have been queued: the BLAS is older than they are, every built scene that holds the model is stale.
void model_changed(rt_model *m)
{
    m->geom_gen++;
    m->built = false;         // rt_scene_update and rt_scene_build rebuild the BLAS (rt_build_blas)
    for (rt_scene *s : m->scenes) rt_scene_model_changed(s);
}

// `input`: the `floats` floats the launch reads, in host or device memory as `mem` says, or nullptr.  launch(const float *on_device) queues the
// producer's kernel or copy on the context's stream and returns RT_OK or, with its message set, an error.
template <class Launch>
int produce(rt_model *m, Writes w, uint32_t mem, const float *input, size_t floats, Launch launch)
{
    rt_context *ctx = m->ctx;
    RT_TRY(rt_use_device(ctx));
    if (w != WRITES_REST_POSE) RT_TRY(rt_context_flush_deferred(ctx));      // frames a deferred pipeline holds are rendered first: they see the mesh as it was
    if (input && mem == RT_MEM_HOST) {                  // a host array goes through the first scratch buffer, a device array is read in place
        RT_TRY(rt_upload(ctx, ctx->scratch[0], input, sizeof(float) * floats));
        input = ctx->scratch[0].as<float>();
    }
    RT_TRY(launch(input));
    HIP_TRY(hipGetLastError());
    if (mem == RT_MEM_HOST) HIP_TRY(hipStreamSynchronize(ctx->stream));     // (the caller's array is its own again, and the scratch buffer anybody's)
    if (w == WRITES_REST_POSE) return RT_OK;            // (nothing that a frame or a scene reads has changed)
    if (w != WRITES_VERTS_MIRRORED) m->h_verts_stale = true;
    model_changed(m);
    return RT_OK;
}

int model_set_range_check(const rt_model *m, const char *who, uint32_t first, uint32_t count)
{
    if (first > m->n_verts || count > m->n_verts - first) {
        rt_set_error("%s: vertices %u .. %llu out of range: the model has %u", who, first, (unsigned long long)first + count, m->n_verts);
        return RT_ERR_STATE;
    }
    return RT_OK;
}

// ---- the attachment sequence -------------------------------------------------------------
// A skin and a set of morph targets are arrays packed on the host, a snapshot of the vertices, and counts that say "none" while they are zero.
struct Count { uint32_t *field; uint32_t value; };
struct Packed { DevBuf *to; const void *from; size_t bytes; };
template <class T> Packed packed(DevBuf &to, const std::vector<T> &from) { return {&to, from.data(), sizeof(T) * from.size()}; }

// the model's vertices as they stand in `from`, device to device, into `to`
int model_snapshot(rt_model *m, DevBuf &to, const DevBuf &from)
{
    const size_t bytes = sizeof(rt_vertex) * (size_t)m->n_verts;
    RT_TRY(to.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(to.p, from.p, bytes, hipMemcpyDeviceToDevice, m->ctx->stream));
    return RT_OK;
}

// Join the stream (a queued kernel may still read the old buffers); the counts to zero (a failure half-way leaves "none"); the arrays up and
// the snapshot taken; join again (the host arrays go out of scope); the counts.  No vertex changes: built scenes stay built.
int model_attach(rt_model *m, std::initializer_list<Count> counts, std::initializer_list<Packed> arrays, DevBuf &snapshot, const DevBuf &verts)
{
    RT_TRY(rt_use_device(m->ctx));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    for (const Count &c : counts) *c.field = 0;
    for (const Packed &a : arrays) RT_TRY(rt_upload(m->ctx, *a.to, a.from, a.bytes));
    RT_TRY(model_snapshot(m, snapshot, verts));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    for (const Count &c : counts) *c.field = c.value;
    return RT_OK;
}

// ... and taken off again: an empty A over it frees every buffer, once no queued kernel reads them.  The vertices stay as they are.
template <class A>
int model_detach(rt_model *m, A &attachment)
{
    RT_TRY(rt_use_device(m->ctx));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    attachment = A();
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_model_create_from_arrays(rt_context *ctx, const rt_vertex *verts, uint32_t n_verts, const uint32_t *indices,
                                uint32_t n_tris, rt_model **out)
{
    RT_REQUIRE(ctx && verts && indices && out, "null argument");
    RT_REQUIRE(n_verts > 0 && n_tris > 0, "a model needs at least one triangle");
    rt_made<rt_model> m;
    RT_TRY(rt_make(ctx, m));
    m->h_verts.assign(verts, verts + n_verts);
    m->h_idx.assign(indices, indices + 3 * (size_t)n_tris);
    return model_finish(m, out);
}

int rt_model_create_from_obj(rt_context *ctx, const char *path, rt_model **out)
{
    RT_REQUIRE(ctx && path && out, "null argument");
    rt_made<rt_model> m;
    RT_TRY(rt_make(ctx, m));
    RT_TRY(rt_obj_parse(path, m->h_verts, m->h_idx));
    return model_finish(m, out);
}

int rt_model_create_from_file(rt_context *ctx, const char *path, rt_model **out)
{
    RT_REQUIRE(ctx && path && out, "null argument");
    const size_t n = strlen(path);
    const bool fbx = n >= 4 && path[n - 4] == '.' && (path[n - 3] | 0x20) == 'f' && (path[n - 2] | 0x20) == 'b' && (path[n - 1] | 0x20) == 'x';
    if (!fbx) return rt_model_create_from_obj(ctx, path, out);
    rt_made<rt_model> m;
    RT_TRY(rt_make(ctx, m));
    RT_TRY(rt_fbx_parse(path, m->h_verts, m->h_idx));
    return model_finish(m, out);
}

int rt_model_get_counts(const rt_model *m, uint32_t *n_verts, uint32_t *n_tris)
{
    RT_REQUIRE(m, "null model");
    if (n_verts) *n_verts = m->n_verts;
    if (n_tris) *n_tris = m->n_tris;
    return RT_OK;
}

int rt_model_set_vertices(rt_model *m, uint32_t first, uint32_t count, const rt_vertex *verts, uint32_t mem)
{
    RT_REQUIRE(m && (verts || count == 0), "null argument");
    RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, "unknown memory selector");
    RT_TRY(model_set_range_check(m, "rt_model_set_vertices", first, count));
    if (count == 0) return RT_OK;
    const bool host = mem == RT_MEM_HOST;
    const size_t bytes = sizeof(rt_vertex) * (size_t)count;
    RT_TRY(produce(m, host ? WRITES_VERTS_MIRRORED : WRITES_VERTS, mem, nullptr, 0, [&](const float *) {        // whole records, copied: no kernel, nothing staged
        HIP_TRY(hipMemcpyAsync(m->d_verts.as<rt_vertex>() + first, verts, bytes, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, m->ctx->stream));
        return RT_OK;
    }));
    if (host && !m->h_verts_stale) memcpy(m->h_verts.data() + first, verts, bytes);
    return RT_OK;
}

int rt_model_set_positions(rt_model *m, uint32_t first, uint32_t count, const float *xyz, uint32_t mem)
{
    RT_REQUIRE(m && (xyz || count == 0), "null argument");
    RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, "unknown memory selector");
    RT_TRY(model_set_range_check(m, "rt_model_set_positions", first, count));
    if (count == 0) return RT_OK;
    const bool host = mem == RT_MEM_HOST;
    RT_TRY(produce(m, host ? WRITES_VERTS_MIRRORED : WRITES_VERTS, mem, xyz, 3 * (size_t)count, [&](const float *src) {
        k_set_positions<<<(count + 255u) / 256u, 256, 0, m->ctx->stream>>>(m->d_verts.as<rt_vertex>(), first, count, src);
        return RT_OK;
    }));
    if (host && !m->h_verts_stale)
        for (uint32_t k = 0; k < count; k++) memcpy(&m->h_verts[(size_t)first + k].position, xyz + 3 * (size_t)k, 12);
    return RT_OK;
}

int rt_model_recompute_normals(rt_model *m)
{
    RT_REQUIRE(m, "null model");
    rt_context *ctx = m->ctx;
    return produce(m, WRITES_VERTS, RT_MEM_DEVICE, nullptr, 0, [&](const float *) -> int {
        if (!m->adj_ready) {  // once per model: the index list never changes
            std::vector<uint32_t> off, tris;
            if (m->n_tris > 0x55555555u || !rt_build_adjacency(m->h_idx.data(), m->n_tris, m->n_verts, off, tris)) {
                rt_set_error("rt_model_recompute_normals: no adjacency for %u triangles over %u vertices", m->n_tris, m->n_verts);
                return RT_ERR_UNSUPPORTED;
            }
            RT_TRY(rt_upload(ctx, m->adj_off, off.data(), 4 * off.size()));
            RT_TRY(rt_upload(ctx, m->adj_tris, tris.data(), 4 * tris.size()));
            HIP_TRY(hipStreamSynchronize(ctx->stream));            // (the vectors go out of scope)
            m->adj_ready = true;
        }
        k_vertex_normals<<<(m->n_verts + 255u) / 256u, 256, 0, ctx->stream>>>(m->d_verts.as<rt_vertex>(), m->n_verts, m->d_idx.as<uint32_t>(),
                                                                              m->adj_off.as<uint32_t>(), m->adj_tris.as<uint32_t>());
        return RT_OK;
    });
}

int rt_model_set_skin(rt_model *m, uint32_t influences, uint32_t n_bones, const uint32_t *bone_indices, const float *weights)
{
    RT_REQUIRE(m, "null model");
    ModelSkin &sk = m->skin;
    if (influences == 0) return model_detach(m, sk);    // no skin: the vertices stay as the last pose left them
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
    // the rest pose: the vertices as they are
    return model_attach(m, {{&sk.k, influences}, {&sk.bones, n_bones}}, {packed(sk.bone, bone), packed(sk.weight, weight)}, sk.rest, m->d_verts);
}

int rt_model_get_skin(const rt_model *m, uint32_t *influences, uint32_t *n_bones)
{
    RT_REQUIRE(m, "null model");
    if (influences) *influences = m->skin.k;
    if (n_bones) *n_bones = m->skin.bones;
    return RT_OK;
}

int rt_model_set_bones(rt_model *m, const float *bones3x4, uint32_t mem)
{
    RT_REQUIRE(m && bones3x4, "null argument");
    RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, "unknown memory selector");
    const ModelSkin &sk = m->skin;
    if (sk.k == 0) {
        rt_set_error("rt_model_set_bones: the model has no skin (rt_model_set_skin gives it one)");
        return RT_ERR_STATE;
    }
    return produce(m, WRITES_VERTS, mem, bones3x4, 12 * (size_t)sk.bones, [&](const float *palette) -> int {
        switch (sk.k) {       // (every pose from the rest pose, the whole mesh)
#define RT_SKIN_CASE(K) case K: launch_skin<K>(m->ctx->stream, sk.bones <= RT_SKIN_LDS_BONES, m->d_verts.as<rt_vertex>(), sk.rest.as<rt_vertex>(), m->n_verts, \
                                               sk.bone.as<uint16_t>(), sk.weight.as<float>(), palette, sk.bones); break
        RT_SKIN_CASE(1); RT_SKIN_CASE(2); RT_SKIN_CASE(3); RT_SKIN_CASE(4); RT_SKIN_CASE(5); RT_SKIN_CASE(6); RT_SKIN_CASE(7); RT_SKIN_CASE(8);
#undef RT_SKIN_CASE
        default: rt_set_error("rt_model_set_bones: %u influences", sk.k); return RT_ERR_STATE;
        }
        return RT_OK;
    });
}

int rt_model_set_morph_targets(rt_model *m, uint32_t n_targets, const uint32_t *target_offsets, const uint32_t *vertex_indices,
                               const float *position_deltas, const float *normal_deltas)
{
    RT_REQUIRE(m, "null model");
    ModelMorph &mo = m->morph;
    if (n_targets == 0) return model_detach(m, mo);     // no targets: the vertices stay as the last weights left them
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
    // the base: the skin's rest pose, or the vertices as they are
    RT_TRY(model_attach(m, {{&mo.targets, n_targets}, {&mo.entries, target_offsets[n_targets]}},
                        {packed(mo.count, pk.count), packed(mo.slice, pk.slice_cell), packed(mo.target, pk.target), packed(mo.dpos, pk.dpos), packed(mo.dnrm, pk.dnrm)},
                        mo.base, m->skin.k ? m->skin.rest : m->d_verts));
    mo.normals = normal_deltas != nullptr;
    return RT_OK;
}

int rt_model_get_morph_targets(const rt_model *m, uint32_t *n_targets, uint32_t *n_entries, uint32_t *has_normals)
{
    RT_REQUIRE(m, "null model");
    if (n_targets) *n_targets = m->morph.targets;
    if (n_entries) *n_entries = m->morph.entries;
    if (has_normals) *has_normals = m->morph.normals ? 1u : 0u;
    return RT_OK;
}

int rt_model_set_morph_weights(rt_model *m, const float *weights, uint32_t mem)
{
    RT_REQUIRE(m && weights, "null argument");
    RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, "unknown memory selector");
    const ModelMorph &mo = m->morph;
    if (mo.targets == 0) {
        rt_set_error("rt_model_set_morph_weights: the model has no morph targets (rt_model_set_morph_targets gives it some)");
        return RT_ERR_STATE;
    }
    const bool skinned = m->skin.k != 0;                // the result is the skin's rest pose
    return produce(m, skinned ? WRITES_REST_POSE : WRITES_VERTS, mem, weights, mo.targets, [&](const float *w) {
        rt_vertex *dst = skinned ? m->skin.rest.as<rt_vertex>() : m->d_verts.as<rt_vertex>();
        const uint32_t blocks = (m->n_verts + 255u) / 256u;
        if (mo.normals)       // (every result from the base, the whole mesh)
            k_morph_vertices<true><<<blocks, 256, 0, m->ctx->stream>>>(dst, mo.base.as<rt_vertex>(), m->n_verts, mo.count.as<uint32_t>(), mo.slice.as<uint32_t>(),
                                                                       mo.target.as<uint16_t>(), mo.dpos.as<float>(), mo.dnrm.as<float>(), w);
        else
            k_morph_vertices<false><<<blocks, 256, 0, m->ctx->stream>>>(dst, mo.base.as<rt_vertex>(), m->n_verts, mo.count.as<uint32_t>(), mo.slice.as<uint32_t>(),
                                                                        mo.target.as<uint16_t>(), mo.dpos.as<float>(), nullptr, w);
        return RT_OK;
    });
}

int rt_model_read_geometry(const rt_model *m, rt_vertex *verts, uint32_t *indices)
{
    RT_REQUIRE(m, "null model");
    if (verts && m->h_verts_stale) {                   // vertices set from device memory: the host mirror follows on demand
        rt_model *w = const_cast<rt_model *>(m);
        RT_TRY(rt_use_device(m->ctx));
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
    rt_retain(m);
    return RT_OK;
}

int rt_model_destroy(rt_model *m) { return rt_release(m); }

}  // extern "C"

