// rt_skeleton.hip -- posed skeletons (include/dxr_amd.h "Posed skeletons"): a joint hierarchy whose local pose -- set by the caller or sampled
// from a baked clip -- becomes world matrices and a skinning palette on the device.  The palette is what rt_model_set_bones(RT_MEM_DEVICE)
// takes: rt_model_set_bones_from_skeleton hands it over and k_skin_vertices (rt_model.hip) runs unchanged.  No reference counterpart: the
// reference imports with aiProcess_PreTransformVertices (libs/DXRFramework/RtModel.cpp:26), which drops bones and node animation.
// Also here, after the kernels: the host steps a skeleton and a crowd do alike over the record they share (rt_pose_source; declared in
// rt_internal.h, called from here, rt_crowd.hip and rt_scene.hip).  The walk over the levels is rt_pose_device.h's, as the arithmetic is.
#include <cmath>
#include <new>

#include "rt_device_math.h"
#include "rt_ik.h"
#include "rt_internal.h"
#include "rt_pose_device.h"
#include "rt_skeleton.h"

namespace {

using namespace rtd;

// ONE block poses a skeleton: no block ever waits on another.  Step 1, every joint at once: L from the pose, stored where W will stand.
// Steps 2 and 3 -- the walk over the levels, then M_j = W_j o inverse_bind_j -- are walk_levels (rt_pose_device.h), which k_crowd_pose ends
// in too.  LDS (n_joints <= RT_SKELETON_LDS_JOINTS): W component major in LDS, and with it the level table and the level offsets, so that a
// level costs LDS round trips only; else W in `joints` and the tables in global memory, a global round trip per level.  The same statements
// either way: the same bytes.  `joints` is read back by other lanes than wrote it: not __restrict__.
template <bool LDS>
__global__ void __launch_bounds__(RT_SKELETON_BLOCK) k_skeleton_pose(const float *__restrict__ pose, const uint32_t *__restrict__ table,
                                                                     const uint32_t *__restrict__ level_offsets, uint32_t n_levels, uint32_t n_joints,
                                                                     const float *__restrict__ inverse_bind, float *joints, float *__restrict__ palette)
{
    constexpr uint32_t N = RT_SKELETON_LDS_JOINTS;
    __shared__ float s_w[LDS ? 12u * N : 1u];
    __shared__ uint32_t s_table[LDS ? N : 1u];
    __shared__ uint32_t s_off[LDS ? N + 1u : 1u];
    const PoseStorage<LDS ? (int)N : -1> at = {LDS ? s_w : joints, LDS ? s_table : table, LDS ? s_off : level_offsets, N};
    const uint32_t tid = threadIdx.x;
    for (uint32_t j = tid; j < n_joints; j += RT_SKELETON_BLOCK) {
        float L[12];
        local_of(pose + RT_SKELETON_POSE_FLOATS * (size_t)j, L);
        at.store(j, L);
        if (LDS) s_table[j] = table[j];
    }
    if (LDS)
        for (uint32_t l = tid; l <= n_levels; l += RT_SKELETON_BLOCK) s_off[l] = level_offsets[l];
    __syncthreads();
    walk_levels<RT_SKELETON_BLOCK, LDS>(at, n_levels, n_joints, inverse_bind, joints, palette);
}

// One lane per joint: the local pose between two keys of a clip, written as rt_skeleton_set_pose takes it, ten floats per joint.
__global__ void __launch_bounds__(256) k_skeleton_sample(const float *__restrict__ key_a, const float *__restrict__ key_b, uint32_t n_joints, float a,
                                                         float *__restrict__ pose)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_joints) return;
    float o[10];
    sample_joint(key_a, key_b, n_joints, j, a, o);
    store_pose(pose, j, o);
}

// The table of a blend's layers (rt_blend_layer, rt_skeleton.h) that travels by value as the kernel's argument: wave uniform, so it comes
// through scalar loads and the branch on the mode is a scalar branch.
struct BlendTable {
    rt_blend_layer layer[RT_SKELETON_MAX_LAYERS];
};

// One lane per joint: the layers of a blend accumulated into the local pose (include/dxr_amd.h "Posed skeletons", blending; the arithmetic
// is blend_joint, rt_pose_device.h).  P starts as layer 0's sample, or as the stored pose, which this lane alone reads and overwrites;
// there is no LDS.  `pose` is read and written in place: not __restrict__.
__global__ void __launch_bounds__(256) k_skeleton_blend(const BlendTable table, uint32_t n_layers, uint32_t n_joints, float *pose)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_joints) return;
    float P[10];
    blend_joint(table.layer, n_layers, n_joints, j, pose + RT_SKELETON_POSE_FLOATS * (size_t)j, P);
    store_pose(pose, j, P);
}

// One block of one wave: lane k < n solves constraint k (include/dxr_amd.h "Posed skeletons", inverse kinematics; the arithmetic is
// rt_ik_solve, rt_ik.h).  The lane reads its own entry where the table lies, in the kernel-argument segment: three 16-byte vector loads at
// 48 * lane, one latency for the wave -- the by-value argument is never copied to scratch (tools/kernel_resources.py: 0 B; a uniform loop
// over the entries with scalar loads and selects, the other way to keep it out of scratch, cost 0.5 us an entry: 22 us for 32).  It reads the
// thirty floats of its three joints, the twelve of W_p from `joints` (the pose before this call: what the last k_skeleton_pose left) and
// writes four floats, or eight.  Every constraint is solved from the same input pose: the host has checked that no lane writes a joint
// another lane reads (rt_skeleton_validate_ik).  `pose` is read and written in place: not __restrict__.
__global__ void __launch_bounds__(64) k_skeleton_ik(const IkTable table, uint32_t n, const float *__restrict__ joints, float *pose)
{
    const uint32_t lane = threadIdx.x;
    if (lane >= n) return;
    const IkEntry &e = table.e[lane];
    const uint32_t kind = e.kind, jc = e.c, jb = e.b, ja = e.a;
    const int32_t jp = e.p;
    float target[3], pole[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        target[c] = e.target[c];
        pole[c] = e.pole[c];
    }
    const float weight = e.weight;
    ik_solve_lane(kind, jc, jb, ja, jp, target, pole, weight, joints, pose);
}

// sk->pose holds a local pose: W and the palette from it, queued on the context's stream
int pose_skeleton(rt_skeleton *sk)
{
    hipStream_t st = sk->ctx->stream;
    const float *pose = sk->pose.as<float>(), *ib = sk->inverse_bind.as<float>();
    const uint32_t *table = sk->table.as<uint32_t>(), *off = sk->d_level_offsets.as<uint32_t>();
    if (sk->n_joints <= RT_SKELETON_LDS_JOINTS)
        k_skeleton_pose<true><<<1, RT_SKELETON_BLOCK, 0, st>>>(pose, table, off, sk->n_levels, sk->n_joints, ib, sk->joints.as<float>(), sk->palette.as<float>());
    else
        k_skeleton_pose<false><<<1, RT_SKELETON_BLOCK, 0, st>>>(pose, table, off, sk->n_levels, sk->n_joints, ib, sk->joints.as<float>(), sk->palette.as<float>());
    HIP_TRY(hipGetLastError());
    sk->queued();
    return RT_OK;
}

}  // namespace

// ---- what a skeleton and a crowd do alike (rt_internal.h) ---------------------------------------------------------------------------------
int rt_pose_require(const rt_pose_source *src, const char *who)
{
    if (src->posed) return RT_OK;
    rt_set_error("%s: the %s has no pose yet (%s)", who, src->noun(), src->pose_hint());
    return RT_ERR_STATE;
}

int rt_pose_refuse_layers(const rt_pose_source *src, const char *who, int what, const uint32_t *actor, uint32_t bad, const rt_skeleton_layer *l, uint32_t n_layers,
                          uint32_t n_clips, uint32_t n_masks)
{
    char msg[512];
    const int rc = rt_skeleton_layers_refusal(what, who, actor, bad, l, n_layers, n_clips, n_masks, src->noun(), src->pose_hint(), msg, sizeof msg);
    rt_set_error("%s", msg);
    return rc;
}

int rt_pose_refuse_ik(const rt_pose_source *src, const char *who, int what, uint32_t n, const rt_skeleton_ik *constraints, const uint32_t bad[3])
{
    char msg[512];
    const int rc = rt_skeleton_ik_refusal(what, who, n, constraints, bad, src->n_joints, src->noun(), src->pose_hint(), msg, sizeof msg);
    rt_set_error("%s", msg);
    return rc;
}

int rt_pose_read_back(rt_pose_source *src, const char *who, const DevBuf &from, size_t floats_per_joint, uint32_t first, uint32_t count, float *to)
{
    RT_TRY(rt_pose_require(src, who));
    if (first > src->n_poses || count > src->n_poses - first) {
        rt_set_error("%s: actors %u .. %u: the crowd has %u", who, first, first + count - 1u, src->n_poses);
        return RT_ERR_INVALID_ARG;
    }
    if (count == 0) return RT_OK;
    const size_t per_pose = floats_per_joint * src->n_joints;
    RT_TRY(rt_use_device(src->ctx));
    HIP_TRY(hipMemcpyAsync(to, from.as<float>() + per_pose * first, sizeof(float) * per_pose * count, hipMemcpyDeviceToHost, src->ctx->stream));
    HIP_TRY(hipStreamSynchronize(src->ctx->stream));
    return RT_OK;
}

int rt_pose_copy_in(rt_pose_source *src, const char *who, const float *trs, uint32_t mem)
{
    if (mem != RT_MEM_HOST && mem != RT_MEM_DEVICE) {
        rt_set_error("%s: unknown memory selector", who);
        return RT_ERR_INVALID_ARG;
    }
    RT_TRY(rt_use_device(src->ctx));
    const size_t bytes = sizeof(float) * RT_SKELETON_POSE_FLOATS * (size_t)src->n_joints * src->n_poses;
    // (the source keeps the poses: its read_pose answers from them, and a device source is the caller's again once the stream has passed the copy)
    HIP_TRY(hipMemcpyAsync(src->pose_of(0), trs, bytes, mem == RT_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, src->ctx->stream));
    return RT_OK;
}

int rt_pose_set_bones(rt_model *m, rt_pose_source *src, uint32_t actor, const char *who)
{
    RT_TRY(rt_pose_require(src, who));
    if (m->skin.k == 0) {
        rt_set_error("%s: the model has no skin (rt_model_set_skin gives it one)", who);
        return RT_ERR_STATE;
    }
    if (m->skin.bones != src->n_joints) {
        rt_set_error("%s: a skin of %u bones and a %s of %u joints", who, m->skin.bones, src->noun(), src->n_joints);
        return RT_ERR_STATE;
    }
    if (m->ctx != src->ctx) {
        rt_set_error("%s: the model and the %s belong to different contexts", who, src->noun());
        return RT_ERR_STATE;
    }
    return rt_model_set_bones(m, src->palette_of(actor), RT_MEM_DEVICE);
}

int rt_pose_device_ptr(const rt_pose_source *src, const char *who, const DevBuf &which, void **ptr)
{
    RT_TRY(rt_pose_require(src, who));
    *ptr = which.p;
    return RT_OK;
}

extern "C" {

int rt_skeleton_create(rt_context *ctx, uint32_t n_joints, const int32_t *parents, const float *inverse_bind, rt_skeleton **out)
{
    RT_REQUIRE(ctx && out, "null argument");
    uint32_t bad = 0;
    switch (rt_skeleton_validate(n_joints, parents, inverse_bind, &bad)) {
    case 0: break;
    case 1: rt_set_error("rt_skeleton_create: null argument"); return RT_ERR_INVALID_ARG;
    case 2: rt_set_error("rt_skeleton_create: %u joints: 1 .. %u are supported", n_joints, RT_SKELETON_MAX_JOINTS); return RT_ERR_INVALID_ARG;
    default:
        rt_set_error("rt_skeleton_create: joint %u names parent %d: a parent is -1 (a root) or a joint before its child", bad, parents[bad]);
        return RT_ERR_INVALID_ARG;
    }
    std::vector<uint32_t> order, table;                 // (before sk: a failed creation joins the stream while what it was uploading is still there)
    rt_made<rt_skeleton> sk;
    RT_TRY(rt_make(ctx, sk));
    sk->n_joints = n_joints;
    sk->parents.assign(parents, parents + n_joints);
    sk->n_levels = rt_skeleton_levels(n_joints, parents, order, sk->level_offsets);
    rt_skeleton_pack_table(parents, order, table);
    RT_TRY(rt_use_device(ctx));
    RT_TRY(rt_upload(ctx, sk->table, table.data(), sizeof(uint32_t) * table.size()));
    RT_TRY(rt_upload(ctx, sk->d_level_offsets, sk->level_offsets.data(), sizeof(uint32_t) * sk->level_offsets.size()));
    RT_TRY(rt_upload(ctx, sk->inverse_bind, inverse_bind, 48 * (size_t)n_joints));
    RT_TRY(sk->pose.reserve(sizeof(float) * RT_SKELETON_POSE_FLOATS * (size_t)n_joints));
    RT_TRY(sk->joints.reserve(48 * (size_t)n_joints));
    RT_TRY(sk->palette.reserve(48 * (size_t)n_joints));
    HIP_TRY(hipStreamSynchronize(ctx->stream));         // (the vectors go out of scope, the caller's array is its own again)
    *out = sk.release();
    return RT_OK;
}

// (a scene with instances attached to it holds it: they keep their last transform)
int rt_skeleton_destroy(rt_skeleton *sk) { return rt_release(sk); }

int rt_skeleton_get_info(const rt_skeleton *sk, uint32_t *n_joints, uint32_t *n_levels, uint32_t *n_clips)
{
    RT_REQUIRE(sk, "null skeleton");
    if (n_joints) *n_joints = sk->n_joints;
    if (n_levels) *n_levels = sk->n_levels;
    if (n_clips) *n_clips = (uint32_t)sk->clips.size();
    return RT_OK;
}

int rt_skeleton_set_pose(rt_skeleton *sk, const float *trs, uint32_t mem)
{
    RT_REQUIRE(sk && trs, "null argument");
    RT_TRY(rt_pose_copy_in(sk, "rt_skeleton_set_pose", trs, mem));
    RT_TRY(pose_skeleton(sk));
    return rt_pose_join_host(sk, mem);
}

int rt_skeleton_add_clip(rt_skeleton *sk, uint32_t n_keys, const float *times, const float *trs, uint32_t *clip_out)
{
    RT_REQUIRE(sk && trs, "null argument");
    uint32_t bad = 0;
    switch (rt_skeleton_validate_times(n_keys, times, &bad)) {
    case 0: break;
    case 1: rt_set_error("rt_skeleton_add_clip: null argument"); return RT_ERR_INVALID_ARG;
    case 2: rt_set_error("rt_skeleton_add_clip: a clip needs at least one key"); return RT_ERR_INVALID_ARG;
    case 3: rt_set_error("rt_skeleton_add_clip: the time of key %u is not finite", bad); return RT_ERR_INVALID_ARG;
    default:
        rt_set_error("rt_skeleton_add_clip: key %u at %g after key %u at %g: the times ascend strictly", bad, (double)times[bad], bad - 1u, (double)times[bad - 1u]);
        return RT_ERR_INVALID_ARG;
    }
    rt_context *ctx = sk->ctx;
    const size_t nj = sk->n_joints, per_key = RT_SKELETON_POSE_FLOATS * nj;
    std::vector<float> keys;
    try {
        keys.resize(per_key * n_keys);
    } catch (const std::bad_alloc &) {
        rt_set_error("out of host memory");
        return RT_ERR_OOM;
    }
    for (size_t k = 0; k < n_keys; k++)                 // joint major -> component major within a key
        for (size_t j = 0; j < nj; j++)
            for (size_t c = 0; c < RT_SKELETON_POSE_FLOATS; c++) keys[k * per_key + c * nj + j] = trs[k * per_key + j * RT_SKELETON_POSE_FLOATS + c];
    SkeletonClip clip;
    clip.times.assign(times, times + n_keys);
    RT_TRY(rt_use_device(ctx));
    RT_TRY(rt_upload(ctx, clip.keys, keys.data(), sizeof(float) * keys.size()));
    RT_TRY(rt_upload(ctx, clip.d_times, times, sizeof(float) * (size_t)n_keys));      // (the copy a crowd's layout names: rt_crowd_set_blend_device searches it on the device)
    HIP_TRY(hipStreamSynchronize(ctx->stream));         // (the vector goes out of scope, and the caller's times are its own again)
    sk->clips.push_back(std::move(clip));               // (earlier clips keep their ids and their buffers)
    if (clip_out) *clip_out = (uint32_t)sk->clips.size() - 1u;
    return RT_OK;
}

int rt_skeleton_clear_clips(rt_skeleton *sk)
{
    RT_REQUIRE(sk, "null skeleton");
    if (sk->clips.empty()) return RT_OK;
    RT_TRY(rt_use_device(sk->ctx));
    HIP_TRY(hipStreamSynchronize(sk->ctx->stream));     // (a sampling kernel that reads a clip may still be queued)
    sk->clips.clear();
    sk->clip_gen++;                                     // (a crowd's layout that names a clip is stale: rt_crowd_set_blend_device refuses it)
    return RT_OK;
}

int rt_skeleton_set_time(rt_skeleton *sk, uint32_t clip, float t)
{
    RT_REQUIRE(sk, "null skeleton");
    RT_REQUIRE(!std::isnan(t), "the time is NaN");
    if (clip >= sk->clips.size()) {
        rt_set_error("rt_skeleton_set_time: clip %u: the skeleton has %zu (rt_skeleton_add_clip adds one)", clip, sk->clips.size());
        return RT_ERR_STATE;
    }
    rt_context *ctx = sk->ctx;
    const SkeletonClip &c = sk->clips[clip];
    const uint32_t n_keys = (uint32_t)c.times.size();
    uint32_t i = 0;
    float a = 0.0f;
    rt_skeleton_segment(n_keys, c.times.data(), t, &i, &a);
    const size_t per_key = RT_SKELETON_POSE_FLOATS * (size_t)sk->n_joints;
    const float *key_a = c.keys.as<float>() + per_key * i;
    const float *key_b = n_keys == 1u ? key_a : key_a + per_key;
    RT_TRY(rt_use_device(ctx));
    k_skeleton_sample<<<(sk->n_joints + 255u) / 256u, 256, 0, ctx->stream>>>(key_a, key_b, sk->n_joints, a, sk->pose.as<float>());
    HIP_TRY(hipGetLastError());
    return pose_skeleton(sk);
}

int rt_skeleton_add_mask(rt_skeleton *sk, const float *weights, uint32_t *mask_out)
{
    RT_REQUIRE(sk && weights, "null argument");
    rt_context *ctx = sk->ctx;
    DevBuf mask;
    RT_TRY(rt_use_device(ctx));
    RT_TRY(rt_upload(ctx, mask, weights, sizeof(float) * (size_t)sk->n_joints));
    HIP_TRY(hipStreamSynchronize(ctx->stream));         // (the caller's array is its own again)
    sk->masks.push_back(std::move(mask));               // (earlier masks keep their ids and their buffers)
    if (mask_out) *mask_out = (uint32_t)sk->masks.size() - 1u;
    return RT_OK;
}

int rt_skeleton_clear_masks(rt_skeleton *sk)
{
    RT_REQUIRE(sk, "null skeleton");
    if (sk->masks.empty()) return RT_OK;
    RT_TRY(rt_use_device(sk->ctx));
    HIP_TRY(hipStreamSynchronize(sk->ctx->stream));     // (a blend kernel that reads a mask may still be queued)
    sk->masks.clear();
    sk->mask_gen++;                                     // (likewise)
    return RT_OK;
}

int rt_skeleton_get_num_masks(const rt_skeleton *sk, uint32_t *n)
{
    RT_REQUIRE(sk && n, "null argument");
    *n = (uint32_t)sk->masks.size();
    return RT_OK;
}

int rt_skeleton_set_blend(rt_skeleton *sk, uint32_t n_layers, const rt_skeleton_layer *layers)
{
    RT_REQUIRE(sk && layers, "null argument");
    const uint32_t n_clips = (uint32_t)sk->clips.size(), n_masks = (uint32_t)sk->masks.size();
    uint32_t bad = 0;
    const int what = rt_skeleton_validate_layers(n_layers, layers, n_clips, n_masks, sk->posed, &bad);
    if (what) return rt_pose_refuse_layers(sk, "rt_skeleton_set_blend", what, nullptr, bad, what > 2 ? &layers[bad] : nullptr, n_layers, n_clips, n_masks);
    rt_context *ctx = sk->ctx;
    BlendTable table = {};
    for (uint32_t k = 0; k < n_layers; k++) {
        const rt_skeleton_layer &l = layers[k];
        const SkeletonClip *c = l.clip == RT_SKELETON_CURRENT_POSE ? nullptr : &sk->clips[l.clip];
        const float *mask = k > 0u && l.mask != RT_SKELETON_NO_MASK ? sk->masks[l.mask].as<float>() : nullptr;
        rt_skeleton_pack_layer(l, k, sk->n_joints, c ? (uint32_t)c->times.size() : 0u, c ? c->times.data() : nullptr, c ? c->keys.as<float>() : nullptr, mask,
                               table.layer[k]);
    }
    RT_TRY(rt_use_device(ctx));
    k_skeleton_blend<<<(sk->n_joints + 255u) / 256u, 256, 0, ctx->stream>>>(table, n_layers, sk->n_joints, sk->pose.as<float>());
    HIP_TRY(hipGetLastError());
    return pose_skeleton(sk);
}

int rt_skeleton_solve_ik(rt_skeleton *sk, uint32_t n, const rt_skeleton_ik *constraints)
{
    RT_REQUIRE(sk && constraints, "null argument");
    const int32_t *parents = sk->parents.data();
    uint32_t bad[3] = {0, 0, 0};
    const int what = rt_skeleton_validate_ik(n, constraints, sk->n_joints, parents, sk->posed, bad);
    if (what) return rt_pose_refuse_ik(sk, "rt_skeleton_solve_ik", what, n, constraints, bad);
    IkTable table = {};
    rt_skeleton_pack_ik(n, constraints, parents, table);
    RT_TRY(rt_use_device(sk->ctx));
    k_skeleton_ik<<<1, 64, 0, sk->ctx->stream>>>(table, n, sk->joints.as<float>(), sk->pose.as<float>());
    HIP_TRY(hipGetLastError());
    return pose_skeleton(sk);
}

int rt_skeleton_read_pose(rt_skeleton *sk, float *trs)
{
    RT_REQUIRE(sk && trs, "null argument");
    return rt_pose_read_back(sk, "rt_skeleton_read_pose", sk->pose, RT_SKELETON_POSE_FLOATS, 0u, 1u, trs);
}

int rt_skeleton_read_joints(rt_skeleton *sk, float *world3x4)
{
    RT_REQUIRE(sk && world3x4, "null argument");
    return rt_pose_read_back(sk, "rt_skeleton_read_joints", sk->joints, 12, 0u, 1u, world3x4);
}

int rt_skeleton_read_palette(rt_skeleton *sk, float *palette3x4)
{
    RT_REQUIRE(sk && palette3x4, "null argument");
    return rt_pose_read_back(sk, "rt_skeleton_read_palette", sk->palette, 12, 0u, 1u, palette3x4);
}

int rt_skeleton_get_palette_device_ptr(rt_skeleton *sk, void **ptr)
{
    RT_REQUIRE(sk && ptr, "null argument");
    return rt_pose_device_ptr(sk, "rt_skeleton_get_palette_device_ptr", sk->palette, ptr);
}

int rt_skeleton_get_joints_device_ptr(rt_skeleton *sk, void **ptr)
{
    RT_REQUIRE(sk && ptr, "null argument");
    return rt_pose_device_ptr(sk, "rt_skeleton_get_joints_device_ptr", sk->joints, ptr);
}

int rt_model_set_bones_from_skeleton(rt_model *m, rt_skeleton *sk)
{
    RT_REQUIRE(m && sk, "null argument");
    return rt_pose_set_bones(m, sk, 0u, "rt_model_set_bones_from_skeleton");
}

}  // extern "C"
