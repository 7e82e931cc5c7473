// rt_crowd.hip -- crowds (include/dxr_amd.h "Posed skeletons", crowds): n_actors poses of ONE skeleton, all made by one launch.  A crowd
// reads its skeleton's hierarchy, inverse binds, clips and masks where they live and owns the actors' poses, world matrices and palettes,
// actor major; what reads a skeleton's palette or W -- the skin kernel, the scene's gather kernel -- reads an actor's slice unchanged.  The
// arithmetic and the walk over the levels are rt_pose_device.h's, the very functions rt_skeleton.hip calls: actor a is, bit for bit, a skeleton
// given the same call.  What the host does alike for both -- the pose check, read-backs, the copy of the caller's poses, handing a palette to
// a skin, the text of a layer refusal -- is rt_skeleton.hip's (rt_internal.h).
// rt_crowd_set_layout + rt_crowd_set_blend_device drive a crowd from device memory: the host checks and uploads, once, which clip, mask
// and mode every layer of every actor has, and a posing call is then the launch alone, its times and weights read where the caller keeps them.
// No reference counterpart, as for rt_skeleton.hip (libs/DXRFramework/RtModel.cpp:26 drops bones and node animation).
#include <cmath>
#include <new>

#include "rt_crowd.h"
#include "rt_internal.h"
#include "rt_pose_device.h"

namespace {

using namespace rtd;

// ONE block poses ONE actor, blockIdx.x: no block waits on another, and a launch of n_actors blocks fills the device where the single
// skeleton's one block fills one CU.  Blend and pose are fused: the local pose never makes a round trip through memory between them.
//   Phase 0, a lane per joint, strided: the actor's accumulated pose P (blend_joint; `layers` are this actor's n_layers records, read through
//     addresses that are uniform over the block: scalar loads, and the branch on a layer's mode stays a scalar branch), written to the
//     actor's slice of `pose`, and local_of(P) into LDS where W will stand.  n_layers == 0 (rt_crowd_set_poses): the slice holds the pose
//     already, and L comes from it as k_skeleton_pose takes it.
//   Phases 1 and 2: walk_levels (rt_pose_device.h), the text k_skeleton_pose ends in: the level walk, then W and W o inverse_bind out to the
//     actor's slices of `joints` and `palette`.
// LDS is dynamic and sized by the rig (rt_crowd_lds_bytes): W component major with a row of n_joints floats per component -- the lanes of a
// wave read consecutive words -- then the level table and the level offsets.  `pose` is read and written in place by the lane that owns the
// joint: not __restrict__.
// The kernel has TWO FORMS.  DEVICE == false: `src` is the table of records the host packed and uploaded (rt_crowd_set_times, _set_blend),
// or nothing it reads (rt_crowd_set_poses).  DEVICE == true (rt_crowd_set_blend_device): `src` names the slots of the crowd's layout and the
// caller's times and weights, all n_actors x n_layers in device memory.  Lane k < n_layers of the block's first wave loads slot (actor, k), its
// time and its weight, finds the segment in the clip's device copy of its key times and writes record k -- rt_crowd_layer_of_slot, the text
// the host packs with -- into a table at the BASE of the block's LDS (rt_crowd_lds_bytes_device), so that the records never touch global
// memory; one barrier; then the phases above run as they are, with blend_joint reading that table (the same word for every lane: a
// broadcast).  Nothing of a time or a weight becomes an address except the segment index, which rt_skeleton_segment keeps inside the clip
// for any 32 bits: no validation on the device, and none needed.
template <bool DEVICE> struct CrowdSource;
template <> struct CrowdSource<false> { using type = const rt_blend_layer *__restrict__; };
struct CrowdDeviceSource {
    const rt_crowd_slot *slots;          // [n_actors][n_layers]
    const float *times, *weights;        // [n_actors][n_layers] each; weights == nullptr: the slots' own
};
template <> struct CrowdSource<true> { using type = CrowdDeviceSource; };

template <uint32_t BLOCK, bool DEVICE>
__global__ void __launch_bounds__(BLOCK) k_crowd_pose(typename CrowdSource<DEVICE>::type src, uint32_t n_layers, const uint32_t *__restrict__ table,
                                                      const uint32_t *__restrict__ level_offsets, uint32_t n_levels, uint32_t n_joints,
                                                      const float *__restrict__ inverse_bind, float *pose, float *__restrict__ joints,
                                                      float *__restrict__ palette)
{
    extern __shared__ __align__(8) float s_dyn[];
    const uint32_t N = n_joints;
    float *s_w = s_dyn;                                          // [12][N]
    if constexpr (DEVICE) s_w += (sizeof(rt_blend_layer) / sizeof(float)) * (size_t)n_layers;      // (behind the records)
    uint32_t *s_table = (uint32_t *)(s_w + 12u * (size_t)N);     // [N]
    uint32_t *s_off = s_table + N;                               // [n_levels + 1] (n_levels <= N)
    const PoseStorage<0> at = {s_w, s_table, s_off, N};
    const uint32_t tid = threadIdx.x, actor = blockIdx.x;
    const rt_blend_layer *mine;
    if constexpr (DEVICE) {
        rt_blend_layer *s_layers = (rt_blend_layer *)s_dyn;      // [n_layers] (n_layers <= RT_SKELETON_MAX_LAYERS < a wave)
        if (tid < n_layers) {
            const size_t e = (size_t)actor * n_layers + tid;
            const rt_crowd_slot slot = src.slots[e];
            rt_blend_layer b;
            rt_crowd_layer_of_slot(slot, n_joints, src.times[e], src.weights ? src.weights[e] : slot.weight, b);
            s_layers[tid] = b;
        }
        __syncthreads();
        mine = s_layers;
    } else
        mine = src + (size_t)actor * n_layers;
    pose += RT_SKELETON_POSE_FLOATS * (size_t)N * actor;
    joints += 12u * (size_t)N * actor;
    palette += 12u * (size_t)N * actor;
    for (uint32_t j = tid; j < n_joints; j += BLOCK) {
        float L[12];
        if (n_layers) {
            float P[10];
            blend_joint(mine, n_layers, n_joints, j, pose + RT_SKELETON_POSE_FLOATS * (size_t)j, P);
            store_pose(pose, j, P);
            local_of(P, L);
        } else
            local_of(pose + RT_SKELETON_POSE_FLOATS * (size_t)j, L);
        at.store(j, L);
        s_table[j] = table[j];
    }
    for (uint32_t l = tid; l <= n_levels; l += BLOCK) s_off[l] = level_offsets[l];
    __syncthreads();
    walk_levels<BLOCK, true>(at, n_levels, n_joints, inverse_bind, joints, palette);
}

// c->pose holds every actor's held pose, and (n_layers > 0) c->layers every actor's records -- or (`device`) c->slots every actor's slots,
// and `device` names the caller's times and weights: ONE launch, queued on the context's stream
template <uint32_t BLOCK>
void launch_pose(rt_crowd *c, uint32_t n_layers, const CrowdDeviceSource *device)
{
    const rt_skeleton *sk = c->sk;
    hipStream_t st = c->ctx->stream;
    const uint32_t *table = sk->table.as<uint32_t>(), *off = sk->d_level_offsets.as<uint32_t>();
    const float *ib = sk->inverse_bind.as<float>();
    float *pose = c->pose.as<float>(), *joints = c->joints.as<float>(), *palette = c->palette.as<float>();
    if (device)
        k_crowd_pose<BLOCK, true><<<c->n_poses, BLOCK, rt_crowd_lds_bytes_device(c->n_joints, n_layers), st>>>(*device, n_layers, table, off, sk->n_levels, c->n_joints, ib,
                                                                                                            pose, joints, palette);
    else
        k_crowd_pose<BLOCK, false><<<c->n_poses, BLOCK, rt_crowd_lds_bytes(c->n_joints), st>>>(c->layers.as<rt_blend_layer>(), n_layers, table, off, sk->n_levels,
                                                                                             c->n_joints, ib, pose, joints, palette);
}

int pose_crowd(rt_crowd *c, uint32_t n_layers, const CrowdDeviceSource *device = nullptr)
{
    const uint32_t block = rt_crowd_block(c->n_joints);
    if (block == 64u) launch_pose<64>(c, n_layers, device);
    else if (block == 128u) launch_pose<128>(c, n_layers, device);
    else launch_pose<256>(c, n_layers, device);
    HIP_TRY(hipGetLastError());
    c->queued();              // (once for the whole crowd)
    return RT_OK;
}

// the skeleton's clips and masks as the packing reads them
void clips_and_masks(const rt_skeleton *sk, std::vector<rt_crowd_clip> &clips, std::vector<const float *> &masks)
{
    clips.resize(sk->clips.size());
    masks.resize(sk->masks.size());
    for (size_t k = 0; k < clips.size(); k++)
        clips[k] = {(uint32_t)sk->clips[k].times.size(), sk->clips[k].times.data(), sk->clips[k].keys.as<float>(), sk->clips[k].d_times.as<float>()};
    for (size_t k = 0; k < masks.size(); k++) masks[k] = sk->masks[k].as<float>();
}

// every actor's validated layers: packed into a staging slot, uploaded -- the one upload of the call -- and posed
int blend_crowd(rt_crowd *c, uint32_t n_layers, const rt_skeleton_layer *layers)
{
    rt_context *ctx = c->ctx;
    const rt_skeleton *sk = c->sk;
    std::vector<rt_crowd_clip> clips;
    std::vector<const float *> masks;
    clips_and_masks(sk, clips, masks);
    const size_t bytes = sizeof(rt_blend_layer) * (size_t)c->n_poses * n_layers;
    RT_TRY(rt_use_device(ctx));
    // (what can refuse comes first: a table that cannot grow keeps the one it has -- nothing is queued that reads it -- and nothing has changed)
    RT_TRY(c->layers.reserve(bytes));
    CrowdStage *s = nullptr;
    RT_TRY(crowd_stage(c, bytes, &s));
    rt_crowd_pack_layers(c->n_poses, n_layers, layers, c->n_joints, clips.data(), masks.data(), (rt_blend_layer *)s->block);
    HIP_TRY(hipMemcpyAsync(c->layers.p, s->block, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(s->event, ctx->stream));
    s->in_flight = true;
    return pose_crowd(c, n_layers);
}

// every actor's list held to rt_crowd_validate_layers; RT_OK, or the refusal under the name of the call that asked
int check_layers(const rt_crowd *c, const char *who, uint32_t n_layers, const rt_skeleton_layer *layers)
{
    const uint32_t n_clips = (uint32_t)c->sk->clips.size(), n_masks = (uint32_t)c->sk->masks.size();
    uint32_t a = 0, bad = 0;
    const int what = rt_crowd_validate_layers(c->n_poses, n_layers, layers, n_clips, n_masks, c->posed, &a, &bad);
    return what ? rt_pose_refuse_layers(c, who, what, &a, bad, what > 2 ? &layers[(size_t)a * n_layers + bad] : nullptr, n_layers, n_clips, n_masks) : RT_OK;
}

}  // namespace

// The next staging slot, the host's to write `bytes` into: the two slots are written in turn, and a slot is waited for only while the copy
// out of it -- the one of the call before last -- has not passed on the stream.  Back-to-back calls therefore never wait for the device
// unless they run two uploads ahead of it.  Declared in rt_internal.h: rt_crowd_ik.hip stages its one upload through it too.
int crowd_stage(rt_crowd *c, size_t bytes, CrowdStage **out)
{
    CrowdStage &s = c->stage[c->next_stage];
    if (s.in_flight) {
        HIP_TRY(hipEventSynchronize(s.event));
        s.in_flight = false;
    }
    if (!s.event) HIP_TRY(hipEventCreateWithFlags(&s.event, hipEventDisableTiming));
    if (s.bytes < bytes) {
        void *b = nullptr;
        if (hipHostMalloc(&b, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            rt_set_error("out of page-locked host memory (%zu bytes)", bytes);
            return RT_ERR_OOM;
        }
        if (s.block) (void)hipHostFree(s.block);
        s.block = b;
        s.bytes = bytes;
    }
    c->next_stage ^= 1u;
    *out = &s;
    return RT_OK;
}

rt_crowd::~rt_crowd()
{
    for (CrowdStage &s : stage) {
        if (s.event) (void)hipEventDestroy(s.event);
        if (s.block) (void)hipHostFree(s.block);
    }
    (void)rt_release(sk);
}

extern "C" {

int rt_crowd_create(rt_skeleton *sk, uint32_t n_actors, rt_crowd **out)
{
    RT_REQUIRE(sk && out, "null argument");
    RT_REQUIRE(n_actors >= 1u, "a crowd has at least one actor");
    if (sk->n_joints > RT_SKELETON_LDS_JOINTS) {
        rt_set_error("rt_crowd_create: a skeleton of %u joints: a crowd poses rigs of up to %u (the actor's world matrices stand in LDS; a larger rig is a skeleton of its own)",
                     sk->n_joints, RT_SKELETON_LDS_JOINTS);
        return RT_ERR_UNSUPPORTED;
    }
    rt_context *ctx = sk->ctx;
    rt_made<rt_crowd> c;
    RT_TRY(rt_make(ctx, c));
    c->is_crowd = true;
    c->sk = sk;
    rt_retain(sk);
    c->n_joints = sk->n_joints;
    c->n_poses = n_actors;
    const size_t joints = (size_t)n_actors * sk->n_joints;
    RT_TRY(rt_use_device(ctx));
    RT_TRY(c->pose.reserve(sizeof(float) * RT_SKELETON_POSE_FLOATS * joints));
    RT_TRY(c->joints.reserve(48 * joints));
    RT_TRY(c->palette.reserve(48 * joints));
    *out = c.release();
    return RT_OK;
}

// (a scene with instances attached to it, or a model posed from it, holds what it needs: the scene retains the crowd, and the last release
// joins the stream)
int rt_crowd_destroy(rt_crowd *c) { return rt_release(c); }

int rt_crowd_get_info(const rt_crowd *c, rt_skeleton **sk, uint32_t *n_actors, uint32_t *n_joints)
{
    RT_REQUIRE(c, "null crowd");
    if (sk) *sk = c->sk;
    if (n_actors) *n_actors = c->n_poses;
    if (n_joints) *n_joints = c->n_joints;
    return RT_OK;
}

int rt_crowd_set_poses(rt_crowd *c, const float *trs, uint32_t mem)
{
    RT_REQUIRE(c && trs, "null argument");
    RT_TRY(rt_pose_copy_in(c, "rt_crowd_set_poses", trs, mem));
    RT_TRY(pose_crowd(c, 0u));
    return rt_pose_join_host(c, mem);
}

int rt_crowd_set_blend(rt_crowd *c, uint32_t n_layers, const rt_skeleton_layer *layers)
{
    RT_REQUIRE(c && layers, "null argument");
    RT_TRY(check_layers(c, "rt_crowd_set_blend", n_layers, layers));
    return blend_crowd(c, n_layers, layers);
}

int rt_crowd_set_layout(rt_crowd *c, uint32_t n_layers, const rt_skeleton_layer *layers)
{
    RT_REQUIRE(c && layers, "null argument");
    if (n_layers < 1u || n_layers > RT_SKELETON_MAX_LAYERS) return check_layers(c, "rt_crowd_set_layout", n_layers, layers);     // (refuses, and reads no entry)
    rt_context *ctx = c->ctx;
    const rt_skeleton *sk = c->sk;
    const size_t n = (size_t)c->n_poses * n_layers;
    std::vector<rt_skeleton_layer> mine;                 // the caller's list without its times
    std::vector<rt_crowd_slot> slots;
    std::vector<rt_crowd_clip> clips;
    std::vector<const float *> masks;
    try {
        mine.resize(n);
        slots.resize(n);
        clips_and_masks(sk, clips, masks);
    } catch (const std::bad_alloc &) {
        rt_set_error("out of host memory");
        return RT_ERR_OOM;
    }
    rt_crowd_layout_layers(n, layers, mine.data());
    RT_TRY(check_layers(c, "rt_crowd_set_layout", n_layers, mine.data()));
    rt_crowd_pack_slots(c->n_poses, n_layers, mine.data(), clips.data(), masks.data(), slots.data());
    RT_TRY(rt_use_device(ctx));
    // a buffer of its own: a launch already queued reads the slots the crowd has, and a refusal here leaves them, and the layout, as they were
    DevBuf fresh;
    RT_TRY(rt_upload(ctx, fresh, slots.data(), sizeof(rt_crowd_slot) * n));
    HIP_TRY(hipStreamSynchronize(ctx->stream));         // (the vector goes out of scope, and nothing queued reads the old slots any more)
    c->slots = std::move(fresh);
    c->layout_layers = n_layers;
    c->layout_clip_gen = sk->clip_gen;
    c->layout_mask_gen = sk->mask_gen;
    return RT_OK;
}

int rt_crowd_get_layout(const rt_crowd *c, uint32_t *n_layers)
{
    RT_REQUIRE(c && n_layers, "null argument");
    *n_layers = c->layout_layers;
    return RT_OK;
}

int rt_crowd_set_blend_device(rt_crowd *c, const float *times, const float *weights)
{
    RT_REQUIRE(c && times, "null argument");
    if (c->layout_layers == 0u) {
        rt_set_error("rt_crowd_set_blend_device: the crowd has no layout (rt_crowd_set_layout gives it one)");
        return RT_ERR_STATE;
    }
    if (c->layout_clip_gen != c->sk->clip_gen || c->layout_mask_gen != c->sk->mask_gen) {
        rt_set_error("rt_crowd_set_blend_device: the layout is stale: the skeleton's %s were cleared after it was set (rt_crowd_set_layout sets a new one)",
                     c->layout_clip_gen != c->sk->clip_gen ? "clips" : "masks");
        return RT_ERR_STATE;
    }
    RT_TRY(rt_use_device(c->ctx));
    const CrowdDeviceSource src = {c->slots.as<rt_crowd_slot>(), times, weights};
    return pose_crowd(c, c->layout_layers, &src);
}

int rt_crowd_set_times(rt_crowd *c, const uint32_t *clips, const float *times)
{
    RT_REQUIRE(c && clips && times, "null argument");
    // the refusals of rt_skeleton_set_time, per actor: every actor's time before any actor's clip, the first bad actor first
    for (uint32_t a = 0; a < c->n_poses; a++)
        if (std::isnan(times[a])) {
            rt_set_error("rt_crowd_set_times: actor %u: the time is NaN", a);
            return RT_ERR_INVALID_ARG;
        }
    for (uint32_t a = 0; a < c->n_poses; a++)
        if (clips[a] >= c->sk->clips.size()) {
            rt_set_error("rt_crowd_set_times: actor %u: clip %u: the skeleton has %zu (rt_skeleton_add_clip adds one)", a, clips[a], c->sk->clips.size());
            return RT_ERR_STATE;
        }
    std::vector<rt_skeleton_layer> layers;
    try {
        layers.resize(c->n_poses);
    } catch (const std::bad_alloc &) {
        rt_set_error("out of host memory");
        return RT_ERR_OOM;
    }
    rt_crowd_layers_of_times(c->n_poses, clips, times, layers.data());
    return blend_crowd(c, 1u, layers.data());
}

int rt_crowd_read_pose(rt_crowd *c, uint32_t first_actor, uint32_t count, float *trs)
{
    RT_REQUIRE(c && trs, "null argument");
    return rt_pose_read_back(c, "rt_crowd_read_pose", c->pose, RT_SKELETON_POSE_FLOATS, first_actor, count, trs);
}

int rt_crowd_read_joints(rt_crowd *c, uint32_t first_actor, uint32_t count, float *world3x4)
{
    RT_REQUIRE(c && world3x4, "null argument");
    return rt_pose_read_back(c, "rt_crowd_read_joints", c->joints, 12, first_actor, count, world3x4);
}

int rt_crowd_read_palette(rt_crowd *c, uint32_t first_actor, uint32_t count, float *palette3x4)
{
    RT_REQUIRE(c && palette3x4, "null argument");
    return rt_pose_read_back(c, "rt_crowd_read_palette", c->palette, 12, first_actor, count, palette3x4);
}

int rt_crowd_get_joints_device_ptr(rt_crowd *c, void **ptr)
{
    RT_REQUIRE(c && ptr, "null argument");
    return rt_pose_device_ptr(c, "rt_crowd_get_joints_device_ptr", c->joints, ptr);
}

int rt_crowd_get_palette_device_ptr(rt_crowd *c, void **ptr)
{
    RT_REQUIRE(c && ptr, "null argument");
    return rt_pose_device_ptr(c, "rt_crowd_get_palette_device_ptr", c->palette, ptr);
}

int rt_model_set_bones_from_crowd(rt_model *m, rt_crowd *c, uint32_t actor)
{
    RT_REQUIRE(m && c, "null argument");
    if (actor >= c->n_poses) {
        rt_set_error("rt_model_set_bones_from_crowd: actor %u: the crowd has %u", actor, c->n_poses);
        return RT_ERR_INVALID_ARG;
    }
    return rt_pose_set_bones(m, c, actor, "rt_model_set_bones_from_crowd");
}

}  // extern "C"
