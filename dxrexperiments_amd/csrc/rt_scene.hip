// rt_scene.hip -- the scene: its instance list and masks, its TLAS, what says whether it is fresh, and its C-ABI entry points
// (include/dxr_amd.h).  Stand-in for libs/DXRFramework/RtScene and for what its build enqueues through the Fallback Layer:
//   RtScene::build  -> TopLevelASGenerator::Generate    -> BuildRaytracingAccelerationStructure
//       (libs/DXRFramework/RtScene.cpp:18-52, Helpers/TopLevelASGenerator.cpp:309-414)
// The tree builder it calls is the LBVH the BLAS uses (rt_lbvh.h, rt_bvh_build.hip).
#include <cstddef>
#include <cstring>
#include <new>

#include "rt_attach.h"
#include "rt_lbvh.h"
#include "rt_level_scan.h"
#include "rt_xform.h"

namespace {

// ---- fresh or stale: rt_scene's built, updatable, pending and masks_dirty, and the records' pending and seen_geom (rt_internal.h), are written
// ---- in this block, nowhere else ----

// rt_scene_add_model: the TLAS no longer stands for this instance list, only rt_scene_build brings the scene back
void scene_list_changed(rt_scene *s) { s->built = false; s->updatable = false; }

// instance i joins the list the next update rewrites (once)
void scene_mark_pending(rt_scene *s, uint32_t i) { if (!s->inst[i].pending) { s->inst[i].pending = true; s->pending.push_back(i); } }

// a setter has stored new transforms for `count` instances of an updatable scene
void scene_transforms_changed(rt_scene *s, uint32_t first, uint32_t count)
{
    for (uint32_t i = first; i < first + count; i++) scene_mark_pending(s, i);
    s->built = false;         // stale until rt_scene_update or rt_scene_build: nothing traces a half-applied state
}

// rt_scene_update has found the skeletons of these attached instances posed anew: they join the list, the scene is stale until it has succeeded
void scene_poses_changed(rt_scene *s, const std::vector<uint32_t> &posed)
{
    for (uint32_t i : posed) scene_mark_pending(s, i);
    if (!posed.empty()) s->built = false;
}

// a setter has changed some instance's visibility on an updatable scene: stale until rt_scene_update or rt_scene_build, as with a pending transform
void scene_masks_changed(rt_scene *s) { s->masks_dirty = true; s->built = false; }

// new vertices of one of the scene's models have been queued (never built, or instances added since: the next build reads them anyway)
void scene_vertices_changed(rt_scene *s) { if (s->updatable) s->built = false; }

// rt_scene_build is about to rewrite the records and the TLAS: if it fails from here on, only another build brings the scene back
void scene_build_begins(rt_scene *s) { s->updatable = false; }

// A build or an update has succeeded: every stored transform and mask has been read, and the vertices of the models of `changed` (an
// update: exactly the instances whose generation differed; nullptr, a build: of every instance).  Nothing is pending, the scene is fresh.
void scene_applied(rt_scene *s, const std::vector<uint32_t> *changed)
{
    // the attached instances it listed now stand where their skeleton's current pose puts them
    const auto listed = [](SceneInstance &in) { if (in.source == XfSource::Joint) in.seen_pose = in.src->pose_count; in.pending = false; };
    if (changed) {
        for (uint32_t i : s->pending) listed(s->inst[i]);
        for (uint32_t i : *changed) s->inst[i].seen_geom = s->inst[i].model->geom_gen;
    } else {
        for (SceneInstance &in : s->inst) { listed(in); in.seen_geom = in.model->geom_gen; }
        s->updatable = true;
    }
    s->pending.clear();
    s->masks_dirty = false;
    s->built = true;
}

// instances of an updatable scene whose model's vertices were set since the scene last wrote their records
size_t scene_changed_instances(const rt_scene *s, std::vector<uint32_t> *which = nullptr)
{
    size_t n = 0;
    if (!s->updatable) return 0;
    for (size_t i = 0; i < s->inst.size(); i++)
        if (s->inst[i].model->geom_gen != s->inst[i].seen_geom) { n++; if (which) which->push_back((uint32_t)i); }
    return n;
}

// ---- the instance list and its bindings: scene_add_instance lengthens the records and the binding mirrors (rt_internal.h), together; nothing else does ----

void scene_add_instance(rt_scene *s, rt_model *m, const float xform[12])
{
    SceneInstance in;                                  // (mask 0xFF: InstanceMask of the reference's descriptors, TopLevelASGenerator.cpp:361)
    in.model = m;
    memcpy(in.xform, xform, sizeof in.xform);
    s->inst.push_back(in);
    s->att_words.resize(s->inst.size(), 0u);
    s->att_local.resize(12 * s->inst.size(), 0.0f);
}

// instance i follows a joint of pose `actor` of src, a skeleton or a crowd (which the scene retains: rt_scene::sources); `word`: the binding
// as the device reads it (rt_attach.h) -- the actor is not in it: it is in the W pointer the device holds for the instance
void scene_bind(rt_scene *s, uint32_t i, rt_pose_source *src, uint32_t actor, uint32_t word)
{
    SceneInstance &in = s->inst[i];
    in.source = src ? XfSource::Joint : XfSource::Host; in.src = src; in.actor = actor; in.seen_pose = 0; s->att_words[i] = word;
}

// ... and no longer: it keeps the floats its last update or build gave it, which the host copy holds
void scene_unbind(rt_scene *s, uint32_t i) { scene_bind(s, i, nullptr, 0u, 0u); }

// attached instances of an updatable scene whose skeleton has been posed since the scene last applied it, and that are not pending already
void scene_posed_instances(const rt_scene *s, std::vector<uint32_t> &which)
{
    for (size_t i = 0; s->updatable && !s->sources.empty() && i < s->inst.size(); i++) {      // (no skeleton: nobody has ever been attached)
        const SceneInstance &in = s->inst[i];
        if (in.source == XfSource::Joint && !in.pending && in.src->posed && in.src->pose_count != in.seen_pose) which.push_back((uint32_t)i);
    }
}

// an update or a build composes every attached instance it lists from W: refused, with nothing changed, while some skeleton has no pose
int scene_require_poses(const rt_scene *s, const char *who)
{
    for (size_t i = 0; !s->sources.empty() && i < s->inst.size(); i++)
        if (s->inst[i].source == XfSource::Joint && !s->inst[i].src->posed) {
            rt_set_error("%s: instance %zu is attached to a %s that has no pose yet (%s)", who, i, s->inst[i].src->noun(), s->inst[i].src->pose_hint());
            return RT_ERR_STATE;
        }
    return RT_OK;
}

// a transform setter whose range holds an attached instance is refused: the joint says where it stands
int scene_refuse_attached(const rt_scene *s, const char *who, uint32_t first, uint32_t count)
{
    uint32_t i = 0;
    if (!rt_attach_range_holds(s->att_words.data(), s->att_words.size(), first, count, &i)) return RT_OK;
    if (s->inst[i].src && s->inst[i].src->is_crowd)
        rt_set_error("%s: instance %u is attached to joint %u of actor %u of a crowd, which gives it its transform (rt_scene_detach_instances lets it go)", who, i,
                     s->att_words[i] & RT_ATTACH_JOINT_MASK, s->inst[i].actor);
    else
        rt_set_error("%s: instance %u is attached to joint %u of a skeleton, which gives it its transform (rt_scene_detach_instances lets it go)", who, i,
                     s->att_words[i] & RT_ATTACH_JOINT_MASK);
    return RT_ERR_STATE;
}

// What d_xf holds for the device-held instances of a range, on its way to their host copies: theirs once the caller has joined the stream
// (*any: there is something to wait for), and they are host-sourced from here on
int scene_bring_down(rt_context *ctx, rt_scene *s, size_t first, size_t count, bool *any)
{
    for (size_t i = first; i < first + count; i++)
        if (s->inst[i].source == XfSource::Device) {
            HIP_TRY(hipMemcpyAsync(s->inst[i].xform, s->d_xf.as<float>() + 12 * i, 48, hipMemcpyDeviceToHost, ctx->stream));
            s->inst[i].source = XfSource::Host;
            *any = true;
        }
    return RT_OK;
}

// d_xf and the three binding arrays for ALL of the scene's instances (k_gather_transforms indexes them by instance): reserved once, and again
// only after rt_scene_add_model has made the list longer (DevBuf::reserve keeps no contents).  What d_xf held then comes down to the host
// copies first and those instances are host-sourced from there on -- the one place where a setter waits; the bindings go up again from their
// host mirrors and the records' skeletons, and a scene that has any waits for that too.  d_xf grows last: its size says that all four stand.
int scene_reserve_device(rt_context *ctx, rt_scene *s)
{
    const size_t n = s->inst.size();
    if (s->d_xf.bytes >= 48 * n) return RT_OK;
    bool held = false, bound = false;
    RT_TRY(scene_bring_down(ctx, s, 0, n, &held));
    if (held) HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<const float *> w_of(n, nullptr);
    for (size_t i = 0; i < n; i++)
        if (s->inst[i].source == XfSource::Joint) { w_of[i] = s->inst[i].src->w_of(s->inst[i].actor); bound = true; }
    RT_TRY(s->d_att_words.reserve(4 * n));
    RT_TRY(s->d_att_local.reserve(48 * n));
    RT_TRY(s->d_att_w.reserve(sizeof(const float *) * n));
    if (bound) {
        HIP_TRY(hipMemcpyAsync(s->d_att_words.p, s->att_words.data(), 4 * n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(s->d_att_local.p, s->att_local.data(), 48 * n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(s->d_att_w.p, w_of.data(), sizeof(const float *) * n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));     // (w_of goes out of scope; the mirrors are the host's to change again)
    } else      // nobody is attached: every word is 0, and the other two arrays are read for attached instances only
        HIP_TRY(hipMemsetAsync(s->d_att_words.p, 0, 4 * n, ctx->stream));
    return s->d_xf.reserve(48 * n);
}

// A scene whose transforms, instance masks or models' vertices were set and not applied yet: says so (the message names them, joined by " and ",
// and the setter of the first) and returns true.
bool scene_stale_error(const rt_scene *s, const char *who)
{
    if (!s || s->built) return false;
    const size_t changed = scene_changed_instances(s), moved = s->pending.size();
    const bool masks = s->updatable && s->masks_dirty;
    if (!changed && !moved && !masks) return false;
    char what[192];
    int at = 0;
    if (changed)
        at += snprintf(what + at, sizeof what - at, "new vertices of the model%s of %zu instance%s", changed == 1 ? "" : "s", changed, changed == 1 ? "" : "s");
    if (moved) at += snprintf(what + at, sizeof what - at, "%s%zu instance transform%s", at ? " and " : "", moved, moved == 1 ? "" : "s");
    if (masks) snprintf(what + at, sizeof what - at, "%sinstance masks", at ? " and " : "");
    rt_set_error("%s: %s pending (%s): rt_scene_update or rt_scene_build applies them", who, what,
                 changed ? "rt_model_set_vertices / _set_positions / _recompute_normals" : moved ? "rt_scene_set_instance_transform" : "rt_scene_set_instance_mask");
    return true;
}

// THE refusal of everything that needs a built scene: the message says what is pending or, if nothing is, `otherwise` (a format that may name
// `who` once)
int scene_refuse(const rt_scene *s, const char *who, const char *otherwise)
{
    if (!scene_stale_error(s, who)) rt_set_error(otherwise, who);
    return RT_ERR_STATE;
}

// the structure a lookup names: which < 0 the TLAS, else the BLAS of instance `which`'s model; nullptr: not built, or no such instance
const BvhDev *pick_bvh(const rt_scene *s, int which)
{
    if (!s || !s->built) return nullptr;
    if (which < 0) return &s->tlas;
    if ((size_t)which >= s->inst.size()) return nullptr;
    return &s->inst[which].model->blas;
}

// ... for the lookup `who`, which is refused (nullptr, the message set: return RT_ERR_STATE) if there is none; blas_only: or if it is the TLAS
const BvhDev *lookup_bvh(const rt_scene *s, int which, const char *who, bool blas_only = false)
{
    const BvhDev *b = pick_bvh(s, which);
    if (b && !(blas_only && which < 0)) return b;
    scene_refuse(s, who, "%s: scene not built or index out of range");
    return nullptr;
}

// `one`: the caller names a single instance, `first`, and its message says so
int scene_range_check(const rt_scene *s, const char *who, uint32_t first, uint32_t count, bool one = false)
{
    const size_t n = s->inst.size();
    if (first > n || count > n - first) {
        if (one) rt_set_error("%s: instance %u out of range: the scene has %zu", who, first, n);
        else rt_set_error("%s: instances %u .. %llu out of range: the scene has %zu", who, first, (unsigned long long)first + count, n);
        return RT_ERR_STATE;
    }
    return RT_OK;
}

// ---- instance masks (rt_scene_set_instance_mask): the TLAS over the visible sub-list ----
//
// Stands in for the InstanceMask member of the instance descriptors (libs/DXRFramework/Helpers/TopLevelASGenerator.cpp:344-362, always 0xFF
// there) under the inclusion mask 0xFF of every TraceRay of the reference.  `vis` holds the visible instances' indices in ascending order;
// the LBVH is built over vis.size() leaves, and wherever it names the j-th of them the TLAS names vis[j].

constexpr unsigned UPD_BLOCK = 256;

// sub-list position -> instance index, in the canonical leaves' `left` and the low words of the sorted keys (vis is increasing: the keys stay
// ascending).  k_lbvh_to_tree takes a TLAS leaf's code from `left`, so the four-wide layout comes out mapped
__global__ void __launch_bounds__(UPD_BLOCK) k_map_visible(rt_bvh_node *__restrict__ nodes, uint64_t *__restrict__ keys, const uint32_t *__restrict__ vis,
                                                          uint32_t n_vis)
{
    const uint32_t k = blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (k >= n_vis) return;
    const uint64_t key = keys[k];
    const uint32_t i = vis[(uint32_t)(key & 0xFFFFFFFFull)];
    keys[k] = (key & 0xFFFFFFFF00000000ull) | i;
    nodes[n_vis - 1 + k].left = i;
}

int map_visible_leaves(rt_context *ctx, rt_scene *s)
{
    const uint32_t nv = s->n_vis;
    k_map_visible<<<grid_for(nv, UPD_BLOCK), UPD_BLOCK, 0, ctx->stream>>>(s->tlas.nodes.as<rt_bvh_node>(), s->tlas.keys.as<uint64_t>(), s->d_vis.as<uint32_t>(), nv);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// room for the TLAS of all n instances, whatever part is visible at the build: an update that shows instances again allocates nothing
int reserve_tlas_for(BvhDev &bv, uint32_t n)
{
    RT_TRY(bv.nodes.reserve(sizeof(rt_bvh_node) * (2 * (size_t)n - 1)));
    RT_TRY(bv.keys.reserve(sizeof(uint64_t) * n));
    RT_TRY(bv.parents.reserve(sizeof(uint32_t) * (2 * (size_t)n - 1)));
    RT_TRY(bv.ranges.reserve(sizeof(uint2) * (n > 1 ? n - 1 : 1)));
    RT_TRY(bv.wide.reserve(sizeof(WNode) * (size_t)(n > 1 ? n - 1 : 1)));
    return RT_OK;
}

// the visible sub-list from the records' masks into s->vis / d_vis / n_vis, uploaded if it differs from the one the scene has (or `force`: a build,
// whose TLAS buffers may be new); RT_ERR_STATE, and nothing changed, if no instance is visible
int rt_scene_apply_masks(rt_context *ctx, rt_scene *s, const char *who, bool force)
{
    const uint32_t n = (uint32_t)s->inst.size();
    std::vector<uint32_t> vis;
    vis.reserve(n);
    for (uint32_t i = 0; i < n; i++)
        if (s->inst[i].mask) vis.push_back(i);
    if (vis.empty()) { rt_set_error("%s: no instance is visible: every instance mask is 0 (rt_scene_set_instance_mask)", who); return RT_ERR_STATE; }
    if (!force && vis == s->vis) return RT_OK;
    s->vis.swap(vis);                                  // (a member: alive whenever the copy runs)
    s->n_vis = (uint32_t)s->vis.size();
    if (s->n_vis == n) return RT_OK;                   // nothing hidden: nobody reads the list
    RT_TRY(s->d_vis.reserve(sizeof(uint32_t) * (size_t)n));       // (for all of them at once: never grows again)
    HIP_TRY(hipMemcpyAsync(s->d_vis.p, s->vis.data(), sizeof(uint32_t) * s->n_vis, hipMemcpyHostToDevice, ctx->stream));
    return RT_OK;
}

// ---- the TLAS: instance list -> records -> world boxes -> tree, ONE path for rt_scene_build and rt_scene_update ----
//
// rt_scene_update stands in for the generators' update path (libs/DXRFramework/Helpers/TopLevelASGenerator.h:144-163 `updateOnly`), which the
// reference's RtScene never calls.  The definition is "update == build", and it holds by construction: a build writes what only a build
// knows (the model part of every record, rt_build_tlas) and then IS an update with every instance pending (rt_update_tlas).  The canonical
// TLAS is a pure function of the instance boxes and every traversal returns the same bits on any tree, so the TLAS is
// always rebuilt -- into the scene's own buffers -- from boxes of which only the listed instances' are computed anew.  Only the listed
// transforms and their indices go up; the records are rewritten, and the work list of the world boxes is made, on the device.

// One lane per listed instance whose transform the device holds or makes (`idx`: their run of the listed indices, n of them; `pend_xf` and
// `back`: their run of the listed transforms and the copy that outlives the arena).  An attached instance (words[i] has RT_ATTACH_BOUND, rt_attach.h):
// T = W_joint o local by compose3x4, always multiplied, or T = W_joint bit for bit when it has no local matrix; T goes into the scene's device
// storage d_xf too, from where on it is a transform set from device memory.  Any other: the twelve floats d_xf holds for it.  A lane reads and
// writes the rows of its own instance only, and an instance is listed once.  The grid's last wave may be partial: these lanes meet nowhere.
__global__ void __launch_bounds__(UPD_BLOCK) k_gather_transforms(const uint32_t *__restrict__ idx, uint32_t n, const uint32_t *__restrict__ words,
                                                                 const float *__restrict__ local, const float *const *__restrict__ w_of, float *d_xf,
                                                                 float *__restrict__ pend_xf, float *__restrict__ back)
{
    const uint32_t k = blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = idx[k];
    const uint32_t word = words[i];                        // (the binding arrays cover every instance: scene_reserve_device)
    float T[12];
    if (word & RT_ATTACH_BOUND) {
        const float *W = w_of[i] + 12u * (size_t)(word & RT_ATTACH_JOINT_MASK);
        float A[12];
#pragma unroll
        for (int e = 0; e < 12; e++) A[e] = W[e];
        if (word & RT_ATTACH_LOCAL) {
            float B[12];
#pragma unroll
            for (int e = 0; e < 12; e++) B[e] = local[12u * (size_t)i + e];
            compose3x4(A, B, T);
        } else {
#pragma unroll
            for (int e = 0; e < 12; e++) T[e] = A[e];
        }
#pragma unroll
        for (int e = 0; e < 12; e++) d_xf[12u * (size_t)i + e] = T[e];
    } else {
#pragma unroll
        for (int e = 0; e < 12; e++) T[e] = d_xf[12u * (size_t)i + e];
    }
#pragma unroll
    for (int e = 0; e < 12; e++) {
        pend_xf[12u * (size_t)k + e] = T[e];
        back[12u * (size_t)k + e] = T[e];
    }
}

constexpr unsigned UPD_BACK_WORDS = 20;      // inv[12], wlo[3], root_code, whi[3], flags: the head of an InstanceRec
static_assert(offsetof(InstanceRec, flags) == 4 * (UPD_BACK_WORDS - 1), "the read-back of an update is the head of the record");

// One lane per listed instance: the transform part of its record -- the inverse (invert3x4, rt_xform.h), the identity flag and the (empty or
// BLAS) box; and the (slot, chunk of INST_BOX_REFS vertex references) work items of the transformed ones, compacted into `items`: a
// wave-wide prefix sum of the lanes' chunk counts, ONE atomic per wave that has any (a ballot says so), every lane then writes its own run.
// The order of the list depends on the order of the atomics; the boxes made from it do not (min / max).  max_items = the chunks of all
// listed instances, transformed or not: the host's bound of the list and the next launch's grid.
__global__ void __launch_bounds__(UPD_BLOCK) k_update_records(InstanceRec *__restrict__ inst, const float *__restrict__ blas_bounds,
                                                              const uint32_t *__restrict__ pend_idx, const float *__restrict__ pend_xf, uint32_t n_pending,
                                                              uint32_t *__restrict__ enc, uint2 *__restrict__ items, uint32_t *__restrict__ n_items,
                                                              uint32_t max_items)
{
    const uint32_t slot = blockIdx.x * UPD_BLOCK + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    uint32_t chunks = 0;
    if (slot < n_pending) {
        const uint32_t i = pend_idx[slot];
        float m[12], inv[12];
        for (int k = 0; k < 12; k++) m[k] = pend_xf[12u * (size_t)slot + k];
        const bool identity = is_identity3x4(m);
        InstanceRec &r = inst[i];
        if (identity)
            for (int k = 0; k < 12; k++) inv[k] = m[k];              // (the floats as given: a -0 stays one)
        else
            invert3x4(m, inv);
        const float inf = __uint_as_float(0x7f800000u);
        for (int k = 0; k < 12; k++) r.inv[k] = inv[k];
        for (int c = 0; c < 3; c++) {
            r.wlo[c] = identity ? blas_bounds[6u * (size_t)i + c] : inf;     // (a transformed instance: empty until k_update_apply)
            r.whi[c] = identity ? blas_bounds[6u * (size_t)i + 3 + c] : -inf;
            enc[6u * (size_t)slot + c] = ENC_POS_INF;                        // (one without triangles keeps the empty box)
            enc[6u * (size_t)slot + 3 + c] = ENC_NEG_INF;
        }
        r.flags = identity ? RT_INST_IDENTITY : 0u;
        if (!identity) chunks = (3u * r.n_prims + INST_BOX_REFS - 1u) / INST_BOX_REFS;
    }
    // (every lane of the block is here: the block is whole waves and nothing has returned)
    if (__ballot(chunks != 0u) == 0ull) return;        // wave-uniform
    const uint32_t incl = rt_scan::wave_inclusive(chunks);
    const uint32_t total = __shfl(incl, 63, 64);
    uint32_t base = 0;
    if (lane == 63u) base = atomicAdd(n_items, total);
    base = __shfl(base, 63, 64);
    const uint32_t first = base + (incl - chunks);
    for (uint32_t c = 0; c < chunks; c++)
        if (first + c < max_items) items[first + c] = make_uint2(slot, c);
}

// the boxes into the records of the listed transformed instances (identity instances keep the box of their BLAS); the head of every listed
// record into the read-back for h_inst
__global__ void k_update_apply(InstanceRec *__restrict__ inst, const uint32_t *__restrict__ pend_idx, uint32_t n_pending,
                               const uint32_t *__restrict__ enc, uint32_t *__restrict__ back)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_pending) return;
    InstanceRec &r = inst[pend_idx[slot]];
    if (!(r.flags & RT_INST_IDENTITY))
        for (int c = 0; c < 3; c++) { r.wlo[c] = f_dec(enc[6u * (size_t)slot + c]); r.whi[c] = f_dec(enc[6u * (size_t)slot + 3 + c]); }
    const uint32_t *head = reinterpret_cast<const uint32_t *>(&r);
    for (unsigned k = 0; k < UPD_BACK_WORDS; k++) back[UPD_BACK_WORDS * (size_t)slot + k] = head[k];
}

// the world box of every visible instance, as it stands in its record (an untouched one's too) -> the TLAS builder's leaf boxes; vis == nullptr:
// nothing is hidden, position j is instance j.  Read from the RECORDS, which nobody writes here: `boxes` may still hold another list's
__global__ void __launch_bounds__(UPD_BLOCK) k_leaf_boxes(const InstanceRec *__restrict__ inst, const uint32_t *__restrict__ vis, uint32_t n_vis,
                                                         Box6 *__restrict__ boxes)
{
    const uint32_t j = blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (j >= n_vis) return;
    const InstanceRec &r = inst[vis ? vis[j] : j];
    for (int c = 0; c < 3; c++) { boxes[j].lo[c] = r.wlo[c]; boxes[j].hi[c] = r.whi[c]; }
}

// The model part of an instance record: what the record says about its model.  A build writes it for every instance; after a deformed
// model's BLAS has been rebuilt (rt_scene_update) DevBuf::reserve may have moved any of the arrays, and n_recs and the reference buffers
// come and go with the shape.  The field list stands twice: in model_desc and in write_model_part.
struct ModelDesc {
    const WNode *wide;
    const TriRec *tris;
    const rt_bvh_node *cnodes;
    const rt_vertex *verts;
    const uint32_t *indices;
    const TriRec *normals;
    const float *rec_boxes;
    const uint32_t *ref_off;
    const float *ref_boxes;
    int root_code;
    uint32_t n_prims, n_recs;
    float bounds[6];             // the BLAS box: the instance's row of blas_bounds
    uint32_t pad_;
};
static_assert(sizeof(ModelDesc) % 8 == 0, "an array of descriptors keeps its pointers aligned");

ModelDesc model_desc(const rt_model *m)
{
    ModelDesc d;
    d.wide = m->blas.wide.as<WNode>();
    d.tris = m->tris.as<TriRec>();
    d.cnodes = m->blas.nodes.as<rt_bvh_node>();
    d.verts = m->d_verts.as<rt_vertex>();
    d.indices = m->d_idx.as<uint32_t>();
    d.normals = m->normals.as<TriRec>();
    d.rec_boxes = m->rec_boxes.p ? m->rec_boxes.as<float>() : nullptr;
    d.ref_off = m->ref_off.p ? m->ref_off.as<uint32_t>() : nullptr;
    d.ref_boxes = m->ref_boxes.p ? m->ref_boxes.as<float>() : nullptr;
    d.root_code = m->blas.root_code;
    d.n_prims = m->n_tris;
    d.n_recs = m->n_recs;
    memcpy(d.bounds, m->blas.bounds, sizeof d.bounds);
    d.pad_ = 0;
    return d;
}

// ... into a record and the instance's row of the BLAS boxes (device: d_inst / blas_bounds; host: h_inst / h_blas_bounds)
__host__ __device__ inline void write_model_part(InstanceRec &r, float *bounds_row, const ModelDesc &d)
{
    r.wide = d.wide; r.tris = d.tris; r.cnodes = d.cnodes; r.verts = d.verts; r.indices = d.indices; r.normals = d.normals;
    r.rec_boxes = d.rec_boxes; r.ref_off = d.ref_off; r.ref_boxes = d.ref_boxes;
    r.root_code = d.root_code; r.n_prims = d.n_prims; r.n_recs = d.n_recs;
    for (int c = 0; c < 6; c++) bounds_row[c] = d.bounds[c];
}

// one lane per affected instance: who = (instance, descriptor)
__global__ void k_update_model_fields(InstanceRec *__restrict__ inst, float *__restrict__ blas_bounds, const ModelDesc *__restrict__ desc,
                                      const uint2 *__restrict__ who, uint32_t n)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = who[k].x;
    write_model_part(inst[i], blas_bounds + 6u * (size_t)i, desc[who[k].y]);
}

// The temporaries of a TLAS build: the LBVH's (rt_lbvh.h) + the listed indices and transforms, their encoded boxes, the work list and its
// count.  LIFETIME: the phases of a build share the arena -- lbvh_from_boxes reads these slices, then rt_build_wide_from_lbvh (as the PLOC
// phase of a BLAS) carves the SAME arena again from its start.  So nothing here may be read behind the wide collapse: whatever has to outlive
// it, as the record heads on their way to h_inst do, lives in a buffer of the scene's own (rt_scene::update_back).
struct TlasTemps : LbvhTemps {
    uint32_t *pend_idx;
    float *pend_xf;
    uint32_t *pend_enc;
    uint2 *items;
    uint32_t *n_items;
};
void carve_tlas(Carver &c, uint32_t n, size_t n_pending, size_t max_items, TlasTemps &t)
{
    carve_lbvh(c, n, t);
    t.pend_idx = c.take<uint32_t>(n_pending);
    t.pend_xf = c.take<float>(12 * n_pending);
    t.pend_enc = c.take<uint32_t>(6 * n_pending);
    t.items = c.take<uint2>(max_items);
    t.n_items = c.take<uint32_t>(1);
}

// the model fields of the records of `changed` (instances whose model was rebuilt) and their rows of blas_bounds, on the device; h_inst follows
int rt_update_model_records(rt_context *ctx, rt_scene *s, const std::vector<uint32_t> &changed)
{
    hipStream_t st = ctx->stream;
    std::vector<const rt_model *> models;              // the distinct models of `changed` (a handful: a linear search)
    std::vector<uint2> who(changed.size());
    for (size_t k = 0; k < changed.size(); k++) {
        const rt_model *m = s->inst[changed[k]].model;
        size_t at = 0;
        while (at < models.size() && models[at] != m) at++;
        if (at == models.size()) models.push_back(m);
        who[k] = make_uint2(changed[k], (uint32_t)at);
    }
    std::vector<ModelDesc> desc(models.size());
    for (size_t k = 0; k < models.size(); k++) desc[k] = model_desc(models[k]);
    // the table and the list go up through a slice of the build arena: the update that follows carves the arena again, behind this kernel on
    // the stream
    const size_t desc_bytes = (sizeof(ModelDesc) * desc.size() + 255) & ~(size_t)255;
    RT_TRY(ctx->build_arena.reserve(desc_bytes + sizeof(uint2) * who.size()));
    ModelDesc *d_desc = ctx->build_arena.as<ModelDesc>();
    uint2 *d_who = (uint2 *)(ctx->build_arena.as<char>() + desc_bytes);
    HIP_TRY(hipMemcpyAsync(d_desc, desc.data(), sizeof(ModelDesc) * desc.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_who, who.data(), sizeof(uint2) * who.size(), hipMemcpyHostToDevice, st));
    k_update_model_fields<<<grid_for(who.size(), UPD_BLOCK), UPD_BLOCK, 0, st>>>(s->d_inst.as<InstanceRec>(), s->blas_bounds.as<float>(), d_desc, d_who,
                                                                                (uint32_t)who.size());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));                 // (the host vectors go out of scope; a reserve of the arena by the update frees this slice)
    for (size_t k = 0; k < changed.size(); k++)        // the host mirrors follow
        write_model_part(s->h_inst[changed[k]], &s->h_blas_bounds[6 * (size_t)changed[k]], desc[who[k].y]);
    return RT_OK;
}

// The listed instances in two runs: first those whose transform the host holds (returns how many), whose floats go up as they always did; then
// those whose transform the device holds or makes, whose slots k_gather_transforms fills.  The slot order decides nothing (k_update_records).
size_t partition_by_source(const rt_scene *s, const std::vector<uint32_t> &listed, std::vector<uint32_t> &list)
{
    std::vector<uint32_t> rest;
    list.reserve(listed.size());
    for (uint32_t i : listed) (s->inst[i].source == XfSource::Host ? list : rest).push_back(i);
    const size_t nh = list.size();
    list.insert(list.end(), rest.begin(), rest.end());
    return nh;
}

// Everything an update queues, and its one join: the transforms of `list` (nh of them from the host: partition_by_source) into their records
// and world boxes, the TLAS over the visible instances, the read-backs.  It creates no event and reads no time; `queued` (or nullptr) is the
// caller's event, which it records behind the wide collapse, in front of the read-back: where update_ms ends
int queue_tlas_update(rt_context *ctx, rt_scene *s, const std::vector<uint32_t> &list, size_t nh, const char *who, hipEvent_t queued)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)s->inst.size();
    const size_t np = list.size(), nd = np - nh;
    std::vector<float> xf(12 * nh);                    // (alive, as list is, until the last synchronisation below)
    size_t max_items = 0;
    for (size_t k = 0; k < np; k++) {
        const SceneInstance &in = s->inst[list[k]];
        if (k < nh) memcpy(&xf[12 * k], in.xform, 12 * sizeof(float));
        max_items += (3 * (size_t)in.model->n_tris + INST_BOX_REFS - 1) / INST_BOX_REFS;
    }
    if (max_items > 0x7fffffffu) { rt_set_error("%s: %zu work items for the world boxes: the limit is 2^31 - 1", who, max_items); return RT_ERR_UNSUPPORTED; }
    TlasTemps t;
    RT_TRY(take_build_temps(ctx, n, t, [n, np, max_items](Carver &c, TlasTemps &tt) { carve_tlas(c, n, np, max_items, tt); }));
    // for all n at once, whatever part is listed or visible: allocated by a build, never again by an update
    RT_TRY(reserve_tlas_for(s->tlas, n));
    RT_TRY(s->update_back.reserve(sizeof(uint32_t) * UPD_BACK_WORDS * (size_t)n));
    std::vector<uint32_t> back(UPD_BACK_WORDS * np);
    std::vector<float> back_xf(12 * nd);
    if (nd) RT_TRY(s->xf_back.reserve(48 * (size_t)n));
    InstanceRec *inst = s->d_inst.as<InstanceRec>();
    if (np) {                                          // (none: an update of masks alone)
        HIP_TRY(hipMemcpyAsync(t.pend_idx, list.data(), np * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (nh) HIP_TRY(hipMemcpyAsync(t.pend_xf, xf.data(), xf.size() * sizeof(float), hipMemcpyHostToDevice, st));
        if (nd) {
            k_gather_transforms<<<grid_for(nd, UPD_BLOCK), UPD_BLOCK, 0, st>>>(t.pend_idx + nh, (uint32_t)nd, s->d_att_words.as<uint32_t>(),
                                                                              s->d_att_local.as<float>(), (const float *const *)s->d_att_w.p,
                                                                              s->d_xf.as<float>(), t.pend_xf + 12 * nh, s->xf_back.as<float>());
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemsetAsync(t.n_items, 0, sizeof(uint32_t), st));
        k_update_records<<<grid_for(np, UPD_BLOCK), UPD_BLOCK, 0, st>>>(inst, s->blas_bounds.as<float>(), t.pend_idx, t.pend_xf, (uint32_t)np, t.pend_enc,
                                                                       t.items, t.n_items, (uint32_t)max_items);
        if (max_items) lbvh_queue_instance_boxes(ctx, (uint32_t)max_items, inst, t.pend_idx, t.pend_xf, t.items, t.n_items, t.pend_enc);
        k_update_apply<<<grid_for(np, UPD_BLOCK), UPD_BLOCK, 0, st>>>(inst, t.pend_idx, (uint32_t)np, t.pend_enc, s->update_back.as<uint32_t>());
    }
    // the records are the full list's, hidden instances' included; the leaves are the visible ones' (all n when nothing is hidden)
    const uint32_t nv = s->n_vis;
    k_leaf_boxes<<<grid_for(nv, UPD_BLOCK), UPD_BLOCK, 0, st>>>(inst, nv < n ? s->d_vis.as<uint32_t>() : nullptr, nv, t.boxes);
    lbvh_queue_box_bounds(ctx, nv, t);
    RT_TRY(lbvh_from_boxes(ctx, s->tlas, nv, t));
    if (nv < n) RT_TRY(map_visible_leaves(ctx, s));
    // the TLAS is walked in the same four-wide layout (a single instance: the root is the leaf of that instance)
    RT_TRY(rt_build_wide_from_lbvh(ctx, s->tlas, true, 1));
    if (nv < n && nv == 1) s->tlas.root_code = ~(int)s->vis[0];       // (the one visible instance's own index)
    if (queued) HIP_TRY(hipEventRecord(queued, st));
    // the final join: it brings back the rewritten records' heads with the TLAS' depth and bounds
    if (np) HIP_TRY(hipMemcpyAsync(back.data(), s->update_back.p, back.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    // ... and, with them, the transforms the device held or made: the host copy follows here, behind everything queued
    if (nd) HIP_TRY(hipMemcpyAsync(back_xf.data(), s->xf_back.p, back_xf.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    RT_TRY(lbvh_collect(ctx, s->tlas));
    for (size_t k = 0; k < np; k++) memcpy((void *)&s->h_inst[list[k]], &back[UPD_BACK_WORDS * k], sizeof(uint32_t) * UPD_BACK_WORDS);
    for (size_t k = 0; k < nd; k++) {
        SceneInstance &in = s->inst[list[nh + k]];
        memcpy(in.xform, &back_xf[12 * k], 12 * sizeof(float));
        if (in.source == XfSource::Device) in.source = XfSource::Host;      // (d_xf holds the same floats: either source serves the next update)
    }
    return RT_OK;
}

// the scene's summary, taken again over all models: a deformation changes depths and can create or remove split references
int take_scene_summary(rt_context *ctx, rt_scene *s, const char *who, size_t n_listed)
{
    const uint32_t n = (uint32_t)s->inst.size();
    uint32_t deepest = 0, canon = s->tlas.max_depth;
    s->has_refs = false;
    for (uint32_t i = 0; i < n; i++) {
        const rt_model *m = s->inst[i].model;
        const BvhDev &b = m->blas;
        deepest = b.fast_depth > deepest ? b.fast_depth : deepest;
        canon = b.max_depth > canon ? b.max_depth : canon;
        s->has_refs = s->has_refs || m->ref_off.p != nullptr;
    }
    // a step leaves at most three siblings behind; two-level walks add the TLAS path and the sentinel that marks the
    // bottom of a BLAS walk
    s->two_level = !(n == 1 && (s->h_inst[0].flags & RT_INST_IDENTITY));
    s->stack_need = s->two_level ? s->tlas.fast_depth + 1 + deepest : deepest;
    // the canonical traversal (parity / counting kernels and the deep-stack path of the fast one) keeps
    // 128-entry private stacks per structure
    if (canon >= 127) { rt_set_error("acceleration structure %u levels deep: the limit is 126", canon); return RT_ERR_UNSUPPORTED; }
    if (ctx->verbose)
        fprintf(stderr, "[dxr_amd] %s: TLAS update, %zu of %u instances, %u visible, depth %u; deepest BLAS layout depth %u (%s); stack need %u; %s walk\n",
                who, n_listed, n, s->n_vis, s->tlas.max_depth, deepest, ctx->use_ploc ? "PLOC" : "LBVH", s->stack_need, s->two_level ? "two-level" : "single-level");
    return RT_OK;
}

// THE TLAS path of a build (listed: every instance, 0 .. n-1) and of an update (s->pending): the listed instances' records and world boxes,
// the TLAS over the visible instances, the scene's summary.  `who` names the caller in messages; `queued`: queue_tlas_update
int rt_update_tlas(rt_context *ctx, rt_scene *s, const std::vector<uint32_t> &listed, const char *who, hipEvent_t queued)
{
    // (the device storage first: should the list have grown since, what d_xf held comes down and is host-sourced in the partition)
    bool from_device = false;                          // (a scene without device storage has no such instance)
    for (size_t k = 0; s->d_xf.bytes && !from_device && k < listed.size(); k++) from_device = s->inst[listed[k]].source != XfSource::Host;
    if (from_device) RT_TRY(scene_reserve_device(ctx, s));
    std::vector<uint32_t> list;
    const size_t nh = partition_by_source(s, listed, list);
    RT_TRY(queue_tlas_update(ctx, s, list, nh, who, queued));
    return take_scene_summary(ctx, s, who, list.size());
}

// the build's share of the TLAS: the model part of every record and the per-instance BLAS boxes, written on the host and uploaded; then
// rt_update_tlas with every instance listed
int rt_build_tlas(rt_context *ctx, rt_scene *s)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)s->inst.size();
    s->h_inst.assign(n, InstanceRec());                // (the build's output, as vis is: one entry per instance of an updatable scene)
    s->h_blas_bounds.resize(6 * (size_t)n);            // (members: alive whenever the copies run)
    std::vector<uint32_t> all(n);                      // (alive until rt_update_tlas has joined the stream)
    for (uint32_t i = 0; i < n; i++) {
        InstanceRec &r = s->h_inst[i];
        write_model_part(r, &s->h_blas_bounds[6 * (size_t)i], model_desc(s->inst[i].model));
        r.pad_ = 0;
        r.material = i;
        all[i] = i;
    }
    RT_TRY(s->d_inst.reserve(sizeof(InstanceRec) * (size_t)n));
    RT_TRY(s->blas_bounds.reserve(6 * (size_t)n * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(s->d_inst.p, s->h_inst.data(), sizeof(InstanceRec) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->blas_bounds.p, s->h_blas_bounds.data(), 6 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    return rt_update_tlas(ctx, s, all, "rt_scene_build", nullptr);
}

}  // namespace

// ---- what the rest of the library asks of a scene (rt_internal.h) ----

rt_scene::~rt_scene()
{
    for (SceneInstance &in : inst) {
        std::vector<rt_scene *> &held = in.model->scenes;      // (the model outlives this: the scene retains it)
        for (size_t k = 0; k < held.size(); k++)
            if (held[k] == this) { held.erase(held.begin() + k); break; }
        rt_model_destroy(in.model);
    }
    for (rt_pose_source *src : sources) (void)rt_release(src);     // (joins the stream when the scene held the last reference)
}

void rt_scene_model_changed(rt_scene *s) { scene_vertices_changed(s); }

int rt_scene_require_built(const rt_scene *s, const char *who, const char *not_built)
{
    return s && s->built ? RT_OK : scene_refuse(s, who, not_built);
}

// ---- the C-ABI entry points ----

extern "C" {

int rt_scene_create(rt_context *ctx, rt_scene **out)
{
    RT_REQUIRE(ctx && out, "null argument");
    rt_made<rt_scene> s;
    RT_TRY(rt_make(ctx, s));
    *out = s.release();
    return RT_OK;
}

int rt_scene_add_model(rt_scene *s, rt_model *m, const float transform3x4[12])
{
    RT_REQUIRE(s && m && transform3x4, "null argument");
    RT_REQUIRE(m->ctx == s->ctx, "model and scene belong to different contexts");
    RT_TRY(rt_context_flush_deferred(s->ctx));       // frames accepted before this change see the scene as it was
    rt_retain(m);
    scene_add_instance(s, m, transform3x4);
    bool held = false;
    for (rt_scene *o : m->scenes) held = held || o == s;
    if (!held) m->scenes.push_back(s);
    scene_list_changed(s);
    s->generation++;
    return RT_OK;
}

int rt_scene_set_instance_transforms(rt_scene *s, uint32_t first, uint32_t count, const float *transforms3x4)
{
    RT_REQUIRE(s && (transforms3x4 || count == 0), "null argument");
    RT_TRY(scene_range_check(s, "rt_scene_set_instance_transforms", first, count));
    if (count == 0) return RT_OK;
    RT_TRY(scene_refuse_attached(s, "rt_scene_set_instance_transforms", first, count));
    RT_TRY(rt_context_flush_deferred(s->ctx));       // frames accepted before this change see the scene as it was
    for (uint32_t k = 0; k < count; k++) {
        memcpy(s->inst[first + k].xform, transforms3x4 + 12 * (size_t)k, sizeof s->inst[0].xform);
        s->inst[first + k].source = XfSource::Host;      // (none of them is attached: the host holds it again)
    }
    if (s->updatable) scene_transforms_changed(s, first, count);      // (never built, or instances added since: the next build reads the stored transforms)
    return RT_OK;
}

int rt_scene_set_instance_transform(rt_scene *s, uint32_t instance, const float transform3x4[12])
{
    RT_REQUIRE(s && transform3x4, "null argument");
    RT_TRY(scene_range_check(s, __func__, instance, 1, true));
    return rt_scene_set_instance_transforms(s, instance, 1, transform3x4);
}

// EXTENSION: the Transform member of the instance descriptors (TopLevelASGenerator.cpp:344-362) from device memory: the floats stay where they
// are until the update's kernels read them (k_gather_transforms)
int rt_scene_set_instance_transforms_mem(rt_scene *s, uint32_t first, uint32_t count, const float *transforms3x4, uint32_t mem)
{
    RT_REQUIRE(s && (transforms3x4 || count == 0), "null argument");
    RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, "unknown memory selector");
    if (mem == RT_MEM_HOST) return rt_scene_set_instance_transforms(s, first, count, transforms3x4);
    RT_TRY(scene_range_check(s, __func__, first, count));
    if (count == 0) return RT_OK;
    RT_TRY(scene_refuse_attached(s, __func__, first, count));
    rt_context *ctx = s->ctx;
    RT_TRY(rt_use_device(ctx));
    RT_TRY(rt_context_flush_deferred(ctx));          // frames accepted before this change see the scene as it was
    RT_TRY(scene_reserve_device(ctx, s));
    // (ordered on the context's stream: the caller's array is its own again once the stream has passed this copy)
    HIP_TRY(hipMemcpyAsync(s->d_xf.as<float>() + 12 * (size_t)first, transforms3x4, 48 * (size_t)count, hipMemcpyDeviceToDevice, ctx->stream));
    for (uint32_t k = 0; k < count; k++) s->inst[first + k].source = XfSource::Device;      // (none of them is attached)
    if (s->updatable) scene_transforms_changed(s, first, count);      // (never built, or instances added since: the next build reads the stored transforms)
    return RT_OK;
}

int rt_scene_get_instance_transforms(const rt_scene *s, uint32_t first, uint32_t count, float *transforms3x4)
{
    RT_REQUIRE(s && (transforms3x4 || count == 0), "null argument");
    RT_TRY(scene_range_check(s, __func__, first, count));
    bool waits = false;
    for (uint32_t k = 0; k < count;) {
        if (s->inst[first + k].source != XfSource::Device) {
            memcpy(transforms3x4 + 12 * (size_t)k, s->inst[first + k].xform, 48);
            k++;
            continue;
        }
        uint32_t run = 1;                              // device-held ones come down run by run, on demand
        while (k + run < count && s->inst[first + k + run].source == XfSource::Device) run++;
        if (!waits) RT_TRY(rt_use_device(s->ctx));
        HIP_TRY(hipMemcpyAsync(transforms3x4 + 12 * (size_t)k, s->d_xf.as<float>() + 12 * (size_t)(first + k), 48 * (size_t)run, hipMemcpyDeviceToHost,
                               s->ctx->stream));
        waits = true;
        k += run;
    }
    if (waits) HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    return RT_OK;
}

// Attaches instances first .. first + count - 1 to joints[k] of pose actors[k] (nullptr: pose 0, a skeleton's only one) of `src`; `what`
// names the kind of source in the messages.  Both entry points below are this.
static int scene_attach(rt_scene *s, const char *who, const char *what, uint32_t first, uint32_t count, rt_pose_source *src, const uint32_t *actors,
                        const uint32_t *joints, const float *local3x4)
{
    uint32_t bad = 0;
    switch (rt_attach_validate((uint32_t)s->inst.size(), first, count, src->n_joints, joints, &bad)) {
    case 0: break;
    case 1: rt_set_error("%s: null argument", who); return RT_ERR_INVALID_ARG;
    case 2: return scene_range_check(s, who, first, count);
    default:
        rt_set_error("%s: entry %u names joint %u: the %s has %u", who, bad, joints[bad], what, src->n_joints);
        return RT_ERR_INVALID_ARG;
    }
    for (uint32_t k = 0; actors && k < count; k++)
        if (actors[k] >= src->n_poses) {
            rt_set_error("%s: entry %u names actor %u: the %s has %u", who, k, actors[k], what, src->n_poses);
            return RT_ERR_INVALID_ARG;
        }
    if (src->ctx != s->ctx) { rt_set_error("%s: the scene and the %s belong to different contexts", who, what); return RT_ERR_STATE; }
    if (count == 0) return RT_OK;
    rt_context *ctx = s->ctx;
    RT_TRY(rt_use_device(ctx));
    RT_TRY(rt_context_flush_deferred(ctx));          // frames accepted before this change see the scene as it was
    // the device first -- the only steps that can refuse -- then, behind the wait, the host: nothing changes if the device refuses
    RT_TRY(scene_reserve_device(ctx, s));              // (where the composed transforms will stand, and the bindings of every instance)
    std::vector<uint32_t> words(count);
    std::vector<const float *> w_of(count, src->w_of(0));
    for (uint32_t k = 0; actors && k < count; k++) w_of[k] = src->w_of(actors[k]);
    rt_attach_pack(count, joints, local3x4 != nullptr, words.data());
    HIP_TRY(hipMemcpyAsync(s->d_att_words.as<uint32_t>() + first, words.data(), 4 * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    if (local3x4)                                      // (without one the rows stay: nobody reads them)
        HIP_TRY(hipMemcpyAsync(s->d_att_local.as<float>() + 12 * (size_t)first, local3x4, 48 * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync((const float **)s->d_att_w.p + first, w_of.data(), sizeof(const float *) * count, hipMemcpyHostToDevice, ctx->stream));
    bool held = false;                                 // (one set from device memory and not applied yet keeps those floats until an update)
    RT_TRY(scene_bring_down(ctx, s, first, count, &held));
    HIP_TRY(hipStreamSynchronize(ctx->stream));         // (the vectors go out of scope, the caller's arrays are its own again)
    held = false;
    for (rt_pose_source *o : s->sources) held = held || o == src;
    if (!held) { s->sources.push_back(src); rt_retain(src); }      // (as the scene retains its models; let go of when the scene goes)
    if (local3x4) memcpy(&s->att_local[12 * (size_t)first], local3x4, 48 * (size_t)count);
    for (uint32_t k = 0; k < count; k++) scene_bind(s, first + k, src, actors ? actors[k] : 0u, words[k]);
    if (s->updatable) scene_transforms_changed(s, first, count);      // (never built, or instances added since: the next build reads the binding)
    return RT_OK;
}

int rt_scene_attach_instances(rt_scene *s, uint32_t first, uint32_t count, rt_skeleton *sk, const uint32_t *joints, const float *local3x4)
{
    RT_REQUIRE(s && sk && (joints || count == 0), "null argument");
    return scene_attach(s, "rt_scene_attach_instances", "skeleton", first, count, sk, nullptr, joints, local3x4);
}

int rt_scene_attach_instances_crowd(rt_scene *s, uint32_t first, uint32_t count, rt_crowd *c, const uint32_t *actors, const uint32_t *joints,
                                    const float *local3x4)
{
    RT_REQUIRE(s && c && ((actors && joints) || count == 0), "null argument");
    static const uint32_t none = 0;                     // (count == 0 with a null `actors`: nothing is read)
    return scene_attach(s, "rt_scene_attach_instances_crowd", "crowd", first, count, c, actors ? actors : &none, joints, local3x4);
}

int rt_scene_detach_instances(rt_scene *s, uint32_t first, uint32_t count)
{
    RT_REQUIRE(s, "null scene");
    RT_TRY(scene_range_check(s, __func__, first, count));
    uint32_t from = 0, last = 0;
    if (!rt_attach_range_holds(s->att_words.data(), s->att_words.size(), first, count, &from)) return RT_OK;      // none attached: nothing to do
    RT_TRY(rt_use_device(s->ctx));
    for (uint32_t i = from; i < first + count; i++)
        if (s->inst[i].source == XfSource::Joint) { scene_unbind(s, i); last = i; }
    // from the first attached one to the last, which the device arrays cover whatever has been added since (a word of 0 is "not attached")
    HIP_TRY(hipMemsetAsync(s->d_att_words.as<uint32_t>() + from, 0, 4 * (size_t)(last - from + 1), s->ctx->stream));
    return RT_OK;
}

int rt_scene_get_instance_attachment(const rt_scene *s, uint32_t instance, rt_skeleton **sk, uint32_t *joint)
{
    RT_REQUIRE(s, "null scene");
    RT_TRY(scene_range_check(s, __func__, instance, 1, true));
    const bool bound = s->inst[instance].source == XfSource::Joint && !s->inst[instance].src->is_crowd;      // (a crowd's: rt_scene_get_instance_crowd_attachment)
    if (sk) *sk = bound ? static_cast<rt_skeleton *>(s->inst[instance].src) : nullptr;
    if (joint) *joint = bound ? s->att_words[instance] & RT_ATTACH_JOINT_MASK : 0u;
    return RT_OK;
}

int rt_scene_get_instance_crowd_attachment(const rt_scene *s, uint32_t instance, rt_crowd **c, uint32_t *actor, uint32_t *joint)
{
    RT_REQUIRE(s, "null scene");
    RT_TRY(scene_range_check(s, __func__, instance, 1, true));
    const bool bound = s->inst[instance].source == XfSource::Joint && s->inst[instance].src->is_crowd;
    if (c) *c = bound ? static_cast<rt_crowd *>(s->inst[instance].src) : nullptr;
    if (actor) *actor = bound ? s->inst[instance].actor : 0u;
    if (joint) *joint = bound ? s->att_words[instance] & RT_ATTACH_JOINT_MASK : 0u;
    return RT_OK;
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
        visibility = visibility || ((s->inst[first + k].mask != 0) != (masks[k] != 0));
        s->inst[first + k].mask = masks[k];
    }
    // (not built: the next build reads the stored masks; the same visibility: only the bytes change)
    if (s->updatable && visibility) scene_masks_changed(s);
    return RT_OK;
}

int rt_scene_set_instance_mask(rt_scene *s, uint32_t instance, uint8_t mask)
{
    RT_REQUIRE(s, "null scene");
    RT_TRY(scene_range_check(s, __func__, instance, 1, true));
    return rt_scene_set_instance_masks(s, instance, 1, &mask);
}

int rt_scene_get_instance_masks(const rt_scene *s, uint32_t first, uint32_t count, uint8_t *masks)
{
    RT_REQUIRE(s && (masks || count == 0), "null argument");
    RT_TRY(scene_range_check(s, "rt_scene_get_instance_masks", first, count));
    for (uint32_t k = 0; k < count; k++) masks[k] = s->inst[first + k].mask;
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
    scene_changed_instances(s, &changed);
    std::vector<uint32_t> posed;                      // attached instances whose skeleton has been posed since the scene last applied it
    scene_posed_instances(s, posed);
    if (s->pending.empty() && changed.empty() && !s->masks_dirty && posed.empty()) return RT_OK;      // nothing to apply: nothing launched, the generation stays
    rt_context *ctx = s->ctx;
    RT_TRY(rt_use_device(ctx));
    RT_TRY(rt_context_flush_deferred(ctx));
    // an attachment to a skeleton that has no pose yet: refused here, with every pending thing kept, as below
    RT_TRY(scene_require_poses(s, "rt_scene_update"));
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
    scene_poses_changed(s, posed);
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
    RT_TRY(rt_use_device(ctx));
    RT_TRY(rt_context_flush_deferred(ctx));
    RT_TRY(scene_require_poses(s, "rt_scene_build"));                 // (an attachment to a skeleton without a pose: refused with everything kept)
    RT_TRY(rt_scene_apply_masks(ctx, s, "rt_scene_build", true));     // (no visible instance: refused as a scene without instances is)
    ScopedEvent e0, e1;
    HIP_TRY(hipEventCreate(&e0.e));
    HIP_TRY(hipEventCreate(&e1.e));
    HIP_TRY(hipEventRecord(e0.e, ctx->stream));
    s->generation++;          // device arrays are about to be reallocated: pipelines drop what they cached
    for (SceneInstance &in : s->inst) RT_TRY(rt_build_blas(ctx, in.model));
    scene_build_begins(s);
    RT_TRY(rt_build_tlas(ctx, s));
    HIP_TRY(hipEventRecord(e1.e, ctx->stream));
    HIP_TRY(hipEventSynchronize(e1.e));
    HIP_TRY(hipEventElapsedTime(&s->build_ms, e0.e, e1.e));
    scene_applied(s, nullptr);
    return RT_OK;
}

int rt_scene_destroy(rt_scene *s) { return rt_release(s); }

int rt_scene_bvh_info(const rt_scene *s, int which, uint32_t *n_prims, uint32_t *n_nodes, uint32_t *max_depth)
{
    const BvhDev *b = lookup_bvh(s, which, __func__);
    if (!b) return RT_ERR_STATE;
    if (n_prims) *n_prims = b->n;
    if (n_nodes) *n_nodes = 2 * b->n - 1;
    if (max_depth) *max_depth = b->max_depth;
    return RT_OK;
}

int rt_scene_bvh_read(const rt_scene *s, int which, rt_bvh_node *nodes, uint64_t *sorted_keys, uint32_t *parents)
{
    const BvhDev *b = lookup_bvh(s, which, __func__);
    if (!b) return RT_ERR_STATE;
    RT_TRY(rt_use_device(s->ctx));
    const size_t nn = 2 * (size_t)b->n - 1;
    if (nodes) HIP_TRY(hipMemcpy(nodes, b->nodes.p, sizeof(rt_bvh_node) * nn, hipMemcpyDeviceToHost));
    if (sorted_keys) HIP_TRY(hipMemcpy(sorted_keys, b->keys.p, sizeof(uint64_t) * b->n, hipMemcpyDeviceToHost));
    if (parents) HIP_TRY(hipMemcpy(parents, b->parents.p, sizeof(uint32_t) * nn, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_scene_wide_info(const rt_scene *s, int which, uint32_t *n_nodes, int32_t *root_code, uint32_t *n_records)
{
    const BvhDev *b = lookup_bvh(s, which, __func__);
    if (!b) return RT_ERR_STATE;
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
    const BvhDev *b = lookup_bvh(s, which, __func__);
    if (!b) return RT_ERR_STATE;
    RT_TRY(rt_use_device(s->ctx));
    if (nodes && b->wide_n) HIP_TRY(hipMemcpy(nodes, b->wide.p, sizeof(WNode) * (size_t)b->wide_n, hipMemcpyDeviceToHost));
    if (records && which >= 0) HIP_TRY(hipMemcpy(records, s->inst[which].model->tris.p, sizeof(TriRec) * (size_t)s->inst[which].model->n_recs, hipMemcpyDeviceToHost));
    return RT_OK;
}

/* the validation boxes of an instance's model (rt_refs.h): *n_refs = 0 when none of its triangles is split */
int rt_scene_refs_info(const rt_scene *s, int which, uint32_t *n_tris, uint32_t *n_refs)
{
    if (!lookup_bvh(s, which, __func__, true)) return RT_ERR_STATE;
    const rt_model *m = s->inst[which].model;
    if (n_tris) *n_tris = m->n_tris;
    if (n_refs) *n_refs = m->ref_off.p ? (uint32_t)(m->ref_boxes.bytes / 24) : 0u;
    return RT_OK;
}

int rt_scene_refs_read(const rt_scene *s, int which, uint32_t *ref_off, float *ref_boxes, float *record_boxes)
{
    if (!lookup_bvh(s, which, __func__, true)) return RT_ERR_STATE;
    const rt_model *m = s->inst[which].model;
    if (!m->ref_off.p) { rt_set_error("rt_scene_refs_read: no triangle of this model is split"); return RT_ERR_STATE; }
    RT_TRY(rt_use_device(s->ctx));
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
    const BvhDev *b = pick_bvh(s, which);              // (its own refusal: it does not say what is pending)
    if (!b || !nodes || n_nodes != b->wide_n) { rt_set_error("rt_debug_wide_write: scene not built, or a different node count"); return RT_ERR_STATE; }
    RT_TRY(rt_use_device(s->ctx));
    HIP_TRY(hipMemcpy(b->wide.p, nodes, sizeof(WNode) * (size_t)n_nodes, hipMemcpyHostToDevice));
    return RT_OK;                                      // (same device pointers, same node count: nothing cached goes stale)
}

int rt_scene_instance_info(const rt_scene *s, uint32_t instance, float world_box[6], float world_to_object[12])
{
    RT_REQUIRE(s, "null scene");
    if (!s->built || instance >= s->inst.size()) return scene_refuse(s, __func__, "scene not built or instance out of range");
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

}  // extern "C"
