/*
 * dxr_amd.h -- C ABI of the MI355X-native progressive ray tracer.
 *
 * This is the drop-in boundary for ONE path of philcn/DXRExperiments: the
 * ProgressiveRaytracingPipeline (BLAS/TLAS build, traversal, ray-triangle
 * intersection, raygen / closest-hit / miss shading, float accumulation).
 * Each export names the reference interface it stands in for (file:line in
 * the reference tree).  D3D12 objects become opaque handles; the program /
 * state / bindings objects of the reference (RtProgram, RtState, RtBindings)
 * survive only in the C++ wrapper (dxrexperiments_amd/include), because HIP
 * kernels are linked at build time and there is no shader table to fill.
 *
 * Conventions
 *   - every function returns RT_OK (0) or a negative RT_ERR_* code and never
 *     throws; rt_last_error() returns the message of the calling thread's
 *     most recent failure.
 *   - a context is bound to one GPU and one HIP stream and is not thread
 *     safe; distinct contexts may be used from distinct threads.
 *   - host pointers passed in are copied before the call returns.
 *   - render / trace calls are asynchronous on the context's stream unless
 *     they return data to host memory; rt_context_synchronize() joins.
 *   - there is NO CPU fallback: without a usable HIP device every call that
 *     needs one fails with RT_ERR_HIP.
 */
#ifndef DXR_AMD_H
#define DXR_AMD_H

#include <stddef.h>
#include "dxr_amd_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_context  rt_context;
typedef struct rt_model    rt_model;
typedef struct rt_scene    rt_scene;
typedef struct rt_pipeline rt_pipeline;
typedef struct rt_skeleton rt_skeleton;
typedef struct rt_crowd rt_crowd;
typedef struct rt_progressive_host rt_progressive_host;

/* ---- library ------------------------------------------------------------- */

const char *rt_version(void);
const char *rt_last_error(void);
/* number of visible HIP devices, or a negative RT_ERR_* code */
int rt_device_count(void);

/* ---- RtContext (libs/DXRFramework/RtContext.h:15-46) ----------------------- */

/* RtContext::create (RtContext.h:15, RtContext.cpp:12-29): device + queue. */
int rt_context_create(int device, rt_context **out);
/* Same, but work is issued on the caller's hipStream_t (e.g. PyTorch's). */
int rt_context_create_on_stream(int device, void *hip_stream, rt_context **out);
int rt_context_destroy(rt_context *ctx);
/* DeviceResources::WaitForGpu (src/utils/DeviceResources.cpp:559) */
int rt_context_synchronize(rt_context *ctx);
int rt_context_get_stream(rt_context *ctx, void **hip_stream_out);
int rt_context_get_device(rt_context *ctx, int *device_out);
/* Bytes of the traversal kernels' global stack rows the context holds (the part of a walk's stack beyond the LDS rows).  Round 5: rows for
 * the threads of the PERSISTENT launches only, i.e. for what can be resident at once (57 MB on an MI355X for the bench scene, whatever the
 * size of a set; rounds 1 - 4: for every thread of the largest launch, and the one-tile-per-wave primary launch has one per pixel slot --
 * 224 MB per 1080p frame of a set, 4.3 GB for a set of 20); that launch now keeps none and hands the rays that would need one to a small
 * retry launch.  Shared by every pipeline of the context; the bench scenes never touch them.  No reference counterpart:
 * the Fallback Layer keeps its traversal stack inside DispatchRays (RtContext.cpp:218-221). */
int rt_context_get_stack_memory(rt_context *ctx, size_t *bytes);

/* Plain device buffers on the context's GPU (CreateBuffer / AllocateUploadBuffer of
 * Helpers/DirectXRaytracingHelper.h:187-208): for callers that feed device pointers to
 * rt_trace_batch(RT_MEM_DEVICE) or rt_denoiser_dispatch without another runtime. */
int rt_device_alloc(rt_context *ctx, size_t bytes, void **device_ptr);
int rt_device_free(rt_context *ctx, void *device_ptr);
int rt_device_upload(rt_context *ctx, void *device_dst, const void *host_src, size_t bytes);     /* synchronous */
int rt_device_download(rt_context *ctx, void *host_dst, const void *device_src, size_t bytes);   /* synchronous */

/* ---- RtModel (libs/DXRFramework/RtModel.h:13, RtModel.cpp:24-118) ---------- */

/* RtModel::create(ctx, filePath) (RtModel.h:13; the reference imports through Assimp, RtModel.cpp:26-27).  By extension:
 * ".fbx" -> the binary-FBX mesh reader (rt_fbx.cpp: Geometry nodes' Vertices / PolygonVertexIndex / LayerElementNormal,
 * zlib arrays; the node hierarchy is flattened as the reference's aiProcess_PreTransformVertices does: Lcl transforms, pivots,
 * offsets, pre / post rotations and RotationOrder down the Model parent chain, geometric transforms, instanced geometry), anything else ->
 * Wavefront OBJ.  See DESIGN.md for the vertex / primitive ordering these readers define. */
int rt_model_create_from_file(rt_context *ctx, const char *path, rt_model **out);
int rt_model_create_from_obj(rt_context *ctx, const char *path, rt_model **out);
/* The arrays RtModel's constructor builds (RtModel.cpp:33-81). */
int rt_model_create_from_arrays(rt_context *ctx, const rt_vertex *verts, uint32_t n_verts,
                                const uint32_t *indices, uint32_t n_tris, rt_model **out);
int rt_model_get_counts(const rt_model *m, uint32_t *n_verts, uint32_t *n_tris);
/* copy the ingested geometry back (host buffers sized by get_counts) */
int rt_model_read_geometry(const rt_model *m, rt_vertex *verts, uint32_t *indices);
int rt_model_retain(rt_model *m);
int rt_model_destroy(rt_model *m);

/* ---- RtScene (libs/DXRFramework/RtScene.h:14-37, RtScene.cpp:18-52) -------- */

int rt_scene_create(rt_context *ctx, rt_scene **out);                     /* RtScene::create  RtScene.h:14 */
/* RtScene::addModel(model, XMMATRIX) (RtScene.h:30): object-to-world as the
 * 3x4 row-major rows the instance desc stores (TopLevelASGenerator.cpp:355-357). */
int rt_scene_add_model(rt_scene *s, rt_model *m, const float transform3x4[12]);
int rt_scene_get_num_instances(const rt_scene *s, uint32_t *n);           /* RtScene.h:32 */
/* RtScene::build(ctx, hitGroupCount) (RtScene.cpp:18-52): BLAS per distinct
 * model (RtModel::build, RtModel.cpp:86-118), then the TLAS, all on the GPU. */
int rt_scene_build(rt_scene *s, uint32_t hit_group_count);
int rt_scene_destroy(rt_scene *s);

/* Inspection of the canonical acceleration structures (tests, tools).
 * which = -1: TLAS; which >= 0: BLAS of the model used by instance `which`. */
int rt_scene_bvh_info(const rt_scene *s, int which, uint32_t *n_prims, uint32_t *n_nodes, uint32_t *max_depth);
int rt_scene_bvh_read(const rt_scene *s, int which, rt_bvh_node *nodes, uint64_t *sorted_keys, uint32_t *parents);
/* world_box: the TLAS leaf box of the instance = the exact box of its triangles' transformed vertices (an identity instance: of its BLAS) */
int rt_scene_instance_info(const rt_scene *s, uint32_t instance, float world_box[6], float world_to_object[12]);
/* Inspection of the PRODUCTION traversal layout of the same structures (tests, tools).  rt_wide_layout_info reports
 * its width and node size: (4, 64) -- 64-B nodes of 16 words:
 *   w0..w2 float origin.xyz of the node's box, w3 float scale.x | w4 lo.x bytes of children 0..3 (child k in bits 8k..),
 *   w5 hi.x, w6 lo.y, w7 hi.y | w8 lo.z, w9 hi.z, w10 float scale.y, w11 float scale.z | w12..w15 int32 child codes;
 *   children packed at the front, larger surface first; plane = fma(byte, scale, origin); a scale of +inf (bytes 0) marks
 *   an axis that is not quantised (non-finite extents): its planes bound nothing.
 * Child codes: >= 0 node index, INT32_MIN unused, otherwise ~code with code = instance (TLAS) or
 * first_record << 3 | (count - 1) (BLAS).  BLAS records are 48 B: nine floats p0 p1 p2, the uint32 primitive index, 8 B
 * padding.  root_code: 0 = node 0, negative = the whole structure is one leaf. */
int rt_wide_layout_info(uint32_t *width, uint32_t *node_bytes);
int rt_scene_wide_info(const rt_scene *s, int which, uint32_t *n_nodes, int32_t *root_code, uint32_t *n_records);
int rt_scene_wide_read(const rt_scene *s, int which, void *nodes, void *records);
/* test / experiment hook: overwrite the node array with a RENUMBERING of itself (same count; node 0 stays the root and the
 * first nodes the breadth-first top the traversal keeps in LDS).  Results do not depend on node numbers. */
int rt_debug_wide_write(rt_scene *s, int which, const void *nodes, uint32_t n_nodes);
/* Split references (round 5; dxrexperiments_amd/csrc/rt_refs.h, defined in oracle/oracle_bvh.h): a long thin triangle whose AABB is more than
 * eight times its own surface is held by the traversal layout as up to 128 references, each with the box of the part of the triangle inside
 * one slab of its longest axis, and a candidate hit on it is accepted only if one of those boxes passes the slab test over [tmin, t] (an
 * unsplit triangle: its own AABB, the rule of rounds 1 - 4).  rt_scene_refs_info: triangles of instance `which`'s model and its boxes in all
 * (0: no triangle is split); rt_scene_refs_read: ref_off[n_tris + 1], the boxes by primitive (6 floats each) and the box of every record of
 * the traversal layout (rt_scene_wide_read's records; meaningful where a record's third word of c says 1).  No reference counterpart: the
 * Fallback Layer's builder is not in the checkout (libs/DXRFramework/Helpers/BottomLevelASGenerator.cpp:333 only calls it). */
int rt_scene_refs_info(const rt_scene *s, int which, uint32_t *n_tris, uint32_t *n_refs);
int rt_scene_refs_read(const rt_scene *s, int which, uint32_t *ref_off, float *ref_boxes, float *record_boxes);
/* milliseconds the last rt_scene_build spent on the GPU (BLAS + TLAS) */
int rt_scene_build_ms(const rt_scene *s, float *ms);

/* Rigid animation -- EXTENSIONS: the reference's RtScene exposes none of this (its only statement of a transform is addModel, RtScene.h:30).
 * rt_scene_set_instance_transform(s): overwrite the object-to-world rows of instances that rt_scene_add_model has added -- the Transform
 * member of the instance descriptor (libs/DXRFramework/Helpers/TopLevelASGenerator.cpp:344-362).  Any twelve floats are taken, as by
 * rt_scene_add_model; frames a deferred pipeline still holds are rendered first (they see the scene as it was); an index out of range is
 * RT_ERR_STATE.  On a scene that was never built the call only overwrites the stored transform.  On a built scene it leaves the scene STALE:
 * until rt_scene_update or rt_scene_build, rt_trace_batch, the render calls and the rt_scene_*_info / _read calls fail as on an unbuilt
 * scene (the message names the pending transforms) -- nothing ever traces a half-applied state.
 * `transforms3x4` of the plural form: count x 12 floats, for instances first .. first + count - 1. */
int rt_scene_set_instance_transform(rt_scene *s, uint32_t instance, const float transform3x4[12]);
int rt_scene_set_instance_transforms(rt_scene *s, uint32_t first, uint32_t count, const float *transforms3x4);
/* EXTENSION: applies the pending transforms on the device -- instance records (fp32 inverse, flags), the world boxes of the pending
 * instances, the TLAS -- and leaves the scene built.  Stands in for the generators' update path (`updateOnly` of
 * TopLevelASGenerator::Generate, libs/DXRFramework/Helpers/TopLevelASGenerator.h:144-163, and `allowUpdate` / `updateOnly` of
 * Helpers/BottomLevelASGenerator.h:136-176), which the reference's RtScene never calls.  The scene afterwards is, array for array, the
 * scene rt_scene_build gives for the same instance list (DESIGN.md "update == build").  It builds no BLAS but those of models whose vertices
 * were set (rt_model_set_vertices, below): on a scene that has not been built since its last rt_scene_add_model it fails (RT_ERR_STATE).  With nothing pending it returns RT_OK and changes nothing; otherwise
 * pipelines drop what they cached from the old geometry (shadow cache, free sphere, primary-mode samples) -- their accumulation buffers are
 * the caller's to clear (rt_pipeline_clear_output), as after a camera change. */
int rt_scene_update(rt_scene *s);
/* EXTENSION: milliseconds the last rt_scene_update spent on the GPU (the BLAS rebuilds of deformed models included), as rt_scene_build_ms */
int rt_scene_update_ms(const rt_scene *s, float *ms);

/* Instance masks -- EXTENSIONS: the InstanceMask member of the instance descriptor (libs/DXRFramework/Helpers/TopLevelASGenerator.cpp:344-362),
 * which the reference fills with the constant 0xFF (line 361) and tests against the InstanceInclusionMask 0xFF of its every TraceRay
 * (ProgressiveRaytracing.hlsl:34,53, RaytracingCommon.hlsli:94, RealtimeRaytracing.hlsl:42,61).  Every instance has an 8-bit mask, 0xFF when
 * rt_scene_add_model adds it; every ray of this library (the two pipelines and rt_trace_batch) carries the inclusion mask 0xFF, so an instance
 * is VISIBLE -- considered by rays -- iff its mask is non-zero.  The byte is stored and returned as given.  With a pool of instances added up
 * front, "add" is "show" and "remove" is "hide": indices, and with them "material i <-> instance i", stay as they are.
 * Arguments as for rt_scene_set_instance_transforms: a null argument is RT_ERR_INVALID_ARG, a range beyond the scene's instances RT_ERR_STATE,
 * count == 0 returns RT_OK and changes nothing; a setter with count > 0 first renders the frames a deferred pipeline still holds (they see
 * the scene as it was).  On a scene that is not updatable (never built, or instances added since the last build) a setter only stores the
 * masks: the next rt_scene_build reads them.  On an updatable scene a call that changes the VISIBILITY of at least one instance (zero <->
 * non-zero) leaves the scene STALE, as a pending transform does: rt_trace_batch, the render calls and the rt_scene_*_info / _read calls fail
 * with RT_ERR_STATE (the message names the pending masks) until rt_scene_update or rt_scene_build.  A call that changes no instance's
 * visibility (the value a mask has; one non-zero value for another) changes the stored bytes and nothing else: the scene stays built.
 * rt_scene_update applies pending masks together with pending transforms and changed models, in one call, with one bump of the generation;
 * rt_scene_build honours the stored masks the same way.  Either fails with RT_ERR_STATE when it would leave NO visible instance (the message
 * says that no instance is visible), as rt_scene_build refuses a scene without instances; the scene stays stale and everything pending is
 * kept, so that showing one instance and updating again succeeds.
 * What the scene then is (DESIGN.md "update == build, with masks"): the instance records and world boxes are those of the FULL list, hidden
 * instances included (rt_scene_instance_info answers for them; they follow their transforms and their models' vertices); the TLAS -- canonical
 * nodes, sorted keys, parents, depth, four-wide layout -- is the TLAS of a fresh build over the visible sub-list in ascending index order,
 * except that wherever that build names the j-th instance of the sub-list this one names the instance's own index (canonical leaves' `left`,
 * the low 32 bits of the sorted keys, the wide nodes' leaf codes ~instance, root_code when one instance is visible);
 * rt_scene_bvh_info(-1) reports n_prims = the number of visible instances.  With every mask non-zero both calls launch what they always did. */
int rt_scene_set_instance_mask(rt_scene *s, uint32_t instance, uint8_t mask);
int rt_scene_set_instance_masks(rt_scene *s, uint32_t first, uint32_t count, const uint8_t *masks);
/* EXTENSION (TopLevelASGenerator.cpp:344-362 as above): the stored masks of instances first .. first + count - 1, pending or applied */
int rt_scene_get_instance_masks(const rt_scene *s, uint32_t first, uint32_t count, uint8_t *masks);

/* Deforming meshes -- EXTENSIONS: the reference's RtModel is immutable once created (RtModel.h:13); its generators have the path
 * (`allowUpdate` / `updateOnly` of libs/DXRFramework/Helpers/BottomLevelASGenerator.h:136-176), which RtModel::build never takes.
 * rt_model_set_vertices / rt_model_set_positions overwrite vertices first .. first + count - 1 of the model's device array, on the context's
 * stream: whole 24-byte records, or count x 3 floats of positions with the normals kept.  The vertex count and the index list never change.
 * `mem` is RT_MEM_HOST or RT_MEM_DEVICE, as for rt_trace_batch; a device source (the output of a skinning, cloth or morph kernel) is copied
 * device to device and nothing goes through the host.  A producer that wrote the source on ANOTHER stream is the caller's to order before the
 * call; a context made with rt_context_create_on_stream on the producer's stream needs nothing.  Frames a deferred pipeline still holds are
 * rendered first (they see the mesh as it was).  count == 0 returns RT_OK and changes nothing; a range beyond the model's vertices is
 * RT_ERR_STATE; a null argument or an unknown `mem` is RT_ERR_INVALID_ARG.  rt_model_read_geometry returns the current vertices (after a
 * device-side set: downloaded on demand).
 * A successful set leaves the model CHANGED, and every built scene that holds it in any instance STALE, exactly as after
 * rt_scene_set_instance_transform: rt_trace_batch, the render calls and the rt_scene_*_info / _read calls fail with RT_ERR_STATE (the message
 * names the pending vertices) until rt_scene_update or rt_scene_build.  rt_scene_update then REBUILDS the BLAS of every changed model by the
 * build's own steps, into the model's own buffers (once, however many scenes hold it), rewrites the model fields of its instances' records
 * on the device, gives those instances their world boxes over the new vertices and rebuilds the TLAS; pending transforms are applied by the
 * same call.  A BLAS is rebuilt, never refitted: after `set + update` the scene is, array for array -- every BLAS's canonical nodes, keys and
 * parents, its production nodes and records, reference offsets and boxes, every instance record, the TLAS -- the scene rt_scene_build gives
 * for the same instance list over fresh models created from the final vertex arrays (DESIGN.md "update == build").  A scene that was never
 * built just reads the new vertices at its next build. */
int rt_model_set_vertices(rt_model *m, uint32_t first, uint32_t count, const rt_vertex *verts, uint32_t mem);
int rt_model_set_positions(rt_model *m, uint32_t first, uint32_t count, const float *xyz, uint32_t mem);   /* count x 3 floats, normals kept */
/* EXTENSION (BottomLevelASGenerator.h:136-176 as above; for producers that write positions only): the normal of every vertex v from the
 * current positions, on the device.  With s = (0, 0, 0): for every triangle that names v at any corner, in ascending order (one that names
 * v more than once counts once), f = cross(p1 - p0, p2 - p0) with the corners in index order and s = s + f componentwise; with
 * d = dot(s, s) = ((x x) + y y) + z z the normal is s * (1 / sqrt(d)) if 0 < d < inf, else (0, 0, 0).  fp32 throughout, no contraction, no
 * atomics: the order is part of the result.  The vertex -> triangle table is built from the index list at the first call.  Marks the model
 * changed as a setter does. */
int rt_model_recompute_normals(rt_model *m);

/* Skeletal animation -- EXTENSIONS: the reference imports with aiProcess_PreTransformVertices and reads only mVertices / mNormals
 * (libs/DXRFramework/RtModel.cpp:26, :38-45), so it has no bones at all; the update path a pose would take is the generators' never-taken
 * one (Helpers/BottomLevelASGenerator.h:136-176).  A model gets a SKIN, the caller sets a bone PALETTE per frame, a kernel writes the model's
 * vertices from the two, and rt_scene_update does the rest as after any rt_model_set_vertices.
 * A skin of a model with V vertices: `influences` = K slots per vertex, 1 <= K <= 8; n_bones, 1 <= n_bones <= 65536; bone_indices[v][k] <
 * n_bones and weights[v][k], both V x K, vertex major (entry [v][k] at v * K + k), host arrays; and the REST POSE, a copy of the model's
 * 24-byte vertex records as they are on the device when the skin is set.  The weights are fp32, taken as given, never renormalised.
 * A palette: n_bones x 12 floats, 3x4 row-major matrices M_b in the layout of the instance transforms -- the caller's finished skinning
 * matrices (current pose x inverse bind); the library knows no hierarchy.
 * The definition, for vertex v with rest position (x, y, z) and rest normal (nx, ny, nz), fp32 throughout, no contraction, in this order:
 *   blend   for each of the 12 entries e: B[e] = weights[v][0] * M_bone[v][0][e]; then for k = 1 .. K - 1 in slot order
 *           B[e] = B[e] + weights[v][k] * M_bone[v][k][e].  Every slot is evaluated: a zero weight is not skipped.
 *   position, per row r: p'_r = ((B[r][0] x + B[r][1] y) + B[r][2] z) + B[r][3]
 *   normal  s_r = (B[r][0] nx + B[r][1] ny) + B[r][2] nz; d = dot(s, s) = ((sx sx) + sy sy) + sz sz; the normal is s * (1 / sqrt(d)) if
 *           0 < d < inf, else (0, 0, 0): the rule of rt_model_recompute_normals.  It goes through the blended LINEAR part, not its inverse
 *           transpose: exact for rotations and uniform scales.  With non-uniform scales call rt_model_recompute_normals afterwards.
 * NaN, inf, negative weights and weights that do not sum to 1 are no errors: the result is what the arithmetic gives.
 * rt_model_set_skin validates on the host: a null argument, influences outside 1 .. 8 or n_bones outside 1 .. 65536 is RT_ERR_INVALID_ARG;
 * so is an index >= n_bones (the message names the vertex and the slot).  It stores the skin on the device and captures the rest pose, device
 * to device on the context's stream.  It does NOT change the model's vertices: nothing is marked changed, built scenes stay built.  Calling it
 * again replaces the skin and captures the rest pose anew from the vertices the model holds then.  influences == 0 (the other arguments are
 * ignored) removes the skin and frees its buffers; the vertices stay what the last pose made them. */
int rt_model_set_skin(rt_model *m, uint32_t influences, uint32_t n_bones,
                      const uint32_t *bone_indices /* V x influences, vertex major */,
                      const float *weights        /* V x influences */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the influences and bones of the model's skin; 0, 0: no skin */
int rt_model_get_skin(const rt_model *m, uint32_t *influences, uint32_t *n_bones);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): every vertex of the model from the rest pose and this palette,
 * by the definition above, on the device -- always the whole mesh and always from the rest pose, never from the previous pose.  `mem`:
 * RT_MEM_HOST (the palette goes up through a scratch buffer and the stream is synchronised before the call returns, as for
 * rt_model_set_positions) or RT_MEM_DEVICE (used in place, ordered on the context's stream; a producer on another stream is the caller's to
 * order, and the palette must stay as it is until the stream has passed the call).  A null argument or an unknown `mem` is
 * RT_ERR_INVALID_ARG; a model without a skin is RT_ERR_STATE (the message names rt_model_set_skin).  Otherwise it behaves as the setters
 * above: frames a deferred pipeline still holds are rendered first, the model is left CHANGED and every built scene that holds it STALE
 * (RT_ERR_STATE from what reads them, the message names the pending vertices) until rt_scene_update or rt_scene_build, which rebuild the BLAS.
 * rt_model_set_vertices / rt_model_set_positions on a skinned model still write the current vertices and leave the rest pose alone: the next
 * rt_model_set_bones overwrites what they wrote.  rt_model_read_geometry returns the skinned vertices. */
int rt_model_set_bones(rt_model *m, const float *bones3x4 /* n_bones x 12 */, uint32_t mem /* RT_MEM_HOST | RT_MEM_DEVICE */);

/* Morph targets -- EXTENSIONS: the reference reads only mVertices / mNormals of an imported mesh (libs/DXRFramework/RtModel.cpp:26, :38-45)
 * and never its aiAnimMesh blend shapes; the update path a morphed mesh would take is the generators' never-taken one
 * (Helpers/BottomLevelASGenerator.h:136-176).  A model gets TARGETS, sparse per-vertex deltas over a BASE; the caller sets one WEIGHT per target
 * per frame, and a kernel writes every vertex as base + the weighted deltas.
 * Targets are sparse and target major, host arrays: target t owns entries target_offsets[t] .. target_offsets[t + 1] - 1; entry e adds
 * position_deltas[3 e ..] to vertex vertex_indices[e] and, with normal_deltas given, normal_deltas[3 e ..] to that vertex's normal.  A dense
 * target simply lists every vertex; a target with no entries is legal.
 * The definition, for vertex v with BASE position b and BASE normal n, fp32 throughout, every product and every sum one rounded operation,
 * no contraction, in this order:
 *   a vertex that no target names gets its base record copied bit for bit, all 24 bytes;
 *   otherwise p = b and s = n, and for every entry that names v, in ascending target order, with w_t the weight of its target and dp, dn its
 *   deltas, for each component c: p_c = p_c + (w_t * dp_c) and, with normal deltas, s_c = s_c + (w_t * dn_c).  Every entry is evaluated: a
 *   zero weight is not skipped, so -0 + (+0 * d) is +0 (for a delta d >= +0), and a NaN weight reaches the vertex.
 *   normal  with normal deltas d = dot(s, s) = ((sx sx) + sy sy) + sz sz and the normal is s * (1 / sqrt(d)) if 0 < d < inf, else (0, 0, 0):
 *           the rule of rt_model_recompute_normals.  Without normal deltas the base normal is copied bit for bit.
 * The weights are taken as given: NaN, inf, negative weights and weights above 1 are no errors.
 * rt_model_set_morph_targets validates on the host, and nothing changes when it refuses: RT_ERR_INVALID_ARG for a null `m`; with
 * n_targets > 0 for a null target_offsets, vertex_indices or position_deltas; for n_targets > 65536 (a target index is stored in 16 bits);
 * for target_offsets[0] != 0 or offsets that decrease (the message names the target); for a vertex index >= V and for indices within one
 * target that do not ascend strictly -- a target names a vertex at most once -- (the message names the target and the entry, the entry by its
 * place in vertex_indices); RT_ERR_UNSUPPORTED for targets whose packed layout (64 cells per slice of 64 vertices and step of its longest
 * run) would take 2^32 cells or more.  It stores the packed targets on the device and captures the BASE, device to device on the context's
 * stream: on a model without a skin the model's vertices as they are then, on a model with a skin the skin's rest pose.  It changes no
 * vertex and marks nothing changed: built scenes stay built.  Calling it again replaces the targets and captures the base anew.
 * n_targets == 0 (the other arguments are ignored) removes the targets and frees their buffers; the vertices stay what the last call made
 * them. */
int rt_model_set_morph_targets(rt_model *m, uint32_t n_targets,
                               const uint32_t *target_offsets   /* n_targets + 1 */,
                               const uint32_t *vertex_indices   /* target_offsets[n_targets] */,
                               const float *position_deltas     /* 3 floats per entry */,
                               const float *normal_deltas       /* 3 floats per entry, or NULL: positions only */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the targets and entries of the model's morph targets and whether
 * they carry normal deltas; each may be NULL; 0, 0, 0: none */
int rt_model_get_morph_targets(const rt_model *m, uint32_t *n_targets, uint32_t *n_entries, uint32_t *has_normals);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): every vertex from the base and these n_targets weights, by the
 * definition above, on the device -- always the whole mesh and always from the base, never from the previous result.  Where the result goes
 * depends on whether the model has a skin when the call is made.
 * NO SKIN: into the model's vertices, and the call behaves as rt_model_set_bones does: frames a deferred pipeline still holds are rendered
 * first, the model is left CHANGED and every built scene that holds it STALE (RT_ERR_STATE from what reads them, the message names the
 * pending vertices) until rt_scene_update or rt_scene_build, which rebuild the BLAS.  rt_model_read_geometry returns the morphed vertices.
 * WITH A SKIN: into the skin's rest pose.  The model's vertices are not touched, nothing is marked changed, built scenes stay built and
 * traceable, and the next rt_model_set_bones poses the morphed rest pose: a frame of a morphed, skinned character is
 * rt_model_set_morph_weights, rt_model_set_bones, rt_scene_update.
 * rt_model_set_skin itself is as it was and captures its rest pose from the model's vertices; giving a morphed model a skin later redirects
 * later morph results to the new rest pose, removing the skin redirects them to the vertices again, and the morph base is recaptured by
 * neither.  `mem` as for rt_model_set_bones: RT_MEM_HOST (the weights go up through a scratch buffer and the stream is synchronised before
 * the call returns) or RT_MEM_DEVICE (used in place, ordered on the context's stream).  A null argument or an unknown `mem` is
 * RT_ERR_INVALID_ARG; a model without targets is RT_ERR_STATE (the message names rt_model_set_morph_targets).  rt_model_set_vertices /
 * rt_model_set_positions on a morphed model still write the current vertices and leave the base alone. */
int rt_model_set_morph_weights(rt_model *m, const float *weights /* n_targets */, uint32_t mem /* RT_MEM_HOST | RT_MEM_DEVICE */);

/* Posed skeletons -- EXTENSIONS: the reference imports with aiProcess_PreTransformVertices (libs/DXRFramework/RtModel.cpp:26), which drops
 * bones, node animation and all; the update path a pose would take is the generators' never-taken one
 * (Helpers/BottomLevelASGenerator.h:136-176).  rt_model_set_bones above takes finished matrices and knows no hierarchy; the hierarchy lives
 * HERE.  A SKELETON is n_joints joints, each with a parent that comes before it (or -1: a root) and an inverse bind matrix; a POSE is ten
 * floats per joint, translation, rotation quaternion, scale; from a pose the device computes every joint's world matrix W_j and the PALETTE
 * M_j that rt_model_set_bones takes, and keeps both; a CLIP is a baked pose per key time, sampled on the device from one float of time.  A
 * frame of an animated character is rt_skeleton_set_time, rt_model_set_bones_from_skeleton, rt_scene_update, and no per-frame array crosses
 * to the device; several models whose skins have n_joints bones may share one skeleton and one palette.
 * The definition, fp32 throughout, every product and every sum one rounded operation, no contraction.  Values are taken as given: a
 * quaternion is not normalised by rt_skeleton_set_pose, and NaN, inf, zero and negative scales are no errors.
 *   local   L of a joint from t, q = (x, y, z, w), s:
 *           xx = x*x, yy = y*y, zz = z*z, xy = x*y, xz = x*z, yz = y*z, wx = w*x, wy = w*y, wz = w*z
 *           R00 = 1 - 2*(yy + zz)   R01 = 2*(xy - wz)       R02 = 2*(xz + wy)
 *           R10 = 2*(xy + wz)       R11 = 1 - 2*(xx + zz)   R12 = 2*(yz - wx)
 *           R20 = 2*(xz - wy)       R21 = 2*(yz + wx)       R22 = 1 - 2*(xx + yy)
 *           L[r][c] = R[r][c] * s_c (T.R.S) and L[r][3] = t_r.  Column vectors, as the instance transforms: q = (0, 0, sqrt(1/2), sqrt(1/2))
 *           turns +x into +y.
 *   product C = A o B of two 3x4 affine matrices:
 *           C[r][c] = (A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c] for c < 3
 *           C[r][3] = ((A[r][0] B[0][3] + A[r][1] B[1][3]) + A[r][2] B[2][3]) + A[r][3]
 *   world   W_j = L_j for a root, bit for bit; otherwise W_j = W_parent(j) o L_j.  The recursion fixes the association: level by level, or
 *           down a joint's chain from its root, the bits are the same.
 *   palette M_j = W_j o inverse_bind_j, always multiplied, for an identity too.
 *   sampling clip c of K keys at t.  The host finds the segment and passes two scalars (i, a): K == 1 or t <= times[0] gives i = 0, a = 0;
 *           t >= times[K-1] gives i = K-2, a = 1; otherwise i is the largest key with times[i] <= t and
 *           a = (t - times[i]) / (times[i+1] - times[i]) in fp32.  Looping is the caller's.  Per joint, with A = key i and B = key i+1 (B = A
 *           when K == 1): every translation and scale component is A_c + (a * (B_c - A_c)).  The quaternion: d = ((Ax Bx + Ay By) + Az Bz) +
 *           Aw Bw; if d < 0 every component of B is negated (the shortest path; a NaN d negates nothing); q_c = A_c + (a * (B_c - A_c));
 *           n = ((qx qx + qy qy) + qz qz) + qw qw; q = q * (1 / sqrt(n)) if 0 < n < inf, else (0, 0, 0, 1): the rule of
 *           rt_model_recompute_normals.  No slerp.  The result is the local pose, and it is posed as by rt_skeleton_set_pose.
 *   blending (rt_skeleton_set_blend): an ordered list of 1 .. RT_SKELETON_MAX_LAYERS (8) LAYERS (rt_skeleton_layer, dxr_amd_types.h), each a
 *           clip, a time, a weight, a MASK (one float per joint, taken as given; RT_SKELETON_NO_MASK: none) and a mode.  fp32 throughout,
 *           every product and every sum one rounded operation, no contraction, values taken as given: a weight is not clamped, NaN and inf
 *           are no errors.  S_k is the pose that layer k's clip gives at its time by the sampling rule above, whole: the segment search on
 *           the host, the lerp, the shortest-path flip, the normalisation with its (0, 0, 0, 1) fallback.  The accumulated pose P, per joint j:
 *           layer 0 is the base: P = S_0 bit for bit; with clip == RT_SKELETON_CURRENT_POSE, P is the pose the skeleton holds as it stands
 *           (what rt_skeleton_read_pose returns; it is read and overwritten by the same lane, in place).  The base layer's weight and mask
 *           are not read, and its mode must be RT_LAYER_BLEND.
 *           layers k >= 1: w = weight_k without a mask, else w = weight_k * mask_k[j], one product.
 *           RT_LAYER_BLEND: every translation and scale component P_c = P_c + (w * (S_c - P_c)).  The quaternion:
 *           d = ((Px Sx + Py Sy) + Pz Sz) + Pw Sw; if d < 0 every component of S is negated (a NaN d negates nothing);
 *           q_c = P_c + (w * (S_c - P_c)); then normalised by the rule above: n = ((qx qx + qy qy) + qz qz) + qw qw,
 *           q * (1 / sqrt(n)) if 0 < n < inf, else (0, 0, 0, 1).
 *           RT_LAYER_ADDITIVE: the reference pose R of an additive clip is what rt_skeleton_set_time(clip, -inf) gives: the sampling rule
 *           with (i, a) = (0, 0), normalisation included.  Translation and scale: P_c = P_c + (w * (S_c - R_c)).  The rotation, in the
 *           joint's local frame: D = conj(R_q) (x) S_q; if D_w < 0 every component of D is negated (a NaN negates nothing);
 *           E_xyz = w * D_xyz and E_w = 1 + (w * (D_w - 1)); E normalised by the rule; P_q = P_q (x) E; P_q normalised by the rule.
 *           conj(q) = (-x, -y, -z, w), and the Hamilton product p (x) q is grouped
 *             x = ((pw qx + px qw) + py qz) - pz qy      y = ((pw qy - px qz) + py qw) + pz qx
 *             z = ((pw qz + px qy) - py qx) + pz qw      w = ((pw qw - px qx) - py qy) - pz qz
 *           The result is written as the skeleton's local pose, ten floats per joint, and posed exactly as rt_skeleton_set_pose poses: the
 *           pose is counted once, and rt_skeleton_read_pose, the palette, the joints and attached instances all follow.  A blend is
 *           stateless, as rt_skeleton_set_time is: a call leaves nothing behind but the pose.  No slerp, no per-channel key times, no
 *           state machine: the caller moves the weights.
 *   inverse kinematics (rt_skeleton_solve_ik): 1 .. RT_SKELETON_MAX_IK (32) CONSTRAINTS (rt_skeleton_ik, dxr_amd_types.h) solved in closed
 *           form against the pose the skeleton holds; each rewrites rotation quaternions of that local pose.  fp32 throughout, every
 *           product and every sum one rounded operation, no contraction, values taken as given: a weight is not clamped, NaN and inf are
 *           no errors.  Only + - * / sqrt, comparisons and selects: no acos, no sin.  A clamp is a comparison and a select, never fmin or
 *           fmax, so a NaN takes the same path everywhere, and every NaN written leaves as the quiet NaN 0x7FC00000.  The Hamilton product,
 *           conj and the normalisation rule with its (0, 0, 0, 1) fallback are those of "blending" above.  On 3-vectors:
 *             u.v = (ux vx + uy vy) + uz vz      u x v = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx)
 *             unit(v) = v * (1 / sqrt(v.v)) if 0 < v.v < inf, else the zero vector and NO ANSWER
 *             rot(q, v) = (v + (w * t)) + (q_xyz x t) with t = 2 * (q_xyz x v)
 *             perp(u) = unit(u x e), e the coordinate axis on which |u| is smallest, the lowest index on a tie
 *             between(u, v), for unit u and v: s = u + v; if s.s < 1e-6, or unit(s) has no answer, the half turn (perp(u), 0) as it stands;
 *               otherwise, with h = unit(s), the quaternion (u x h, u.h) normalised by the rule.  (The half vector stays well conditioned
 *               up to the half turn; (u x v, 1 + u.v) does not.)
 *             turn(a, b) = between(unit(a), unit(b)), and the identity (0, 0, 0, 1) where either has no answer
 *             M(p) of a 3x4 matrix and a point: M(p)_r = ((M[r][0] px + M[r][1] py) + M[r][2] pz) + M[r][3], the product's last column
 *           PARENT SPACE.  A two-bone constraint names its TIP c; b = parent(c) is the middle joint, a = parent(b) the chain's root.  An aim
 *           names the joint j it turns.  Where a (or j) is a root of the skeleton, target and pole are used as given, bit for bit.
 *           Otherwise, with p its parent and I = inverse(W_p) -- the adjugate / determinant inverse of the instance transforms, every NaN
 *           of I the quiet NaN; W_p as the skeleton's joints hold it, the pose before this call -- T = I(target) and P = I(pole).  An aim's
 *           axis is not transformed: it lives in the joint's own frame.
 *           TWO-BONE.  1: A and B are the stored quaternions of a and b, normalised by the rule.  2: pa = t_a, pb = L_a(t_b),
 *           pc = L_a(L_b(t_c)), L_a and L_b by "local" from (t_a, A, s_a) and (t_b, B, s_b).  3: l1 = sqrt((pb - pa).(pb - pa)),
 *           l2 = sqrt((pc - pb).(pc - pb)), g = T - pa, n = unit(g), d = sqrt(g.g).  4: lo = |l1 - l2|, hi = l1 + l2; if d < lo then
 *           d = lo; then if d > hi then d = hi.  5: if n has no answer, or not d > 0, or not l1 > 0, or not l2 > 0, the solved rotations
 *           are A and B themselves.  6: otherwise x = ((l1 l1 - l2 l2) + d d) / (2 d); hh = l1 l1 - x x; h = sqrt(hh if hh > 0 else 0);
 *           m = unit(k - n * (k.n)) with k = P - pa; if that has no answer the same with k = pb - pa; if that has none either, perp(n);
 *           pb' = (pa + n * x) + m * h and pc' = pa + n * d; Da = turn(pb - pa, pb' - pa); A' = normalised(Da (x) A);
 *           b1 = pa + rot(Da, pb - pa) and c1 = pa + rot(Da, pc - pa); Db = turn(c1 - b1, pc' - b1);
 *           B' = normalised((conj(A') (x) (Db (x) A')) (x) B).
 *           AIM.  Q is the stored quaternion of j, normalised; v = unit(rot(Q, axis)) and w = unit(T - t_j); if either has no answer
 *           Q' = Q, otherwise Q' = normalised(between(v, w) (x) Q).
 *           WEIGHT.  Each written quaternion goes from the normalised input A towards the solved A' by the RT_LAYER_BLEND rule:
 *           d = ((Ax A'x + Ay A'y) + Az A'z) + Aw A'w; if d < 0 every component of A' is negated; q_c = A_c + (weight * (A'_c - A_c)),
 *           normalised by the rule.  A weight of 0 therefore writes normalised(A): the stored quaternion, normalised (and once more, by the rule).
 *           A two-bone constraint writes the quaternions of a and b, an aim that of j.  Every translation, every scale, and the rotation
 *           of every joint that no constraint turns keep their bits.  All constraints of one call are solved side by side from the same
 *           input pose, so they must be INDEPENDENT: every constraint reads its tip (its aimed joint) and all of that joint's ancestors,
 *           and no joint written by one constraint may be read by another.  Four limbs of one body pass; an aim on a hand whose arm is
 *           solved in the same call does not: that is two calls, the second seeing the first's pose.  The result is posed exactly as
 *           rt_skeleton_set_pose poses, and the pose is counted once.
 *           GROUPS (rt_skeleton_solve_ik_groups, rt_crowd_set_ik_chain_groups).  Constraints that depend on one another -- the hand aimed
 *           at what its arm has just reached for, a foot aimed after its leg is planted -- go into ONE call as an ordered list of
 *           1 .. RT_SKELETON_MAX_IK_GROUPS (8) groups, given as group_sizes[n_groups] over one array of n = the sum of the sizes
 *           constraints, n at most RT_SKELETON_MAX_IK (32).  The constraints WITHIN a group are independent by the rule above; ACROSS
 *           groups anything goes: a later group may read or write what an earlier group wrote.  The call leaves pose, joints and palette
 *           exactly as n_groups successive rt_skeleton_solve_ik calls would, one per group in order, bit for bit: group g reads the W of
 *           the pose that group g - 1 left, the whole list is checked before anything is solved, and a list of one group is
 *           rt_skeleton_solve_ik itself.  Eight groups is a choice: the ends of the groups travel to the kernel by value as eight bytes
 *           beside the table of constraints.  The pose is counted once.
 *           Geometry: the tip reaches the clamped target exactly, up to rounding, when a and b carry uniform scale; ancestors may be any
 *           invertible affine matrices.  Under non-uniform scale on a or b the answer is still this definition, but the tip's position is
 *           approximate.  Twist about the bones is whatever the input pose had.  No joint limits, no chains longer than two bones, no CCD
 *           or FABRIK.
 *   crowds  (rt_crowd_*): a CROWD is n_actors poses of ONE skeleton.  It retains the skeleton and reads its hierarchy, inverse binds, clips
 *           and masks where they live -- a clip or mask added after the crowd was made is there for the next call -- and owns three device
 *           arrays, actor major: pose[n_actors][n_joints][10], joints[n_actors][n_joints][12], palette[n_actors][n_joints][12].  Actor a of
 *           a crowd is, bit for bit, a skeleton given the same call: rt_crowd_set_poses is rt_skeleton_set_pose with actor a's n_joints x 10
 *           floats, rt_crowd_set_times rt_skeleton_set_time(clips[a], times[a]), rt_crowd_set_blend rt_skeleton_set_blend with actor a's
 *           n_layers layers, by the definitions above and by the same statements (the segment (i, a) of every sampled layer found on the
 *           host); RT_SKELETON_CURRENT_POSE on layer 0 is that actor's own held pose.  Every posing call poses ALL actors with one kernel
 *           launch and counts one pose for the whole crowd.  No per-actor IK chains: every actor solves the crowd's one list
 *           (rt_crowd_set_ik_chains) with its own targets, poles and weights (rt_crowd_solve_ik); no posing of a sub-range of actors, no
 *           rigs above 1024 joints.  A CHAIN is the kind and the joint of an rt_skeleton_ik: those become addresses, so the host checks
 *           the list once, against the hierarchy that never changes; an actor's VALUES -- a target, a pole and a weight per chain -- are
 *           plain floats that are taken as given, from host or device memory.  Actor a after rt_crowd_solve_ik is, bit for bit, a
 *           skeleton that holds actor a's pose and is given rt_skeleton_solve_ik with the constraints (kind_k, joint_k,
 *           target[a * n + k], pole[a * n + k], weight[a * n + k]): pose, joints and palette, by the definition above ("inverse
 *           kinematics") and by the same statements, for every weight that is not NaN.  A constraint reads W of its chain root's parent
 *           from the pose the actor holds when the call is made -- the actor's joints as the last posing call left them --, as
 *           rt_skeleton_solve_ik does.  The host refuses a NaN weight it sees; a NaN weight in DEVICE memory is no error, and follows
 *           WEIGHT above literally: q_c = A_c + (NaN * (A'_c - A_c)) is NaN in all four components, so the sum of squares is NaN, the
 *           normalisation rule has no answer and every quaternion that constraint writes is (0, 0, 0, 1) -- both joints of a two-bone
 *           chain, the joint of an aim.  The crowd's list may be an ordered list of groups (rt_crowd_set_ik_chain_groups; GROUPS above):
 *           actor a is then a skeleton that holds the actor's pose and is given rt_skeleton_solve_ik_groups with the same constraints,
 *           the value arrays running over the whole list, and all groups of all actors are solved in one launch.  A NaN weight in device
 *           memory does what it does today, and later groups solve against the pose that gives.  Times and weights may be read from device memory (rt_crowd_set_blend_device); the LAYOUT -- which clip, which mask
 *           and which mode every layer of every actor has -- is the host's (rt_crowd_set_layout): those three are indices that become
 *           addresses, so the host checks them once, while a time and a weight are plain floats that are taken as given.  Actor a of
 *           rt_crowd_set_blend_device is, bit for bit, rt_crowd_set_blend with the layout's layers and time = times[a * n_layers + k],
 *           weight = weights[a * n_layers + k] wherever no time is NaN: the segment (i, a) is then found on the device, by the statements
 *           the host finds it with.  The host never sees those times, so a NaN is no error there.  It follows the segment's statements
 *           literally: on a clip of one key it gives (0, 0), the key itself; on any other clip both range tests fail, every comparison of
 *           the search fails and the search ends at i = 0, so it gives (0, NaN) and that layer's sample is NaN.  -inf samples the first
 *           key and +inf the last, as everywhere.  For any 32 bits in `times` the two keys a layer reads are keys of its clip, and the
 *           search reads key times inside [0, n_keys); a weight is never an address.  The call is therefore memory-safe whatever the
 *           arrays hold, and nothing on the device validates, flags or asserts.
 * Validation is done on the host, and nothing changes when a call refuses.  Setting a pose touches no model and no scene.
 * rt_skeleton_create: a null argument is RT_ERR_INVALID_ARG; so is n_joints outside 1 .. 65536 (the skin's bone limit), and a parent that is
 * neither -1 nor < j -- parents come before children -- (the message names the joint).  inverse_bind: n_joints x 12, 3x4 row-major, as
 * instance transforms.  The arrays are copied. */
int rt_skeleton_create(rt_context *ctx, uint32_t n_joints,
                       const int32_t *parents      /* n_joints; -1: a root */,
                       const float *inverse_bind   /* n_joints x 12, 3x4 row-major, as instance transforms */,
                       rt_skeleton **out);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): joins the context's stream first, so destroying a skeleton right
 * after rt_model_set_bones_from_skeleton is legal: the skin kernel already queued reads a live palette. */
int rt_skeleton_destroy(rt_skeleton *sk);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the joints, the levels of the hierarchy (a forest of roots: 1)
 * and the clips; each may be NULL */
int rt_skeleton_get_info(const rt_skeleton *sk, uint32_t *n_joints, uint32_t *n_levels, uint32_t *n_clips);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the local pose, n_joints x 10 floats tx ty tz  qx qy qz qw
 * sx sy sz, and from it W and the palette by the definition above, on the device, on the context's stream.  `mem` is RT_MEM_HOST (the
 * stream is synchronised before the call returns) or RT_MEM_DEVICE (copied device to device into the skeleton's own pose, ordered on the
 * context's stream), as for rt_model_set_bones; a null argument or an unknown `mem` is RT_ERR_INVALID_ARG. */
int rt_skeleton_set_pose(rt_skeleton *sk, const float *trs /* n_joints x 10: tx ty tz  qx qy qz qw  sx sy sz */, uint32_t mem);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): a baked clip, one pose of every joint per key; host arrays.
 * RT_ERR_INVALID_ARG for a null sk, times or trs, for n_keys == 0, for a time that is not finite and for times that do not ascend strictly
 * (the message names the key).  *clip_out (may be NULL) is the clip's id; adding clips keeps earlier clip ids valid. */
int rt_skeleton_add_clip(rt_skeleton *sk, uint32_t n_keys, const float *times /* n_keys */,
                         const float *trs /* n_keys x n_joints x 10, key major */, uint32_t *clip_out);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): removes every clip; ids start at 0 again.  The pose stays. */
int rt_skeleton_clear_clips(rt_skeleton *sk);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): samples clip `clip` at t and poses the skeleton with the result,
 * by the definition above: two kernels on the context's stream, nothing is uploaded and nothing waits.  RT_ERR_INVALID_ARG for a NaN t
 * (-inf and +inf are the first and the last key), RT_ERR_STATE for an unknown clip. */
int rt_skeleton_set_time(rt_skeleton *sk, uint32_t clip, float t);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): a mask for the layers of a blend, one float per joint, taken as
 * given.  The array is copied and stored on the device (the call synchronises the stream, as rt_skeleton_add_clip does).  *mask_out (may be
 * NULL) is the mask's id; adding masks keeps earlier mask ids valid.  A null sk or weights is RT_ERR_INVALID_ARG. */
int rt_skeleton_add_mask(rt_skeleton *sk, const float *weights /* n_joints, host */, uint32_t *mask_out);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): removes every mask, after joining the context's stream (a blend
 * already queued reads live masks); ids start at 0 again.  The pose stays. */
int rt_skeleton_clear_masks(rt_skeleton *sk);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the masks the skeleton holds; a null argument is
 * RT_ERR_INVALID_ARG */
int rt_skeleton_get_num_masks(const rt_skeleton *sk, uint32_t *n);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): blends and layers clips by the definition above ("blending") and
 * poses the skeleton with the result: two kernels on the context's stream, the blend and the pose; nothing is uploaded and nothing waits --
 * the segment, `a`, the weights and the modes of the layers travel as kernel arguments.  Validation runs on the host before anything is
 * queued, and nothing changes when the call refuses; the message names the layer.  RT_ERR_INVALID_ARG: a null argument, n_layers outside
 * 1 .. 8, a NaN time on a layer that samples (-inf and +inf are the first and the last key), an unknown mode, an additive layer 0,
 * RT_SKELETON_CURRENT_POSE on a layer other than 0.  RT_ERR_STATE: an unknown clip or mask id (the message names the layer and how many
 * there are), RT_SKELETON_CURRENT_POSE before the first pose (the message names rt_skeleton_set_pose).  Every layer is held to the first
 * group before any is held to the second.  One layer without a mask is rt_skeleton_set_time, bit for bit. */
int rt_skeleton_set_blend(rt_skeleton *sk, uint32_t n_layers, const rt_skeleton_layer *layers /* n_layers, host */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): solves n (1 .. 32) two-bone reach and aim constraints against the
 * pose the skeleton holds -- from rt_skeleton_set_pose, _set_time, _set_blend or an earlier _solve_ik -- by the definition above ("inverse
 * kinematics"), rewrites the rotation quaternions of the joints it turns and poses the skeleton with the result: two kernels on the context's
 * stream, the solve and the pose; nothing is uploaded and nothing waits -- the constraints travel as a kernel argument.  Stateless, as a blend
 * is.  A frame is _set_blend or _set_time, _solve_ik, rt_model_set_bones_from_skeleton, rt_scene_update.  Validation runs on the host before
 * anything is queued, and nothing changes when the call refuses; the message names the constraint.  RT_ERR_INVALID_ARG: a null argument, n
 * outside 1 .. 32, an unknown kind, a joint >= n_joints (the message gives both numbers), a two-bone tip with fewer than two ancestors (the
 * message names the joint and says why), a NaN weight, two constraints that are not independent (the message names both constraints and the
 * shared joint).  RT_ERR_STATE: the skeleton has no pose yet (the message names rt_skeleton_set_pose).  Every constraint is held to the first
 * group before the state is looked at. */
int rt_skeleton_solve_ik(rt_skeleton *sk, uint32_t n, const rt_skeleton_ik *constraints /* n, host */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): solves an ordered list of n_groups (1 .. 8) groups of
 * constraints, group g being constraints[offset_g .. offset_g + group_sizes[g]), by the definition above ("inverse kinematics", GROUPS): the
 * result is, bit for bit, that of rt_skeleton_solve_ik(sk, group_sizes[g], constraints + offset_g) for g = 0, 1, ... in order.  On a
 * skeleton of at most 1024 joints it is exactly ONE kernel launch on the context's stream, one block that solves a group, walks the pose and
 * meets at a barrier before the next group; nothing is uploaded and nothing waits -- the constraints and the ends of the groups travel as
 * kernel arguments.  A larger skeleton is checked as a whole and then takes the loop of rt_skeleton_solve_ik, two launches per group.
 * Validation runs on the host before anything is queued, and nothing changes when the call refuses.  Refused, in this order: a null argument;
 * n_groups outside 1 .. RT_SKELETON_MAX_IK_GROUPS (group_sizes is not read); a group of size 0 (the message names the group); a total
 * outside 1 .. 32 (no constraint is read); then every constraint of the list held to the rules of rt_skeleton_solve_ik -- kind, joint, two
 * ancestors under a two-bone tip, NaN weight, the messages those of rt_skeleton_solve_ik under this call's name with list indices --; then,
 * group by group, two constraints of one group of which one writes a joint the other reads (the message names both list indices, the joint
 * and the group, and says to put the reader in a later group): all RT_ERR_INVALID_ARG.  RT_ERR_STATE: the skeleton has no pose yet. */
int rt_skeleton_solve_ik_groups(rt_skeleton *sk, uint32_t n_groups, const uint32_t *group_sizes /* n_groups, host */,
                                const rt_skeleton_ik *constraints /* sum of the sizes, host */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the local pose last set or sampled.  This and the calls below
 * that return what a pose made are RT_ERR_STATE before the first pose (the message names rt_skeleton_set_pose); the reads synchronise. */
int rt_skeleton_read_pose(rt_skeleton *sk, float *trs /* n_joints x 10 */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): W_j, n_joints x 12: for attaching instances to joints
 * (rt_scene_set_instance_transform) */
int rt_skeleton_read_joints(rt_skeleton *sk, float *world3x4 /* n_joints x 12 */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): M_j, n_joints x 12 */
int rt_skeleton_read_palette(rt_skeleton *sk, float *palette3x4 /* n_joints x 12 */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the palette where it lives, n_joints x 12 floats of device memory
 * that every later pose overwrites on the context's stream and rt_skeleton_destroy frees */
int rt_skeleton_get_palette_device_ptr(rt_skeleton *sk, void **ptr);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): poses a skinned model from the skeleton's palette.  A null argument
 * is RT_ERR_INVALID_ARG; RT_ERR_STATE before the skeleton's first pose (the message names rt_skeleton_set_pose), for a model without a skin
 * (the message names rt_model_set_skin), for a skin whose n_bones != n_joints (the message gives both numbers) and for a model and a skeleton
 * of different contexts.  Otherwise it is exactly rt_model_set_bones(m, palette, RT_MEM_DEVICE): frames a deferred pipeline still holds are
 * rendered first, the model is left CHANGED and every built scene that holds it STALE until rt_scene_update or rt_scene_build. */
int rt_model_set_bones_from_skeleton(rt_model *m, rt_skeleton *sk);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): a crowd of n_actors poses of `sk` ("crowds" above), which it
 * retains: destroying the skeleton while the crowd lives is legal.  A null argument or n_actors == 0 is RT_ERR_INVALID_ARG; a skeleton of
 * more than 1024 joints is RT_ERR_UNSUPPORTED (the message gives both numbers: an actor's world matrices stand in LDS, and the path through
 * global memory stays the single skeleton's); a device allocation that fails is RT_ERR_OOM.  The crowd has no pose yet. */
int rt_crowd_create(rt_skeleton *sk, uint32_t n_actors, rt_crowd **out);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): joins the context's stream first, as rt_skeleton_destroy does, so
 * destroying a crowd right after rt_model_set_bones_from_crowd is legal; a scene with instances attached to it retains it. */
int rt_crowd_destroy(rt_crowd *c);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the crowd's skeleton, its actors and the joints of each; each
 * may be NULL */
int rt_crowd_get_info(const rt_crowd *c, rt_skeleton **sk, uint32_t *n_actors, uint32_t *n_joints);   /* each may be NULL */
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the local pose of every actor, and from it every actor's W and
 * palette: one copy and one kernel on the context's stream.  `mem` as for rt_skeleton_set_pose: RT_MEM_HOST synchronises the stream before
 * the call returns, RT_MEM_DEVICE copies device to device, ordered on the stream; a null argument or an unknown `mem` is RT_ERR_INVALID_ARG. */
int rt_crowd_set_poses(rt_crowd *c, const float *trs /* n_actors x n_joints x 10 */, uint32_t mem);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): actor a samples clip clips[a] at times[a] and is posed with the
 * result: rt_crowd_set_blend with one layer per actor, without a mask (one layer without a mask is rt_skeleton_set_time, bit for bit).  One
 * upload and one kernel, as for rt_crowd_set_blend.  The refusals are rt_skeleton_set_time's, and the message names the actor: a null
 * argument or a NaN time is RT_ERR_INVALID_ARG, an unknown clip RT_ERR_STATE (after rt_skeleton_clear_clips: every clip); every actor's time
 * is looked at before any actor's clip, and the first bad actor wins. */
int rt_crowd_set_times(rt_crowd *c, const uint32_t *clips /* n_actors */, const float *times /* n_actors */);   /* host arrays */
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): every actor blends and layers clips as rt_skeleton_set_blend
 * does, all actors with n_layers layers, actor a's at layers[a * n_layers].  The per-actor records -- where the two keys and the reference
 * keys of a layer's clip stand, `a`, weight, mask, mode -- cross to the device in ONE upload ordered on the context's stream, and ONE kernel
 * blends and poses every actor.  The call does not wait for the device: the records are staged in two page-locked slots written in turn,
 * each with an event recorded behind the copy out of it, and a slot is waited for only while the copy of the call before last has not
 * passed -- back-to-back calls are safe and wait only when they run two uploads ahead of the device.  Each actor's list is held to the
 * rules of rt_skeleton_set_blend unchanged, and the message names the actor and the layer; the first bad actor wins, and every actor is
 * held to the first group (RT_ERR_INVALID_ARG: mode, additive base, RT_SKELETON_CURRENT_POSE above layer 0, NaN time) before any actor is
 * held to the second (RT_ERR_STATE: unknown clip, unknown mask, RT_SKELETON_CURRENT_POSE before the crowd's first pose -- the message names
 * rt_crowd_set_poses).  A device table that cannot grow is RT_ERR_OOM.  Nothing changes when the call refuses. */
int rt_crowd_set_blend(rt_crowd *c, uint32_t n_layers, const rt_skeleton_layer *layers /* n_actors x n_layers, actor major, host */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the LAYOUT of the crowd ("crowds" above): clip, mask, mode and a
 * default weight of every layer of every actor, all actors with n_layers layers, actor a's at layers[a * n_layers].  The `time` of an entry is
 * not read (a NaN there is fine).  Every actor's list is held to the rules of rt_crowd_set_blend with every time taken as 0 -- the same
 * codes in the same order, every actor to the first group before any to the second, the first bad actor wins, the messages those of
 * rt_crowd_set_blend under this call's name; RT_SKELETON_CURRENT_POSE on layer 0 needs a crowd that has a pose.  One slot per actor and
 * layer -- where the clip's keys and its key times stand on the device, how many keys, the mask or none (the base layer's is dropped), the
 * mode, the weight -- is uploaded ONCE; the call synchronises the stream, as rt_skeleton_add_clip does.  It poses nothing and counts no
 * pose.  The layout stays until the next rt_crowd_set_layout; rt_crowd_set_poses, rt_crowd_set_times and rt_crowd_set_blend neither use it
 * nor disturb it.  A null argument is RT_ERR_INVALID_ARG, a device allocation that fails RT_ERR_OOM.  Nothing changes when the call
 * refuses: the crowd keeps the layout it had. */
int rt_crowd_set_layout(rt_crowd *c, uint32_t n_layers, const rt_skeleton_layer *layers /* n_actors x n_layers, actor major, host */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the layers of the crowd's layout, stale or not; 0: it has none.
 * A null argument is RT_ERR_INVALID_ARG. */
int rt_crowd_get_layout(const rt_crowd *c, uint32_t *n_layers /* 0: none */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): poses every actor from the crowd's layout and times and weights in
 * DEVICE memory: layer k of actor a is the layout's layer with time = times[a * n_layers + k] and weight = weights[a * n_layers + k], or the
 * layout's own weight when `weights` is NULL.  Exactly ONE kernel launch on the context's stream: no upload, no host loop over the actors,
 * no wait -- the host's cost does not grow with actors or layers.  By the definition above ("crowds") actor a is, bit for bit,
 * rt_crowd_set_blend with those layers for times that are not NaN -- pose, joints and palette -- and with a layout of one layer the call is
 * rt_crowd_set_times with the times on the device.  It counts one pose for the whole crowd.  The values are taken as given: NaN, -inf, +inf
 * and any weight are no error, as in rt_skeleton_solve_ik, and the call is memory-safe for any 32 bits in either array ("crowds" above says
 * why).  The caller orders its writes of `times` and `weights` before the call on the context's stream; the arrays are the caller's again once
 * the stream has passed the launch.  A null c or times is RT_ERR_INVALID_ARG.  RT_ERR_STATE: a crowd without a layout, and a STALE layout --
 * rt_skeleton_clear_clips or rt_skeleton_clear_masks has freed what its slots point to since it was set (adding clips or masks keeps ids
 * and addresses, and stales nothing); both messages name rt_crowd_set_layout.  Nothing changes when the call refuses. */
int rt_crowd_set_blend_device(rt_crowd *c, const float *times /* n_actors x n_layers, device */, const float *weights /* n_actors x n_layers, device, or NULL */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the local poses of actors first_actor .. first_actor + count - 1.
 * This and the calls below that return what a pose made are RT_ERR_STATE before the first pose (the message names rt_crowd_set_poses); a
 * range beyond the actors is RT_ERR_INVALID_ARG (the message gives both numbers); the reads synchronise. */
int rt_crowd_read_pose(rt_crowd *c, uint32_t first_actor, uint32_t count, float *trs /* count x n_joints x 10 */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): W_j of those actors, count x n_joints x 12 */
int rt_crowd_read_joints(rt_crowd *c, uint32_t first_actor, uint32_t count, float *world3x4 /* count x n_joints x 12 */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): M_j of those actors, count x n_joints x 12 */
int rt_crowd_read_palette(rt_crowd *c, uint32_t first_actor, uint32_t count, float *palette3x4 /* count x n_joints x 12 */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): W where it lives, n_actors x n_joints x 12 floats of device
 * memory, actor major, that every later posing call overwrites on the context's stream and rt_crowd_destroy frees */
int rt_crowd_get_joints_device_ptr(rt_crowd *c, void **ptr);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the palettes where they live, likewise */
int rt_crowd_get_palette_device_ptr(rt_crowd *c, void **ptr);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): poses a skinned model from actor `actor`'s palette: exactly
 * rt_model_set_bones(m, palette + actor * n_joints * 12, RT_MEM_DEVICE).  The refusals are those of rt_model_set_bones_from_skeleton, with
 * the crowd in the skeleton's place; an actor >= n_actors is RT_ERR_INVALID_ARG (the message gives both numbers). */
int rt_model_set_bones_from_crowd(rt_model *m, rt_crowd *c, uint32_t actor);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the CHAINS of the crowd ("crowds" above): the one list of
 * 1 .. RT_SKELETON_MAX_IK (32) constraints that every actor solves.  Reads `kind` and `joint` of every entry and keeps its `pole` and
 * `weight` as the defaults of rt_crowd_solve_ik calls that bring no poles or no weights; the `target` of an entry is not read.  The list is
 * held to the rules of rt_skeleton_solve_ik unchanged -- the same codes in the same order, the messages those of rt_skeleton_solve_ik under
 * this call's name, the NaN weight being an entry's default weight -- except that it needs no pose: kind, joint, two ancestors under a
 * two-bone tip and independence are matters of the hierarchy, which never changes.  The checked list travels to every solve by value, as a
 * kernel argument: the call poses nothing, counts no pose, touches no device memory and does not wait.  The list stays until the next
 * rt_crowd_set_ik_chains; no other crowd call uses it or disturbs it.  A null argument is RT_ERR_INVALID_ARG.  Nothing changes when the
 * call refuses: the crowd keeps the list it had. */
int rt_crowd_set_ik_chains(rt_crowd *c, uint32_t n, const rt_skeleton_ik *chains /* n, host */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the chains the crowd holds; 0: it has none.  A null argument is
 * RT_ERR_INVALID_ARG. */
int rt_crowd_get_ik_chains(const rt_crowd *c, uint32_t *n /* 0: none */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the chains of the crowd as an ordered list of groups ("inverse
 * kinematics" above, GROUPS): what rt_crowd_set_ik_chains takes, with the list cut into n_groups (1 .. 8) groups of group_sizes[g]
 * entries.  The refusals are those of rt_skeleton_solve_ik_groups in the same order under this call's name, except that a list needs no
 * pose.  rt_crowd_solve_ik keeps its signature and solves whatever list the crowd holds: its value arrays run over the whole list,
 * n_actors x n with n the sum of the sizes, and rt_crowd_get_ik_chains answers that n.  A list of more than one group is exactly ONE launch
 * per rt_crowd_solve_ik, after the one upload where the values are the host's; a list of one group is rt_crowd_set_ik_chains with the same
 * list, bit for bit and launch for launch.  rt_crowd_set_ik_chains sets a list of one group.  Nothing changes when the call refuses: the
 * crowd keeps the list it had. */
int rt_crowd_set_ik_chain_groups(rt_crowd *c, uint32_t n_groups, const uint32_t *group_sizes /* n_groups, host */,
                                 const rt_skeleton_ik *chains /* sum of the sizes, host */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): the groups of the list the crowd holds; 0: it has none.
 * `group_sizes` takes the sizes of the *n_groups groups (room for RT_SKELETON_MAX_IK_GROUPS) and may be NULL.  After rt_crowd_set_ik_chains
 * it says 1 and {n}.  A null c or n_groups is RT_ERR_INVALID_ARG. */
int rt_crowd_get_ik_chain_groups(const rt_crowd *c, uint32_t *n_groups /* 0: none */,
                                 uint32_t *group_sizes /* RT_SKELETON_MAX_IK_GROUPS, or NULL */);
/* EXTENSION (RtModel.cpp:26 and BottomLevelASGenerator.h:136-176 as above): every actor solves the crowd's chains against the pose it holds
 * and is posed with the result ("crowds" above): constraint k of actor a has target targets[(a * n + k) * 3 ..], pole poles[(a * n + k) * 3 ..]
 * and weight weights[a * n + k]; a NULL `poles` or `weights` takes every chain's default.  A frame of a reaching crowd is
 * rt_crowd_set_blend_device, rt_crowd_solve_ik, rt_scene_update.  It counts one pose for the whole crowd.  Refused, in this order: a null c
 * or targets and an unknown `mem` (RT_ERR_INVALID_ARG), a crowd without chains (RT_ERR_STATE; the message names rt_crowd_set_ik_chains), a
 * crowd without a pose (RT_ERR_STATE; the message names rt_crowd_set_poses).
 * RT_MEM_DEVICE: exactly ONE kernel launch on the context's stream: no upload, no host loop over the actors, no wait.  The values are taken
 * as given, as rt_crowd_set_blend_device takes its times: NaN, -inf, +inf and any weight are no error ("crowds" above says what a NaN weight
 * does).  A value never becomes an address -- the joints are those of the host-checked chains -- so the call is memory-safe for any 32 bits
 * in the three arrays.  The caller orders its writes of the arrays before the call on the context's stream; they are the caller's again once
 * the stream has passed the launch.
 * RT_MEM_HOST: the host sees the weights, and a NaN weight is RT_ERR_INVALID_ARG (the message names the actor and the constraint; the first
 * bad actor wins); targets and poles are taken as given, as on a skeleton.  The arrays the call brings cross to the device in ONE upload, one
 * behind another, through the two page-locked staging slots of rt_crowd_set_blend and under their event rule, into a buffer the crowd owns;
 * the same launch follows, and the call does not wait: back-to-back calls are safe.  A device buffer that cannot grow is RT_ERR_OOM.
 * Nothing changes when the call refuses. */
int rt_crowd_solve_ik(rt_crowd *c, const float *targets /* n_actors x n x 3 */, const float *poles /* n_actors x n x 3, or NULL */,
                      const float *weights /* n_actors x n, or NULL */, uint32_t mem /* RT_MEM_HOST | RT_MEM_DEVICE */);

/* Attached instances -- EXTENSIONS: instance transforms that come from the device.  The reference's only statement of a transform is addModel
 * (RtScene.h:30); what these calls write is the Transform member of the instance descriptor
 * (libs/DXRFramework/Helpers/TopLevelASGenerator.cpp:344-362), and the path that applies it is the generators' never-taken update path
 * (`updateOnly` of TopLevelASGenerator::Generate, Helpers/TopLevelASGenerator.h:144-163), as for rt_scene_update.
 * DEVICE-SOURCED TRANSFORMS.  rt_scene_set_instance_transforms_mem with RT_MEM_HOST is exactly rt_scene_set_instance_transforms.  With
 * RT_MEM_DEVICE the count x 12 floats are copied device to device, on the context's stream, into storage the scene owns -- for all of the
 * scene's instances, reserved once (again only when rt_scene_add_model has made the list longer since; what it held then comes down to the host
 * first) -- so the caller's array is free again once the stream has passed the call; a producer on another stream is the caller's to order, as
 * for rt_model_set_vertices.  Nothing is downloaded and nothing waits.  Arguments, refusals, the flush of deferred frames and the STALE rule
 * are exactly those of the host setter: a null argument is RT_ERR_INVALID_ARG, a range beyond the instances RT_ERR_STATE, count == 0 a
 * no-op, on a scene that is not updatable the floats are only stored (the next rt_scene_build reads them); an unknown `mem` is
 * RT_ERR_INVALID_ARG.  rt_scene_update and rt_scene_build fill those instances' slots of the listed transforms from the scene's device
 * storage, with a kernel; host-set instances keep the upload they have; the host copy of the transforms follows in the final join that the
 * update already has (the read-back of the record heads): no new synchronisation goes in front of the kernels.
 * ATTACHMENTS.  An attached instance i with joint j of skeleton sk gets, at every rt_scene_update or rt_scene_build that applies a pose, the
 * transform T_i = W_j o local_i, computed on the device with the product C = A o B exactly as "Posed skeletons" above states it: fp32
 * throughout, every product and every sum one rounded operation, no contraction, always multiplied, for an identity too.  With local3x4 ==
 * NULL, T_i = W_j bit for bit.  Values are taken as given: NaN, inf and zero scales are no errors, as for any instance transform.  From there
 * on T_i is exactly a transform set by rt_scene_set_instance_transforms_mem(RT_MEM_DEVICE): the identity test on the composed floats, the
 * inverse, the world box, the TLAS; after the update the scene is, array for array, the scene a fresh rt_scene_build gives for the same
 * instance list with T_i passed to rt_scene_add_model (DESIGN.md "update == build, with attachments").  A skeleton of roots only, with a
 * clip, is keyframed rigid animation of instances: a frame is rt_skeleton_set_time, rt_scene_update.
 * Attaching stores the binding; `joints` and `local3x4` are copied to the device once (the call synchronises the stream, as
 * rt_skeleton_create does).  On an updatable scene it marks the instances pending and the scene STALE, as a transform setter does; on a scene
 * that is not updatable the next build reads it.  Attaching changes no stored transform: rt_scene_get_instance_transforms returns the old floats
 * until an update or build has applied a pose, and the composed ones afterwards.  Attaching again replaces the binding.
 * Posing a skeleton touches no model and no scene: a built scene stays built and traceable in the state of its last update.  The skeleton
 * counts its poses, and rt_scene_update treats every attached instance whose skeleton has been posed since the scene last applied it as
 * pending -- such an update is no longer the "nothing pending" no-op -- and applies the pose together with pending transforms, masks and
 * changed models, in one call, with one bump of the generation, after the frames a deferred pipeline still holds.  An update or build with
 * an attachment to a skeleton that has no pose yet is RT_ERR_STATE (the message names rt_skeleton_set_pose) and everything pending is kept, as
 * when no instance is visible.  A transform setter of either kind, host or _mem, whose range holds an attached instance is RT_ERR_STATE (the
 * message names the instance and rt_scene_detach_instances) and nothing changes.  Detaching keeps the transform that the last update or build
 * gave the instance and marks nothing; detaching an instance that is not attached is a no-op.
 * rt_scene_attach_instances refuses, and nothing changes when a call refuses: a null argument (s, sk, joints) is RT_ERR_INVALID_ARG; so is
 * a joint >= n_joints (the message names the entry and both numbers); a range beyond the instances is RT_ERR_STATE; so is a skeleton of another
 * context.  count == 0 is a no-op.
 * Lifetime: the scene retains an attached skeleton as it retains its models, until the scene itself goes; rt_skeleton_destroy drops the
 * caller's reference, and the attached instances then simply keep their last transform.  Several scenes, and several instances, may attach to
 * one skeleton, each with its own record of the pose it last applied. */
/* EXTENSION (TopLevelASGenerator.cpp:344-362, RtScene.h:30 and TopLevelASGenerator.h:144-163 as above): rt_scene_set_instance_transforms from
 * host or device memory */
int rt_scene_set_instance_transforms_mem(rt_scene *s, uint32_t first, uint32_t count, const float *transforms3x4 /* count x 12 */,
                                         uint32_t mem /* RT_MEM_HOST | RT_MEM_DEVICE */);
/* EXTENSION (TopLevelASGenerator.cpp:344-362, RtScene.h:30 and TopLevelASGenerator.h:144-163 as above): the twelve floats the scene holds for
 * each of instances first .. first + count - 1, pending or applied, into a host array.  Device-held ones are downloaded on demand: only then
 * does the call synchronise. */
int rt_scene_get_instance_transforms(const rt_scene *s, uint32_t first, uint32_t count, float *transforms3x4 /* host, count x 12 */);
/* EXTENSION (TopLevelASGenerator.cpp:344-362, RtScene.h:30 and TopLevelASGenerator.h:144-163 as above): attaches instances first .. first +
 * count - 1 to joints[k] of `sk`, with local3x4[k] (NULL: none) as above */
int rt_scene_attach_instances(rt_scene *s, uint32_t first, uint32_t count, rt_skeleton *sk,
                              const uint32_t *joints /* count */, const float *local3x4 /* count x 12, or NULL */);
/* EXTENSION (TopLevelASGenerator.cpp:344-362, RtScene.h:30 and TopLevelASGenerator.h:144-163 as above): lets instances first .. first + count
 * - 1 go; a range beyond the instances is RT_ERR_STATE */
int rt_scene_detach_instances(rt_scene *s, uint32_t first, uint32_t count);
/* EXTENSION (TopLevelASGenerator.cpp:344-362, RtScene.h:30 and TopLevelASGenerator.h:144-163 as above): *sk = the skeleton instance `instance`
 * is attached to (NULL: none) and *joint its joint; either pointer may be NULL; an instance out of range is RT_ERR_STATE */
int rt_scene_get_instance_attachment(const rt_scene *s, uint32_t instance, rt_skeleton **sk /* NULL: none */, uint32_t *joint);
/* EXTENSION (TopLevelASGenerator.cpp:344-362, RtScene.h:30 and TopLevelASGenerator.h:144-163 as above): ATTACHMENTS TO A CROWD are
 * attachments as above with W taken from the actor's slice: instance first + k follows joints[k] of actor actors[k] of `c`, T_i = W_j of
 * that actor o local_i.  The pending rule (the crowd counts one pose per posing call), the refusal of an update or build before the crowd's
 * first pose (the message names rt_crowd_set_poses), the refusal of transform setters, detaching, retention until the scene goes and
 * "update == build, with attachments" are those of a skeleton's attachments, by the same code.  A null argument (s, c, actors, joints) is
 * RT_ERR_INVALID_ARG; so is a joint >= n_joints or an actor >= n_actors (the message names the entry and both numbers); a range beyond the
 * instances and a crowd of another context are RT_ERR_STATE.  rt_scene_get_instance_attachment reports skeleton attachments only: none for
 * an instance attached to a crowd.  rt_scene_detach_instances lets go of either kind. */
int rt_scene_attach_instances_crowd(rt_scene *s, uint32_t first, uint32_t count, rt_crowd *c,
                                    const uint32_t *actors /* count */, const uint32_t *joints /* count */, const float *local3x4 /* count x 12, or NULL */);
/* EXTENSION (TopLevelASGenerator.cpp:344-362, RtScene.h:30 and TopLevelASGenerator.h:144-163 as above): *c = the crowd instance `instance`
 * is attached to (NULL: none, also for one attached to a skeleton), *actor and *joint where; each pointer may be NULL; an instance out of
 * range is RT_ERR_STATE */
int rt_scene_get_instance_crowd_attachment(const rt_scene *s, uint32_t instance, rt_crowd **c /* NULL: none */, uint32_t *actor, uint32_t *joint);
/* EXTENSION (TopLevelASGenerator.cpp:344-362, RtScene.h:30 and TopLevelASGenerator.h:144-163 as above; RtModel.cpp:26 and
 * BottomLevelASGenerator.h:136-176 as for the skeleton's other calls): W_j where it lives, n_joints x 12 floats of device memory that every
 * later pose overwrites on the context's stream, as rt_skeleton_get_palette_device_ptr; RT_ERR_STATE before the first pose */
int rt_skeleton_get_joints_device_ptr(rt_skeleton *sk, void **ptr);

/* ---- raw TraceRay over a batch (HLSL TraceRay semantics, used by tests and
 *      the traversal benchmark; ProgressiveRaytracing.hlsl:34,53,
 *      RaytracingCommon.hlsli:94) ------------------------------------------- */

#define RT_MEM_HOST   0u
#define RT_MEM_DEVICE 1u
#define RT_TRACE_FAST       0u   /* production kernel */
#define RT_TRACE_CANONICAL  1u   /* reference-order kernel, also fills the counters */

/* origin_tmin / dir_tmax: n x float4.  Outputs (each may be NULL): t (-1 on
 * miss), u, v, prim, inst (RT_NO_HIT on miss), nodes / tris traversal
 * counters (RT_TRACE_CANONICAL only).  mem says where ALL pointers live. */
int rt_trace_batch(rt_context *ctx, const rt_scene *s,
                   const float *origin_tmin, const float *dir_tmax, size_t n,
                   uint32_t ray_flags, uint32_t kernel, uint32_t mem,
                   float *t, float *u, float *v, uint32_t *prim, uint32_t *inst,
                   uint32_t *cnt_nodes, uint32_t *cnt_tris);
/* average GPU milliseconds of the traversal kernel in the last rt_trace_batch */
int rt_trace_last_ms(rt_context *ctx, float *ms);

/* ---- RaytracingPipeline / ProgressiveRaytracingPipeline
 *      (include/RaytracingPipeline.h:8-39, include/ProgressiveRaytracingPipeline.h:19-40,
 *       src/ProgressiveRaytracingPipeline.cpp) ------------------------------- */

#define RT_PIPELINE_PROGRESSIVE 0u
/* RealtimeRaytracingPipeline (include/RealtimeRaytracingPipeline.h:15-74, src/RealtimeRaytracingPipeline.cpp,
 * assets/shaders/RealtimeRaytracing.hlsl): same traversal and lights, one Phong-lobe bounce, no accumulation,
 * two outputs: 0 = direct lighting, 1 = indirect specular (the DenoiseCompositor's inputs) */
#define RT_PIPELINE_REALTIME    1u

int rt_pipeline_create(rt_context *ctx, uint32_t kind, rt_pipeline **out);   /* ::create  ProgressiveRaytracingPipeline.h:19 */
int rt_pipeline_destroy(rt_pipeline *p);
const char *rt_pipeline_get_name(const rt_pipeline *p);                      /* getName   :40 */
int rt_pipeline_set_scene(rt_pipeline *p, rt_scene *s);                      /* setScene  .cpp:93-97 */
int rt_pipeline_add_material(rt_pipeline *p, const rt_material_params *m);   /* addMaterial .h:30; material i <-> instance i */
int rt_pipeline_set_material(rt_pipeline *p, uint32_t index, const rt_material_params *m);
/* loadResources (.cpp:104-125): the environment cube map (t1/space2).  faces =
 * 6 x size x size RGBA float32, D3D face order +X -X +Y -Y +Z -Z. */
int rt_pipeline_set_environment_cube(rt_pipeline *p, const float *faces_rgba32f, uint32_t size);
int rt_pipeline_set_environment_constant(rt_pipeline *p, const float rgb[3]);
/* RT_CUBE_SEAMLESS (default: what TextureCube.SampleLevel does on any D3D12 device, RaytracingCommon.hlsli:152) or
 * RT_CUBE_FACE_CLAMP */
int rt_pipeline_set_environment_filter(rt_pipeline *p, uint32_t filter);
/* DDS cube map, DXGI_FORMAT_R16G16B16A16_FLOAT or R32G32B32A32_FLOAT, mip 0 used */
int rt_pipeline_load_environment_dds(rt_pipeline *p, const char *path);
/* createOutputResource(format, w, h) (.cpp:127-149); accumulation is always fp32,
 * `format` selects what rt_pipeline_read_output converts to. */
int rt_pipeline_create_output(rt_pipeline *p, uint32_t format, uint32_t width, uint32_t height);
/* Render into caller-owned device memory (w*h*4 floats), e.g. a torch tensor. */
int rt_pipeline_bind_output(rt_pipeline *p, void *device_rgba32f, uint32_t width, uint32_t height);
int rt_pipeline_build_acceleration_structures(rt_pipeline *p);               /* .cpp:99-102 */
/* MAX_RADIANCE_RAY_DEPTH / MAX_SHADOW_RAY_DEPTH (RaytracingCommon.hlsli:11-12); defaults 1, 2 (the values the
 * reference compiles in).  The radiance depth may be raised to 4 (specular chains, BASELINE config 5);
 * more -> RT_ERR_UNSUPPORTED.  The shadow depth is unbounded (levels past the radiance depth cast none). */
int rt_pipeline_set_depth_limits(rt_pipeline *p, uint32_t max_radiance_depth, uint32_t max_shadow_depth);
int rt_pipeline_set_accumulation_mode(rt_pipeline *p, uint32_t mode);        /* RT_ACCUM_* */
/* The reference's accumulation STORAGE: its output texture is DXGI_FORMAT_R16G16B16A16_FLOAT (src/DXRExperimentsApp.cpp:28 ->
 * src/ProgressiveRaytracingPipeline.cpp:127-131) and RayGen read-modify-writes it every frame (assets/shaders/ProgressiveRaytracing.hlsl:36-38):
 * the running mean is read as fp16, formed in fp32 and rounded back to fp16 by the store, every frame.
 *   format = RT_FORMAT_R32G32B32A32_FLOAT (default; north_star's "float accumulation buffer"): the mean stays fp32 from frame to frame, and an
 *            output created as RGBA16F is only converted when it is read;
 *   format = RT_FORMAT_R16G16B16A16_FLOAT: every frame's mean is rounded to fp16 (rounding = RT_ROUND_NEAREST_EVEN, or RT_ROUND_TOWARD_ZERO --
 *            the D3D11 functional spec's rule for float -> lower-precision float; hardware differs, parity unpinned) before the next frame
 *            reads it.  The buffer stays 16 B per pixel (values exactly representable in fp16); RT_ACCUM_SUM images are not rounded.
 * Flushes a deferred set; applies from the next frame. */
int rt_pipeline_set_accumulation_storage(rt_pipeline *p, uint32_t format, uint32_t rounding);
/* evaluateDirectionalLight / evaluatePointLight trace their shadow ray even when N.L == 0 (RaytracingCommon.hlsli:126-147) and
 * then multiply the visibility by that zero.  off (default): they are traversed like every other ray, as in the reference.
 * on: such rays are emitted and counted (rt_stats.rays_shadow) but not traversed (rt_stats.rays_shadow_skipped); the image is
 * bit-identical either way.  Measured: a third of the shadow rays of the bench scene, but they end within a few steps inside
 * the closed geometry they start in, so the frame time does not move; -7 % on the single-sided 10 M-triangle terrain. */
int rt_pipeline_set_skip_unlit_shadow_rays(rt_pipeline *p, int on);
/* The shadow cache: a light buffer of occluders for the any-hit (shadow) searches.  TraceRay with
 * ACCEPT_FIRST_HIT_AND_END_SEARCH (assets/shaders/RaytracingCommon.hlsli:84-96) only asks whether ANY triangle lies between the
 * point and the light; the triangle that last answered that for rays at the same place in light space (the cell of the origin
 * projected along the directional light, the cube-map texel of the direction from the point light) is tested first, and the
 * walk only starts if it does not occlude.  The visibility -- and the image -- are the same bit for bit; the time is not
 * (bench scene: shadow stage -19 %).  cells_per_side: -1 automatic (by triangle count; the option shadow_cache_res overrides),
 * 0 off, else 16..8192 (the table takes 10 * cells^2 bytes, 20 * cells^2 for scenes of several instances). */
int rt_pipeline_set_shadow_cache(rt_pipeline *p, int cells_per_side);
/* cells per side the last rendered frame used (0: it ran without the cache -- AO view, or switched off) */
int rt_pipeline_get_shadow_cache(const rt_pipeline *p, int *cells_per_side);
/* The free sphere around the point light: shootShadowRay towards it (RaytracingCommon.hlsli:84-96, :133-147) ends where no
 * geometry can lie any more -- a lower bound of the light's distance from the nearest triangle, found by a device pass the first
 * frame with a new (scene, light position) queues behind itself and later frames pick up when it has landed; the visibility is
 * the same bit for bit.  Returns the radius in use for the light position of the last update() (0: none known yet, or none
 * possible: the light touches geometry).  Never waits.  Env RT_FREE_RADIUS=0 switches the sphere off. */
int rt_pipeline_get_free_sphere(rt_pipeline *p, float *radius);
int rt_pipeline_clear_output(rt_pipeline *p);
/* update(): the 188-byte constant buffer the reference fills each frame (.cpp:177-213) */
int rt_pipeline_update(rt_pipeline *p, const rt_per_frame_constants *constants);
/* render(cmdList, frameIndex, w, h) (.cpp:215-247): one 1-spp progressive frame. */
int rt_pipeline_render(rt_pipeline *p, uint32_t width, uint32_t height);
/* n frames = n x { update(&constants[i]); render(w, h) } with the same bits in the output, rendered through SHARED sets of
 * launches (up to 32 frames each): the sample-batch mode of BASELINE configs[2] (256 spp accumulated).  The reference issues one
 * DispatchRays per frame (src/ProgressiveRaytracingPipeline.cpp:188-195, :244) and RayGen folds each frame into gOutput
 * with that frame's accumCount (assets/shaders/ProgressiveRaytracing.hlsl:36-38); here the rays of the frames of a batch
 * share the ray queues (a slot's frame selects constants, lights and RNG seed), so the persistent traversal launches and
 * their tails are paid once per batch, and the resolve kernel folds a pixel's frames in frame order -- the running mean is
 * the one n single frames leave.  Frames with accumCount >= maxIterations are skipped (:14-16).  Progressive pipeline only;
 * afterwards the pipeline's constants are constants[n - 1].  Queue memory grows with the batch (1080p: at most 0.47 GB per frame;
 * rt_pipeline_set_queue_budget). */
int rt_pipeline_render_batch(rt_pipeline *p, uint32_t width, uint32_t height, const rt_per_frame_constants *constants, uint32_t n);
/* Reserves everything a set of `frames` frames of width x height allocates -- ray / hit / shadow queues, the set's constants, the
 * shadow cache's table and (scene built) the traversal kernels' global stack rows -- now, so that the first set of that size does
 * not allocate (the counterpart of createOutputResource for the per-frame work memory the reference's Fallback Layer keeps inside
 * DispatchRays).  width x height may be the packed rows of a rank's bands.  Optional: all of it also grows on demand. */
int rt_pipeline_reserve_batch(rt_pipeline *p, uint32_t width, uint32_t height, uint32_t frames);
/* same, restricted to pixel rectangle [x0,x1) x [y0,y1) (tile sharding) */
int rt_pipeline_render_tile(rt_pipeline *p, uint32_t width, uint32_t height,
                            uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1);
/* same, restricted to the interleaved row bands {b : b mod world == rank} of band_rows rows each (rt_tile_bands), all of
 * them in ONE set of launches: the per-frame call of a tile-partitioned multi-GPU run.  band_rows must be a multiple of 8. */
int rt_pipeline_render_bands(rt_pipeline *p, uint32_t width, uint32_t height, uint32_t band_rows, uint32_t rank, uint32_t world);
/* rt_pipeline_render_batch restricted to the rank's bands: n frames of a tile-partitioned run through shared sets of launches
 * (BASELINE configs[4]: at 8 ranks a band set of ONE 4K frame is an eighth of a frame per persistent launch; sets of frames give
 * the launches back their length).  Pixels are seeded by their global index (assets/shaders/ProgressiveRaytracing.hlsl:89), so
 * the rows equal the same rows of n whole frames bit for bit. */
int rt_pipeline_render_bands_batch(rt_pipeline *p, uint32_t width, uint32_t height, uint32_t band_rows, uint32_t rank, uint32_t world,
                                   const rt_per_frame_constants *constants, uint32_t n);
/* Sets of frames BEHIND the reference's own per-frame calls (src/DXRExperimentsApp.cpp:162-165, :194: one update() and one
 * render() per frame; accumulation order src/ProgressiveRaytracingPipeline.cpp:188-195).  With max_frames > 1, rt_pipeline_render
 * records the frame's constants and returns; the recorded frames go through ONE set of launches (rt_pipeline_render_batch:
 * bit for bit the image of rendering each frame at once) as soon as max_frames (<= 32) have gathered, or when a call reads what
 * they produce (read_output, get_output_device_ptr, checkpoints, statistics, the counting re-walks), changes what they would
 * see (scene, materials, environment, output, depth limits, accumulation mode, clear), or synchronises the context.  Errors of
 * a deferred frame surface at the call that flushes it.  Progressive pipeline only; 0 or 1 = render() renders (the default). */
int rt_pipeline_set_deferred(rt_pipeline *p, uint32_t max_frames);
int rt_pipeline_get_deferred(const rt_pipeline *p, uint32_t *max_frames, uint32_t *pending);      /* either may be NULL */
int rt_pipeline_flush(rt_pipeline *p);
/* Queue memory.  A set of launches reserves the worst case of its ray / hit / shadow queues up front when that fits `bytes`
 * (0: the default, a quarter of the device's memory, or the option queue_budget_mb); above it every radiance level is sized by the
 * count the compaction before it has produced (one 4-byte read-back per level and set).  get: bytes reserved now, and whether
 * the last set of launches sized its levels by count. */
int rt_pipeline_set_queue_budget(rt_pipeline *p, size_t bytes);
int rt_pipeline_get_queue_memory(rt_pipeline *p, size_t *bytes_reserved, uint32_t *sized_by_count);
int rt_pipeline_get_num_outputs(const rt_pipeline *p, int *n);               /* getNumOutputs .h:34 */
int rt_pipeline_get_output_device_ptr(rt_pipeline *p, uint32_t id, void **ptr); /* getOutputResource .h:35 */
/* synchronises; host buffer is w*h*4 floats (RGBA32F) or halfs (RGBA16F) */
int rt_pipeline_read_output(rt_pipeline *p, void *host, size_t bytes);
int rt_pipeline_read_output_n(rt_pipeline *p, uint32_t id, void *host, size_t bytes);   /* output id < getNumOutputs() */
/* the inverse of rt_pipeline_read_output for the fp32 accumulation image (w*h*16 bytes): resume of an accumulation */
int rt_pipeline_write_output(rt_pipeline *p, const void *host_rgba32f, size_t bytes);
/* Accumulation checkpoint (the reference loses its accumulation on exit): the fp32 accumulation
 * image plus the host-side state update() carries from frame to frame (mAccumCount, last camera, options, flags,
 * RNG) in one file.  Loading it into a pipeline with an output of the same size and continuing reproduces the
 * uninterrupted run bit for bit.  `h` may be NULL (image only). */
int rt_pipeline_save_checkpoint(rt_pipeline *p, const rt_progressive_host *h, const char *path);
int rt_pipeline_load_checkpoint(rt_pipeline *p, rt_progressive_host *h, const char *path);
/* synchronises; stage timings need rt_pipeline_enable_timing(p, frames > 0): HIP events
 * are recorded around every stage kernel on the context stream, in a ring that
 * remembers the last `frames` frames */
int rt_pipeline_get_stats(rt_pipeline *p, rt_stats *out);
int rt_pipeline_enable_timing(rt_pipeline *p, int frames);
/* sums over every frame since rt_pipeline_reset_totals (ray counts exact; stage times
 * summed over the frames still in the timing ring, out->frames says how many) */
int rt_pipeline_get_totals(rt_pipeline *p, rt_stats *out);
int rt_pipeline_reset_totals(rt_pipeline *p);
/* Re-traces the ray queues of the LAST rendered frame with the canonical traversal and
 * returns its node / triangle counters per stage: out[RT_STAGE_COUNT].  These are the
 * ALGORITHMIC-bytes inputs of the roofline (32 B per node, 36 B per triangle, 48 B per ray). */
int rt_pipeline_count_work(rt_pipeline *p, rt_stage_work *out);
/* Re-walks the ray queues of the LAST rendered frame with a counting instantiation of the PRODUCTION traversal
 * (same tree, same order, same early exits) and returns what it fetched per stage: out[RT_STAGE_COUNT].  Outputs
 * of the frame are rewritten with identical values.  Input of the L2-request roofline. */
int rt_pipeline_count_walk(rt_pipeline *p, rt_stage_walk *out);
/* per-pixel primary-hit records of the last render (tests): w*h each, may be NULL */
int rt_pipeline_read_primary_hits(rt_pipeline *p, float *t, uint32_t *prim, uint32_t *inst);

/* ---- host-side frame logic (src/ProgressiveRaytracingPipeline.cpp:151-213,
 *      libs/MiniEngine/Camera.cpp:19-36) --------------------------------------- */

/* camera = eye[3] at[3] up[3] vfov aspect(width/height) */
int rt_camera_look(const float eye[3], const float at[3], const float up[3], float forward_out[3], float up_out[3]);
int rt_camera_basis(const float forward[3], const float up[3], float vfov, float aspect,
                    float U[4], float V[4], float W[4]);                    /* calculateCameraVariables :151-168 */
int rt_progressive_host_create(uint32_t rng_seed, rt_progressive_host **out);
int rt_progressive_host_destroy(rt_progressive_host *h);
int rt_progressive_host_options(rt_progressive_host *h, rt_debug_options **options);   /* mShaderDebugOptions :74-84 */
int rt_progressive_host_set_flags(rt_progressive_host *h, int accumulation_enabled, int animation_paused);
int rt_progressive_host_reset(rt_progressive_host *h);                      /* frameDirty :309-311 */
/* serialised host state (see rt_pipeline_save_checkpoint): call with buf = NULL to get the size in *bytes */
int rt_progressive_host_save_state(const rt_progressive_host *h, void *buf, size_t capacity, size_t *bytes);
int rt_progressive_host_load_state(rt_progressive_host *h, const void *buf, size_t bytes);
int rt_progressive_host_update(rt_progressive_host *h, const float camera[11], float elapsed_time,
                               uint32_t elapsed_frames, uint32_t width, uint32_t height,
                               rt_per_frame_constants *out);                /* update :177-213 */

/* RealtimeRaytracingPipeline::update (src/RealtimeRaytracingPipeline.cpp:168-199): as above but accumCount = 0 and
 * options = { environmentStrength 1, rest 0 } */
int rt_realtime_host_update(rt_progressive_host *h, const float camera[11], float elapsed_time,
                            uint32_t elapsed_frames, uint32_t width, uint32_t height, rt_per_frame_constants *out);

/* ---- DenoiseCompositor (include/DenoiseCompositor.h:5-59, src/DenoiseCompositor.cpp,
 *      assets/shaders/BilateralFilter.hlsli, DenoiseCommon.hlsli): separable joint-bilateral filter of the
 *      indirect-specular AOV guided by the direct-lighting AOV, then composite + exposure + Reinhard + gamma ---- */
typedef struct rt_denoiser rt_denoiser;
typedef struct rt_denoiser_params {       /* cbuffer Params, DenoiseCommon.hlsli:18-26 */
    float    exposure;                    /* defaults src/DenoiseCompositor.cpp:44-49: 1.0 */
    float    gamma;                       /* 2.2 */
    uint32_t tonemap;                     /* 1 */
    uint32_t gammaCorrect;                /* 0 */
    int32_t  maxKernelSize;               /* 12; taps on each side, <= 20 (the reference's LDS cache extent) */
    uint32_t debugVisualize;              /* 0 composite, 1 denoised only, 2 input, 3 joint */
} rt_denoiser_params;
int rt_denoiser_create(rt_context *ctx, rt_denoiser **out);                                    /* ::create  DenoiseCompositor.h:10 */
int rt_denoiser_destroy(rt_denoiser *d);
int rt_denoiser_get_params(rt_denoiser *d, rt_denoiser_params **params);                       /* mConstantBuffer */
int rt_denoiser_create_output(rt_denoiser *d, uint32_t format, uint32_t width, uint32_t height); /* createOutputResource .cpp:70-93 */
/* dispatch(cmdList, {directLightingSrv, indirectSpecularSrv}, frameIndex, w, h) (.cpp:109-148): inputs are device
 * RGBA32F images, e.g. outputs 0 and 1 of the realtime pipeline */
int rt_denoiser_dispatch(rt_denoiser *d, const void *direct_lighting, const void *indirect_specular, uint32_t width, uint32_t height);
int rt_denoiser_get_output_device_ptr(rt_denoiser *d, void **ptr);                             /* getOutputResource .h:23 */
int rt_denoiser_read_output(rt_denoiser *d, void *host, size_t bytes);                         /* final (pass V) image */
int rt_denoiser_read_intermediate(rt_denoiser *d, void *host, size_t bytes);                   /* pass H image (tests) */
int rt_denoiser_last_ms(rt_denoiser *d, float *ms);

/* ---- multi-GPU: the reference drives one device (src/DXRExperimentsApp.cpp:107-130); a multi-GPU caller is
 *      one such process PER GPU (scene and acceleration structures replicated) and exactly one collective, issued on the
 *      context's stream through RCCL (librccl.so is opened on first use).  Create the processes before any of them
 *      touches the GPU.  examples/progressive_multi.cpp is the worked example; DESIGN.md section 5 the cost model. ---- */
/* host-side partitions (no device needed) */
/* frames {f < n_frames : f mod world == rank} (partition A: sample batches, rendered with RT_ACCUM_SUM) */
int rt_shard_frame_count(uint32_t rank, uint32_t world, uint32_t n_frames, uint32_t *count);
/* interleaved row bands {b : b mod world == rank}, band b = rows [b*band_rows, min((b+1)*band_rows, height)) (partition B:
 * image tiles for rt_pipeline_render_tile); y0 / y1 may be NULL to count */
int rt_tile_bands(uint32_t height, uint32_t band_rows, uint32_t rank, uint32_t world, uint32_t *y0, uint32_t *y1, uint32_t capacity,
                  uint32_t *n_bands);
/* what rt_dist_gather_bands sends per rank: ceil(bands / world) band slots of band_rows x width RGBA32F texels */
int rt_tile_gather_layout(uint32_t width, uint32_t height, uint32_t band_rows, uint32_t world, uint32_t *slots_per_rank, size_t *floats_per_rank);
typedef struct rt_dist rt_dist;
int rt_dist_get_unique_id(void *id128);                                   /* ncclGetUniqueId: rank 0 makes it, the launcher hands it round */
/* ncclCommInitRank on ctx's device.  Before that, the ranks of one node compare the PCI bus ids of their devices through
 * files in /dev/shm named after the id (RT_DIST_CHECK_SECONDS, default 20, 0 = off): two ranks on one device -- where RCCL
 * would fail late or hang -- are RT_ERR_INVALID_ARG here.  (The reference runs on one adapter, NodeMask 0:
 * libs/DXRFramework/RtContext.cpp:37.) */
int rt_dist_create(rt_context *ctx, int rank, int world, const void *id128, rt_dist **out);
int rt_dist_destroy(rt_dist *d);
int rt_dist_get_rank(const rt_dist *d, int *rank, int *world);
/* partition A: in-place SUM all-reduce of `count` floats (the RT_ACCUM_SUM image of rt_pipeline_get_output_device_ptr) */
int rt_dist_all_reduce_sum(rt_dist *d, void *device_f32, size_t count);
/* partition B: every rank holds its own bands of the width x height RGBA32F image; afterwards every rank holds all of it */
int rt_dist_gather_bands(rt_dist *d, void *device_rgba32f, uint32_t width, uint32_t height, uint32_t band_rows);
/* HIP-event time of the last collective on the context's stream (all-reduce; gather: pack + all-gather + unpack); synchronises */
int rt_dist_last_collective_ms(rt_dist *d, float *ms);
/* "0000:c1:00.0"-style PCI bus id of the context's device: what a launcher prints per rank */
int rt_dist_device_pci_bus_id(const rt_context *ctx, char *out, size_t capacity);

/* ---- image files for host copies of the outputs (the reference only blits to its window,
 *      src/DXRExperimentsApp.cpp:213-214).  rgba32f = width*height float4, row 0 on top. ---------------- */
/* lossless fp32 RGBA OpenEXR (single-part scan-line file, no compression, FLOAT channels A B G R) */
int rt_image_write_exr(const char *path, const float *rgba32f, uint32_t width, uint32_t height);
/* lossless fp32 RGB portable float map */
int rt_image_write_pfm(const char *path, const float *rgba32f, uint32_t width, uint32_t height);
/* 8-bit RGB PNG for viewing: v*exposure, optional Reinhard v/(1+v), v^(1/gamma) (the compositor's display
 * transform, DenoiseCommon.hlsli:29-41, with host libm: not a parity path) */
int rt_image_write_png(const char *path, const float *rgba32f, uint32_t width, uint32_t height,
                       float exposure, float gamma, int tonemap);

/* ---- device math probes (tests): evaluate the kernels' deterministic
 *      sin/cos/exp/log/pow/sqrt/div and samplers on the GPU ------------------- */
int rt_debug_math(rt_context *ctx, int fn, const float *x, const float *y, float *out, size_t n);
int rt_debug_sample(rt_context *ctx, int kind, const uint32_t *seeds, const float *vec3_in, float exponent,
                    float *vec3_out, float *pdf_brdf, uint32_t *seeds_out, size_t n);
int rt_debug_read_secondary_ray(rt_pipeline *p, uint32_t index, float origin_tmin[4], float dir_tmax[4]);   /* tools/longest_walk.py */
/* The entry lists the last set of launches started its primary rays from (option primary_entries): *n_tiles = 8x8 tiles of the set's rectangle,
 * row-major (0: the set ran without lists), *cut = the cut the lists were made with.  entries (may be NULL): for the tiles first_tile ..
 * first_tile + count - 1, 33 pairs each of (int32 child code as in rt_scene_wide_read's nodes, float32 bits of tnear); a list ends with
 * the code 0x7FFFFFFE.  tests/test_gpu_primary_entries.py */
int rt_debug_read_primary_entries(rt_pipeline *p, uint32_t first_tile, uint32_t count, uint32_t *entries, uint32_t *n_tiles, uint32_t *cut);
/* Experiment and test knobs of a context, in ONE place (round 5; rounds 1 - 4 read 19 environment variables where they were used).
 * Defaults are the measured best; nothing here changes a result bit -- only which kernels and layouts produce it.  The library
 * reads exactly one environment variable for its behaviour, once, in rt_context_create: RT_DEBUG_OPTIONS="name=value,name=value",
 * applied through this function (an unknown name or a value out of range fails the creation).  (rt_dist also reads the
 * launcher's LOCAL_WORLD_SIZE.)  The reference has no counterpart: its knobs are ImGui widgets (src/ProgressiveRaytracingPipeline.cpp:249-312).
 *   lds_top=0|1              traversal kernels read the top of the tree from LDS (1)
 *   lds_stack_rows=0|6|18    6: the small-stack instantiation of the traversal kernels (tests of the overflow path); 0 / 18: default
 *   persistent_blocks_per_cu=0..16   grid of the persistent launches (0: the occupancy API's answer)
 *   fast_bvh=ploc|lbvh       traversal layout collapsed from the PLOC tree (default) or from the canonical LBVH; set before building
 *   build_batch=0..64        PLOC rounds / collapse levels launched between two looks at the device-side state (0: the builders' estimates)
 *   leaf_max=1..8            triangles per collapsed leaf (2)
 *   wide_sah=0|1, sah_node=x, sah_prim=x   surface-area-optimal collapse and its costs (off; 1.0, 0.5)
 *   verbose=0|1              build phases and structure depths on stderr
 *   shadow_cache_res=-1|0|16..8192   cells per side for pipelines that were not told by rt_pipeline_set_shadow_cache (-1: by triangle count)
 *   shadow_cache_pixels=-1|0|1, primary_persistent=-1|0|1   (-1: on for two-level scenes only)
 *   seven_waves_always=0|1   single frames on the sets' kernels
 *   free_radius=0|1          the free sphere around the point light (1)
 *   batch_max=0..32          frames per set of launches (0: 32)
 *   split_refs=0|1           the traversal layout holds long thin triangles as several references (1; rt_scene_refs_info).  Results do not
 *                            depend on it: the candidate rule follows the references either way
 *   fail_ploc_rounds=0|1     (tests) the PLOC layout of every build is thrown away as if its rounds had made no progress (what non-finite boxes
 *                            cause): the LBVH is collapsed instead
 *   primary_retry_cap=n      entries of the retry list behind the one-tile-per-wave primary launch (0: 2^20; tests make it overflow)
 *   queue_budget_mb=n        worst-case queue bytes a set may reserve up front (0: a quarter of the device's memory)
 *   primary_entries=-1|0|1   primary rays start from their 8x8 tile's list of entry nodes, made once per set of launches, instead of the root
 *                            (-1: sets of at least 4 frames of single-level scenes with lds_top=1 whose primary launch is not persistent -- a
 *                            shorter set does not pay for its lists; a set whose frames do not share the camera's U, V, W runs without
 *                            lists whatever the option says)
 *   primary_entries_cut=0..128   the lists cut the tree below its first n breadth-first nodes (0: 128)
 *   primary_entries_cap=0..32    entries a list may hold before its tile falls back to a coarser cut, at last to the root (0: 32; tests: 1)
 *   dist_check_seconds=x     how long rt_dist_create waits for the other ranks' device ids (5)
 * Every value but fast_bvh's must be a number in full ("true", "4x", "" are RT_ERR_INVALID_ARG, not 0); RT_DEBUG_OPTIONS items must be name=value. */
int rt_debug_set_option(rt_context *ctx, const char *name, const char *value);
/* test hook: device allocations of more than `bytes` bytes fail with RT_ERR_OOM as if the device were full (0: no limit) */
int rt_debug_set_alloc_limit(size_t bytes);
int rt_debug_sample_cube(rt_context *ctx, const float *faces_rgba32f, uint32_t size, uint32_t filter, const float *dirs, float *out, size_t n);
/* ONE step of the traversal engine (csrc/rt_wide_step.h, the function the trace kernels call) per item, from an empty stack, on caller-supplied
 * four-wide nodes in the 64-B layout of rt_scene_wide_read: item i steps on node node_index[i] with the ray origin_tmin[4 i ..] (origin, tmin),
 * dir_tbest[4 i ..] (direction, the far limit of the window).  variant: RT_WIDE_STEP_ANYHIT (the unordered step; else the closest-hit one),
 * RT_WIDE_STEP_DEEP (the instantiation whose stack continues in global rows; else the pure-LDS one), RT_WIDE_STEP_LDS_TOP (the nodes are
 * read from the LDS-resident top: at most 128 nodes; else from global memory).  out: five int32 per item -- the node code entered (0x7FFFFFFE:
 * every child was culled), the stack pointer after the step, and the rows pushed in stack order (INT32_MIN above the stack pointer).
 * tests/test_gpu_wide_step.py holds it to oracle/wide_step_model.h. */
#define RT_WIDE_STEP_ANYHIT  1u
#define RT_WIDE_STEP_DEEP    2u
#define RT_WIDE_STEP_LDS_TOP 4u
int rt_debug_wide_step(rt_context *ctx, const void *nodes, uint32_t n_nodes, const int32_t *node_index, const float *origin_tmin,
                       const float *dir_tbest, size_t n, uint32_t variant, int32_t *out);
/* The DDS cube-map reader behind rt_pipeline_load_environment_dds, without a device (tests run it on the reference's
 * own assets/textures/CathedralRadiance.dds): *size = edge length of mip 0; faces_rgba32f (may be NULL to query the
 * size) receives 6 x size x size x 4 floats when capacity_floats is large enough, else RT_ERR_INVALID_ARG. */
int rt_dds_read_cube(const char *path, float *faces_rgba32f, size_t capacity_floats, uint32_t *size);
/* The OBJ reader behind rt_model_create_from_obj, without a device: counts first (verts / indices NULL), then data. */
int rt_obj_read(const char *path, rt_vertex *verts, uint32_t capacity_verts, uint32_t *indices, uint32_t capacity_tris,
                uint32_t *n_verts, uint32_t *n_tris);
/* The binary-FBX reader behind rt_model_create_from_file, likewise.  The arrays are the file's meshes with the node hierarchy
 * flattened ("FBX ingestion"): Geometry objects in file order, each once per Model it is connected to.
 * RT_ERR_UNSUPPORTED names what is not applied (RotationOrder 6, InheritType 0 / 2 under a scaled ancestor, a singular transform,
 * ASCII FBX); RT_ERR_IO a malformed file (parent cycle, chain deeper than 256, a Model under two Models). */
int rt_fbx_read(const char *path, rt_vertex *verts, uint32_t capacity_verts, uint32_t *indices, uint32_t capacity_tris,
                uint32_t *n_verts, uint32_t *n_tris);

#ifdef __cplusplus
}
#endif
#endif /* DXR_AMD_H */
