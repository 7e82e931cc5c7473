// DXRFramework.h -- header-only C++ mirror of the reference's DXRFramework wrapper
// (libs/DXRFramework/Rt{Context,Model,Scene,Program,State,Bindings,Params}.h) over the
// C ABI in include/dxr_amd.h.  Same class names, same factory / method names and argument
// meaning, same error behaviour (exceptions), so host code written against the reference
// keeps its shape; D3D12 handle types are replaced as listed below.
//
//   ID3D12Device* / ID3D12GraphicsCommandList*   -> device ordinal (+ optional hipStream_t)
//   ID3D12Resource* / descriptor handles          -> device pointers owned by the library
//   DXIL libraries / shader identifiers           -> names of the built-in entry points;
//                                                    RtProgram::Desc records and validates them,
//                                                    there is no runtime shader linking on HIP
//   shader-table records (RtBindings / RtParams)  -> root constants of the hit records are
//                                                    forwarded as per-instance materials
//   DirectX::XMMATRIX                             -> DXRFramework::Matrix (row-vector 4x4, row major)
#pragma once

#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "dxr_amd.h"

// D3D12 types the reference's call sites name, kept so that they compile unchanged (src/DXRExperimentsApp.cpp:186-215):
//   D3D12_GPU_DESCRIPTOR_HANDLE   the reference hands SRV / UAV descriptor-heap handles of its output textures to the
//                                 denoiser; here the handle's 64-bit `ptr` is the DEVICE ADDRESS of the RGBA32F image
//   ID3D12GraphicsCommandList     opaque and never defined: work goes to the RtContext's stream, the argument is ignored
//   D3D12_RESOURCE_STATES         resource barriers have no HIP analogue on one in-order stream: transitionResource is a no-op
struct D3D12_GPU_DESCRIPTOR_HANDLE { unsigned long long ptr; };
struct ID3D12GraphicsCommandList;
enum D3D12_RESOURCE_STATES { D3D12_RESOURCE_STATE_UNORDERED_ACCESS = 0x8, D3D12_RESOURCE_STATE_NON_PIXEL_SHADER_RESOURCE = 0x40 };

namespace DXRFramework
{
    // what the reference's ThrowIfFailed / HrException do (Helpers/DirectXHelper.h:22-64)
    class RtException : public std::runtime_error
    {
    public:
        RtException(int code, const std::string &what) : std::runtime_error(what), mCode(code) {}
        int code() const { return mCode; }
    private:
        int mCode;
    };

    inline void ThrowIfFailed(int rc)
    {
        if (rc != RT_OK) throw RtException(rc, rt_last_error());
    }

    // Row-vector convention like DirectX::XMMATRIX: v' = v * M, translation in row 3.
    struct Matrix
    {
        float m[4][4];
        static Matrix identity()
        {
            Matrix r;
            std::memset(r.m, 0, sizeof r.m);
            r.m[0][0] = r.m[1][1] = r.m[2][2] = r.m[3][3] = 1.0f;
            return r;
        }
        static Matrix translation(float x, float y, float z)
        {
            Matrix r = identity();
            r.m[3][0] = x; r.m[3][1] = y; r.m[3][2] = z;
            return r;
        }
        // first three rows of the transpose: what D3D12_RAYTRACING_INSTANCE_DESC::Transform stores
        // (Helpers/TopLevelASGenerator.cpp:355-357)
        void toInstanceTransform(float out[12]) const
        {
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) out[4 * r + c] = m[c][r];
        }
    };

    class RtBindings;
    class RtState;

    // ---- RtContext (RtContext.h:11-58) -------------------------------------------------
    class RtContext
    {
    public:
        using SharedPtr = std::shared_ptr<RtContext>;

        // reference: create(ID3D12Device*, ID3D12GraphicsCommandList*, bool forceComputeFallback)
        static SharedPtr create(int device = 0, void *hipStream = nullptr, bool useCallerStream = false)
        {
            rt_context *h = nullptr;
            ThrowIfFailed(useCallerStream ? rt_context_create_on_stream(device, hipStream, &h) : rt_context_create(device, &h));
            return SharedPtr(new RtContext(h));
        }
        ~RtContext() { rt_context_destroy(mHandle); }

        rt_context *getHandle() const { return mHandle; }
        int getDevice() const { int d = 0; ThrowIfFailed(rt_context_get_device(mHandle, &d)); return d; }
        void *getStream() const { void *s = nullptr; ThrowIfFailed(rt_context_get_stream(mHandle, &s)); return s; }
        bool isUsingNativeDxr() const { return false; }
        void waitForGpu() { ThrowIfFailed(rt_context_synchronize(mHandle)); }
        // RtContext::transitionResource (RtContext.cpp:224-232): kernels of one stream run in order, nothing to do
        void transitionResource(void *, D3D12_RESOURCE_STATES, D3D12_RESOURCE_STATES) {}

        // raytrace(bindings, state, width, height, depth) (RtContext.cpp:192-222); defined below
        inline void raytrace(std::shared_ptr<RtBindings> bindings, std::shared_ptr<RtState> state, uint32_t width, uint32_t height, uint32_t depth);

    private:
        explicit RtContext(rt_context *h) : mHandle(h) {}
        rt_context *mHandle;
    };

    // ---- RtSkeleton -- EXTENSION: the reference has no counterpart (it imports with aiProcess_PreTransformVertices, RtModel.cpp:26, which
    // drops bones, node animation and all; the update path is the never-taken one, Helpers/BottomLevelASGenerator.h:136-176).  A joint
    // hierarchy posed on the device: create: numJoints parents (-1: a root, else a joint before its child) and 3x4 row-major inverse bind
    // matrices; setPose: numJoints x 10 floats tx ty tz  qx qy qz qw  sx sy sz; addClip: numKeys ascending key times and numKeys x numJoints
    // x 10 floats, returns the clip's id; setTime: samples a clip and poses the skeleton with the result, nothing is uploaded
    // (include/dxr_amd.h "Posed skeletons" states the arithmetic).  A skinned model takes the palette with setBones(skeleton).
    class RtSkeleton
    {
    public:
        using SharedPtr = std::shared_ptr<RtSkeleton>;

        static SharedPtr create(RtContext::SharedPtr context, const int32_t *parents, const float *inverseBind3x4, uint32_t numJoints)
        {
            rt_skeleton *h = nullptr;
            ThrowIfFailed(rt_skeleton_create(context->getHandle(), numJoints, parents, inverseBind3x4, &h));
            return SharedPtr(new RtSkeleton(context, h));
        }
        ~RtSkeleton() { rt_skeleton_destroy(mHandle); }

        rt_skeleton *getHandle() const { return mHandle; }
        RtContext::SharedPtr getContext() const { return mContext; }
        void setPose(const float *trs, bool deviceMemory = false)
        {
            ThrowIfFailed(rt_skeleton_set_pose(mHandle, trs, deviceMemory ? RT_MEM_DEVICE : RT_MEM_HOST));
        }
        uint32_t addClip(const float *times, const float *trs, uint32_t numKeys)
        {
            uint32_t clip = 0;
            ThrowIfFailed(rt_skeleton_add_clip(mHandle, numKeys, times, trs, &clip));
            return clip;
        }
        void setTime(uint32_t clip, float t) { ThrowIfFailed(rt_skeleton_set_time(mHandle, clip, t)); }
        // EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): clips blended and layered on the device.  addMask:
        // numJoints weights, one per joint, returns the mask's id; setBlend: 1 .. RT_SKELETON_MAX_LAYERS layers (rt_skeleton_layer: clip,
        // time, weight, mask, mode), sampled, accumulated and posed on the device, nothing is uploaded
        uint32_t addMask(const float *weights)
        {
            uint32_t mask = 0;
            ThrowIfFailed(rt_skeleton_add_mask(mHandle, weights, &mask));
            return mask;
        }
        void clearMasks() { ThrowIfFailed(rt_skeleton_clear_masks(mHandle)); }
        void setBlend(const rt_skeleton_layer *layers, uint32_t numLayers) { ThrowIfFailed(rt_skeleton_set_blend(mHandle, numLayers, layers)); }
        // EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): 1 .. RT_SKELETON_MAX_IK two-bone reach and aim
        // constraints (rt_skeleton_ik: kind, joint, target, pole, weight) solved on the device against the pose the skeleton holds, and the
        // skeleton posed with the result; nothing is uploaded.  The constraints of one call are independent; dependent ones go into the ordered groups of solveIKGroups
        void solveIK(const rt_skeleton_ik *constraints, uint32_t count) { ThrowIfFailed(rt_skeleton_solve_ik(mHandle, count, constraints)); }
        // EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): numGroups (1 .. RT_SKELETON_MAX_IK_GROUPS) ordered
        // groups of groupSizes[g] constraints over one array: the constraints of a group are independent, a later group sees the pose the
        // earlier ones left -- reach, then aim the hand -- bit for bit one solveIK per group, in one launch (rt_skeleton_solve_ik_groups)
        void solveIKGroups(const rt_skeleton_ik *constraints, const uint32_t *groupSizes, uint32_t numGroups)
        {
            ThrowIfFailed(rt_skeleton_solve_ik_groups(mHandle, numGroups, groupSizes, constraints));
        }

    private:
        RtSkeleton(RtContext::SharedPtr ctx, rt_skeleton *h) : mContext(ctx), mHandle(h) {}
        RtContext::SharedPtr mContext;
        rt_skeleton *mHandle;
    };

    // ---- RtCrowd -- EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): numActors poses of ONE RtSkeleton, all
    // made by one launch (include/dxr_amd.h "Posed skeletons", crowds): actor a is, bit for bit, a skeleton given the same call.  The crowd
    // reads the skeleton's clips and masks where they live and keeps it alive.  setPoses: numActors x numJoints x 10 floats; setTimes: a
    // clip and a time per actor; setBlend: numLayers layers per actor, actor major.  A skinned model takes one actor's palette with
    // setBones(crowd, actor); instances follow actors' joints with RtScene::attach(..., crowd, actors, joints): a frame is one setTimes and
    // one RtScene::update, whatever the number of actors.  setLayout + setBlendDevice: the clips, masks and modes of every actor's layers are
    // checked and uploaded once, and a frame's times and weights are read from DEVICE memory -- one launch, nothing uploaded.  setIKChains +
    // solveIK / solveIKDevice: one list of reach and aim chains for every actor, checked once, and every actor's own targets, poles and
    // weights per frame -- one launch that solves and poses all actors.
    class RtCrowd
    {
    public:
        using SharedPtr = std::shared_ptr<RtCrowd>;

        static SharedPtr create(RtSkeleton::SharedPtr skeleton, uint32_t numActors)
        {
            rt_crowd *h = nullptr;
            ThrowIfFailed(rt_crowd_create(skeleton->getHandle(), numActors, &h));
            return SharedPtr(new RtCrowd(skeleton, h));
        }
        ~RtCrowd() { rt_crowd_destroy(mHandle); }

        rt_crowd *getHandle() const { return mHandle; }
        RtSkeleton::SharedPtr getSkeleton() const { return mSkeleton; }
        RtContext::SharedPtr getContext() const { return mSkeleton->getContext(); }
        uint32_t getNumActors() const { uint32_t n = 0; ThrowIfFailed(rt_crowd_get_info(mHandle, nullptr, &n, nullptr)); return n; }
        void setPoses(const float *trs) { ThrowIfFailed(rt_crowd_set_poses(mHandle, trs, RT_MEM_HOST)); }
        void setPosesDevice(const float *trs) { ThrowIfFailed(rt_crowd_set_poses(mHandle, trs, RT_MEM_DEVICE)); }
        void setTimes(const uint32_t *clips, const float *times) { ThrowIfFailed(rt_crowd_set_times(mHandle, clips, times)); }
        void setBlend(const rt_skeleton_layer *layers, uint32_t numLayers) { ThrowIfFailed(rt_crowd_set_blend(mHandle, numLayers, layers)); }
        // EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): the layout -- clip, mask, mode and a default weight of
        // numLayers layers per actor, actor major; the times are not read -- checked and uploaded once (rt_crowd_set_layout)
        void setLayout(const rt_skeleton_layer *layers, uint32_t numLayers) { ThrowIfFailed(rt_crowd_set_layout(mHandle, numLayers, layers)); }
        uint32_t getLayoutLayers() const { uint32_t n = 0; ThrowIfFailed(rt_crowd_get_layout(mHandle, &n)); return n; }
        // EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): every actor posed from the layout and numActors x
        // numLayers times (and weights; nullptr: the layout's) in DEVICE memory, written on the context's stream: one launch (rt_crowd_set_blend_device)
        void setBlendDevice(const float *times, const float *weights = nullptr) { ThrowIfFailed(rt_crowd_set_blend_device(mHandle, times, weights)); }
        // EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): the chains -- kind and joint of 1 .. RT_SKELETON_MAX_IK
        // constraints, the one list every actor solves, with a default pole and weight each; the targets are not read -- checked once (rt_crowd_set_ik_chains)
        void setIKChains(const rt_skeleton_ik *chains, uint32_t count) { ThrowIfFailed(rt_crowd_set_ik_chains(mHandle, count, chains)); }
        uint32_t getIKChains() const { uint32_t n = 0; ThrowIfFailed(rt_crowd_get_ik_chains(mHandle, &n)); return n; }
        // EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): the chains as numGroups (1 .. RT_SKELETON_MAX_IK_GROUPS)
        // ordered groups of groupSizes[g] entries: what RtSkeleton::solveIKGroups takes, checked once; solveIK / solveIKDevice then solve all
        // groups of all actors in one launch, their value arrays running over the whole list (rt_crowd_set_ik_chain_groups)
        void setIKChainGroups(const rt_skeleton_ik *chains, const uint32_t *groupSizes, uint32_t numGroups)
        {
            ThrowIfFailed(rt_crowd_set_ik_chain_groups(mHandle, numGroups, groupSizes, chains));
        }
        uint32_t getIKChainGroups(uint32_t *groupSizes = nullptr) const { uint32_t n = 0; ThrowIfFailed(rt_crowd_get_ik_chain_groups(mHandle, &n, groupSizes)); return n; }
        // EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): every actor solves the chains against the pose it holds,
        // with numActors x count x 3 targets (and poles, and numActors x count weights; nullptr: the chains' own) from host arrays, and is posed
        // with the result: one upload, one launch (rt_crowd_solve_ik, RT_MEM_HOST)
        void solveIK(const float *targets, const float *poles = nullptr, const float *weights = nullptr)
        {
            ThrowIfFailed(rt_crowd_solve_ik(mHandle, targets, poles, weights, RT_MEM_HOST));
        }
        // EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): ... with the values in DEVICE memory, written on the
        // context's stream: one launch, nothing uploaded (rt_crowd_solve_ik, RT_MEM_DEVICE)
        void solveIKDevice(const float *targets, const float *poles = nullptr, const float *weights = nullptr)
        {
            ThrowIfFailed(rt_crowd_solve_ik(mHandle, targets, poles, weights, RT_MEM_DEVICE));
        }

    private:
        RtCrowd(RtSkeleton::SharedPtr sk, rt_crowd *h) : mSkeleton(sk), mHandle(h) {}
        RtSkeleton::SharedPtr mSkeleton;
        rt_crowd *mHandle;
    };

    // ---- RtModel (RtModel.h:9-40) ------------------------------------------------------
    class RtModel
    {
    public:
        using SharedPtr = std::shared_ptr<RtModel>;

        static SharedPtr create(RtContext::SharedPtr context, const std::string &filePath)
        {
            rt_model *h = nullptr;
            int rc = rt_model_create_from_file(context->getHandle(), filePath.c_str(), &h);      // .fbx or .obj
            if (rc != RT_OK) {
                // the reference substitutes one triangle when the import fails (RtModel.cpp:58-68)
                static const rt_vertex tri[3] = {{{0.0f, 0.25f, 0.0f}, {0, 0, 1}}, {{0.25f, -0.25f, 0.0f}, {0, 0, 1}}, {{-0.25f, -0.25f, 0.0f}, {0, 0, 1}}};
                static const uint32_t idx[3] = {0, 2, 1};
                ThrowIfFailed(rt_model_create_from_arrays(context->getHandle(), tri, 3, idx, 1, &h));
            }
            return SharedPtr(new RtModel(context, h));
        }
        static SharedPtr create(RtContext::SharedPtr context, const rt_vertex *verts, uint32_t numVertices, const uint32_t *indices, uint32_t numTriangles)
        {
            rt_model *h = nullptr;
            ThrowIfFailed(rt_model_create_from_arrays(context->getHandle(), verts, numVertices, indices, numTriangles, &h));
            return SharedPtr(new RtModel(context, h));
        }
        ~RtModel() { rt_model_destroy(mHandle); }

        rt_model *getHandle() const { return mHandle; }
        uint32_t getNumVertices() const { uint32_t v = 0, t = 0; ThrowIfFailed(rt_model_get_counts(mHandle, &v, &t)); return v; }
        uint32_t getNumTriangles() const { uint32_t v = 0, t = 0; ThrowIfFailed(rt_model_get_counts(mHandle, &v, &t)); return t; }

        // EXTENSIONS (the reference's RtModel never changes once created; its generators' `allowUpdate` / `updateOnly` path,
        // Helpers/BottomLevelASGenerator.h:136-176, is never taken): new vertices for a mesh whose counts and index list stay.  setVertices:
        // whole records; setPositions: count x 3 floats, normals kept; deviceMemory: the source is device memory (copied device to device).
        // recomputeNormals: every normal from the current positions, on the device.  Every built scene that holds the model renders nothing
        // until its update() (which rebuilds this model's BLAS) or build().
        void setVertices(const rt_vertex *verts, uint32_t count, uint32_t first = 0, bool deviceMemory = false)
        {
            ThrowIfFailed(rt_model_set_vertices(mHandle, first, count, verts, deviceMemory ? RT_MEM_DEVICE : RT_MEM_HOST));
        }
        void setPositions(const float *xyz, uint32_t count, uint32_t first = 0, bool deviceMemory = false)
        {
            ThrowIfFailed(rt_model_set_positions(mHandle, first, count, xyz, deviceMemory ? RT_MEM_DEVICE : RT_MEM_HOST));
        }
        void recomputeNormals() { ThrowIfFailed(rt_model_recompute_normals(mHandle)); }

        // EXTENSIONS (the reference imports with aiProcess_PreTransformVertices and reads only mVertices / mNormals, RtModel.cpp:26, :38-45:
        // it has no bones; the update path is the never-taken one, Helpers/BottomLevelASGenerator.h:136-176): skeletal animation.  setSkin:
        // numVertices x influences bone indices and weights, vertex major, host arrays; the vertices as they are become the rest pose and stay
        // as they are.  setBones: numBones x 12 floats of 3x4 row-major skinning matrices (pose x inverse bind); the device writes every vertex
        // from the rest pose (include/dxr_amd.h states the arithmetic), and every built scene that holds the model renders nothing until its
        // update() or build().  clearSkin: no skin any more, the vertices stay what the last pose made them.
        void setSkin(const uint32_t *boneIndices, const float *weights, uint32_t influences, uint32_t numBones)
        {
            ThrowIfFailed(rt_model_set_skin(mHandle, influences, numBones, boneIndices, weights));
        }
        void clearSkin() { ThrowIfFailed(rt_model_set_skin(mHandle, 0, 0, nullptr, nullptr)); }
        void setBones(const float *bones3x4, bool deviceMemory = false)
        {
            ThrowIfFailed(rt_model_set_bones(mHandle, bones3x4, deviceMemory ? RT_MEM_DEVICE : RT_MEM_HOST));
        }
        // EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): the palette of a posed RtSkeleton of as many joints
        // as the skin has bones, in place on the device
        void setBones(const RtSkeleton::SharedPtr &skeleton) { ThrowIfFailed(rt_model_set_bones_from_skeleton(mHandle, skeleton->getHandle())); }
        // EXTENSION (RtModel.cpp:26 and Helpers/BottomLevelASGenerator.h:136-176 as above): ... of one actor of a posed RtCrowd
        void setBones(const std::shared_ptr<RtCrowd> &crowd, uint32_t actor) { ThrowIfFailed(rt_model_set_bones_from_crowd(mHandle, crowd->getHandle(), actor)); }

        // EXTENSIONS (the reference reads only mVertices / mNormals of an imported mesh, RtModel.cpp:26, :38-45, never its blend shapes; the
        // update path is the never-taken one, Helpers/BottomLevelASGenerator.h:136-176): morph targets.  setMorphTargets: numTargets sparse
        // targets, target major, host arrays -- target t owns entries targetOffsets[t] .. targetOffsets[t + 1] - 1, entry e adds
        // positionDeltas[3 e ..] (and normalDeltas[3 e ..] unless null) to vertex vertexIndices[e]; the vertices as they are (with a skin: its
        // rest pose) become the base and stay as they are.  setMorphWeights: numTargets weights; the device writes every vertex from the base
        // (include/dxr_amd.h states the arithmetic) -- without a skin into the model's vertices, and every built scene that holds the model
        // renders nothing until its update() or build(); with a skin into the skin's rest pose, which the next setBones poses.
        // clearMorphTargets: no targets any more, the vertices stay what the last call made them.
        void setMorphTargets(uint32_t numTargets, const uint32_t *targetOffsets, const uint32_t *vertexIndices, const float *positionDeltas,
                             const float *normalDeltas = nullptr)
        {
            ThrowIfFailed(rt_model_set_morph_targets(mHandle, numTargets, targetOffsets, vertexIndices, positionDeltas, normalDeltas));
        }
        void clearMorphTargets() { ThrowIfFailed(rt_model_set_morph_targets(mHandle, 0, nullptr, nullptr, nullptr, nullptr)); }
        void setMorphWeights(const float *weights, bool deviceMemory = false)
        {
            ThrowIfFailed(rt_model_set_morph_weights(mHandle, weights, deviceMemory ? RT_MEM_DEVICE : RT_MEM_HOST));
        }

    private:
        RtModel(RtContext::SharedPtr ctx, rt_model *h) : mContext(ctx), mHandle(h) {}
        RtContext::SharedPtr mContext;
        rt_model *mHandle;
    };

    // ---- RtScene (RtScene.h:9-49) ------------------------------------------------------
    class RtScene
    {
    public:
        using SharedPtr = std::shared_ptr<RtScene>;

        // the reference creates scenes before binding them to a context; the handle is made on first use
        static SharedPtr create() { return SharedPtr(new RtScene()); }
        ~RtScene() { if (mHandle) rt_scene_destroy(mHandle); }

        void addModel(RtModel::SharedPtr model, const Matrix &transform) { mInstances.push_back({model, transform, 0xFF}); }
        RtModel::SharedPtr getModel(uint32_t index) const { return mInstances[index].model; }
        uint32_t getNumInstances() const { return static_cast<uint32_t>(mInstances.size()); }

        // build(context, hitGroupCount) (RtScene.cpp:18-52): BLAS per model, then the TLAS
        void build(RtContext::SharedPtr context, uint32_t hitGroupCount)
        {
            realize(context);
            ThrowIfFailed(rt_scene_build(mHandle, hitGroupCount));
        }
        rt_scene *getHandle(RtContext::SharedPtr context) { realize(context); return mHandle; }
        // EXTENSIONS (the reference's RtScene has neither; its generators' update path -- `updateOnly`, Helpers/TopLevelASGenerator.h:144-163 --
        // is never called).  setTransform: a new object-to-world matrix for an instance already added; on a built scene nothing renders
        // until update() or build().  update(context): applies the transforms set since on the device (rt_scene_update); no BLAS is built
        // but those of models whose vertices were set since (RtModel::setVertices / setPositions / recomputeNormals).
        void setTransform(uint32_t index, const Matrix &transform)
        {
            if (index >= mInstances.size()) throw std::runtime_error("RtScene::setTransform: instance out of range");
            mInstances[index].transform = transform;
            if (index < mRealized) {
                float x[12];
                transform.toInstanceTransform(x);
                ThrowIfFailed(rt_scene_set_instance_transform(mHandle, index, x));
            }
        }
        // setInstanceMask / getInstanceMask: the InstanceMask byte of the instance descriptor (Helpers/TopLevelASGenerator.cpp:344-362, 0xFF in
        // the reference); every ray carries the inclusion mask 0xFF, so an instance is hit iff its mask is non-zero.  A pool of instances
        // added up front is shown and hidden with it; a change of visibility is applied by update() or build(), as a transform is.
        void setInstanceMask(uint32_t index, uint8_t mask)
        {
            if (index >= mInstances.size()) throw std::runtime_error("RtScene::setInstanceMask: instance out of range");
            mInstances[index].mask = mask;
            if (index < mRealized) ThrowIfFailed(rt_scene_set_instance_mask(mHandle, index, mask));
        }
        uint8_t getInstanceMask(uint32_t index) const
        {
            if (index >= mInstances.size()) throw std::runtime_error("RtScene::getInstanceMask: instance out of range");
            return mInstances[index].mask;
        }
        void update(RtContext::SharedPtr context)
        {
            realize(context);
            ThrowIfFailed(rt_scene_update(mHandle));
        }
        // EXTENSIONS (the reference's only statement of a transform is addModel, RtScene.h:30; what these write is the Transform member of the
        // instance descriptor, Helpers/TopLevelASGenerator.cpp:344-362, applied by the generators' never-taken update path,
        // Helpers/TopLevelASGenerator.h:144-163): transforms that come from the device (include/dxr_amd.h "Attached instances").
        // setTransforms: count x 12 floats, 3x4 row-major, for instances first .. first + count - 1 of a scene that build(), update() or
        // getHandle() has bound to a context; deviceMemory: the source is device memory, copied device to device on the context's stream --
        // nothing is downloaded and nothing waits.  getTransforms: the floats the scene holds, pending or applied.  attach: the instances
        // follow joints[k] of the skeleton -- at every update() or build() that applies a pose their transform is W_joint o locals[k]
        // (locals == nullptr: W_joint itself), composed on the device: a frame is RtSkeleton::setTime, RtScene::update.  The scene keeps the
        // skeleton alive.  detach: the instances keep the transform their last update() or build() gave them.
        void setTransforms(uint32_t first, uint32_t count, const float *transforms3x4, bool deviceMemory = false)
        {
            requireRealized("RtScene::setTransforms", first, count);
            ThrowIfFailed(rt_scene_set_instance_transforms_mem(mHandle, first, count, transforms3x4, deviceMemory ? RT_MEM_DEVICE : RT_MEM_HOST));
        }
        void getTransforms(uint32_t first, uint32_t count, float *transforms3x4) const
        {
            requireRealized("RtScene::getTransforms", first, count);
            ThrowIfFailed(rt_scene_get_instance_transforms(mHandle, first, count, transforms3x4));
        }
        void attach(uint32_t first, uint32_t count, RtSkeleton::SharedPtr skeleton, const uint32_t *joints, const float *locals = nullptr)
        {
            realize(skeleton->getContext());
            ThrowIfFailed(rt_scene_attach_instances(mHandle, first, count, skeleton->getHandle(), joints, locals));
        }
        // ... of actor actors[k] of a crowd (rt_scene_attach_instances_crowd); the scene keeps the crowd alive
        void attach(uint32_t first, uint32_t count, const std::shared_ptr<RtCrowd> &crowd, const uint32_t *actors, const uint32_t *joints, const float *locals = nullptr)
        {
            realize(crowd->getContext());
            ThrowIfFailed(rt_scene_attach_instances_crowd(mHandle, first, count, crowd->getHandle(), actors, joints, locals));
        }
        void detach(uint32_t first, uint32_t count)
        {
            requireRealized("RtScene::detach", first, count);
            ThrowIfFailed(rt_scene_detach_instances(mHandle, first, count));
        }
        float getUpdateMilliseconds() const { float ms = 0; if (mHandle) rt_scene_update_ms(mHandle, &ms); return ms; }
        float getBuildMilliseconds() const { float ms = 0; if (mHandle) rt_scene_build_ms(mHandle, &ms); return ms; }

    private:
        RtScene() = default;
        struct Node { RtModel::SharedPtr model; Matrix transform; uint8_t mask; };
        // ONE rt_scene handle per RtScene for its whole life (a pipeline that was given the handle by setScene keeps
        // seeing the scene the caller keeps editing, as with the reference's shared RtScene object): instances added
        // since the last call are appended to it
        void realize(RtContext::SharedPtr context)
        {
            if (!mHandle) {
                ThrowIfFailed(rt_scene_create(context->getHandle(), &mHandle));
                mContext = context;
            }
            for (; mRealized < mInstances.size(); mRealized++) {
                float x[12];
                mInstances[mRealized].transform.toInstanceTransform(x);
                ThrowIfFailed(rt_scene_add_model(mHandle, mInstances[mRealized].model->getHandle(), x));
                if (mInstances[mRealized].mask != 0xFF) ThrowIfFailed(rt_scene_set_instance_mask(mHandle, (uint32_t)mRealized, mInstances[mRealized].mask));
            }
        }
        void requireRealized(const char *who, uint32_t first, uint32_t count) const
        {
            if (!mHandle || size_t(first) + count > mRealized)
                throw std::runtime_error(std::string(who) + ": instances beyond those the scene has bound to a context (build() or getHandle() first)");
        }
        std::vector<Node> mInstances;
        RtContext::SharedPtr mContext;
        rt_scene *mHandle = nullptr;
        size_t mRealized = 0;
    };

    // ---- RtProgram (RtProgram.h:17-123): a description of which built-in entry points are used ----
    class RootSignatureGenerator {};   // placeholder for the D3D12 root-signature configurators

    class RtProgram
    {
    public:
        using SharedPtr = std::shared_ptr<RtProgram>;

        class Desc
        {
        public:
            Desc() = default;
            // reference: addShaderLibrary(bytecode, size, exports); here the "library" is the set of kernels
            // compiled into the HIP library, the exports are checked against it at create()
            Desc &addShaderLibrary(const std::vector<std::wstring> &symbolExports) { mExports.insert(mExports.end(), symbolExports.begin(), symbolExports.end()); return *this; }
            Desc &setRayGen(const std::string &raygen) { mRayGen = raygen; return *this; }
            Desc &addMiss(uint32_t missIndex, const std::string &miss)
            {
                if (mMiss.size() <= missIndex) mMiss.resize(missIndex + 1);
                mMiss[missIndex] = miss;
                return *this;
            }
            Desc &addHitGroup(uint32_t hitIndex, const std::string &closestHit, const std::string &anyHit, const std::string &intersection = "")
            {
                if (mHit.size() <= hitIndex) mHit.resize(hitIndex + 1);
                mHit[hitIndex] = {closestHit, anyHit, intersection};
                return *this;
            }
            using RootSignatureConfigurator = std::function<void(RootSignatureGenerator &config)>;
            Desc &configureGlobalRootSignature(RootSignatureConfigurator) { return *this; }
            Desc &configureRayGenRootSignature(RootSignatureConfigurator) { return *this; }
            Desc &configureHitGroupRootSignature(RootSignatureConfigurator) { return *this; }
            Desc &configureMissRootSignature(RootSignatureConfigurator) { return *this; }
        private:
            friend class RtProgram;
            struct Hit { std::string closestHit, anyHit, intersection; };
            std::string mRayGen;
            std::vector<std::string> mMiss;
            std::vector<Hit> mHit;
            std::vector<std::wstring> mExports;
        };

        static SharedPtr create(RtContext::SharedPtr context, const Desc &desc, uint32_t maxPayloadSize = 14 * sizeof(float), uint32_t maxAttributesSize = 32)
        {
            (void)maxPayloadSize; (void)maxAttributesSize;
            // the progressive kernels implement exactly this program (src/ProgressiveRaytracingPipeline.cpp:33-39)
            static const char *known[] = {"RayGen", "PrimaryClosestHit", "PrimaryMiss", "ShadowClosestHit", "ShadowAnyHit", "ShadowMiss", ""};
            auto check = [](const std::string &n) {
                for (const char *k : known) if (n == k) return;
                throw std::logic_error("RtProgram: entry point '" + n + "' is not built into the HIP library");
            };
            check(desc.mRayGen);
            for (const std::string &m : desc.mMiss) check(m);
            for (const Desc::Hit &h : desc.mHit) { check(h.closestHit); check(h.anyHit); check(h.intersection); }
            return SharedPtr(new RtProgram(context, desc));
        }
        uint32_t getHitProgramCount() const { return static_cast<uint32_t>(mDesc.mHit.size()); }
        uint32_t getMissProgramCount() const { return static_cast<uint32_t>(mDesc.mMiss.size()); }
        const std::string &getRayGenProgram() const { return mDesc.mRayGen; }

    private:
        RtProgram(RtContext::SharedPtr ctx, const Desc &d) : mContext(ctx), mDesc(d) {}
        RtContext::SharedPtr mContext;
        Desc mDesc;
    };

    // ---- RtState (RtState.h:10-43) -----------------------------------------------------
    class RtState
    {
    public:
        using SharedPtr = std::shared_ptr<RtState>;
        static SharedPtr create(RtContext::SharedPtr context) { return SharedPtr(new RtState(context)); }

        void setProgram(RtProgram::SharedPtr pProg) { mProgram = pProg; }
        RtProgram::SharedPtr getProgram() const { return mProgram; }
        void setMaxTraceRecursionDepth(uint32_t maxDepth) { mMaxTraceRecursionDepth = maxDepth; }
        uint32_t getMaxTraceRecursionDepth() const { return mMaxTraceRecursionDepth; }
        void setMaxPayloadSize(uint32_t maxSize) { mMaxPayloadSize = maxSize; }
        uint32_t getMaxPayloadSize() const { return mMaxPayloadSize; }
        void setMaxAttributeSize(uint32_t maxSize) { mMaxAttributeSize = maxSize; }
        uint32_t getMaxAttributeSize() const { return mMaxAttributeSize; }

    private:
        explicit RtState(RtContext::SharedPtr ctx) : mContext(ctx) {}
        RtContext::SharedPtr mContext;
        RtProgram::SharedPtr mProgram;
        uint32_t mMaxTraceRecursionDepth = 1, mMaxPayloadSize = 20, mMaxAttributeSize = 8;
    };

    // ---- RtParams (RtParams.h:9-52): root arguments of one shader record ----------------
    class RtParams
    {
    public:
        using SharedPtr = std::shared_ptr<RtParams>;
        static SharedPtr create(uint32_t initialOffset = 0) { return SharedPtr(new RtParams(initialOffset)); }

        void allocateStorage(uint32_t sizeInBytes) { mCapacity = sizeInBytes; }
        void appendHeapRanges(uint64_t gpuHandle) { push(&gpuHandle, 8); }
        void appendDescriptor(uint64_t descriptorHandle) { push(&descriptorHandle, 8); }
        void append32BitConstants(const void *constants, uint32_t num32BitConstants)
        {
            mConstantsOffset = mData.size();
            mNumConstants = num32BitConstants;
            push(constants, 4u * num32BitConstants);
        }
        // storage is consumed by every apply(), callers re-append each frame (RtParams.cpp:17-27)
        void reset() { mData.clear(); mNumConstants = 0; }
        const void *constants() const { return mNumConstants ? mData.data() + mConstantsOffset : nullptr; }
        uint32_t numConstants() const { return mNumConstants; }

    private:
        explicit RtParams(uint32_t initialOffset) : mInitialOffset(initialOffset) {}
        void push(const void *p, size_t n)
        {
            if (mData.size() + n > mCapacity) return;      // out-of-bounds writes are dropped with a log line in the reference (RtParams.cpp:35-37)
            const uint8_t *b = static_cast<const uint8_t *>(p);
            mData.insert(mData.end(), b, b + n);
        }
        std::vector<uint8_t> mData;
        size_t mCapacity = 80, mConstantsOffset = 0;
        uint32_t mNumConstants = 0, mInitialOffset;
    };

    // ---- RtBindings (RtBindings.h:12-67): the shader table ------------------------------
    class RtBindings
    {
    public:
        using SharedPtr = std::shared_ptr<RtBindings>;
        static SharedPtr create(RtContext::SharedPtr context, RtProgram::SharedPtr program, RtScene::SharedPtr scene)
        {
            return SharedPtr(new RtBindings(context, program, scene));
        }

        // (the table grows when instances were added to the scene after the bindings were made)
        const RtParams::SharedPtr &getHitVars(uint32_t rayID, uint32_t meshID)
        {
            auto &perRay = mHitParams.at(rayID);
            while (perRay.size() <= meshID) perRay.push_back(RtParams::create(32));
            return perRay[meshID];
        }
        const RtParams::SharedPtr &getRayGenVars() { return mRayGenParams; }
        const RtParams::SharedPtr &getMissVars(uint32_t rayID) { return mMissParams[rayID]; }
        const RtProgram::SharedPtr &getProgram() { return mProgram; }
        uint32_t getHitProgramsCount() const { return mProgram->getHitProgramCount(); }
        uint32_t getMissProgramsCount() const { return mProgram->getMissProgramCount(); }
        uint32_t getRecordSize() const { return 128; }      // ROUND_UP(32 + 80, 32) (RtBindings.cpp:60-61)

        // apply(context, state) (RtBindings.cpp:100-129): write every record.  Here: the 16 root constants of
        // the ray-type-0 hit record of instance i become material i of the bound pipeline.
        void apply(RtContext::SharedPtr, std::shared_ptr<RtState>)
        {
            if (!mPipeline) throw std::logic_error("RtBindings::apply: no pipeline bound");
            for (uint32_t inst = 0; inst < mHitParams[0].size(); ++inst) {
                RtParams::SharedPtr p = mHitParams[0][inst];
                if (p->numConstants() == sizeof(rt_material_params) / 4) {
                    rt_material_params m;
                    std::memcpy(&m, p->constants(), sizeof m);
                    if (inst < mMaterialsSet) ThrowIfFailed(rt_pipeline_set_material(mPipeline, inst, &m));
                    else { ThrowIfFailed(rt_pipeline_add_material(mPipeline, &m)); mMaterialsSet++; }
                }
            }
            for (auto &perRay : mHitParams) for (auto &p : perRay) p->reset();
            for (auto &p : mMissParams) p->reset();
        }
        void bindPipeline(rt_pipeline *p) { mPipeline = p; }
        rt_pipeline *getPipeline() const { return mPipeline; }

    private:
        RtBindings(RtContext::SharedPtr, RtProgram::SharedPtr program, RtScene::SharedPtr scene) : mProgram(program), mScene(scene)
        {
            mRayGenParams = RtParams::create(32);
            mHitParams.resize(program->getHitProgramCount());
            for (auto &perRay : mHitParams)
                for (uint32_t j = 0; j < scene->getNumInstances(); ++j) perRay.push_back(RtParams::create(32));
            for (uint32_t i = 0; i < program->getMissProgramCount(); ++i) mMissParams.push_back(RtParams::create(32));
        }
        RtProgram::SharedPtr mProgram;
        RtScene::SharedPtr mScene;
        RtParams::SharedPtr mRayGenParams;
        std::vector<std::vector<RtParams::SharedPtr>> mHitParams;
        std::vector<RtParams::SharedPtr> mMissParams;
        rt_pipeline *mPipeline = nullptr;
        uint32_t mMaterialsSet = 0;
    };

    inline void RtContext::raytrace(std::shared_ptr<RtBindings> bindings, std::shared_ptr<RtState>, uint32_t width, uint32_t height, uint32_t depth)
    {
        (void)depth;      // the reference passes Depth = 3 and only uses .xy of the launch index (ProgressiveRaytracingPipeline.cpp:244)
        ThrowIfFailed(rt_pipeline_render(bindings->getPipeline(), width, height));
    }
}
