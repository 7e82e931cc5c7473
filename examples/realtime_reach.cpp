// A pose that meets the scene, through the reference-shaped C++ API: the tube and the four-joint chain of realtime_character.cpp, played
// from its baked clip (RtSkeleton::setTime), and then made to REACH -- a target is carried round a circle, a two-bone constraint on joints
// 1-2-3 puts the chain's last joint on it, and a second root joint with a box attached to it (RtScene::attach) is AIMED at the same target in
// the same call (RtSkeleton::solveIK: the two constraints are independent).  Per frame the host sends one float of time and two constraints
// of 36 bytes as kernel arguments: setTime, solveIK, RtModel::setBones(skeleton), RtScene::update -- nothing is read back to solve on the
// host and no pose is uploaded (extensions: the reference imports with aiProcess_PreTransformVertices, RtModel.cpp:26, which drops bones and
// node animation, and never takes its generators' update path, Helpers/BottomLevelASGenerator.h:136-176).  The joints are read back each
// frame (rt_skeleton_read_joints) only to print how far the tip ended from the target and the box's axis from the target's direction.
// Rendered by the RealtimeRaytracingPipeline and filtered by the DenoiseCompositor; the denoised last frame is written as a PNG or PFM.
//
//   realtime_reach <width> <height> <frames> <out.png|out.pfm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "DenoiseCompositor.h"
#include "RealtimeRaytracingPipeline.h"

using namespace DXRFramework;

namespace {

const uint32_t JOINTS = 5, KEYS = 3, TIP = 3, TURRET = 4;

// a cube of side 1 about the origin: four vertices per face, with the face's normal
void cube(std::vector<rt_vertex> &verts, std::vector<uint32_t> &indices)
{
    for (int axis = 0; axis < 3; ++axis)
        for (int side = -1; side <= 1; side += 2) {
            const uint32_t base = (uint32_t)verts.size();
            for (int corner = 0; corner < 4; ++corner) {
                float p[3], nrm[3] = {0.0f, 0.0f, 0.0f};
                p[axis] = 0.5f * float(side);
                p[(axis + 1) % 3] = (corner & 1) ? 0.5f : -0.5f;
                p[(axis + 2) % 3] = (corner & 2) ? 0.5f : -0.5f;
                nrm[axis] = float(side);
                verts.push_back({{p[0], p[1], p[2]}, {nrm[0], nrm[1], nrm[2]}});
            }
            if (side > 0) indices.insert(indices.end(), {base, base + 1, base + 3, base, base + 3, base + 2});
            else indices.insert(indices.end(), {base, base + 3, base + 1, base, base + 2, base + 3});
        }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s width height frames out.png|out.pfm\n", argv[0]);
        return 2;
    }
    const UINT width = std::atoi(argv[1]), height = std::atoi(argv[2]), frames = std::atoi(argv[3]);
    try {
        // the tube: RINGS rings of SEGS vertices about the y axis, y = -1.5 .. 1.5, radius 0.35.  Joint j < 4 sits at y = -1.5 + 0.75 j; a
        // vertex follows the two joints about it, half and half where the upper one sits, with a smooth crossover
        const uint32_t RINGS = 32, SEGS = 48, CHAIN = 4;
        const float SPAN = 0.75f;
        std::vector<rt_vertex> verts;
        std::vector<uint32_t> indices, bones;
        std::vector<float> weights;
        for (uint32_t r = 0; r < RINGS; ++r)
            for (uint32_t s = 0; s < SEGS; ++s) {
                const float a = 6.2831853f * float(s) / float(SEGS), y = -1.5f + 3.0f * float(r) / float(RINGS - 1);
                verts.push_back({{0.35f * std::cos(a), y, 0.35f * std::sin(a)}, {std::cos(a), 0.0f, std::sin(a)}});
                const float c = (y + 1.5f) / SPAN - 0.5f;
                const uint32_t k0 = c <= 0.0f ? 0u : c >= float(CHAIN - 1) ? CHAIN - 1 : uint32_t(c), k1 = k0 + 1 < CHAIN ? k0 + 1 : k0;
                float t = c - float(k0);
                t = t < 0.0f ? 0.0f : t > 1.0f ? 1.0f : t;
                const float w1 = t * t * (3.0f - 2.0f * t);
                bones.push_back(k0); bones.push_back(k1);
                weights.push_back(1.0f - w1); weights.push_back(w1);
            }
        for (uint32_t r = 0; r + 1 < RINGS; ++r)
            for (uint32_t s = 0; s < SEGS; ++s) {
                const uint32_t a = r * SEGS + s, b = r * SEGS + (s + 1) % SEGS, c = a + SEGS, d = b + SEGS;
                indices.insert(indices.end(), {a, c, b, b, c, d});
            }
        const uint32_t n = (uint32_t)verts.size(), tris = (uint32_t)(indices.size() / 3);
        std::vector<rt_vertex> boxVerts;
        std::vector<uint32_t> boxIndices;
        cube(boxVerts, boxIndices);

        // the chain: joint 0 a root at the tube's lower end, joints 1 .. 3 each SPAN above their parent; joint 4 a second root beside the
        // tube, the turret.  The inverse bind matrices undo the chain's rest pose; the turret skins nothing
        const int32_t parents[JOINTS] = {-1, 0, 1, 2, -1};
        const float turretAt[3] = {-2.0f, -0.75f, 0.0f};
        float inverseBind[JOINTS * 12] = {};
        for (uint32_t j = 0; j < JOINTS; ++j) {
            inverseBind[12 * j] = inverseBind[12 * j + 5] = inverseBind[12 * j + 10] = 1.0f;
            if (j < CHAIN) inverseBind[12 * j + 7] = 1.5f - SPAN * float(j);
        }
        // the clip: the bind pose, every joint of the chain above its root turned about z, then about x the other way; the turret stays
        const float times[KEYS] = {0.0f, 1.0f, 2.0f};
        const float turns[KEYS][4] = {{0, 0, 0, 1}, {0, 0, std::sin(0.3f), std::cos(0.3f)}, {std::sin(-0.25f), 0, 0, std::cos(-0.25f)}};
        float keys[KEYS * JOINTS * 10];
        for (uint32_t k = 0; k < KEYS; ++k)
            for (uint32_t j = 0; j < JOINTS; ++j) {
                float *trs = keys + (k * JOINTS + j) * 10;
                trs[0] = 0.0f; trs[1] = j == 0 ? -1.5f : SPAN; trs[2] = 0.0f;
                if (j == TURRET)
                    for (int c = 0; c < 3; ++c) trs[c] = turretAt[c];
                for (int c = 0; c < 4; ++c) trs[3 + c] = (j == 0 || j == TURRET) ? turns[0][c] : turns[k][c];
                trs[7] = trs[8] = trs[9] = 1.0f;
            }
        // the box on the turret: a pointer along the joint's +y, the axis that is aimed
        const uint32_t turretJoint[1] = {TURRET};
        const float turretLocal[12] = {0.2f, 0, 0, 0, 0, 1.0f, 0, 0.5f, 0, 0, 0.2f, 0};

        auto context = RtContext::create(0);
        auto scene = RtScene::create();
        auto model = RtModel::create(context, verts.data(), n, indices.data(), tris);
        model->setSkin(bones.data(), weights.data(), 2, JOINTS);  // the vertices as created are the rest pose
        auto box = RtModel::create(context, boxVerts.data(), (uint32_t)boxVerts.size(), boxIndices.data(), (uint32_t)(boxIndices.size() / 3));
        auto skeleton = RtSkeleton::create(context, parents, inverseBind, JOINTS);
        const uint32_t clip = skeleton->addClip(times, keys, KEYS);
        auto pipeline = RealtimeRaytracingPipeline::create(context);
        scene->addModel(model, Matrix::translation(0.0f, 0.0f, 0.0f));
        scene->addModel(box, Matrix::translation(0.0f, 0.0f, 0.0f));             // (where the first pose puts it is decided below)
        for (int m = 0; m < 2; ++m) {
            RaytracingPipeline::Material material{};
            material.params.albedo = {m ? 0.85f : 0.3f, 0.6f, m ? 0.3f : 0.85f, 1.0f};
            material.params.specular = {0.58f, 0.58f, 0.58f, 1.0f};
            material.params.roughness = 0.5f;
            material.params.reflectivity = 0.7f;
            material.params.type = 0;
            pipeline->addMaterial(material);
        }
        skeleton->setTime(clip, 0.0f);                    // a pose for the build to apply
        scene->attach(1, 1, skeleton, turretJoint, turretLocal);

        auto camera = std::make_shared<Math::Camera>();
        camera->SetAspectRatio(float(width) / float(height));
        camera->SetEyeAtUp({-0.5f, 0.5f, 6.0f}, {-0.5f, 0.0f, 0.0f}, {0, 1, 0});

        pipeline->setScene(scene);
        pipeline->setCamera(camera);
        pipeline->loadResources(3);
        pipeline->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);
        pipeline->buildAccelerationStructures();

        auto denoiser = DenoiseCompositor::create(context);
        denoiser->loadResources(3, false);
        denoiser->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);

        double update_ms = 0.0, pose_ms = 0.0, worstTip = 0.0, worstAim = 0.0;
        const auto t0 = std::chrono::steady_clock::now();
        for (UINT frame = 1; frame <= frames; ++frame) {
            const float t = std::fmod(0.1f * float(frame), times[KEYS - 1]);      // (looping is the caller's)
            // the target goes round a circle that the chain can reach from joint 1 (at most 1.39 away; the two bones are 1.5 long)
            const float phi = 0.35f * float(frame);
            const float target[3] = {0.7f * std::cos(phi), 0.15f + 0.3f * std::sin(phi), 0.7f * std::sin(phi)};
            rt_skeleton_ik constraints[2] = {};
            constraints[0].kind = RT_IK_TWO_BONE;
            constraints[0].joint = TIP;
            constraints[0].pole[2] = 3.0f;                // the middle joint bends towards the camera's side
            constraints[1].kind = RT_IK_AIM;
            constraints[1].joint = TURRET;
            constraints[1].pole[1] = 1.0f;                // the axis: the turret's +y
            for (int k = 0; k < 2; ++k) {
                std::memcpy(constraints[k].target, target, sizeof target);
                constraints[k].weight = 1.0f;
            }
            const auto p0 = std::chrono::steady_clock::now();
            skeleton->setTime(clip, t);                   // one float: the clip is sampled and the chain posed on the device
            skeleton->solveIK(constraints, 2);            // the played pose meets the target: two lanes of one wave, then the pose kernel again
            model->setBones(skeleton);                    // the palette is used where it lies
            pose_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - p0).count();
            scene->update(context);                       // the tube's BLAS rebuilt, the box's transform composed from its joint, the TLAS: on the device
            update_ms += scene->getUpdateMilliseconds();
            float W[JOINTS * 12];
            ThrowIfFailed(rt_skeleton_read_joints(skeleton->getHandle(), W));
            double tip = 0.0, len = 0.0, far = 0.0;
            for (int r = 0; r < 3; ++r) {
                const double d = double(W[12 * TIP + 4 * r + 3]) - target[r], g = double(target[r]) - turretAt[r], y = W[12 * TURRET + 4 * r + 1];
                tip += d * d; len += y * y; far += g * g;
            }
            double aim = 0.0;                              // | unit(the turret's +y) - unit(target - turret) |
            for (int r = 0; r < 3; ++r) {
                const double e = W[12 * TURRET + 4 * r + 1] / std::sqrt(len) - (double(target[r]) - turretAt[r]) / std::sqrt(far);
                aim += e * e;
            }
            worstTip = std::fmax(worstTip, std::sqrt(tip));
            worstAim = std::fmax(worstAim, std::sqrt(aim));
            pipeline->update(0.0f, frame, (frame + 2) % 3, frame % 3, width, height);
            pipeline->render(frame % 3, width, height);
            DenoiseCompositor::InputComponents inputs = {};
            inputs.directLightingSrv = pipeline->getOutputSrvHandle(0);
            inputs.indirectSpecularSrv = pipeline->getOutputSrvHandle(1);
            denoiser->dispatch(nullptr, inputs, frame % 3, width, height);
        }
        std::vector<float> image(size_t(width) * height * 4);
        denoiser->readOutput(image.data(), image.size() * sizeof(float));
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%s, %u skinned vertices, %u triangles, %u joints, 2 constraints solved on the device: %u frames, %.2f fps, %.3f ms per frame, posing calls "
                    "%.3f ms per frame on the host, BLAS + TLAS update %.3f ms per frame on the device\n",
                    pipeline->getName(), n, tris, JOINTS, frames, frames / s, frames ? 1e3 * s / frames : 0.0, frames ? pose_ms / frames : 0.0,
                    frames ? update_ms / frames : 0.0);
        std::printf("largest tip-to-target distance %.3e of a chain %.2f long, largest aim error %.3e\n", worstTip, 2.0 * SPAN, worstAim);

        const std::string out = argv[4];
        const bool png = out.size() > 4 && out.compare(out.size() - 4, 4, ".png") == 0;
        ThrowIfFailed(png ? rt_image_write_png(out.c_str(), image.data(), width, height, 1.0f, 1.0f, 0)
                          : rt_image_write_pfm(out.c_str(), image.data(), width, height));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
