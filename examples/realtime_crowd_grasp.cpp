// A crowd that GRASPS, through the reference-shaped C++ API: the crowd of realtime_crowd_reach.cpp -- 196 four-joint arms on a grid, each made
// of boxes attached to its joints (RtScene::attach), every one played from its own clip -- with a SECOND group of constraints.  Group 0 is the
// reach of realtime_crowd_reach.cpp: one two-bone constraint on joints 1-2-3 that puts the last joint, the hand, on the actor's own grasp
// point.  Group 1 aims the hand: joint 3 is turned until its bone axis points at the actor's target, the thing it reaches for, which hangs a
// little above the grasp point and is carried round a circle above the arm's foot.  The aim depends on the reach -- it reads the world
// matrix the reach has just given joint 2 --, so one list of independent constraints refuses the pair; as an ordered list of two groups,
// set once with RtCrowd::setIKChainGroups, it is one call and one launch.  The values are the actors': every actor's grasp point and target
// for EVERY frame, its pole, its axis and its clip times are made up front with + - * / alone and uploaded ONCE (rt_device_alloc,
// rt_device_upload).  Per frame the host makes ONE RtCrowd::setBlendDevice, ONE RtCrowd::solveIKDevice and ONE RtScene::update: two launches
// sample, reach, aim and pose all 196 hierarchies, and nothing is uploaded inside the loop (extensions: the reference imports with
// aiProcess_PreTransformVertices, RtModel.cpp:26, which drops bones and node animation, states a transform only in addModel, RtScene.h:30,
// and never takes its generators' update path, Helpers/BottomLevelASGenerator.h:136-176).  The joints are read back each frame
// (rt_crowd_read_joints) only to print how far the hands ended from their grasp points and how far their axes from the directions to their
// targets; at the end actor 0 is compared, byte for byte, with an RtSkeleton given the same pose and RtSkeleton::solveIKGroups.  Rendered
// by the RealtimeRaytracingPipeline and filtered by the DenoiseCompositor; the denoised last frame is written as a PNG or PFM.
//
//   realtime_crowd_grasp <width> <height> <frames> <out.png|out.pfm>
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

const uint32_t JOINTS = 4, KEYS = 3, TIP = 3, SIDE = 14, ACTORS = SIDE * SIDE;
const uint32_t CHAINS = 2;                  // per actor: the reach (group 0), then the aim of the hand (group 1)
const float SPAN = 0.75f, PITCH = 3.0f, LIFT = 0.35f;

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

// where actor a's arm stands
void footOf(uint32_t a, float &x, float &z)
{
    x = PITCH * (float(a % SIDE) - 0.5f * float(SIDE - 1));
    z = PITCH * (float(a / SIDE) - 0.5f * float(SIDE - 1));
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
        std::vector<rt_vertex> verts;
        std::vector<uint32_t> indices;
        cube(verts, indices);

        // the chain of realtime_reach.cpp: joint 0 a root at the arm's foot, joints 1 .. 3 each SPAN above their parent
        const int32_t parents[JOINTS] = {-1, 0, 1, 2};
        float inverseBind[JOINTS * 12] = {};
        for (uint32_t j = 0; j < JOINTS; ++j) inverseBind[12 * j] = inverseBind[12 * j + 5] = inverseBind[12 * j + 10] = 1.0f;
        // the clip of an actor: the bind pose on the actor's square, every joint above the root turned about z, then about x the other way
        const float times[KEYS] = {0.0f, 1.0f, 2.0f};
        const float turns[KEYS][4] = {{0, 0, 0, 1}, {0, 0, 0.29552021f, 0.95533649f}, {-0.24740396f, 0, 0, 0.96891242f}};      // (0.3 about z, -0.25 about x, each a half angle)
        auto clipOf = [&](uint32_t a, float *keys) {
            float x, z;
            footOf(a, x, z);
            for (uint32_t k = 0; k < KEYS; ++k)
                for (uint32_t j = 0; j < JOINTS; ++j) {
                    float *trs = keys + (k * JOINTS + j) * 10;
                    trs[0] = j == 0 ? x : 0.0f; trs[1] = j == 0 ? -1.5f : SPAN; trs[2] = j == 0 ? z : 0.0f;
                    for (int c = 0; c < 4; ++c) trs[3 + c] = j == 0 ? turns[0][c] : turns[k][c];
                    trs[7] = trs[8] = trs[9] = 1.0f;
                }
        };
        // a box per joint: a bone from the joint to its child, and a small cube on the tip
        std::vector<uint32_t> instActors(ACTORS * JOINTS), instJoints(ACTORS * JOINTS);
        std::vector<float> locals(ACTORS * JOINTS * 12, 0.0f);
        for (uint32_t a = 0; a < ACTORS; ++a)
            for (uint32_t j = 0; j < JOINTS; ++j) {
                const uint32_t i = a * JOINTS + j;
                instActors[i] = a;
                instJoints[i] = j;
                const bool tip = j == TIP;
                locals[12 * i] = locals[12 * i + 10] = tip ? 0.4f : 0.25f;
                locals[12 * i + 5] = tip ? 0.4f : SPAN;
                locals[12 * i + 7] = tip ? 0.0f : 0.5f * SPAN;
            }

        auto context = RtContext::create(0);
        auto scene = RtScene::create();
        auto model = RtModel::create(context, verts.data(), (uint32_t)verts.size(), indices.data(), (uint32_t)(indices.size() / 3));
        auto pipeline = RealtimeRaytracingPipeline::create(context);
        for (uint32_t i = 0; i < ACTORS * JOINTS; ++i) {
            scene->addModel(model, Matrix::translation(0.0f, 0.0f, 0.0f));      // (where the first pose puts it is decided below)
            RaytracingPipeline::Material material{};
            material.params.albedo = {i % JOINTS == TIP ? 0.85f : 0.3f, 0.6f, i % JOINTS == TIP ? 0.3f : 0.85f, 1.0f};
            material.params.specular = {0.58f, 0.58f, 0.58f, 1.0f};
            material.params.roughness = 0.5f;
            material.params.reflectivity = 0.7f;
            material.params.type = 0;
            pipeline->addMaterial(material);
        }

        // the tables of every frame: actor a plays its clip at its own time (the clip loops, and the actors start spread over it) and its
        // grasp point goes round a circle that its chain can reach from joint 1 (at most 1.39 away; the two bones are 1.5 long), at its own
        // phase; the target hangs LIFT above the grasp point.  The circle is the rational one, (1 - u u) / (1 + u u) and 2 u / (1 + u u),
        // a half per sign: every float here comes from + - * / and fmod alone, so that tests/golden/make_ik_group_bounds.py restates them
        // bit for bit.  Per actor and frame the values of the list: entry 0 the reach's, entry 1 the aim's.
        std::vector<float> timeTable(size_t(frames + 1) * ACTORS), targetTable(size_t(frames + 1) * ACTORS * CHAINS * 3), poles(ACTORS * CHAINS * 3);
        for (uint32_t a = 0; a < ACTORS; ++a) {
            float x, z;
            footOf(a, x, z);
            float *pole = &poles[size_t(a) * CHAINS * 3];
            pole[0] = x; pole[1] = 0.0f; pole[2] = z + 3.0f;       // every middle joint bends towards the camera's side
            pole[3] = 0.0f; pole[4] = 1.0f; pole[5] = 0.0f;        // the axis of the aim, in the hand's own frame: the way the bones run
            for (UINT frame = 0; frame <= frames; ++frame) {
                timeTable[size_t(frame) * ACTORS + a] = std::fmod(0.1f * float(frame) + 0.01f * float((a * 37u) % 200u), times[KEYS - 1]);      // (looping is the caller's)
                const float phase = std::fmod(0.05f * float(frame) + 0.013f * float(a), 1.0f);
                const float u = 2.0f * phase - 1.0f, den = 1.0f + u * u;
                const float co = ((a & 1u) ? -1.0f : 1.0f) * ((1.0f - u * u) / den), si = (2.0f * u) / den;
                float *grasp = &targetTable[(size_t(frame) * ACTORS + a) * CHAINS * 3], *target = grasp + 3;
                grasp[0] = x + 0.7f * co; grasp[1] = 0.15f + 0.3f * si; grasp[2] = z + 0.7f * si;
                target[0] = grasp[0]; target[1] = grasp[1] + LIFT; target[2] = grasp[2];
            }
        }
        float keys[KEYS * JOINTS * 10];
        auto skeleton = RtSkeleton::create(context, parents, inverseBind, JOINTS);
        std::vector<rt_skeleton_layer> layout(ACTORS);
        for (uint32_t a = 0; a < ACTORS; ++a) {
            clipOf(a, keys);
            layout[a] = {skeleton->addClip(times, keys, KEYS), 0.0f, 1.0f, RT_SKELETON_NO_MASK, RT_LAYER_BLEND};
        }
        auto crowd = RtCrowd::create(skeleton, ACTORS);
        crowd->setLayout(layout.data(), 1);               // checked and uploaded once
        rt_skeleton_ik chains[CHAINS] = {};
        chains[0].kind = RT_IK_TWO_BONE;                  // group 0: the reach on joints 1-2-3
        chains[1].kind = RT_IK_AIM;                       // group 1: the hand, turned after the reach has moved it
        chains[0].joint = chains[1].joint = TIP;
        chains[0].weight = chains[1].weight = 1.0f;       // (every actor's weights: the calls bring none; poles and axes are the actors' own)
        const uint32_t groupSizes[2] = {1, 1};
        crowd->setIKChainGroups(chains, groupSizes, 2);   // checked once against the hierarchy: as ONE group the pair is refused
        void *dTimes = nullptr, *dTargets = nullptr, *dPoles = nullptr;
        ThrowIfFailed(rt_device_alloc(context->getHandle(), timeTable.size() * sizeof(float), &dTimes));
        ThrowIfFailed(rt_device_alloc(context->getHandle(), targetTable.size() * sizeof(float), &dTargets));
        ThrowIfFailed(rt_device_alloc(context->getHandle(), poles.size() * sizeof(float), &dPoles));
        ThrowIfFailed(rt_device_upload(context->getHandle(), dTimes, timeTable.data(), timeTable.size() * sizeof(float)));       // every frame's, once
        ThrowIfFailed(rt_device_upload(context->getHandle(), dTargets, targetTable.data(), targetTable.size() * sizeof(float)));
        ThrowIfFailed(rt_device_upload(context->getHandle(), dPoles, poles.data(), poles.size() * sizeof(float)));
        crowd->setBlendDevice((const float *)dTimes);     // a pose for the build to apply
        scene->attach(0, ACTORS * JOINTS, crowd, instActors.data(), instJoints.data(), locals.data());

        auto camera = std::make_shared<Math::Camera>();
        camera->SetAspectRatio(float(width) / float(height));
        camera->SetEyeAtUp({0.0f, 16.0f, 36.0f}, {0.0f, 0.0f, 0.0f}, {0, 1, 0});

        pipeline->setScene(scene);
        pipeline->setCamera(camera);
        pipeline->loadResources(3);
        pipeline->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);
        pipeline->buildAccelerationStructures();

        auto denoiser = DenoiseCompositor::create(context);
        denoiser->loadResources(3, false);
        denoiser->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);

        double update_ms = 0.0, calls_ms = 0.0, worstTip = 0.0, worstAngle = 0.0;
        std::vector<float> W(size_t(ACTORS) * JOINTS * 12);
        const auto t0 = std::chrono::steady_clock::now();
        for (UINT frame = 1; frame <= frames; ++frame) {
            const auto p0 = std::chrono::steady_clock::now();
            crowd->setBlendDevice((const float *)dTimes + size_t(frame) * ACTORS);      // one launch: every actor's clip sampled and posed
            crowd->solveIKDevice((const float *)dTargets + size_t(frame) * ACTORS * CHAINS * 3, (const float *)dPoles);      // one launch: every played pose reaches, is walked, aims its hand, and is posed again
            scene->update(context);                       // every box composed from its actor's joint, the records, the world boxes, the TLAS: on the device
            calls_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - p0).count();
            update_ms += scene->getUpdateMilliseconds();
            ThrowIfFailed(rt_crowd_read_joints(crowd->getHandle(), 0, ACTORS, W.data()));
            for (uint32_t a = 0; a < ACTORS; ++a) {
                const float *grasp = &targetTable[(size_t(frame) * ACTORS + a) * CHAINS * 3], *target = grasp + 3, *hand = &W[(size_t(a) * JOINTS + TIP) * 12];
                double tip = 0.0, axis[3], to[3];
                for (int r = 0; r < 3; ++r) {
                    const double d = double(hand[4 * r + 3]) - grasp[r];
                    tip += d * d;
                    axis[r] = double(hand[4 * r + 1]);    // the hand's y axis in the world: the aimed axis (0, 1, 0)
                    to[r] = double(target[r]) - double(hand[4 * r + 3]);
                }
                worstTip = std::fmax(worstTip, std::sqrt(tip));
                const double cx = axis[1] * to[2] - axis[2] * to[1], cy = axis[2] * to[0] - axis[0] * to[2], cz = axis[0] * to[1] - axis[1] * to[0];
                worstAngle = std::fmax(worstAngle, std::atan2(std::sqrt(cx * cx + cy * cy + cz * cz), axis[0] * to[0] + axis[1] * to[1] + axis[2] * to[2]));
            }
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
        std::printf("%s, %u boxes on %u joints of %u actors, 2 groups of 1 chain per actor solved on the device: %u frames, %.2f fps, %.3f ms per frame, posing + solve + update "
                    "%.3f ms per frame on the host, TLAS update %.3f ms per frame on the device\n",
                    pipeline->getName(), ACTORS * JOINTS, JOINTS, ACTORS, frames, frames / s, frames ? 1e3 * s / frames : 0.0, frames ? calls_ms / frames : 0.0,
                    frames ? update_ms / frames : 0.0);
        std::printf("largest tip-to-target distance %.3e of a chain %.2f long, over %u actors\n", worstTip, 2.0 * SPAN, ACTORS);
        std::printf("largest angle between the aimed axis and the direction to the target %.3e rad, over %u actors\n", worstAngle, ACTORS);

        // actor 0 against a skeleton of its own: the pose the last frame's blend gave it, then the same two groups with actor 0's values
        {
            float held[JOINTS * 10], mine[3][JOINTS * 12], theirs[3][JOINTS * 12];
            crowd->setBlendDevice((const float *)dTimes + size_t(frames) * ACTORS);
            ThrowIfFailed(rt_crowd_read_pose(crowd->getHandle(), 0, 1, held));
            crowd->solveIKDevice((const float *)dTargets + size_t(frames) * ACTORS * CHAINS * 3, (const float *)dPoles);
            ThrowIfFailed(rt_crowd_read_pose(crowd->getHandle(), 0, 1, theirs[0]));
            ThrowIfFailed(rt_crowd_read_joints(crowd->getHandle(), 0, 1, theirs[1]));
            ThrowIfFailed(rt_crowd_read_palette(crowd->getHandle(), 0, 1, theirs[2]));
            rt_skeleton_ik own[CHAINS];
            for (uint32_t k = 0; k < CHAINS; ++k) {
                own[k] = chains[k];
                for (int r = 0; r < 3; ++r) {
                    own[k].target[r] = targetTable[(size_t(frames) * ACTORS * CHAINS + k) * 3 + r];
                    own[k].pole[r] = poles[3 * k + r];
                }
            }
            skeleton->setPose(held);
            skeleton->solveIKGroups(own, groupSizes, 2);
            ThrowIfFailed(rt_skeleton_read_pose(skeleton->getHandle(), mine[0]));
            ThrowIfFailed(rt_skeleton_read_joints(skeleton->getHandle(), mine[1]));
            ThrowIfFailed(rt_skeleton_read_palette(skeleton->getHandle(), mine[2]));
            const bool same = std::memcmp(mine[0], theirs[0], sizeof(float) * JOINTS * 10) == 0 && std::memcmp(mine[1], theirs[1], sizeof mine[1]) == 0 &&
                              std::memcmp(mine[2], theirs[2], sizeof mine[2]) == 0;
            std::printf("actor 0 equals a skeleton given the same pose and solveIKGroups, byte for byte: %s\n", same ? "yes" : "no");
        }

        ThrowIfFailed(rt_device_free(context->getHandle(), dTimes));
        ThrowIfFailed(rt_device_free(context->getHandle(), dTargets));
        ThrowIfFailed(rt_device_free(context->getHandle(), dPoles));

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
