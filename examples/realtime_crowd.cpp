// A crowd of small machines through the reference-shaped C++ API: the rig and the six boxes of realtime_machines.cpp, 196 times -- every
// machine an ACTOR of one RtCrowd on one RtSkeleton, standing on its own square of a 14 x 14 grid (a clip per square: the same motion with
// the base placed there) and running at its own clip time.  Per frame the host makes ONE RtCrowd::setTimes and ONE RtScene::update: a clip
// id and a time per actor cross to the device in one upload, one launch samples and poses all 196 hierarchies, and the update composes the
// 1176 boxes from their actors' joints and rewrites the records, the world boxes and the TLAS (extensions: the reference states a transform
// only in addModel, RtScene.h:30, fills the Transform member of the instance descriptor once, Helpers/TopLevelASGenerator.cpp:344-362, and
// never takes its generators' update path, Helpers/TopLevelASGenerator.h:144-163).  With `skeletons` the same frame is driven the way there
// was before: a skeleton per machine, 196 RtSkeleton::setTime calls a frame; the image is the same image.
//
//   realtime_crowd <width> <height> <frames> <out.png|out.pfm> [skeletons]
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

const uint32_t JOINTS = 5, KEYS = 3, BOXES = 6, SIDE = 14, ACTORS = SIDE * SIDE;

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
        std::fprintf(stderr, "usage: %s width height frames out.png|out.pfm [skeletons]\n", argv[0]);
        return 2;
    }
    const UINT width = std::atoi(argv[1]), height = std::atoi(argv[2]), frames = std::atoi(argv[3]);
    const bool asSkeletons = argc > 5 && std::strcmp(argv[5], "skeletons") == 0;
    try {
        std::vector<rt_vertex> verts;
        std::vector<uint32_t> indices;
        cube(verts, indices);

        // the hierarchy: a base (0), on it an arm (1) and a counterweight (4), on the arm two hands (2, 3): three levels
        const int32_t parents[JOINTS] = {-1, 0, 1, 1, 0};
        float inverseBind[JOINTS * 12] = {};
        for (uint32_t j = 0; j < JOINTS; ++j) inverseBind[12 * j] = inverseBind[12 * j + 5] = inverseBind[12 * j + 10] = 1.0f;
        const float times[KEYS] = {0.0f, 1.0f, 2.0f};
        const float offsets[JOINTS][3] = {{0.0f, -1.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {1.25f, 0.75f, 0.0f}, {-1.25f, 0.75f, 0.0f}, {0.0f, 0.25f, -1.5f}};
        const float turns[KEYS][JOINTS][4] = {
            {{0, 0, 0, 1}, {0, 0, 0, 1}, {0, 0, 0, 1}, {0, 0, 0, 1}, {0, 0, 0, 1}},
            {{0, 0.5f, 0, 1}, {0, 0, 0.25f, 1}, {0.5f, 0, 0, 1}, {0, 0, -0.5f, 1}, {0, -0.25f, 0, 1}},
            {{0, -0.25f, 0, 1}, {0.25f, 0, -0.25f, 1}, {0, 0.5f, 0.5f, 1}, {-0.5f, 0, 0, 1}, {0.125f, 0.5f, 0, 1}}};
        // the clip of actor a: that motion with the base on the actor's square
        auto clipOf = [&](uint32_t a, float *keys) {
            for (uint32_t k = 0; k < KEYS; ++k)
                for (uint32_t j = 0; j < JOINTS; ++j) {
                    float *trs = keys + (k * JOINTS + j) * 10;
                    for (int c = 0; c < 3; ++c) trs[c] = offsets[j][c];
                    if (j == 0) {
                        trs[0] += 6.0f * (float(a % SIDE) - 0.5f * float(SIDE - 1));
                        trs[2] += 6.0f * (float(a / SIDE) - 0.5f * float(SIDE - 1));
                    }
                    for (int c = 0; c < 4; ++c) trs[3 + c] = turns[k][j][c];
                    trs[7] = trs[8] = trs[9] = 1.0f;
                }
        };
        // box b of an actor follows joint joints[b]; its local matrix shapes the unit cube into the part and places it on the joint
        const uint32_t joints[BOXES] = {0, 1, 2, 3, 4, 2};
        const float shape[BOXES][6] = {{2.5f, 0.25f, 2.5f, 0, 0, 0},   {0.5f, 1.5f, 0.5f, 0, 0, 0},       {0.75f, 0.25f, 0.25f, 0, 0, 0},
                                       {0.75f, 0.25f, 0.25f, 0, 0, 0}, {0.75f, 0.75f, 0.75f, 0, 0, 0},    {0.25f, 0.25f, 0.5f, 0.5f, 0, 0.25f}};
        std::vector<uint32_t> instActors(ACTORS * BOXES), instJoints(ACTORS * BOXES);
        std::vector<float> locals(ACTORS * BOXES * 12, 0.0f);
        for (uint32_t a = 0; a < ACTORS; ++a)
            for (uint32_t b = 0; b < BOXES; ++b) {
                const uint32_t i = a * BOXES + b;
                instActors[i] = a;
                instJoints[i] = joints[b];
                for (int r = 0; r < 3; ++r) {
                    locals[12 * i + 5 * r] = shape[b][r];
                    locals[12 * i + 4 * r + 3] = shape[b][3 + r];
                }
            }

        auto context = RtContext::create(0);
        auto scene = RtScene::create();
        auto model = RtModel::create(context, verts.data(), (uint32_t)verts.size(), indices.data(), (uint32_t)(indices.size() / 3));
        auto pipeline = RealtimeRaytracingPipeline::create(context);
        for (uint32_t i = 0; i < ACTORS * BOXES; ++i) {
            scene->addModel(model, Matrix::translation(0.0f, 0.0f, 0.0f));      // (where the first pose puts it is decided below)
            RaytracingPipeline::Material material{};
            material.params.albedo = {0.25f + 0.12f * float(i % BOXES), 0.6f, 0.85f - 0.1f * float(i % BOXES), 1.0f};
            material.params.specular = {0.58f, 0.58f, 0.58f, 1.0f};
            material.params.roughness = 0.5f;
            material.params.reflectivity = 0.7f;
            material.params.type = 0;
            pipeline->addMaterial(material);
        }

        // every actor at its own time: the clip loops, and the actors start spread over it
        std::vector<uint32_t> clips(ACTORS);
        std::vector<float> now(ACTORS);
        auto timesOf = [&](UINT frame) {
            for (uint32_t a = 0; a < ACTORS; ++a) now[a] = std::fmod(0.125f * float(frame) + 0.01f * float((a * 37u) % 200u), times[KEYS - 1]);      // (looping is the caller's)
        };
        float keys[KEYS * JOINTS * 10];
        RtSkeleton::SharedPtr skeleton;
        RtCrowd::SharedPtr crowd;
        std::vector<RtSkeleton::SharedPtr> singles;
        timesOf(0);
        if (!asSkeletons) {
            skeleton = RtSkeleton::create(context, parents, inverseBind, JOINTS);
            for (uint32_t a = 0; a < ACTORS; ++a) {
                clipOf(a, keys);
                clips[a] = skeleton->addClip(times, keys, KEYS);
            }
            crowd = RtCrowd::create(skeleton, ACTORS);
            crowd->setTimes(clips.data(), now.data());        // a pose for the build to apply
            scene->attach(0, ACTORS * BOXES, crowd, instActors.data(), instJoints.data(), locals.data());
        } else
            for (uint32_t a = 0; a < ACTORS; ++a) {
                singles.push_back(RtSkeleton::create(context, parents, inverseBind, JOINTS));
                clipOf(a, keys);
                clips[a] = singles[a]->addClip(times, keys, KEYS);
                singles[a]->setTime(clips[a], now[a]);
                scene->attach(a * BOXES, BOXES, singles[a], joints, &locals[12 * a * BOXES]);
            }

        auto camera = std::make_shared<Math::Camera>();
        camera->SetAspectRatio(float(width) / float(height));
        camera->SetEyeAtUp({0.0f, 30.0f, 70.0f}, {0.0f, 0.0f, 0.0f}, {0, 1, 0});

        pipeline->setScene(scene);
        pipeline->setCamera(camera);
        pipeline->loadResources(3);
        pipeline->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);
        pipeline->buildAccelerationStructures();

        auto denoiser = DenoiseCompositor::create(context);
        denoiser->loadResources(3, false);
        denoiser->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);

        double update_ms = 0.0, calls_ms = 0.0;
        const auto t0 = std::chrono::steady_clock::now();
        for (UINT frame = 1; frame <= frames; ++frame) {
            timesOf(frame);
            const auto p0 = std::chrono::steady_clock::now();
            if (crowd) crowd->setTimes(clips.data(), now.data());     // one upload, one launch: every actor sampled and posed on the device
            else
                for (uint32_t a = 0; a < ACTORS; ++a) singles[a]->setTime(clips[a], now[a]);
            scene->update(context);                       // every box composed from its actor's joint, the records, the world boxes, the TLAS: on the device
            calls_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - p0).count();
            update_ms += scene->getUpdateMilliseconds();
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
        std::vector<float> held(ACTORS * BOXES * 12);
        scene->getTransforms(0, ACTORS * BOXES, held.data());
        uint32_t sum = 2166136261u;                      // FNV-1a over the bytes of the transforms the scene holds
        for (size_t k = 0; k < held.size() * sizeof(float); ++k) sum = (sum ^ reinterpret_cast<const unsigned char *>(held.data())[k]) * 16777619u;
        std::printf("%s, %u boxes on %u joints of %u actors, posed as %s: %u frames, %.2f fps, %.3f ms per frame, posing + update %.3f ms per frame on the host, "
                    "TLAS update %.3f ms per frame on the device, transforms checksum %08x\n",
                    pipeline->getName(), ACTORS * BOXES, JOINTS, ACTORS, crowd ? "a crowd" : "skeletons", frames, frames / s, frames ? 1e3 * s / frames : 0.0,
                    frames ? calls_ms / frames : 0.0, frames ? update_ms / frames : 0.0, sum);

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
