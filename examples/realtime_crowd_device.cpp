// The crowd of realtime_crowd.cpp -- 196 small machines, every one an ACTOR of one RtCrowd on one RtSkeleton -- driven from DEVICE memory.
// Every actor has a LAYOUT of two layers, set once with RtCrowd::setLayout: its walk, and over it a second clip (the same rig, waving)
// that the frames cross-fade to.  The times and weights of ALL frames are made up front and uploaded ONCE (rt_device_alloc,
// rt_device_upload): a table of frames x actors x 2 floats each, as a simulation that keeps its clocks on the device would hold them.  Per
// frame the host makes ONE RtCrowd::setBlendDevice(table + frame * actors * 2) and ONE RtScene::update: one launch finds every layer's
// segment, blends and poses all 196 hierarchies, and nothing is uploaded inside the loop (extensions: the reference states a transform only
// in addModel, RtScene.h:30, fills the Transform member of the instance descriptor once, Helpers/TopLevelASGenerator.cpp:344-362, and never
// takes its generators' update path, Helpers/TopLevelASGenerator.h:144-163).  With `host` the same frames are driven through
// RtCrowd::setBlend, the layers packed on the host and uploaded every frame; the image is the same image.
//
//   realtime_crowd_device <width> <height> <frames> <out.png|out.pfm> [host]
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
        std::fprintf(stderr, "usage: %s width height frames out.png|out.pfm [host]\n", argv[0]);
        return 2;
    }
    const UINT width = std::atoi(argv[1]), height = std::atoi(argv[2]), frames = std::atoi(argv[3]);
    const bool onHost = argc > 5 && std::strcmp(argv[5], "host") == 0;
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
        // ... and the motion the walk is cross-faded to: the hands wave, the arm leans back
        const float waves[KEYS][JOINTS][4] = {
            {{0, 0, 0, 1}, {-0.25f, 0, 0, 1}, {0, 0, 0.5f, 1}, {0, 0, -0.5f, 1}, {0, 0, 0, 1}},
            {{0, 0, 0, 1}, {-0.25f, 0, 0.125f, 1}, {0, 0.25f, 1, 1}, {0, -0.25f, -1, 1}, {0, 0.25f, 0, 1}},
            {{0, 0, 0, 1}, {-0.25f, 0, -0.125f, 1}, {0, -0.25f, 0.25f, 1}, {0, 0.25f, -0.25f, 1}, {0, -0.25f, 0, 1}}};
        // a clip of actor a: one of the two motions with the base on the actor's square
        auto clipOf = [&](uint32_t a, const float (*turns)[JOINTS][4], float *keys) {
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

        // the table of every frame: actor a walks at its own time (the clip loops, and the actors start spread over it), waves at another, and
        // fades from the one to the other and back, each actor at its own phase
        const uint32_t LAYERS = 2, perFrame = ACTORS * LAYERS;
        std::vector<float> timeTable(size_t(frames + 1) * perFrame), weightTable(size_t(frames + 1) * perFrame);
        for (UINT frame = 0; frame <= frames; ++frame)
            for (uint32_t a = 0; a < ACTORS; ++a) {
                float *t = &timeTable[size_t(frame) * perFrame + a * LAYERS], *w = &weightTable[size_t(frame) * perFrame + a * LAYERS];
                t[0] = std::fmod(0.125f * float(frame) + 0.01f * float((a * 37u) % 200u), times[KEYS - 1]);      // (looping is the caller's)
                t[1] = std::fmod(0.25f * float(frame) + 0.02f * float((a * 11u) % 100u), times[KEYS - 1]);
                w[0] = 1.0f;                                  // (the base layer's weight is not read)
                w[1] = 0.5f - 0.5f * std::cos(0.5f * float(frame) + 0.1f * float(a % SIDE));
            }
        float keys[KEYS * JOINTS * 10];
        auto skeleton = RtSkeleton::create(context, parents, inverseBind, JOINTS);
        std::vector<rt_skeleton_layer> layout(perFrame);
        for (uint32_t a = 0; a < ACTORS; ++a) {
            clipOf(a, turns, keys);
            layout[a * LAYERS] = {skeleton->addClip(times, keys, KEYS), 0.0f, 1.0f, RT_SKELETON_NO_MASK, RT_LAYER_BLEND};
            clipOf(a, waves, keys);
            layout[a * LAYERS + 1] = {skeleton->addClip(times, keys, KEYS), 0.0f, 0.0f, RT_SKELETON_NO_MASK, RT_LAYER_BLEND};
        }
        auto crowd = RtCrowd::create(skeleton, ACTORS);
        // the layers of a frame as RtCrowd::setBlend takes them: what the `host` path packs and uploads every frame
        std::vector<rt_skeleton_layer> layers(layout);
        auto layersOf = [&](UINT frame) {
            for (uint32_t e = 0; e < perFrame; ++e) {
                layers[e].time = timeTable[size_t(frame) * perFrame + e];
                layers[e].weight = weightTable[size_t(frame) * perFrame + e];
            }
        };
        void *dTimes = nullptr, *dWeights = nullptr;
        if (!onHost) {
            crowd->setLayout(layout.data(), LAYERS);          // checked and uploaded once
            ThrowIfFailed(rt_device_alloc(context->getHandle(), timeTable.size() * sizeof(float), &dTimes));
            ThrowIfFailed(rt_device_alloc(context->getHandle(), weightTable.size() * sizeof(float), &dWeights));
            ThrowIfFailed(rt_device_upload(context->getHandle(), dTimes, timeTable.data(), timeTable.size() * sizeof(float)));       // every frame's, once
            ThrowIfFailed(rt_device_upload(context->getHandle(), dWeights, weightTable.data(), weightTable.size() * sizeof(float)));
            crowd->setBlendDevice((const float *)dTimes, (const float *)dWeights);      // a pose for the build to apply
        } else {
            layersOf(0);
            crowd->setBlend(layers.data(), LAYERS);
        }
        scene->attach(0, ACTORS * BOXES, crowd, instActors.data(), instJoints.data(), locals.data());

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
            const auto p0 = std::chrono::steady_clock::now();
            if (!onHost)      // one launch: every layer's segment found, every actor blended and posed on the device; nothing crosses
                crowd->setBlendDevice((const float *)dTimes + size_t(frame) * perFrame, (const float *)dWeights + size_t(frame) * perFrame);
            else {
                layersOf(frame);
                crowd->setBlend(layers.data(), LAYERS);
            }
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
        std::printf("%s, %u boxes on %u joints of %u actors, posed from %s: %u frames, %.2f fps, %.3f ms per frame, posing + update %.3f ms per frame on the host, "
                    "TLAS update %.3f ms per frame on the device, transforms checksum %08x\n",
                    pipeline->getName(), ACTORS * BOXES, JOINTS, ACTORS, onHost ? "host layers" : "device times", frames, frames / s, frames ? 1e3 * s / frames : 0.0,
                    frames ? calls_ms / frames : 0.0, frames ? update_ms / frames : 0.0, sum);

        if (dTimes) ThrowIfFailed(rt_device_free(context->getHandle(), dTimes));
        if (dWeights) ThrowIfFailed(rt_device_free(context->getHandle(), dWeights));

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
