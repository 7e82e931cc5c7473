// Clips blended and layered on the device, through the reference-shaped C++ API: the tube and the four-joint chain of realtime_character.cpp
// with three clips (RtSkeleton::addClip) -- the chain bends left, it bends right, and it twists about its own axis -- and a mask over the upper
// two joints (RtSkeleton::addMask).  Per frame the host sends three layers of five words each: RtSkeleton::setBlend cross-fades the two bends,
// adds the twist to the masked joints (RT_LAYER_ADDITIVE) and poses the chain on the device, RtModel::setBones(skeleton) skins the tube from
// the palette where it lies, RtScene::update rebuilds the one BLAS and the TLAS over it (extensions: the reference imports with
// aiProcess_PreTransformVertices, RtModel.cpp:26, which drops bones and node animation, and never takes its generators' update path,
// Helpers/BottomLevelASGenerator.h:136-176).  With a fifth argument `host` the frame goes the way it had to go before blends existed: every
// clip is sampled on the device and read back (rt_skeleton_set_time + rt_skeleton_read_pose), the host blends by the definition of
// include/dxr_amd.h "Posed skeletons" and uploads the result (RtSkeleton::setPose).
// Rendered by the RealtimeRaytracingPipeline and filtered by the DenoiseCompositor; the denoised last frame is written as a PNG or PFM.
//
//   realtime_blend <width> <height> <frames> <out.png|out.pfm> [host]
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

const uint32_t JOINTS = 4, KEYS = 2, CLIPS = 3, LAYERS = 3;

// the host's part of a frame before blends: the definition of include/dxr_amd.h "Posed skeletons", blending, in plain C++
void unitOrIdentity(float q[4])
{
    const float n = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    for (int c = 0; c < 4; ++c) q[c] = n > 0.0f && std::isfinite(n) ? q[c] * (1.0f / std::sqrt(n)) : (c == 3 ? 1.0f : 0.0f);
}

void hamilton(const float p[4], const float q[4], float r[4])
{
    r[0] = ((p[3] * q[0] + p[0] * q[3]) + p[1] * q[2]) - p[2] * q[1];
    r[1] = ((p[3] * q[1] - p[0] * q[2]) + p[1] * q[3]) + p[2] * q[0];
    r[2] = ((p[3] * q[2] + p[0] * q[1]) - p[1] * q[0]) + p[2] * q[3];
    r[3] = ((p[3] * q[3] - p[0] * q[0]) - p[1] * q[1]) - p[2] * q[2];
}

void hostBlend(float *P, const float *S, float w)
{
    float s[10];
    std::memcpy(s, S, sizeof s);
    if (((P[3] * s[3] + P[4] * s[4]) + P[5] * s[5]) + P[6] * s[6] < 0.0f)
        for (int c = 3; c < 7; ++c) s[c] = -s[c];
    for (int c = 0; c < 10; ++c) P[c] = P[c] + w * (s[c] - P[c]);
    unitOrIdentity(P + 3);
}

void hostAdd(float *P, const float *S, const float *R, float w)
{
    for (int c = 0; c < 3; ++c) {
        P[c] = P[c] + w * (S[c] - R[c]);
        P[7 + c] = P[7 + c] + w * (S[7 + c] - R[7 + c]);
    }
    const float conj[4] = {-R[3], -R[4], -R[5], R[6]};
    float D[4], E[4], q[4];
    hamilton(conj, S + 3, D);
    if (D[3] < 0.0f)
        for (int c = 0; c < 4; ++c) D[c] = -D[c];
    for (int c = 0; c < 3; ++c) E[c] = w * D[c];
    E[3] = 1.0f + w * (D[3] - 1.0f);
    unitOrIdentity(E);
    hamilton(P + 3, E, q);
    unitOrIdentity(q);
    std::memcpy(P + 3, q, sizeof q);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s width height frames out.png|out.pfm [host]\n", argv[0]);
        return 2;
    }
    const UINT width = std::atoi(argv[1]), height = std::atoi(argv[2]), frames = std::atoi(argv[3]);
    const bool onHost = argc > 5 && std::string(argv[5]) == "host";
    try {
        // the tube of realtime_character.cpp: RINGS rings of SEGS vertices about the y axis, y = -1.5 .. 1.5, radius 0.35.  Joint j sits at
        // y = -1.5 + 0.75 j; a vertex follows the two joints about it, with a smooth crossover
        const uint32_t RINGS = 32, SEGS = 48;
        const float SPAN = 0.75f;
        std::vector<rt_vertex> verts;
        std::vector<uint32_t> indices, bones;
        std::vector<float> weights;
        for (uint32_t r = 0; r < RINGS; ++r)
            for (uint32_t s = 0; s < SEGS; ++s) {
                const float a = 6.2831853f * float(s) / float(SEGS), y = -1.5f + 3.0f * float(r) / float(RINGS - 1);
                // (an ellipse, not a circle: a twist about the tube's axis shows)
                verts.push_back({{0.45f * std::cos(a), y, 0.25f * std::sin(a)}, {std::cos(a), 0.0f, std::sin(a)}});
                const float c = (y + 1.5f) / SPAN - 0.5f;
                const uint32_t k0 = c <= 0.0f ? 0u : c >= float(JOINTS - 1) ? JOINTS - 1 : uint32_t(c), k1 = k0 + 1 < JOINTS ? k0 + 1 : k0;
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

        // the chain: joint 0 a root at the tube's lower end, every other joint SPAN above its parent; the inverse bind matrices undo that
        const int32_t parents[JOINTS] = {-1, 0, 1, 2};
        float inverseBind[JOINTS * 12] = {};
        for (uint32_t j = 0; j < JOINTS; ++j) {
            inverseBind[12 * j] = inverseBind[12 * j + 5] = inverseBind[12 * j + 10] = 1.0f;
            inverseBind[12 * j + 7] = 1.5f - SPAN * float(j);
        }
        // the clips, two keys each, from the bind pose to: every joint above the root turned about z one way (bend left), the other way
        // (bend right), about y (the twist: an additive clip, its first key the reference pose)
        const float times[KEYS] = {0.0f, 1.0f};
        const float turns[CLIPS][4] = {{0, 0, std::sin(0.3f), std::cos(0.3f)}, {0, 0, std::sin(-0.3f), std::cos(-0.3f)}, {0, std::sin(0.5f), 0, std::cos(0.5f)}};
        float keys[CLIPS][KEYS * JOINTS * 10];
        for (uint32_t c = 0; c < CLIPS; ++c)
            for (uint32_t k = 0; k < KEYS; ++k)
                for (uint32_t j = 0; j < JOINTS; ++j) {
                    float *trs = keys[c] + (k * JOINTS + j) * 10;
                    trs[0] = 0.0f; trs[1] = j == 0 ? -1.5f : SPAN; trs[2] = 0.0f;
                    trs[3] = trs[4] = trs[5] = 0.0f; trs[6] = 1.0f;
                    if (j > 0 && k == 1)
                        for (int q = 0; q < 4; ++q) trs[3 + q] = turns[c][q];
                    trs[7] = trs[8] = trs[9] = 1.0f;
                }
        const float upper[JOINTS] = {0.0f, 0.0f, 1.0f, 1.0f};     // the twist reaches the upper two joints only

        auto context = RtContext::create(0);
        auto scene = RtScene::create();
        auto model = RtModel::create(context, verts.data(), n, indices.data(), tris);
        model->setSkin(bones.data(), weights.data(), 2, JOINTS);  // the vertices as created are the rest pose
        auto skeleton = RtSkeleton::create(context, parents, inverseBind, JOINTS);
        uint32_t clip[CLIPS];
        for (uint32_t c = 0; c < CLIPS; ++c) clip[c] = skeleton->addClip(times, keys[c], KEYS);
        const uint32_t mask = skeleton->addMask(upper);
        auto pipeline = RealtimeRaytracingPipeline::create(context);
        scene->addModel(model, Matrix::translation(0.0f, 0.0f, 0.0f));
        RaytracingPipeline::Material material{};
        material.params.albedo = {0.3f, 0.6f, 0.85f, 1.0f};
        material.params.specular = {0.58f, 0.58f, 0.58f, 1.0f};
        material.params.roughness = 0.5f;
        material.params.reflectivity = 0.7f;
        material.params.type = 0;
        pipeline->addMaterial(material);

        auto camera = std::make_shared<Math::Camera>();
        camera->SetAspectRatio(float(width) / float(height));
        camera->SetEyeAtUp({0.0f, 0.5f, 5.0f}, {0.0f, 0.0f, 0.0f}, {0, 1, 0});

        pipeline->setScene(scene);
        pipeline->setCamera(camera);
        pipeline->loadResources(3);
        pipeline->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);
        pipeline->buildAccelerationStructures();

        auto denoiser = DenoiseCompositor::create(context);
        denoiser->loadResources(3, false);
        denoiser->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);

        double update_ms = 0.0, pose_ms = 0.0;
        const auto t0 = std::chrono::steady_clock::now();
        for (UINT frame = 1; frame <= frames; ++frame) {
            // the caller moves the times and the weights: a cross-fade from left to right and back, the twist coming and going
            const float t = 0.5f + 0.5f * std::sin(0.35f * float(frame));
            const float fade = 0.5f - 0.5f * std::cos(0.2f * float(frame)), twist = 0.5f + 0.5f * std::sin(0.15f * float(frame));
            const rt_skeleton_layer layers[LAYERS] = {{clip[0], t, 1.0f, RT_SKELETON_NO_MASK, RT_LAYER_BLEND},
                                                      {clip[1], t, fade, RT_SKELETON_NO_MASK, RT_LAYER_BLEND},
                                                      {clip[2], 1.0f, twist, mask, RT_LAYER_ADDITIVE}};
            const auto p0 = std::chrono::steady_clock::now();
            if (onHost) {
                float S[CLIPS][JOINTS * 10], R[JOINTS * 10];
                for (uint32_t c = 0; c < CLIPS; ++c) {
                    skeleton->setTime(clip[c], layers[c].time);
                    ThrowIfFailed(rt_skeleton_read_pose(skeleton->getHandle(), S[c]));
                }
                skeleton->setTime(clip[2], -INFINITY);     // the reference pose of the additive clip
                ThrowIfFailed(rt_skeleton_read_pose(skeleton->getHandle(), R));
                for (uint32_t j = 0; j < JOINTS; ++j) {
                    hostBlend(S[0] + 10 * j, S[1] + 10 * j, layers[1].weight);
                    hostAdd(S[0] + 10 * j, S[2] + 10 * j, R + 10 * j, layers[2].weight * upper[j]);
                }
                skeleton->setPose(S[0]);
            } else {
                skeleton->setBlend(layers, LAYERS);       // sixty bytes: the clips are sampled, blended and the chain posed on the device
            }
            model->setBones(skeleton);                    // the palette is used where it lies
            pose_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - p0).count();
            scene->update(context);                       // the BLAS rebuilt over the skinned vertices, the instance record, the TLAS: on the device
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
        std::printf("%s, %u skinned vertices, %u triangles, %u joints, %u clips, %u layers, blended on the %s: %u frames, %.2f fps, %.3f ms per frame, "
                    "posing calls %.3f ms per frame on the host, BLAS + TLAS update %.3f ms per frame on the device\n",
                    pipeline->getName(), n, tris, JOINTS, CLIPS, LAYERS, onHost ? "host" : "device", frames, frames / s, frames ? 1e3 * s / frames : 0.0,
                    frames ? pose_ms / frames : 0.0, frames ? update_ms / frames : 0.0);

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
