// An animated character through the reference-shaped C++ API: the tube of realtime_skinned.cpp on a chain of four joints (RtSkeleton::create),
// every vertex weighted between two neighbouring joints (RtModel::setSkin), and a baked clip of three keys (RtSkeleton::addClip).  Per frame
// the host sends ONE float: RtSkeleton::setTime samples the clip and poses the chain on the device, RtModel::setBones(skeleton) skins the tube
// from the palette where it lies, RtScene::update rebuilds the one BLAS and the TLAS over it (extensions: the reference imports with
// aiProcess_PreTransformVertices, RtModel.cpp:26, which drops bones and node animation, and never takes its generators' update path,
// Helpers/BottomLevelASGenerator.h:136-176).  With a fifth argument `host` the frame goes the way it had to go before skeletons existed:
// the host samples the keys, walks the chain, multiplies by the inverse bind matrices and uploads the palette with RtModel::setBones(float *).
// Rendered by the RealtimeRaytracingPipeline and filtered by the DenoiseCompositor; the denoised last frame is written as a PNG or PFM.
//
//   realtime_character <width> <height> <frames> <out.png|out.pfm> [host]
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

const uint32_t JOINTS = 4, KEYS = 3;

// the host's part of a frame before skeletons: the definition of include/dxr_amd.h "Posed skeletons" for a chain, in plain C++
void localOf(const float *trs, float L[12])
{
    const float x = trs[3], y = trs[4], z = trs[5], w = trs[6];
    const float R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) L[4 * r + c] = R[3 * r + c] * trs[7 + c];
        L[4 * r + 3] = trs[r];
    }
}

void compose(const float A[12], const float B[12], float C[12])
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) C[4 * r + c] = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
        C[4 * r + 3] = ((A[4 * r] * B[3] + A[4 * r + 1] * B[7]) + A[4 * r + 2] * B[11]) + A[4 * r + 3];
    }
}

void hostPalette(const float *times, const float *keys, const float *inverseBind, float t, float *palette)
{
    uint32_t i = 0;
    float a = 0.0f;
    if (t >= times[KEYS - 1]) { i = KEYS - 2; a = 1.0f; }
    else if (t > times[0]) {
        while (times[i + 1] <= t) ++i;
        a = (t - times[i]) / (times[i + 1] - times[i]);
    }
    float W[JOINTS][12];
    for (uint32_t j = 0; j < JOINTS; ++j) {
        const float *A = keys + (i * JOINTS + j) * 10;
        float B[10], trs[10], L[12];
        std::memcpy(B, A + JOINTS * 10, sizeof B);
        if (((A[3] * B[3] + A[4] * B[4]) + A[5] * B[5]) + A[6] * B[6] < 0.0f)
            for (int c = 3; c < 7; ++c) B[c] = -B[c];
        for (int c = 0; c < 10; ++c) trs[c] = A[c] + a * (B[c] - A[c]);
        const float n = ((trs[3] * trs[3] + trs[4] * trs[4]) + trs[5] * trs[5]) + trs[6] * trs[6];
        for (int c = 3; c < 7; ++c) trs[c] = n > 0.0f && std::isfinite(n) ? trs[c] * (1.0f / std::sqrt(n)) : (c == 6 ? 1.0f : 0.0f);
        localOf(trs, L);
        if (j == 0) std::memcpy(W[j], L, sizeof L);
        else compose(W[j - 1], L, W[j]);                 // (a chain: joint j - 1 is the parent)
        compose(W[j], inverseBind + 12 * j, palette + 12 * j);
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
    const bool onHost = argc > 5 && std::string(argv[5]) == "host";
    try {
        // the tube: RINGS rings of SEGS vertices about the y axis, y = -1.5 .. 1.5, radius 0.35.  Joint j sits at y = -1.5 + 0.75 j; a vertex
        // follows the two joints about it, half and half where the upper one sits, with a smooth crossover
        const uint32_t RINGS = 32, SEGS = 48;
        const float SPAN = 0.75f;
        std::vector<rt_vertex> verts;
        std::vector<uint32_t> indices, bones;
        std::vector<float> weights;
        for (uint32_t r = 0; r < RINGS; ++r)
            for (uint32_t s = 0; s < SEGS; ++s) {
                const float a = 6.2831853f * float(s) / float(SEGS), y = -1.5f + 3.0f * float(r) / float(RINGS - 1);
                verts.push_back({{0.35f * std::cos(a), y, 0.35f * std::sin(a)}, {std::cos(a), 0.0f, std::sin(a)}});
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
        // the clip: the bind pose, every joint above the root turned about z, then about x the other way
        const float times[KEYS] = {0.0f, 1.0f, 2.0f};
        const float turns[KEYS][4] = {{0, 0, 0, 1}, {0, 0, std::sin(0.3f), std::cos(0.3f)}, {std::sin(-0.25f), 0, 0, std::cos(-0.25f)}};
        float keys[KEYS * JOINTS * 10];
        for (uint32_t k = 0; k < KEYS; ++k)
            for (uint32_t j = 0; j < JOINTS; ++j) {
                float *trs = keys + (k * JOINTS + j) * 10;
                trs[0] = 0.0f; trs[1] = j == 0 ? -1.5f : SPAN; trs[2] = 0.0f;
                for (int c = 0; c < 4; ++c) trs[3 + c] = j == 0 ? turns[0][c] : turns[k][c];
                trs[7] = trs[8] = trs[9] = 1.0f;
            }

        auto context = RtContext::create(0);
        auto scene = RtScene::create();
        auto model = RtModel::create(context, verts.data(), n, indices.data(), tris);
        model->setSkin(bones.data(), weights.data(), 2, JOINTS);  // the vertices as created are the rest pose
        auto skeleton = RtSkeleton::create(context, parents, inverseBind, JOINTS);
        const uint32_t clip = skeleton->addClip(times, keys, KEYS);
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
            const float t = std::fmod(0.1f * float(frame), times[KEYS - 1]);      // (looping is the caller's)
            const auto p0 = std::chrono::steady_clock::now();
            if (onHost) {
                float palette[JOINTS * 12];
                hostPalette(times, keys, inverseBind, t, palette);
                model->setBones(palette);
            } else {
                skeleton->setTime(clip, t);               // one float: the clip is sampled and the chain posed on the device
                model->setBones(skeleton);                // the palette is used where it lies
            }
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
        std::printf("%s, %u skinned vertices, %u triangles, %u joints, %u keys, posed on the %s: %u frames, %.2f fps, %.3f ms per frame, posing calls "
                    "%.3f ms per frame on the host, BLAS + TLAS update %.3f ms per frame on the device\n",
                    pipeline->getName(), n, tris, JOINTS, KEYS, onHost ? "host" : "device", frames, frames / s, frames ? 1e3 * s / frames : 0.0,
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
