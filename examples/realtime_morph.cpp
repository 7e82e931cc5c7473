// A morphed mesh through the reference-shaped C++ API: a grid of 64 x 64 vertices with one sparse morph target, a bump over the vertices
// within 1.2 of the middle (RtModel::setMorphTargets), weighted by a sine every frame through RtModel::setMorphWeights + RtScene::update
// (extensions: the reference reads only mVertices / mNormals of an imported mesh, RtModel.cpp:26, :38-45, never its blend shapes; and it never
// takes its generators' update path, Helpers/BottomLevelASGenerator.h:136-176).  Per frame the host sends one float; the vertices are written
// on the device from the base, the normals recomputed there, the one BLAS rebuilt in place and the TLAS over it.  Rendered by the
// RealtimeRaytracingPipeline and filtered by the DenoiseCompositor as in realtime_skinned.cpp; the denoised last frame is written as a PNG or
// PFM.
//
//   realtime_morph <width> <height> <frames> <out.png|out.pfm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "DenoiseCompositor.h"
#include "RealtimeRaytracingPipeline.h"

using namespace DXRFramework;

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s width height frames out.png|out.pfm\n", argv[0]);
        return 2;
    }
    const UINT width = std::atoi(argv[1]), height = std::atoi(argv[2]), frames = std::atoi(argv[3]);
    try {
        // the grid: N x N vertices over x, z = -2 .. 2 at y = 0; the target lifts the vertices within 1.2 of the middle by a smooth bump of
        // height 1 and names no other vertex
        const uint32_t N = 64;
        std::vector<rt_vertex> verts;
        std::vector<uint32_t> indices, named;
        std::vector<float> deltas;
        for (uint32_t j = 0; j < N; ++j)
            for (uint32_t i = 0; i < N; ++i) {
                const float x = -2.0f + 4.0f * float(i) / float(N - 1), z = -2.0f + 4.0f * float(j) / float(N - 1);
                verts.push_back({{x, 0.0f, z}, {0.0f, 1.0f, 0.0f}});
                const float r = std::sqrt(x * x + z * z) / 1.2f;
                if (r < 1.0f) {
                    const float h = (1.0f - r * r) * (1.0f - r * r);
                    named.push_back(j * N + i);                   // (ascending: a target names its vertices in order, each once)
                    deltas.insert(deltas.end(), {0.0f, h, 0.0f});
                }
            }
        for (uint32_t j = 0; j + 1 < N; ++j)
            for (uint32_t i = 0; i + 1 < N; ++i) {
                const uint32_t a = j * N + i, b = a + 1, c = a + N, d = c + 1;
                indices.insert(indices.end(), {a, c, b, b, c, d});
            }
        const uint32_t n = (uint32_t)verts.size(), tris = (uint32_t)(indices.size() / 3);
        const uint32_t offsets[2] = {0, (uint32_t)named.size()};

        auto context = RtContext::create(0);
        auto scene = RtScene::create();
        auto model = RtModel::create(context, verts.data(), n, indices.data(), tris);
        model->setMorphTargets(1, offsets, named.data(), deltas.data());        // the vertices as created are the base
        auto pipeline = RealtimeRaytracingPipeline::create(context);
        scene->addModel(model, Matrix::translation(0.0f, 0.0f, 0.0f));
        RaytracingPipeline::Material material{};
        material.params.albedo = {0.85f, 0.5f, 0.3f, 1.0f};
        material.params.specular = {0.58f, 0.58f, 0.58f, 1.0f};
        material.params.roughness = 0.5f;
        material.params.reflectivity = 0.7f;
        material.params.type = 0;
        pipeline->addMaterial(material);

        auto camera = std::make_shared<Math::Camera>();
        camera->SetAspectRatio(float(width) / float(height));
        camera->SetEyeAtUp({0.0f, 2.5f, 5.0f}, {0.0f, 0.0f, 0.0f}, {0, 1, 0});

        pipeline->setScene(scene);
        pipeline->setCamera(camera);
        pipeline->loadResources(3);
        pipeline->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);
        pipeline->buildAccelerationStructures();

        auto denoiser = DenoiseCompositor::create(context);
        denoiser->loadResources(3, false);
        denoiser->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);

        double update_ms = 0.0;
        const auto t0 = std::chrono::steady_clock::now();
        for (UINT frame = 1; frame <= frames; ++frame) {
            const float weight = std::sin(0.5f * float(frame));  // the bump rises, sinks below the grid and comes back
            model->setMorphWeights(&weight);
            model->recomputeNormals();                // (the target carries positions only)
            scene->update(context);                   // the BLAS rebuilt over the morphed vertices, the instance record, the TLAS: on the device
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
        std::printf("%s, %u morphed vertices, %u triangles, 1 target of %u entries: %u frames, %.2f fps, BLAS + TLAS update %.3f ms per frame on the device\n",
                    pipeline->getName(), n, tris, (unsigned)named.size(), frames, frames / s, frames ? update_ms / frames : 0.0);

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
