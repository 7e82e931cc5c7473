// A deforming mesh through the reference-shaped C++ API: one model whose vertices are waved every frame with RtModel::setPositions +
// RtModel::recomputeNormals + RtScene::update (extensions: the reference's RtModel never changes and never takes its generators' update
// path, Helpers/BottomLevelASGenerator.h:136-176), rendered by the RealtimeRaytracingPipeline and filtered by the DenoiseCompositor as in
// realtime_animated.cpp.  No model and no scene is thrown away: every update rebuilds the one BLAS in place, by the build's own steps, and
// the TLAS over it; the denoised last frame is written as a PNG or PFM.
//
//   realtime_deform <model.obj> <width> <height> <frames> <out.png|out.pfm>
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
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s model.obj width height frames out.png|out.pfm\n", argv[0]);
        return 2;
    }
    const UINT width = std::atoi(argv[2]), height = std::atoi(argv[3]), frames = std::atoi(argv[4]);
    try {
        auto context = RtContext::create(0);
        auto scene = RtScene::create();
        auto model = RtModel::create(context, argv[1]);
        auto pipeline = RealtimeRaytracingPipeline::create(context);
        scene->addModel(model, Matrix::translation(0.0f, 0.0f, 0.0f));
        RaytracingPipeline::Material material{};
        material.params.albedo = {0.8f, 0.45f, 0.25f, 1.0f};
        material.params.specular = {0.58f, 0.58f, 0.58f, 1.0f};
        material.params.roughness = 0.5f;
        material.params.reflectivity = 0.7f;
        material.params.type = 0;
        pipeline->addMaterial(material);

        // the rest pose, and the positions the wave writes from it (a producer on the device would hand setPositions its own buffer)
        const uint32_t n = model->getNumVertices();
        std::vector<rt_vertex> rest(n);
        ThrowIfFailed(rt_model_read_geometry(model->getHandle(), rest.data(), nullptr));
        std::vector<float> xyz(3 * size_t(n));

        auto camera = std::make_shared<Math::Camera>();
        camera->SetAspectRatio(float(width) / float(height));
        camera->SetEyeAtUp({0.0f, 1.0f, 4.0f}, {0.0f, 0.0f, 0.0f}, {0, 1, 0});

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
            const float phase = 0.35f * float(frame);
            for (uint32_t v = 0; v < n; ++v) {
                const rt_float3 p = rest[v].position;
                xyz[3 * size_t(v) + 0] = p.x + 0.15f * std::sin(3.0f * p.y + phase);
                xyz[3 * size_t(v) + 1] = p.y;
                xyz[3 * size_t(v) + 2] = p.z + 0.15f * std::cos(3.0f * p.y + phase);
            }
            model->setPositions(xyz.data(), n);
            model->recomputeNormals();
            scene->update(context);                   // the BLAS rebuilt over the new vertices, the instance record, the TLAS: on the device
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
        std::printf("%s, %u waving vertices: %u frames, %.2f fps, BLAS + TLAS update %.3f ms per frame on the device\n", pipeline->getName(), n, frames,
                    frames / s, frames ? update_ms / frames : 0.0);

        const std::string out = argv[5];
        const bool png = out.size() > 4 && out.compare(out.size() - 4, 4, ".png") == 0;
        ThrowIfFailed(png ? rt_image_write_png(out.c_str(), image.data(), width, height, 1.0f, 1.0f, 0)
                          : rt_image_write_pfm(out.c_str(), image.data(), width, height));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
