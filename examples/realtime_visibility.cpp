// Objects that appear and disappear, through the reference-shaped C++ API: a pool of instances of one model is added up front on a grid, and
// every frame another part of it is alive -- shown and hidden with RtScene::setInstanceMask + RtScene::update (extensions: the reference fills
// the InstanceMask of its instance descriptors with the constant 0xFF, Helpers/TopLevelASGenerator.cpp:344-362, and traces every ray with the
// inclusion mask 0xFF).  Indices and materials stay where they are; no scene is thrown away, no BLAS is built after the first frame and no
// instance is parked outside the scene.  Rendered by the RealtimeRaytracingPipeline and filtered by the DenoiseCompositor as in
// realtime_animated.cpp; the denoised last frame is written as a PNG or PFM.
//
//   realtime_visibility <model.obj> <width> <height> <frames> <out.png|out.pfm> [grid side, default 4]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "DenoiseCompositor.h"
#include "RealtimeRaytracingPipeline.h"

using namespace DXRFramework;

// instance k of the pool is alive in `frame` unless (k + frame) is a multiple of three: a third of the pool is hidden, another third every frame
static bool alive(int k, UINT frame) { return (UINT(k) + frame) % 3u != 0u; }

int main(int argc, char **argv)
{
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s model.obj width height frames out.png|out.pfm [grid side]\n", argv[0]);
        return 2;
    }
    const UINT width = std::atoi(argv[2]), height = std::atoi(argv[3]), frames = std::atoi(argv[4]);
    const int side = argc > 6 ? std::atoi(argv[6]) : 4;
    if (side < 2 || side > 64) { std::fprintf(stderr, "grid side 2 .. 64\n"); return 2; }
    try {
        auto context = RtContext::create(0);
        auto scene = RtScene::create();
        auto model = RtModel::create(context, argv[1]);
        auto pipeline = RealtimeRaytracingPipeline::create(context);
        const float spacing = 3.0f;
        for (int k = 0; k < side * side; ++k) {
            scene->addModel(model, Matrix::translation((float(k % side) - 0.5f * float(side - 1)) * spacing, 0.0f, (float(k / side) - 0.5f * float(side - 1)) * spacing));
            RaytracingPipeline::Material material{};
            material.params.albedo = {0.25f + 0.7f * float(k % 3 == 0), 0.25f + 0.7f * float(k % 3 == 1), 0.25f + 0.7f * float(k % 3 == 2), 1.0f};
            material.params.specular = {0.58f, 0.58f, 0.58f, 1.0f};
            material.params.roughness = 0.5f;
            material.params.reflectivity = 0.7f;
            material.params.type = k % 3;
            pipeline->addMaterial(material);
        }
        auto camera = std::make_shared<Math::Camera>();
        camera->SetAspectRatio(float(width) / float(height));
        camera->SetEyeAtUp({0.0f, 1.2f * float(side), 2.4f * float(side)}, {0.0f, 0.0f, 0.0f}, {0, 1, 0});

        pipeline->setScene(scene);
        pipeline->setCamera(camera);
        pipeline->loadResources(3);
        pipeline->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);
        pipeline->buildAccelerationStructures();      // the BLAS and the TLAS of the whole pool: the only build

        auto denoiser = DenoiseCompositor::create(context);
        denoiser->loadResources(3, false);
        denoiser->createOutputResource(RT_FORMAT_R32G32B32A32_FLOAT, width, height);

        double update_ms = 0.0;
        int shown = side * side;
        const auto t0 = std::chrono::steady_clock::now();
        for (UINT frame = 1; frame <= frames; ++frame) {
            shown = 0;
            for (int k = 0; k < side * side; ++k) {
                scene->setInstanceMask((uint32_t)k, alive(k, frame) ? 0xFF : 0x00);
                shown += alive(k, frame);
            }
            scene->update(context);                   // the TLAS of the instances alive now, on the device; the records stay the pool's
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
        std::printf("%s, a pool of %d instances, %d alive in the last frame: %u frames, %.2f fps, TLAS update %.3f ms per frame on the device\n", pipeline->getName(),
                    side * side, shown, frames, frames / s, frames ? update_ms / frames : 0.0);

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
