// A skinned mesh through the reference-shaped C++ API: a tube of 2,976 triangles with two bones, every vertex weighted between them along
// the tube's length (RtModel::setSkin), bent a little further every frame by RtModel::setBones + RtScene::update (extensions: the reference
// imports with aiProcess_PreTransformVertices and reads only mVertices / mNormals, RtModel.cpp:26, :38-45, so it has no bones; and it never
// takes its generators' update path, Helpers/BottomLevelASGenerator.h:136-176).  Per frame the host sends two 3x4 matrices; the vertices are
// written on the device from the rest pose, the one BLAS is rebuilt in place and the TLAS over it.  Rendered by the
// RealtimeRaytracingPipeline and filtered by the DenoiseCompositor as in realtime_deform.cpp; the denoised last frame is written as a PNG or
// PFM.
//
//   realtime_skinned <width> <height> <frames> <out.png|out.pfm>
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
        // the tube: RINGS rings of SEGS vertices about the y axis, y = -1.5 .. 1.5, radius 0.35; the lower end follows bone 0, the upper
        // end bone 1, and the weights cross over smoothly about the joint at y = 0
        const uint32_t RINGS = 32, SEGS = 48;
        std::vector<rt_vertex> verts;
        std::vector<uint32_t> indices, bones;
        std::vector<float> weights;
        for (uint32_t r = 0; r < RINGS; ++r)
            for (uint32_t s = 0; s < SEGS; ++s) {
                const float a = 6.2831853f * float(s) / float(SEGS), y = -1.5f + 3.0f * float(r) / float(RINGS - 1);
                verts.push_back({{0.35f * std::cos(a), y, 0.35f * std::sin(a)}, {std::cos(a), 0.0f, std::sin(a)}});
                float t = (y + 0.6f) / 1.2f;
                t = t < 0.0f ? 0.0f : t > 1.0f ? 1.0f : t;
                const float w1 = t * t * (3.0f - 2.0f * t);
                bones.push_back(0); bones.push_back(1);
                weights.push_back(1.0f - w1); weights.push_back(w1);
            }
        for (uint32_t r = 0; r + 1 < RINGS; ++r)
            for (uint32_t s = 0; s < SEGS; ++s) {
                const uint32_t a = r * SEGS + s, b = r * SEGS + (s + 1) % SEGS, c = a + SEGS, d = b + SEGS;
                indices.insert(indices.end(), {a, c, b, b, c, d});
            }
        const uint32_t n = (uint32_t)verts.size(), tris = (uint32_t)(indices.size() / 3);

        auto context = RtContext::create(0);
        auto scene = RtScene::create();
        auto model = RtModel::create(context, verts.data(), n, indices.data(), tris);
        model->setSkin(bones.data(), weights.data(), 2, 2);       // the vertices as created are the rest pose
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

        double update_ms = 0.0;
        const auto t0 = std::chrono::steady_clock::now();
        for (UINT frame = 1; frame <= frames; ++frame) {
            // the palette: bone 0 stays, bone 1 turns about the z axis through the joint (the origin): a rotation, so the normals are exact
            const float a = 0.2f * float(frame);
            const float palette[24] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0,
                                       std::cos(a), -std::sin(a), 0, 0, std::sin(a), std::cos(a), 0, 0, 0, 0, 1, 0};
            model->setBones(palette);
            scene->update(context);                   // the BLAS rebuilt over the skinned vertices, the instance record, the TLAS: on the device
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
        std::printf("%s, %u skinned vertices, %u triangles, 2 bones: %u frames, %.2f fps, BLAS + TLAS update %.3f ms per frame on the device\n",
                    pipeline->getName(), n, tris, frames, frames / s, frames ? update_ms / frames : 0.0);

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
