// denoise_backend.cpp — HIPPathTracer::set_denoise through the reference's interface (compiled and run by
// tests/test_gpu_denoise.py): the App's scene, FRAMES progressive frames, then get_render_result() with the
// denoiser off, on (default parameters) and off again. Writes to OUT, for the test to compare with the
// Python path: u32 W, H, N; N spheres (x, y, z, r) in the order the backend uploads them; the W*H RGBA8
// pixels with the denoiser off; the W*H pixels with it on.
//
//   denoise_backend W H FRAMES OUT
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "render/PathTracer.h"
#include "render/Scene.h"
#include "render/Types.h"
#include "spt.h"

#include "../../software-path-tracer_amd/csrc/HIPPathTracer.h"

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: denoise_backend W H FRAMES OUT\n");
        return 2;
    }
    const uint32_t W = (uint32_t)std::atoi(argv[1]), H = (uint32_t)std::atoi(argv[2]), frames = (uint32_t)std::atoi(argv[3]);
    // App::App's scene (src/App.cpp:101-123)
    auto scene = std::make_shared<render::Scene>();
    auto add = [&](float x, float y, float z, float r) {
        auto* s = scene->CreateNode<render::SphereObject>("sphere");
        s->SetRadius(r);
        s->SetPosition(render::Vec3(x, y, z));
    };
    add(0.0f, -1.0f, 5.0f, 1.0f);
    add(0.0f, -102.0f, 5.0f, 100.0f);
    for (int x = -5; x <= 5; x += 2)
        for (int y = -5; y <= 5; y += 2) add((float)x, (float)y, 10.0f, 0.5f);
    auto settings = std::make_shared<render::RenderSettings>();
    settings->setResolution(W, H);
    render::HIPPathTracer tracer(0);
    tracer.set_scene(scene);
    tracer.set_settings(settings);
    for (uint32_t f = 0; f < frames; ++f) tracer.render();

    const size_t n = (size_t)W * H;
    const std::vector<uint32_t> plain(tracer.get_render_result().image_buffer.begin(),
                                      tracer.get_render_result().image_buffer.begin() + n);
    spt_denoise_params params;
    if (spt_denoise_params_default(&params) != SPT_OK) return 1;
    tracer.set_denoise(&params);
    const std::vector<uint32_t> denoised(tracer.get_render_result().image_buffer.begin(),
                                         tracer.get_render_result().image_buffer.begin() + n);
    tracer.set_denoise(nullptr);
    const std::vector<uint32_t> again(tracer.get_render_result().image_buffer.begin(),
                                      tracer.get_render_result().image_buffer.begin() + n);
    if (again != plain) {
        std::fprintf(stderr, "the result with the denoiser switched off again differs from the first\n");
        return 1;
    }
    if (tracer.frame_count() != frames) return 1;

    std::vector<float> spheres;
    for (const auto& [id, node] : scene->GetAllNodes()) {
        (void)id;
        const auto* s = static_cast<const render::SphereObject*>(node);
        const auto p = s->GetPosition();
        spheres.insert(spheres.end(), {p.x, p.y, p.z, s->GetRadius()});
    }
    std::FILE* f = std::fopen(argv[4], "wb");
    if (!f) return 1;
    const uint32_t head[3] = {W, H, (uint32_t)(spheres.size() / 4)};
    bool ok = std::fwrite(head, sizeof(head), 1, f) == 1;
    ok = ok && std::fwrite(spheres.data(), sizeof(float), spheres.size(), f) == spheres.size();
    ok = ok && std::fwrite(plain.data(), sizeof(uint32_t), n, f) == n;
    ok = ok && std::fwrite(denoised.data(), sizeof(uint32_t), n, f) == n;
    ok = (std::fclose(f) == 0) && ok;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
