// display_backend.cpp — RenderSettings::setAutoExposure and HIPPathTracer::set_tonemap through the reference's
// interface (compiled and run by tests/test_gpu_display.py): the App's scene in settings mode, SPP frames per
// render(), and get_render_result() three times, each after one render() of a fresh accumulation (a settings
// change restarts it; the frames are the same ones every time):
//   A  setAutoExposure(true, 0.18f), setExposure(1.5f), set_tonemap(SPT_TONEMAP_ACES)
//   B  setAutoExposure(false), set_tonemap(SPT_TONEMAP_CLAMP): the backend without this feature
//   C  as A with set_denoise (default parameters) on
// and, after B without a render(), B's frames with auto-exposure switched on (B', CLAMP) and off again (which has
// to be B: checked here).
// Writes to OUT, for the test to rebuild from a Context: u32 W, H, N; N spheres (x, y, z, r) in the order the
// backend uploads them; the W*H*4 floats of the accumulation; the W*H RGBA8 pixels of A, B, C and B'.
//
//   display_backend W H SPP OUT
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
        std::fprintf(stderr, "usage: display_backend W H SPP OUT\n");
        return 2;
    }
    const uint32_t W = (uint32_t)std::atoi(argv[1]), H = (uint32_t)std::atoi(argv[2]), spp = (uint32_t)std::atoi(argv[3]);
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
    settings->setMaxBounces(4);
    settings->setRussianRouletteDepth(2);
    settings->setSamplesPerPixel(spp);
    settings->setExposure(1.5f);
    render::HIPPathTracer tracer(0);
    tracer.set_settings_mode(true);
    tracer.set_scene(scene);
    tracer.set_settings(settings);

    const size_t n = (size_t)W * H;
    auto shot = [&]() {
        tracer.render();
        const auto& r = tracer.get_render_result();
        return std::vector<uint32_t>(r.image_buffer.begin(), r.image_buffer.begin() + n);
    };
    settings->setAutoExposure(true, 0.18f);
    tracer.set_tonemap(SPT_TONEMAP_ACES);
    const std::vector<uint32_t> a = shot();
    if (tracer.frame_count() != spp) return 1;
    std::vector<float> accum;
    tracer.read_accumulation(accum);

    settings->setAutoExposure(false);
    tracer.set_tonemap(SPT_TONEMAP_CLAMP);
    const std::vector<uint32_t> b = shot();
    if (tracer.frame_count() != spp) return 1;  // (the settings change restarted the accumulation)
    // no render() between: auto-exposure switched on the settings shows B's frames metered (CLAMP), and switched
    // off again the plain resolve, not what the metered resolve left in the result buffer
    auto result = [&]() {
        const auto& r = tracer.get_render_result();
        return std::vector<uint32_t>(r.image_buffer.begin(), r.image_buffer.begin() + n);
    };
    settings->setAutoExposure(true, 0.18f);
    const std::vector<uint32_t> b_metered = result();
    settings->setAutoExposure(false, 0.18f);
    if (result() != b) {
        std::fprintf(stderr, "the result with auto-exposure switched off again differs from the plain resolve\n");
        return 1;
    }

    spt_denoise_params params;
    if (spt_denoise_params_default(&params) != SPT_OK) return 1;
    tracer.set_denoise(&params);
    settings->setAutoExposure(true, 0.18f);
    tracer.set_tonemap(SPT_TONEMAP_ACES);
    const std::vector<uint32_t> c = shot();
    if (tracer.frame_count() != spp) return 1;
    std::vector<float> again;
    tracer.read_accumulation(again);
    if (again != accum) {
        std::fprintf(stderr, "the restarted accumulation differs from the first\n");
        return 1;
    }

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
    ok = ok && std::fwrite(accum.data(), sizeof(float), accum.size(), f) == accum.size();
    for (const auto* img : {&a, &b, &c, &b_metered}) ok = ok && std::fwrite(img->data(), sizeof(uint32_t), n, f) == n;
    ok = (std::fclose(f) == 0) && ok;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
