// noise_backend.cpp — HIPPathTracer::set_noise_target through the reference's interface (compiled and run by
// tests/test_gpu_noise.py): the App's scene in reference mode, one frame per render().
//   1. with the target on, render() until converged() (at most MAX calls); the frame count then stops, five
//      more render() calls change no bit of get_render_result(), and a camera change clears converged();
//   2. a second tracer with the target off renders as many frames: its result is what a backend without the
//      feature gives (the test rebuilds it from a Context).
// Writes to OUT: u32 W, H, N, the frame count at convergence, the render() calls made until then; N spheres
// (x, y, z, r) in the order the backend uploads them; f64 noise() at convergence; the W*H*4 floats of the converged
// accumulation; the W*H RGBA8 pixels of the converged result and of the second tracer's.
//
//   noise_backend W H TARGET QUANTILE MAX OUT
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "render/PathTracer.h"
#include "render/Scene.h"
#include "render/Types.h"
#include "spt.h"

#include "../../software-path-tracer_amd/csrc/HIPPathTracer.h"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: noise_backend W H TARGET QUANTILE MAX OUT\n");
        return 2;
    }
    const uint32_t W = (uint32_t)std::atoi(argv[1]), H = (uint32_t)std::atoi(argv[2]);
    const double target = std::atof(argv[3]), quantile = std::atof(argv[4]);
    const uint32_t max_calls = (uint32_t)std::atoi(argv[5]);
    // App::App's scene (src/App.cpp:101-123); one per tracer: a tracer marks its scene's changes processed
    auto make_scene = [] {
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
        return scene;
    };
    auto scene = make_scene();
    auto settings = std::make_shared<render::RenderSettings>();
    settings->setResolution(W, H);
    const size_t n = (size_t)W * H;

    render::HIPPathTracer tracer(0);
    tracer.set_scene(scene);
    tracer.set_settings(settings);
    CHECK(!tracer.converged() && std::isinf(tracer.noise()));
    tracer.set_noise_target(target, quantile);
    uint32_t calls = 0;
    while (!tracer.converged() && calls < max_calls) {
        tracer.render();
        ++calls;
        CHECK(tracer.frame_count() == calls);
    }
    CHECK(tracer.converged() && tracer.noise() <= target);
    const uint32_t frames = tracer.frame_count();
    const double noise = tracer.noise();
    auto result = [&](render::HIPPathTracer& t) {
        const auto& r = t.get_render_result();
        return std::vector<uint32_t>(r.image_buffer.begin(), r.image_buffer.begin() + n);
    };
    const std::vector<uint32_t> shown = result(tracer);
    std::vector<float> accum, again;
    tracer.read_accumulation(accum);
    for (int k = 0; k < 5; ++k) {
        tracer.render();
        CHECK(tracer.converged() && tracer.frame_count() == frames && tracer.noise() == noise);
        CHECK(result(tracer) == shown);
    }
    tracer.read_accumulation(again);
    CHECK(again == accum);
    // a camera change restarts the accumulation: not converged, one frame
    const float eye[3] = {0.5f, 0.25f, -1.0f}, at[3] = {0.0f, 0.0f, 5.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    spt_camera cam;
    CHECK(spt_camera_look_at(eye, at, up, 60.0f, &cam) == SPT_OK);
    tracer.set_camera(&cam);
    CHECK(tracer.converged());  // (it takes effect at the next render())
    tracer.render();
    CHECK(!tracer.converged() && tracer.frame_count() == 1 && std::isinf(tracer.noise()));

    // the target off (never set): as many frames from a tracer that makes today's calls
    render::HIPPathTracer plain(0);
    plain.set_scene(make_scene());
    auto plain_settings = std::make_shared<render::RenderSettings>();
    plain_settings->setResolution(W, H);
    plain.set_settings(plain_settings);
    plain.set_noise_target(0.0);
    for (uint32_t k = 0; k < frames; ++k) plain.render();
    CHECK(plain.frame_count() == frames && !plain.converged());
    const std::vector<uint32_t> off = result(plain);
    plain.read_accumulation(again);
    CHECK(again == accum);

    std::vector<float> spheres;
    for (const auto& [id, node] : scene->GetAllNodes()) {
        (void)id;
        const auto* s = static_cast<const render::SphereObject*>(node);
        const auto p = s->GetPosition();
        spheres.insert(spheres.end(), {p.x, p.y, p.z, s->GetRadius()});
    }
    std::FILE* f = std::fopen(argv[6], "wb");
    if (!f) return 1;
    const uint32_t head[5] = {W, H, (uint32_t)(spheres.size() / 4), frames, calls};
    bool ok = std::fwrite(head, sizeof(head), 1, f) == 1;
    ok = ok && std::fwrite(spheres.data(), sizeof(float), spheres.size(), f) == spheres.size();
    ok = ok && std::fwrite(&noise, sizeof(noise), 1, f) == 1;
    ok = ok && std::fwrite(accum.data(), sizeof(float), accum.size(), f) == accum.size();
    for (const auto* img : {&shown, &off}) ok = ok && std::fwrite(img->data(), sizeof(uint32_t), n, f) == n;
    ok = (std::fclose(f) == 0) && ok;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
