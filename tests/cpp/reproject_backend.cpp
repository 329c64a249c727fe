// reproject_backend.cpp — HIPPathTracer::set_reproject through the reference's interface (compiled and run by
// tests/test_gpu_reproject.py): the App's scene through camera A, FRAMES progressive frames, the camera moves
// to B, one more frame. With reprojection off (the one-sample image of B) and with it on (the blend of A's
// reprojected frames with that sample), each twice in turn, and the second also denoised. Writes to OUT, for
// the test to compare with the Python path: u32 W, H, N; N spheres (x, y, z, r) in the order the backend
// uploads them; the two cameras (spt_camera); W*H RGBA8 pixels each: off, on, on and denoised.
//
//   reproject_backend W H FRAMES OUT
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
        std::fprintf(stderr, "usage: reproject_backend W H FRAMES OUT\n");
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

    const float eye_a[3] = {1.5f, 0.75f, -2.0f}, eye_b[3] = {1.35f, 0.8f, -1.9f}, target[3] = {0.0f, -1.0f, 5.0f},
                up[3] = {0.0f, 1.0f, 0.0f};
    spt_camera cam_a, cam_b;
    if (spt_camera_look_at(eye_a, target, up, 55.0f, &cam_a) != SPT_OK) return 1;
    if (spt_camera_look_at(eye_b, target, up, 55.0f, &cam_b) != SPT_OK) return 1;
    spt_reproject_params rp;
    spt_denoise_params dp;
    if (spt_reproject_params_default(&rp) != SPT_OK || spt_denoise_params_default(&dp) != SPT_OK) return 1;

    render::HIPPathTracer tracer(0);
    tracer.set_scene(scene);
    tracer.set_settings(settings);
    const size_t n = (size_t)W * H;
    // (reprojection is switched on only once A's first frame is rendered: the move to A itself reuses nothing)
    auto move = [&](bool reproject) {
        tracer.set_reproject(nullptr);
        tracer.set_camera(&cam_a);
        for (uint32_t f = 0; f < frames; ++f) {
            tracer.render();
            if (f == 0 && reproject) tracer.set_reproject(&rp);
        }
        tracer.set_camera(&cam_b);
        tracer.render();
        return std::vector<uint32_t>(tracer.get_render_result().image_buffer.begin(),
                                     tracer.get_render_result().image_buffer.begin() + n);
    };
    const std::vector<uint32_t> off = move(false);
    const std::vector<uint32_t> on = move(true);
    // with it off again the sequence gives the first image again: nothing of the history is left
    if (move(false) != off) {
        std::fprintf(stderr, "the run with reprojection switched off again differs from the first\n");
        return 1;
    }
    if (move(true) != on) {
        std::fprintf(stderr, "the second run with reprojection on differs from the first\n");
        return 1;
    }
    if (tracer.frame_count() != 1) return 1;
    tracer.set_denoise(&dp);
    const std::vector<uint32_t> on_denoised(tracer.get_render_result().image_buffer.begin(),
                                            tracer.get_render_result().image_buffer.begin() + n);
    tracer.set_denoise(nullptr);

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
    ok = ok && std::fwrite(&cam_a, sizeof(cam_a), 1, f) == 1;
    ok = ok && std::fwrite(&cam_b, sizeof(cam_b), 1, f) == 1;
    ok = ok && std::fwrite(off.data(), sizeof(uint32_t), n, f) == n;
    ok = ok && std::fwrite(on.data(), sizeof(uint32_t), n, f) == n;
    ok = ok && std::fwrite(on_denoised.data(), sizeof(uint32_t), n, f) == n;
    ok = (std::fclose(f) == 0) && ok;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
