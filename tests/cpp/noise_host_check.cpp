// noise_host_check.cpp — the noise estimate's host functions (spt_noise_update_host, spt_noise_meter_host,
// spt_noise_from_histogram) in a program of its own, compiled with csrc/spt_host.cpp under AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_noise_host.py. No device call: it runs without a GPU.
//
// IN:  u32 W, H, K; K rising frame counts; K accumulations of W*H*4 floats.
// OUT: the W*H*4 floats of the moments after the K batches; then for radius 0, 1, 2: 256 counts, W*H floats of e2.
// Every array is allocated at its exact size, so a read or write past an image's end is caught.
//
//   noise_host_check IN OUT
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "spt.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: noise_host_check IN OUT\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    uint32_t head[3];
    if (std::fread(head, sizeof(head), 1, f) != 1) return 1;
    const uint32_t W = head[0], H = head[1], K = head[2];
    const size_t n = (size_t)W * H;
    std::vector<uint32_t> frames(K);
    if (K < 2 || std::fread(frames.data(), sizeof(uint32_t), K, f) != K) return 1;
    std::vector<float> moments(4 * n, 7.0f);  // (the first batch ignores what they hold)
    uint32_t before = 0;
    for (uint32_t k = 0; k < K; ++k) {
        std::vector<float> accum(4 * n);
        if (std::fread(accum.data(), sizeof(float), accum.size(), f) != accum.size()) return 1;
        if (spt_noise_update_host(accum.data(), n, (float)(frames[k] - before), (float)before, moments.data()) != SPT_OK) {
            std::fprintf(stderr, "spt_noise_update_host failed at batch %u\n", k);
            return 1;
        }
        before = frames[k];
    }
    std::fclose(f);
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 1;
    bool ok = std::fwrite(moments.data(), sizeof(float), moments.size(), o) == moments.size();
    for (uint32_t radius = 0; radius <= 2; ++radius) {
        spt_noise_params p;
        if (spt_noise_params_default(&p) != SPT_OK) return 1;
        p.radius = radius;
        std::vector<uint32_t> counts(SPT_NOISE_BINS);
        std::vector<float> e2(n);
        if (spt_noise_meter_host(moments.data(), W, H, K, (float)before, &p, counts.data(), e2.data()) != SPT_OK) return 1;
        if (spt_noise_meter_host(moments.data(), W, H, K, (float)before, &p, counts.data(), nullptr) != SPT_OK) return 1;
        uint64_t total = 0;
        for (uint32_t c : counts) total += c;
        double rel = -1.0;
        if (total != n || spt_noise_from_histogram(counts.data(), 0.95, &rel) != SPT_OK || !(rel >= 0.0)) return 1;
        ok = ok && std::fwrite(counts.data(), sizeof(uint32_t), counts.size(), o) == counts.size();
        ok = ok && std::fwrite(e2.data(), sizeof(float), e2.size(), o) == e2.size();
    }
    // refused inputs return before they touch an array
    spt_noise_params bad{};
    bad.radius = 3;
    std::vector<uint32_t> counts(SPT_NOISE_BINS);
    ok = ok && spt_noise_meter_host(moments.data(), W, H, K, (float)before, &bad, counts.data(), nullptr) == SPT_ERR_INVALID;
    ok = ok && spt_noise_meter_host(moments.data(), W, H, 1, (float)before, nullptr, counts.data(), nullptr) == SPT_ERR_INVALID;
    ok = ok && spt_noise_update_host(moments.data(), n, NAN, 0.0f, moments.data()) == SPT_ERR_INVALID;
    ok = ok && spt_noise_update_host(moments.data(), n, 3.0e9f, 0.0f, moments.data()) == SPT_ERR_INVALID;
    ok = (std::fclose(o) == 0) && ok;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
