// guided_host_check.cpp — the variance-guided denoiser's host function (spt_atrous_guided_host) in a program of
// its own, compiled with csrc/spt_host.cpp under AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_guided_host.py. No device call: it runs without a GPU.
//
// IN:  u32 W, H, B, F (batches, frame count); then the mean colour, the moments, feat_a and feat_b, W*H*4 floats each.
// OUT: the W*H*4 floats of the filtered colour, then the W*H floats of its variance (default parameters).
// Every array is allocated at its exact size, so a read or write past an image's end is caught.
//
//   guided_host_check IN OUT
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "spt.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: guided_host_check IN OUT\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    uint32_t head[4];
    if (std::fread(head, sizeof(head), 1, f) != 1) return 1;
    const uint32_t W = head[0], H = head[1], B = head[2], F = head[3];
    const size_t n = (size_t)W * H;
    std::vector<float> rgba(4 * n), moments(4 * n), feat_a(4 * n), feat_b(4 * n);
    for (std::vector<float>* a : {&rgba, &moments, &feat_a, &feat_b})
        if (std::fread(a->data(), sizeof(float), a->size(), f) != a->size()) return 1;
    std::fclose(f);

    spt_guided_params p;
    if (spt_guided_params_default(&p) != SPT_OK) return 1;
    std::vector<float> out(4 * n), var(n);
    if (spt_atrous_guided_host(rgba.data(), moments.data(), feat_a.data(), feat_b.data(), W, H, B, F, &p, out.data(),
                               var.data()) != SPT_OK) {
        std::fprintf(stderr, "spt_atrous_guided_host failed\n");
        return 1;
    }
    bool ok = true;
    // without the variance, with the defaults by NULL, and in place: the same colour
    std::vector<float> again(4 * n);
    ok = ok && spt_atrous_guided_host(rgba.data(), moments.data(), feat_a.data(), feat_b.data(), W, H, B, F, nullptr,
                                      again.data(), nullptr) == SPT_OK;
    ok = ok && std::memcmp(again.data(), out.data(), sizeof(float) * 4 * n) == 0;
    std::vector<float> inplace(rgba);
    ok = ok && spt_atrous_guided_host(inplace.data(), moments.data(), feat_a.data(), feat_b.data(), W, H, B, F, &p,
                                      inplace.data(), nullptr) == SPT_OK;
    ok = ok && std::memcmp(inplace.data(), out.data(), sizeof(float) * 4 * n) == 0;
    // every level count and the prefilter's other setting run to the end
    for (uint32_t levels = 1; levels <= 6; ++levels) {
        spt_guided_params q = p;
        q.levels = levels;
        q.prefilter = levels & 1u;
        ok = ok && spt_atrous_guided_host(rgba.data(), moments.data(), feat_a.data(), feat_b.data(), W, H, B, F, &q,
                                          again.data(), nullptr) == SPT_OK;
    }
    // refused inputs return before they touch an array
    spt_guided_params bad = p;
    bad.variance_floor = 0.0f;
    ok = ok && spt_atrous_guided_host(rgba.data(), moments.data(), feat_a.data(), feat_b.data(), W, H, B, F, &bad,
                                      again.data(), nullptr) == SPT_ERR_INVALID;
    bad = p;
    bad.sigma_variance = NAN;
    ok = ok && spt_atrous_guided_host(rgba.data(), moments.data(), feat_a.data(), feat_b.data(), W, H, B, F, &bad,
                                      again.data(), nullptr) == SPT_ERR_INVALID;
    ok = ok && spt_atrous_guided_host(rgba.data(), moments.data(), feat_a.data(), feat_b.data(), W, H, 1, F, &p,
                                      again.data(), nullptr) == SPT_ERR_INVALID;
    ok = ok && spt_atrous_guided_host(rgba.data(), moments.data(), feat_a.data(), feat_b.data(), W, H, B, 0, &p,
                                      again.data(), nullptr) == SPT_ERR_INVALID;
    ok = ok && spt_atrous_guided_host(rgba.data(), nullptr, feat_a.data(), feat_b.data(), W, H, B, F, &p, again.data(),
                                      nullptr) == SPT_ERR_INVALID;

    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 1;
    ok = ok && std::fwrite(out.data(), sizeof(float), out.size(), o) == out.size();
    ok = ok && std::fwrite(var.data(), sizeof(float), var.size(), o) == var.size();
    ok = (std::fclose(o) == 0) && ok;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
