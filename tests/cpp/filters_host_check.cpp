// filters_host_check.cpp — the host functions of the a-trous filter, the reprojection, the luminance meter and the
// display transform (spt_atrous_host, spt_reproject_host, spt_luminance_histogram_host, spt_exposure_from_histogram,
// spt_display_host) in a program of its own, compiled with csrc/spt_host.cpp under AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_filters_host.py. No device call: it runs without a GPU.
//
// IN:  u32 W, H, F (the frames in the sums), M (entries of the material table); f32 exposure; the previous view's
//      spt_camera (64 bytes); M words of material_reusable; then W*H*4 floats each: the sums of F frames, their mean,
//      the current view's feat_a and feat_b, the previous view's image with lengths, its feat_a and feat_b.
// OUT: the filtered mean at 1..6 levels (6 images of W*H*4 floats); the reprojected history without and with the
//      material table, each for a NULL and for the posed previous camera (4 images); the 256 counts of sums / F;
//      the exposure they give (1 float); sums / F through each of the three tonemap operators (3 * W*H words).
// Every array is allocated at its exact size, so a read or write past an image's end is caught.
//
//   filters_host_check IN OUT
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "spt.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: filters_host_check IN OUT\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    uint32_t head[4];
    float exposure;
    spt_camera cam;
    if (std::fread(head, sizeof(head), 1, f) != 1 || std::fread(&exposure, sizeof(exposure), 1, f) != 1 ||
        std::fread(&cam, sizeof(cam), 1, f) != 1)
        return 1;
    const uint32_t W = head[0], H = head[1], F = head[2], M = head[3];
    const size_t n = (size_t)W * H;
    std::vector<uint32_t> reusable(M);
    if (std::fread(reusable.data(), sizeof(uint32_t), M, f) != M) return 1;
    std::vector<float> sums(4 * n), mean(4 * n), cur_a(4 * n), cur_b(4 * n), hist(4 * n), hist_a(4 * n), hist_b(4 * n);
    for (std::vector<float>* a : {&sums, &mean, &cur_a, &cur_b, &hist, &hist_a, &hist_b})
        if (std::fread(a->data(), sizeof(float), a->size(), f) != a->size()) return 1;
    std::fclose(f);
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 1;
    bool ok = true;
    auto put = [&](const void* p, size_t size, size_t count) { ok = ok && std::fwrite(p, size, count, o) == count; };

    // ---- the a-trous filter: every level count; the defaults by NULL and in place give the five-level image
    spt_denoise_params dp;
    ok = ok && spt_denoise_params_default(&dp) == SPT_OK;
    std::vector<float> out(4 * n), five(4 * n);
    for (uint32_t levels = 1; levels <= 6; ++levels) {
        spt_denoise_params q = dp;
        q.levels = levels;
        ok = ok && spt_atrous_host(mean.data(), cur_a.data(), cur_b.data(), W, H, &q, out.data()) == SPT_OK;
        put(out.data(), sizeof(float), out.size());
        if (levels == dp.levels) five = out;
    }
    ok = ok && spt_atrous_host(mean.data(), cur_a.data(), cur_b.data(), W, H, nullptr, out.data()) == SPT_OK;
    ok = ok && std::memcmp(out.data(), five.data(), sizeof(float) * 4 * n) == 0;
    std::vector<float> inplace(mean);
    ok = ok && spt_atrous_host(inplace.data(), cur_a.data(), cur_b.data(), W, H, &dp, inplace.data()) == SPT_OK;
    ok = ok && std::memcmp(inplace.data(), five.data(), sizeof(float) * 4 * n) == 0;
    spt_denoise_params bad_dp = dp;
    bad_dp.levels = 0;  // refused inputs return before they touch an array
    ok = ok && spt_atrous_host(mean.data(), cur_a.data(), cur_b.data(), W, H, &bad_dp, out.data()) == SPT_ERR_INVALID;

    // ---- the reprojection: without and with the material table, a NULL and the posed previous camera
    spt_reproject_params rp;
    ok = ok && spt_reproject_params_default(&rp) == SPT_OK;
    for (const uint32_t* table : {(const uint32_t*)nullptr, (const uint32_t*)reusable.data()})
        for (const spt_camera* prev : {(const spt_camera*)nullptr, (const spt_camera*)&cam}) {
            ok = ok && spt_reproject_host(table ? &rp : nullptr, prev, W, H, cur_a.data(), cur_b.data(), hist.data(),
                                          hist_a.data(), hist_b.data(), table, table ? M : 0u, out.data()) == SPT_OK;
            put(out.data(), sizeof(float), out.size());
        }
    spt_reproject_params bad_rp = rp;
    bad_rp.max_history = 0.5f;
    ok = ok && spt_reproject_host(&bad_rp, &cam, W, H, cur_a.data(), cur_b.data(), hist.data(), hist_a.data(),
                                  hist_b.data(), nullptr, 0u, out.data()) == SPT_ERR_INVALID;

    // ---- the luminance meter and the exposure it gives
    std::vector<uint32_t> counts(SPT_METER_BINS);
    ok = ok && spt_luminance_histogram_host(sums.data(), n, (float)F, counts.data()) == SPT_OK;
    put(counts.data(), sizeof(uint32_t), counts.size());
    ok = ok && spt_luminance_histogram_host(sums.data(), n, 0.0f, counts.data()) == SPT_ERR_INVALID;
    spt_exposure_params ep;
    ok = ok && spt_exposure_params_default(&ep) == SPT_OK;
    float e_null = -1.0f, e_given = -2.0f;
    ok = ok && spt_exposure_from_histogram(counts.data(), nullptr, &e_null) == SPT_OK;
    ok = ok && spt_exposure_from_histogram(counts.data(), &ep, &e_given) == SPT_OK;
    ok = ok && std::memcmp(&e_null, &e_given, sizeof(float)) == 0;
    put(&e_null, sizeof(float), 1);
    spt_exposure_params bad_ep = ep;
    bad_ep.low_fraction = bad_ep.high_fraction = 0.5f;
    ok = ok && spt_exposure_from_histogram(counts.data(), &bad_ep, &e_given) == SPT_ERR_INVALID;

    // ---- the display transform, each operator
    std::vector<uint32_t> words(n);
    for (uint32_t tonemap : {(uint32_t)SPT_TONEMAP_CLAMP, (uint32_t)SPT_TONEMAP_REINHARD, (uint32_t)SPT_TONEMAP_ACES}) {
        const spt_display d = {tonemap, exposure, {0u, 0u}};
        ok = ok && spt_display_host(sums.data(), n, (float)F, &d, words.data()) == SPT_OK;
        put(words.data(), sizeof(uint32_t), words.size());
    }
    const spt_display bad_d = {(uint32_t)SPT_TONEMAP_ACES + 1u, exposure, {0u, 0u}};
    ok = ok && spt_display_host(sums.data(), n, (float)F, &bad_d, words.data()) == SPT_ERR_INVALID;

    ok = (std::fclose(o) == 0) && ok;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
