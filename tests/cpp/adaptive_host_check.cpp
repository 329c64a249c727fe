// adaptive_host_check.cpp — csrc/spt_adaptive.h's functions on the host, in a program of its own: compiled as plain
// C++ (the header alone, tests/host_program.py) with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_adaptive_host.py, which compares what it writes with tests/adaptive_ref.py. No device call: it runs
// without a GPU.
//
// IN:  u32 W, H, B, F (batches and frames of the selection), radius, min_batches; f32 rel_error, exposure;
//      W*H floats of e2; W*H words of stop; W*H*4 floats of sums.
// OUT: W*H keep bytes; W*H*4 floats of the mean image; W*H RGBA8 words.
// Invalid parameters: exit status 3 and no output. Every array is allocated at its exact size, so a read or write
// past an image's end is caught.
//
//   adaptive_host_check IN OUT
#include <cstdint>
#include <cstdio>
#include <vector>

#include "spt_adaptive.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: adaptive_host_check IN OUT\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    uint32_t head[6];
    float par[2];
    if (std::fread(head, sizeof(head), 1, f) != 1 || std::fread(par, sizeof(par), 1, f) != 1) return 1;
    const uint32_t W = head[0], H = head[1], B = head[2], F = head[3];
    const spt::AdaptiveParams p{par[0], head[4], head[5]};
    const size_t n = (size_t)W * H;
    std::vector<float> e2(n), accum(4 * n);
    std::vector<uint32_t> stop(n);
    if (std::fread(e2.data(), sizeof(float), n, f) != n || std::fread(stop.data(), sizeof(uint32_t), n, f) != n ||
        std::fread(accum.data(), sizeof(float), 4 * n, f) != 4 * n)
        return 1;
    std::fclose(f);
    std::vector<uint8_t> keep(n, 7);
    if (!spt::adaptive_select_image(e2.data(), stop.data(), W, H, B, F, p, keep.data())) return 3;
    bool ok = true;
    for (size_t i = 0; i < n; ++i) ok = ok && keep[i] <= 1 && !(keep[i] && stop[i]);  // a retired pixel never comes back
    std::vector<float> mean(4 * n);
    std::vector<uint32_t> words(n);
    for (size_t i = 0; i < n; ++i) {
        const float4 a = make_float4(accum[4 * i], accum[4 * i + 1], accum[4 * i + 2], accum[4 * i + 3]);
        const float4 m = spt::adaptive_mean_pixel(a);
        mean[4 * i] = m.x;
        mean[4 * i + 1] = m.y;
        mean[4 * i + 2] = m.z;
        mean[4 * i + 3] = m.w;
        words[i] = spt::adaptive_rgba8(a, par[1]);
    }
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 1;
    ok = ok && std::fwrite(keep.data(), 1, n, o) == n;
    ok = ok && std::fwrite(mean.data(), sizeof(float), mean.size(), o) == mean.size();
    ok = ok && std::fwrite(words.data(), sizeof(uint32_t), words.size(), o) == words.size();
    ok = (std::fclose(o) == 0) && ok;
    std::printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
