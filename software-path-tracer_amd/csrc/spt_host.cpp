// spt_host.cpp — include/spt.h's entry points that take no context and make no device call: every filter over
// the caller's arrays (each pixel by the header its kernels compile: the same bits), the parameter defaults, the
// histograms' readings, the camera and environment helpers. Plain C++, no HIP runtime: it runs alone under the
// sanitizers (tests/host_program.py). The four that go through spt_device.h are in spt_capi.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "spt.h"
#include "spt_atrous.h"
#include "spt_atrous_guided.h"
#include "spt_display.h"
#include "spt_noise.h"
#include "spt_params.h"
#include "spt_reproject.h"

using namespace spt;

template <class P>
static int put_defaults(P* out, const P& defaults) {
    if (!out) return SPT_ERR_INVALID;
    *out = defaults;
    return SPT_OK;
}
int spt_denoise_params_default(spt_denoise_params* out) { return put_defaults(out, kDenoiseDefaults); }
int spt_guided_params_default(spt_guided_params* out) { return put_defaults(out, kGuidedDefaults); }
int spt_reproject_params_default(spt_reproject_params* out) { return put_defaults(out, kReprojectDefaults); }
int spt_exposure_params_default(spt_exposure_params* out) { return put_defaults(out, kExposureDefaults); }
int spt_noise_params_default(spt_noise_params* out) { return put_defaults(out, kNoiseDefaults); }

int spt_atrous_host(const float* rgba, const float* feat_a, const float* feat_b, uint32_t width, uint32_t height,
                    const spt_denoise_params* params, float* out) {
    if (!rgba || !feat_a || !feat_b || !out || width == 0 || height == 0) return SPT_ERR_INVALID;
    if ((uint64_t)width * height >= (1ull << 31)) return SPT_ERR_INVALID;
    const spt_denoise_params p = params_or(params, kDenoiseDefaults);
    if (denoise_params_error(p)) return SPT_ERR_INVALID;
    const size_t n = (size_t)width * height;
    const int w = (int)width, h = (int)height;
    std::vector<float> buf[2] = {std::vector<float>(4 * n), std::vector<float>(4 * n)};
    const float* in = rgba;
    for (uint32_t l = 0; l < p.levels; ++l) {
        const AtrousLevel lv = atrous_level(l, p.sigma_color, p.sigma_plane, p.normal_power_log2);
        float* dst = buf[l & 1u].data();
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t at = (size_t)y * width + (size_t)x;
                const float4 cp = pixel_of(in, at);
                const float4 o = atrous_pixel(atrous_tap(cp, pixel_of(feat_a, at), pixel_of(feat_b, at)), cp.w, x, y, w, h, lv,
                                              [&](int, int, int qx, int qy) {
                                                  const size_t q = (size_t)qy * width + (size_t)qx;
                                                  return atrous_tap(pixel_of(in, q), pixel_of(feat_a, q), pixel_of(feat_b, q));
                                              });
                store_pixel(dst, at, o);
            }
        in = dst;
    }
    std::memcpy(out, in, sizeof(float) * 4 * n);
    return SPT_OK;
}

int spt_atrous_guided_host(const float* rgba, const float* moments, const float* feat_a, const float* feat_b,
                           uint32_t width, uint32_t height, uint32_t batches, uint32_t frame_count,
                           const spt_guided_params* params, float* out, float* out_variance) {
    if (!rgba || !moments || !feat_a || !feat_b || !out || width == 0 || height == 0) return SPT_ERR_INVALID;
    if ((uint64_t)width * height >= (1ull << 31)) return SPT_ERR_INVALID;
    if (batches < 2 || frame_count == 0) return SPT_ERR_INVALID;
    const spt_guided_params p = params_or(params, kGuidedDefaults);
    if (guided_params_error(p)) return SPT_ERR_INVALID;
    const size_t n = (size_t)width * height;
    const int w = (int)width, h = (int)height;
    const float inv = guided_inv(batches, frame_count);
    std::vector<float> v0(n);
    for (size_t i = 0; i < n; ++i) v0[i] = guided_variance0(moments[4 * i + 1], inv);
    std::vector<float> vbuf[2] = {std::vector<float>(n), std::vector<float>(n)};
    std::vector<float> cbuf[2] = {std::vector<float>(4 * n), std::vector<float>(4 * n)};
    // (the level before level 0 "wrote" slot 1: the colour is the caller's, the variance the prefilter's)
    if (p.prefilter) {
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                vbuf[1][(size_t)y * width + (size_t)x] = guided_prefilter_pixel(
                    x, y, w, h, [&](int qx, int qy) { return v0[(size_t)qy * width + (size_t)qx]; });
    } else {
        vbuf[1] = v0;
    }
    const float* in = rgba;
    const float* vin = vbuf[1].data();
    for (uint32_t l = 0; l < p.levels; ++l) {
        const GuidedLevel lv = guided_level(l, p);
        float* dst = cbuf[l & 1u].data();
        float* vdst = vbuf[l & 1u].data();
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t at = (size_t)y * width + (size_t)x;
                const float4 cp = pixel_of(in, at);
                float pv;
                const float4 o = guided_pixel(
                    guided_tap(cp, pixel_of(feat_a, at), pixel_of(feat_b, at), vin[at]), cp.w, x, y, w, h, lv,
                    [&](int, int, int qx, int qy) {
                        const size_t q = (size_t)qy * width + (size_t)qx;
                        return guided_tap(pixel_of(in, q), pixel_of(feat_a, q), pixel_of(feat_b, q), vin[q]);
                    },
                    &pv);
                store_pixel(dst, at, o);
                vdst[at] = pv;
            }
        in = dst;
        vin = vdst;
    }
    std::memcpy(out, in, sizeof(float) * 4 * n);
    if (out_variance) std::memcpy(out_variance, vin, sizeof(float) * n);
    return SPT_OK;
}

int spt_reproject_basis(const spt_camera* cam, float rows[9], float origin[3], float* j) {
    if (!rows || !origin || !j) return SPT_ERR_INVALID;
    if (cam && camera_error(*cam)) return SPT_ERR_INVALID;
    const ReprojectView v = reproject_view(cam);
    for (int a = 0; a < 3; ++a) {
        rows[a] = v.ru[a];
        rows[3 + a] = v.rv[a];
        rows[6 + a] = v.rw[a];
        origin[a] = v.o[a];
    }
    *j = v.j;
    return SPT_OK;
}

int spt_reproject_host(const spt_reproject_params* params, const spt_camera* prev_camera, uint32_t width, uint32_t height,
                       const float* cur_a, const float* cur_b, const float* hist_rgba, const float* hist_a,
                       const float* hist_b, const uint32_t* material_reusable, uint32_t n_materials, float* out) {
    if (!cur_a || !cur_b || !hist_rgba || !hist_a || !hist_b || !out || width == 0 || height == 0) return SPT_ERR_INVALID;
    if ((uint64_t)width * height >= (1ull << 31)) return SPT_ERR_INVALID;
    const spt_reproject_params p = params_or(params, kReprojectDefaults);
    if (reproject_params_error(p)) return SPT_ERR_INVALID;
    if (prev_camera && camera_error(*prev_camera)) return SPT_ERR_INVALID;
    const ReprojectView v = reproject_view(prev_camera);
    const size_t n = (size_t)width * height;
    for (size_t at = 0; at < n; ++at) {
        const float4 o = reproject_pixel(
            pixel_of(cur_a, at), pixel_of(cur_b, at), (int)width, (int)height, v, p, material_reusable, n_materials,
            [&](size_t q) { return pixel_of(hist_a, q); }, [&](size_t q) { return pixel_of(hist_b, q); },
            [&](size_t q) { return pixel_of(hist_rgba, q); });
        store_pixel(out, at, o);
    }
    return SPT_OK;
}

int spt_meter_bin(float luminance, uint32_t* bin) {
    if (!bin) return SPT_ERR_INVALID;
    *bin = meter_bin(luminance);
    return SPT_OK;
}

int spt_luminance_histogram_host(const float* rgba, uint64_t n_pixels, float divisor, uint32_t counts[SPT_METER_BINS]) {
    if (!rgba || !counts || n_pixels == 0 || !divisor_ok(divisor)) return SPT_ERR_INVALID;
    std::memset(counts, 0, sizeof(uint32_t) * SPT_METER_BINS);
    for (uint64_t i = 0; i < n_pixels; ++i) counts[meter_bin(pixel_luminance(pixel_of(rgba, i), divisor))] += 1u;
    return SPT_OK;
}

int spt_exposure_from_histogram(const uint32_t counts[SPT_METER_BINS], const spt_exposure_params* params, float* exposure) {
    if (!counts || !exposure) return SPT_ERR_INVALID;
    const spt_exposure_params p = params_or(params, kExposureDefaults);
    if (!exposure_params_ok(p)) return SPT_ERR_INVALID;
    uint64_t total = 0;
    for (int b = 1; b < SPT_METER_BINS; ++b) total += counts[b];
    if (total == 0) {
        *exposure = 1.0f;
        return SPT_OK;
    }
    const double n = (double)total;
    const double lo = (double)p.low_fraction * n, hi = (1.0 - (double)p.high_fraction) * n;
    double c0 = 0.0, sw = 0.0, sl = 0.0;
    for (int b = 1; b < SPT_METER_BINS; ++b) {
        const double c1 = c0 + (double)counts[b];
        const double w = std::max(0.0, std::min(c1, hi) - std::max(c0, lo));
        const int key = kMeterKeyBase + b, e = (key >> 3) - 127, k = key & 7;
        const double centre = (double)e + std::log2(1.0 + ((double)k + 0.5) / 8.0);
        sw += w;
        sl += w * centre;
        c0 = c1;
    }
    double x = (double)p.target_luminance / std::exp2(sl / sw);
    x = std::min(std::max(x, (double)p.min_exposure), (double)p.max_exposure);
    *exposure = (float)x;
    return SPT_OK;
}

int spt_display_host(const float* rgba, uint64_t n_pixels, float divisor, const spt_display* display, uint32_t* out) {
    if (!rgba || !display || !out || n_pixels == 0 || !divisor_ok(divisor)) return SPT_ERR_INVALID;
    const spt_display d = *display;
    if (display_error(d)) return SPT_ERR_INVALID;
    for (uint64_t i = 0; i < n_pixels; ++i) out[i] = display_rgba8(pixel_of(rgba, i), divisor, d);
    return SPT_OK;
}

int spt_noise_update_host(const float* accum_rgba, uint64_t n_pixels, float batch_frames, float frames_before, float* moments) {
    if (!accum_rgba || !moments || n_pixels == 0) return SPT_ERR_INVALID;
    if (!noise_count_ok(batch_frames) || !(frames_before == 0.0f || noise_count_ok(frames_before))) return SPT_ERR_INVALID;
    if ((double)frames_before + (double)batch_frames > (double)kNoiseMaxFrames) return SPT_ERR_INVALID;
    const NoiseBatch b = noise_batch(batch_frames, frames_before);
    for (uint64_t i = 0; i < n_pixels; ++i) {
        const float4 s = frames_before == 0.0f ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : pixel_of(moments, i);
        store_pixel(moments, i, noise_update_pixel(pixel_of(accum_rgba, i), s, b));
    }
    return SPT_OK;
}

int spt_noise_meter_host(const float* moments, uint32_t width, uint32_t height, uint32_t batches, float frames,
                         const spt_noise_params* params, uint32_t counts[SPT_NOISE_BINS], float* e2) {
    if (!moments || !counts) return SPT_ERR_INVALID;
    const spt_noise_params p = params_or(params, kNoiseDefaults);
    if (noise_params_error(p) || noise_image_error(width, height, batches, frames)) return SPT_ERR_INVALID;
    const float inv = noise_inv(batches, frames);
    const int w = (int)width, h = (int)height, radius = (int)p.radius;
    for (int b = 0; b < SPT_NOISE_BINS; ++b) counts[b] = 0u;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t i = (size_t)y * width + x;
            const float e = radius == 0 ? noise_e2(moments[4 * i], moments[4 * i + 1], inv, p.dark_floor)
                                        : noise_pooled_e2(x, y, w, h, radius, inv, p.dark_floor, [&](int tx, int ty) {
                                              const size_t t = (size_t)ty * width + tx;
                                              return make_float2(moments[4 * t], moments[4 * t + 1]);
                                          });
            if (e2) e2[i] = e;
            counts[noise_bin(e)] += 1u;
        }
    return SPT_OK;
}

int spt_noise_from_histogram(const uint32_t counts[SPT_NOISE_BINS], double quantile, double* rel_error) {
    if (!counts || !rel_error || !(quantile > 0.0 && quantile <= 1.0)) return SPT_ERR_INVALID;
    uint64_t total = 0;
    for (int b = 0; b < SPT_NOISE_BINS; ++b) total += counts[b];
    *rel_error = 0.0;
    if (total == 0) return SPT_OK;
    const double need = quantile * (double)total;
    uint64_t cum = 0;
    int bin = SPT_NOISE_BINS - 1;
    for (int b = 0; b < SPT_NOISE_BINS; ++b) {
        cum += counts[b];
        if ((double)cum >= need) {
            bin = b;
            break;
        }
    }
    if (bin == 0) return SPT_OK;
    if (bin == SPT_NOISE_BINS - 1) {
        *rel_error = HUGE_VAL;
        return SPT_OK;
    }
    const uint32_t bits = (uint32_t)(kNoiseKeyBase + bin + 1) << 20;
    float edge;
    __builtin_memcpy(&edge, &bits, sizeof(edge));
    *rel_error = std::sqrt((double)edge);
    return SPT_OK;
}

int spt_camera_look_at(const float eye[3], const float target[3], const float up[3], float vfov_degrees,
                       spt_camera* out) {
    if (!eye || !target || !up || !out) return SPT_ERR_INVALID;
    if (!(vfov_degrees > 0.0f && vfov_degrees < 180.0f)) return SPT_ERR_INVALID;
    auto norm = [](double v[3]) {
        const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (!(l > 0.0) || !std::isfinite(l)) return false;
        for (int a = 0; a < 3; ++a) v[a] /= l;
        return true;
    };
    double f[3], r[3], t[3];
    for (int a = 0; a < 3; ++a) f[a] = (double)target[a] - (double)eye[a];
    if (!norm(f)) return SPT_ERR_INVALID;  // eye == target
    const double upd[3] = {up[0], up[1], up[2]};
    r[0] = upd[1] * f[2] - upd[2] * f[1];  // cross(up, f)
    r[1] = upd[2] * f[0] - upd[0] * f[2];
    r[2] = upd[0] * f[1] - upd[1] * f[0];
    // up parallel to the view direction: |cross| vanishes against |up| (|f| = 1)
    const double ul = std::sqrt(upd[0] * upd[0] + upd[1] * upd[1] + upd[2] * upd[2]);
    const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (!(ul > 0.0) || !std::isfinite(ul) || !(rl > 1e-12 * ul)) return SPT_ERR_INVALID;
    if (!norm(r)) return SPT_ERR_INVALID;
    t[0] = f[1] * r[2] - f[2] * r[1];  // cross(f, r)
    t[1] = f[2] * r[0] - f[0] * r[2];
    t[2] = f[0] * r[1] - f[1] * r[0];
    // tan(vfov / 2); 90 degrees is exactly 1 (tan(pi / 4) in double is 1 - 1 ulp)
    const double h = vfov_degrees == 90.0f ? 1.0 : std::tan((double)vfov_degrees * (3.14159265358979323846 / 360.0));
    spt_camera cam{};
    for (int a = 0; a < 3; ++a) {
        cam.origin[a] = eye[a];
        cam.u[a] = (float)(r[a] * h);
        cam.v[a] = (float)(t[a] * h);
        cam.w[a] = (float)f[a];
    }
    *out = cam;
    return SPT_OK;
}

int spt_env_octa_from_equirect(const float* src, uint32_t sw, uint32_t sh, float* dst, uint32_t dw, uint32_t dh) {
    if (!src || !dst || sw == 0 || sh == 0 || dw == 0 || dh == 0) return SPT_ERR_INVALID;
    const double kPi = 3.14159265358979323846;
    for (uint32_t iy = 0; iy < dh; ++iy) {
        for (uint32_t ix = 0; ix < dw; ++ix) {
            // octahedral decode of the texel centre (the inverse of octa_texel's projection)
            double px = 2.0 * (ix + 0.5) / dw - 1.0, pz = 2.0 * (iy + 0.5) / dh - 1.0;
            double y = 1.0 - std::fabs(px) - std::fabs(pz);
            if (y < 0.0) {
                const double fx = (1.0 - std::fabs(pz)) * (px >= 0.0 ? 1.0 : -1.0);
                const double fz = (1.0 - std::fabs(px)) * (pz >= 0.0 ? 1.0 : -1.0);
                px = fx;
                pz = fz;
            }
            const double len = std::sqrt(px * px + y * y + pz * pz);
            const double x = px / len, yy = y / len, z = pz / len;
            const double phi = std::atan2(x, -z);                              // [-pi, pi]
            const double theta = std::acos(std::max(-1.0, std::min(1.0, yy)));  // 0 at +y
            uint32_t sx = (uint32_t)((phi + kPi) / (2.0 * kPi) * sw), sy = (uint32_t)(theta / kPi * sh);
            sx = std::min(sx, sw - 1u);
            sy = std::min(sy, sh - 1u);
            const float* t = src + 3ull * ((size_t)sy * sw + sx);
            float* o = dst + 4ull * ((size_t)iy * dw + ix);
            o[0] = t[0];
            o[1] = t[1];
            o[2] = t[2];
            o[3] = 1.0f;
        }
    }
    return SPT_OK;
}
