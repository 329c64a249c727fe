// spt_params.h — the host side of every parameter record of include/spt.h, once each: its default value, its
// validator (nullptr or true: valid; the texts are part of the interface) and the "NULL means the defaults"
// step. Shared by spt_host.cpp and the context's entry points (spt_capi.hip, spt_capi_post.hip). Plain C++.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "spt.h"
#include "spt_atrous.h"
#include "spt_noise.h"

namespace spt {

static_assert(sizeof(spt_denoise_params) == 32, "spt_denoise_params is 32 bytes");
static_assert(sizeof(spt_guided_params) == 32, "spt_guided_params is 32 bytes");
static_assert(sizeof(spt_reproject_params) == 32, "spt_reproject_params is 32 bytes");
static_assert(sizeof(spt_exposure_params) == 32, "spt_exposure_params is 32 bytes");
static_assert(sizeof(spt_display) == 16, "spt_display is 16 bytes");
static_assert(sizeof(spt_noise_params) == 16, "spt_noise_params is 16 bytes");

// the caller's parameters, or the defaults for NULL
template <class P>
P params_or(const P* params, const P& defaults) { return params ? *params : defaults; }

constexpr spt_denoise_params kDenoiseDefaults = {5u, 1.0f, 0.05f, 5u, {0u, 0u, 0u, 0u}};
inline const char* denoise_params_error(const spt_denoise_params& p) {
    if (p.levels < 1u || p.levels > kAtrousMaxLevels) return "spt_denoise_params: levels outside 1..6";
    if (!(p.sigma_color > 0.0f) || !std::isfinite(p.sigma_color)) return "spt_denoise_params: sigma_color must be > 0 and finite";
    if (!(p.sigma_plane > 0.0f) || !std::isfinite(p.sigma_plane)) return "spt_denoise_params: sigma_plane must be > 0 and finite";
    if (p.normal_power_log2 > kAtrousMaxNormalPower) return "spt_denoise_params: normal_power_log2 outside 0..7";
    if (p.reserved[0] | p.reserved[1] | p.reserved[2] | p.reserved[3]) return "spt_denoise_params: reserved must be 0";
    return nullptr;
}

constexpr spt_guided_params kGuidedDefaults = {5u, 4.0f, 0.05f, 5u, 1e-8f, 1u, {0u, 0u}};
inline const char* guided_params_error(const spt_guided_params& p) {
    if (p.levels < 1u || p.levels > kAtrousMaxLevels) return "spt_guided_params: levels outside 1..6";
    if (!(p.sigma_variance > 0.0f) || !std::isfinite(p.sigma_variance)) return "spt_guided_params: sigma_variance must be > 0 and finite";
    if (!(p.sigma_plane > 0.0f) || !std::isfinite(p.sigma_plane)) return "spt_guided_params: sigma_plane must be > 0 and finite";
    if (p.normal_power_log2 > kAtrousMaxNormalPower) return "spt_guided_params: normal_power_log2 outside 0..7";
    if (!(p.variance_floor > 0.0f) || !std::isfinite(p.variance_floor)) return "spt_guided_params: variance_floor must be > 0 and finite";
    if (p.prefilter > 1u) return "spt_guided_params: prefilter must be 0 or 1";
    if (p.reserved[0] | p.reserved[1]) return "spt_guided_params: reserved must be 0";
    return nullptr;
}

constexpr spt_reproject_params kReprojectDefaults = {32.0f, 0.9f, 0.01f, 0.01f, {0u, 0u, 0u, 0u}};
inline const char* reproject_params_error(const spt_reproject_params& p) {
    if (!std::isfinite(p.max_history) || !(p.max_history >= 1.0f)) return "spt_reproject_params: max_history must be finite and >= 1";
    if (!std::isfinite(p.normal_min)) return "spt_reproject_params: normal_min must be finite";
    if (!std::isfinite(p.plane_tolerance) || !(p.plane_tolerance >= 0.0f)) return "spt_reproject_params: plane_tolerance must be finite and >= 0";
    if (!std::isfinite(p.min_weight) || !(p.min_weight > 0.0f)) return "spt_reproject_params: min_weight must be finite and > 0";
    if (p.reserved[0] | p.reserved[1] | p.reserved[2] | p.reserved[3]) return "spt_reproject_params: reserved must be 0";
    return nullptr;
}

constexpr spt_exposure_params kExposureDefaults = {0.18f, 0.1f, 0.02f, 0.015625f, 64.0f, {0u, 0u, 0u}};
inline bool exposure_params_ok(const spt_exposure_params& p) {
    for (const float v : {p.target_luminance, p.low_fraction, p.high_fraction, p.min_exposure, p.max_exposure})
        if (!std::isfinite(v)) return false;
    if (!(p.target_luminance > 0.0f) || !(p.min_exposure > 0.0f) || !(p.max_exposure > 0.0f)) return false;
    if (p.min_exposure > p.max_exposure) return false;
    if (p.low_fraction < 0.0f || p.high_fraction < 0.0f) return false;
    if ((double)p.low_fraction + (double)p.high_fraction >= 1.0) return false;
    return !(p.reserved[0] | p.reserved[1] | p.reserved[2]);
}
inline const char* display_error(const spt_display& d) {
    if (d.tonemap > SPT_TONEMAP_ACES) return "spt_display: unknown tonemap operator";
    if (!std::isfinite(d.exposure) || d.exposure < 0.0f) return "spt_display: exposure must be finite and >= 0";
    if (d.reserved[0] | d.reserved[1]) return "spt_display: reserved must be 0";
    return nullptr;
}
inline bool divisor_ok(float divisor) { return std::isfinite(divisor) && divisor > 0.0f; }

constexpr spt_noise_params kNoiseDefaults = {1u, 0.01f, {0u, 0u}};
inline const char* noise_params_error(const spt_noise_params& p) {
    if (p.radius > (uint32_t)kNoiseMaxRadius) return "spt_noise_params: radius must be 0, 1 or 2";
    if (!std::isfinite(p.dark_floor) || p.dark_floor < 0.0f) return "spt_noise_params: dark_floor must be finite and >= 0";
    if (p.reserved[0] | p.reserved[1]) return "spt_noise_params: reserved must be 0";
    return nullptr;
}

inline const char* camera_error(const spt_camera& cam) {
    double w2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(cam.origin[a]) || !std::isfinite(cam.u[a]) || !std::isfinite(cam.v[a]) ||
            !std::isfinite(cam.w[a]))
            return "camera: non-finite value";
        w2 += (double)cam.w[a] * cam.w[a];
    }
    if (!(w2 > 0.0)) return "camera: w (forward) is zero";
    if (cam.flags & ~(uint32_t)SPT_CAMERA_JITTER) return "camera: unknown flags";
    if (cam.reserved[0] | cam.reserved[1] | cam.reserved[2]) return "camera: reserved must be 0";
    return nullptr;
}
inline const char* lens_error(const spt_lens& l) {
    if (!std::isfinite(l.radius) || l.radius < 0.0f) return "lens: radius must be finite and >= 0";
    if (!std::isfinite(l.focus_distance) || !(l.focus_distance > 0.0f)) return "lens: focus_distance must be finite and > 0";
    if (l.reserved[0] | l.reserved[1]) return "lens: reserved must be 0";
    return nullptr;
}
inline const char* model_error(const spt_material_model& m) {
    if (m.reserved[0] | m.reserved[1]) return "material model: reserved must be 0";
    if (!std::isfinite(m.param)) return "material model: non-finite parameter";
    if (m.kind == SPT_MAT_DIFFUSE) return m.param == 0.0f ? nullptr : "material model: a DIFFUSE parameter must be 0";
    if (m.kind == SPT_MAT_METAL) return m.param >= 0.0f && m.param <= 1.0f ? nullptr : "material model: fuzz outside [0, 1]";
    if (m.kind == SPT_MAT_DIELECTRIC) return m.param > 0.0f ? nullptr : "material model: index of refraction not > 0";
    return "material model: unknown kind";
}

// pixel i of an array of RGBA floats, and back
inline float4 pixel_of(const float* a, uint64_t i) { return make_float4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]); }
inline void store_pixel(float* a, uint64_t i, float4 v) { a[4 * i] = v.x, a[4 * i + 1] = v.y, a[4 * i + 2] = v.z, a[4 * i + 3] = v.w; }

}  // namespace spt
