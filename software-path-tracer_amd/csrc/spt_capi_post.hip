// spt_capi_post.hip — the C-ABI's post-processing entry points on a context (spt_ctx.h): first-hit features,
// the two denoisers, the denoised, history and blended images, reprojection, the luminance meter with the
// display resolve, the noise estimate. The same definitions over host arrays: spt_host.cpp.
#include <algorithm>
#include <cstring>

#include "spt_ctx.h"
#include "spt_denoise.h"
#include "spt_denoise_guided.h"
#include "spt_display.h"
#include "spt_noise.h"
#include "spt_params.h"
#include "spt_reproject.h"

using namespace spt;

extern "C" {
// ---- first-hit features and the denoiser ---------------------------------------------------------
namespace {
// the images are those of the current scene, camera and configuration (rendered now if they are not)
int ensure_features(spt_ctx* c) {
    if (!c->has_scene) return fail(c, SPT_ERR_NO_SCENE, "Scene not set before rendering");
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "features before spt_configure");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->derived.valid(kFeatures) || c->pixels == 0) return SPT_OK;
    for (Dev<float4>* img : {&c->feat_a, &c->feat_b, &c->feat_albedo})
        if (const int rc = ensure_buf(c, *img, c->pixels, "spt_render_features"); rc != SPT_OK) return rc;
    launch_features(base_params(c), c->d_mat_map, c->feat_a, c->feat_b, c->feat_albedo, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    c->derived.produced(kFeatures);
    return SPT_OK;
}
// what every entry point over a whole image starts with (the denoisers, spt_history_capture, spt_reproject,
// spt_history_blend): a scene, a configuration of one shard, and (features) its current feature images
int whole_image_ready(spt_ctx* c, const char* who, bool features) {
    if (!c->has_scene) return fail(c, SPT_ERR_NO_SCENE, "Scene not set before rendering");
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, std::string(who) + " before spt_configure");
    if (c->cfg.shard_count != 1u) return fail(c, SPT_ERR_INVALID, std::string(who) + " needs the whole image (shard_count 1)");
    // (the grids of k_reproject and the filters' straight form have a block row per 4 image rows)
    if (c->cfg.height > 4u * 65535u) return fail(c, SPT_ERR_INVALID, std::string(who) + ": image taller than 262140 rows");
    if (features) return ensure_features(c);
    SPT_HIP(c, hipSetDevice(c->device));
    return SPT_OK;
}
}  // namespace

int spt_render_features(spt_ctx* c) {
    if (!c) return SPT_ERR_INVALID;
    return ensure_features(c);
}

int spt_read_features(spt_ctx* c, float* feat_a, float* feat_b, float* albedo) {
    if (!c) return SPT_ERR_INVALID;
    const int rc = ensure_features(c);
    if (rc != SPT_OK || c->pixels == 0) return rc;
    const size_t bytes = sizeof(float4) * c->pixels;
    if (feat_a) SPT_HIP(c, hipMemcpyAsync(feat_a, c->feat_a, bytes, hipMemcpyDeviceToHost, on_stream(c)));
    if (feat_b) SPT_HIP(c, hipMemcpyAsync(feat_b, c->feat_b, bytes, hipMemcpyDeviceToHost, on_stream(c)));
    if (albedo) SPT_HIP(c, hipMemcpyAsync(albedo, c->feat_albedo, bytes, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

int spt_features_device_ptr(spt_ctx* c, void** feat_a, void** feat_b, void** albedo, size_t* bytes) {
    if (!c || !bytes) return SPT_ERR_INVALID;
    const int rc = ensure_features(c);
    if (rc != SPT_OK) return rc;
    if (feat_a) *feat_a = c->feat_a;
    if (feat_b) *feat_b = c->feat_b;
    if (albedo) *albedo = c->feat_albedo;
    *bytes = sizeof(float4) * (size_t)c->pixels;
    return SPT_OK;
}

// the filter over `in` / divisor (divisor 0: `in` is already the mean), into the ctx's denoised image
static int denoise_image(spt_ctx* c, const float4* in0, float divisor, const spt_denoise_params* params) {
    const spt_denoise_params p = params_or(params, kDenoiseDefaults);
    // (a missing scene or configuration is reported first, then invalid parameters)
    if (const char* msg = denoise_params_error(p); msg && c->has_scene && c->configured) return fail(c, SPT_ERR_INVALID, msg);
    const int rc = whole_image_ready(c, "spt_denoise", true);
    if (rc != SPT_OK || c->pixels == 0) return rc;
    for (Dev<float4>& img : c->dn)
        if (const int rc = ensure_buf(c, img, c->pixels, "spt_denoise"); rc != SPT_OK) return rc;
    c->derived.begin(kDenoised);
    c->dn_guided = false;
    const int forced = c->dn_form;  // spt_set_denoise_form: one form for every level (measurement), or -1
    for (uint32_t l = 0; l < p.levels; ++l) {
        const AtrousLevel lv = atrous_level(l, p.sigma_color, p.sigma_plane, p.normal_power_log2);
        const float4* in = l == 0 ? in0 : c->dn[(l - 1u) & 1u];
        launch_atrous(forced >= 0 ? forced : atrous_form_of_step(lv.step), in, l == 0 ? divisor : 0.0f,
                      c->feat_a, c->feat_b, c->dn[l & 1u], c->cfg.width, c->cfg.height, lv, on_stream(c));
        SPT_HIP(c, hipGetLastError());
    }
    c->derived.produced_denoised((int)((p.levels - 1u) & 1u));
    return SPT_OK;
}

int spt_denoise(spt_ctx* c, uint32_t frame_count, const spt_denoise_params* params) {
    if (!c) return SPT_ERR_INVALID;
    // (a missing scene or configuration is reported first, by denoise_image; a divisor of 0 would mean "already a mean")
    if (c->has_scene && c->configured && frame_count == 0) return fail(c, SPT_ERR_INVALID, "No frames rendered yet");
    return denoise_image(c, c->accum, (float)frame_count, params);
}

int spt_denoise_guided(spt_ctx* c, uint32_t frame_count, const spt_guided_params* params) {
    if (!c) return SPT_ERR_INVALID;
    const spt_guided_params p = params_or(params, kGuidedDefaults);
    const char* msg = frame_count == 0 ? "No frames rendered yet" : guided_params_error(p);
    if (msg && c->has_scene && c->configured) return fail(c, SPT_ERR_INVALID, msg);  // (after a missing scene or configuration)
    if (const int rc = whole_image_ready(c, "spt_denoise_guided", false); rc != SPT_OK) return rc;
    if (c->noise_batches < 2 || !c->noise_state)
        return fail(c, SPT_ERR_INVALID, "spt_denoise_guided: fewer than two spt_noise_update batches since the accumulation restarted");
    const int rc = ensure_features(c);
    if (rc != SPT_OK || c->pixels == 0) return rc;
    for (Dev<float4>& img : c->dn)
        if (const int rc = ensure_buf(c, img, c->pixels, "spt_denoise_guided"); rc != SPT_OK) return rc;
    for (Dev<float>& plane : c->dn_var)
        if (const int rc = ensure_buf(c, plane, c->pixels, "spt_denoise_guided"); rc != SPT_OK) return rc;
    c->derived.begin(kDenoised);
    c->dn_guided = false;
    // the variance plane "the level before the first" wrote: slot 1, so that level l reads slot (l - 1) & 1
    launch_guided_variance(c->noise_state, c->dn_var[1], c->cfg.width, c->cfg.height, guided_inv(c->noise_batches, frame_count),
                           p.prefilter != 0u, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    const int forced = c->dn_form;  // spt_set_denoise_form: one form for every level (measurement), or -1
    for (uint32_t l = 0; l < p.levels; ++l) {
        const GuidedLevel lv = guided_level(l, p);
        const float4* in = l == 0 ? (const float4*)c->accum : (const float4*)c->dn[(l - 1u) & 1u];
        launch_guided_level(forced >= 0 ? forced : guided_form_of_step(lv.step), in, l == 0 ? (float)frame_count : 0.0f,
                            c->dn_var[(l + 1u) & 1u], c->feat_a, c->feat_b, c->dn[l & 1u], c->dn_var[l & 1u],
                            c->cfg.width, c->cfg.height, lv, on_stream(c));
        SPT_HIP(c, hipGetLastError());
    }
    c->derived.produced_denoised((int)((p.levels - 1u) & 1u));
    c->dn_guided = true;
    return SPT_OK;
}

int spt_read_denoised_variance(spt_ctx* c, float* host_v) {
    if (!c || !host_v) return SPT_ERR_INVALID;
    if (!c->derived.valid(kDenoised) || !c->dn_guided)
        return fail(c, SPT_ERR_INVALID, "no guided denoised image: spt_denoise_guided first");
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipMemcpyAsync(host_v, c->dn_var[c->derived.dn_result], sizeof(float) * c->pixels, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

int spt_set_denoise_form(spt_ctx* c, int form) {
    if (!c) return SPT_ERR_INVALID;
    if (form != -1 && form != kAtrousStraight && form != kAtrousTiled)
        return fail(c, SPT_ERR_INVALID, "spt_set_denoise_form: -1 (automatic), 0 (straight) or 1 (tiled)");
    c->dn_form = form;
    return SPT_OK;
}

// ---- the post-processed images: denoised, active history, blended ---------------------------------
// Each is described once: a pointer, whether it is valid (spt_ctx_state.h) and what to say when it is not.
// Reading one back, handing out its address and resolving it to RGBA8 are one body each, for all of them.
enum PostImage { kImgDenoised, kImgHistory, kImgBlended };
// the image, or nullptr with the ctx's error set: there is none
static float4* post_image(spt_ctx* c, PostImage which) {
    const DerivedState& d = c->derived;
    const struct {
        float4* img;  // (a valid one was allocated: never nullptr)
        const char* missing;
    } images[] = {{d.valid(kDenoised) ? c->dn[d.dn_result] : nullptr, "no denoised image: spt_denoise first"},
                  {d.valid(kHistory) ? c->hist : nullptr, "no active history: spt_reproject first"},
                  {d.valid(kBlended) ? c->blend : nullptr, "no blended image: spt_history_blend first"}};
    if (!images[which].img) fail(c, SPT_ERR_INVALID, images[which].missing);
    return images[which].img;
}

static int read_image(spt_ctx* c, PostImage which, float* host_rgba) {
    if (!c || !host_rgba) return SPT_ERR_INVALID;
    const float4* img = post_image(c, which);
    if (!img) return SPT_ERR_INVALID;
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipMemcpyAsync(host_rgba, img, sizeof(float4) * c->pixels, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

static int image_device_ptr(spt_ctx* c, PostImage which, void** dptr, size_t* bytes) {
    if (!c || !dptr || !bytes) return SPT_ERR_INVALID;
    float4* img = post_image(c, which);
    if (!img) return SPT_ERR_INVALID;
    *dptr = img;
    *bytes = sizeof(float4) * (size_t)c->pixels;
    return SPT_OK;
}

// spt_resolve_rgba8_exposure of an image that is already a mean (divisor 1)
static int resolve_mean_rgba8(spt_ctx* c, PostImage which, float exposure, uint32_t* host_out) {
    if (!c || !host_out) return SPT_ERR_INVALID;
    const float4* img = post_image(c, which);
    return img ? resolve_image(c, img, 1.0f, exposure, host_out) : SPT_ERR_INVALID;
}

int spt_read_denoised(spt_ctx* c, float* host_rgba) { return read_image(c, kImgDenoised, host_rgba); }
int spt_denoised_device_ptr(spt_ctx* c, void** dptr, size_t* bytes) { return image_device_ptr(c, kImgDenoised, dptr, bytes); }
int spt_resolve_denoised_rgba8(spt_ctx* c, float exposure, uint32_t* host_out) {
    return resolve_mean_rgba8(c, kImgDenoised, exposure, host_out);
}

// ---- temporal reprojection ------------------------------------------------------------------------
int spt_history_capture(spt_ctx* c, uint32_t frame_count) {
    if (!c) return SPT_ERR_INVALID;
    if (const int rc = whole_image_ready(c, "spt_history_capture", true); rc != SPT_OK) return rc;
    if (frame_count == 0) return fail(c, SPT_ERR_INVALID, "No frames rendered yet");
    if (const int rc = ensure_buf(c, c->hist_view, 3 * (size_t)c->pixels, "spt_history_capture"); rc != SPT_OK) return rc;
    c->derived.begin(kCapturedView);
    const int layout = c->hist_layout >= 0 ? c->hist_layout : kHistoryDefault;
    launch_history_capture(layout, c->accum, (float)frame_count, c->derived.valid(kHistory) ? c->hist : nullptr, c->feat_a, c->feat_b,
                           c->hist_view, c->pixels, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    c->hist_view_layout = layout;
    c->hist_view_has_camera = c->has_camera;
    c->hist_view_camera = c->camera;
    c->derived.produced(kCapturedView);
    return SPT_OK;
}

int spt_reproject(spt_ctx* c, const spt_reproject_params* params) {
    if (!c) return SPT_ERR_INVALID;
    const spt_reproject_params p = params_or(params, kReprojectDefaults);
    if (const char* msg = reproject_params_error(p)) return fail(c, SPT_ERR_INVALID, msg);
    if (const int rc = whole_image_ready(c, "spt_reproject", true); rc != SPT_OK) return rc;
    if (!c->derived.valid(kCapturedView)) return fail(c, SPT_ERR_INVALID, "no captured view: spt_history_capture first");
    if (const int rc = ensure_buf(c, c->hist, c->pixels, "spt_reproject"); rc != SPT_OK) return rc;
    c->derived.begin(kHistory);
    const uint32_t n_mats = (uint32_t)c->h_mats.size();
    if (c->bsdf && !c->derived.valid(kReusable)) {
        // (spt_set_material_models drained the stream before it changed the models: nothing reads the old words)
        std::vector<uint32_t> words(n_mats);
        for (uint32_t m = 0; m < n_mats; ++m) words[m] = c->h_models[m].kind == SPT_MAT_DIFFUSE ? 1u : 0u;
        if (const int rc = ensure_buf(c, c->d_reusable, n_mats, "spt_reproject"); rc != SPT_OK) return rc;
        SPT_HIP(c, hipMemcpy(c->d_reusable, words.data(), sizeof(uint32_t) * n_mats, hipMemcpyHostToDevice));
        c->derived.produced(kReusable);
    }
    const ReprojectView v = reproject_view(c->hist_view_has_camera ? &c->hist_view_camera : nullptr);
    launch_reproject(c->hist_view_layout, c->feat_a, c->feat_b, c->hist_view, c->hist, c->cfg.width, c->cfg.height, v, p,
                     c->bsdf ? c->d_reusable : nullptr, n_mats, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    c->derived.produced(kHistory);
    return SPT_OK;
}

int spt_history_clear(spt_ctx* c) {
    if (!c) return SPT_ERR_INVALID;
    c->derived.drop(Change::HistoryClear);
    return SPT_OK;
}

int spt_read_history(spt_ctx* c, float* host_rgba) { return read_image(c, kImgHistory, host_rgba); }
int spt_history_device_ptr(spt_ctx* c, void** dptr, size_t* bytes) { return image_device_ptr(c, kImgHistory, dptr, bytes); }

int spt_history_blend(spt_ctx* c, uint32_t frame_count) {
    if (!c) return SPT_ERR_INVALID;
    if (const int rc = whole_image_ready(c, "spt_history_blend", false); rc != SPT_OK) return rc;
    if (frame_count == 0) return fail(c, SPT_ERR_INVALID, "No frames rendered yet");
    if (const int rc = ensure_buf(c, c->blend, c->pixels, "spt_history_blend"); rc != SPT_OK) return rc;
    c->derived.begin(kBlended);
    launch_history_blend(c->accum, (float)frame_count, c->derived.valid(kHistory) ? c->hist : nullptr, c->blend, c->pixels, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    c->derived.produced(kBlended);
    return SPT_OK;
}

int spt_read_blended(spt_ctx* c, float* host_rgba) { return read_image(c, kImgBlended, host_rgba); }
int spt_blended_device_ptr(spt_ctx* c, void** dptr, size_t* bytes) { return image_device_ptr(c, kImgBlended, dptr, bytes); }
int spt_resolve_blended_rgba8(spt_ctx* c, float exposure, uint32_t* host_out) {
    return resolve_mean_rgba8(c, kImgBlended, exposure, host_out);
}

int spt_denoise_blended(spt_ctx* c, const spt_denoise_params* params) {
    if (!c) return SPT_ERR_INVALID;
    const float4* img = post_image(c, kImgBlended);
    return img ? denoise_image(c, img, 0.0f, params) : SPT_ERR_INVALID;
}

int spt_set_history_layout(spt_ctx* c, int layout) {
    if (!c) return SPT_ERR_INVALID;
    if (layout != -1 && layout != kHistoryPlanes && layout != kHistoryRecords)
        return fail(c, SPT_ERR_INVALID, "spt_set_history_layout: -1 (automatic), 0 (three images) or 1 (48-byte records)");
    c->hist_layout = layout;
    return SPT_OK;
}

// ---- exposure and tone mapping: the luminance meter and the display resolve -------------------------
namespace {
// The ctx image `image` with its divisor (the frame count for the sums, 1 for a mean), or nullptr with the
// status to return in *rc.
const float4* display_source(spt_ctx* c, uint32_t image, uint32_t frame_count, float* divisor, int* rc) {
    *rc = SPT_ERR_INVALID;
    if (image > SPT_IMAGE_BLENDED) {
        fail(c, SPT_ERR_INVALID, "unknown image: SPT_IMAGE_ACCUM, SPT_IMAGE_DENOISED or SPT_IMAGE_BLENDED");
        return nullptr;
    }
    if (!c->configured) {
        *rc = fail(c, SPT_ERR_NOT_CONFIGURED, "not configured");
        return nullptr;
    }
    *divisor = 1.0f;
    if (image != SPT_IMAGE_ACCUM) return post_image(c, image == SPT_IMAGE_DENOISED ? kImgDenoised : kImgBlended);
    if (frame_count == 0) {
        fail(c, SPT_ERR_INVALID, "No frames rendered yet");
        return nullptr;
    }
    *divisor = (float)frame_count;
    return c->accum;
}

// counts = the histogram of img[0..n) / divisor, waited for
int meter_image(spt_ctx* c, const char* who, const float4* img, uint64_t n, float divisor, uint32_t* counts) {
    SPT_HIP(c, hipSetDevice(c->device));
    if (const int rc = ensure_buf(c, c->meter_counts, SPT_METER_BINS, who); rc != SPT_OK) return rc;
    SPT_HIP(c, hipMemsetAsync(c->meter_counts, 0, sizeof(uint32_t) * SPT_METER_BINS, on_stream(c)));
    launch_meter(c->meter_form >= 0 ? c->meter_form : meter_default_form(), img, n, divisor, c->meter_counts, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    SPT_HIP(c, hipMemcpyAsync(counts, c->meter_counts, sizeof(uint32_t) * SPT_METER_BINS, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

}  // namespace

int spt_meter_luminance(spt_ctx* c, uint32_t image, uint32_t frame_count, uint32_t counts[SPT_METER_BINS]) {
    if (!c || !counts) return SPT_ERR_INVALID;
    float divisor = 1.0f;
    int rc = SPT_OK;
    const float4* img = display_source(c, image, frame_count, &divisor, &rc);
    if (!img) return rc;
    return meter_image(c, "spt_meter_luminance", img, c->pixels, divisor, counts);
}

int spt_meter_device_image(spt_ctx* c, const void* device_rgba, uint64_t n_pixels, float divisor,
                           uint32_t counts[SPT_METER_BINS]) {
    if (!c || !device_rgba || !counts) return SPT_ERR_INVALID;
    if (n_pixels == 0) return fail(c, SPT_ERR_INVALID, "spt_meter_device_image: no pixels");
    if (!divisor_ok(divisor)) return fail(c, SPT_ERR_INVALID, "spt_meter_device_image: divisor must be finite and > 0");
    return meter_image(c, "spt_meter_device_image", (const float4*)device_rgba, n_pixels, divisor, counts);
}

int spt_resolve_display_rgba8(spt_ctx* c, uint32_t image, uint32_t frame_count, const spt_display* display,
                              uint32_t* host_out) {
    if (!c || !display || !host_out) return SPT_ERR_INVALID;
    const spt_display d = *display;
    if (const char* msg = display_error(d)) return fail(c, SPT_ERR_INVALID, msg);
    float divisor = 1.0f;
    int rc = SPT_OK;
    const float4* img = display_source(c, image, frame_count, &divisor, &rc);
    if (!img) return rc;
    return resolve_image_by(c, host_out, [&](uint32_t* out, hipStream_t s) {
        launch_display(img, c->pixels, divisor, d, out, s);
    });
}

int spt_resolve_display_device_image(spt_ctx* c, const void* device_rgba, uint64_t n_pixels, float divisor,
                                     const spt_display* display, uint32_t* host_out) {
    if (!c || !device_rgba || !display || !host_out) return SPT_ERR_INVALID;
    if (n_pixels == 0) return fail(c, SPT_ERR_INVALID, "spt_resolve_display_device_image: no pixels");
    if (!divisor_ok(divisor))
        return fail(c, SPT_ERR_INVALID, "spt_resolve_display_device_image: divisor must be finite and > 0");
    const spt_display d = *display;
    if (const char* msg = display_error(d)) return fail(c, SPT_ERR_INVALID, msg);
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->display_stage.size() < n_pixels) {
        SPT_HIP(c, hipStreamSynchronize(on_stream(c)));  // (no earlier resolve may still read the old one)
        if (!c->display_stage.ensure_at_least(n_pixels))
            return fail(c, SPT_ERR_HIP, "spt_resolve_display_device_image: allocation failed");
    }
    launch_display((const float4*)device_rgba, n_pixels, divisor, d, c->display_stage, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    SPT_HIP(c, hipMemcpyAsync(host_out, c->display_stage, sizeof(uint32_t) * n_pixels, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

int spt_set_meter_form(spt_ctx* c, int form) {
    if (!c) return SPT_ERR_INVALID;
    if (form != -1 && form != kMeterLanes && form != kMeterPeel)
        return fail(c, SPT_ERR_INVALID, "spt_set_meter_form: -1 (automatic), 0 (an add per lane) or 1 (an add per distinct bin)");
    c->meter_form = form;
    return SPT_OK;
}

// ---- noise estimate: batch moments, the meter, the stop rule ------------------------------------------
namespace {
// counts and the e2 image (may be nullptr) of width x height device moments, waited for
int noise_meter_image(spt_ctx* c, const char* who, const float4* state, uint32_t width, uint32_t height, uint32_t batches,
                      float W, const spt_noise_params& p, uint32_t* counts, float* e2) {
    SPT_HIP(c, hipSetDevice(c->device));
    if (const int rc = ensure_buf(c, c->meter_counts, SPT_METER_BINS, who); rc != SPT_OK) return rc;
    SPT_HIP(c, hipMemsetAsync(c->meter_counts, 0, sizeof(uint32_t) * SPT_NOISE_BINS, on_stream(c)));
    launch_noise_meter(state, width, height, (int)p.radius, noise_inv(batches, W), p.dark_floor, c->meter_counts, e2, on_stream(c));
    SPT_HIP(c, hipGetLastError());
    SPT_HIP(c, hipMemcpyAsync(counts, c->meter_counts, sizeof(uint32_t) * SPT_NOISE_BINS, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}
static_assert(SPT_NOISE_BINS == SPT_METER_BINS, "the two meters share the ctx's 256 device words");
}  // namespace

int spt_noise_update(spt_ctx* c, uint32_t frame_count) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "spt_noise_update before spt_configure");
    if (frame_count <= c->noise_frames) return fail(c, SPT_ERR_INVALID, "spt_noise_update: no frames since the last update");
    if (frame_count > (1u << 24)) return fail(c, SPT_ERR_INVALID, "spt_noise_update: more than 2^24 frames");
    SPT_HIP(c, hipSetDevice(c->device));
    const size_t pixels = std::max<size_t>(c->pixels, 1);
    if (const int rc = ensure_buf(c, c->noise_state, pixels, "spt_noise_update"); rc != SPT_OK) return rc;
    if (c->noise_batches == 0) SPT_HIP(c, hipMemsetAsync(c->noise_state, 0, sizeof(float4) * pixels, on_stream(c)));
    const float w = (float)(frame_count - c->noise_frames);
    launch_noise_update(c->accum, c->noise_state, c->pixels, noise_batch(w, c->noise_W), on_stream(c));
    SPT_HIP(c, hipGetLastError());
    c->noise_W = c->noise_W + w;
    c->noise_frames = frame_count;
    c->noise_batches += 1u;
    c->noise_metered = false;
    return SPT_OK;
}

int spt_noise_batches(const spt_ctx* c, uint32_t* batches, uint32_t* frames) {
    if (!c) return SPT_ERR_INVALID;
    if (batches) *batches = c->noise_batches;
    if (frames) *frames = c->noise_frames;
    return SPT_OK;
}

int spt_noise_meter(spt_ctx* c, const spt_noise_params* params, uint32_t counts[SPT_NOISE_BINS]) {
    if (!c || !counts) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "spt_noise_meter before spt_configure");
    const spt_noise_params p = params_or(params, kNoiseDefaults);
    if (const char* msg = noise_params_error(p)) return fail(c, SPT_ERR_INVALID, msg);
    if (c->noise_batches < 2) return fail(c, SPT_ERR_INVALID, "spt_noise_meter: fewer than two updates since the accumulation restarted");
    if (p.radius > 0 && c->cfg.shard_count != 1u)
        return fail(c, SPT_ERR_INVALID, "spt_noise_meter: pooling (radius > 0) needs the whole image (shard_count 1)");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pixels == 0) {
        std::memset(counts, 0, sizeof(uint32_t) * SPT_NOISE_BINS);
        return SPT_OK;
    }
    if (const int rc = ensure_buf(c, c->noise_e2, c->pixels, "spt_noise_meter"); rc != SPT_OK) return rc;
    const int rc = noise_meter_image(c, "spt_noise_meter", c->noise_state,c->cfg.width, c->rows, c->noise_batches, c->noise_W, p, counts, c->noise_e2);
    c->noise_metered = rc == SPT_OK;
    return rc;
}

int spt_read_noise_moments(spt_ctx* c, float* host_moments) {
    if (!c || !host_moments) return SPT_ERR_INVALID;
    if (!c->noise_state || c->noise_batches == 0) return fail(c, SPT_ERR_INVALID, "no noise moments: spt_noise_update first");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pixels == 0) return SPT_OK;
    SPT_HIP(c, hipMemcpyAsync(host_moments, c->noise_state, sizeof(float4) * c->pixels, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

int spt_read_noise(spt_ctx* c, float* host_e2) {
    if (!c || !host_e2) return SPT_ERR_INVALID;
    if (!c->noise_e2 || !c->noise_metered) return fail(c, SPT_ERR_INVALID, "no noise image: spt_noise_meter first");
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipMemcpyAsync(host_e2, c->noise_e2, sizeof(float) * c->pixels, hipMemcpyDeviceToHost, on_stream(c)));
    SPT_HIP(c, hipStreamSynchronize(on_stream(c)));
    return SPT_OK;
}

int spt_noise_device_ptr(spt_ctx* c, void** moments, void** e2, uint64_t* pixels) {
    if (!c) return SPT_ERR_INVALID;
    if (!c->configured) return fail(c, SPT_ERR_NOT_CONFIGURED, "not configured");
    if (moments) *moments = c->noise_state;
    if (e2) *e2 = c->noise_e2;
    if (pixels) *pixels = c->pixels;
    return SPT_OK;
}

int spt_noise_meter_device_image(spt_ctx* c, const void* device_moments, uint32_t width, uint32_t height, uint32_t batches,
                                 float frames, const spt_noise_params* params, uint32_t counts[SPT_NOISE_BINS],
                                 void* device_e2) {
    if (!c || !device_moments || !counts) return SPT_ERR_INVALID;
    const spt_noise_params p = params_or(params, kNoiseDefaults);
    if (const char* msg = noise_params_error(p)) return fail(c, SPT_ERR_INVALID, msg);
    if (const char* msg = noise_image_error(width, height, batches, frames)) return fail(c, SPT_ERR_INVALID, msg);
    return noise_meter_image(c, "spt_noise_meter_device_image", (const float4*)device_moments, width, height, batches, frames, p, counts, (float*)device_e2);
}
}  // extern "C"
