// HIPPathTracer.h — render::PathTracer backend over libspt_hip.so (the GPU_HIP backend).
//
// Mirrors render::CPUPathTracer (reference libs/render/src/engines/pathtracer/backends/cpu/
// CPUPathTracer.h:21-75) member for member: the same progressive state (frame count, dirty/resize
// handling, backend-owned RenderResult), with the integrator running on an MI355X through the C-ABI
// (include/spt.h). Errors follow the reference's fail-stop convention: verify() prints and aborts
// (render_assert.h:15-25).
#pragma once

#include <cmath>
#include <memory>
#include <vector>

#include "render/PathTracer.h"
#include "spt.h"

namespace render
{
	class HIPPathTracer : public PathTracer
	{
	public:
		explicit HIPPathTracer(int device_id = 0);
		~HIPPathTracer() override;

		HIPPathTracer(const HIPPathTracer &) = delete;
		HIPPathTracer &operator=(const HIPPathTracer &) = delete;

		void render() override;

		void set_scene(std::shared_ptr<Scene> scene) override { m_scene = scene; }
		void set_settings(std::shared_ptr<RenderSettings> settings) override { m_renderSettings = settings; }

		std::shared_ptr<Scene> get_scene() const override { return m_scene; }
		std::shared_ptr<RenderSettings> get_settings() const override { return m_renderSettings; }

		std::string get_backend_name() const override { return "GPU Path Tracer (HIP, MI355X gfx950)"; }
		BackendType get_backend_type() const override { return BackendType::GPU_HIP; }

		const PathTracer::RenderResult &get_render_result() override;

		// Not in the reference interface: the float RGBA accumulation (W*H*4), for tests and tools.
		void read_accumulation(std::vector<float> &out);
		uint32_t frame_count() const { return m_frameCount; }

		// Not in the reference interface: honour RenderSettings' max bounces,
		// Russian-roulette depth, samples per pixel per render() call, progressive flag and
		// exposure, which CPUPathTracer ignores (CPUPathTracer.cpp:199, :264, :101-104). Off by
		// default: reference mode renders bit-identically to the reference. Takes effect at the
		// next render() (it re-configures and restarts the accumulation).
		void set_settings_mode(bool enabled);
		bool settings_mode() const { return m_settingsMode; }

		// Not in the reference interface (its camera is hard-coded, CPUPathTracer.cpp:53-73): the camera
		// of the next render() on (spt.h spt_camera, e.g. from spt_camera_look_at; copied), and back to
		// the reference's. A change takes effect at the next render(), which restarts the accumulation.
		void set_camera(const spt_camera *camera);
		void clear_camera() { set_camera(nullptr); }

		// Not in the reference interface: a thin lens on that camera (spt.h spt_lens; copied) from the
		// next render() on, which restarts the accumulation; nullptr or radius 0 removes it. It needs a
		// camera (render() fails without one), stays when the camera moves, and goes with clear_camera() at
		// the moment of that call: a lens set before it, applied or still pending, is dropped.
		void set_lens(const spt_lens *lens);
		void clear_lens() { set_lens(nullptr); }

		// Not in the reference interface (it shades one Lambertian 0.7, CPUPathTracer.cpp:260-274): the
		// material models of the next render() on (spt.h spt_material_model; copied), one per material of
		// the uploaded scene — this backend's scenes have the single reference material, so n is 1 — or
		// (nullptr, 0) for all-diffuse. Kept across scene rebuilds; a change restarts the accumulation.
		void set_material_models(const spt_material_model *models, uint32_t n);

		// Not in the reference interface (it shows the noisy mean): while on, get_render_result() returns the
		// denoised image (spt.h spt_denoise with these parameters; copied) of the frames accumulated so far.
		// nullptr switches it off, which is the default. render() and the accumulation are the same either
		// way, except that a one-frame render() does not fuse the plain resolve into its launch while on.
		void set_denoise(const spt_denoise_params *params);

		// Not in the reference interface: the variance-guided denoiser (spt.h spt_denoise_guided with these
		// parameters; copied). While on, render() folds a batch into the ctx's noise estimate every
		// kNoiseUpdateEvery frames, with or without a noise target (it meters only with one), and
		// get_render_result() returns the guided image once kGuidedMinBatches batches are folded; below that
		// the variance is too noisy to guide and it returns the plain spt_denoise image
		// (set_denoise's parameters if that is on too, else the defaults). A camera, scene or settings change
		// restarts the sequence through the ctx's own invalidation. With set_reproject on the blend is shown
		// as without this call: the guided filter is not applied to it (its variance is not tracked).
		// nullptr switches it off, which is the default: the backend then makes exactly the calls it makes
		// without this.
		static constexpr uint32_t kGuidedMinBatches = 4;
		void set_denoise_guided(const spt_guided_params *params);

		// Not in the reference interface (it restarts at one sample after every change): temporal reprojection
		// (spt.h spt_reproject with these parameters; copied). While on, a camera or lens change that arrives
		// with frames accumulated captures the view before it is applied and reprojects it after, and
		// get_render_result() returns the blend of that history with the frames since (the denoised blend with
		// set_denoise on). A scene or settings change drops the history through the ctx's own invalidation.
		// nullptr switches it off and drops the history; off is the default, and the backend is then what it
		// is without this call (a one-frame render() fuses its resolve only while off).
		void set_reproject(const spt_reproject_params *params);

		// Not in the reference interface (its resolve clamps): the tone-mapping operator of get_render_result()
		// (spt.h spt_tonemap); SPT_TONEMAP_CLAMP, the default, is the plain resolve. With another operator, or in
		// settings mode with RenderSettings::getAutoExposure(), get_render_result() meters the image it is about
		// to show (spt_meter_luminance), takes spt_exposure_from_histogram with getTargetLuminance() as the
		// target, multiplies it by getExposure() (the compensation) and resolves with spt_resolve_display_rgba8;
		// a one-frame render() then does not fuse the plain resolve into its launch. render() and the
		// accumulation are the same either way.
		void set_tonemap(uint32_t tonemap);
		// The auto-exposure's parameters besides the target, which always comes from the settings (copied);
		// nullptr: the library's defaults.
		void set_exposure_params(const spt_exposure_params *params);

		// Not in the reference interface (it renders for as long as its window is open): a stop rule. While
		// rel_error > 0, render() folds the frames since the last fold into the ctx's noise estimate
		// (spt_noise_update) once kNoiseUpdateEvery frames have gathered, and after every kNoiseMeterEvery folds
		// meters it (spt_noise_meter with the default parameters: one stream wait and a 1 KB copy) and takes
		// spt_noise_from_histogram at `quantile`: noise(). Once that is at most rel_error the tracer is
		// converged(): render() then returns without tracing, the frame count stays, and get_render_result()
		// goes on returning the converged image through whichever path is selected. Anything that restarts the
		// accumulation clears converged() and noise(). rel_error <= 0 switches it off, which is the default:
		// the backend then makes exactly the calls it makes without this. The cadences keep the folds and the
		// waits below 5 % each of the frames they follow at 1920 x 1080.
		static constexpr uint32_t kNoiseUpdateEvery = 8;
		static constexpr uint32_t kNoiseMeterEvery = 4;
		void set_noise_target(double rel_error, double quantile = 0.95);
		double noise() const { return m_noise; }  // the last metered value; +inf before the first metering
		bool converged() const { return m_converged; }

	private:
		void invalidate();
		bool display_on() const;
		void resolve_display(uint32_t image, float exposure);
		void rebuild_scene();

		spt_ctx *m_ctx = nullptr;
		std::vector<spt_prim> m_uploaded;  // the primitives last uploaded (spt_update_prims diffs against them)
		bool m_hasUpload = false;
		std::shared_ptr<Scene> m_scene;
		std::shared_ptr<RenderSettings> m_renderSettings;
		PathTracer::RenderResult m_render_result;
		uint32_t m_frameCount = 0;
		bool m_outputDirty = true;
		bool m_settingsMode = false;
		bool m_modeChanged = false;
		bool m_outputRegistered = false;  // the result buffer is page-locked and GPU-mapped
		uint32_t m_resolvedAt = 0;         // render() resolved the result for this frame count (0: none)
		float m_resolvedExposure = 1.0f;   // ... with this exposure
		spt_camera m_camera{};             // set_camera's, while m_hasCamera
		bool m_hasCamera = false;
		bool m_cameraChanged = false;
		spt_lens m_lens{};                 // set_lens's, while m_hasLens
		bool m_hasLens = false;
		bool m_lensChanged = false;
		std::vector<spt_material_model> m_models;  // set_material_models's (empty: all diffuse)
		bool m_modelsChanged = false;
		spt_denoise_params m_denoise{};            // set_denoise's, while m_denoiseOn
		bool m_denoiseOn = false;
		spt_guided_params m_guided{};              // set_denoise_guided's, while m_guidedOn
		bool m_guidedOn = false;
		spt_reproject_params m_reproject{};        // set_reproject's, while m_reprojectOn
		bool m_reprojectOn = false;
		uint32_t m_tonemap = SPT_TONEMAP_CLAMP;    // set_tonemap's
		spt_exposure_params m_exposureParams{};    // set_exposure_params's, while m_hasExposureParams
		bool m_hasExposureParams = false;
		double m_noiseTarget = 0.0;                // set_noise_target's; <= 0: off
		double m_noiseQuantile = 0.95;
		double m_noise = HUGE_VAL;
		bool m_converged = false;
		uint32_t m_noiseFolds = 0;                 // folds since the last metering
		void noise_restart();
		void noise_step();
	};
} // namespace render
