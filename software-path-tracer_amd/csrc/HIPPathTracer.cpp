// HIPPathTracer.cpp — the GPU_HIP render::PathTracer backend (host C++ above the C-ABI).
//
// Control flow restates render::CPUPathTracer (reference libs/render/src/engines/pathtracer/backends/
// cpu/CPUPathTracer.cpp): render() :43-85, get_render_result() :87-117, invalidate() :119-161,
// rebuild_scene() :328-404. The pixel loop, trace_ray and the resolve run on the GPU
// (spt_render / spt_resolve_rgba8, or both in one launch: spt_render_resolve_rgba8).
#include "HIPPathTracer.h"

#include <cstring>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "render/Scene.h"
#include "render/Types.h"
#include "spt.h"

namespace render
{
	namespace
	{
		// verify(): always-on check that prints and aborts (render_assert.h:15-25).
		void verify(bool condition, const char *message, const char *func, int line)
		{
			if (!condition)
			{
				std::fprintf(stderr, "VERIFY: %s in %s() at %s:%d\n", message, func, __FILE__, line);
				std::abort();
			}
		}
#define SPT_VERIFY(cond, msg) verify((cond), (msg), __func__, __LINE__)

		void verify_spt(spt_ctx *ctx, int rc, const char *what, const char *func, int line)
		{
			if (rc != SPT_OK)
			{
				std::fprintf(stderr, "VERIFY: %s failed (%d): %s in %s() at %s:%d\n", what, rc,
							 ctx ? spt_last_error(ctx) : "", func, __FILE__, line);
				std::abort();
			}
		}
#define SPT_CALL(ctx, call) verify_spt((ctx), (call), #call, __func__, __LINE__)

		// The reference integrator's fixed parameters (CPUPathTracer.cpp:199, :264).
		constexpr uint32_t kReferenceBounces = 4;
		constexpr uint32_t kReferenceRRDepth = 2;
	} // namespace

	HIPPathTracer::HIPPathTracer(int device_id)
	{
		// CPUPathTracer::CPUPathTracer (:25-35): default settings, then device init
		m_renderSettings = std::make_shared<RenderSettings>();
		const int rc = spt_create(&m_ctx, device_id);
		SPT_VERIFY(rc == SPT_OK && m_ctx != nullptr, "HIP device (gfx950) not available");
	}

	HIPPathTracer::~HIPPathTracer()
	{
		spt_destroy(m_ctx); // (unregisters the result buffer before the vector is freed)
	}

	void HIPPathTracer::render()
	{
		SPT_VERIFY(m_ctx != nullptr, "HIP context not initialized");
		SPT_VERIFY(m_scene != nullptr, "Scene not set before rendering");
		if (m_settingsMode && !m_renderSettings->getProgressive())
			m_frameCount = 0; // a fresh accumulation every call
		invalidate();
		if (m_noiseTarget > 0.0)
		{
			if (m_frameCount == 0)
				noise_restart(); // (the ctx's estimate restarted with the accumulation: spt_reset)
			else if (m_converged)
				return; // nothing traced, the frame count stays, what render() resolved stays valid
		}
		// reference mode: one progressive frame = 1 sample per pixel, seeded with m_frameCount + 1
		// (:61); settings mode: getSamplesPerPixel() such frames in one call (k_paths from 4)
		const uint32_t n = m_settingsMode ? std::max<uint32_t>(1u, m_renderSettings->getSamplesPerPixel()) : 1u;
		m_resolvedAt = 0;
		if (m_outputRegistered && n < SPT_PERSISTENT_MIN_FRAMES && !m_denoiseOn && !m_guidedOn && !m_reprojectOn && !display_on())
		{
			// the App reads the result after every render() (App.cpp:230-240): a one-frame call's resolve
			// rides in the frame's own launch, its pixels stored into the registered result buffer as their
			// paths end (longer calls keep render() asynchronous and resolve in get_render_result())
			const float exposure = m_settingsMode ? m_renderSettings->getExposure() : 1.0f;
			SPT_CALL(m_ctx, spt_render_resolve_rgba8(m_ctx, m_frameCount, n, m_frameCount + n, exposure,
													 m_render_result.image_buffer.data()));
			m_resolvedAt = m_frameCount + n;
			m_resolvedExposure = exposure;
		}
		else
		{
			SPT_CALL(m_ctx, spt_render(m_ctx, m_frameCount, n));
		}
		m_frameCount += n;
		if (m_noiseTarget > 0.0 || m_guidedOn)
			noise_step();
	}

	void HIPPathTracer::set_noise_target(double rel_error, double quantile)
	{
		SPT_VERIFY(quantile > 0.0 && quantile <= 1.0, "the noise quantile must be in (0, 1]");
		m_noiseTarget = rel_error > 0.0 ? rel_error : 0.0; // (NaN: off)
		m_noiseQuantile = quantile;
		// (another quantile reads another value off the next metering's histogram: not converged until then)
		m_noise = HUGE_VAL;
		m_converged = false;
	}

	void HIPPathTracer::noise_restart()
	{
		m_noise = HUGE_VAL;
		m_converged = false;
		m_noiseFolds = 0;
	}

	void HIPPathTracer::noise_step()
	{
		// a target switched on over frames that were never folded: they are the first batch
		uint32_t batches = 0, folded = 0;
		SPT_CALL(m_ctx, spt_noise_batches(m_ctx, &batches, &folded));
		if (m_frameCount - folded < kNoiseUpdateEvery)
			return;
		SPT_CALL(m_ctx, spt_noise_update(m_ctx, m_frameCount));
		if (!(m_noiseTarget > 0.0))
			return; // (folded for set_denoise_guided alone: nothing to meter)
		if (++m_noiseFolds < kNoiseMeterEvery || batches + 1u < 2u)
			return;
		m_noiseFolds = 0;
		uint32_t counts[SPT_NOISE_BINS];
		SPT_CALL(m_ctx, spt_noise_meter(m_ctx, nullptr, counts));
		SPT_VERIFY(spt_noise_from_histogram(counts, m_noiseQuantile, &m_noise) == SPT_OK, "invalid noise quantile");
		m_converged = m_noise <= m_noiseTarget;
	}

	void HIPPathTracer::set_settings_mode(bool enabled)
	{
		if (enabled != m_settingsMode)
		{
			m_settingsMode = enabled;
			m_modeChanged = true;
		}
	}

	void HIPPathTracer::set_camera(const spt_camera *camera)
	{
		m_hasCamera = camera != nullptr;
		if (camera)
			m_camera = *camera;
		m_cameraChanged = true;
		if (!camera)
		{
			// the lens goes with its camera, set or pending, at this moment. The ctx drops its own only when
			// render() hands it the cleared camera; if a new camera arrives before that, the ctx would keep
			// its lens across it, so the removal stays pending and render() sends it once a camera is back
			m_hasLens = false;
			m_lensChanged = true;
		}
	}

	void HIPPathTracer::set_lens(const spt_lens *lens)
	{
		m_hasLens = lens != nullptr;
		if (lens)
			m_lens = *lens;
		m_lensChanged = true;
	}

	void HIPPathTracer::set_material_models(const spt_material_model *models, uint32_t n)
	{
		m_models.assign(models ? models : nullptr, models ? models + n : nullptr);
		m_modelsChanged = true;
	}

	void HIPPathTracer::set_denoise(const spt_denoise_params *params)
	{
		m_denoiseOn = params != nullptr;
		if (params)
			m_denoise = *params;
		m_resolvedAt = 0; // (what render() resolved was the other kind of image)
	}

	void HIPPathTracer::set_denoise_guided(const spt_guided_params *params)
	{
		m_guidedOn = params != nullptr;
		if (params)
			m_guided = *params;
		m_resolvedAt = 0; // (what render() resolved was the other kind of image)
	}

	void HIPPathTracer::set_reproject(const spt_reproject_params *params)
	{
		m_reprojectOn = params != nullptr;
		if (params)
			m_reproject = *params;
		else
			SPT_CALL(m_ctx, spt_history_clear(m_ctx));
		m_resolvedAt = 0; // (what render() resolved was the other kind of image)
	}

	void HIPPathTracer::set_tonemap(uint32_t tonemap)
	{
		SPT_VERIFY(tonemap <= SPT_TONEMAP_ACES, "unknown tone-mapping operator");
		m_tonemap = tonemap;
		m_resolvedAt = 0; // (what render() resolved was the other kind of image)
	}

	void HIPPathTracer::set_exposure_params(const spt_exposure_params *params)
	{
		m_hasExposureParams = params != nullptr;
		if (params)
			m_exposureParams = *params;
	}

	bool HIPPathTracer::display_on() const
	{
		return m_tonemap != SPT_TONEMAP_CLAMP || (m_settingsMode && m_renderSettings->getAutoExposure());
	}

	void HIPPathTracer::resolve_display(uint32_t image, float exposure)
	{
		if (m_settingsMode && m_renderSettings->getAutoExposure())
		{
			// meter the image about to be shown; the setting's exposure is the compensation on top
			uint32_t counts[SPT_METER_BINS];
			SPT_CALL(m_ctx, spt_meter_luminance(m_ctx, image, m_frameCount, counts));
			spt_exposure_params p;
			SPT_CALL(m_ctx, spt_exposure_params_default(&p));
			if (m_hasExposureParams)
				p = m_exposureParams;
			p.target_luminance = m_renderSettings->getTargetLuminance();
			float metered = 1.0f;
			SPT_VERIFY(spt_exposure_from_histogram(counts, &p, &metered) == SPT_OK, "invalid auto-exposure parameters");
			exposure = metered * exposure;
		}
		spt_display d{};
		d.tonemap = m_tonemap;
		d.exposure = exposure;
		SPT_CALL(m_ctx, spt_resolve_display_rgba8(m_ctx, image, m_frameCount, &d, m_render_result.image_buffer.data()));
		m_resolvedAt = 0; // (the buffer no longer holds what render() resolved: auto-exposure is switched on the settings)
	}

	const PathTracer::RenderResult &HIPPathTracer::get_render_result()
	{
		SPT_VERIFY(m_frameCount > 0, "No frames rendered yet");
		const float exposure = m_settingsMode ? m_renderSettings->getExposure() : 1.0f;
		const bool display = display_on(); // auto-exposure or an operator: the metered display resolve of the same image
		if (m_reprojectOn)
		{
			// the history (if the ctx holds one) blended with the frames so far: a mean, resolved with divisor 1
			SPT_CALL(m_ctx, spt_history_blend(m_ctx, m_frameCount));
			if (m_denoiseOn)
				SPT_CALL(m_ctx, spt_denoise_blended(m_ctx, &m_denoise));
			if (display)
				resolve_display(m_denoiseOn ? SPT_IMAGE_DENOISED : SPT_IMAGE_BLENDED, exposure);
			else if (m_denoiseOn)
				SPT_CALL(m_ctx, spt_resolve_denoised_rgba8(m_ctx, exposure, m_render_result.image_buffer.data()));
			else
				SPT_CALL(m_ctx, spt_resolve_blended_rgba8(m_ctx, exposure, m_render_result.image_buffer.data()));
			return m_render_result;
		}
		if (m_denoiseOn || m_guidedOn)
		{
			// the filtered mean of the frames so far, resolved with divisor 1 (into the registered buffer): the
			// variance-guided filter once its variance is worth reading, the plain one until then
			uint32_t batches = 0;
			if (m_guidedOn)
				SPT_CALL(m_ctx, spt_noise_batches(m_ctx, &batches, nullptr));
			if (m_guidedOn && batches >= kGuidedMinBatches)
				SPT_CALL(m_ctx, spt_denoise_guided(m_ctx, m_frameCount, &m_guided));
			else
				SPT_CALL(m_ctx, spt_denoise(m_ctx, m_frameCount, m_denoiseOn ? &m_denoise : nullptr));
			if (display)
				resolve_display(SPT_IMAGE_DENOISED, exposure);
			else
				SPT_CALL(m_ctx, spt_resolve_denoised_rgba8(m_ctx, exposure, m_render_result.image_buffer.data()));
			return m_render_result;
		}
		if (display)
		{
			resolve_display(SPT_IMAGE_ACCUM, exposure);
			return m_render_result;
		}
		if (m_resolvedAt == m_frameCount && m_resolvedExposure == exposure)
			return m_render_result; // resolved by render() (spt_render_resolve_rgba8), already in host memory
		// device-side resolve: accum / frameCount, clamp, (uint8)(c * 255), rgba_to_uint32
		if (m_settingsMode)
			SPT_CALL(m_ctx, spt_resolve_rgba8_exposure(m_ctx, m_frameCount, m_renderSettings->getExposure(),
													   m_render_result.image_buffer.data()));
		else
			SPT_CALL(m_ctx, spt_resolve_rgba8(m_ctx, m_frameCount, m_render_result.image_buffer.data()));
		return m_render_result;
	}

	void HIPPathTracer::read_accumulation(std::vector<float> &out)
	{
		out.resize((size_t)m_render_result.width * m_render_result.height * 4);
		if (!out.empty())
			SPT_CALL(m_ctx, spt_read_accum(m_ctx, out.data()));
	}

	void HIPPathTracer::invalidate()
	{
		bool needs_rebuild = false;
		if (m_scene->hasChanges())
		{
			m_frameCount = 0;
			m_outputDirty = true;
			needs_rebuild = true;
		}
		bool reconfigure = false;
		if (m_modeChanged)
		{
			m_frameCount = 0;
			m_outputDirty = true;
			m_modeChanged = false;
			reconfigure = true;
		}
		if (m_renderSettings->isDirty())
		{
			m_frameCount = 0;
			m_outputDirty = true;
			m_renderSettings->clearDirty();
			reconfigure = true;
		}
		if (m_render_result.width != m_renderSettings->getWidth() || m_render_result.height != m_renderSettings->getHeight())
		{
			m_render_result.width = m_renderSettings->getWidth();
			m_render_result.height = m_renderSettings->getHeight();
			// the result buffer is page-locked and GPU-mapped: get_render_result's resolve kernel writes
			// it over PCIe directly (spt_register_host_output); re-registered whenever it reallocates
			SPT_CALL(m_ctx, spt_register_host_output(m_ctx, nullptr, 0));
			m_outputRegistered = false;
			m_render_result.image_buffer.resize((size_t)m_render_result.width * m_render_result.height);
			// (a buffer the runtime cannot register keeps the staging-and-copy resolve: same pixels)
			if (!m_render_result.image_buffer.empty())
				m_outputRegistered = spt_register_host_output(m_ctx, m_render_result.image_buffer.data(),
															  m_render_result.image_buffer.size() * sizeof(uint32_t)) == SPT_OK;
			m_frameCount = 0;
			m_outputDirty = true;
			reconfigure = true;
		}
		if (reconfigure)
		{
			spt_config cfg{};
			cfg.width = m_render_result.width;
			cfg.height = m_render_result.height;
			cfg.max_bounces = m_settingsMode ? m_renderSettings->getMaxBounces() : kReferenceBounces;
			cfg.rr_depth = m_settingsMode ? m_renderSettings->getRussianRouletteDepth() : kReferenceRRDepth;
			cfg.flags = 0;  // ::abs(int) semantics of the reference's Linux build (:320)
			cfg.shard_rank = 0;
			cfg.shard_count = 1;
			cfg.frames_in_flight = 1;  // progressive: one frame per render() call
			SPT_CALL(m_ctx, spt_configure(m_ctx, &cfg));
		}
		// temporal reprojection: what the frames so far show is kept across the move (m_frameCount is 0 here if
		// anything above changed the radiance: nothing is captured then)
		const bool reuse = m_reprojectOn && m_frameCount > 0 && (m_cameraChanged || m_lensChanged);
		if (reuse)
			SPT_CALL(m_ctx, spt_history_capture(m_ctx, m_frameCount));
		if (m_cameraChanged)
		{
			// another view: a fresh accumulation, and nothing resolved for it yet
			SPT_CALL(m_ctx, spt_set_camera(m_ctx, m_hasCamera ? &m_camera : nullptr));
			m_cameraChanged = false;
			m_frameCount = 0;
			m_resolvedAt = 0;
			m_outputDirty = true;
		}
		if (m_lensChanged)
		{
			// (after the camera: a lens needs one) other camera rays: a fresh accumulation too
			// (removing the lens of no camera is nothing to do: the ctx has none either)
			if (m_hasLens || m_hasCamera)
				SPT_CALL(m_ctx, spt_set_camera_lens(m_ctx, m_hasLens ? &m_lens : nullptr));
			m_lensChanged = false;
			m_frameCount = 0;
			m_resolvedAt = 0;
			m_outputDirty = true;
		}
		if (reuse)
			SPT_CALL(m_ctx, spt_reproject(m_ctx, &m_reproject));
		if (m_frameCount == 0)
		{
			SPT_CALL(m_ctx, spt_reset(m_ctx));
		}
		if (needs_rebuild)
		{
			rebuild_scene();
			m_scene->markChangesProcessed();
		}
		// after the rebuild: the models need a scene, and spt_set_scene resets them (spt_update_prims keeps them)
		if (m_modelsChanged || (needs_rebuild && !m_models.empty()))
		{
			SPT_CALL(m_ctx, spt_set_material_models(m_ctx, m_models.empty() ? nullptr : m_models.data(),
													(uint32_t)m_models.size()));
			m_modelsChanged = false;
			m_frameCount = 0;
			m_resolvedAt = 0;
			m_outputDirty = true;
		}
	}

	void HIPPathTracer::rebuild_scene()
	{
		// One sphere primitive per SPHERE_OBJECT node, in registry order (:362-400); one gray
		// Lambertian material (throughput *= 0.7, :260) and the reference sky (:286-292).
		std::vector<spt_prim> prims;
		for (const auto &[id, node] : m_scene->GetAllNodes())
		{
			(void)id;
			if (node->GetType() != NodeType::SPHERE_OBJECT)
				continue;
			const auto *sphere = static_cast<const SphereObject *>(node);
			// glm::vec3 under the reference's Scene.h, render::Vec3 under include/render/Scene.h
			const auto pos = sphere->GetPosition();
			spt_prim p{};
			p.type = SPT_PRIM_SPHERE;
			p.material = 0;
			p.p0[0] = pos.x;
			p.p0[1] = pos.y;
			p.p0[2] = pos.z;
			p.p0[3] = sphere->GetRadius();
			prims.push_back(p);
		}
		spt_material mat{};
		mat.albedo[0] = mat.albedo[1] = mat.albedo[2] = 0.7f;
		spt_env env{};
		env.sky_enabled = 1;
		env.horizon[0] = env.horizon[1] = env.horizon[2] = 1.0f;
		env.zenith[0] = 0.5f;
		env.zenith[1] = 0.7f;
		env.zenith[2] = 1.0f;
		// Same primitive count as the uploaded scene (spheres moved or resized):
		// replace only the changed primitives — a BVH scene is refitted, not rebuilt (spt_update_prims).
		if (m_hasUpload && prims.size() == m_uploaded.size())
		{
			std::vector<uint32_t> idx;
			std::vector<spt_prim> changed;
			for (size_t i = 0; i < prims.size(); ++i)
			{
				if (std::memcmp(&prims[i], &m_uploaded[i], sizeof(spt_prim)) != 0)
				{
					idx.push_back((uint32_t)i);
					changed.push_back(prims[i]);
				}
			}
			SPT_CALL(m_ctx, spt_update_prims(m_ctx, idx.data(), changed.data(), (uint32_t)idx.size()));
		}
		else
		{
			SPT_CALL(m_ctx, spt_set_scene(m_ctx, prims.data(), (uint32_t)prims.size(), &mat, 1, &env));
		}
		m_uploaded = std::move(prims);
		m_hasUpload = true;
	}
} // namespace render
