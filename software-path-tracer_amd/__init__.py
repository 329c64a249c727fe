"""software-path-tracer_amd — MI355X (gfx950) path-tracing integrator, Python host side.

Binds the C-ABI of ``libspt_hip.so`` (``include/spt.h``) with ctypes and mirrors the reference's
backend interface ``render::PathTracer`` (reference ``libs/render/include/render/PathTracer.h:13-51``)
so that tests and ``bench.py`` read like the reference's own call sites (``src/App.cpp:98-133``,
``src/App.cpp:230-240``). The production host side is C++ (``csrc/HIPPathTracer.cpp``); this module is
the Python plumbing around the same C-ABI.

There is no CPU fallback: if ``libspt_hip.so`` is missing or no gfx950 device is usable, the calls
raise. The CPU oracle under ``oracle/`` is test infrastructure and is never imported from here.

Import with ``importlib.import_module("software-path-tracer_amd")`` (the directory name is not a
Python identifier).
"""
from __future__ import annotations

import ctypes
import enum
import os
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPT_LIB_PATH") or os.path.join(_HERE, "libspt_hip.so")  # override: experiments only
RENDER_LIB_PATH = os.path.join(_HERE, "libspt_render.so")

# ---------------------------------------------------------------------------------------------
# C types (must match include/spt.h)
# ---------------------------------------------------------------------------------------------
SPT_OK = 0
SPT_ERR = {
    -1: "SPT_ERR_INVALID",
    -2: "SPT_ERR_HIP",
    -3: "SPT_ERR_NO_DEVICE",
    -4: "SPT_ERR_NO_SCENE",
    -5: "SPT_ERR_NOT_CONFIGURED",
    -6: "SPT_ERR_CAPACITY",
}

PRIM_SPHERE, PRIM_QUAD, PRIM_TRIANGLE = 0, 1, 2
FLAG_ABS_FLOAT = 1
FLAG_SPLIT_KERNELS = 2  # separate extend (closest hit) and shade launches per bounce
FLAG_WAVEFRONT = 4      # flat scenes: keep the wavefront schedule (no persistent k_paths launch)
FLAG_SORTED_RAYS = 1 << 3  # SPT_FLAG_SORTED_RAYS: BVH scenes, wavefront with binned (sorted) ray queues
FLAG_NEE = 1 << 4  # SPT_FLAG_NEE: next-event estimation (light sampling; superset of the reference)
SCHEDULE_SPLIT, SCHEDULE_FUSED, SCHEDULE_PERSISTENT, SCHEDULE_FRAME = 0, 1, 2, 3  # spt_stats.schedule
PERSISTENT_MIN_FRAMES = 4  # SPT_PERSISTENT_MIN_FRAMES
PROFILE_EVENTS, PROFILE_COUNTERS, PROFILE_SPAN = 1, 2, 4  # spt_set_profiling modes

SCENE_C1_SPHERE_GROUND = 0
SCENE_APP_DEFAULT = 1
SCENE_CORNELL = 2
SCENE_BUNNYLIKE = 3
SCENE_INTERIOR_1M = 4
SCENE_IDS = {
    "c1": SCENE_C1_SPHERE_GROUND,
    "app": SCENE_APP_DEFAULT,
    "cornell": SCENE_CORNELL,
    "bunnylike": SCENE_BUNNYLIKE,
    "interior1m": SCENE_INTERIOR_1M,
}

PRIM_DTYPE = np.dtype(
    [("type", "<u4"), ("material", "<u4"), ("reserved", "<u4", (2,)), ("p0", "<f4", (4,)), ("p1", "<f4", (4,)),
     ("p2", "<f4", (4,))],
    align=False,
)
MATERIAL_DTYPE = np.dtype([("albedo", "<f4", (3,)), ("emission", "<f4", (3,))])
assert PRIM_DTYPE.itemsize == 64 and MATERIAL_DTYPE.itemsize == 24
# spt_material_model: one per material (Context.set_material_models)
MATERIAL_MODEL_DTYPE = np.dtype([("kind", "<u4"), ("param", "<f4"), ("reserved", "<u4", (2,))])
assert MATERIAL_MODEL_DTYPE.itemsize == 16
MAT_DIFFUSE, MAT_METAL, MAT_DIELECTRIC = 0, 1, 2  # spt_material_kind
METER_BINS = 256  # SPT_METER_BINS
NOISE_BINS = 256  # SPT_NOISE_BINS
IMAGE_ACCUM, IMAGE_DENOISED, IMAGE_BLENDED = 0, 1, 2  # spt_image
TONEMAP_CLAMP, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2  # spt_tonemap


class SptEnv(ctypes.Structure):
    _fields_ = [("sky_enabled", ctypes.c_uint32), ("horizon", ctypes.c_float * 3), ("zenith", ctypes.c_float * 3)]


class SptConfig(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_uint32),
        ("height", ctypes.c_uint32),
        ("max_bounces", ctypes.c_uint32),
        ("rr_depth", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("shard_rank", ctypes.c_uint32),
        ("shard_count", ctypes.c_uint32),
        ("frames_in_flight", ctypes.c_uint32),
    ]


class SptCamera(ctypes.Structure):
    """spt_camera: origin, image-plane right u and up v (scaled by tan(vfov / 2)), forward w; 64 bytes."""
    _fields_ = [
        ("origin", ctypes.c_float * 3),
        ("u", ctypes.c_float * 3),
        ("v", ctypes.c_float * 3),
        ("w", ctypes.c_float * 3),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 3),
    ]


class SptLens(ctypes.Structure):
    """spt_lens: the aperture's radius (world units) and the focus distance of a camera's thin lens; 16 bytes."""
    _fields_ = [
        ("radius", ctypes.c_float),
        ("focus_distance", ctypes.c_float),
        ("reserved", ctypes.c_uint32 * 2),
    ]


CAMERA_JITTER = 1  # SPT_CAMERA_JITTER
SPT_MAX_BOUNCES = 32


class SptStats(ctypes.Structure):
    _fields_ = [
        ("frames", ctypes.c_uint64),
        ("paths", ctypes.c_uint64),
        ("segments", ctypes.c_uint64 * SPT_MAX_BOUNCES),
        ("segments_total", ctypes.c_uint64),
        ("passes", ctypes.c_uint64),
        ("extend_launches", ctypes.c_uint64),
        ("extend_ms", ctypes.c_double),
        ("extend_segments", ctypes.c_uint64),
        ("shade_launches", ctypes.c_uint64),
        ("shade_ms", ctypes.c_double),
        ("other_ms", ctypes.c_double),
        ("extend_ms_bounce", ctypes.c_double * SPT_MAX_BOUNCES),
        ("shade_ms_bounce", ctypes.c_double * SPT_MAX_BOUNCES),
        ("bvh_nodes", ctypes.c_uint64),
        ("scene_bytes", ctypes.c_uint64),
        ("radiance_updates", ctypes.c_uint64 * SPT_MAX_BOUNCES),
        ("tail_ms", ctypes.c_double),
        ("tail_launches", ctypes.c_uint64),
        ("tail_bounce", ctypes.c_uint64),
        ("fused", ctypes.c_uint64),
        ("persistent_ms", ctypes.c_double),
        ("persistent_launches", ctypes.c_uint64),
        ("schedule", ctypes.c_uint64),
        ("lane_slots", ctypes.c_uint64),
        ("lane_busy", ctypes.c_uint64),
        ("bvh_node_visits", ctypes.c_uint64),
        ("prim_tests", ctypes.c_uint64),
        ("flat_fast_path", ctypes.c_uint64),
        ("specialized", ctypes.c_uint64),
        ("shadow_rays", ctypes.c_uint64),
        ("emitters", ctypes.c_uint64),
        ("stack_bytes", ctypes.c_uint64),
        ("stack_need", ctypes.c_uint64),
        ("stalled_waves", ctypes.c_uint64),
        ("view_cached", ctypes.c_uint64),
        ("view_live_pixels", ctypes.c_uint64),
        ("flat_pairs", ctypes.c_uint64),
        ("flat_pair_second_passes", ctypes.c_uint64),
        ("view_split", ctypes.c_uint64),
        ("flat_sphere_second_passes", ctypes.c_uint64),
    ]
    # spt_get_view_wide's answer, set by Context.stats(): 1 when the last k_paths launch ran the wide form
    # (a query of its own: spt_stats keeps its size)
    view_wide = 0
    # spt_get_flat_ranges' answer, likewise: 1 when the last k_paths launch ran with the scene's range bit in force
    flat_ranges = 0

    def as_dict(self) -> dict:
        d = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            d[k] = list(v) if isinstance(v, ctypes.Array) else v
        d["view_wide"] = self.view_wide
        d["flat_ranges"] = self.flat_ranges
        return d


# Every symbol include/spt.h declares (checked by tests/test_capi_symbols.py).
EXPORTED_SYMBOLS = (
    "spt_abi_version", "spt_device_count", "spt_create", "spt_destroy", "spt_last_error", "spt_set_stream",
    "spt_set_scene", "spt_configure", "spt_reset", "spt_get_frame_count", "spt_render", "spt_synchronize",
    "spt_shard_pixels", "spt_read_accum", "spt_accum_device_ptr", "spt_copy_accum_device", "spt_resolve_rgba8",
    "spt_resolve_rgba8_exposure", "spt_register_host_output", "spt_render_resolve_rgba8", "spt_assemble_rows",
    "spt_set_profiling", "spt_get_stats", "spt_get_view_wide", "spt_get_flat_ranges", "spt_stats_clear", "spt_build_scene",
    "spt_set_env_map", "spt_env_octa_from_equirect",
    "spt_comm_available", "spt_comm_unique_id", "spt_comm_init", "spt_gather_image", "spt_gather_image_overlapped", "spt_gather_wait",
    "spt_comm_destroy", "spt_set_tuning",
    "spt_specialize_scene", "spt_compile_flat_kernels", "spt_update_prims",
    "spt_set_camera", "spt_camera_look_at", "spt_camera_ray",
    "spt_set_camera_lens", "spt_camera_lens_ray", "spt_camera_focus_at_hit",
    "spt_set_material_models", "spt_bsdf_sample",
    "spt_render_features", "spt_read_features", "spt_features_device_ptr",
    "spt_denoise_params_default", "spt_denoise", "spt_set_denoise_form", "spt_read_denoised", "spt_denoised_device_ptr",
    "spt_resolve_denoised_rgba8", "spt_atrous_host",
    "spt_guided_params_default", "spt_denoise_guided", "spt_read_denoised_variance", "spt_atrous_guided_host",
    "spt_reproject_params_default", "spt_history_capture", "spt_reproject", "spt_history_clear", "spt_read_history",
    "spt_history_device_ptr", "spt_history_blend", "spt_read_blended", "spt_blended_device_ptr",
    "spt_resolve_blended_rgba8", "spt_denoise_blended", "spt_set_history_layout", "spt_reproject_basis",
    "spt_reproject_host",
    "spt_exposure_params_default", "spt_meter_luminance", "spt_meter_device_image", "spt_resolve_display_rgba8",
    "spt_resolve_display_device_image", "spt_set_meter_form", "spt_meter_bin", "spt_luminance_histogram_host",
    "spt_exposure_from_histogram", "spt_display_host",
    "spt_noise_params_default", "spt_noise_update", "spt_noise_batches", "spt_noise_meter", "spt_read_noise_moments",
    "spt_read_noise", "spt_noise_device_ptr", "spt_noise_meter_device_image",
    "spt_noise_update_host", "spt_noise_meter_host", "spt_noise_from_histogram",
)
COMM_ID_BYTES = 128  # SPT_COMM_ID_BYTES


class SptTuning(ctypes.Structure):
    """spt_tuning: schedule knobs for measurement and tests (0 / -1 = automatic; results never change)."""
    _fields_ = [
        ("fused", ctypes.c_int32),
        ("tail_bounce", ctypes.c_uint32),
        ("persistent", ctypes.c_int32),
        ("frame_kernel", ctypes.c_int32),
        ("chunks_per_wave", ctypes.c_uint32),
        ("px_shift", ctypes.c_uint32),
        ("subqueues", ctypes.c_uint32),
        ("bvh_max_leaf", ctypes.c_uint32),
        ("bvh_bins", ctypes.c_uint32),
        ("specialize", ctypes.c_int32),
        ("view_cache", ctypes.c_int32),
        ("split_streams", ctypes.c_int32),
        ("wide_chunks", ctypes.c_int32),
    ]

    def __init__(self, **kw):
        super().__init__(fused=-1, persistent=-1, frame_kernel=-1)
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"unknown spt_tuning field {k}")
            setattr(self, k, v)


class DenoiseParams(ctypes.Structure):
    """spt_denoise_params (32 bytes): the a-trous filter's levels (1..6), colour and plane-distance widths
    (> 0) and the normal weight's exponent as log2 (0..7). DenoiseParams() holds the library's defaults
    (spt_denoise_params_default); keyword arguments replace single fields."""
    _fields_ = [
        ("levels", ctypes.c_uint32),
        ("sigma_color", ctypes.c_float),
        ("sigma_plane", ctypes.c_float),
        ("normal_power_log2", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 4),
    ]

    def __init__(self, **kw):
        super().__init__()
        rc = load_library().spt_denoise_params_default(ctypes.byref(self))
        if rc != SPT_OK:
            raise SptError(f"spt_denoise_params_default -> {SPT_ERR.get(rc, rc)}")
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"unknown spt_denoise_params field {k}")
            setattr(self, k, v)


class GuidedParams(ctypes.Structure):
    """spt_guided_params (32 bytes): the variance-guided a-trous filter's levels (1..6), the colour weight's width
    in standard deviations of a pixel's mean luminance (> 0), the plane-distance width (> 0), the normal weight's
    exponent as log2 (0..7), the variance added under the colour weight's divisor (> 0) and whether the variance
    goes through the 3 x 3 prefilter (0 or 1). GuidedParams() holds the library's defaults
    (spt_guided_params_default); keyword arguments replace single fields."""
    _fields_ = [
        ("levels", ctypes.c_uint32),
        ("sigma_variance", ctypes.c_float),
        ("sigma_plane", ctypes.c_float),
        ("normal_power_log2", ctypes.c_uint32),
        ("variance_floor", ctypes.c_float),
        ("prefilter", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 2),
    ]

    def __init__(self, **kw):
        super().__init__()
        rc = load_library().spt_guided_params_default(ctypes.byref(self))
        if rc != SPT_OK:
            raise SptError(f"spt_guided_params_default -> {SPT_ERR.get(rc, rc)}")
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"unknown spt_guided_params field {k}")
            setattr(self, k, v)


class ReprojectParams(ctypes.Structure):
    """spt_reproject_params (32 bytes): the most frames a reprojected history counts for (>= 1), the least
    cosine between the two views' normals, the plane distance allowed as a share of the hit distance (>= 0)
    and the least sum of valid taps' weights (> 0). ReprojectParams() holds the library's defaults
    (spt_reproject_params_default); keyword arguments replace single fields."""
    _fields_ = [
        ("max_history", ctypes.c_float),
        ("normal_min", ctypes.c_float),
        ("plane_tolerance", ctypes.c_float),
        ("min_weight", ctypes.c_float),
        ("reserved", ctypes.c_uint32 * 4),
    ]

    def __init__(self, **kw):
        super().__init__()
        rc = load_library().spt_reproject_params_default(ctypes.byref(self))
        if rc != SPT_OK:
            raise SptError(f"spt_reproject_params_default -> {SPT_ERR.get(rc, rc)}")
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"unknown spt_reproject_params field {k}")
            setattr(self, k, v)


class ExposureParams(ctypes.Structure):
    """spt_exposure_params (32 bytes): the luminance the histogram's trimmed log-average is brought to (> 0), the
    shares of non-black pixels left out at the dark and the bright end (>= 0, below 1 in sum) and the limits of
    the result (> 0). ExposureParams() holds the library's defaults (spt_exposure_params_default); keyword
    arguments replace single fields."""
    _fields_ = [
        ("target_luminance", ctypes.c_float),
        ("low_fraction", ctypes.c_float),
        ("high_fraction", ctypes.c_float),
        ("min_exposure", ctypes.c_float),
        ("max_exposure", ctypes.c_float),
        ("reserved", ctypes.c_uint32 * 3),
    ]

    def __init__(self, **kw):
        super().__init__()
        rc = load_library().spt_exposure_params_default(ctypes.byref(self))
        if rc != SPT_OK:
            raise SptError(f"spt_exposure_params_default -> {SPT_ERR.get(rc, rc)}")
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"unknown spt_exposure_params field {k}")
            setattr(self, k, v)


class Display(ctypes.Structure):
    """spt_display (16 bytes): the tone-mapping operator (TONEMAP_CLAMP, the default: the plain resolve's clamp;
    TONEMAP_REINHARD; TONEMAP_ACES) and the exposure (finite, >= 0; default 1)."""
    _fields_ = [
        ("tonemap", ctypes.c_uint32),
        ("exposure", ctypes.c_float),
        ("reserved", ctypes.c_uint32 * 2),
    ]

    def __init__(self, tonemap: int = TONEMAP_CLAMP, exposure: float = 1.0):
        super().__init__(tonemap=tonemap, exposure=exposure)


class NoiseParams(ctypes.Structure):
    """spt_noise_params (16 bytes): the pooling radius of the noise meter (0, 1 or 2) and the luminance added to
    a pixel's mean before the error is taken relative to it (finite, >= 0). NoiseParams() holds the library's
    defaults (spt_noise_params_default); keyword arguments replace single fields."""
    _fields_ = [
        ("radius", ctypes.c_uint32),
        ("dark_floor", ctypes.c_float),
        ("reserved", ctypes.c_uint32 * 2),
    ]

    def __init__(self, **kw):
        super().__init__()
        rc = load_library().spt_noise_params_default(ctypes.byref(self))
        if rc != SPT_OK:
            raise SptError(f"spt_noise_params_default -> {SPT_ERR.get(rc, rc)}")
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"unknown spt_noise_params field {k}")
            setattr(self, k, v)


_lib: Optional[ctypes.CDLL] = None


class SptError(RuntimeError):
    pass


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libspt_hip.so. Raises loudly if it is missing — there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise SptError(f"libspt_hip.so not built at {path} (run `make` or __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    P, U32, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    sig = {
        "spt_abi_version": ([], I),
        "spt_device_count": ([ctypes.POINTER(I)], I),
        "spt_create": ([ctypes.POINTER(P), I], I),
        "spt_destroy": ([P], None),
        "spt_last_error": ([P], ctypes.c_char_p),
        "spt_set_stream": ([P, P], I),
        "spt_set_scene": ([P, P, U32, P, U32, ctypes.POINTER(SptEnv)], I),
        "spt_configure": ([P, ctypes.POINTER(SptConfig)], I),
        "spt_reset": ([P], I),
        "spt_get_frame_count": ([P, ctypes.POINTER(U32)], I),
        "spt_render": ([P, U32, U32], I),
        "spt_synchronize": ([P], I),
        "spt_shard_pixels": ([P, ctypes.POINTER(ctypes.c_uint64)], I),
        "spt_read_accum": ([P, P], I),
        "spt_accum_device_ptr": ([P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)], I),
        "spt_copy_accum_device": ([P, P], I),
        "spt_resolve_rgba8": ([P, U32, P], I),
        "spt_resolve_rgba8_exposure": ([P, U32, ctypes.c_float, P], I),
        "spt_register_host_output": ([P, P, ctypes.c_size_t], I),
        "spt_render_resolve_rgba8": ([P, U32, U32, U32, ctypes.c_float, P], I),
        "spt_assemble_rows": ([P, P, P], I),
        "spt_set_profiling": ([P, I], I),
        "spt_set_env_map": ([P, P, U32, U32], I),
        "spt_env_octa_from_equirect": ([P, U32, U32, P, U32, U32], I),
        "spt_get_stats": ([P, ctypes.POINTER(SptStats)], I),
        "spt_get_view_wide": ([P, ctypes.POINTER(ctypes.c_uint64)], I),
        "spt_get_flat_ranges": ([P, ctypes.POINTER(ctypes.c_uint64)], I),
        "spt_stats_clear": ([P], I),
        "spt_build_scene": ([U32, P, ctypes.POINTER(U32), P, ctypes.POINTER(U32), ctypes.POINTER(SptEnv)], I),
        "spt_comm_available": ([], I),
        "spt_comm_unique_id": ([P], I),
        "spt_comm_init": ([P, P, I, I], I),
        "spt_gather_image": ([P, P], I),
        "spt_gather_image_overlapped": ([P, P], I),
        "spt_gather_wait": ([P], I),
        "spt_comm_destroy": ([P], I),
        "spt_set_tuning": ([P, ctypes.POINTER(SptTuning)], I),
        "spt_specialize_scene": ([P], I),
        "spt_update_prims": ([P, P, P, U32], I),
        "spt_compile_flat_kernels": ([P, U32, I, ctypes.c_char_p, ctypes.c_size_t], I),
        "spt_set_camera": ([P, ctypes.POINTER(SptCamera)], I),
        "spt_camera_look_at": ([ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                ctypes.POINTER(ctypes.c_float), ctypes.c_float, ctypes.POINTER(SptCamera)], I),
        "spt_camera_ray": ([ctypes.POINTER(SptCamera), U32, U32, U32, U32, ctypes.c_float, ctypes.c_float,
                            ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)], I),
        "spt_set_camera_lens": ([P, ctypes.POINTER(SptLens)], I),
        "spt_camera_lens_ray": ([ctypes.POINTER(SptCamera), ctypes.POINTER(SptLens), U32, U32, U32, U32,
                                 ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                 ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)], I),
        "spt_camera_focus_at_hit": ([ctypes.POINTER(SptCamera), U32, U32, U32, U32, ctypes.c_float, ctypes.c_float,
                                     ctypes.c_float, ctypes.POINTER(ctypes.c_float)], I),
        "spt_set_material_models": ([P, P, U32], I),
        "spt_bsdf_sample": ([P, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), I, U32,
                             ctypes.POINTER(U32), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(I),
                             ctypes.POINTER(I)], I),
        "spt_render_features": ([P], I),
        "spt_read_features": ([P, P, P, P], I),
        "spt_features_device_ptr": ([P, ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(P),
                                     ctypes.POINTER(ctypes.c_size_t)], I),
        "spt_denoise_params_default": ([ctypes.POINTER(DenoiseParams)], I),
        "spt_denoise": ([P, U32, ctypes.POINTER(DenoiseParams)], I),
        "spt_set_denoise_form": ([P, I], I),
        "spt_read_denoised": ([P, P], I),
        "spt_denoised_device_ptr": ([P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)], I),
        "spt_resolve_denoised_rgba8": ([P, ctypes.c_float, P], I),
        "spt_atrous_host": ([P, P, P, U32, U32, ctypes.POINTER(DenoiseParams), P], I),
        "spt_guided_params_default": ([ctypes.POINTER(GuidedParams)], I),
        "spt_denoise_guided": ([P, U32, ctypes.POINTER(GuidedParams)], I),
        "spt_read_denoised_variance": ([P, P], I),
        "spt_atrous_guided_host": ([P, P, P, P, U32, U32, U32, U32, ctypes.POINTER(GuidedParams), P, P], I),
        "spt_reproject_params_default": ([ctypes.POINTER(ReprojectParams)], I),
        "spt_history_capture": ([P, U32], I),
        "spt_reproject": ([P, ctypes.POINTER(ReprojectParams)], I),
        "spt_history_clear": ([P], I),
        "spt_read_history": ([P, P], I),
        "spt_history_device_ptr": ([P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)], I),
        "spt_history_blend": ([P, U32], I),
        "spt_read_blended": ([P, P], I),
        "spt_blended_device_ptr": ([P, ctypes.POINTER(P), ctypes.POINTER(ctypes.c_size_t)], I),
        "spt_resolve_blended_rgba8": ([P, ctypes.c_float, P], I),
        "spt_denoise_blended": ([P, ctypes.POINTER(DenoiseParams)], I),
        "spt_set_history_layout": ([P, I], I),
        "spt_reproject_basis": ([ctypes.POINTER(SptCamera), P, P, ctypes.POINTER(ctypes.c_float)], I),
        "spt_reproject_host": ([ctypes.POINTER(ReprojectParams), ctypes.POINTER(SptCamera), U32, U32, P, P, P, P, P, P,
                                U32, P], I),
        "spt_exposure_params_default": ([ctypes.POINTER(ExposureParams)], I),
        "spt_meter_luminance": ([P, U32, U32, P], I),
        "spt_meter_device_image": ([P, P, ctypes.c_uint64, ctypes.c_float, P], I),
        "spt_resolve_display_rgba8": ([P, U32, U32, ctypes.POINTER(Display), P], I),
        "spt_resolve_display_device_image": ([P, P, ctypes.c_uint64, ctypes.c_float, ctypes.POINTER(Display), P], I),
        "spt_set_meter_form": ([P, I], I),
        "spt_meter_bin": ([ctypes.c_float, ctypes.POINTER(U32)], I),
        "spt_luminance_histogram_host": ([P, ctypes.c_uint64, ctypes.c_float, P], I),
        "spt_exposure_from_histogram": ([P, ctypes.POINTER(ExposureParams), ctypes.POINTER(ctypes.c_float)], I),
        "spt_display_host": ([P, ctypes.c_uint64, ctypes.c_float, ctypes.POINTER(Display), P], I),
        "spt_noise_params_default": ([ctypes.POINTER(NoiseParams)], I),
        "spt_noise_update": ([P, U32], I),
        "spt_noise_batches": ([P, ctypes.POINTER(U32), ctypes.POINTER(U32)], I),
        "spt_noise_meter": ([P, ctypes.POINTER(NoiseParams), P], I),
        "spt_read_noise_moments": ([P, P], I),
        "spt_read_noise": ([P, P], I),
        "spt_noise_device_ptr": ([P, ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(ctypes.c_uint64)], I),
        "spt_noise_meter_device_image": ([P, P, U32, U32, U32, ctypes.c_float, ctypes.POINTER(NoiseParams), P, P], I),
        "spt_noise_update_host": ([P, ctypes.c_uint64, ctypes.c_float, ctypes.c_float, P], I),
        "spt_noise_meter_host": ([P, U32, U32, U32, ctypes.c_float, ctypes.POINTER(NoiseParams), P, P], I),
        "spt_noise_from_histogram": ([P, ctypes.c_double, ctypes.POINTER(ctypes.c_double)], I),
    }
    for name, (args, res) in sig.items():
        if os.environ.get("SPT_LIB_PATH") and not hasattr(lib, name):
            continue  # an experiment library built from an older source (A/B runs only)
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def _ptr(a: np.ndarray) -> ctypes.c_void_p:
    return ctypes.c_void_p(a.ctypes.data) if a.size else ctypes.c_void_p(0)


def reference_env(sky: bool = True) -> SptEnv:
    """Reference sky gradient (CPUPathTracer.cpp:286-292)."""
    e = SptEnv()
    e.sky_enabled = 1 if sky else 0
    e.horizon[:] = (1.0, 1.0, 1.0)
    e.zenith[:] = (0.5, 0.7, 1.0)
    return e


def env_octa_from_equirect(equirect_rgb: np.ndarray, width: int, height: int) -> np.ndarray:
    """Resample an equirectangular (h, w, 3) float image into a (height, width, 4) octahedral map
    (spt_env_octa_from_equirect; host-only)."""
    src = np.ascontiguousarray(equirect_rgb, dtype=np.float32)
    dst = np.zeros((height, width, 4), dtype=np.float32)
    rc = load_library().spt_env_octa_from_equirect(src.ctypes.data, src.shape[1], src.shape[0], dst.ctypes.data,
                                                   width, height)
    if rc != 0:
        raise SptError(f"spt_env_octa_from_equirect: {rc}")
    return dst


def synthetic_env_map(size: int = 512, seed: int = 0x5eed) -> np.ndarray:
    """A deterministic HDR sky for tests and the bench (no image files offline): an equirectangular
    gradient with a bright sun disk and seeded noise, resampled to a size x size octahedral map."""
    h, w = size // 2, size
    theta = (np.arange(h, dtype=np.float64) + 0.5) / h * np.pi
    phi = (np.arange(w, dtype=np.float64) + 0.5) / w * 2 * np.pi - np.pi
    th, ph = np.meshgrid(theta, phi, indexing="ij")
    y = np.cos(th)
    base = np.stack([0.6 + 0.4 * y, 0.7 + 0.3 * y, 1.0 + 0.2 * y], axis=-1)
    sun = np.exp(-((th - 0.6) ** 2 + (ph - 0.8) ** 2) / 0.002)[..., None] * np.array([40.0, 36.0, 30.0])
    ground = (y < 0)[..., None] * np.array([-0.3, -0.35, -0.5])
    noise = np.random.default_rng(seed).uniform(0.0, 0.05, size=(h, w, 1))
    equirect = np.maximum(base + sun + ground + noise, 0.0).astype(np.float32)
    return env_octa_from_equirect(equirect, size, size)


def look_at(eye, target, up=(0.0, 1.0, 0.0), vfov: float = 90.0, jitter: bool = False) -> SptCamera:
    """spt_camera_look_at (host only): the camera at `eye` looking at `target` with a vertical field of
    view of `vfov` degrees; jitter sets SPT_CAMERA_JITTER (a uniform point of the pixel per sample)."""
    f3 = ctypes.c_float * 3
    cam = SptCamera()
    rc = load_library().spt_camera_look_at(f3(*eye), f3(*target), f3(*up), float(vfov), ctypes.byref(cam))
    if rc != SPT_OK:
        raise SptError(f"spt_camera_look_at -> {SPT_ERR.get(rc, rc)}")
    if jitter:
        cam.flags |= CAMERA_JITTER
    return cam


def camera_ray(cam: SptCamera, width: int, height: int, x: int, y: int, jx: float = 0.0, jy: float = 0.0):
    """spt_camera_ray (host only): origin and direction (two float32 arrays of 3) of pixel (x, y) with
    jitter (jx, jy), from the function the kernels compile: the same bits."""
    o = np.zeros(3, dtype=np.float32)
    d = np.zeros(3, dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = load_library().spt_camera_ray(ctypes.byref(cam), width, height, x, y, float(jx), float(jy),
                                       o.ctypes.data_as(fp), d.ctypes.data_as(fp))
    if rc != SPT_OK:
        raise SptError(f"spt_camera_ray -> {SPT_ERR.get(rc, rc)}")
    return o, d


def _lens(lens, focus_distance=None) -> SptLens:
    """An SptLens from one, or from (radius, focus_distance)."""
    if isinstance(lens, SptLens):
        return lens
    out = SptLens()
    out.radius, out.focus_distance = float(lens), float(focus_distance)
    return out


def camera_lens_ray(cam: SptCamera, lens, width: int, height: int, x: int, y: int, jx: float = 0.0, jy: float = 0.0,
                    u1: float = 0.0, u2: float = 0.0):
    """spt_camera_lens_ray (host only): origin and direction (two float32 arrays of 3) of the ray of pixel
    (x, y) with jitter (jx, jy) from the point (u1, u2) of the aperture of `lens` (an SptLens or a
    (radius, focus_distance) pair), from the function the kernels compile: the same bits."""
    l = lens if isinstance(lens, SptLens) else _lens(*lens)
    o = np.zeros(3, dtype=np.float32)
    d = np.zeros(3, dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = load_library().spt_camera_lens_ray(ctypes.byref(cam), ctypes.byref(l), width, height, x, y, float(jx),
                                            float(jy), float(u1), float(u2), o.ctypes.data_as(fp),
                                            d.ctypes.data_as(fp))
    if rc != SPT_OK:
        raise SptError(f"spt_camera_lens_ray -> {SPT_ERR.get(rc, rc)}")
    return o, d


def camera_focus_at_hit(cam: SptCamera, width: int, height: int, x: int, y: int, t: float, jx: float = 0.0,
                        jy: float = 0.0) -> float:
    """spt_camera_focus_at_hit (host only): the focus distance that puts the point at distance t along the
    camera ray of pixel (x, y) with jitter (jx, jy) in focus."""
    f = ctypes.c_float()
    rc = load_library().spt_camera_focus_at_hit(ctypes.byref(cam), width, height, x, y, float(jx), float(jy),
                                                float(t), ctypes.byref(f))
    if rc != SPT_OK:
        raise SptError(f"spt_camera_focus_at_hit -> {SPT_ERR.get(rc, rc)}")
    return f.value


def material_models(models) -> np.ndarray:
    """A MATERIAL_MODEL_DTYPE array from (kind, param) pairs (or such an array itself)."""
    if isinstance(models, np.ndarray) and models.dtype == MATERIAL_MODEL_DTYPE:
        return np.ascontiguousarray(models)
    out = np.zeros(len(models), dtype=MATERIAL_MODEL_DTYPE)
    for i, (kind, param) in enumerate(models):
        out[i]["kind"], out[i]["param"] = kind, param
    return out


def bsdf_sample(kind: int, param: float, d, n, entering: bool, state: int, flags: int = 0):
    """spt_bsdf_sample (host only): the scattering step the kernels compile, the same bits. d: the incoming
    direction, n: the surface's outward unit normal (nf = n if entering else -n), state: the RNG state.
    Returns (direction float32[3], transmitted, absorbed, state after the model's draws)."""
    m = material_models([(kind, param)])
    f3 = ctypes.c_float * 3
    out = np.zeros(3, dtype=np.float32)
    st, tr, ab = ctypes.c_uint32(state), ctypes.c_int(0), ctypes.c_int(0)
    rc = load_library().spt_bsdf_sample(m.ctypes.data, f3(*d), f3(*n), int(bool(entering)), flags, ctypes.byref(st),
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(tr),
                                        ctypes.byref(ab))
    if rc != SPT_OK:
        raise SptError(f"spt_bsdf_sample -> {SPT_ERR.get(rc, rc)}")
    return out, bool(tr.value), bool(ab.value), st.value


def atrous_host(rgba: np.ndarray, feat_a: np.ndarray, feat_b: np.ndarray,
                params: Optional[DenoiseParams] = None) -> np.ndarray:
    """spt_atrous_host (host only): the denoiser's filter on (h, w, 4) float32 arrays — the mean colour and
    the two feature images — by the function the kernels compile: the same bits as Context.denoise."""
    c = np.ascontiguousarray(rgba, dtype=np.float32)
    a = np.ascontiguousarray(feat_a, dtype=np.float32)
    b = np.ascontiguousarray(feat_b, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 4 or a.shape != c.shape or b.shape != c.shape:
        raise ValueError("atrous_host: rgba, feat_a and feat_b must be (height, width, 4) arrays of one shape")
    out = np.zeros_like(c)
    rc = load_library().spt_atrous_host(_ptr(c), _ptr(a), _ptr(b), c.shape[1], c.shape[0],
                                        ctypes.byref(params) if params is not None else None, _ptr(out))
    if rc != SPT_OK:
        raise SptError(f"spt_atrous_host -> {SPT_ERR.get(rc, rc)}")
    return out


def atrous_guided_host(rgba: np.ndarray, moments: np.ndarray, feat_a: np.ndarray, feat_b: np.ndarray, batches: int,
                       frame_count: int, params: Optional[GuidedParams] = None) -> Tuple[np.ndarray, np.ndarray]:
    """spt_atrous_guided_host (host only): (colour (h, w, 4), variance (h, w)) of the variance-guided filter on
    (h, w, 4) float32 arrays — the mean colour, the noise moments after `batches` batches and the two feature
    images — by the functions the kernels compile: the same bits as Context.denoise_guided."""
    c = np.ascontiguousarray(rgba, dtype=np.float32)
    m = np.ascontiguousarray(moments, dtype=np.float32)
    a = np.ascontiguousarray(feat_a, dtype=np.float32)
    b = np.ascontiguousarray(feat_b, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 4 or m.shape != c.shape or a.shape != c.shape or b.shape != c.shape:
        raise ValueError("atrous_guided_host: rgba, moments, feat_a and feat_b must be (height, width, 4) arrays of one shape")
    out, var = np.zeros_like(c), np.zeros(c.shape[:2], dtype=np.float32)
    rc = load_library().spt_atrous_guided_host(_ptr(c), _ptr(m), _ptr(a), _ptr(b), c.shape[1], c.shape[0], batches,
                                               frame_count, ctypes.byref(params) if params is not None else None,
                                               _ptr(out), _ptr(var))
    if rc != SPT_OK:
        raise SptError(f"spt_atrous_guided_host -> {SPT_ERR.get(rc, rc)}")
    return out, var


def reproject_basis(cam: Optional[SptCamera]):
    """spt_reproject_basis (host only): (rows (3, 3) = ru, rv, rw; origin (3,); j') of a captured view's camera as
    the reprojection reads it; None: the reference's camera."""
    rows, origin, j = np.zeros((3, 3), dtype=np.float32), np.zeros(3, dtype=np.float32), ctypes.c_float(0.0)
    rc = load_library().spt_reproject_basis(ctypes.byref(cam) if cam is not None else None, _ptr(rows), _ptr(origin),
                                            ctypes.byref(j))
    if rc != SPT_OK:
        raise SptError(f"spt_reproject_basis -> {SPT_ERR.get(rc, rc)}")
    return rows, origin, float(j.value)


def reproject_host(prev_cam: Optional[SptCamera], cur_a: np.ndarray, cur_b: np.ndarray, hist_rgba: np.ndarray,
                   hist_a: np.ndarray, hist_b: np.ndarray, params: Optional[ReprojectParams] = None,
                   material_reusable=None) -> np.ndarray:
    """spt_reproject_host (host only): the captured view (hist_rgba: mean radiance and length; hist_a / hist_b: its
    features; prev_cam: its camera, None for the reference's) mapped into the view whose features are cur_a /
    cur_b, all (h, w, 4) float32, by the function the kernels compile: the same bits as Context.reproject.
    material_reusable: one entry per material, 0 / False for a METAL or DIELECTRIC one; None: all reusable."""
    arrs = [np.ascontiguousarray(x, dtype=np.float32) for x in (cur_a, cur_b, hist_rgba, hist_a, hist_b)]
    if arrs[0].ndim != 3 or arrs[0].shape[2] != 4 or any(x.shape != arrs[0].shape for x in arrs):
        raise ValueError("reproject_host: the five images must be (height, width, 4) arrays of one shape")
    table = None if material_reusable is None else np.ascontiguousarray(material_reusable, dtype=np.uint32)
    out = np.empty_like(arrs[0])
    rc = load_library().spt_reproject_host(ctypes.byref(params) if params is not None else None,
                                           ctypes.byref(prev_cam) if prev_cam is not None else None,
                                           arrs[0].shape[1], arrs[0].shape[0], *[_ptr(x) for x in arrs],
                                           ctypes.c_void_p(table.ctypes.data) if table is not None else None,
                                           0 if table is None else table.size, _ptr(out))
    if rc != SPT_OK:
        raise SptError(f"spt_reproject_host -> {SPT_ERR.get(rc, rc)}")
    return out


def _pixels(rgba: np.ndarray, who: str) -> np.ndarray:
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    if a.ndim < 1 or a.shape[-1] != 4:
        raise ValueError(f"{who}: rgba must be an array of float RGBA pixels (last axis 4)")
    return a


def meter_bin(luminance) -> int:
    """spt_meter_bin (host only): the histogram bin of one luminance value, by the function the kernel compiles."""
    b = ctypes.c_uint32(0)
    rc = load_library().spt_meter_bin(ctypes.c_float(luminance), ctypes.byref(b))
    if rc != SPT_OK:
        raise SptError(f"spt_meter_bin -> {SPT_ERR.get(rc, rc)}")
    return int(b.value)


def luminance_histogram_host(rgba: np.ndarray, divisor: float = 1.0) -> np.ndarray:
    """spt_luminance_histogram_host (host only): the METER_BINS counts of rgba / divisor (float RGBA pixels, any
    leading shape), by the functions the kernel compiles: the same counts as Context.meter_luminance."""
    a = _pixels(rgba, "luminance_histogram_host")
    counts = np.zeros(METER_BINS, dtype=np.uint32)
    rc = load_library().spt_luminance_histogram_host(_ptr(a), a.size // 4, divisor, _ptr(counts))
    if rc != SPT_OK:
        raise SptError(f"spt_luminance_histogram_host -> {SPT_ERR.get(rc, rc)}")
    return counts


def exposure_from_histogram(counts: np.ndarray, params: Optional[ExposureParams] = None) -> float:
    """spt_exposure_from_histogram (host only): the exposure that brings the trimmed log-average luminance of a
    histogram (METER_BINS counts; shards' counts added up) to params.target_luminance; 1.0 for an all-black one."""
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    if c.shape != (METER_BINS,):
        raise ValueError("exposure_from_histogram: counts must hold METER_BINS values")
    e = ctypes.c_float(0.0)
    rc = load_library().spt_exposure_from_histogram(_ptr(c), ctypes.byref(params) if params is not None else None,
                                                    ctypes.byref(e))
    if rc != SPT_OK:
        raise SptError(f"spt_exposure_from_histogram -> {SPT_ERR.get(rc, rc)}")
    return float(e.value)


def display_host(rgba: np.ndarray, display: Display, divisor: float = 1.0) -> np.ndarray:
    """spt_display_host (host only): rgba / divisor through the display transform as RGBA8 (uint32, R in the high
    byte; the shape of rgba without its last axis), by the function the kernel compiles: the same bytes as
    Context.resolve_display_rgba8."""
    a = _pixels(rgba, "display_host")
    out = np.zeros(a.shape[:-1], dtype=np.uint32)
    rc = load_library().spt_display_host(_ptr(a), a.size // 4, divisor, ctypes.byref(display), _ptr(out))
    if rc != SPT_OK:
        raise SptError(f"spt_display_host -> {SPT_ERR.get(rc, rc)}")
    return out


def noise_update_host(accum: np.ndarray, batch_frames: float, frames_before: float = 0.0,
                      moments: Optional[np.ndarray] = None) -> np.ndarray:
    """spt_noise_update_host (host only): the moments (the shape of accum) after folding one batch of batch_frames
    frames into `moments`, which held frames_before frames (None with frames_before 0: the first batch); accum is
    the accumulation after the batch. By the function the kernel compiles: the same bits as Context.noise_update."""
    a = _pixels(accum, "noise_update_host")
    if moments is None:
        if frames_before != 0:
            raise ValueError("noise_update_host: moments are needed once frames were folded")
        m = np.zeros_like(a)
    else:
        m = np.array(moments, dtype=np.float32, order="C")
        if m.shape != a.shape:
            raise ValueError("noise_update_host: moments and accum differ in shape")
    rc = load_library().spt_noise_update_host(_ptr(a), a.size // 4, batch_frames, frames_before, _ptr(m))
    if rc != SPT_OK:
        raise SptError(f"spt_noise_update_host -> {SPT_ERR.get(rc, rc)}")
    return m


def noise_meter_host(moments: np.ndarray, batches: int, frames: float, params: Optional[NoiseParams] = None
                     ) -> Tuple[np.ndarray, np.ndarray]:
    """spt_noise_meter_host (host only): (counts, e2) of a (height, width, 4) image of moments after `batches`
    batches of `frames` frames in all: the NOISE_BINS counts and the (height, width) squared relative errors, by
    the functions the kernels compile: the same bits as Context.noise_meter / read_noise."""
    m = _pixels(moments, "noise_meter_host")
    if m.ndim != 3:
        raise ValueError("noise_meter_host: moments must be (height, width, 4)")
    h, w = m.shape[:2]
    counts = np.zeros(NOISE_BINS, dtype=np.uint32)
    e2 = np.zeros((h, w), dtype=np.float32)
    rc = load_library().spt_noise_meter_host(_ptr(m), w, h, batches, frames,
                                             ctypes.byref(params) if params is not None else None, _ptr(counts), _ptr(e2))
    if rc != SPT_OK:
        raise SptError(f"spt_noise_meter_host -> {SPT_ERR.get(rc, rc)}")
    return counts, e2


def noise_from_histogram(counts: np.ndarray, quantile: float = 0.95) -> float:
    """spt_noise_from_histogram (host only): the relative error that the share `quantile` of the pixels stays
    below: the square root of the upper edge of the bin at which the cumulative count reaches it. 0 for bin 0 and
    an empty histogram, inf for the last bin."""
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    if c.shape != (NOISE_BINS,):
        raise ValueError("noise_from_histogram: counts must hold NOISE_BINS values")
    e = ctypes.c_double(0.0)
    rc = load_library().spt_noise_from_histogram(_ptr(c), quantile, ctypes.byref(e))
    if rc != SPT_OK:
        raise SptError(f"spt_noise_from_histogram -> {SPT_ERR.get(rc, rc)}")
    return float(e.value)


def build_scene(scene: "int | str") -> Tuple[np.ndarray, np.ndarray, SptEnv]:
    """Deterministic synthetic scene (host-only, no GPU): (prims, materials, env)."""
    lib = load_library()
    sid = SCENE_IDS[scene] if isinstance(scene, str) else int(scene)
    n_p, n_m = ctypes.c_uint32(0), ctypes.c_uint32(0)
    env = SptEnv()
    rc = lib.spt_build_scene(sid, None, ctypes.byref(n_p), None, ctypes.byref(n_m), ctypes.byref(env))
    if rc != SPT_OK:
        raise SptError(f"spt_build_scene({sid}) -> {SPT_ERR.get(rc, rc)}")
    prims = np.zeros(n_p.value, dtype=PRIM_DTYPE)
    mats = np.zeros(n_m.value, dtype=MATERIAL_DTYPE)
    rc = lib.spt_build_scene(sid, _ptr(prims), ctypes.byref(n_p), _ptr(mats), ctypes.byref(n_m), ctypes.byref(env))
    if rc != SPT_OK:
        raise SptError(f"spt_build_scene({sid}) -> {SPT_ERR.get(rc, rc)}")
    return prims, mats, env


def compile_flat_kernels(prims: np.ndarray, env_map: bool = False) -> None:
    """spt_compile_flat_kernels (host only, no GPU): compile the persistent kernels specialized to
    the flat scene's shape into the process cache; raises with the compiler log on failure."""
    prims = np.ascontiguousarray(prims, dtype=PRIM_DTYPE)
    log = ctypes.create_string_buffer(1 << 16)
    rc = load_library().spt_compile_flat_kernels(_ptr(prims), len(prims), 1 if env_map else 0, log, len(log))
    if rc != SPT_OK:
        raise SptError(f"spt_compile_flat_kernels -> {SPT_ERR.get(rc, rc)}: {log.value.decode(errors='replace')}")


def sphere_prims(spheres: Sequence[Tuple[float, float, float, float]], material: int = 0) -> np.ndarray:
    p = np.zeros(len(spheres), dtype=PRIM_DTYPE)
    for i, (x, y, z, r) in enumerate(spheres):
        p[i]["type"] = PRIM_SPHERE
        p[i]["material"] = material
        p[i]["p0"] = (x, y, z, r)
    return p


def reference_materials() -> np.ndarray:
    """Reference mode: one gray Lambertian, throughput *= 0.7 (CPUPathTracer.cpp:260)."""
    m = np.zeros(1, dtype=MATERIAL_DTYPE)
    m[0]["albedo"] = (0.7, 0.7, 0.7)
    return m


class Context:
    """RAII wrapper of one spt_ctx (one HIP device)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.spt_create(ctypes.byref(h), device)
        if rc != SPT_OK:
            raise SptError(f"spt_create(device={device}) -> {SPT_ERR.get(rc, rc)} (needs a gfx950 GPU)")
        self.h = h
        self.width = self.height = 0
        self.cfg = SptConfig()
        self._out_reg = None  # the array registered by register_host_output
        self._camera: Optional[SptCamera] = None  # a copy of set_camera's (focus_at)

    def _check(self, rc: int, what: str) -> None:
        if rc != SPT_OK:
            msg = self.lib.spt_last_error(self.h)
            raise SptError(f"{what} -> {SPT_ERR.get(rc, rc)}: {msg.decode() if msg else ''}")

    def close(self) -> None:
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.spt_destroy(self.h)  # (unregisters the host output first)
            self.h = ctypes.c_void_p()
            self._out_reg = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_scene(self, prims: np.ndarray, mats: np.ndarray, env: SptEnv) -> None:
        prims = np.ascontiguousarray(prims, dtype=PRIM_DTYPE)
        mats = np.ascontiguousarray(mats, dtype=MATERIAL_DTYPE)
        self._check(self.lib.spt_set_scene(self.h, _ptr(prims), len(prims), _ptr(mats), len(mats), ctypes.byref(env)),
                    "spt_set_scene")

    def update_prims(self, indices, prims: np.ndarray) -> None:
        """spt_update_prims: replace primitives `indices` of the current scene (BVH: refit, no rebuild)."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32)
        prims = np.ascontiguousarray(prims, dtype=PRIM_DTYPE)
        if len(idx) != len(prims):
            raise ValueError("indices and prims differ in length")
        self._check(self.lib.spt_update_prims(self.h, _ptr(idx), _ptr(prims), len(idx)), "spt_update_prims")

    def configure(self, width: int, height: int, max_bounces: int = 4, rr_depth: int = 2, flags: int = 0,
                  shard_rank: int = 0, shard_count: int = 1, frames_in_flight: int = 0) -> None:
        c = SptConfig(width, height, max_bounces, rr_depth, flags, shard_rank, shard_count, frames_in_flight)
        self._check(self.lib.spt_configure(self.h, ctypes.byref(c)), "spt_configure")
        self.cfg = c
        self.width, self.height = width, height

    def set_stream(self, hip_stream: int) -> None:
        self._check(self.lib.spt_set_stream(self.h, ctypes.c_void_p(hip_stream or 0)), "spt_set_stream")

    def reset(self) -> None:
        self._check(self.lib.spt_reset(self.h), "spt_reset")

    @property
    def frame_count(self) -> int:
        v = ctypes.c_uint32()
        self._check(self.lib.spt_get_frame_count(self.h, ctypes.byref(v)), "spt_get_frame_count")
        return v.value

    def render(self, first_frame: int, n_frames: int = 1) -> None:
        self._check(self.lib.spt_render(self.h, first_frame, n_frames), "spt_render")

    def synchronize(self) -> None:
        self._check(self.lib.spt_synchronize(self.h), "spt_synchronize")

    @property
    def shard_pixels(self) -> int:
        v = ctypes.c_uint64()
        self._check(self.lib.spt_shard_pixels(self.h, ctypes.byref(v)), "spt_shard_pixels")
        return v.value

    def read_accum(self) -> np.ndarray:
        out = np.zeros((self.shard_pixels, 4), dtype=np.float32)
        self._check(self.lib.spt_read_accum(self.h, _ptr(out)), "spt_read_accum")
        return out

    def accum_device_ptr(self) -> Tuple[int, int]:
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self.lib.spt_accum_device_ptr(self.h, ctypes.byref(p), ctypes.byref(n)), "spt_accum_device_ptr")
        return p.value or 0, n.value

    def copy_accum_device(self, dst_dev_ptr: int) -> None:
        self._check(self.lib.spt_copy_accum_device(self.h, ctypes.c_void_p(dst_dev_ptr)), "spt_copy_accum_device")

    def register_host_output(self, out: Optional[np.ndarray]) -> None:
        """spt_register_host_output: `out` (uint32, C-contiguous, >= shard_pixels) becomes the page-locked,
        GPU-mapped image buffer that resolve_rgba8(out=out) has the resolve kernel write directly; None
        unregisters. The Context keeps a reference to it while registered."""
        if out is None:
            self._check(self.lib.spt_register_host_output(self.h, None, 0), "spt_register_host_output")
            self._out_reg = None
            return
        if out.dtype != np.uint32 or not out.flags["C_CONTIGUOUS"] or out.size < self.shard_pixels:
            raise SptError("register_host_output: need a C-contiguous uint32 array of >= shard_pixels")
        self._check(self.lib.spt_register_host_output(self.h, _ptr(out), out.nbytes), "spt_register_host_output")
        self._out_reg = out

    def resolve_rgba8(self, frame_count: int, exposure: float = 1.0, out: Optional[np.ndarray] = None) -> np.ndarray:
        if out is None:
            out = np.zeros(self.shard_pixels, dtype=np.uint32)
        elif out.dtype != np.uint32 or not out.flags["C_CONTIGUOUS"] or out.size < self.shard_pixels:
            raise SptError("resolve_rgba8: out must be a C-contiguous uint32 array of >= shard_pixels")
        if exposure == 1.0:
            self._check(self.lib.spt_resolve_rgba8(self.h, frame_count, _ptr(out)), "spt_resolve_rgba8")
        else:
            self._check(self.lib.spt_resolve_rgba8_exposure(self.h, frame_count, exposure, _ptr(out)),
                        "spt_resolve_rgba8_exposure")
        return out

    def render_resolve_rgba8(self, first_frame: int, n_frames: int, frame_count: int, exposure: float = 1.0,
                             out: Optional[np.ndarray] = None) -> np.ndarray:
        """spt_render_resolve_rgba8: render(first_frame, n_frames), then resolve_rgba8(frame_count, exposure,
        out) — fused into the last frame's launch when `out` is the registered buffer and the call runs
        k_frame (the App's render() + get_render_result(), App.cpp:230-240)."""
        if out is None:
            out = np.zeros(self.shard_pixels, dtype=np.uint32)
        elif out.dtype != np.uint32 or not out.flags["C_CONTIGUOUS"] or out.size < self.shard_pixels:
            raise SptError("render_resolve_rgba8: out must be a C-contiguous uint32 array of >= shard_pixels")
        self._check(self.lib.spt_render_resolve_rgba8(self.h, first_frame, n_frames, frame_count, exposure, _ptr(out)),
                    "spt_render_resolve_rgba8")
        return out

    def assemble_rows(self, gathered_dev_ptr: int, out_dev_ptr: int) -> None:
        self._check(self.lib.spt_assemble_rows(self.h, ctypes.c_void_p(gathered_dev_ptr), ctypes.c_void_p(out_dev_ptr)),
                    "spt_assemble_rows")

    def set_tuning(self, **kw) -> None:
        """spt_set_tuning with the given SptTuning fields (the others automatic)."""
        self._check(self.lib.spt_set_tuning(self.h, ctypes.byref(SptTuning(**kw))), "spt_set_tuning")

    def specialize_scene(self) -> None:
        """spt_specialize_scene: compile and load the flat scene's shape-specialized kernels now."""
        self._check(self.lib.spt_specialize_scene(self.h), "spt_specialize_scene")

    def comm_init(self, comm_id: bytes, n_ranks: int, rank: int) -> None:
        """Join the RCCL communicator `comm_id` (from comm_unique_id() on rank 0) as rank / n_ranks."""
        if len(comm_id) != COMM_ID_BYTES:
            raise ValueError("communicator id must be 128 bytes")
        buf = ctypes.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        self._check(self.lib.spt_comm_init(self.h, buf, n_ranks, rank), "spt_comm_init")

    def gather_image(self, root_image_dev_ptr: int = 0) -> None:
        """Collective: the ranks' row shards gathered to rank 0 over RCCL and assembled into the full
        float RGBA image at root_image_dev_ptr (device memory, rank 0; ignored elsewhere)."""
        self._check(self.lib.spt_gather_image(self.h, ctypes.c_void_p(root_image_dev_ptr or 0)), "spt_gather_image")

    def gather_image_overlapped(self, root_image_dev_ptr: int = 0) -> None:
        """spt_gather_image_overlapped: the same collective on the ctx's own comm stream, from a snapshot
        of the shard taken now, so that the next render() calls overlap it; gather_wait() orders the
        integrator's stream after it (root_image then holds the frames rendered before this call)."""
        self._check(self.lib.spt_gather_image_overlapped(self.h, ctypes.c_void_p(root_image_dev_ptr or 0)),
                    "spt_gather_image_overlapped")

    def gather_wait(self) -> None:
        self._check(self.lib.spt_gather_wait(self.h), "spt_gather_wait")

    def comm_destroy(self) -> None:
        self._check(self.lib.spt_comm_destroy(self.h), "spt_comm_destroy")

    def set_env_map(self, rgba: Optional[np.ndarray]) -> None:
        """Octahedral environment map (h, w, 4) float32 for the miss radiance, or None for the
        gradient sky (spt_set_env_map; resets the accumulation)."""
        if rgba is None:
            self._check(self.lib.spt_set_env_map(self.h, None, 0, 0), "spt_set_env_map")
            return
        a = np.ascontiguousarray(rgba, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("environment map must be (height, width, 4) float32")
        self._env_keep = a
        self._check(self.lib.spt_set_env_map(self.h, a.ctypes.data, a.shape[1], a.shape[0]), "spt_set_env_map")

    def set_camera(self, cam: Optional[SptCamera]) -> None:
        """spt_set_camera: the camera of later renders (look_at), or None for the reference's pinhole at
        the origin; resets the accumulation."""
        self._check(self.lib.spt_set_camera(self.h, ctypes.byref(cam) if cam is not None else None), "spt_set_camera")
        # (for focus_at; a copy: the ctx copied it too)
        self._camera = SptCamera.from_buffer_copy(cam) if cam is not None else None

    def set_camera_lens(self, radius=None, focus_distance: float = 1.0) -> None:
        """spt_set_camera_lens: a thin lens on the ctx's camera — the aperture's radius in world units (or an
        SptLens) and the distance of the plane in focus — or None / radius 0 for none; resets the accumulation.
        set_camera(cam) keeps the lens, set_camera(None) drops it."""
        if radius is None:
            self._check(self.lib.spt_set_camera_lens(self.h, None), "spt_set_camera_lens")
            return
        lens = _lens(radius, focus_distance)
        self._check(self.lib.spt_set_camera_lens(self.h, ctypes.byref(lens)), "spt_set_camera_lens")

    def focus_at(self, x: int, y: int) -> Optional[float]:
        """Click to focus: the focus distance that puts what pixel (x, y) of the full image shows — its first
        hit (read_features) — in focus, or None where its chief ray misses the scene. Needs a camera, and
        row y on this ctx's shard."""
        if self._camera is None:
            raise SptError("focus_at needs a camera (set_camera)")
        w, h = self.width, self.height
        rank, count = int(self.cfg.shard_rank), max(1, int(self.cfg.shard_count))
        if not (0 <= x < w and 0 <= y < h) or y % count != rank:
            raise SptError("focus_at: the pixel is outside the image or on another ctx's rows")
        _, feat_b, _ = self.read_features()
        t = float(feat_b.reshape(-1, w, 4)[y // count, x, 3])
        if not np.isfinite(t):
            return None
        j = 0.5 if self._camera.flags & CAMERA_JITTER else 0.0
        return camera_focus_at_hit(self._camera, w, h, x, y, t, j, j)

    def set_material_models(self, models) -> None:
        """spt_set_material_models: one model per material of the current scene — a MATERIAL_MODEL_DTYPE array
        or (kind, param) pairs with kind MAT_DIFFUSE / MAT_METAL (param: fuzz) / MAT_DIELECTRIC (param: index of
        refraction) — or None for all-diffuse; resets the accumulation."""
        if models is None:
            self._check(self.lib.spt_set_material_models(self.h, None, 0), "spt_set_material_models")
            return
        m = material_models(models)
        self._check(self.lib.spt_set_material_models(self.h, m.ctypes.data, len(m)), "spt_set_material_models")

    def render_features(self) -> None:
        """spt_render_features: the first-hit feature images of the current scene, camera and configuration
        (asynchronous; read them with read_features)."""
        self._check(self.lib.spt_render_features(self.h), "spt_render_features")

    def read_features(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """spt_read_features: (feat_a, feat_b, albedo), each (shard_pixels, 4) float32 — position and material
        bits, shading normal and distance, albedo and primitive bits; view the bit lanes as uint32."""
        n = self.shard_pixels
        a, b, alb = (np.zeros((n, 4), dtype=np.float32) for _ in range(3))
        self._check(self.lib.spt_read_features(self.h, _ptr(a), _ptr(b), _ptr(alb)), "spt_read_features")
        return a, b, alb

    def features_device_ptr(self) -> Tuple[int, int, int, int]:
        """spt_features_device_ptr: (feat_a, feat_b, albedo, bytes of each)."""
        a, b, alb, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self.lib.spt_features_device_ptr(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(alb),
                                                     ctypes.byref(n)), "spt_features_device_ptr")
        return a.value or 0, b.value or 0, alb.value or 0, n.value

    def denoise(self, frame_count: int, params: Optional[DenoiseParams] = None) -> None:
        """spt_denoise: filter the mean of the frame_count frames accumulated so far into the ctx's denoised
        image (asynchronous); params None: the defaults."""
        self._check(self.lib.spt_denoise(self.h, frame_count, ctypes.byref(params) if params is not None else None),
                    "spt_denoise")

    def denoise_guided(self, frame_count: int, params: Optional[GuidedParams] = None) -> None:
        """spt_denoise_guided: the variance-guided filter of the mean of the frame_count frames accumulated so
        far, with the noise moments folded so far (noise_update, at least two batches), into the ctx's denoised
        image (asynchronous; read_denoised / resolve_denoised_rgba8 take it from there). params=None: the defaults."""
        self._check(self.lib.spt_denoise_guided(self.h, frame_count, ctypes.byref(params) if params is not None else None),
                    "spt_denoise_guided")

    def read_denoised_variance(self) -> np.ndarray:
        """spt_read_denoised_variance: the variance the last denoise_guided propagated, per pixel of the shard."""
        out = np.zeros(self.shard_pixels, dtype=np.float32)
        self._check(self.lib.spt_read_denoised_variance(self.h, _ptr(out)), "spt_read_denoised_variance")
        return out

    def set_denoise_form(self, form: int) -> None:
        """spt_set_denoise_form (measurement and tests): 0 the straight kernel form at every level of later
        denoise calls, 1 the LDS-tiled one, -1 the library's choice per step. The image is the same."""
        self._check(self.lib.spt_set_denoise_form(self.h, form), "spt_set_denoise_form")

    def read_denoised(self) -> np.ndarray:
        out = np.zeros((self.shard_pixels, 4), dtype=np.float32)
        self._check(self.lib.spt_read_denoised(self.h, _ptr(out)), "spt_read_denoised")
        return out

    def denoised_device_ptr(self) -> Tuple[int, int]:
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self.lib.spt_denoised_device_ptr(self.h, ctypes.byref(p), ctypes.byref(n)), "spt_denoised_device_ptr")
        return p.value or 0, n.value

    def resolve_denoised_rgba8(self, exposure: float = 1.0, out: Optional[np.ndarray] = None) -> np.ndarray:
        """spt_resolve_denoised_rgba8: the denoised image as RGBA8 (into the registered buffer directly when
        `out` is that array)."""
        if out is None:
            out = np.zeros(self.shard_pixels, dtype=np.uint32)
        elif out.dtype != np.uint32 or not out.flags["C_CONTIGUOUS"] or out.size < self.shard_pixels:
            raise SptError("resolve_denoised_rgba8: out must be a C-contiguous uint32 array of >= shard_pixels")
        self._check(self.lib.spt_resolve_denoised_rgba8(self.h, exposure, _ptr(out)), "spt_resolve_denoised_rgba8")
        return out

    def history_capture(self, frame_count: int) -> None:
        """spt_history_capture: store what is shown now (the active history blended with the frame_count frames
        accumulated), its features and camera as the captured view (asynchronous)."""
        self._check(self.lib.spt_history_capture(self.h, frame_count), "spt_history_capture")

    def reproject(self, params: Optional[ReprojectParams] = None) -> None:
        """spt_reproject: map the captured view into the current camera's; the result is the active history."""
        self._check(self.lib.spt_reproject(self.h, ctypes.byref(params) if params is not None else None), "spt_reproject")

    def history_clear(self) -> None:
        self._check(self.lib.spt_history_clear(self.h), "spt_history_clear")

    def set_history_layout(self, layout: int) -> None:
        """spt_set_history_layout (measurement and tests): 0 the captured view as three images, 1 as 48-byte
        records, -1 the library's choice. The images are the same."""
        self._check(self.lib.spt_set_history_layout(self.h, layout), "spt_set_history_layout")

    def read_history(self) -> np.ndarray:
        """spt_read_history: the active history, (shard_pixels, 4) float32: mean radiance and length in frames."""
        out = np.empty((self.shard_pixels, 4), dtype=np.float32)
        self._check(self.lib.spt_read_history(self.h, _ptr(out)), "spt_read_history")
        return out

    def history_device_ptr(self) -> Tuple[int, int]:
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self.lib.spt_history_device_ptr(self.h, ctypes.byref(p), ctypes.byref(n)), "spt_history_device_ptr")
        return int(p.value or 0), int(n.value)

    def history_blend(self, frame_count: int) -> None:
        """spt_history_blend: the active history blended with the frame_count frames accumulated, into the ctx's
        blended image (asynchronous; read_blended / resolve_blended_rgba8 / denoise_blended take it from there)."""
        self._check(self.lib.spt_history_blend(self.h, frame_count), "spt_history_blend")

    def read_blended(self) -> np.ndarray:
        out = np.empty((self.shard_pixels, 4), dtype=np.float32)
        self._check(self.lib.spt_read_blended(self.h, _ptr(out)), "spt_read_blended")
        return out

    def blended_device_ptr(self) -> Tuple[int, int]:
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self.lib.spt_blended_device_ptr(self.h, ctypes.byref(p), ctypes.byref(n)), "spt_blended_device_ptr")
        return int(p.value or 0), int(n.value)

    def resolve_blended_rgba8(self, exposure: float = 1.0, out: Optional[np.ndarray] = None) -> np.ndarray:
        """spt_resolve_blended_rgba8: the blended image as RGBA8 (into the registered buffer directly when `out`
        is that buffer)."""
        if out is None:
            out = np.empty(self.shard_pixels, dtype=np.uint32)
        if out.dtype != np.uint32 or not out.flags.c_contiguous or out.size < self.shard_pixels:
            raise SptError("resolve_blended_rgba8: out must be a C-contiguous uint32 array of >= shard_pixels")
        self._check(self.lib.spt_resolve_blended_rgba8(self.h, exposure, _ptr(out)), "spt_resolve_blended_rgba8")
        return out

    def denoise_blended(self, params: Optional[DenoiseParams] = None) -> None:
        """spt_denoise_blended: the a-trous filter over the blended image, into the denoised image
        (read_denoised / resolve_denoised_rgba8)."""
        self._check(self.lib.spt_denoise_blended(self.h, ctypes.byref(params) if params is not None else None),
                    "spt_denoise_blended")

    def meter_luminance(self, frame_count: int = 0, image: int = IMAGE_ACCUM) -> np.ndarray:
        """spt_meter_luminance: the METER_BINS counts of the ctx's image (of its shard; shards' counts add up):
        the accumulation over frame_count, or the denoised or blended image (a mean: frame_count is ignored)."""
        counts = np.zeros(METER_BINS, dtype=np.uint32)
        self._check(self.lib.spt_meter_luminance(self.h, image, frame_count, _ptr(counts)), "spt_meter_luminance")
        return counts

    def meter_device_image(self, dev_ptr: int, n_pixels: int, divisor: float = 1.0) -> np.ndarray:
        """spt_meter_device_image: the same for n_pixels float RGBA pixels at a device address of the caller's."""
        counts = np.zeros(METER_BINS, dtype=np.uint32)
        self._check(self.lib.spt_meter_device_image(self.h, ctypes.c_void_p(dev_ptr), n_pixels, divisor, _ptr(counts)),
                    "spt_meter_device_image")
        return counts

    def set_meter_form(self, form: int) -> None:
        """spt_set_meter_form (measurement and tests): 0 one LDS add per lane in later meterings, 1 one add per
        distinct bin of a wave, -1 the library's choice. The counts are the same."""
        self._check(self.lib.spt_set_meter_form(self.h, form), "spt_set_meter_form")

    def resolve_display_rgba8(self, frame_count: int, display: Display, image: int = IMAGE_ACCUM,
                              out: Optional[np.ndarray] = None) -> np.ndarray:
        """spt_resolve_display_rgba8: the ctx's image through the display transform as RGBA8 (into the registered
        buffer directly when `out` is that buffer)."""
        if out is None:
            out = np.zeros(self.shard_pixels, dtype=np.uint32)
        elif out.dtype != np.uint32 or not out.flags["C_CONTIGUOUS"] or out.size < self.shard_pixels:
            raise SptError("resolve_display_rgba8: out must be a C-contiguous uint32 array of >= shard_pixels")
        self._check(self.lib.spt_resolve_display_rgba8(self.h, image, frame_count, ctypes.byref(display), _ptr(out)),
                    "spt_resolve_display_rgba8")
        return out

    def resolve_display_device_image(self, dev_ptr: int, n_pixels: int, display: Display, divisor: float = 1.0,
                                     out: Optional[np.ndarray] = None) -> np.ndarray:
        """spt_resolve_display_device_image: n_pixels float RGBA pixels at a device address of the caller's through
        the display transform as RGBA8."""
        if out is None:
            out = np.zeros(n_pixels, dtype=np.uint32)
        elif out.dtype != np.uint32 or not out.flags["C_CONTIGUOUS"] or out.size < n_pixels:
            raise SptError("resolve_display_device_image: out must be a C-contiguous uint32 array of >= n_pixels")
        self._check(self.lib.spt_resolve_display_device_image(self.h, ctypes.c_void_p(dev_ptr), n_pixels, divisor,
                                                              ctypes.byref(display), _ptr(out)),
                    "spt_resolve_display_device_image")
        return out

    def noise_update(self, frame_count: int) -> None:
        """spt_noise_update: fold the frames since the last update (or restart) into the per-pixel moments;
        frame_count: the frames the accumulation holds. Asynchronous on the ctx stream."""
        self._check(self.lib.spt_noise_update(self.h, frame_count), "spt_noise_update")

    def noise_batches(self) -> Tuple[int, int]:
        """spt_noise_batches: (batches, frames) folded since the accumulation last restarted."""
        b, f = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(self.lib.spt_noise_batches(self.h, ctypes.byref(b), ctypes.byref(f)), "spt_noise_batches")
        return int(b.value), int(f.value)

    def noise_meter(self, radius: int = 1, dark_floor: float = 0.01) -> np.ndarray:
        """spt_noise_meter: the NOISE_BINS counts of the per-pixel squared relative error (noise_from_histogram
        reads a quantile off them), pooled over (2 radius + 1)^2 windows; also writes the image read_noise
        returns. Needs two updates since the last restart."""
        counts = np.zeros(NOISE_BINS, dtype=np.uint32)
        p = NoiseParams(radius=radius, dark_floor=dark_floor)
        self._check(self.lib.spt_noise_meter(self.h, ctypes.byref(p), _ptr(counts)), "spt_noise_meter")
        return counts

    def read_noise_moments(self) -> np.ndarray:
        """spt_read_noise_moments: (shard pixels, 4) float32: mean, m2, prevL, 0."""
        out = np.zeros((self.shard_pixels, 4), dtype=np.float32)
        self._check(self.lib.spt_read_noise_moments(self.h, _ptr(out)), "spt_read_noise_moments")
        return out

    def read_noise(self) -> np.ndarray:
        """spt_read_noise: the last metering's squared relative error per pixel of the shard."""
        out = np.zeros(self.shard_pixels, dtype=np.float32)
        self._check(self.lib.spt_read_noise(self.h, _ptr(out)), "spt_read_noise")
        return out

    def noise_device_ptr(self) -> Tuple[int, int, int]:
        """spt_noise_device_ptr: (moments address, e2 address, pixels); an address is 0 while its image does not exist."""
        m, e, n = ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_uint64(0)
        self._check(self.lib.spt_noise_device_ptr(self.h, ctypes.byref(m), ctypes.byref(e), ctypes.byref(n)),
                    "spt_noise_device_ptr")
        return int(m.value or 0), int(e.value or 0), int(n.value)

    def noise_meter_device_image(self, dev_ptr: int, width: int, height: int, batches: int, frames: float,
                                 params: Optional[NoiseParams] = None, e2_dev_ptr: int = 0) -> np.ndarray:
        """spt_noise_meter_device_image: the counts of width * height moments at a device address of the caller's
        after `batches` batches of `frames` frames in all; e2_dev_ptr (0: none) receives the per-pixel values."""
        counts = np.zeros(NOISE_BINS, dtype=np.uint32)
        self._check(self.lib.spt_noise_meter_device_image(
            self.h, ctypes.c_void_p(dev_ptr), width, height, batches, frames,
            ctypes.byref(params) if params is not None else None, _ptr(counts), ctypes.c_void_p(e2_dev_ptr)),
            "spt_noise_meter_device_image")
        return counts

    def set_profiling(self, enable, counters: bool = False, span: bool = False) -> None:
        """enable: HIP-event timing of every launch; counters: k_paths also counts segments per
        bounce (a slower kernel variant; the wavefront schedules always count); span: instead of
        per-launch events, one event pair around all k_paths / k_frame launches until profiling is
        switched off (SPT_PROFILE_SPAN; only with enable)."""
        mode = (PROFILE_EVENTS if enable and not span else 0) | (PROFILE_COUNTERS if counters else 0) | \
            (PROFILE_SPAN if span and enable else 0)
        self._check(self.lib.spt_set_profiling(self.h, mode), "spt_set_profiling")

    def stats(self) -> SptStats:
        s = SptStats()
        self._check(self.lib.spt_get_stats(self.h, ctypes.byref(s)), "spt_get_stats")
        wide = ctypes.c_uint64(0)
        self._check(self.lib.spt_get_view_wide(self.h, ctypes.byref(wide)), "spt_get_view_wide")
        s.view_wide = int(wide.value)
        ranges = ctypes.c_uint64(0)
        if not os.environ.get("SPT_LIB_PATH") or hasattr(self.lib, "spt_get_flat_ranges"):  # (an older A/B library: 0)
            self._check(self.lib.spt_get_flat_ranges(self.h, ctypes.byref(ranges)), "spt_get_flat_ranges")
        s.flat_ranges = int(ranges.value)
        return s

    def clear_stats(self) -> None:
        self._check(self.lib.spt_stats_clear(self.h), "spt_stats_clear")


def comm_available() -> bool:
    """True if this process can reach RCCL (spt_comm_available: symbols resolved; nothing created)."""
    return load_library().spt_comm_available() == SPT_OK


def comm_unique_id() -> bytes:
    """A new RCCL communicator id (rank 0; share it with the other ranks out of band)."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    rc = load_library().spt_comm_unique_id(buf)
    if rc != SPT_OK:
        raise SptError(f"spt_comm_unique_id -> {SPT_ERR.get(rc, rc)}")
    return buf.raw


def device_count() -> int:
    lib = load_library()
    n = ctypes.c_int()
    lib.spt_device_count(ctypes.byref(n))
    return n.value


# ---------------------------------------------------------------------------------------------
# Mirror of the reference interface (PathTracer.h:13-51, Types.h:43-95, Scene.h:123-227)
# ---------------------------------------------------------------------------------------------
class BackendType(enum.IntEnum):
    """PathTracer::BackendType (PathTracer.h:16-21) + the new GPU_HIP backend."""

    CPU_EMBREE = 0
    GPU_OPTIX = 1
    GPU_METAL = 2
    GPU_HIP = 3


class RenderSettings:
    """render::RenderSettings with its dirty flag (Types.h:43-95, RenderSettings.cpp:5-54)."""

    def __init__(self):
        self._width, self._height = 512, 512
        self._progressive = True
        self._spp, self._max_bounces, self._rr_depth = 64, 8, 3
        self._exposure = 1.0
        self._auto_exposure, self._target_luminance = False, 0.18
        self._dirty = True  # dirty on construction

    def _set(self, name, value):
        if getattr(self, name) != value:
            setattr(self, name, value)
            self._dirty = True

    def setResolution(self, width: int, height: int) -> None:
        if (self._width, self._height) != (width, height):
            self._width, self._height = width, height
            self._dirty = True

    def setProgressive(self, v: bool) -> None:
        self._set("_progressive", v)

    def setSamplesPerPixel(self, v: int) -> None:
        self._set("_spp", v)

    def setMaxBounces(self, v: int) -> None:
        self._set("_max_bounces", v)

    def setRussianRouletteDepth(self, v: int) -> None:
        self._set("_rr_depth", v)

    def setExposure(self, v: float) -> None:
        self._set("_exposure", v)

    def setAutoExposure(self, enabled: bool, target_luminance: float = 0.18) -> None:
        if (self._auto_exposure, self._target_luminance) != (enabled, target_luminance):
            self._auto_exposure, self._target_luminance = enabled, target_luminance
            self._dirty = True

    def getAutoExposure(self) -> bool:
        return self._auto_exposure

    def getTargetLuminance(self) -> float:
        return self._target_luminance

    def getProgressive(self) -> bool:
        return self._progressive

    def getWidth(self) -> int:
        return self._width

    def getHeight(self) -> int:
        return self._height

    def getSamplesPerPixel(self) -> int:
        return self._spp

    def getMaxBounces(self) -> int:
        return self._max_bounces

    def getRussianRouletteDepth(self) -> int:
        return self._rr_depth

    def getExposure(self) -> float:
        return self._exposure

    def isDirty(self) -> bool:
        return self._dirty

    def clearDirty(self) -> None:
        self._dirty = False


class SphereObject:
    """render::SphereObject (Scene.h:123-133): position + radius."""

    def __init__(self, name: str = "Sphere"):
        self.name = name
        self.position = (0.0, 0.0, 0.0)
        self.radius = 1.0

    def SetPosition(self, p) -> None:
        self.position = tuple(float(v) for v in p)

    def SetRadius(self, r: float) -> None:
        self.radius = float(r)

    def GetPosition(self):
        return self.position

    def GetRadius(self) -> float:
        return self.radius


class Scene:
    """render::Scene (Scene.h:135-227): node registry + change flag."""

    def __init__(self):
        self._nodes = []
        self._has_changes = True

    def CreateNode(self, cls=SphereObject, name: str = "Sphere"):
        n = cls(name)
        self._nodes.append(n)
        return n

    def GetAllNodes(self):
        return list(self._nodes)

    def hasChanges(self) -> bool:
        return self._has_changes

    def markChangesProcessed(self) -> None:
        self._has_changes = False


class RenderResult:
    """PathTracer::RenderResult (PathTracer.h:23-28): RGBA8888 u32 per pixel, R in the high byte."""

    def __init__(self):
        self.image_buffer = np.zeros(0, dtype=np.uint32)
        self.width = 0
        self.height = 0


class PathTracer:
    """Abstract render::PathTracer (PathTracer.h:13-51)."""

    BackendType = BackendType

    @staticmethod
    def create_path_tracer(backend: BackendType) -> "PathTracer":
        # PathTracer.cpp:9-22; the reference's CPU_EMBREE backend is not part of this build
        if backend == BackendType.GPU_HIP:
            return HIPPathTracer()
        raise RuntimeError("Unknown backend type")


class HIPPathTracer(PathTracer):
    """GPU_HIP backend with CPUPathTracer's progressive-state semantics (CPUPathTracer.cpp:43-161).

    Reference mode (default): spheres of the Scene, albedo 0.7, sky on, 4 bounces, RR after bounce 2,
    one sample per pixel per render(); RenderSettings other than the resolution are ignored, as
    CPUPathTracer ignores them (CPUPathTracer.cpp:199, :264, :101-104).

    settings_mode=True honours RenderSettings instead: getMaxBounces,
    getRussianRouletteDepth, getSamplesPerPixel (frames traced per render() call — one spt_render
    call, so 64 spp run the persistent k_paths schedule), getProgressive (False: every render()
    starts a fresh accumulation) and getExposure (applied in the resolve).
    """

    def __init__(self, device: int = 0, max_bounces: int = 4, rr_depth: int = 2, flags: int = 0,
                 settings_mode: bool = False):
        self._ctx = Context(device)
        self._scene: Optional[Scene] = None
        self._settings = RenderSettings()
        self._result = RenderResult()
        self._frame_count = 0
        self._max_bounces, self._rr_depth, self._flags = max_bounces, rr_depth, flags
        self._settings_mode = settings_mode
        self._camera: Optional[SptCamera] = None
        self._camera_dirty = False
        self._lens: Optional[SptLens] = None
        self._lens_dirty = False
        self._models = None
        self._models_dirty = False
        self._denoise: Optional[DenoiseParams] = None
        self._guided: Optional[GuidedParams] = None
        self._reproject: Optional[ReprojectParams] = None
        self._tonemap = TONEMAP_CLAMP
        self._exposure_params: Optional[ExposureParams] = None
        self._noise_target, self._noise_quantile = 0.0, 0.95
        self._noise, self._converged, self._noise_folds = float("inf"), False, 0

    # HIPPathTracer::kNoiseUpdateEvery / kNoiseMeterEvery
    NOISE_UPDATE_EVERY = 8
    NOISE_METER_EVERY = 4
    # HIPPathTracer::kGuidedMinBatches: below it the variance is too noisy to guide
    GUIDED_MIN_BATCHES = 4

    def set_noise_target(self, rel_error: float, quantile: float = 0.95) -> None:
        """Not in the reference interface: a stop rule. While rel_error > 0, render() folds the frames since the
        last fold into the ctx's noise estimate (Context.noise_update) once NOISE_UPDATE_EVERY frames have
        gathered, meters it after every NOISE_METER_EVERY folds (Context.noise_meter, default parameters) and takes
        noise_from_histogram at `quantile`: noise(). Once that is at most rel_error the tracer is converged():
        render() returns without tracing and the frame count stays. Anything that restarts the accumulation
        clears both. rel_error <= 0 (the default) switches it off."""
        if not 0.0 < quantile <= 1.0:
            raise SptError("set_noise_target: the quantile must be in (0, 1]")
        self._noise_target = rel_error if rel_error > 0.0 else 0.0
        self._noise_quantile = quantile
        self._noise, self._converged = float("inf"), False

    def noise(self) -> float:
        """The last metered value; inf before the first metering."""
        return self._noise

    def converged(self) -> bool:
        return self._converged

    def frame_count(self) -> int:
        return self._frame_count

    def _noise_step(self) -> None:
        batches, folded = self._ctx.noise_batches()  # (a target switched on over unfolded frames: the first batch)
        if self._frame_count - folded < self.NOISE_UPDATE_EVERY:
            return
        self._ctx.noise_update(self._frame_count)
        if self._noise_target <= 0.0:  # (folded for set_denoise_guided alone: nothing to meter)
            return
        self._noise_folds += 1
        if self._noise_folds < self.NOISE_METER_EVERY or batches + 1 < 2:
            return
        self._noise_folds = 0
        self._noise = noise_from_histogram(self._ctx.noise_meter(), self._noise_quantile)
        self._converged = self._noise <= self._noise_target

    def set_tonemap(self, tonemap: int) -> None:
        """Not in the reference interface: the tone-mapping operator of get_render_result() (TONEMAP_CLAMP, the
        default: the plain resolve; TONEMAP_REINHARD; TONEMAP_ACES). render() and the accumulation are the same."""
        if tonemap not in (TONEMAP_CLAMP, TONEMAP_REINHARD, TONEMAP_ACES):
            raise SptError("set_tonemap: unknown operator")
        self._tonemap = tonemap

    def set_exposure_params(self, params: Optional[ExposureParams]) -> None:
        """Not in the reference interface: the auto-exposure's parameters besides the target, which always comes
        from the settings (setAutoExposure); None: the library's defaults."""
        self._exposure_params = params

    def _display_on(self) -> bool:
        return self._tonemap != TONEMAP_CLAMP or (self._settings_mode and self._settings.getAutoExposure())

    def _resolve_display(self, image: int, exposure: float) -> np.ndarray:
        """Meter the image about to be shown (settings mode with auto-exposure), then resolve it with the operator."""
        if self._settings_mode and self._settings.getAutoExposure():
            p = ExposureParams()
            if self._exposure_params is not None:
                ctypes.memmove(ctypes.byref(p), ctypes.byref(self._exposure_params), ctypes.sizeof(p))
            p.target_luminance = self._settings.getTargetLuminance()
            auto = exposure_from_histogram(self._ctx.meter_luminance(self._frame_count, image), p)
            exposure = float(np.float32(auto) * np.float32(exposure))  # (the setting is the compensation)
        return self._ctx.resolve_display_rgba8(self._frame_count, Display(self._tonemap, exposure), image)

    def set_reproject(self, params: Optional[ReprojectParams]) -> None:
        """Not in the reference interface: temporal reprojection. While params is not None, a camera or lens change
        that arrives with frames accumulated captures the view before it is applied and reprojects it after
        (Context.history_capture / reproject with these parameters), and get_render_result() returns the blend
        of that history with the frames since (the denoised blend with set_denoise on). None (the default)
        switches it off and drops the history."""
        self._reproject = params
        if params is None:
            self._ctx.history_clear()

    def set_denoise(self, params: Optional[DenoiseParams]) -> None:
        """Not in the reference interface: while params is not None, get_render_result() returns the denoised
        image (Context.denoise with these parameters) of the frames accumulated so far; None (the default)
        returns the plain mean. render() and the accumulation are the same either way."""
        self._denoise = params

    def set_denoise_guided(self, params: Optional[GuidedParams]) -> None:
        """Not in the reference interface: while params is not None, render() folds a batch into the ctx's noise
        estimate every NOISE_UPDATE_EVERY frames (with or without a noise target) and get_render_result() returns
        the variance-guided denoised image (Context.denoise_guided with these parameters) once GUIDED_MIN_BATCHES
        batches are folded; below that it returns the plain denoised image (Context.denoise with set_denoise's
        parameters, or the defaults). Anything that restarts the accumulation restarts the sequence. With
        set_reproject on, the blend is shown as without this call: the guided filter is not applied to it.
        None (the default) switches it off."""
        self._guided = params

    def set_scene(self, scene: Scene) -> None:
        self._scene = scene

    def set_camera(self, cam: Optional[SptCamera]) -> None:
        """Not in the reference interface: the camera (look_at) of the next render() on, or None for the
        reference's; the accumulation restarts there."""
        self._camera = cam
        self._camera_dirty = True
        if cam is None:
            # the lens goes with its camera, set or pending, at this moment (as HIPPathTracer::set_camera); the
            # removal stays pending, for the ctx keeps its lens if a new camera arrives before the next render()
            self._lens = None
            self._lens_dirty = True

    def set_lens(self, radius=None, focus_distance: float = 1.0) -> None:
        """Not in the reference interface: a thin lens on the camera (Context.set_camera_lens) from the next
        render() on, or None / radius 0 for none; the accumulation restarts there. It needs a camera
        (set_camera), stays when the camera moves and goes with it at the moment of set_camera(None): a lens
        set before that call, applied or still pending, is dropped."""
        self._lens = None if radius is None else _lens(radius, focus_distance)
        self._lens_dirty = True

    def set_material_models(self, models) -> None:
        """Not in the reference interface: one model per material of the scene (Context.set_material_models; the
        backend's scenes have the one reference material) from the next render() on, or None for all-diffuse;
        the accumulation restarts there. A scene rebuild keeps them."""
        self._models = None if models is None else material_models(models)
        self._models_dirty = True

    def set_settings(self, settings: RenderSettings) -> None:
        self._settings = settings

    def get_scene(self) -> Optional[Scene]:
        return self._scene

    def get_settings(self) -> RenderSettings:
        return self._settings

    def get_backend_name(self) -> str:
        return "GPU Path Tracer (HIP, gfx950)"

    def get_backend_type(self) -> BackendType:
        return BackendType.GPU_HIP

    def _invalidate(self) -> None:
        # CPUPathTracer.cpp:119-161
        needs_rebuild = False
        if self._scene.hasChanges():
            self._frame_count = 0
            needs_rebuild = True
        size_changed = (self._result.width, self._result.height) != (self._settings.getWidth(),
                                                                     self._settings.getHeight())
        if self._settings.isDirty() or size_changed:
            self._frame_count = 0
            self._settings.clearDirty()
            self._result.width, self._result.height = self._settings.getWidth(), self._settings.getHeight()
            bounces, rr = self._max_bounces, self._rr_depth
            if self._settings_mode:
                bounces, rr = self._settings.getMaxBounces(), self._settings.getRussianRouletteDepth()
            self._ctx.configure(self._result.width, self._result.height, bounces, rr, self._flags)
        # (the frame count is 0 here if anything above changed the radiance: nothing is captured then)
        reuse = self._reproject is not None and self._frame_count > 0 and (self._camera_dirty or self._lens_dirty)
        if reuse:
            self._ctx.history_capture(self._frame_count)
        if self._camera_dirty:
            self._frame_count = 0
            self._camera_dirty = False
            self._ctx.set_camera(self._camera)
        if self._lens_dirty:
            self._frame_count = 0
            self._lens_dirty = False
            if self._lens is not None or self._camera is not None:  # (no camera: the ctx has no lens either)
                self._ctx.set_camera_lens(self._lens)
        if reuse:
            self._ctx.reproject(self._reproject)
        if self._frame_count == 0:
            self._ctx.reset()
        if needs_rebuild:
            spheres = [(*n.GetPosition(), n.GetRadius()) for n in self._scene.GetAllNodes()
                       if isinstance(n, SphereObject)]
            self._ctx.set_scene(sphere_prims(spheres), reference_materials(), reference_env(True))
            self._scene.markChangesProcessed()
        # (after the rebuild: spt_set_scene resets the models, and they need a scene)
        if self._models_dirty or (needs_rebuild and self._models is not None):
            self._frame_count = 0
            self._models_dirty = False
            self._ctx.set_material_models(self._models)

    def render(self) -> None:
        if self._scene is None:
            raise SptError("Scene not set before rendering")  # verify, CPUPathTracer.cpp:46
        if self._settings_mode and not self._settings.getProgressive():
            self._frame_count = 0  # a fresh accumulation every call
        self._invalidate()
        if self._noise_target > 0.0:
            if self._frame_count == 0:  # (the ctx's estimate restarted with the accumulation)
                self._noise, self._converged, self._noise_folds = float("inf"), False, 0
            elif self._converged:
                return  # nothing traced, the frame count stays
        n = max(1, self._settings.getSamplesPerPixel()) if self._settings_mode else 1
        self._ctx.render(self._frame_count, n)
        self._frame_count += n
        if self._noise_target > 0.0 or self._guided is not None:
            self._noise_step()

    def get_render_result(self) -> RenderResult:
        if self._frame_count <= 0:
            raise SptError("No frames rendered yet")  # CPUPathTracer.cpp:89
        exposure = self._settings.getExposure() if self._settings_mode else 1.0
        display = self._display_on()  # auto-exposure or an operator: the metered display resolve of the same image
        if self._reproject is not None:
            self._ctx.history_blend(self._frame_count)
            if self._denoise is not None:
                self._ctx.denoise_blended(self._denoise)
                self._result.image_buffer = (self._resolve_display(IMAGE_DENOISED, exposure) if display else
                                             self._ctx.resolve_denoised_rgba8(exposure))
            else:
                self._result.image_buffer = (self._resolve_display(IMAGE_BLENDED, exposure) if display else
                                             self._ctx.resolve_blended_rgba8(exposure))
            return self._result
        if self._guided is not None or self._denoise is not None:
            if self._guided is not None and self._ctx.noise_batches()[0] >= self.GUIDED_MIN_BATCHES:
                self._ctx.denoise_guided(self._frame_count, self._guided)
            else:
                self._ctx.denoise(self._frame_count, self._denoise)
            self._result.image_buffer = (self._resolve_display(IMAGE_DENOISED, exposure) if display else
                                         self._ctx.resolve_denoised_rgba8(exposure))
            return self._result
        if display:
            self._result.image_buffer = self._resolve_display(IMAGE_ACCUM, exposure)
            return self._result
        self._result.image_buffer = self._ctx.resolve_rgba8(self._frame_count, exposure)
        return self._result

    def read_accumulation(self) -> np.ndarray:
        return self._ctx.read_accum()
