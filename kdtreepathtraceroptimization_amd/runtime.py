"""ctypes binding of the C-ABI in include/kdpt.h.

Python here is plumbing (tests, bench, torch.distributed); the path tracer is
the in-tree HIP library ``libkdpt.so``.  There is no CPU fallback: if the
library is missing or cannot open a HIP device every entry point raises.

Mirrors the reference's operator interface (src/pathtrace.h:6-21):
``PathTracer(scene, options)``          ~ pathtraceInit(Scene*, enablekd)
``PathTracer.trace_iteration(iter)``    ~ pathtrace(pbo, frame, iter, ...flags)
``PathTracer.close()``                  ~ pathtraceFree(Scene*, enablekd)
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KDPT_LIBRARY") or os.path.join(HERE, "libkdpt.so")

KDPT_OK = 0


class KdptError(RuntimeError):
    pass


# ---------------------------------------------------------------- structs
class Geom(C.Structure):  # struct Geom, src/sceneStructs.h:22-31
    _fields_ = [("type", C.c_int), ("materialid", C.c_int), ("translation", C.c_float * 3),
                ("rotation", C.c_float * 3), ("scale", C.c_float * 3), ("transform", C.c_float * 16),
                ("inverseTransform", C.c_float * 16), ("invTranspose", C.c_float * 16)]


class Material(C.Structure):  # struct Material, src/sceneStructs.h:33-44
    _fields_ = [("color", C.c_float * 3), ("specular_exponent", C.c_float), ("specular_color", C.c_float * 3),
                ("hasReflective", C.c_float), ("hasRefractive", C.c_float), ("indexOfRefraction", C.c_float),
                ("emittance", C.c_float), ("transmittance", C.c_float * 3)]


class Camera(C.Structure):  # struct Camera, src/sceneStructs.h:46-55
    _fields_ = [("resolution", C.c_int * 2), ("position", C.c_float * 3), ("lookAt", C.c_float * 3),
                ("view", C.c_float * 3), ("up", C.c_float * 3), ("right", C.c_float * 3), ("fov", C.c_float * 2),
                ("pixelLength", C.c_float * 2)]


class NodeBare(C.Structure):  # KDN::NodeBare, src/KDnode.h:64-82
    _fields_ = [("axis", C.c_int), ("splitPos", C.c_float), ("mins", C.c_float * 3), ("maxs", C.c_float * 3),
                ("ID", C.c_int), ("parentID", C.c_int), ("leftID", C.c_int), ("rightID", C.c_int),
                ("triIdStart", C.c_int), ("triIdSize", C.c_int), ("tmin", C.c_float), ("tmax", C.c_float)]


class TriBare(C.Structure):  # KDN::TriBare, src/KDnode.h:51-62
    _fields_ = [(n, C.c_float) for n in ("x1", "x2", "x3", "y1", "y2", "y3", "z1", "z2", "z3",
                                          "nx1", "nx2", "nx3", "ny1", "ny2", "ny3", "nz1", "nz2", "nz3")] + [
        ("mtlIdx", C.c_int)]


class PathSegment(C.Structure):  # struct PathSegment, src/sceneStructs.h:65-71
    _fields_ = [("origin", C.c_float * 3), ("direction", C.c_float * 3), ("isinside", C.c_uint8),
                ("pad_", C.c_uint8 * 3), ("sdepth", C.c_float), ("color", C.c_float * 3), ("pixelIndex", C.c_int),
                ("remainingBounces", C.c_int), ("materialIdHit", C.c_int)]


class Scene(C.Structure):
    _fields_ = [("camera", Camera), ("traceDepth", C.c_int), ("geoms", C.POINTER(Geom)), ("num_geoms", C.c_int),
                ("materials", C.POINTER(Material)), ("num_materials", C.c_int), ("has_obj", C.c_int),
                ("nodes", C.POINTER(NodeBare)), ("num_nodes", C.c_int), ("tris", C.POINTER(TriBare)),
                ("num_tris", C.c_int), ("obj_materialOffsets", C.POINTER(C.c_int)), ("num_shapes", C.c_int),
                ("obj_verts", C.POINTER(C.c_float)), ("num_obj_verts", C.c_int), ("obj_norms", C.POINTER(C.c_float)),
                ("num_obj_norms", C.c_int), ("obj_polyoffsets", C.POINTER(C.c_int)),
                ("obj_polysidxflat", C.POINTER(C.c_int)), ("polyidxcount", C.c_int),
                ("obj_bboxes", C.POINTER(C.c_float)), ("num_bbox_floats", C.c_int)]


class Options(C.Structure):
    _fields_ = [("focal_length", C.c_float), ("dof_angle", C.c_float), ("softness", C.c_float),
                ("cacherays", C.c_int), ("antialias", C.c_int), ("enable_sss", C.c_int), ("testing_mode", C.c_int),
                ("compaction", C.c_int), ("enable_kd", C.c_int), ("viz_kd", C.c_int), ("use_bbox", C.c_int),
                ("short_stack", C.c_int), ("bounce_cap", C.c_int), ("block_size", C.c_int),
                ("external_image", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("segments", C.c_longlong), ("seg_per_bounce", C.c_longlong * 32), ("bounces", C.c_int),
                ("iterations", C.c_int), ("ms_last_iteration", C.c_float), ("ms_intersect", C.c_float),
                ("total_segments", C.c_longlong), ("intersect_ms_total", C.c_double),
                ("intersect_launches_total", C.c_longlong), ("intersect_device_ms_total", C.c_double),
                ("intersect_device_launches_total", C.c_longlong), ("intersect_grid_share", C.c_float),
                ("total_trace_rays", C.c_longlong), ("create_ms", C.c_double), ("mask_build_ms", C.c_double)]


class SceneDesc(C.Structure):
    _fields_ = [("res", C.c_int * 2), ("fovy", C.c_float), ("iterations", C.c_int), ("traceDepth", C.c_int),
                ("eye", C.c_float * 3), ("lookAt", C.c_float * 3), ("up", C.c_float * 3),
                ("num_materials", C.c_int), ("materials", C.POINTER(Material)), ("num_geoms", C.c_int),
                ("geom_type", C.POINTER(C.c_int)), ("geom_material", C.POINTER(C.c_int)),
                ("geom_trs", C.POINTER(C.c_float)), ("ntri", C.c_int), ("verts9", C.POINTER(C.c_float)),
                ("norms9", C.POINTER(C.c_float)), ("shape_of_tri", C.POINTER(C.c_int)), ("num_shapes", C.c_int),
                ("shape_materials", C.POINTER(Material)), ("kd_max_depth", C.c_int)]


class RayHit(C.Structure):  # kdpt_ray_hit: one record of kdpt_cast_rays
    _fields_ = [("t", C.c_float), ("kind", C.c_int), ("prim", C.c_int), ("material", C.c_int),
                ("point", C.c_float * 3), ("normal", C.c_float * 3)]


HIT_INVALID, HIT_NONE, HIT_GEOM, HIT_TRIANGLE = -1, 0, 1, 2  # kdpt_ray_hit.kind (KDPT_HIT_*)
CAST_NORMALIZE = 1  # kdpt_cast_rays flag (KDPT_CAST_NORMALIZE)
RAY_HIT_DTYPE = np.dtype([("t", "<f4"), ("kind", "<i4"), ("prim", "<i4"), ("material", "<i4"),
                          ("point", "<f4", 3), ("normal", "<f4", 3)])
assert C.sizeof(RayHit) == 40 and RAY_HIT_DTYPE.itemsize == 40


class CastStats(NamedTuple):  # kdpt_cast_stats
    rays: int         # rays cast since create/reset
    traced: int       # ... of which reached the KD traversal kernel
    device_ms: float  # the last cast's device time


class TraceRaysStats(NamedTuple):  # kdpt_trace_rays_stats: of the last kdpt_trace_rays
    segments: int     # path segments launched into the intersect stage, summed over its iterations
    traced: int       # ... of which were handed to the KD traversal kernel
    device_ms: float  # the call's device time

class Noise(C.Structure):  # kdpt_noise: kdpt_noise_estimate's result
    _fields_ = [("samples", C.c_longlong), ("pixels", C.c_longlong), ("above", C.c_longlong),
                ("nonfinite", C.c_longlong), ("mean", C.c_double), ("max", C.c_float), ("pad_", C.c_float)]


class Adaptive(C.Structure):  # kdpt_adaptive: kdpt_trace_adaptive's result
    _fields_ = [("pixels", C.c_longlong), ("active", C.c_longlong), ("pixel_samples", C.c_longlong),
                ("segments", C.c_longlong), ("traced", C.c_longlong), ("device_ms", C.c_double)]


class DenoiseParams(C.Structure):  # kdpt_denoise_params: the filter's knobs (kdpt_default_denoise_params)
    _fields_ = [("passes", C.c_int), ("normal_power_log2", C.c_int), ("sigma_l", C.c_float), ("sigma_z", C.c_float),
                ("eps_l", C.c_float), ("pad_", C.c_float)]


class DenoiseStats(NamedTuple):  # kdpt_denoise_stats: of the last kdpt_denoise
    guide_ms: float   # the pinhole rays, their traversal and hit records
    filter_ms: float  # packing, the passes and the copy out


class TemporalParams(C.Structure):  # kdpt_temporal_params: the temporal stage's knobs (kdpt_default_temporal_params)
    _fields_ = [("alpha", C.c_float), ("sigma_z", C.c_float), ("normal_min", C.c_float), ("max_history", C.c_int),
                ("pad_", C.c_float * 2)]


class TemporalStats(NamedTuple):  # kdpt_temporal_stats: of the last kdpt_denoise_temporal
    guide_ms: float      # the pinhole rays, their traversal and hit records
    temporal_ms: float   # packing and the temporal stage
    filter_ms: float     # the passes and the copy out
    valid: int           # the frame's valid pixels
    with_history: int    # ... of which found history


assert C.sizeof(Noise) == 48 and C.sizeof(Adaptive) == 48 and C.sizeof(DenoiseParams) == 24
assert C.sizeof(TemporalParams) == 24
assert C.sizeof(Geom) == 236 and C.sizeof(Material) == 56 and C.sizeof(Camera) == 84
assert C.sizeof(NodeBare) == 64 and C.sizeof(TriBare) == 76 and C.sizeof(PathSegment) == 56

EXPORTS = [
    "kdpt_default_options", "kdpt_create", "kdpt_trace_iteration", "kdpt_trace_iteration_async", "kdpt_trace_iterations", "kdpt_synchronize",
    "kdpt_read_image", "kdpt_write_pbo", "kdpt_reset", "kdpt_get_stats", "kdpt_destroy", "kdpt_last_error",
    "kdpt_image_device_ptr", "kdpt_debug_paths", "kdpt_count_iteration", "kdpt_count_split", "kdpt_wave_profile", "kdpt_selftest_math", "kdpt_selftest_rng", "kdpt_selftest_rng_draws",
    "kdpt_selftest_fresnel", "kdpt_selftest_libm", "kdpt_selftest_libm_digest", "kdpt_scene_load", "kdpt_scene_build", "kdpt_scene_view", "kdpt_scene_free",
    "kdpt_save_rgb8", "kdpt_save_png", "kdpt_save_hdr", "kdpt_png_encode", "kdpt_write_png", "kdpt_hdr_encode",
    "kdpt_write_hdr", "kdpt_free", "kdpt_set_tuning", "kdpt_selftest_glm", "kdpt_set_options", "kdpt_scene_build_device",
    "kdpt_scene_kd_build_ms", "kdpt_build_kd_device", "kdpt_scene_load_device", "kdpt_trace_config",
    "kdpt_cull_margin", "kdpt_comm_unique_id", "kdpt_comm_init", "kdpt_render_frames", "kdpt_render_sharded",
    "kdpt_comm_library", "kdpt_cull_masks", "kdpt_cast_rays", "kdpt_cast_stats",
    "kdpt_set_camera", "kdpt_camera_rays", "kdpt_trace_rays", "kdpt_trace_rays_stats", "kdpt_shade_staged",
    "kdpt_set_moments", "kdpt_read_moments", "kdpt_noise_map", "kdpt_noise_estimate", "kdpt_trace_rays_moments",
    "kdpt_selftest_scatter", "kdpt_selftest_shade",
    "kdpt_active_pixels", "kdpt_trace_adaptive", "kdpt_read_sample_counts", "kdpt_save_counted",
    "kdpt_selftest_active_list",
    "kdpt_group_create", "kdpt_group_render_frames", "kdpt_group_synchronize", "kdpt_group_context",
    "kdpt_group_active_pixels", "kdpt_group_trace_adaptive", "kdpt_group_set_camera", "kdpt_group_set_options",
    "kdpt_group_reset", "kdpt_group_destroy",
    "kdpt_default_denoise_params", "kdpt_denoise_buffers", "kdpt_denoise", "kdpt_denoise_stats",
    "kdpt_default_temporal_params", "kdpt_temporal_buffers", "kdpt_denoise_temporal", "kdpt_temporal_reset",
    "kdpt_temporal_stats",
]

REDUCE_RCCL, REDUCE_COPY = 0, 1  # kdpt_render_sharded's reduce (KDPT_REDUCE_*)
GROUP_MOMENTS = 1  # kdpt_group_create flag (KDPT_GROUP_MOMENTS)


def set_process_tuning(name: str, value: float):
    """kdpt_set_tuning(NULL, ...): a process-wide knob that contexts created afterwards start with
    ("reduce_spin_us", "cluster_chord")."""
    lib = load_library()
    _check(lib.kdpt_set_tuning(None, name.encode(), float(value)), f"kdpt_set_tuning(NULL, {name})")

_lib = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load the in-tree libkdpt.so (HIP runtime shared with torch when torch is imported)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise KdptError(f"{path} is missing: run `python -m kdtreepathtraceroptimization_amd._build` "
                        "(there is no CPU fallback)")
    try:  # one HIP runtime per process: let torch's libamdhip64 (same soname) win if present
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(path)
    P = C.POINTER
    lib.kdpt_default_options.argtypes = [P(Options)]
    lib.kdpt_default_options.restype = None
    lib.kdpt_create.argtypes = [P(Scene), P(Options), C.c_int, P(C.c_void_p)]
    lib.kdpt_trace_iteration.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.kdpt_trace_iteration_async.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.kdpt_trace_iterations.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.kdpt_synchronize.argtypes = [C.c_void_p]
    lib.kdpt_read_image.argtypes = [C.c_void_p, P(C.c_float)]
    lib.kdpt_write_pbo.argtypes = [C.c_void_p, C.c_int, P(C.c_uint8)]
    lib.kdpt_reset.argtypes = [C.c_void_p]
    lib.kdpt_get_stats.argtypes = [C.c_void_p, P(Stats)]
    lib.kdpt_destroy.argtypes = [C.c_void_p]
    lib.kdpt_last_error.restype = C.c_char_p
    lib.kdpt_image_device_ptr.argtypes = [C.c_void_p, P(C.c_void_p)]
    lib.kdpt_debug_paths.argtypes = [C.c_void_p, C.c_int, C.c_int, P(PathSegment), P(C.c_int)]
    lib.kdpt_count_iteration.argtypes = [C.c_void_p, C.c_int, P(C.c_ulonglong)]
    if hasattr(lib, "kdpt_count_split"):  # diagnostic; absent from older builds used in A/B runs
        lib.kdpt_count_split.argtypes = [C.c_void_p, P(C.c_ulonglong)]
    lib.kdpt_wave_profile.argtypes = [C.c_void_p, P(C.c_ulonglong), C.c_int]
    lib.kdpt_selftest_math.argtypes = [P(C.c_float), C.c_int, P(C.c_float), P(C.c_float)]
    lib.kdpt_selftest_rng.argtypes = [P(C.c_int), C.c_int, C.c_int, P(C.c_float)]
    lib.kdpt_selftest_fresnel.argtypes = [P(C.c_float), C.c_int, C.c_float, P(C.c_float)]
    lib.kdpt_trace_config.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_longlong)]
    if hasattr(lib, "kdpt_cull_margin"):  # absent from older builds used in A/B runs
        lib.kdpt_cull_margin.argtypes = [C.c_void_p, P(C.c_float), P(C.c_double), P(C.c_int)]
    if hasattr(lib, "kdpt_shade_staged"):
        lib.kdpt_shade_staged.argtypes = [C.c_void_p, P(C.c_int)]
    if hasattr(lib, "kdpt_cull_masks"):
        lib.kdpt_cull_masks.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int), C.c_void_p]
    if hasattr(lib, "kdpt_render_frames"):
        lib.kdpt_comm_unique_id.argtypes = [C.c_void_p]
        lib.kdpt_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        if hasattr(lib, "kdpt_comm_library"):
            lib.kdpt_comm_library.argtypes = [C.c_char_p, C.c_int]
        lib.kdpt_render_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.kdpt_render_sharded.argtypes = [P(Scene), P(Options), C.c_int, P(C.c_int), C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.kdpt_selftest_rng_draws.argtypes = [C.c_int, P(C.c_uint32), C.c_int, C.c_int, P(C.c_float)]
    if hasattr(lib, "kdpt_selftest_libm"):  # absent from older builds used in A/B runs
        lib.kdpt_selftest_libm.argtypes = [C.c_int, P(C.c_float), C.c_int, P(C.c_double)]
        lib.kdpt_selftest_libm_digest.argtypes = [C.c_int, C.c_uint32, C.c_ulonglong, P(C.c_ulonglong)]
    lib.kdpt_scene_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, P(C.c_void_p)]
    lib.kdpt_scene_build.argtypes = [P(SceneDesc), P(C.c_void_p)]
    lib.kdpt_scene_view.argtypes = [C.c_void_p, P(Scene)]
    lib.kdpt_scene_free.argtypes = [C.c_void_p]
    lib.kdpt_save_rgb8.argtypes = [C.c_void_p, C.c_float, P(C.c_uint8)]
    lib.kdpt_save_png.argtypes = [C.c_void_p, C.c_char_p, C.c_float]
    lib.kdpt_save_hdr.argtypes = [C.c_void_p, C.c_char_p, C.c_float]
    lib.kdpt_png_encode.argtypes = [P(C.c_uint8), C.c_int, C.c_int, P(P(C.c_uint8)), P(C.c_size_t)]
    lib.kdpt_write_png.argtypes = [C.c_char_p, P(C.c_uint8), C.c_int, C.c_int]
    lib.kdpt_hdr_encode.argtypes = [P(C.c_float), C.c_int, C.c_int, P(P(C.c_uint8)), P(C.c_size_t)]
    lib.kdpt_write_hdr.argtypes = [C.c_char_p, P(C.c_float), C.c_int, C.c_int]
    lib.kdpt_free.argtypes = [C.c_void_p]
    lib.kdpt_free.restype = None
    if hasattr(lib, "kdpt_scene_build_device"):
        lib.kdpt_scene_build_device.argtypes = [P(SceneDesc), C.c_int, P(C.c_void_p)]
        lib.kdpt_scene_kd_build_ms.argtypes = [C.c_void_p, P(C.c_double)]
        lib.kdpt_scene_load_device.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                               P(C.c_void_p)]
        lib.kdpt_build_kd_device.argtypes = [P(C.c_float), P(C.c_float), P(C.c_int), C.c_int, C.c_int, C.c_int,
                                             P(C.c_void_p), P(C.c_int), P(C.c_void_p), P(C.c_int), P(C.c_double)]
    if hasattr(lib, "kdpt_set_options"):
        lib.kdpt_set_options.argtypes = [C.c_void_p, P(Options)]
    if hasattr(lib, "kdpt_selftest_glm"):
        lib.kdpt_selftest_glm.argtypes = [C.c_int, P(C.c_float), C.c_int, P(C.c_float)]
    if hasattr(lib, "kdpt_selftest_scatter"):  # absent from older builds used in A/B runs
        lib.kdpt_selftest_scatter.argtypes = [P(C.c_float), C.c_int, P(C.c_float)]
        lib.kdpt_selftest_shade.argtypes = [P(C.c_float), C.c_int, P(C.c_float)]
    if hasattr(lib, "kdpt_set_tuning"):  # absent from older builds used in A/B runs
        lib.kdpt_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    if hasattr(lib, "kdpt_cast_rays"):  # absent from older builds used in A/B runs
        lib.kdpt_cast_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
        lib.kdpt_cast_stats.argtypes = [C.c_void_p, P(C.c_longlong), P(C.c_longlong), P(C.c_double)]
    if hasattr(lib, "kdpt_trace_rays"):  # absent from older builds used in A/B runs
        lib.kdpt_set_camera.argtypes = [C.c_void_p, P(Camera)]
        lib.kdpt_camera_rays.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.kdpt_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p]
        lib.kdpt_trace_rays_stats.argtypes = [C.c_void_p, P(C.c_longlong), P(C.c_longlong), P(C.c_double)]
    if hasattr(lib, "kdpt_set_moments"):  # absent from older builds used in A/B runs
        lib.kdpt_set_moments.argtypes = [C.c_void_p, C.c_int]
        lib.kdpt_read_moments.argtypes = [C.c_void_p, P(C.c_float), P(C.c_longlong)]
        lib.kdpt_noise_map.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
        lib.kdpt_noise_estimate.argtypes = [C.c_void_p, C.c_float, C.c_float, P(Noise)]
        lib.kdpt_trace_rays_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int,
                                                C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(lib, "kdpt_trace_adaptive"):  # absent from older builds used in A/B runs
        lib.kdpt_active_pixels.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p, P(C.c_longlong)]
        lib.kdpt_trace_adaptive.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                            P(Adaptive)]
        lib.kdpt_read_sample_counts.argtypes = [C.c_void_p, P(C.c_int)]
        lib.kdpt_save_counted.argtypes = [C.c_void_p, P(C.c_uint8), P(C.c_float)]
        lib.kdpt_selftest_active_list.argtypes = [P(C.c_float), C.c_int, C.c_float, P(C.c_int), P(C.c_int)]
    if hasattr(lib, "kdpt_group_create"):  # absent from older builds used in A/B runs
        lib.kdpt_group_create.argtypes = [P(Scene), P(Options), C.c_int, P(C.c_int), C.c_int, C.c_int, P(C.c_void_p)]
        lib.kdpt_group_render_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.kdpt_group_synchronize.argtypes = [C.c_void_p]
        lib.kdpt_group_context.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p)]
        lib.kdpt_group_active_pixels.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p, P(C.c_longlong)]
        lib.kdpt_group_trace_adaptive.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                                  C.c_float, P(Adaptive)]
        lib.kdpt_group_set_camera.argtypes = [C.c_void_p, P(Camera)]
        lib.kdpt_group_set_options.argtypes = [C.c_void_p, P(Options)]
        lib.kdpt_group_reset.argtypes = [C.c_void_p]
        lib.kdpt_group_destroy.argtypes = [C.c_void_p]
    if hasattr(lib, "kdpt_denoise"):  # absent from older builds used in A/B runs
        lib.kdpt_default_denoise_params.argtypes = [P(DenoiseParams)]
        lib.kdpt_default_denoise_params.restype = None
        lib.kdpt_denoise_buffers.argtypes = [C.c_int, C.c_int, C.c_int, P(C.c_float), P(C.c_float), P(C.c_float),
                                             P(C.c_float), P(C.c_float), P(C.c_int), P(DenoiseParams), P(C.c_float),
                                             P(C.c_float)]
        lib.kdpt_denoise.argtypes = [C.c_void_p, P(DenoiseParams), C.c_void_p, C.c_void_p]
        lib.kdpt_denoise_stats.argtypes = [C.c_void_p, P(C.c_double), P(C.c_double)]
    if hasattr(lib, "kdpt_denoise_temporal"):  # absent from older builds used in A/B runs
        lib.kdpt_default_temporal_params.argtypes = [P(TemporalParams)]
        lib.kdpt_default_temporal_params.restype = None
        lib.kdpt_temporal_buffers.argtypes = (
            [C.c_int, C.c_int, C.c_int] +
            [P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_int)] +
            [P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_int), P(C.c_float)] +
            [P(Camera), P(TemporalParams), P(C.c_float), P(C.c_float), P(C.c_float)])
        lib.kdpt_denoise_temporal.argtypes = [C.c_void_p, P(TemporalParams), P(DenoiseParams), C.c_void_p, C.c_void_p]
        lib.kdpt_temporal_reset.argtypes = [C.c_void_p]
        lib.kdpt_temporal_stats.argtypes = [C.c_void_p, P(C.c_double), P(C.c_double), P(C.c_double),
                                            P(C.c_longlong), P(C.c_longlong)]
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != KDPT_OK:
        msg = load_library().kdpt_last_error().decode(errors="replace")
        raise KdptError(f"{what} failed ({rc}): {msg}")


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _iptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int))


MATERIAL_DTYPE = np.dtype([("color", "<f4", 3), ("specular_exponent", "<f4"), ("specular_color", "<f4", 3),
                           ("hasReflective", "<f4"), ("hasRefractive", "<f4"), ("indexOfRefraction", "<f4"),
                           ("emittance", "<f4"), ("transmittance", "<f4", 3)])
assert MATERIAL_DTYPE.itemsize == 56


@dataclass
class SceneDescription:
    """What the reference's parsers produce before any matrix/camera/KD work."""
    res: tuple
    fovy: float
    iterations: int
    trace_depth: int
    eye: np.ndarray
    look_at: np.ndarray
    up: np.ndarray
    materials: np.ndarray          # MATERIAL_DTYPE[nm]
    geom_type: np.ndarray          # int32[ng]
    geom_material: np.ndarray      # int32[ng]
    geom_trs: np.ndarray           # float32[ng, 9]
    verts9: Optional[np.ndarray] = None   # float32[ntri, 9]
    norms9: Optional[np.ndarray] = None   # float32[ntri, 9]
    shape_of_tri: Optional[np.ndarray] = None  # int32[ntri]
    shape_materials: Optional[np.ndarray] = None  # MATERIAL_DTYPE[nshapes]
    kd_max_depth: int = 13                 # KDtree::split(13) in Scene::loadObj (src/scene.cpp:868-872)

    def with_overrides(self, res=None, depth=None) -> "SceneDescription":
        import dataclasses
        d = dataclasses.replace(self)
        if res is not None:
            d.res = (int(res[0]), int(res[1]))
        if depth is not None:
            d.trace_depth = int(depth)
        return d

    def to_c(self):
        """Build a SceneDesc (the numpy arrays it points into are returned to keep them alive)."""
        keep = []

        def arr(x, dt):
            a = np.ascontiguousarray(x, dtype=dt)
            keep.append(a)
            return a

        mats = arr(self.materials, MATERIAL_DTYPE)
        d = SceneDesc()
        d.res[0], d.res[1] = int(self.res[0]), int(self.res[1])
        d.fovy = float(np.float32(self.fovy))
        d.iterations = int(self.iterations)
        d.traceDepth = int(self.trace_depth)
        for i in range(3):
            d.eye[i], d.lookAt[i], d.up[i] = float(self.eye[i]), float(self.look_at[i]), float(self.up[i])
        d.num_materials = len(mats)
        d.materials = mats.ctypes.data_as(C.POINTER(Material))
        gt, gm, gtrs = arr(self.geom_type, np.int32), arr(self.geom_material, np.int32), arr(self.geom_trs, np.float32)
        d.num_geoms = len(gt)
        d.geom_type, d.geom_material, d.geom_trs = _iptr(gt), _iptr(gm), _fptr(gtrs)
        if self.verts9 is not None and len(self.verts9):
            v9, n9 = arr(self.verts9, np.float32), arr(self.norms9, np.float32)
            st, sm = arr(self.shape_of_tri, np.int32), arr(self.shape_materials, MATERIAL_DTYPE)
            d.ntri = len(st)
            d.verts9, d.norms9, d.shape_of_tri = _fptr(v9), _fptr(n9), _iptr(st)
            d.num_shapes = len(sm)
            d.shape_materials = sm.ctypes.data_as(C.POINTER(Material))
        d.kd_max_depth = int(self.kd_max_depth)
        return d, keep


class SceneData:
    """A built scene (Scene::geoms/materials/newNodesBare/newTrianglesBare + camera), owned by libkdpt."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        self.view = Scene()
        _check(load_library().kdpt_scene_view(self._h, C.byref(self.view)), "kdpt_scene_view")

    @classmethod
    def from_files(cls, scene_path: str, obj_path: Optional[str] = None, res=None, depth=None,
                   kd_device: Optional[int] = None) -> "SceneData":
        """kdpt_scene_load (host KD build) or kdpt_scene_load_device (KD tree built on GPU kd_device)."""
        lib = load_library()
        h = C.c_void_p()
        w, hh = (res if res is not None else (0, 0))
        if kd_device is None:
            rc = lib.kdpt_scene_load(scene_path.encode(), obj_path.encode() if obj_path else None, int(w), int(hh),
                                     int(depth or 0), C.byref(h))
        else:
            rc = lib.kdpt_scene_load_device(scene_path.encode(), obj_path.encode() if obj_path else None, int(w),
                                            int(hh), int(depth or 0), int(kd_device), C.byref(h))
        _check(rc, f"kdpt_scene_load({scene_path}, {obj_path})")
        return cls(h)

    @classmethod
    def from_description(cls, desc: SceneDescription, kd_device: Optional[int] = None) -> "SceneData":
        """kdpt_scene_build (host KD build), or kdpt_scene_build_device with the KD tree built on GPU
        `kd_device` (byte-identical)."""
        lib = load_library()
        d, keep = desc.to_c()
        h = C.c_void_p()
        if kd_device is None:
            _check(lib.kdpt_scene_build(C.byref(d), C.byref(h)), "kdpt_scene_build")
        else:
            _check(lib.kdpt_scene_build_device(C.byref(d), int(kd_device), C.byref(h)), "kdpt_scene_build_device")
        del keep
        return cls(h)

    def kd_build_ms(self) -> float:
        ms = C.c_double()
        _check(load_library().kdpt_scene_kd_build_ms(self._h, C.byref(ms)), "kdpt_scene_kd_build_ms")
        return float(ms.value)

    @property
    def resolution(self):
        return int(self.view.camera.resolution[0]), int(self.view.camera.resolution[1])

    def nodes_bytes(self) -> bytes:
        return C.string_at(self.view.nodes, C.sizeof(NodeBare) * self.view.num_nodes)

    def tris_bytes(self) -> bytes:
        return C.string_at(self.view.tris, C.sizeof(TriBare) * self.view.num_tris)

    def geoms_bytes(self) -> bytes:
        return C.string_at(self.view.geoms, C.sizeof(Geom) * self.view.num_geoms)

    def materials_bytes(self) -> bytes:
        return C.string_at(self.view.materials, C.sizeof(Material) * self.view.num_materials)

    def camera_bytes(self) -> bytes:
        return bytes(self.view.camera)

    def close(self):
        if self._h:
            load_library().kdpt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _encoded(fn, ptr, w, h, what) -> bytes:
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t()
    _check(fn(ptr, int(w), int(h), C.byref(out), C.byref(n)), what)
    try:
        return C.string_at(out, n.value)
    finally:
        load_library().kdpt_free(out)


def png_encode(rgb: np.ndarray) -> bytes:
    """PNG bytes of an (H, W, 3) uint8 image, as stb_image_write's stbi_write_png encodes them."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    return _encoded(load_library().kdpt_png_encode, rgb.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, "kdpt_png_encode")


def hdr_encode(rgb: np.ndarray) -> bytes:
    """Radiance .hdr bytes of an (H, W, 3) float32 image, as stb_image_write's stbi_write_hdr writes them."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[:2]
    return _encoded(load_library().kdpt_hdr_encode, _fptr(rgb), w, h, "kdpt_hdr_encode")


def default_options(**overrides) -> Options:
    o = Options()
    load_library().kdpt_default_options(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def default_denoise_params(**overrides) -> DenoiseParams:
    """kdpt_default_denoise_params: 5 passes, cos^128 normals, sigma_l 4, sigma_z 0.02, eps_l 1e-8."""
    p = DenoiseParams()
    load_library().kdpt_default_denoise_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def denoise_buffers(color, variance, normal, point, depth, ids, params: Optional[DenoiseParams] = None,
                    device: int = 0, return_variance: bool = False):
    """kdpt_denoise_buffers: the filter alone on caller data -- color, normal, point (H, W, 3) float32, variance and
    depth (H, W) float32, ids (H, W) int32 -- on `device`.  Returns the filtered colour (H, W, 3), or (colour,
    variance) with return_variance."""
    col = np.ascontiguousarray(color, dtype=np.float32)
    if col.ndim != 3 or col.shape[2] != 3:
        raise ValueError(f"color: expected (H, W, 3), got {col.shape}")
    h, w = col.shape[:2]
    var, dep = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (variance, depth))
    nrm, pnt = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (normal, point))
    idv = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    for name, a, n in (("variance", var, 1), ("depth", dep, 1), ("ids", idv, 1), ("normal", nrm, 3), ("point", pnt, 3)):
        if a.size != n * w * h:
            raise ValueError(f"{name}: {a.size} values for a {w} x {h} image")
    p = params if params is not None else default_denoise_params()
    out = np.empty((h, w, 3), dtype=np.float32)
    ov = np.empty((h, w), dtype=np.float32) if return_variance else None
    _check(load_library().kdpt_denoise_buffers(int(device), w, h, _fptr(col), _fptr(var), _fptr(nrm), _fptr(pnt),
                                               _fptr(dep), _iptr(idv), C.byref(p), _fptr(out),
                                               _fptr(ov) if return_variance else None), "kdpt_denoise_buffers")
    return (out, ov) if return_variance else out


def default_temporal_params(**overrides) -> TemporalParams:
    """kdpt_default_temporal_params: alpha 0.2, sigma_z 0.02, normal_min 0.9, max_history 32."""
    p = TemporalParams()
    load_library().kdpt_default_temporal_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _frame_arrays(what, color, variance, normal, point, depth, ids, shape=None):
    col = np.ascontiguousarray(color, dtype=np.float32)
    if col.ndim != 3 or col.shape[2] != 3:
        raise ValueError(f"{what}color: expected (H, W, 3), got {col.shape}")
    h, w = col.shape[:2]
    if shape is not None and (h, w) != shape:
        raise ValueError(f"{what}color: {w} x {h} beside a {shape[1]} x {shape[0]} frame")
    var, dep = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (variance, depth))
    nrm, pnt = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (normal, point))
    idv = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    for name, a, n in (("variance", var, 1), ("depth", dep, 1), ("ids", idv, 1), ("normal", nrm, 3), ("point", pnt, 3)):
        if a.size != n * w * h:
            raise ValueError(f"{what}{name}: {a.size} values for a {w} x {h} image")
    return (h, w), (col, var, nrm, pnt, dep, idv)


def temporal_buffers(color, variance, normal, point, depth, ids, history=None, params: Optional[TemporalParams] = None,
                     device: int = 0):
    """kdpt_temporal_buffers: the temporal stage alone on caller data -- the current frame as denoise_buffers takes
    it, and `history`, None or (color, variance, normal, point, depth, ids, length, camera): the previous frame's
    arrays of the same shapes, its lengths (H, W) float32 and the Camera it was made under.  Returns (colour (H, W, 3),
    variance (H, W), length (H, W)): the blended frame, which with the current guides and camera is the next call's
    history."""
    (h, w), cur = _frame_arrays("", color, variance, normal, point, depth, ids)
    p = params if params is not None else default_temporal_params()
    hist, cam = [None] * 7, None
    if history is not None:
        _, ha = _frame_arrays("history ", *history[:6], shape=(h, w))
        ln = np.ascontiguousarray(history[6], dtype=np.float32).reshape(-1)
        if ln.size != w * h:
            raise ValueError(f"history length: {ln.size} values for a {w} x {h} image")
        hist = [_fptr(a) for a in ha[:5]] + [_iptr(ha[5]), _fptr(ln)]
        cam = C.byref(history[7])
    out = np.empty((h, w, 3), dtype=np.float32)
    ov, ol = np.empty((h, w), dtype=np.float32), np.empty((h, w), dtype=np.float32)
    _check(load_library().kdpt_temporal_buffers(int(device), w, h, *[_fptr(a) for a in cur[:5]], _iptr(cur[5]), *hist,
                                                cam, C.byref(p), _fptr(out), _fptr(ov), _fptr(ol)),
           "kdpt_temporal_buffers")
    return out, ov, ol


def orbit_camera(camera: Camera, degrees: float) -> Camera:
    """A copy of `camera` turned about its lookAt point around its `up` axis by `degrees` (a turntable step).  With
    k = up / |up|, v = position - lookAt and t = radians(degrees), Rodrigues' formula in float32:
        v' = v cos t + (k x v) sin t + k (k . v) (1 - cos t);   position' = lookAt + v'
    then view' = normalize(lookAt - position') and right' = normalize(cross(view', up)), as the scene loader makes
    them.  up, lookAt, resolution, fov and pixelLength are kept."""
    f32 = np.float32
    out = Camera.from_buffer_copy(bytes(camera))
    pos, look, up = (np.array(a[:], f32) for a in (camera.position, camera.lookAt, camera.up))
    k = up / f32(np.sqrt(np.dot(up, up)))
    v = pos - look
    t = np.deg2rad(f32(degrees)).astype(f32)
    c, s = f32(np.cos(t)), f32(np.sin(t))
    v2 = (v * c + np.cross(k, v).astype(f32) * s + k * (f32(np.dot(k, v)) * (f32(1) - c))).astype(f32)
    pos2 = (look + v2).astype(f32)
    view = look - pos2
    view = (view / f32(np.sqrt(np.dot(view, view)))).astype(f32)
    right = np.cross(view, up).astype(f32)
    right = (right / f32(np.sqrt(np.dot(right, right)))).astype(f32)
    for name, val in (("position", pos2), ("view", view), ("right", right)):
        setattr(out, name, (C.c_float * 3)(*[float(x) for x in val]))
    return out


class PathTracer:
    """One device context: pathtraceInit / pathtrace / pathtraceFree."""

    def __init__(self, scene: SceneData, options: Optional[Options] = None, device: int = 0):
        self.scene = scene
        self.lib = load_library()
        self.opt = options if options is not None else default_options()
        self._ctx = C.c_void_p()
        _check(self.lib.kdpt_create(C.byref(scene.view), C.byref(self.opt), int(device), C.byref(self._ctx)),
               "kdpt_create")
        self.width, self.height = scene.resolution

    def trace_iteration(self, iteration: int, frame: int = 0):
        _check(self.lib.kdpt_trace_iteration(self._ctx, int(frame), int(iteration)), "kdpt_trace_iteration")

    def trace_iteration_async(self, iteration: int, frame: int = 0):
        _check(self.lib.kdpt_trace_iteration_async(self._ctx, int(frame), int(iteration)), "kdpt_trace_iteration_async")

    def trace_iterations(self, first: int, count: int, stride: int = 1, pipeline: int = 3, batch: int = 1,
                         frame: int = 0):
        """Iterations first + k*stride (k < count): batches of `batch` sharing each intersect launch,
        `pipeline` batches in flight (kdpt_trace_iterations; async)."""
        _check(self.lib.kdpt_trace_iterations(self._ctx, int(frame), int(first), int(count), int(stride),
                                              int(pipeline), int(batch)), "kdpt_trace_iterations")

    def synchronize(self):
        _check(self.lib.kdpt_synchronize(self._ctx), "kdpt_synchronize")

    def comm_init(self, nranks: int, rank: int, comm_id: Optional[bytes]):
        """kdpt_comm_init: join an spp-sharded group (comm_id from comm_unique_id() on rank 0; None = no
        communicator, render_frames hands each rank's frame shares out for the caller to reduce)."""
        buf = None if comm_id is None else C.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        _check(self.lib.kdpt_comm_init(self._ctx, int(nranks), int(rank), buf), "kdpt_comm_init")

    def render_frames(self, first_frame: int, frames: int, spp: int, pipeline: int = 8, batch: int = 8,
                      out=None):
        """kdpt_render_frames (async): this rank's share of frames of `spp` global iterations each, reduced
        to rank 0 and added into its image; out: None, a device pointer (int) or a float32 numpy array of
        frames * 3*W*H values (host copies complete at synchronize())."""
        ptr = None if out is None else (int(out) if isinstance(out, int) else out.ctypes.data)
        _check(self.lib.kdpt_render_frames(self._ctx, int(first_frame), int(frames), int(spp), int(pipeline),
                                           int(batch), ptr), "kdpt_render_frames")

    def image(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 3), dtype=np.float32)
        _check(self.lib.kdpt_read_image(self._ctx, _fptr(out)), "kdpt_read_image")
        return out

    def pbo(self, iteration: int) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        _check(self.lib.kdpt_write_pbo(self._ctx, int(iteration), out.ctypes.data_as(C.POINTER(C.c_uint8))),
               "kdpt_write_pbo")
        return out

    def set_options(self, options: Options):
        """kdpt_set_options: pathtrace()'s per-call flags for the next iterations (same context)."""
        _check(self.lib.kdpt_set_options(self._ctx, C.byref(options)), "kdpt_set_options")
        self.opt = options

    def set_tuning(self, name: str, value: float):
        """kdpt_set_tuning: an explicit A/B or diagnostic knob (the library reads no environment); the names
        are listed at kdpt_set_tuning in include/kdpt.h, e.g. "cast_chunk" (rays per chunk of cast_rays,
        default 1 << 20, at least 64)."""
        _check(self.lib.kdpt_set_tuning(self._ctx, name.encode(), float(value)), f"kdpt_set_tuning({name})")

    def cast_rays(self, origins, directions, normalize: bool = True) -> np.ndarray:
        """kdpt_cast_rays on host arrays: the closest hit of each ray (origins, directions: n x 3 float32), as a
        RAY_HIT_DTYPE array of n records -- what the path tracer's intersect stage computes for that ray.
        normalize=True applies the reference's glm::normalize to each direction; otherwise directions must be
        unit length (|dot(d, d) - 1| <= 1e-6) or the ray is rejected (kind HIT_INVALID)."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError(f"{len(o)} origins but {len(d)} directions")
        out = np.empty(len(o), dtype=RAY_HIT_DTYPE)
        self.cast_rays_ptr(o.ctypes.data, d.ctypes.data, len(o), out.ctypes.data, normalize=normalize)
        return out

    def cast_rays_ptr(self, origins_ptr: int, directions_ptr: int, n: int, out_ptr: int, normalize: bool = True):
        """kdpt_cast_rays on raw pointers, each host memory or memory of the context's device (e.g. a torch
        tensor's data_ptr()): 3 n floats, 3 n floats, n 40-byte records.  Synchronous."""
        _check(self.lib.kdpt_cast_rays(self._ctx, C.c_void_p(int(origins_ptr)), C.c_void_p(int(directions_ptr)),
                                       int(n), CAST_NORMALIZE if normalize else 0, C.c_void_p(int(out_ptr))),
               "kdpt_cast_rays")

    def cast_stats(self) -> "CastStats":
        """kdpt_cast_stats: rays cast and rays that reached the KD traversal kernel since create/reset, and the
        last cast's device time in ms."""
        r, t, ms = C.c_longlong(), C.c_longlong(), C.c_double()
        _check(self.lib.kdpt_cast_stats(self._ctx, C.byref(r), C.byref(t), C.byref(ms)), "kdpt_cast_stats")
        return CastStats(int(r.value), int(t.value), float(ms.value))

    def set_camera(self, camera):
        """kdpt_set_camera: the pinhole camera of the iterations enqueued from now on (a Camera, or a SceneData
        whose camera is taken).  Its resolution must be the context's; the image, stats and iteration counter are
        kept (reset() clears them)."""
        cam = camera.view.camera if isinstance(camera, SceneData) else camera
        _check(self.lib.kdpt_set_camera(self._ctx, C.byref(cam)), "kdpt_set_camera")

    def camera_rays(self, iteration: int):
        """kdpt_camera_rays: the W*H rays the device generates for `iteration` with the context's current camera
        and options, as (origins, directions), each (W*H, 3) float32 with index = y*W + x."""
        n = self.width * self.height
        o, d = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        self.camera_rays_ptr(iteration, o.ctypes.data, d.ctypes.data)
        return o, d

    def camera_rays_ptr(self, iteration: int, origins_ptr: int, directions_ptr: int):
        """kdpt_camera_rays into raw pointers (host memory or memory of the context's device): 3*W*H floats each."""
        _check(self.lib.kdpt_camera_rays(self._ctx, int(iteration), C.c_void_p(int(origins_ptr)),
                                         C.c_void_p(int(directions_ptr))), "kdpt_camera_rays")

    def trace_rays(self, origins, directions, first_iter: int = 1, count: int = 1,
                   normalize: bool = True, moments: bool = False):
        """kdpt_trace_rays on host arrays: the radiance the path tracer gathers for each of n <= W*H rays
        (origins, directions: n x 3 float32), summed over iterations first_iter .. first_iter + count - 1, as an
        (n, 3) float32 array.  Ray i is traced as pixel i of an n-pixel image whose camera produced these rays.
        normalize as in cast_rays; a rejected ray's radiance is NaN in all three channels.
        moments=True (kdpt_trace_rays_moments) returns (radiance, sumsq): sumsq is the sum over the iterations of
        the squared per-iteration contributions, same shape, for per-ray error bars."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError(f"{len(o)} origins but {len(d)} directions")
        out = np.empty((len(o), 3), dtype=np.float32)
        if moments:
            sq = np.empty((len(o), 3), dtype=np.float32)
            self.trace_rays_moments_ptr(o.ctypes.data, d.ctypes.data, len(o), out.ctypes.data, sq.ctypes.data,
                                        first_iter=first_iter, count=count, normalize=normalize)
            return out, sq
        self.trace_rays_ptr(o.ctypes.data, d.ctypes.data, len(o), out.ctypes.data, first_iter=first_iter,
                            count=count, normalize=normalize)
        return out

    def trace_rays_moments_ptr(self, origins_ptr: int, directions_ptr: int, n: int, radiance_ptr: int,
                               sumsq_ptr: int, first_iter: int = 1, count: int = 1, normalize: bool = True):
        """kdpt_trace_rays_moments on raw pointers, each host memory or memory of the context's device: 3 n floats
        each.  Synchronous."""
        _check(self.lib.kdpt_trace_rays_moments(self._ctx, C.c_void_p(int(origins_ptr)),
                                                C.c_void_p(int(directions_ptr)), int(n), int(first_iter), int(count),
                                                CAST_NORMALIZE if normalize else 0, C.c_void_p(int(radiance_ptr)),
                                                C.c_void_p(int(sumsq_ptr))), "kdpt_trace_rays_moments")

    def set_moments(self, on: bool = True):
        """kdpt_set_moments: keep (or drop) the per-pixel sum of squares beside the image.  Turning it on is
        accepted only on a context nothing has been accumulated into since create / reset()."""
        _check(self.lib.kdpt_set_moments(self._ctx, 1 if on else 0), "kdpt_set_moments")

    def moments(self):
        """kdpt_read_moments: (sumsq, samples) -- the (H*W, 3) float32 sum over the accumulated iterations of the
        squared per-iteration pixel values, and the number of those iterations."""
        sq = np.empty((self.height * self.width, 3), dtype=np.float32)
        n = C.c_longlong()
        _check(self.lib.kdpt_read_moments(self._ctx, _fptr(sq), C.byref(n)), "kdpt_read_moments")
        return sq, int(n.value)

    def noise_map(self, floor: float = 1e-2, out_ptr: Optional[int] = None):
        """kdpt_noise_map: the per-pixel relative standard error of the mean, (H, W) float32 (formula in
        include/kdpt.h).  out_ptr: write W*H floats to that raw pointer (host or the context's device) instead and
        return None."""
        if out_ptr is not None:
            _check(self.lib.kdpt_noise_map(self._ctx, float(floor), C.c_void_p(int(out_ptr))), "kdpt_noise_map")
            return None
        out = np.empty((self.height, self.width), dtype=np.float32)
        _check(self.lib.kdpt_noise_map(self._ctx, float(floor), C.c_void_p(out.ctypes.data)), "kdpt_noise_map")
        return out

    def noise_estimate(self, floor: float = 1e-2, threshold: float = 0.0) -> Noise:
        """kdpt_noise_estimate: the noise map reduced on the device (samples, pixels, above, nonfinite, mean,
        max); deterministic, for stopping rules."""
        r = Noise()
        _check(self.lib.kdpt_noise_estimate(self._ctx, float(floor), float(threshold), C.byref(r)),
               "kdpt_noise_estimate")
        return r

    def active_pixels(self, floor: float = 1e-2, threshold: float = 0.0, out_ptr: Optional[int] = None):
        """kdpt_active_pixels: the indices (y*W + x, ascending, int32) of the pixels whose noise is finite and above
        `threshold` -- the list kdpt_trace_adaptive would trace.  out_ptr: write them to that raw pointer (W*H ints of
        host memory or of the context's device) instead and return their number."""
        n = C.c_longlong()
        if out_ptr is not None:
            _check(self.lib.kdpt_active_pixels(self._ctx, float(floor), float(threshold), C.c_void_p(int(out_ptr)),
                                               C.byref(n)), "kdpt_active_pixels")
            return int(n.value)
        out = np.empty(self.height * self.width, dtype=np.int32)
        _check(self.lib.kdpt_active_pixels(self._ctx, float(floor), float(threshold), C.c_void_p(out.ctypes.data),
                                           C.byref(n)), "kdpt_active_pixels")
        return out[:int(n.value)].copy()

    def trace_adaptive(self, first_iter: int, count: int, pipeline: int = 8, batch: int = 16, floor: float = 1e-2,
                       threshold: float = 0.0) -> Adaptive:
        """kdpt_trace_adaptive: iterations first_iter .. first_iter + count - 1 over the active pixels only (noise
        finite and above `threshold`), added into the image, the second moments and the per-pixel sample counts.
        Synchronous; returns the call's kdpt_adaptive record."""
        r = Adaptive()
        _check(self.lib.kdpt_trace_adaptive(self._ctx, int(first_iter), int(count), int(pipeline), int(batch),
                                            float(floor), float(threshold), C.byref(r)), "kdpt_trace_adaptive")
        return r

    def sample_counts(self) -> np.ndarray:
        """kdpt_read_sample_counts: the samples per pixel, (H, W) int32 (uniform iterations + adaptive ones)."""
        out = np.empty((self.height, self.width), dtype=np.int32)
        _check(self.lib.kdpt_read_sample_counts(self._ctx, out.ctypes.data_as(C.POINTER(C.c_int))),
               "kdpt_read_sample_counts")
        return out

    def save_counted(self, lin: bool = False):
        """kdpt_save_counted: save_rgb8's bytes with every pixel divided by its own sample count, (H, W, 3) uint8;
        lin=True returns (rgb, lin), lin being the (H, W, 3) float32 image save_hdr would write."""
        rgb = np.empty((self.height, self.width, 3), dtype=np.uint8)
        flt = np.empty((self.height, self.width, 3), dtype=np.float32) if lin else None
        _check(self.lib.kdpt_save_counted(self._ctx, rgb.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          _fptr(flt) if lin else None), "kdpt_save_counted")
        return (rgb, flt) if lin else rgb

    def denoise(self, params: Optional[DenoiseParams] = None, variance: bool = False):
        """kdpt_denoise: the render's per-pixel means through the variance-guided edge-avoiding filter (include/kdpt.h
        "Denoising"), (H, W, 3) float32; variance=True returns (colour, variance), the latter (H, W) float32: the
        filtered variance of the means.  Needs moments and at least 2 iterations; leaves the render state alone."""
        p = params if params is not None else default_denoise_params()
        col = np.empty((self.height, self.width, 3), dtype=np.float32)
        var = np.empty((self.height, self.width), dtype=np.float32) if variance else None
        _check(self.lib.kdpt_denoise(self._ctx, C.byref(p), C.c_void_p(col.ctypes.data),
                                     C.c_void_p(var.ctypes.data) if variance else None), "kdpt_denoise")
        return (col, var) if variance else col

    def denoise_ptr(self, params: Optional[DenoiseParams], color_ptr: int, variance_ptr: Optional[int] = None):
        """kdpt_denoise into raw pointers (host memory or the context's device): 3*W*H floats, and W*H floats."""
        p = params if params is not None else default_denoise_params()
        _check(self.lib.kdpt_denoise(self._ctx, C.byref(p), C.c_void_p(int(color_ptr)),
                                     C.c_void_p(int(variance_ptr)) if variance_ptr is not None else None),
               "kdpt_denoise")

    def denoise_stats(self) -> "DenoiseStats":
        """kdpt_denoise_stats: the last denoise's device times in ms (guides, filter)."""
        g, f = C.c_double(), C.c_double()
        _check(self.lib.kdpt_denoise_stats(self._ctx, C.byref(g), C.byref(f)), "kdpt_denoise_stats")
        return DenoiseStats(g.value, f.value)

    def denoise_temporal(self, tparams: Optional[TemporalParams] = None, dparams: Optional[DenoiseParams] = None,
                         variance: bool = False):
        """kdpt_denoise_temporal: denoise() with the previous call's result reprojected into this frame first
        (include/kdpt.h "Temporal accumulation"): (H, W, 3) float32, or (colour, variance) with variance=True.  The
        call stores this frame as the next one's history; the history survives reset(), set_camera() and
        set_options(), so a frame of a camera path is "set_camera, reset, trace, denoise_temporal"."""
        tp = tparams if tparams is not None else default_temporal_params()
        dp = dparams if dparams is not None else default_denoise_params()
        col = np.empty((self.height, self.width, 3), dtype=np.float32)
        var = np.empty((self.height, self.width), dtype=np.float32) if variance else None
        _check(self.lib.kdpt_denoise_temporal(self._ctx, C.byref(tp), C.byref(dp), C.c_void_p(col.ctypes.data),
                                              C.c_void_p(var.ctypes.data) if variance else None),
               "kdpt_denoise_temporal")
        return (col, var) if variance else col

    def denoise_temporal_ptr(self, tparams: Optional[TemporalParams], dparams: Optional[DenoiseParams],
                             color_ptr: int, variance_ptr: Optional[int] = None):
        """kdpt_denoise_temporal into raw pointers (host memory or the context's device): 3*W*H floats, W*H floats."""
        tp = tparams if tparams is not None else default_temporal_params()
        dp = dparams if dparams is not None else default_denoise_params()
        _check(self.lib.kdpt_denoise_temporal(self._ctx, C.byref(tp), C.byref(dp), C.c_void_p(int(color_ptr)),
                                              C.c_void_p(int(variance_ptr)) if variance_ptr is not None else None),
               "kdpt_denoise_temporal")

    def temporal_reset(self):
        """kdpt_temporal_reset: drop the history; the next denoise_temporal() equals denoise()."""
        _check(self.lib.kdpt_temporal_reset(self._ctx), "kdpt_temporal_reset")

    def temporal_stats(self) -> "TemporalStats":
        """kdpt_temporal_stats: the last denoise_temporal's device times in ms (guides, temporal stage, filter) and
        its counts of valid pixels and of those that found history."""
        g, t, f = C.c_double(), C.c_double(), C.c_double()
        v, w = C.c_longlong(), C.c_longlong()
        _check(self.lib.kdpt_temporal_stats(self._ctx, C.byref(g), C.byref(t), C.byref(f), C.byref(v), C.byref(w)),
               "kdpt_temporal_stats")
        return TemporalStats(g.value, t.value, f.value, int(v.value), int(w.value))

    def trace_rays_ptr(self, origins_ptr: int, directions_ptr: int, n: int, radiance_ptr: int, first_iter: int = 1,
                       count: int = 1, normalize: bool = True):
        """kdpt_trace_rays on raw pointers, each host memory or memory of the context's device (e.g. a torch
        tensor's data_ptr()): 3 n floats each.  Synchronous."""
        _check(self.lib.kdpt_trace_rays(self._ctx, C.c_void_p(int(origins_ptr)), C.c_void_p(int(directions_ptr)),
                                        int(n), int(first_iter), int(count), CAST_NORMALIZE if normalize else 0,
                                        C.c_void_p(int(radiance_ptr))), "kdpt_trace_rays")

    def trace_rays_stats(self) -> "TraceRaysStats":
        """kdpt_trace_rays_stats: the last trace_rays' segments, rays handed to the KD traversal kernel and device
        time in ms (the query's own totals: stats() never sees them)."""
        s, t, ms = C.c_longlong(), C.c_longlong(), C.c_double()
        _check(self.lib.kdpt_trace_rays_stats(self._ctx, C.byref(s), C.byref(t), C.byref(ms)), "kdpt_trace_rays_stats")
        return TraceRaysStats(int(s.value), int(t.value), float(ms.value))

    def reset(self):
        _check(self.lib.kdpt_reset(self._ctx), "kdpt_reset")

    def save_rgb8(self, samples: float) -> np.ndarray:
        """saveImage's bytes (src/main.cpp:1087-1108, src/image.cpp:22-35), computed on the GPU."""
        out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        _check(self.lib.kdpt_save_rgb8(self._ctx, float(samples), out.ctypes.data_as(C.POINTER(C.c_uint8))),
               "kdpt_save_rgb8")
        return out

    def save_png(self, path: str, samples: float):
        """image::savePNG of the current image: the PNG the reference writes (stb encoder, restated)."""
        _check(self.lib.kdpt_save_png(self._ctx, os.fsencode(path), float(samples)), "kdpt_save_png")

    def save_hdr(self, path: str, samples: float):
        """image::saveHDR (Radiance RGBE, stb encoder restated)."""
        _check(self.lib.kdpt_save_hdr(self._ctx, os.fsencode(path), float(samples)), "kdpt_save_hdr")

    def stats(self) -> Stats:
        s = Stats()
        _check(self.lib.kdpt_get_stats(self._ctx, C.byref(s)), "kdpt_get_stats")
        return s

    def image_device_ptr(self) -> int:
        p = C.c_void_p()
        _check(self.lib.kdpt_image_device_ptr(self._ctx, C.byref(p)), "kdpt_image_device_ptr")
        return int(p.value or 0)

    def debug_paths(self, iteration: int, stop_depth: int):
        n = self.width * self.height
        out = (PathSegment * n)()
        cnt = C.c_int()
        _check(self.lib.kdpt_debug_paths(self._ctx, int(iteration), int(stop_depth), out, C.byref(cnt)),
               "kdpt_debug_paths")
        return np.frombuffer(bytes(out), dtype=PATH_DTYPE)[: cnt.value].copy()

    def count_iteration(self, iteration: int):
        out = (C.c_ulonglong * 3)()
        _check(self.lib.kdpt_count_iteration(self._ctx, int(iteration), out), "kdpt_count_iteration")
        return int(out[0]), int(out[1]), int(out[2])

    TREE_MODES = {0: "hbm-64B", 1: "hbm-32B", 2: "lds-32B", 3: "lds-16B-derived", 4: "lds-16B-derived+hbm-clusters",
                  5: "lds-16B-derived+supers"}

    def trace_config(self) -> dict:
        """kdpt_trace_config: where the intersect kernel reads the tree, its workgroup, grid and LDS."""
        m, b, g, l = C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
        _check(self.lib.kdpt_trace_config(self._ctx, C.byref(m), C.byref(b), C.byref(g), C.byref(l)),
               "kdpt_trace_config")
        out = {"tree": self.TREE_MODES.get(m.value, str(m.value)), "block": b.value, "grid": g.value,
               "lds_tree_bytes": l.value}
        if hasattr(self.lib, "kdpt_cull_margin"):
            out.update(self.cull_margin())
        if hasattr(self.lib, "kdpt_cull_masks"):
            n, ncl = C.c_int(), C.c_int()
            _check(self.lib.kdpt_cull_masks(self._ctx, C.byref(n), C.byref(ncl), None), "kdpt_cull_masks")
            out["cull_mask_n"] = n.value
        if hasattr(self.lib, "kdpt_shade_staged"):
            st = C.c_int()
            _check(self.lib.kdpt_shade_staged(self._ctx, C.byref(st)), "kdpt_shade_staged")
            out["shade_staged"] = bool(st.value)  # the fused shading kernels' geoms and materials in LDS
        return out

    def cull_margin(self) -> dict:
        """kdpt_cull_margin: the cluster cull's margin coefficient, the scene's rigorous one, exact or not."""
        k, r, e = C.c_float(), C.c_double(), C.c_int()
        _check(self.lib.kdpt_cull_margin(self._ctx, C.byref(k), C.byref(r), C.byref(e)), "kdpt_cull_margin")
        return {"cull_margin": k.value, "cull_rigorous": r.value, "cull_exact": bool(e.value)}

    def cull_masks(self):
        """kdpt_cull_masks: (mask_n, masks) of the masked cull as the device built them, a bucket-major array of
        shape [6 mask_n^2, num_clusters]; (0, None) when the scene has none."""
        n, ncl = C.c_int(), C.c_int()
        _check(self.lib.kdpt_cull_masks(self._ctx, C.byref(n), C.byref(ncl), None), "kdpt_cull_masks")
        if n.value == 0:
            return 0, None
        masks = np.zeros((6 * n.value * n.value, ncl.value), np.uint64)
        _check(self.lib.kdpt_cull_masks(self._ctx, C.byref(n), C.byref(ncl), masks.ctypes.data), "kdpt_cull_masks")
        return n.value, masks

    def trace_grid_share(self) -> float:
        return float(self.stats().intersect_grid_share)

    def count_split(self):
        """(AABB tests made before the intersect kernel, segments handed to it) of the last count_iteration."""
        out = (C.c_ulonglong * 2)()
        _check(self.lib.kdpt_count_split(self._ctx, out), "kdpt_count_split")
        return int(out[0]), int(out[1])

    def wave_profile(self):
        """Cycle profile of the intersect kernel in the last count_iteration (kdpt_wave_profile)."""
        out = (C.c_ulonglong * 256)()
        n = self.lib.kdpt_wave_profile(self._ctx, out, 256)
        _check(0 if n > 0 else n, "kdpt_wave_profile")
        keys = ("node_trips", "node_cycles", "big_sweeps", "big_cycles", "small_phases", "small_rounds",
                "small_cycles", "final_cycles", "setup_cycles", "geom_cycles", "post_cycles", "node_lane_steps",
                "big_leaves", "big_clusters", "big_pass", "big_multi", "small_pairs", "node_leafwait_steps",
                "node_done_steps", "tail_cycles", "tail_node_done_steps", "big_supers", "big_cull_cycles",
                "chunks", "chunk_cycles", "aabb", "tri", "hit")
        prof = dict(zip(keys, (int(out[k]) for k in range(len(keys)))))
        k0 = len(keys)
        if n >= k0 + 64:
            prof["wave_life_10us"] = [int(out[k]) for k in range(k0, k0 + 64)]
        if n >= k0 + 144:
            prof["ray_steps_hist4"] = [int(out[k]) for k in range(k0 + 64, k0 + 128)]
            prof["chord_steps"] = [int(out[k]) for k in range(k0 + 128, k0 + 136)]
            prof["chord_rays"] = [int(out[k]) for k in range(k0 + 136, k0 + 144)]
        return prof

    _owner = None  # a view of a context someone else owns (RenderGroup.context): the owner, kept alive

    @classmethod
    def borrowed(cls, owner, scene: SceneData, options: Options, handle: C.c_void_p) -> "PathTracer":
        """A PathTracer over a context that `owner` owns: close() lets go of the handle and destroys nothing."""
        self = cls.__new__(cls)
        self.scene, self.lib, self.opt, self._ctx, self._owner = scene, load_library(), options, handle, owner
        self.width, self.height = scene.resolution
        return self

    def close(self):
        if self._ctx and self._owner is None:
            self.lib.kdpt_destroy(self._ctx)
        self._ctx = C.c_void_p()
        self._owner = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RenderGroup:
    """kdpt_group: one process, one context per device, kept alive between calls -- frames sharded over the ranks,
    with moments=True second moments through the reduce, the noise estimate on rank 0 and adaptive rounds across
    the ranks.  A context manager; close() destroys the group and every context."""

    def __init__(self, scene: SceneData, devices, options: Optional[Options] = None, reduce: int = REDUCE_RCCL,
                 moments: bool = False):
        self.scene = scene
        self.lib = load_library()
        self.opt = options if options is not None else default_options()
        self.devices = [int(d) for d in devices]
        self.reduce = int(reduce)
        self.moments = bool(moments)
        self.width, self.height = scene.resolution
        self._g = C.c_void_p()
        devs = (C.c_int * len(self.devices))(*self.devices)
        _check(self.lib.kdpt_group_create(C.byref(scene.view), C.byref(self.opt), len(self.devices), devs,
                                          self.reduce, GROUP_MOMENTS if self.moments else 0, C.byref(self._g)),
               "kdpt_group_create")

    def render_frames(self, first_frame: int, frames: int, spp: int, pipeline: int = 8, batch: int = 8, out=None):
        """kdpt_group_render_frames (async): out is None, a device pointer (int) or a float32 numpy array of
        frames * 3*W*H values, complete at synchronize()."""
        ptr = None if out is None else (int(out) if isinstance(out, int) else out.ctypes.data)
        _check(self.lib.kdpt_group_render_frames(self._g, int(first_frame), int(frames), int(spp), int(pipeline),
                                                 int(batch), ptr), "kdpt_group_render_frames")

    def render(self, first_frame: int, frames: int, spp: int, pipeline: int = 8, batch: int = 8) -> np.ndarray:
        """render_frames + synchronize: the reduced frames, (frames, H, W, 3) float32."""
        out = np.zeros((frames, self.height, self.width, 3), dtype=np.float32)
        self.render_frames(first_frame, frames, spp, pipeline, batch, out)
        self.synchronize()
        return out

    def synchronize(self):
        _check(self.lib.kdpt_group_synchronize(self._g), "kdpt_group_synchronize")

    def context(self, rank: int = 0) -> PathTracer:
        """kdpt_group_context: rank's context as a PathTracer that does not own it, for reads and queries (image,
        moments, noise_map, noise_estimate, sample_counts, save_*, stats, cast_rays, trace_rays, camera_rays, and
        denoise, denoise_temporal and temporal_reset on rank 0 of a group with moments)."""
        h = C.c_void_p()
        _check(self.lib.kdpt_group_context(self._g, int(rank), C.byref(h)), "kdpt_group_context")
        return PathTracer.borrowed(self, self.scene, self.opt, h)

    def active_pixels(self, floor: float = 1e-2, threshold: float = 0.0) -> np.ndarray:
        """kdpt_group_active_pixels: the list the next trace_adaptive would trace (int32, ascending)."""
        n = C.c_longlong()
        out = np.empty(self.height * self.width, dtype=np.int32)
        _check(self.lib.kdpt_group_active_pixels(self._g, float(floor), float(threshold),
                                                 C.c_void_p(out.ctypes.data), C.byref(n)),
               "kdpt_group_active_pixels")
        return out[:int(n.value)].copy()

    def trace_adaptive(self, first_iter: int, count: int, pipeline: int = 8, batch: int = 16, floor: float = 1e-2,
                       threshold: float = 0.0) -> Adaptive:
        """kdpt_group_trace_adaptive: iterations first_iter .. first_iter + count - 1 over the active pixels, dealt
        to the ranks in turn and added on rank 0.  Synchronous; returns the call's kdpt_adaptive record."""
        r = Adaptive()
        _check(self.lib.kdpt_group_trace_adaptive(self._g, int(first_iter), int(count), int(pipeline), int(batch),
                                                  float(floor), float(threshold), C.byref(r)),
               "kdpt_group_trace_adaptive")
        return r

    def set_camera(self, camera):
        """kdpt_group_set_camera: every rank's camera (a Camera, or a SceneData whose camera is taken)."""
        cam = camera.view.camera if isinstance(camera, SceneData) else camera
        _check(self.lib.kdpt_group_set_camera(self._g, C.byref(cam)), "kdpt_group_set_camera")

    def set_options(self, options: Options):
        _check(self.lib.kdpt_group_set_options(self._g, C.byref(options)), "kdpt_group_set_options")
        self.opt = options

    def reset(self):
        _check(self.lib.kdpt_group_reset(self._g), "kdpt_group_reset")

    def close(self):
        if self._g:
            self.lib.kdpt_group_destroy(self._g)
            self._g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PATH_DTYPE = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("isinside", "u1"), ("pad", "u1", 3),
                       ("sdepth", "<f4"), ("color", "<f4", 3), ("pixelIndex", "<i4"), ("remainingBounces", "<i4"),
                       ("materialIdHit", "<i4")])
assert PATH_DTYPE.itemsize == 56


def imgsum(image: np.ndarray) -> float:
    """Sum as the survey's anchor table defines it: per-pixel float32 (r+g+b), accumulated in double."""
    im = np.asarray(image, dtype=np.float32).reshape(-1, 3)
    per_px = (im[:, 0] + im[:, 1]) + im[:, 2]  # float32 adds, left to right
    return float(np.sum(per_px.astype(np.float64)))


COMM_ID_BYTES = 128


def comm_library() -> str:
    """kdpt_comm_library: the RCCL library file the library's reduces go through."""
    lib = load_library()
    buf = C.create_string_buffer(4096)
    _check(lib.kdpt_comm_library(buf, 4096), "kdpt_comm_library")
    return buf.value.decode(errors="replace")


def comm_unique_id() -> bytes:
    """kdpt_comm_unique_id: the RCCL unique id rank 0 hands to every rank."""
    lib = load_library()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib.kdpt_comm_unique_id(buf), "kdpt_comm_unique_id")
    return buf.raw


def render_sharded(scene: "SceneData", devices, first_frame: int, frames: int, spp: int,
                   options: Optional[Options] = None, pipeline: int = 8, batch: int = 8,
                   reduce: int = REDUCE_RCCL) -> np.ndarray:
    """kdpt_render_sharded: one process, one context per device; returns the reduced frames
    (frames, H, W, 3)."""
    lib = load_library()
    opt = options if options is not None else default_options()
    devs = (C.c_int * len(devices))(*devices)
    w, h = scene.resolution
    out = np.zeros((frames, h, w, 3), dtype=np.float32)
    _check(lib.kdpt_render_sharded(C.byref(scene.view), C.byref(opt), len(devices), devs, int(first_frame),
                                   int(frames), int(spp), int(pipeline), int(batch), int(reduce),
                                   out.ctypes.data), "kdpt_render_sharded")
    return out


def build_kd_device(verts9: np.ndarray, norms9: np.ndarray, mtl: np.ndarray, maxdepth: int = 13, device: int = 0):
    """kdpt_build_kd_device over a triangle soup: (NodeBare bytes, TriBare bytes, build ms)."""
    lib = load_library()
    v = np.ascontiguousarray(verts9, np.float32).reshape(-1, 9)
    n = np.ascontiguousarray(norms9, np.float32).reshape(-1, 9)
    m = np.ascontiguousarray(mtl, np.int32).reshape(-1)
    nodes, tris = C.c_void_p(), C.c_void_p()
    nn, nt, ms = C.c_int(), C.c_int(), C.c_double()
    _check(lib.kdpt_build_kd_device(_fptr(v), _fptr(n), _iptr(m), len(v), int(maxdepth), int(device), C.byref(nodes),
                                    C.byref(nn), C.byref(tris), C.byref(nt), C.byref(ms)), "kdpt_build_kd_device")
    try:
        nb = C.string_at(nodes.value, 64 * nn.value) if nn.value else b""
        tb = C.string_at(tris.value, 76 * nt.value) if nt.value else b""
    finally:
        lib.kdpt_free(nodes)
        lib.kdpt_free(tris)
    return nb, tb, float(ms.value)
