"""project3-cuda-path-tracer_amd -- MI355X-native hot path of CIS565 Project3-CUDA-Path-Tracer.

Python host-side mirror of the reference's renderer interface (src/pathtrace.h:6-8):

    pathtraceInit(scene)                 reference src/pathtrace.cu:75-85
    pathtrace(pbo, frame, iteration)     reference src/pathtrace.cu:123-174
    pathtraceFree()                      reference src/pathtrace.cu:87-92

over the C ABI declared in include/pt_amd.h (csrc/libpt_amd.so, hand-written HIP for gfx950) and
the C++ scene loader in host/ (libpt_host.so).  There is NO CPU fallback: importing works
anywhere (so the library's symbols can be checked), but every compute entry point fails loudly
when the extension or a GPU is missing.  This package never touches oracle/.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# PT_AMD_LIB: another build of the same library (A/B measurements of kernel variants); never a different backend
LIB_PATH = os.environ.get("PT_AMD_LIB") or os.path.join(HERE, "csrc", "libpt_amd.so")
HOST_LIB_PATH = os.path.join(HERE, "host", "libpt_host.so")

# byte-identical to reference src/sceneStructs.h:18-47 (include/pt_amd.h PtGeom/PtMaterial/PtCamera)
GEOM_DTYPE = np.dtype([
    ("type", "<i4"), ("materialid", "<i4"),
    ("translation", "<f4", 3), ("rotation", "<f4", 3), ("scale", "<f4", 3),
    ("transform", "<f4", 16), ("inverseTransform", "<f4", 16), ("invTranspose", "<f4", 16),
])
MATERIAL_DTYPE = np.dtype([
    ("color", "<f4", 3), ("specularExponent", "<f4"), ("specularColor", "<f4", 3),
    ("hasReflective", "<f4"), ("hasRefractive", "<f4"), ("indexOfRefraction", "<f4"),
    ("emittance", "<f4"),
])
CAMERA_DTYPE = np.dtype([
    ("resolution", "<i4", 2), ("position", "<f4", 3), ("view", "<f4", 3), ("up", "<f4", 3),
    ("fov", "<f4", 2),
])
assert GEOM_DTYPE.itemsize == 236 and MATERIAL_DTYPE.itemsize == 44 and CAMERA_DTYPE.itemsize == 52

PT_MAX_DEPTH = 62
PT_MAX_BATCH = 256
PT_FLAG_KERNEL_TIMING = 1
PT_FLAG_ACCUM_SHARD_ROWS = 2
PT_FLAG_DIRECT_LIGHTING = 4
PT_FLAG_TRACE_AHEAD = 8
PT_FLAG_MIXTURE_WEIGHTED = 16
PT_FLAG_MOMENTS = 32
PT_FLAG_TEMPORAL = 64
# the constants of temporal reprojection (include/pt_amd.h): the cap on a pixel's effective history, the least dot of the two normals, the
# largest distance from the new hit's tangent plane as a fraction of the hit's distance, the least sum of bilinear weights
PT_TEMPORAL_MAX_HISTORY, PT_TEMPORAL_NORMAL_DOT, PT_TEMPORAL_PLANE_FRACTION, PT_TEMPORAL_MIN_WEIGHT = 32.0, 0.9, 0.01, 0.5
PT_FLAG_DISPLAY_FILTER = 128
# the display filter's one setting (include/pt_amd.h): denoise_var's defaults
PT_DISPLAY_LEVELS, PT_DISPLAY_GUIDE_ITER, PT_DISPLAY_SIGMA_LUM, PT_DISPLAY_SIGMA_NORMAL, PT_DISPLAY_SIGMA_POSITION = 5, 1, 4.0, 0.35, 2.0
PT_FLAG_SPATIAL_VARIANCE = 256
# the spatial variance estimate (include/pt_amd.h): the count below which a pixel takes it, and the radius of its window
PT_SPATIAL_MIN_COUNT, PT_SPATIAL_RADIUS = 2.0, 1
PT_FLAG_DEMODULATE = 512
# albedo demodulation (include/pt_amd.h): the floor of a pixel's mean first-hit albedo
PT_DEMOD_MIN_ALBEDO = 0.015625
# history carries albedo (include/pt_amd.h, "demodulated history"): the flag, and the smallest sample count from which the renderer's own mean
# albedo -- not the blend with the reprojected one -- is multiplied back behind the filter
PT_FLAG_DEMOD_HISTORY = 1024
PT_DEMOD_HISTORY_MIN_OWN = 2
# a flag about cost alone (include/pt_amd.h): a full pt_init that repeats the live renderer's own call with another pose moves the camera in place
PT_FLAG_KEEP_RENDERER = 2048
# history follows moved objects (include/pt_amd.h, "object history"): the flag, and the cap of the history's count in a view that shows a
# primitive in another pose than the history's
PT_FLAG_OBJECT_HISTORY = 4096
PT_OBJECT_HISTORY_MAX = 4.0
# motion blur (include/pt_amd.h, "motion blur"): the flag, the poses across the shutter, the iterations that share one
PT_FLAG_MOTION = 8192            # motion blur: pt_init takes PT_MOTION_STEPS poses of the scene, iteration i renders PT_MOTION_STEP(i)'s
PT_MOTION_STEPS = 16
PT_MOTION_RUN = 8


def motion_step(iteration):
    """PT_MOTION_STEP (include/pt_amd.h): the step iteration `iteration` >= 1 renders -- runs of PT_MOTION_RUN iterations, bit-reversed."""
    r = ((iteration - 1) // PT_MOTION_RUN) % PT_MOTION_STEPS
    return ((r & 1) << 3) | ((r & 2) << 1) | ((r & 4) >> 1) | ((r & 8) >> 3)

# second link target of the same source: + the test-only entry points of include/pt_amd_test.h (tests/ and profiles/ only)
TEST_LIB_PATH = os.path.join(HERE, "csrc", "libpt_amd_test.so")

# every symbol include/pt_amd.h declares: the product's whole exported surface
ABI_SYMBOLS = [
    "pt_init", "pt_iterate", "pt_iterate_batch", "pt_sync", "pt_readback", "pt_readback_rgba8", "pt_counters",
    "pt_counters_reset", "pt_free", "pt_last_error", "pt_device_count",
    "pt_scan_exclusive_i32", "pt_compact_nonzero_i32", "pt_pin_host", "pt_unpin_host", "pt_set_meshes", "pt_set_meshes_sized", "pt_abi_version",
    "pt_ctx_create", "pt_ctx_make_current", "pt_ctx_current", "pt_ctx_destroy",
    "pt_group_create", "pt_group_destroy", "pt_group_size", "pt_group_collective", "pt_group_set_meshes", "pt_group_init", "pt_group_iterate_batch",
    "pt_group_iterate", "pt_group_reduce", "pt_group_sync", "pt_group_readback", "pt_group_counters",
    "pt_set_textures", "pt_group_set_textures", "pt_set_bump_maps", "pt_group_set_bump_maps",
    "pt_denoise", "pt_denoise_rgba8", "pt_gbuffer",
    "pt_readback_moments", "pt_variance", "pt_denoise_var", "pt_denoise_var_rgba8",
    "pt_noise_stats", "pt_iterate_until",
]
PT_AMD_ABI_VERSION = 7
PT_SAME_SCENE = 0           # pt_init(cam, NULL, 0, NULL, 0, PT_SAME_SCENE, NULL): the camera move (pathtraceSetCamera)
# every symbol include/pt_amd_test.h declares: libpt_amd_test.so only -- the product library must NOT export them
TEST_ABI_SYMBOLS = [
    "pt_debug_trace_paths",
    "pt_test_utilhash", "pt_test_rng", "pt_test_intersect", "pt_test_hemisphere", "pt_test_sincos", "pt_test_reflect_refract",
    "pt_test_slab_quotients", "pt_test_slab_quotients_sweep", "pt_test_box_fast_sweep", "pt_test_sphere_cull_sweep", "pt_test_unscaled_sqrt_sweep",
    "pt_test_force_fault", "pt_test_pow", "pt_test_wall_box_sweep", "pt_test_mesh_intersect", "pt_test_mesh_intersect2", "pt_test_mesh_bvh",
    "pt_test_mesh_cull_sweep", "pt_test_camera_cull_sweep", "pt_test_camera_cull_tables", "pt_test_camera_list",
    "pt_test_camera_resolved", "pt_test_face_hit_sweep", "pt_test_wall_faces", "pt_test_wall_face_sweep", "pt_test_wall_resolve_tally", "pt_test_candidate_tally",
    "pt_test_wall_plane_sweep", "pt_test_wall_planes", "pt_test_sphere_halfline_sweep", "pt_test_sphere_cluster_sweep", "pt_test_sphere_clusters", "pt_test_camera_cull_margin",
    "pt_test_group_fail_next_reduce", "pt_test_sphere_group_sweep", "pt_test_texture_sample", "pt_test_texture_uv",
    "pt_test_bump_normal", "pt_test_denoise", "pt_test_denoise_var", "pt_test_noise_stats", "pt_test_exp_neg_poly", "pt_test_bounce_form", "pt_test_live_device_buffers",
    "pt_test_renderer_state", "pt_test_scene_plan", "pt_test_temporal", "pt_test_temporal_camera", "pt_test_history",
    "pt_test_display", "pt_test_spatial_variance", "pt_test_albedo", "pt_test_demodulate", "pt_test_temporal_albedo", "pt_test_history_albedo",
    "pt_test_group_create_virtual", "pt_test_emulated_reduce", "pt_test_slab_decisions", "pt_test_sphere_groups", "pt_test_group_tally",
    "pt_test_camera_resolved_device", "pt_test_last_camera_move", "pt_test_keep_mismatch",
    "pt_test_motion_table", "pt_test_history_motion", "pt_test_temporal_motion", "pt_test_live_handles", "pt_test_pose_tables",
]


class PtOptions(C.Structure):
    _fields_ = [("shard_rank", C.c_int32), ("shard_count", C.c_int32), ("device", C.c_int32),
                ("flags", C.c_int32), ("pipeline_depth", C.c_int32), ("max_batch", C.c_int32),
                ("stream", C.c_void_p), ("accum_dev", C.c_void_p), ("lens_radius", C.c_float), ("focal_distance", C.c_float)]


class PtTestPlanSummary(C.Structure):      # include/pt_amd_test.h
    _fields_ = [("state_bits", C.c_uint32)] + [(n, C.c_int32) for n in ("nBinned", "nWalls", "nSphCull", "nSphGroups", "nLocalPad", "firstSkipped", "poolChunks")] + \
               [("ldsBytes", C.c_uint64), ("ldsBytesNext", C.c_uint64), ("histBits", C.c_int32), ("grpLds", C.c_int32)]


class PtMesh(C.Structure):
    _fields_ = [("geom", C.c_int32), ("ntris", C.c_int32), ("tris", C.c_void_p), ("normals", C.c_void_p), ("materials", C.c_void_p)]


class PtTexture(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.c_void_p)]


class PtTexBinding(C.Structure):
    _fields_ = [("geom", C.c_int32), ("texture", C.c_int32), ("ntris", C.c_int32), ("uvs", C.c_void_p)]


class PtBumpBinding(C.Structure):
    _fields_ = [("geom", C.c_int32), ("texture", C.c_int32), ("scale", C.c_float), ("ntris", C.c_int32), ("uvs", C.c_void_p)]


class PtDenoiseParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("guide_iter", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float)]


class PtDenoiseVarParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("guide_iter", C.c_int32), ("sigma_lum", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float)]


PT_NOISE_TILE = 16


class PtNoiseStats(C.Structure):
    _fields_ = [("samples", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("converged", C.c_int32), ("tiles", C.c_int64),
                ("unconverged", C.c_int64), ("max_rel_var", C.c_float), ("thr2", C.c_float)]


class PtNoiseTarget(C.Structure):
    _fields_ = [("threshold", C.c_float), ("lum_floor", C.c_float), ("max_unconverged_fraction", C.c_float), ("min_samples", C.c_int32),
                ("max_samples", C.c_int32), ("check_every", C.c_int32), ("lookahead", C.c_int32)]


class PtCounters(C.Structure):
    _fields_ = [("live", C.c_int64 * (PT_MAX_DEPTH + 2)), ("light_hits", C.c_int64), ("misses", C.c_int64),
                ("iterations", C.c_int64), ("bounce_launches", C.c_int64), ("bounce_kernel_ms", C.c_double),
                ("raygen_kernel_ms", C.c_double), ("raygen_launches", C.c_int64), ("ended_early", C.c_int64 * (PT_MAX_DEPTH + 2))]


class PtError(RuntimeError):
    pass


_lib = None
_test = None
_last_init = None           # the arguments of the last pathtraceInit (debug_trace_paths re-creates the scene in the test library)
_host = None
_atexit_registered = False


def _bind(L, with_tests):
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.pt_init.argtypes = [vp, vp, i32, vp, i32, i32, C.POINTER(PtOptions)]
    L.pt_iterate.argtypes = [i32, i32, vp]
    L.pt_iterate_batch.argtypes = [i32, i32, i32, vp]
    L.pt_sync.argtypes = []
    L.pt_readback.argtypes = [vp]
    L.pt_readback_rgba8.argtypes = [i32, vp]
    L.pt_counters.argtypes = [C.POINTER(PtCounters)]
    L.pt_counters_reset.argtypes = []
    L.pt_free.argtypes = []
    L.pt_free.restype = None
    L.pt_last_error.restype = C.c_char_p
    L.pt_device_count.argtypes = []
    L.pt_scan_exclusive_i32.argtypes = [vp, vp, i64, vp]
    L.pt_compact_nonzero_i32.argtypes = [vp, vp, i64, vp, vp]
    L.pt_pin_host.argtypes = [vp, C.c_size_t]
    L.pt_unpin_host.argtypes = []
    L.pt_set_meshes.argtypes = [C.POINTER(PtMesh), i32]
    L.pt_set_meshes_sized.argtypes = [C.POINTER(PtMesh), i32, C.c_size_t]
    L.pt_abi_version.argtypes = []
    L.pt_ctx_create.argtypes = []
    L.pt_ctx_create.restype = vp
    L.pt_ctx_make_current.argtypes = [vp]
    L.pt_ctx_current.argtypes = []
    L.pt_ctx_current.restype = vp
    L.pt_ctx_destroy.argtypes = [vp]
    L.pt_group_create.argtypes = [C.POINTER(vp), i32, C.POINTER(C.c_int32)]
    L.pt_group_destroy.argtypes = [vp]
    L.pt_group_destroy.restype = None
    L.pt_group_size.argtypes = [vp]
    L.pt_group_collective.argtypes = [vp]
    L.pt_group_collective.restype = C.c_char_p
    L.pt_group_set_meshes.argtypes = [vp, C.POINTER(PtMesh), i32]
    L.pt_set_textures.argtypes = [C.POINTER(PtTexture), i32, C.c_size_t, C.POINTER(PtTexBinding), i32, C.c_size_t]
    L.pt_group_set_textures.argtypes = [vp, C.POINTER(PtTexture), i32, C.c_size_t, C.POINTER(PtTexBinding), i32, C.c_size_t]
    L.pt_set_bump_maps.argtypes = [C.POINTER(PtBumpBinding), i32, C.c_size_t]
    L.pt_group_set_bump_maps.argtypes = [vp, C.POINTER(PtBumpBinding), i32, C.c_size_t]
    L.pt_group_init.argtypes = [vp, vp, vp, i32, vp, i32, i32, C.POINTER(PtOptions)]
    L.pt_group_iterate_batch.argtypes = [vp, i32, i32, i32]
    L.pt_group_iterate.argtypes = [vp, i32, i32]
    L.pt_group_reduce.argtypes = [vp]
    L.pt_group_sync.argtypes = [vp]
    L.pt_group_readback.argtypes = [vp, vp]
    L.pt_group_counters.argtypes = [vp, C.POINTER(PtCounters)]
    L.pt_denoise.argtypes = [i32, C.POINTER(PtDenoiseParams), C.c_size_t, vp]
    L.pt_denoise_rgba8.argtypes = [i32, C.POINTER(PtDenoiseParams), C.c_size_t, vp]
    L.pt_gbuffer.argtypes = [i32, vp, vp, vp]
    L.pt_readback_moments.argtypes = [vp]
    L.pt_variance.argtypes = [i32, vp]
    L.pt_denoise_var.argtypes = [i32, C.POINTER(PtDenoiseVarParams), C.c_size_t, vp, vp]
    L.pt_denoise_var_rgba8.argtypes = [i32, C.POINTER(PtDenoiseVarParams), C.c_size_t, vp]
    L.pt_noise_stats.argtypes = [i32, C.c_float, C.c_float, C.POINTER(PtNoiseStats), C.c_size_t, vp]
    L.pt_iterate_until.argtypes = [i32, i32, C.POINTER(PtNoiseTarget), C.c_size_t, C.POINTER(PtNoiseStats), C.POINTER(C.c_int32)]
    if with_tests:
        L.pt_debug_trace_paths.argtypes = [i32, i32, vp, vp, vp, vp, C.POINTER(C.c_int32)]
        u64p = C.POINTER(C.c_uint64)
        L.pt_test_utilhash.argtypes = [vp, vp, i32]
        L.pt_test_rng.argtypes = [vp, i32, i32, vp]
        L.pt_test_intersect.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp]
        L.pt_test_hemisphere.argtypes = [vp, vp, i32, vp]
        L.pt_test_sincos.argtypes = [vp, i32, vp, vp]
        L.pt_test_reflect_refract.argtypes = [vp, vp, vp, i32, vp, vp]
        L.pt_test_slab_quotients.argtypes = [vp, vp, i32, vp, vp, vp, vp]
        L.pt_test_slab_quotients_sweep.argtypes = [C.c_uint64, i64, u64p]
        L.pt_test_box_fast_sweep.argtypes = [vp, i32, C.c_uint64, i64, u64p, u64p]
        L.pt_test_sphere_cull_sweep.argtypes = [vp, i32, C.c_uint64, i64, u64p, u64p]
        L.pt_test_sphere_halfline_sweep.argtypes = [vp, i32, C.c_uint64, i64, u64p, u64p, u64p]
        L.pt_test_sphere_cluster_sweep.argtypes = [vp, i32, C.c_uint64, i64, u64p, u64p, vp]
        L.pt_test_sphere_clusters.argtypes = [vp, i32, vp, vp, i32, vp]
        L.pt_test_unscaled_sqrt_sweep.argtypes = [u64p]
        L.pt_test_force_fault.argtypes = [i32]
        L.pt_test_pow.argtypes = [vp, vp, i32, vp]
        L.pt_test_wall_box_sweep.argtypes = [vp, i32, C.c_uint64, i64, u64p, u64p]
        L.pt_test_mesh_intersect.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]
        L.pt_test_mesh_intersect2.argtypes = [vp, vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.pt_test_mesh_bvh.argtypes = [vp, i32, i32, vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.pt_test_mesh_cull_sweep.argtypes = [vp, vp, i32, C.c_uint64, i64] + [u64p] * 3
        L.pt_test_camera_cull_sweep.argtypes = [vp, vp, i32, i32] + [u64p] * 3
        L.pt_test_camera_cull_tables.argtypes = [vp, vp, i32, vp, vp, vp]
        L.pt_test_camera_list.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
        L.pt_test_camera_resolved.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
        L.pt_test_camera_resolved_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
        L.pt_test_last_camera_move.argtypes = [vp, vp, vp]
        L.pt_test_keep_mismatch.argtypes = [vp, i32]
        L.pt_test_face_hit_sweep.argtypes = [vp, vp, i32, i32, C.c_uint64, u64p]
        L.pt_test_wall_faces.argtypes = [vp, vp, i32, vp, i32, i32, C.POINTER(PtOptions), vp, vp]
        L.pt_test_wall_face_sweep.argtypes = [vp, i32, C.c_uint64, i64, u64p]
        L.pt_test_wall_resolve_tally.argtypes = [u64p]
        L.pt_test_candidate_tally.argtypes = [u64p]
        L.pt_test_group_tally.argtypes = [u64p]
        L.pt_test_sphere_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(PtOptions), C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.pt_test_slab_decisions.argtypes = [vp, vp, i32, vp, vp]
        L.pt_test_camera_cull_margin.argtypes = [vp, vp, i32, i32, C.POINTER(C.c_double), u64p]
        L.pt_test_wall_plane_sweep.argtypes = [vp, i32, C.c_uint64, i64, C.POINTER(C.c_int32)] + [u64p] * 3
        L.pt_test_wall_planes.argtypes = [vp, i32, vp, vp] + [C.POINTER(C.c_int32)] * 3
        L.pt_test_group_fail_next_reduce.argtypes = [vp, i32]
        L.pt_test_group_create_virtual.argtypes = [C.POINTER(vp), i32, C.POINTER(C.c_int32), i32]
        L.pt_test_emulated_reduce.argtypes = [C.POINTER(vp), i32, i64, i32, vp, C.POINTER(vp)]
        L.pt_test_sphere_group_sweep.argtypes = [vp, i32, C.c_uint64, i64, u64p, u64p, C.POINTER(C.c_int32)]
        L.pt_test_texture_sample.argtypes = [vp, i32, i32, vp, i32, vp]
        L.pt_test_texture_uv.argtypes = [i32, vp, vp, i32, vp]
        L.pt_test_bump_normal.argtypes = [vp, i32, i32, vp, vp, i32, vp]
        L.pt_test_denoise.argtypes = [i32, C.POINTER(PtDenoiseParams), C.c_size_t, i32, vp, vp]
        L.pt_test_denoise_var.argtypes = [i32, C.POINTER(PtDenoiseVarParams), C.c_size_t, i32, vp, vp, vp]
        L.pt_test_noise_stats.argtypes = [vp, vp, i32, i32, i32, C.c_float, C.c_float, C.POINTER(PtNoiseStats), C.c_size_t, vp, i32, i32, vp]
        L.pt_test_exp_neg_poly.argtypes = [vp, i32, vp]
        L.pt_test_temporal_camera.argtypes = [vp, vp]
        L.pt_test_temporal.argtypes = [i32, i32, i32, i32] + [vp] * 11 + [i32, vp]
        L.pt_test_history.argtypes = [vp] * 6
        L.pt_test_display.argtypes = [i32, i32, i32, vp, vp]
        L.pt_test_spatial_variance.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, C.c_float, C.c_float, vp, i32, vp]
        L.pt_test_albedo.argtypes = [vp]
        L.pt_test_temporal_albedo.argtypes = [i32] * 5 + [vp] * 11 + [C.c_float] + [vp] * 3 + [i32, vp]
        L.pt_test_history_albedo.argtypes = [vp, vp]
        L.pt_test_motion_table.argtypes = [vp, vp, i32, vp, vp]
        L.pt_test_history_motion.argtypes = [vp, vp, vp]
        L.pt_test_temporal_motion.argtypes = [i32] * 6 + [vp] * 12 + [i32, C.c_float, C.c_float] + [vp] * 3 + [i32, vp]
        L.pt_test_demodulate.argtypes = [i32] * 7 + [vp] * 6 + [C.c_float] * 4 + [vp] * 4 + [i32, vp]
        L.pt_test_bounce_form.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
        L.pt_test_live_device_buffers.argtypes = []
        L.pt_test_live_device_buffers.restype = i64
        L.pt_test_pose_tables.argtypes = [C.POINTER(C.c_int64)]
        L.pt_test_live_handles.argtypes = []
        L.pt_test_live_handles.restype = i64
        L.pt_test_renderer_state.argtypes = [C.POINTER(C.c_uint32)]
        L.pt_test_scene_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(PtOptions), C.POINTER(PtTestPlanSummary)]
    return L


def _load(path, with_tests):
    if not os.path.exists(path):
        raise PtError("HIP extension missing: %s (run __graft_entry__.build()); there is no CPU fallback" % path)
    # torch (device memory / streams / RCCL plumbing) bundles its own libamdhip64.so; it has to be
    # loaded FIRST so that this library binds to the same HIP runtime instance (same soname) and
    # torch stream handles / device pointers are valid here.  Two runtimes in one process break both.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    return _bind(C.CDLL(path), with_tests)


def lib():
    """The HIP extension (the product library).  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, False)
    return _lib


def test_lib():
    """libpt_amd_test.so: the same source linked with the test-only entry points of include/pt_amd_test.h.  It holds its own
    renderer instance; the product path never loads it."""
    global _test
    if _test is None:
        _test = _load(TEST_LIB_PATH, True)
    return _test


class renderer_from_test_library:
    """Context manager for the one test that has to reach INTO a renderer (pt_test_force_fault): inside it the renderer API of
    this module drives the instance that lives in libpt_amd_test.so."""

    def __enter__(self):
        global _lib
        self._saved = lib()
        _lib = test_lib()
        return self

    def __exit__(self, *exc):
        global _lib
        _lib.pt_free()
        _lib = self._saved
        return False


def _check(rc, L=None):
    if rc != 0:
        raise PtError("pt_amd error %d: %s" % (rc, (L or lib()).pt_last_error().decode()))


def _tcheck(rc):
    _check(rc, test_lib())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def device_count():
    return lib().pt_device_count()


# --------------------------------------------------------------------------- scene (host/ loader)
def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise PtError("host library missing: %s (run __graft_entry__.build())" % HOST_LIB_PATH)
        H = C.CDLL(HOST_LIB_PATH)
        vp = C.c_void_p
        H.pth_scene_load.restype = vp
        H.pth_scene_load.argtypes = [C.c_char_p]
        H.pth_scene_free.argtypes = [vp]
        H.pth_scene_free.restype = None
        for n in ("pth_scene_num_geoms", "pth_scene_num_materials", "pth_scene_iterations", "pth_scene_depth"):
            getattr(H, n).argtypes = [vp]
            getattr(H, n).restype = C.c_int
        for n in ("pth_scene_geoms", "pth_scene_materials", "pth_scene_camera"):
            getattr(H, n).argtypes = [vp]
            getattr(H, n).restype = vp
        H.pth_scene_image_name.argtypes = [vp]
        H.pth_scene_image_name.restype = C.c_char_p
        H.pth_scene_motion_steps.argtypes = [vp]
        H.pth_scene_step_geoms.argtypes = [vp, C.c_int]
        H.pth_scene_step_geoms.restype = vp
        H.pth_scene_set_resolution.argtypes = [vp, C.c_int, C.c_int]
        H.pth_scene_set_resolution.restype = None
        H.pth_scene_num_meshes.argtypes = [vp]
        for n in ("pth_scene_mesh_geom", "pth_scene_mesh_ntris"):
            getattr(H, n).argtypes = [vp, C.c_int]
        H.pth_scene_mesh_tris.argtypes = [vp, C.c_int]
        H.pth_scene_mesh_tris.restype = vp
        for n in ("pth_scene_mesh_normals", "pth_scene_mesh_materials", "pth_scene_mesh_uvs", "pth_scene_texture_rgb"):
            getattr(H, n).argtypes = [vp, C.c_int]
            getattr(H, n).restype = vp
        H.pth_scene_num_textures.argtypes = [vp]
        for n in ("pth_scene_texture_width", "pth_scene_texture_height", "pth_scene_geom_texture", "pth_scene_geom_bump"):
            getattr(H, n).argtypes = [vp, C.c_int]
        H.pth_scene_geom_bump_scale.argtypes = [vp, C.c_int]
        H.pth_scene_geom_bump_scale.restype = C.c_float
        H.pth_scene_texture_path.argtypes = [vp, C.c_int]
        H.pth_scene_texture_path.restype = C.c_char_p
        for n in ("pth_save_png", "pth_save_hdr"):
            getattr(H, n).argtypes = [C.c_char_p, vp, C.c_int, C.c_int, C.c_float]
            getattr(H, n).restype = C.c_int
        _host = H
    return _host


class Scene:
    """Mirror of the reference's `Scene` (src/scene.h:13-26): geoms, materials, state."""

    def __init__(self, filename):
        H = host_lib()
        h = H.pth_scene_load(os.fsencode(filename))
        if not h:
            raise IOError("Error reading from file - aborting!")  # reference src/scene.cpp:12-15
        self._h = h
        self._refresh()

    def _refresh(self):
        H, h = host_lib(), self._h
        ng, nm = H.pth_scene_num_geoms(h), H.pth_scene_num_materials(h)
        self.geoms = np.frombuffer(C.string_at(H.pth_scene_geoms(h), 236 * ng), GEOM_DTYPE).copy() if ng \
            else np.zeros(0, GEOM_DTYPE)
        self.materials = np.frombuffer(C.string_at(H.pth_scene_materials(h), 44 * nm), MATERIAL_DTYPE).copy() if nm \
            else np.zeros(0, MATERIAL_DTYPE)
        self.camera = np.frombuffer(C.string_at(H.pth_scene_camera(h), 52), CAMERA_DTYPE).copy()
        self.iterations = H.pth_scene_iterations(h)
        self.traceDepth = H.pth_scene_depth(h)
        self.imageName = H.pth_scene_image_name(h).decode()
        # `mesh <file.obj>` objects (README.md:236): geom index -> (ntris, 9) float32 triangles in object space
        self.meshes = {}
        self.mesh_normals = {}      # geom index -> (ntris, 9) vertex normals (`vn`); absent: flat shading
        self.mesh_materials = {}    # geom index -> (ntris,) int32 scene material per face (`usemtl <k>`, -1 = the object's); absent: none
        self.mesh_uvs = {}          # geom index -> (ntris, 6) float32 corner texture coordinates (`vt`); absent: none
        for i in range(H.pth_scene_num_meshes(h)):
            nt = H.pth_scene_mesh_ntris(h, i)
            g = H.pth_scene_mesh_geom(h, i)
            self.meshes[g] = np.frombuffer(C.string_at(H.pth_scene_mesh_tris(h, i), 36 * nt), np.float32).reshape(nt, 9).copy()
            nptr, mptr = H.pth_scene_mesh_normals(h, i), H.pth_scene_mesh_materials(h, i)
            if nptr:
                self.mesh_normals[g] = np.frombuffer(C.string_at(nptr, 36 * nt), np.float32).reshape(nt, 9).copy()
            if mptr:
                self.mesh_materials[g] = np.frombuffer(C.string_at(mptr, 4 * nt), np.int32).copy()
            uptr = H.pth_scene_mesh_uvs(h, i)
            if uptr:
                self.mesh_uvs[g] = np.frombuffer(C.string_at(uptr, 24 * nt), np.float32).reshape(nt, 6).copy()
        # `TEXTURE <file>` lines: the scene's textures ((H, W, 3) float32, row 0 = top) and per geom the index of its texture or -1
        self.textures = []
        self.texture_paths = []
        for i in range(H.pth_scene_num_textures(h)):
            tw, th = H.pth_scene_texture_width(h, i), H.pth_scene_texture_height(h, i)
            self.textures.append(np.frombuffer(C.string_at(H.pth_scene_texture_rgb(h, i), 12 * tw * th), np.float32).reshape(th, tw, 3).copy())
            self.texture_paths.append(H.pth_scene_texture_path(h, i).decode())
        self.geom_textures = np.array([H.pth_scene_geom_texture(h, g) for g in range(ng)], np.int32)
        # `BUMP <file> <scale>` lines: per geom the index of its height map among `textures` or -1, and its scale (0 where unbumped)
        self.geom_bumps = np.array([H.pth_scene_geom_bump(h, g) for g in range(ng)], np.int32)
        self.bump_scales = np.array([H.pth_scene_geom_bump_scale(h, g) for g in range(ng)], np.float32)
        # TRANS_END / ROTAT_END / SCALE_END lines: the scene in PT_MOTION_STEPS poses across the shutter, (steps, ngeoms) records -- step s
        # is byte for byte the geoms of a static scene file with the values interpolated at (s + 0.5) / steps -- or None: nothing moves
        steps = H.pth_scene_motion_steps(h)
        self.step_geoms = np.stack([np.frombuffer(C.string_at(H.pth_scene_step_geoms(h, k), GEOM_DTYPE.itemsize * ng), GEOM_DTYPE) for k in range(steps)]) \
            if steps and ng else None
        w, hh = (int(v) for v in self.camera["resolution"][0])
        self.image = np.zeros((hh, w, 3), np.float32)   # RenderState::image (src/sceneStructs.h:53)

    def set_resolution(self, w, h):
        """RES override; fov.x is recomputed as src/scene.cpp:133-136 does."""
        host_lib().pth_scene_set_resolution(self._h, w, h)
        self._refresh()

    def __del__(self):
        if getattr(self, "_h", None) and _host is not None:   # _host is gone during interpreter shutdown
            _host.pth_scene_free(self._h)
            self._h = None


# --------------------------------------------------------------------------- renderer API
_scene = None


def pathtraceInit(scene, shard_rank=0, shard_count=1, stream=0, accum_dev=0, device=-1, flags=0, traceDepth=None,
                  pipeline_depth=0, max_batch=0, lens_radius=0.0, focal_distance=0.0, direct_lighting=False, trace_ahead=False,
                  mixture_weighted=False, moments=False, temporal=False, display_filter=False, spatial_variance=False, demodulate=False,
                  demod_history=False, keep=False, object_history=False, motion=None):
    """reference src/pathtrace.cu:75-85.  `scene` is borrowed until pathtraceFree().
    motion: PT_FLAG_MOTION (include/pt_amd.h, "motion blur") -- None: motion-blurred where the scene file defines motion (scene.step_geoms),
    static otherwise; False: the static scene (scene.geoms); True: scene.step_geoms, which must exist; or an array of PT_MOTION_STEPS x
    len(scene.geoms) geom records of the caller's own, step-major.  Iteration i then renders step motion_step(i) alone, and the frame is, bit
    for bit, the sum of those iterations of static renderers.  Not with temporal, object_history, display_filter, demodulate,
    spatial_variance or keep; denoise* and gbuffer refuse a motion-blurred renderer.
    object_history: PT_FLAG_OBJECT_HISTORY (with moments=True and temporal=True) -- calling pathtraceInit AGAIN over the live renderer with the
    same objects in other poses (geoms' types and materials, the materials and everything registered equal byte for byte; translation,
    rotation, scale and the matrices free) carries the history over and reprojects it through each primitive's own motion; any other change
    of the scene drops the history.  History passes only between renderers that agree on the flag.
    keep: PT_FLAG_KEEP_RENDERER -- a flag about cost alone: calling pathtraceInit AGAIN over the live renderer with the same scene, arguments
    and registered meshes, textures and height maps (compared byte for byte) and another pose moves the camera in place, as pathtraceSetCamera
    does; anything else is the full call.  The result is the full call's bit for bit either way.
    demod_history: PT_FLAG_DEMOD_HISTORY (with moments=True, temporal=True and demodulate=True, which go together under it alone) -- the
    history a re-initialisation carries over also holds the old view's mean first-hit albedo, and denoise_var / denoise_var_rgba8 / the display
    divide the blend of history and new samples by the blended albedo.  History passes only between renderers that agree on the flag.
    demodulate: PT_FLAG_DEMODULATE (with moments=True; not with temporal or trace_ahead) -- every pathtrace / pathtrace_batch also adds the
    first-hit albedo of its iterations' camera rays to a per-pixel sum, and denoise_var / denoise_var_rgba8 -- with display_filter=True the
    display's bytes too -- divide the pixel's mean albedo out in front of the filter and multiply it back behind it: textures survive.
    Everything else is the unflagged renderer's.
    spatial_variance: PT_FLAG_SPATIAL_VARIANCE (with moments=True) -- denoise_var / denoise_var_rgba8 accept samples=1: a pixel with fewer than
    PT_SPATIAL_MIN_COUNT effective samples is filtered under a variance estimated from its neighbours, and with display_filter=True the first
    displayed frame is filtered too.  From two samples on everything is the unflagged renderer's.
    display_filter: PT_FLAG_DISPLAY_FILTER (moments=True must be given with it: it implies nothing) -- the `pbo` of pathtrace / pathtrace_batch
    and readback_rgba8 receive the bytes of denoise_var_rgba8 with its defaults (PT_DISPLAY_*) instead of the raw accumulator's, made on the
    device behind the commit, on the renderer's stream, without a synchronisation.  Everything else is the unflagged renderer's.
    temporal: PT_FLAG_TEMPORAL (with moments=True, no lens, no trace_ahead) -- calling pathtraceInit AGAIN, WITHOUT pathtraceFree() in between,
    with a moved camera is what carries the last view's samples over as history: denoise_var / denoise_var_rgba8 of the new renderer then filter
    the blend of the reprojected history with the new samples.  pathtraceFree() drops the history (call it when the scene itself changes).
    moments: PT_FLAG_MOMENTS -- the renderer also sums every sample's squared luminance (readback_moments, variance, denoise_var).
    lens_radius / focal_distance / direct_lighting: the README extras (depth of field, direct lighting), off by default.
    trace_ahead: PT_FLAG_TRACE_AHEAD -- pathtrace(pbo, frame, iter) called once per iteration draws on batches of max_batch
    iterations traced ahead (same image, bit for bit)."""
    global _scene
    if direct_lighting:
        flags |= PT_FLAG_DIRECT_LIGHTING
    if trace_ahead:
        flags |= PT_FLAG_TRACE_AHEAD
    if mixture_weighted:        # the REFL > 0 mixture with its 1 / p weights (src/interactions.h:54-58 to the letter; default: without)
        flags |= PT_FLAG_MIXTURE_WEIGHTED
    if moments:
        flags |= PT_FLAG_MOMENTS
    if temporal:
        flags |= PT_FLAG_TEMPORAL
    if display_filter:
        flags |= PT_FLAG_DISPLAY_FILTER
    if spatial_variance:
        flags |= PT_FLAG_SPATIAL_VARIANCE
    if demodulate:
        flags |= PT_FLAG_DEMODULATE
    if demod_history:
        flags |= PT_FLAG_DEMOD_HISTORY
    if keep:
        flags |= PT_FLAG_KEEP_RENDERER
    if object_history:
        flags |= PT_FLAG_OBJECT_HISTORY
    geoms = np.ascontiguousarray(scene.geoms)
    ngeoms = len(geoms)
    if motion is None:
        motion = getattr(scene, "step_geoms", None) is not None
    if motion is True:
        if getattr(scene, "step_geoms", None) is None:
            raise PtError("pathtraceInit(motion=True): the scene defines no motion (TRANS_END / ROTAT_END / SCALE_END)")
        motion = scene.step_geoms
    if motion is not False:
        geoms = np.ascontiguousarray(np.asarray(motion, GEOM_DTYPE).reshape(-1))
        if len(geoms) != PT_MOTION_STEPS * ngeoms:
            raise PtError("pathtraceInit(motion=...): %d geom records, PT_MOTION_STEPS x %d expected" % (len(geoms), ngeoms))
        flags |= PT_FLAG_MOTION
    opt = PtOptions(shard_rank, shard_count, device, flags, pipeline_depth, max_batch, stream or None, accum_dev or None,
                    lens_radius, focal_distance)
    mats = np.ascontiguousarray(scene.materials)
    cam = np.ascontiguousarray(scene.camera)
    depth = scene.traceDepth if traceDepth is None else traceDepth
    set_meshes(getattr(scene, "meshes", None) or {}, getattr(scene, "mesh_normals", None), getattr(scene, "mesh_materials", None))
    set_textures(*_scene_textures(scene))
    set_bump_maps(*_scene_bumps(scene))
    global _atexit_registered
    if not _atexit_registered:
        # an interpreter that exits with a live renderer (an exception between pathtrace and pathtraceFree): drain the streams
        # and release everything while the interpreter, torch and the HIP runtime are still whole (the library registers its own
        # exit handler as well, for hosts that are not Python)
        import atexit
        atexit.register(pathtraceFree)
        _atexit_registered = True
    _check(lib().pt_init(_p(cam), _p(geoms), ngeoms, _p(mats), len(mats), depth, C.byref(opt)))
    _scene = scene
    global _last_init
    _last_init = (cam, geoms, mats, depth, (shard_rank, shard_count, device, flags, lens_radius, focal_distance),
                  (getattr(scene, "meshes", None) or {}, getattr(scene, "mesh_normals", None), getattr(scene, "mesh_materials", None)),
                  _scene_textures(scene), _scene_bumps(scene))


def pathtraceSetCamera(camera_or_scene):
    """pt_init's same-scene form (include/pt_amd.h: PT_SAME_SCENE): move the camera of the live renderer in place -- what pathtraceInit called again with the same scene, arguments and
    the new camera would leave behind, bit for bit (under temporal=True the old view becomes the history), without giving up the renderer's
    buffers.  Takes a camera record (scene.camera, or a copy with another pose) or a Scene, whose camera it reads; the resolution must be
    the live renderer's."""
    global _last_init
    cam = np.ascontiguousarray(getattr(camera_or_scene, "camera", camera_or_scene)).copy()
    _check(lib().pt_init(_p(cam), None, 0, None, 0, PT_SAME_SCENE, None))
    if _last_init is not None:
        _last_init = (cam,) + tuple(_last_init[1:])


def pose_tables():
    """pt_test_pose_tables (test library; see renderer_from_test_library): the scene tables the live renderer's pt_init allocated --
    {"poses", "own_buffers", "own_bytes" (one pose's own tables), "shared_buffers", "shared_bytes" (held once: texels, mesh records),
    "all_own_bytes" (every pose's own tables together)}."""
    out = (C.c_int64 * 6)()
    _tcheck(test_lib().pt_test_pose_tables(out))
    return dict(zip(("poses", "own_buffers", "own_bytes", "shared_buffers", "shared_bytes", "all_own_bytes"), (int(v) for v in out)))


def camera_move_info():
    """pt_test_last_camera_move (test library; see renderer_from_test_library): which way this thread's last pathtraceSetCamera -- or
    pathtraceInit(..., keep=True) -- went: {"fast": True / False / None (no move yet, the last one was refused, or the keep=True call ran
    the full call), "tables_uploaded": n, "bytes_uploaded": n}."""
    out = [C.c_int(0) for _ in range(3)]
    _tcheck(test_lib().pt_test_last_camera_move(*[C.byref(o) for o in out]))
    fast = out[0].value
    return {"fast": None if fast < 0 else bool(fast), "tables_uploaded": out[1].value, "bytes_uploaded": out[2].value}


def keep_mismatch():
    """pt_test_keep_mismatch (test library): why this thread's last pathtraceInit(..., keep=True) ran the full call -- the name of the first
    comparison that failed ("geoms", "materials", "traceDepth", "flags", "texels", ..., "no live renderer"), "" where it moved in place."""
    buf = C.create_string_buffer(64)
    _tcheck(test_lib().pt_test_keep_mismatch(buf, len(buf)))
    return buf.value.decode()


def scene_plan(scene, traceDepth=None, **options):
    """pt_test_scene_plan: what pathtraceInit(scene, ...) would plan, on the host alone (no GPU) -- a PtTestPlanSummary, or the PtError of
    the refusal.  options: PtOptions fields by name (flags, shard_rank, shard_count, max_batch, lens_radius, ...)."""
    T = test_lib()
    # (the scene's meshes, textures and bindings are registered with the test library, as pathtraceInit registers them with the renderer's)
    set_meshes(getattr(scene, "meshes", None) or {}, getattr(scene, "mesh_normals", None), getattr(scene, "mesh_materials", None), L=T)
    set_textures(*_scene_textures(scene), L=T)
    set_bump_maps(*_scene_bumps(scene), L=T)
    opt = PtOptions(shard_count=1, device=-1)
    for name, value in options.items():
        setattr(opt, name, value)
    geoms, mats, cam = np.ascontiguousarray(scene.geoms), np.ascontiguousarray(scene.materials), np.ascontiguousarray(scene.camera)
    out = PtTestPlanSummary()
    _check(T.pt_test_scene_plan(_p(cam), _p(geoms), len(geoms), _p(mats), len(mats), scene.traceDepth if traceDepth is None else traceDepth,
                                C.byref(opt), C.byref(out)), T)
    return out


def _mesh_array(meshes, normals=None, materials=None):
    """(PtMesh array, count, the arrays it points into) for pt_set_meshes / pt_group_set_meshes"""
    keep = [(int(g), np.ascontiguousarray(t, np.float32).reshape(-1, 9)) for g, t in sorted(meshes.items())]
    extra = []                                       # (keeps the attribute arrays alive across the call)
    arr = (PtMesh * max(len(keep), 1))()
    for i, (g, t) in enumerate(keep):
        nn = (normals or {}).get(g)
        mm = (materials or {}).get(g)
        nn = None if nn is None else np.ascontiguousarray(nn, np.float32).reshape(len(t), 9)
        mm = None if mm is None else np.ascontiguousarray(mm, np.int32).reshape(len(t))
        extra += [nn, mm]
        arr[i] = PtMesh(g, len(t), t.ctypes.data, None if nn is None else nn.ctypes.data, None if mm is None else mm.ctypes.data)
    return arr, len(keep), (keep, extra)


def set_meshes(meshes, normals=None, materials=None, L=None):
    """pt_set_meshes: {geom index: (ntris, 9) triangles in object space} for the next pathtraceInit (an empty dict clears); optionally
    {geom index: (ntris, 9) vertex normals} and {geom index: (ntris,) int32 face materials}.  Through the sized entry point: a
    library built against another PtMesh refuses instead of striding through garbage."""
    arr, n, alive = _mesh_array(meshes, normals, materials)
    L = L or lib()
    _check(L.pt_set_meshes_sized(arr, n, C.sizeof(PtMesh)), L)


def _scene_textures(scene):
    """(textures, geom_textures, mesh_uvs) of a Scene -- or of any object with those attributes; none: untextured"""
    return (list(getattr(scene, "textures", None) or []), getattr(scene, "geom_textures", None), getattr(scene, "mesh_uvs", None) or {})


def _texture_arrays(textures, geom_textures=None, mesh_uvs=None):
    """(PtTexture array, count, PtTexBinding array, count, the arrays they point into) for pt_set_textures / pt_group_set_textures.
    A geom is bound when geom_textures[g] >= 0; a bound mesh geom carries its UVs from mesh_uvs[g] ((ntris, 6) float32)."""
    tex = [np.ascontiguousarray(t, np.float32).reshape(np.shape(t)[0], np.shape(t)[1], 3) for t in textures]
    tarr = (PtTexture * max(len(tex), 1))()
    for i, t in enumerate(tex):
        tarr[i] = PtTexture(t.shape[1], t.shape[0], t.ctypes.data)
    gt = [] if geom_textures is None else [int(x) for x in np.asarray(geom_textures).reshape(-1)]
    binds, uvs = [], []
    for g, k in enumerate(gt):
        if k < 0:
            continue
        u = (mesh_uvs or {}).get(g)
        u = None if u is None else np.ascontiguousarray(u, np.float32).reshape(-1, 6)
        uvs.append(u)
        binds.append(PtTexBinding(g, k, 0 if u is None else len(u), None if u is None else u.ctypes.data))
    barr = (PtTexBinding * max(len(binds), 1))(*binds)
    return tarr, len(tex), barr, len(binds), (tex, uvs)


def _scene_bumps(scene):
    """(geom_bumps, bump_scales, mesh_uvs) of a Scene -- or of any object with those attributes; none: unbumped (a scene object without
    them CLEARS the bump maps of an earlier one)"""
    return (getattr(scene, "geom_bumps", None), getattr(scene, "bump_scales", None), getattr(scene, "mesh_uvs", None) or {})


def _bump_arrays(geom_bumps=None, bump_scales=None, mesh_uvs=None):
    """(PtBumpBinding array, count, the arrays they point into) for pt_set_bump_maps / pt_group_set_bump_maps.  A geom is bumped when
    geom_bumps[g] >= 0 (an index into the registered textures), with scale bump_scales[g]; a bumped mesh geom carries its UVs from mesh_uvs[g]."""
    gb = [] if geom_bumps is None else [int(x) for x in np.asarray(geom_bumps).reshape(-1)]
    sc = np.zeros(len(gb), np.float32) if bump_scales is None else np.asarray(bump_scales, np.float32).reshape(-1)
    binds, uvs = [], []
    for g, k in enumerate(gb):
        if k < 0:
            continue
        u = (mesh_uvs or {}).get(g)
        u = None if u is None else np.ascontiguousarray(u, np.float32).reshape(-1, 6)
        uvs.append(u)
        binds.append(PtBumpBinding(g, k, float(sc[g]), 0 if u is None else len(u), None if u is None else u.ctypes.data))
    barr = (PtBumpBinding * max(len(binds), 1))(*binds)
    return barr, len(binds), uvs


def set_bump_maps(geom_bumps=None, bump_scales=None, mesh_uvs=None, L=None):
    """pt_set_bump_maps for the next pathtraceInit: `geom_bumps` per geom the index of its height map among the textures of set_textures
    or -1, `bump_scales` per geom its scale, `mesh_uvs` {geom index: (ntris, 6) corner UVs} for the bumped meshes.  None / empty clears."""
    barr, nb, alive = _bump_arrays(geom_bumps, bump_scales, mesh_uvs)
    L = L or lib()
    _check(L.pt_set_bump_maps(barr, nb, C.sizeof(PtBumpBinding)), L)


def set_textures(textures, geom_textures=None, mesh_uvs=None, L=None):
    """pt_set_textures for the next pathtraceInit: `textures` a list of (H, W, 3) float32 images (row 0 = top), `geom_textures` per geom the
    index of its texture or -1, `mesh_uvs` {geom index: (ntris, 6) corner UVs} for the textured meshes.  Empty lists clear."""
    tarr, nt, barr, nb, alive = _texture_arrays(textures, geom_textures, mesh_uvs)
    L = L or lib()
    _check(L.pt_set_textures(tarr, nt, C.sizeof(PtTexture), barr, nb, C.sizeof(PtTexBinding)), L)


def pathtrace(pbo, frame, iteration, readback=True):
    """reference src/pathtrace.cu:123-174: one iteration; `pbo` is a DEVICE pointer (int) or None.
    With readback=True the running sum lands in scene.image like the reference's D2H copy (:170-171).
    `pbo` receives sendImageToPBO's bytes of the accumulator over `iteration` samples -- under display_filter=True the bytes
    denoise_var_rgba8(iteration) would return at that point of the stream (the blend with the context's history included; iteration 1: the
    unfiltered bytes), written on the device behind the commit.  They are valid once the renderer's stream has passed them."""
    _check(lib().pt_iterate(frame, iteration, pbo or None))
    if readback and _scene is not None:
        _check(lib().pt_readback(_p(_scene.image)))


def pathtrace_batch(pbo, frame, first_iteration, count, readback=False, until=None):
    """`count` iterations in one wavefront (pt_iterate_batch); same result as `count` pathtrace() calls.
    `pbo` (a device pointer or None) receives the bytes of the accumulator over first_iteration + count - 1 samples; under display_filter=True
    those of denoise_var_rgba8(first_iteration + count - 1), as pathtrace's.
    until: a noise threshold, or a dict of iterate_until()'s keywords with one -- then AT MOST `count` iterations (any number, in batches of
    max_batch) are rendered, until the frame's tiles pass (pt_iterate_until; no `pbo`), and (statistics, samples_done) is returned."""
    if until is not None:
        if pbo:
            raise PtError("pathtrace_batch: until= takes no pbo")
        kw = dict(until) if isinstance(until, dict) else {"threshold": until}
        res = iterate_until(first_iteration, max_samples=first_iteration + count - 1, frame=frame, **kw)
    else:
        _check(lib().pt_iterate_batch(frame, first_iteration, count, pbo or None))
        res = None
    if readback and _scene is not None:
        _check(lib().pt_readback(_p(_scene.image)))
    return res


def pathtraceFree():
    """reference src/pathtrace.cu:87-92; legal before the first pathtraceInit (src/main.cpp:91-94)."""
    global _scene
    if _lib is not None:          # (nothing to free in a library that was never loaded)
        _lib.pt_free()
    _scene = None


def sync():
    _check(lib().pt_sync())


def force_fault(which):
    """Diagnostics (test library only, see renderer_from_test_library): set the renderer's device fault word by hand (2), or clear it (0)."""
    _tcheck(test_lib().pt_test_force_fault(which))


def readback(npixels):
    """Un-normalised running sum of the WHOLE frame (W*H*3 floats; with PT_FLAG_ACCUM_SHARD_ROWS the other shards'
    rows are zero).  `npixels` must be the frame's pixel count: pt_readback always writes that many."""
    if _scene is not None:
        res = _scene.camera["resolution"][0]
        if int(res[0]) * int(res[1]) != npixels:
            raise PtError("readback: the frame has %d pixels, not %d" % (int(res[0]) * int(res[1]), npixels))
    out = np.empty(npixels * 3, np.float32)
    _check(lib().pt_readback(_p(out)))
    return out


def readback_rgba8(iteration, npixels):
    """sendImageToPBO's bytes of the accumulator over `iteration` samples (pt_readback_rgba8): (npixels, 4).  Under display_filter=True the
    bytes denoise_var_rgba8(iteration) returns -- what a `pbo` given to pathtrace would hold; iteration 1: the unfiltered bytes."""
    out = np.empty((npixels, 4), np.uint8)
    _check(lib().pt_readback_rgba8(iteration, _p(out)))
    return out


# default sigmas of the denoiser: colour in units of the image's mean (few samples of a scene with a bright light are far apart), the normal's
# in units of a unit vector's difference, the position's in world units (Cornell's box is 10 units wide): the values tests/test_denoise_cpu.py
# tries on a 4-iteration Cornell frame
DENOISE_SIGMA_COLOR, DENOISE_SIGMA_NORMAL, DENOISE_SIGMA_POSITION = 2.0, 0.35, 2.0


def _frame_pixels():
    if _scene is None:
        raise PtError("no scene: pathtraceInit first")
    res = _scene.camera["resolution"][0]
    return int(res[0]) * int(res[1])


def _denoise_params(levels, sigma_color, sigma_normal, sigma_position, guide_iter):
    return PtDenoiseParams(levels, guide_iter, sigma_color, sigma_normal, sigma_position)


def denoise(samples, levels=5, sigma_color=DENOISE_SIGMA_COLOR, sigma_normal=DENOISE_SIGMA_NORMAL,
            sigma_position=DENOISE_SIGMA_POSITION, guide_iter=1):
    """The accumulator's mean over `samples`, filtered by `levels` passes of the edge-avoiding a-trous filter (pt_denoise): W*H*3 floats.
    The accumulator is left as it is."""
    out = np.empty(_frame_pixels() * 3, np.float32)
    prm = _denoise_params(levels, sigma_color, sigma_normal, sigma_position, guide_iter)
    _check(lib().pt_denoise(samples, C.byref(prm), C.sizeof(prm), _p(out)))
    return out


def denoise_rgba8(samples, levels=5, sigma_color=DENOISE_SIGMA_COLOR, sigma_normal=DENOISE_SIGMA_NORMAL,
                  sigma_position=DENOISE_SIGMA_POSITION, guide_iter=1):
    """... converted like the preview's pixels (pt_denoise_rgba8): (W*H, 4) bytes."""
    out = np.empty((_frame_pixels(), 4), np.uint8)
    prm = _denoise_params(levels, sigma_color, sigma_normal, sigma_position, guide_iter)
    _check(lib().pt_denoise_rgba8(samples, C.byref(prm), C.sizeof(prm), _p(out)))
    return out


def gbuffer(guide_iter=1):
    """The denoiser's guide buffers (pt_gbuffer): the nearest hits of iteration `guide_iter`'s camera rays as (pos_t (W*H, 4), normal (W*H, 3),
    geom (W*H,) int32); a miss is (0, 0, 0, -1), zeros and -1."""
    n = _frame_pixels()
    pos_t, nrm, geom = np.empty((n, 4), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.int32)
    _check(lib().pt_gbuffer(guide_iter, _p(pos_t), _p(nrm), _p(geom)))
    return pos_t, nrm, geom


def test_denoise(samples, form, levels=5, sigma_color=DENOISE_SIGMA_COLOR, sigma_normal=DENOISE_SIGMA_NORMAL,
                 sigma_position=DENOISE_SIGMA_POSITION, guide_iter=1, timing=False):
    """denoise() with the form of k_atrous_*<AtrousPlain> named (test library, inside renderer_from_test_library): 0 the product's choice, 1 the plain gather,
    2 / 3 LDS tiles of 64 x 4 / 64 x 8.  timing=True: also the kernel times in ms, k_gbuffer first (0 when cached), then each level."""
    out = np.empty(_frame_pixels() * 3, np.float32)
    ms = np.zeros(1 + levels, np.float32)
    prm = _denoise_params(levels, sigma_color, sigma_normal, sigma_position, guide_iter)
    _tcheck(test_lib().pt_test_denoise(samples, C.byref(prm), C.sizeof(prm), form, _p(out), _p(ms) if timing else None))
    return (out, ms) if timing else out


# the variance-guided filter's colour sigma, in standard errors of the pixel's mean luminance: one value for every sample count
DENOISE_SIGMA_LUM = 4.0


def readback_moments():
    """Per pixel the sum of its samples' squared luminance (pt_readback_moments; a renderer initialised with moments=True): W*H floats."""
    out = np.empty(_frame_pixels(), np.float32)
    _check(lib().pt_readback_moments(_p(out)))
    return out


def variance(samples):
    """The variance of every pixel's mean luminance over `samples` (pt_variance): W*H floats."""
    out = np.empty(_frame_pixels(), np.float32)
    _check(lib().pt_variance(samples, _p(out)))
    return out


def denoise_var(samples, levels=5, sigma_lum=DENOISE_SIGMA_LUM, sigma_normal=DENOISE_SIGMA_NORMAL, sigma_position=DENOISE_SIGMA_POSITION,
                guide_iter=1, with_variance=False):
    """The accumulator's mean over `samples` through the variance-guided a-trous filter (pt_denoise_var): W*H*3 floats; with_variance=True:
    (that, the filtered variance of the mean luminance, W*H floats).  Both accumulators are left as they are."""
    n = _frame_pixels()
    out = np.empty(n * 3, np.float32)
    var = np.empty(n, np.float32) if with_variance else None
    prm = PtDenoiseVarParams(levels, guide_iter, sigma_lum, sigma_normal, sigma_position)
    _check(lib().pt_denoise_var(samples, C.byref(prm), C.sizeof(prm), _p(out), _p(var) if with_variance else None))
    return (out, var) if with_variance else out


def denoise_var_rgba8(samples, levels=5, sigma_lum=DENOISE_SIGMA_LUM, sigma_normal=DENOISE_SIGMA_NORMAL,
                      sigma_position=DENOISE_SIGMA_POSITION, guide_iter=1):
    """... converted like the preview's pixels (pt_denoise_var_rgba8): (W*H, 4) bytes."""
    out = np.empty((_frame_pixels(), 4), np.uint8)
    prm = PtDenoiseVarParams(levels, guide_iter, sigma_lum, sigma_normal, sigma_position)
    _check(lib().pt_denoise_var_rgba8(samples, C.byref(prm), C.sizeof(prm), _p(out)))
    return out


def test_denoise_var(samples, form, levels=5, sigma_lum=DENOISE_SIGMA_LUM, sigma_normal=DENOISE_SIGMA_NORMAL,
                     sigma_position=DENOISE_SIGMA_POSITION, guide_iter=1, timing=False):
    """denoise_var(with_variance=True) with the form of k_atrous_*<AtrousGuided> named, as test_denoise: (rgb, variance[, ms])."""
    n = _frame_pixels()
    out, var = np.empty(n * 3, np.float32), np.empty(n, np.float32)
    ms = np.zeros(1 + levels, np.float32)
    prm = PtDenoiseVarParams(levels, guide_iter, sigma_lum, sigma_normal, sigma_position)
    _tcheck(test_lib().pt_test_denoise_var(samples, C.byref(prm), C.sizeof(prm), form, _p(out), _p(var), _p(ms) if timing else None))
    return (out, var, ms) if timing else (out, var)


def test_display(samples, form, pbo, fused=True, timing=False):
    """pt_test_display (test library, inside renderer_from_test_library): the display path of a moments=True renderer into the DEVICE pointer
    `pbo`, every level -- the last included -- in the form named (0 the product's choice, 1 the gather, 2 / 3 the tiles); fused=False: the
    last level writes packed RGB and k_to_rgba8 converts it.  On the renderer's stream, not synchronised -- unless timing=True: then the
    1 + PT_DISPLAY_LEVELS kernel times in ms are returned (k_gbuffer first; the last level's with k_to_rgba8 where fused=False)."""
    ms = np.zeros(1 + PT_DISPLAY_LEVELS, np.float32)
    _tcheck(test_lib().pt_test_display(samples, form, 1 if fused else 0, pbo, _p(ms) if timing else None))
    return ms if timing else None


# the luminance a tile's mean is floored with before the noise statistics divide by it: 5 % of a white diffuse surface's
NOISE_LUM_FLOOR = 0.05


def _noise_result(st, tile_map):
    out = {f: getattr(st, f) for f, _ in PtNoiseStats._fields_}
    out["converged"] = bool(out["converged"])
    if tile_map is not None:
        out["tile_rel_var"] = tile_map.reshape(st.tiles_y, st.tiles_x)
    return out


def _frame_tiles():
    res = _scene.camera["resolution"][0] if _scene is not None else (0, 0)
    return ((int(res[0]) + PT_NOISE_TILE - 1) // PT_NOISE_TILE) * ((int(res[1]) + PT_NOISE_TILE - 1) // PT_NOISE_TILE)


def noise_stats(samples, threshold, lum_floor=NOISE_LUM_FLOOR, tile_map=False):
    """How converged the accumulator is after `samples` iterations (pt_noise_stats; a renderer initialised with moments=True): a dict of
    PtNoiseStats' fields -- tiles of 16 x 16 pixels, `unconverged` of them with a relative standard error above `threshold`, max_rel_var the
    largest squared one -- and with tile_map=True "tile_rel_var", (tiles_y, tiles_x) floats."""
    _frame_pixels()
    st = PtNoiseStats()
    tm = np.empty(_frame_tiles(), np.float32) if tile_map else None
    _check(lib().pt_noise_stats(samples, threshold, lum_floor, C.byref(st), C.sizeof(st), _p(tm) if tile_map else None))
    return _noise_result(st, tm)


def iterate_until(first_iteration, threshold, max_samples, lum_floor=NOISE_LUM_FLOOR, max_unconverged_fraction=0.0, min_samples=2, check_every=8,
                  lookahead=1, frame=0):
    """Render iterations first_iteration, ... until the frame's tiles pass `threshold` or `max_samples` are in the accumulator
    (pt_iterate_until): (the final accumulator's statistics as noise_stats gives them, samples_done)."""
    tgt = PtNoiseTarget(threshold, lum_floor, max_unconverged_fraction, min_samples, max_samples, check_every, lookahead)
    st = PtNoiseStats()
    done = C.c_int32(0)
    _check(lib().pt_iterate_until(frame, first_iteration, C.byref(tgt), C.sizeof(tgt), C.byref(st), C.byref(done)))
    return _noise_result(st, None), int(done.value)


def test_noise_stats(rgb_sum, lum_sq_sum, w, h, samples, threshold, lum_floor=NOISE_LUM_FLOOR, tiles_per_wave=0, timing_reps=0):
    """noise_stats(tile_map=True) of host arrays S (h, w, 3) and Q (h, w) through k_noise_stats, no renderer; tiles_per_wave: the tiles a wave
    of the grid takes (0: the library's choice; the same bits whatever it is); timing_reps > 0: (that, ms) with ms (reps, 2): k_noise_stats'
    and k_variance's kernel times over the same arrays."""
    S = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    Q = np.ascontiguousarray(lum_sq_sum, np.float32).reshape(-1)
    if S.size != w * h * 3 or Q.size != w * h:
        raise PtError("test_noise_stats: S must hold w * h * 3 floats, Q w * h")
    st = PtNoiseStats()
    tm = np.empty(((w + PT_NOISE_TILE - 1) // PT_NOISE_TILE) * ((h + PT_NOISE_TILE - 1) // PT_NOISE_TILE), np.float32)
    ms = np.zeros((max(timing_reps, 1), 2), np.float32)
    _tcheck(test_lib().pt_test_noise_stats(_p(S), _p(Q), w, h, samples, threshold, lum_floor, C.byref(st), C.sizeof(st), _p(tm), tiles_per_wave, timing_reps,
                                           _p(ms) if timing_reps > 0 else None))
    res = _noise_result(st, tm)
    return (res, ms) if timing_reps > 0 else res


def test_temporal_camera(camera):
    """pt_test_temporal_camera (host only): the 16 floats k_temporal takes for a view -- eye, pixLenX, pixLenY, halfW, halfH, the rows r0, r1, r2 --
    of a CAMERA_DTYPE record."""
    cam = np.ascontiguousarray(camera)
    out = np.empty(16, np.float32)
    _tcheck(test_lib().pt_test_temporal_camera(_p(cam), _p(out)))
    return out


def test_temporal(capture, w, h, samples, rgb_sum, lum_sq_sum, pos_t, nrm_id, hc, hn, hpos_t, hnrm_id, cam16, timing_reps=0):
    """k_temporal over host arrays (test library, no renderer): the current view's S (h, w, 3), Q (h, w) and guide buffers pos_t, nrm_id
    ((h, w, 4) float32 each, nrm_id[..., 3] = the bits of the int32 primitive index), the history hc (h, w, 4), hn (h, w) and its guides, the old
    camera's 16 floats.  capture=False: the filter form, (h * w, 4) = (c, variance); capture=True: (Hc' (h * w, 4), Hn' (h * w,)); capture=2: the
    moments form, (M (h * w, 4), N (h * w,)) with the count uncapped.  timing_reps > 0: also the kernel times in ms."""
    f = lambda a, k: np.ascontiguousarray(a, np.float32).reshape(w * h * k)
    S, Q, pos, nrm, Hc, Hn, Hpos, Hnrm = f(rgb_sum, 3), f(lum_sq_sum, 1), f(pos_t, 4), f(nrm_id, 4), f(hc, 4), f(hn, 1), f(hpos_t, 4), f(hnrm_id, 4)
    cam = np.ascontiguousarray(cam16, np.float32).reshape(16)
    out, out_n = np.empty((w * h, 4), np.float32), np.empty(w * h, np.float32)
    ms = np.zeros(max(timing_reps, 1), np.float32)
    _tcheck(test_lib().pt_test_temporal(int(capture), w, h, samples, _p(S), _p(Q), _p(pos), _p(nrm), _p(Hc), _p(Hn), _p(Hpos), _p(Hnrm), _p(cam),
                                        _p(out), _p(out_n), timing_reps, _p(ms) if timing_reps > 0 else None))
    res = (out, out_n) if capture else out
    return (res, ms) if timing_reps > 0 else res


def test_spatial_variance(radius, form, w, h, m4, n, pos_t, nrm_id, sigma_normal=DENOISE_SIGMA_NORMAL, sigma_position=DENOISE_SIGMA_POSITION,
                          timing_reps=0):
    """k_spatial_variance_*<radius> over host arrays (test library, no renderer): M (h, w, 4) = (mean r, g, b, m2), N (h, w) the effective sample
    counts and the guide buffers pos_t, nrm_id ((h, w, 4) each, as test_temporal takes them).  radius 1, 2 or 3; form 0: the gather, 1: the LDS
    tiles.  Returns (h * w, 4) = (c, variance); timing_reps > 0: also the kernel times in ms."""
    f = lambda a, k: np.ascontiguousarray(a, np.float32).reshape(w * h * k)
    M, N, pos, nrm = f(m4, 4), f(n, 1), f(pos_t, 4), f(nrm_id, 4)
    out = np.empty((w * h, 4), np.float32)
    ms = np.zeros(max(timing_reps, 1), np.float32)
    _tcheck(test_lib().pt_test_spatial_variance(radius, form, w, h, _p(M), _p(N), _p(pos), _p(nrm), sigma_normal, sigma_position, _p(out), timing_reps,
                                                _p(ms) if timing_reps > 0 else None))
    return (out, ms) if timing_reps > 0 else out


def test_albedo():
    """pt_test_albedo (inside renderer_from_test_library, a demodulate=True renderer): the albedo sums, (npixels, 4) -- [:, :3] the sum of the
    committed iterations' first-hit albedo, [:, 3] their number."""
    out = np.empty((_frame_pixels(), 4), np.float32)
    _tcheck(test_lib().pt_test_albedo(_p(out)))
    return out


def test_demodulate(form, w, h, samples, levels, asum, pos_t, nrm_id, rgb_sum=None, lum_sq_sum=None, img=None, bytes_out=False, want_var=True,
                    sigma_lum=DENOISE_SIGMA_LUM, sigma_normal=DENOISE_SIGMA_NORMAL, sigma_position=DENOISE_SIGMA_POSITION,
                    min_albedo=PT_DEMOD_MIN_ALBEDO, timing_reps=0):
    """k_demodulate and the `levels` levels behind it over host arrays (test library, no renderer; pt_test_demodulate): asum (h, w, 4) the albedo
    sums, the guide buffers as test_temporal takes them, every level in `form` (1 the gather, 2 / 3 the tiles), the last one AtrousDemod's.
    img=None: from the accumulators rgb_sum (h, w, 3), lum_sq_sum (h, w); img (h, w, 4) = (r, g, b, variance): rewritten in place.
    Returns a dict: "demod" (h * w, 4) k_demodulate's image, and "rgb" (h * w, 3) with "var" (h * w,) or None -- or, bytes_out=True, "rgba"
    (h * w, 4) uint8; timing_reps > 0: also "ms" (reps, 2), k_demodulate's and the last level's kernel times."""
    f = lambda a, k: np.ascontiguousarray(a, np.float32).reshape(w * h * k)
    inplace = img is not None
    A, pos, nrm = f(asum, 4), f(pos_t, 4), f(nrm_id, 4)
    S = None if inplace else f(rgb_sum, 3)
    Q = None if inplace else f(lum_sq_sum, 1)
    I = f(img, 4) if inplace else None
    demod = np.empty((w * h, 4), np.float32)
    rgb = None if bytes_out else np.empty((w * h, 3), np.float32)
    var = np.empty(w * h, np.float32) if (want_var and not bytes_out) else None
    rgba = np.empty((w * h, 4), np.uint8) if bytes_out else None
    ms = np.zeros((max(timing_reps, 1), 2), np.float32)
    q = lambda a: None if a is None else _p(a)
    _tcheck(test_lib().pt_test_demodulate(form, 1 if inplace else 0, 1 if bytes_out else 0, w, h, samples, levels, q(S), q(Q), q(I), _p(A), _p(pos), _p(nrm),
                                          sigma_lum, sigma_normal, sigma_position, min_albedo, _p(demod), q(rgb), q(var), q(rgba), timing_reps,
                                          _p(ms) if timing_reps > 0 else None))
    res = {"demod": demod, "rgb": rgb, "var": var, "rgba": rgba}
    if timing_reps > 0:
        res["ms"] = ms
    return res


def test_history():
    """pt_test_history: the history the test library's current context holds (inside renderer_from_test_library) -- None, or a dict of hc
    (H, W, 4), hn (H, W), hpos_t, hnrm_id (H, W, 4) and cam (16,), and (pt_test_history_motion) motion: the motion table as the device holds it,
    (ngeoms, 24) float32 as test_motion_table returns it, or None where the history holds none; cap: the count's cap the blends take."""
    T = test_lib()
    wh = np.zeros(2, np.int32)
    _tcheck(T.pt_test_history(_p(wh), None, None, None, None, None))
    w, h = int(wh[0]), int(wh[1])
    if w == 0:
        return None
    hc, hn, hpos, hnrm = np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32), np.empty((h, w, 4), np.float32), np.empty((h, w, 4), np.float32)
    cam = np.empty(16, np.float32)
    _tcheck(T.pt_test_history(_p(wh), _p(hc), _p(hn), _p(hpos), _p(hnrm), _p(cam)))
    n, cap = np.zeros(1, np.int32), np.zeros(1, np.float32)
    _tcheck(T.pt_test_history_motion(_p(n), None, _p(cap)))
    motion = None
    if int(n[0]) > 0:
        motion = np.empty((int(n[0]), 24), np.float32)
        _tcheck(T.pt_test_history_motion(_p(n), _p(motion), None))
    return dict(hc=hc, hn=hn, hpos_t=hpos, hnrm_id=hnrm, cam=cam, motion=motion, cap=float(cap[0]))


def test_motion_table(geoms_then, geoms_now):
    """pt_test_motion_table (host only): the motion table pt_init makes under object_history=True between the geoms the history's view was
    rendered with and a call's (GEOM_DTYPE records of equal number).  Returns (rows (n, 24) float32, any): a row is m[3][4] row by row, then
    (G[0], state bits), (G[1], 0), (G[2], 0) -- rows[:, 15].view(int32) is the state 0 / 1 / 2; any: a row has another state than 0."""
    a, b = np.ascontiguousarray(geoms_then), np.ascontiguousarray(geoms_now)
    if len(a) != len(b) or len(a) < 1:
        raise ValueError("test_motion_table: two geom arrays of one length >= 1")
    rows, flag = np.zeros((len(a), 24), np.float32), np.zeros(1, np.int32)
    _tcheck(test_lib().pt_test_motion_table(_p(a), _p(b), len(a), _p(rows), _p(flag)))
    return rows, bool(flag[0])


def test_temporal_motion(form, albedo, motion, w, h, samples, rgb_sum, lum_sq_sum, pos_t, nrm_id, hc, hn, hpos_t, hnrm_id, cam16, rows=None,
                         hist_cap=PT_OBJECT_HISTORY_MAX, asum=None, ha=None, min_albedo=PT_DEMOD_MIN_ALBEDO, timing_reps=0):
    """Any (FORM, ALBEDO, MOTION) form of k_temporal over host arrays (test library, no renderer; pt_test_temporal_motion): test_temporal's
    arrays; form 0 / 1 / 2 / 3: the filter, capture, moments form and -- albedo=True alone -- the fused demodulating filter; albedo=True: asum and
    ha as test_temporal_albedo takes them; motion=True: rows (n, 24) as test_motion_table returns them, hist_cap step 6's cap.  Returns
    (out (h * w, 4), out_n (h * w,) or None, (Ab, tot) (h * w, 4) or None); timing_reps > 0: also the kernel times in ms."""
    f = lambda a, k: np.ascontiguousarray(a, np.float32).reshape(w * h * k)
    S, Q, pos, nrm = f(rgb_sum, 3), f(lum_sq_sum, 1), f(pos_t, 4), f(nrm_id, 4)
    Hc, Hn, Hpos, Hnrm = f(hc, 4), f(hn, 1), f(hpos_t, 4), f(hnrm_id, 4)
    A = f(asum, 4) if albedo else None
    Ha = f(ha, 4) if albedo else None
    R = np.ascontiguousarray(rows, np.float32).reshape(-1, 24) if motion else None
    cam = np.ascontiguousarray(cam16, np.float32).reshape(16)
    out, out_n = np.empty((w * h, 4), np.float32), np.empty(w * h, np.float32)
    out_a = np.empty((w * h, 4), np.float32) if albedo else None
    ms = np.zeros(max(timing_reps, 1), np.float32)
    q = lambda a: None if a is None else _p(a)
    _tcheck(test_lib().pt_test_temporal_motion(int(form), int(bool(albedo)), int(bool(motion)), w, h, samples, _p(S), _p(Q), _p(pos), _p(nrm), q(A),
                                               _p(Hc), _p(Hn), q(Ha), _p(Hpos), _p(Hnrm), _p(cam), q(R), 0 if R is None else len(R), float(hist_cap),
                                               float(min_albedo), _p(out), _p(out_n), q(out_a), timing_reps, _p(ms) if timing_reps > 0 else None))
    res = (out, out_n if form in (1, 2) else None, out_a)
    return (res, ms) if timing_reps > 0 else res


def test_temporal_albedo(form, w, h, samples, rgb_sum, lum_sq_sum, pos_t, nrm_id, asum, hc, hn, ha, hpos_t, hnrm_id, cam16, front=0,
                         min_albedo=PT_DEMOD_MIN_ALBEDO, timing_reps=0):
    """The ALBEDO forms of k_temporal over host arrays (test library, no renderer; pt_test_temporal_albedo): test_temporal's arguments, and asum
    (h, w, 4) the current view's albedo sums, ha (h, w, 4) the history's albedo.  form 0 / 1 / 2: the filter, capture, moments form.  front (form
    0): 0 the blend alone, 1 the fused front, 2 the two launches it fuses.  Returns (out (h * w, 4), out_n (h * w,) or None, (Ab, tot) (h * w, 4));
    timing_reps > 0: also the times of the front in ms."""
    f = lambda a, k: np.ascontiguousarray(a, np.float32).reshape(w * h * k)
    S, Q, pos, nrm, A = f(rgb_sum, 3), f(lum_sq_sum, 1), f(pos_t, 4), f(nrm_id, 4), f(asum, 4)
    Hc, Hn, Ha, Hpos, Hnrm = f(hc, 4), f(hn, 1), f(ha, 4), f(hpos_t, 4), f(hnrm_id, 4)
    cam = np.ascontiguousarray(cam16, np.float32).reshape(16)
    out, out_n, out_a = np.empty((w * h, 4), np.float32), np.empty(w * h, np.float32), np.empty((w * h, 4), np.float32)
    ms = np.zeros(max(timing_reps, 1), np.float32)
    _tcheck(test_lib().pt_test_temporal_albedo(int(form), int(front), w, h, samples, _p(S), _p(Q), _p(pos), _p(nrm), _p(A), _p(Hc), _p(Hn), _p(Ha),
                                               _p(Hpos), _p(Hnrm), _p(cam), min_albedo, _p(out), _p(out_n), _p(out_a), timing_reps,
                                               _p(ms) if timing_reps > 0 else None))
    res = (out, out_n if form else None, out_a)
    return (res, ms) if timing_reps > 0 else res


def test_history_albedo():
    """pt_test_history_albedo: the albedo image (H, W, 4) = (Ab, tot) of the history the test library's current context holds (inside
    renderer_from_test_library), or None: no history, or one made without demod_history=True."""
    T = test_lib()
    wh = np.zeros(2, np.int32)
    _tcheck(T.pt_test_history_albedo(_p(wh), None))
    w, h = int(wh[0]), int(wh[1])
    if w == 0:
        return None
    ha = np.empty((h, w, 4), np.float32)
    _tcheck(T.pt_test_history_albedo(_p(wh), _p(ha)))
    return ha


def test_exp_neg_poly(a):
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty_like(a)
    _tcheck(test_lib().pt_test_exp_neg_poly(_p(a), a.size, _p(out)))
    return out


def test_emulated_reduce(sends, in_place=False):
    """pt_test_emulated_reduce: the emulated reduce of virtual device groups on its own (test library).  sends: 1..8 float32 arrays of one length,
    rank by rank; root 0.  Returns (what the root received, every rank's device send buffer as the call left it)."""
    sends = [np.ascontiguousarray(s, np.float32).reshape(-1) for s in sends]
    n = sends[0].size
    if any(s.size != n for s in sends):
        raise PtError("test_emulated_reduce: send buffers of one length")
    recv = np.empty(n, np.float32)
    after = [np.empty(n, np.float32) for _ in sends]
    ptrs = lambda arrs: (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    _tcheck(test_lib().pt_test_emulated_reduce(ptrs(sends), len(sends), n, 1 if in_place else 0, _p(recv), ptrs(after)))
    return recv, after


def counters():
    c = PtCounters()
    _check(lib().pt_counters(C.byref(c)))
    return c


def counters_reset():
    _check(lib().pt_counters_reset())


def debug_trace_paths(iteration, bounces, npixels):
    """State of the paths alive after `bounces` bounces of `iteration` (sorted by pixel).  A diagnostic of the TEST library (the product
    exports none since round 5): the scene of the last pathtraceInit is initialised in libpt_amd_test.so's own renderer -- the same
    kernels, its own instance -- traced there and freed again; the product's renderer is not touched."""
    if _last_init is None:
        raise PtError("debug_trace_paths before pathtraceInit")
    T = test_lib()
    cam, geoms, mats, depth, (rank, count, device, flags, lens_radius, focal_distance), meshes, textures, bumps = _last_init
    if _lib is T:                                    # (renderer_from_test_library: the renderer IS the test library's)
        own = False
    else:
        own = True
        set_meshes(*meshes, L=T)
        set_textures(*textures, L=T)
        set_bump_maps(*bumps, L=T)
        opt = PtOptions(rank, count, device, flags & ~(PT_FLAG_TRACE_AHEAD | PT_FLAG_KERNEL_TIMING), 1, 1, None, None, lens_radius, focal_distance)
        ngeoms = len(geoms) // (PT_MOTION_STEPS if flags & PT_FLAG_MOTION else 1)      # (motion blur: every step's geoms)
        _tcheck(T.pt_init(_p(cam), _p(geoms), ngeoms, _p(mats), len(mats), depth, C.byref(opt)))
    try:
        o, d, c = (np.empty((npixels, 3), np.float32) for _ in range(3))
        pix = np.empty(npixels, np.int32)
        n = C.c_int32(0)
        _tcheck(T.pt_debug_trace_paths(iteration, bounces, _p(o), _p(d), _p(c), _p(pix), C.byref(n)))
    finally:
        if own:
            T.pt_free()
    k = n.value
    return o[:k], d[:k], c[:k], pix[:k]


class Context:
    """pt_ctx_*: a renderer instance of its own.  `with ctx:` makes it the calling thread's current context -- the renderer API of
    this module then drives it -- and puts the previous one back."""

    def __init__(self):
        self.handle = lib().pt_ctx_create()
        if not self.handle:
            raise PtError("pt_ctx_create failed: %s" % lib().pt_last_error().decode())

    def __enter__(self):
        self._prev = lib().pt_ctx_current()
        _check(lib().pt_ctx_make_current(self.handle))
        return self

    def __exit__(self, *exc):
        _check(lib().pt_ctx_make_current(self._prev))
        return False

    def destroy(self):
        if self.handle:
            _check(lib().pt_ctx_destroy(self.handle))
            self.handle = None


class Group:
    """pt_group_*: n contexts rendering the row shards y % n of one frame, member i on devices[i] (default: i % device count).
    virtual=[...] (test library only, inside renderer_from_test_library): member i on VIRTUAL device virtual[i] of the one HIP device, each a
    device of its own to the group (pt_test_group_create_virtual), the frame assembled by collective "reduce" (the emulated reduce) or "host"."""

    def __init__(self, n, devices=None, virtual=None, collective="reduce"):
        h = C.c_void_p()
        if virtual is not None:
            if _lib is None or _lib is not _test:
                raise PtError("Group(virtual=...) exists in the test library only: use it inside renderer_from_test_library()")
            if devices is not None or len(virtual) != n or collective not in ("reduce", "host"):
                raise PtError("Group(virtual=...): n virtual device indices, no devices, collective 'reduce' or 'host'")
            _check(lib().pt_test_group_create_virtual(C.byref(h), n, (C.c_int32 * n)(*virtual), 1 if collective == "reduce" else 0))
        else:
            dv = None if devices is None else (C.c_int32 * n)(*devices)
            _check(lib().pt_group_create(C.byref(h), n, dv))
        self.handle, self.n, self._scene = h, n, None

    @property
    def collective(self):
        return lib().pt_group_collective(self.handle).decode()

    def init(self, scene, traceDepth=None, flags=0, pipeline_depth=0, max_batch=0, lens_radius=0.0, focal_distance=0.0):
        geoms, mats, cam = (np.ascontiguousarray(x) for x in (scene.geoms, scene.materials, scene.camera))
        arr, nm, alive = _mesh_array(getattr(scene, "meshes", None) or {}, getattr(scene, "mesh_normals", None), getattr(scene, "mesh_materials", None))
        _check(lib().pt_group_set_meshes(self.handle, arr, nm))
        tarr, nt, barr, nb, alive_t = _texture_arrays(*_scene_textures(scene))
        _check(lib().pt_group_set_textures(self.handle, tarr, nt, C.sizeof(PtTexture), barr, nb, C.sizeof(PtTexBinding)))
        bbarr, nbb, alive_b = _bump_arrays(*_scene_bumps(scene))
        _check(lib().pt_group_set_bump_maps(self.handle, bbarr, nbb, C.sizeof(PtBumpBinding)))
        opt = PtOptions(0, 1, -1, flags, pipeline_depth, max_batch, None, None, lens_radius, focal_distance)
        _check(lib().pt_group_init(self.handle, _p(cam), _p(geoms), len(geoms), _p(mats), len(mats),
                                   scene.traceDepth if traceDepth is None else traceDepth, C.byref(opt)))
        self._scene = scene

    def iterate_batch(self, first_iteration, count, frame=0):
        _check(lib().pt_group_iterate_batch(self.handle, frame, first_iteration, count))

    def iterate(self, iteration, frame=0):
        """config C3 as written: one iteration on every member, then the frame's (asynchronous) assembly"""
        _check(lib().pt_group_iterate(self.handle, frame, iteration))

    def reduce(self):
        """assemble the frame from what has been committed so far (asynchronous)"""
        _check(lib().pt_group_reduce(self.handle))

    def sync(self):
        _check(lib().pt_group_sync(self.handle))

    def readback(self):
        res = self._scene.camera["resolution"][0]
        out = np.empty(int(res[0]) * int(res[1]) * 3, np.float32)
        _check(lib().pt_group_readback(self.handle, _p(out)))
        return out

    def counters(self):
        c = PtCounters()
        _check(lib().pt_group_counters(self.handle, C.byref(c)))
        return c

    def destroy(self):
        if self.handle:
            lib().pt_group_destroy(self.handle)
            self.handle = None


def save_png(basename, image_sum, samples):
    """saveImage + image::savePNG (reference src/main.cpp:49-70, src/image.cpp:22-39): divide by the
    sample count, mirror X, clamp, x255, truncate; writes <basename>.png."""
    img = np.ascontiguousarray(image_sum, np.float32)
    h, w = img.shape[0], img.shape[1]
    rc = host_lib().pth_save_png(os.fsencode(basename), _p(img), w, h, C.c_float(samples))
    if rc != 0:
        raise IOError("could not write %s.png" % basename)


def save_hdr(basename, image_sum, samples):
    """saveImage + image::saveHDR (reference src/main.cpp:49-70, src/image.cpp:41-45): writes <basename>.hdr."""
    img = np.ascontiguousarray(image_sum, np.float32)
    h, w = img.shape[0], img.shape[1]
    if host_lib().pth_save_hdr(os.fsencode(basename), _p(img), w, h, C.c_float(samples)) != 0:
        raise IOError("could not write %s.hdr" % basename)


# --------------------------------------------------------------------------- primitive / scan entry points (host arrays)
def _geoms_args(geoms):
    """a PtGeom array as the entry points take it: (pointer, count)"""
    g = np.ascontiguousarray(geoms)
    return _p(g), len(g)


def _camera_args(camera, geoms):
    """(camera pointer, geoms pointer, count)"""
    return (_p(np.ascontiguousarray(camera)),) + _geoms_args(geoms)


def _mesh_args(geom, tris):
    """one mesh geom and its triangles: (geom pointer, triangles pointer, triangle count)"""
    tr = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    return _p(np.ascontiguousarray(geom).reshape(-1)[:1]), _p(tr), len(tr)


def _u64_outs(fn, sizes, *args, then=()):
    """fn(*args, one uint64 array of each of `sizes` by reference, *then) -> every value of them in order, as ints"""
    outs = [(C.c_uint64 * n)() for n in sizes]
    _tcheck(fn(*args, *outs, *then))
    return tuple(int(v) for a in outs for v in a)


def _ray_hits(rays, sentinel):
    """the rays of an intersect test, their count, and its per-ray outputs t, p, n, outside, culled as the kernels expect to find them"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = len(rays)
    return rays, n, (np.empty(n, np.float32), np.full((n, 3), sentinel, np.float32), np.full((n, 3), sentinel, np.float32),
                     np.ones(n, np.int32), np.zeros(n, np.int32))


def _sized_camera_list(fn, camera, geoms, shard_rank, shard_count, faces):
    """camera_list / camera_resolved in their two calls: the sizes with null arrays, then the arrays.  -> None where no list is built, else
    ([pix, wave ranges, signature entries, and with `faces` the per-wave faces], sizes)"""
    args = _camera_args(camera, geoms) + (shard_rank, shard_count)
    sizes = np.zeros(4, np.int64)
    _tcheck(fn(*args, *[None] * (4 if faces else 3), _p(sizes)))
    if sizes[0] < 0:
        return None
    n = int(sizes[0])
    out = [np.zeros(n, np.uint32), np.zeros((n // 64, 2), np.int32), np.zeros(int(sizes[1]), np.int32)]
    if faces:
        out.append(np.zeros(n // 64, np.int32))
    _tcheck(fn(*args, *[_p(a) for a in out], _p(sizes)))
    return out, sizes


def test_utilhash(x):
    x = np.ascontiguousarray(x, np.uint32)
    out = np.empty_like(x)
    _tcheck(test_lib().pt_test_utilhash(_p(x), _p(out), x.size))
    return out


def test_rng(seeds, ndraws):
    seeds = np.ascontiguousarray(seeds, np.uint32)
    out = np.empty((seeds.size, ndraws), np.float32)
    _tcheck(test_lib().pt_test_rng(_p(seeds), seeds.size, ndraws, _p(out)))
    return out


def test_intersect(geoms, geom_index, rays, sentinel=-7.0):
    gi = np.ascontiguousarray(geom_index, np.int32)
    rays, n, outs = _ray_hits(rays, sentinel)
    _tcheck(test_lib().pt_test_intersect(*_geoms_args(geoms), _p(gi), _p(rays), n, *[_p(a) for a in outs[:4]]))
    return outs[:4]


def test_mesh_intersect(geom, tris, rays, flat=False, sentinel=-7.0):
    """Rays against one mesh geom on the GPU (hierarchy, or flat=True: plain triangle list).  Returns t, p, n, outside, culled."""
    rays, n, outs = _ray_hits(rays, sentinel)
    _tcheck(test_lib().pt_test_mesh_intersect(*_mesh_args(geom, tris), 1 if flat else 0, _p(rays), n, *[_p(a) for a in outs]))
    return outs


def test_mesh_intersect2(geom, tris, rays, normals=None, materials=None, flat=False, sentinel=-7.0):
    """test_mesh_intersect with the mesh's attributes (normals (ntris, 9), materials (ntris,) or None) and the winner's name.  Returns t, p, n,
    outside, culled, tri (the file index of the triangle that was hit, -1 on a miss), face_mat (its own material; -1: none, or a miss)."""
    g, tr, nt = _mesh_args(geom, tris)
    nrm = None if normals is None else _p(np.ascontiguousarray(normals, np.float32).reshape(nt, 9))
    mat = None if materials is None else _p(np.ascontiguousarray(materials, np.int32).reshape(nt))
    rays, n, outs = _ray_hits(rays, sentinel)
    outs += (np.full(n, -2, np.int32), np.full(n, -2, np.int32))
    _tcheck(test_lib().pt_test_mesh_intersect2(g, tr, nrm, mat, nt, 1 if flat else 0, _p(rays), n, *[_p(a) for a in outs]))
    return outs


def test_mesh_cull_sweep(geom, tris, seed, rays):
    """Device sweep of the bounding-ball test of one mesh geom.  Returns (culled, violations, hits)."""
    return _u64_outs(test_lib().pt_test_mesh_cull_sweep, (1, 1, 1), *_mesh_args(geom, tris), seed, rays)


MESH_LEAF = 0x80000000
# the two kinds of 64-byte record of a mesh (pt_device.h: MeshRec)
MESH_TRI_DTYPE = np.dtype([("v0", "<f4", 3), ("v1", "<f4", 3), ("v2", "<f4", 3), ("margin", "<f4"), ("pad", "<u4", 2)])
MESH_NODE_DTYPE = np.dtype([("planes", "<f2", 6), ("ref", "<u4"), ("far_planes", "<f2", 6), ("far_ref", "<u4")])
MESH_TRI_UNITS, MESH_NODE_UNITS = 3, 2


def mesh_bvh(tris, octant=0):
    """The hierarchy pt_init builds for a mesh (host only), in the layout for rays of direction octant `octant` (bit a set:
    component a negative) -> (triangle records [ntris], inner nodes [max(ntris - 1, 1)], first unit of the inner nodes, stack
    levels a lane needs).  A node holds the boxes and refs of its near (planes, ref) and far (far_planes, far_ref) child, a box
    as six half-precision planes: the three a ray of the octant enters through (lo where its direction is positive, hi where
    negative), then the three it leaves through; lo rounded down, hi up.  Refs count units of 16 bytes: with MESH_LEAF set it is
    triangle (ref & ~MESH_LEAF) / 3, any other is inner node (ref - first unit) / 2."""
    tr = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    nt = len(tr)
    out = np.zeros((5 * nt + 4, 4), np.uint32)
    n, need = C.c_int(len(out)), C.c_int(0)
    _tcheck(test_lib().pt_test_mesh_bvh(_p(tr), nt, octant, _p(out), C.byref(n), C.byref(need)))
    first = 3 * nt + (3 * nt) % 2
    assert n.value == first + 2 * max(nt - 1, 1)
    return (out[:3 * nt].reshape(-1).view(MESH_TRI_DTYPE).reshape(-1), out[first:n.value].reshape(-1).view(MESH_NODE_DTYPE).reshape(-1),
            first, need.value)


def test_hemisphere(normals, iter_index_depth):
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    iid = np.ascontiguousarray(iter_index_depth, np.int32).reshape(-1, 3)
    out = np.empty_like(normals)
    _tcheck(test_lib().pt_test_hemisphere(_p(normals), _p(iid), len(normals), _p(out)))
    return out


def test_texture_sample(texture, uv):
    """The kernels' bilinear texture lookup on the GPU: texture (H, W, 3) float32 (row 0 = top), uv (n, 2) -> (n, 3) float32."""
    t = np.ascontiguousarray(texture, np.float32)
    u = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    out = np.empty((len(u), 3), np.float32)
    _tcheck(test_lib().pt_test_texture_sample(_p(t), t.shape[1], t.shape[0], _p(u), len(u), _p(out)))
    return out


def test_texture_uv(kind, inp, face=None):
    """The kernels' texture coordinates on the GPU: kind 0 sphere / 1 cube (inp (n, 3) object-space hit points, face (n,) int32 for cubes),
    2 mesh (inp (n, 8): barycentric u, v and the corner UVs u0 v0 u1 v1 u2 v2) -> (n, 2) float32."""
    a = np.ascontiguousarray(inp, np.float32).reshape(len(inp), -1)
    f = None if face is None else np.ascontiguousarray(face, np.int32)
    out = np.empty((len(a), 2), np.float32)
    _tcheck(test_lib().pt_test_texture_uv(kind, _p(a), None if f is None else _p(f), len(a), _p(out)))
    return out


def test_bump_normal(height, kind, inp):
    """The kernels' bump mapping on the GPU (include/pt_amd_test.h, pt_test_bump_normal): height (H, W) float32 (row 0 = top), kind (n,) int32,
    inp (n, 40) float32 -> (n, 16) float32 {hu, hv, Pu, Pv, Ns, bumped, u, v, 0, 0}."""
    hm = np.ascontiguousarray(height, np.float32)
    k = np.ascontiguousarray(kind, np.int32).reshape(-1)
    a = np.ascontiguousarray(inp, np.float32).reshape(len(k), 40)
    out = np.empty((len(k), 16), np.float32)
    _tcheck(test_lib().pt_test_bump_normal(_p(hm), hm.shape[1], hm.shape[0], _p(k), _p(a), len(k), _p(out)))
    return out


def test_sincos(x):
    x = np.ascontiguousarray(x, np.float32)
    s, c = np.empty_like(x), np.empty_like(x)
    _tcheck(test_lib().pt_test_sincos(_p(x), x.size, _p(s), _p(c)))
    return s, c


def test_pow(x, e):
    x = np.ascontiguousarray(x, np.float32)
    e = np.ascontiguousarray(e, np.float32)
    out = np.empty_like(x)
    _tcheck(test_lib().pt_test_pow(_p(x), _p(e), x.size, _p(out)))
    return out


def test_reflect_refract(I, N, eta):
    I = np.ascontiguousarray(I, np.float32).reshape(-1, 3)
    N = np.ascontiguousarray(N, np.float32).reshape(-1, 3)
    eta = np.ascontiguousarray(eta, np.float32)
    r1, r2 = np.empty_like(I), np.empty_like(I)
    _tcheck(test_lib().pt_test_reflect_refract(_p(I), _p(N), _p(eta), len(I), _p(r1), _p(r2)))
    return r1, r2


def test_slab_quotients(o, d):
    o = np.ascontiguousarray(o, np.float32)
    d = np.ascontiguousarray(d, np.float32)
    out = [np.empty_like(o) for _ in range(4)]
    _tcheck(test_lib().pt_test_slab_quotients(_p(o), _p(d), o.size, *[_p(a) for a in out]))
    return out


def test_slab_quotients_sweep(seed, pairs):
    return _u64_outs(test_lib().pt_test_slab_quotients_sweep, (1,), seed, pairs)[0]


def test_unscaled_sqrt_sweep():
    return list(_u64_outs(test_lib().pt_test_unscaled_sqrt_sweep, (4,)))


def test_sphere_cull_sweep(geoms, seed, rays):
    return _u64_outs(test_lib().pt_test_sphere_cull_sweep, (1, 1), *_geoms_args(geoms), seed, rays)


def test_sphere_halfline_sweep(geoms, seed, rays):
    """-> (certified misses, of them with the centre behind the origin, violations)"""
    return _u64_outs(test_lib().pt_test_sphere_halfline_sweep, (1, 1, 1), *_geoms_args(geoms), seed, rays)


def _cluster_info(info):
    """pt_test_sphere_clusters' info18 -> {omax, n0, boxes (2, 6): lo, hi}"""
    return {"omax": float(info[0]), "n0": int(info[1]), "boxes": info[2:].reshape(2, 8)[:, :6].copy()}


def test_sphere_cluster_sweep(geoms, seed, rays):
    """geoms: a whole scene (spheres and cubes) -> (certificates issued per cluster [2], violations, {omax, n0, boxes[2][6]})"""
    info = np.zeros(18, np.float32)
    c0, c1, bad = _u64_outs(test_lib().pt_test_sphere_cluster_sweep, (2, 1), *_geoms_args(geoms), seed, rays, then=(info.ctypes.data,))
    return [c0, c1], bad, _cluster_info(info)


def test_sphere_group_sweep(geoms, seed, rays):
    """(group certificates issued, violations, groups): pt_test_sphere_group_sweep"""
    ng = C.c_int32()
    return _u64_outs(test_lib().pt_test_sphere_group_sweep, (1, 1), *_geoms_args(geoms), seed, rays, then=(C.byref(ng),)) + (int(ng.value),)


def sphere_clusters(geoms):
    """The two clusters of spheres pt_init builds for a sphere-heavy scene without meshes (host only).
    -> {omax, n0, boxes (2, 6): lo, hi}, table (primitive index per entry of the sweep's table: cluster 0 first, n0 entries)"""
    info = np.zeros(18, np.float32)
    table = np.zeros(len(geoms) + 2, np.int32)
    n = C.c_int32(0)
    _tcheck(test_lib().pt_test_sphere_clusters(*_geoms_args(geoms), info.ctypes.data, table.ctypes.data, len(table), C.byref(n)))
    return _cluster_info(info), table[:n.value].copy()


def test_wall_box_sweep(geoms, seed, rays):
    return _u64_outs(test_lib().pt_test_wall_box_sweep, (1, 1), *_geoms_args(geoms), seed, rays)


def test_slab_decisions(cube, org, dirs):
    """pt_test_slab_decisions: the slab certificate's two evaluations on the caller's rays against one cube.  Returns (flags (n,) uint32 --
    bit 0 shared reciprocals, bit 1 axis by axis, bit 2 the origin within the box's bound, bit 3 the full box test hits --, box lo (3,),
    box hi (3,), the bound)."""
    g = np.ascontiguousarray(cube).reshape(-1)[:1]
    rays = np.ascontiguousarray(np.concatenate([np.asarray(org, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)], axis=1))
    flags, box = np.zeros(len(rays), np.uint32), np.zeros(7, np.float32)
    _tcheck(test_lib().pt_test_slab_decisions(_p(g), _p(rays), len(rays), _p(flags), _p(box)))
    return flags, box[:3].copy(), box[3:6].copy(), np.float32(box[6])


def camera_cull_tables(camera, geoms):
    """The camera-ray culling tables pt_init derives (host only).  Returns (rects (n, 4), scene rect (4,), spans (H, n, 2))."""
    H = int(np.ascontiguousarray(camera)["resolution"][0][1])
    rects = np.zeros((len(geoms), 4), np.int32)
    scene = np.zeros(4, np.int32)
    spans = np.zeros((H, len(geoms), 2), np.int32)
    _tcheck(test_lib().pt_test_camera_cull_tables(*_camera_args(camera, geoms), _p(rects), _p(scene), _p(spans)))
    return rects, scene, spans


def camera_list(camera, geoms, shard_rank=0, shard_count=1):
    """The camera rays' packed work list pt_init builds for one shard (host only, no length cap).  Returns None where it is not built,
    else (pix (n,) uint32: x | y << 16 or 0xffffffff, wave ranges (n / 64, 2), signature entries, pixels listed, pixels of the shard)."""
    r = _sized_camera_list(test_lib().pt_test_camera_list, camera, geoms, shard_rank, shard_count, False)
    return r and (*r[0], int(r[1][2]), int(r[1][3]))


def camera_resolved(camera, geoms, shard_rank=0, shard_count=1):
    """camera_list as pt_init builds it for the untextured forms: one-cube signatures split by the cube face their pixels' camera rays are
    certified to enter through (host only, no length cap).  Returns None where the list is not built, else (pix, wave ranges, signature
    entries, per wave its face 2 axis + (side > 0) or -1)."""
    r = _sized_camera_list(test_lib().pt_test_camera_resolved, camera, geoms, shard_rank, shard_count, True)
    return r and tuple(r[0])


def camera_resolved_device(camera, geoms, shard_rank=0, shard_count=1, with_ms=False):
    """camera_resolved with the face certificates evaluated on the device (k_camera_faces), as the camera move (pathtraceSetCamera) evaluates them: the same four
    arrays, or None.  with_ms: -> (arrays or None, the launches' time in ms by HIP events)."""
    ms = C.c_float(0.0)
    fn = test_lib().pt_test_camera_resolved_device
    r = _sized_camera_list(lambda *a: fn(*a, C.byref(ms)), camera, geoms, shard_rank, shard_count, True)
    res = r and tuple(r[0])
    return (res, ms.value) if with_ms else res


def test_face_hit_sweep(camera, geoms, samples=64, seed=1):
    """Device sweep of the resolved waves' box test against the full one.  Returns (rays, mismatches, resolved pixels)."""
    return _u64_outs(test_lib().pt_test_face_hit_sweep, (3,), *_camera_args(camera, geoms), samples, seed)


def wall_faces(scene, traceDepth=None, **options):
    """pt_test_wall_faces: the inner face pt_init would name per primitive of the scene (2 axis + (side > 0), -1: none) and the clearance
    that goes with it, on the host alone (no GPU).  options: PtOptions fields by name, as for scene_plan."""
    T = test_lib()
    set_meshes(getattr(scene, "meshes", None) or {}, getattr(scene, "mesh_normals", None), getattr(scene, "mesh_materials", None), L=T)
    set_textures(*_scene_textures(scene), L=T)
    set_bump_maps(*_scene_bumps(scene), L=T)
    opt = PtOptions(shard_count=1, device=-1)
    for name, value in options.items():
        setattr(opt, name, value)
    geoms, mats, cam = np.ascontiguousarray(scene.geoms), np.ascontiguousarray(scene.materials), np.ascontiguousarray(scene.camera)
    face, beyond = np.full(len(geoms), -2, np.int32), np.zeros(len(geoms), np.float32)
    _check(T.pt_test_wall_faces(_p(cam), _p(geoms), len(geoms), _p(mats), len(mats), scene.traceDepth if traceDepth is None else traceDepth,
                                C.byref(opt), _p(face), _p(beyond)), T)
    return face, beyond


def test_wall_face_sweep(geoms, seed, rays):
    """Device sweep of the later bounces' face certificate and its resolved box test against the box test, on the walls among `geoms`
    (cubes).  Returns (accepted, mismatching, rejected although the box test hits through the face, rejected in all)."""
    return _u64_outs(test_lib().pt_test_wall_face_sweep, (4,), *_geoms_args(geoms), seed, rays)


def wall_resolve_tally():
    """The test library's tally of its renderer's later bounces since the last call (read and cleared): (wave-tiles that hold a path, of
    them one-wall tiles whose wall has a face, of those the waves that took the face, lanes whose certificate failed)."""
    return _u64_outs(test_lib().pt_test_wall_resolve_tally, (4,))


def candidate_tally():
    """The test library's tally of its renderer's candidate tiles since the last call (read and cleared): (later wave-tiles that hold a
    path, of them candidate tiles, of those tiles of one wall that has an inner face, lanes of candidate tiles that hit a binned primitive,
    scattered paths of a binning scene, of them candidates by the balls alone, candidates by the rule in force, candidates by the balls
    beside that rule)."""
    return _u64_outs(test_lib().pt_test_candidate_tally, (8,))


def group_tally():
    """The test library's tally of its renderer's grouped sweep since the last call (read and cleared): (rounds of 64 groups run, waves that
    ran level 2 from LDS, waves that ran it from global memory, calls of passes() from inside the group loop, group words parked, the
    largest number of words a lane had parked at once)."""
    return _u64_outs(test_lib().pt_test_group_tally, (6,))


def sphere_groups(scene, traceDepth=None, **options):
    """pt_test_sphere_groups: the swept primitives' table pt_init would build for the scene, on the host alone (no GPU), even where a later
    phase of the plan refuses the scene.  options: PtOptions fields by name, as for scene_plan.  -> a namespace of table (primitive per
    entry, padding included), centre (n, 3), threshold (n,), K (n,) per entry, n0, grpN0, nSphGroups, nswept, grouped, grpOMax, sphDirScale,
    balls (nSphGroups, 4): {centre, threshold}."""
    import types
    T = test_lib()
    set_meshes(getattr(scene, "meshes", None) or {}, getattr(scene, "mesh_normals", None), getattr(scene, "mesh_materials", None), L=T)
    set_textures(*_scene_textures(scene), L=T)
    set_bump_maps(*_scene_bumps(scene), L=T)
    opt = PtOptions(shard_count=1, device=-1)
    for name, value in options.items():
        setattr(opt, name, value)
    geoms, mats, cam = np.ascontiguousarray(scene.geoms), np.ascontiguousarray(scene.materials), np.ascontiguousarray(scene.camera)
    cap = 2 * len(geoms) + 32
    table, entries, balls = np.zeros(cap, np.int32), np.zeros((cap, 5), np.float32), np.zeros((cap, 4), np.float32)
    info, bounds = np.zeros(6, np.int32), np.zeros(2, np.float32)
    _check(T.pt_test_sphere_groups(_p(cam), _p(geoms), len(geoms), _p(mats), len(mats), scene.traceDepth if traceDepth is None else traceDepth,
                                   C.byref(opt), _p(table), _p(entries), cap, _p(balls), cap, _p(info), _p(bounds)), T)
    n, ng = int(info[0]), int(info[3])
    return types.SimpleNamespace(table=table[:n].copy(), centre=entries[:n, :3].copy(), threshold=entries[:n, 3].copy(), K=entries[:n, 4].copy(),
                                 n0=int(info[1]), grpN0=int(info[2]), nSphGroups=ng, nswept=int(info[4]), grouped=bool(info[5]),
                                 grpOMax=float(bounds[0]), sphDirScale=float(bounds[1]), balls=balls[:ng].copy())


def test_camera_cull_sweep(camera, geoms, samples=1):
    """Device sweep of the camera-ray culling for one (camera, primitive set).  Returns (hits, culled pairs, violations)."""
    return _u64_outs(test_lib().pt_test_camera_cull_sweep, (1, 1, 1), *_camera_args(camera, geoms), samples)


def test_camera_cull_margin(camera, geoms, samples=1):
    """Device measurement of the culling tables' inflation margin for one (camera, primitive set).  Returns (largest fraction of the
    inflation a hit of the reference's test needed, hits that needed any)."""
    w = C.c_double()
    needed, = _u64_outs(test_lib().pt_test_camera_cull_margin, (1,), *_camera_args(camera, geoms), samples, C.byref(w))
    return float(w.value), needed


def test_box_fast_sweep(geoms, seed, rays):
    """Device sweep of the box test's fast slab phase against the reference's loop.  Returns (rays, decided by the fast path, hits
    among those, bit mismatches, mismatches of the fast reciprocal, mismatches of the fast quotient)."""
    return _u64_outs(test_lib().pt_test_box_fast_sweep, (4, 2), *_geoms_args(geoms), seed, rays)


def test_wall_plane_sweep(geoms, seed, rays):
    """Device sweep of the one-plane-per-wall certificates.  Returns (walls with a plane, certified, violations, single-wall rays)."""
    n = C.c_int32(0)
    counts = _u64_outs(test_lib().pt_test_wall_plane_sweep, (1, 1, 1), *_geoms_args(geoms), seed, rays, C.byref(n))
    return (int(n.value),) + counts


def test_wall_planes(geoms):
    """Host only (no GPU): the planes pt_init keeps for rotated walls.  Returns (planes [nplane][5] = normal, threshold, far; wall_geom, nslot, nwalls)."""
    planes = np.zeros((6, 5), np.float32)
    wg = np.zeros(6, np.int32)
    ns, npl, nw = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _tcheck(test_lib().pt_test_wall_planes(*_geoms_args(geoms), _p(planes), _p(wg), C.byref(ns), C.byref(npl), C.byref(nw)))
    return planes[:npl.value].copy(), wg[:nw.value].copy(), int(ns.value), int(nw.value)


def scan_exclusive_dev(in_ptr, out_ptr, n, stream=0):
    _check(lib().pt_scan_exclusive_i32(in_ptr, out_ptr, n, stream or None))


def compact_nonzero_dev(in_ptr, out_ptr, n, count_ptr, stream=0):
    _check(lib().pt_compact_nonzero_i32(in_ptr, out_ptr, n, count_ptr, stream or None))
