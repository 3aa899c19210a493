"""ctypes mirror of include/rt_abi.h and include/rt_host.h.

The structs below are field-for-field copies of the C ABI (which in turn
mirrors the reference's Material / Primitive / Camera / SceneSettings /
FilterCache / AccumulationBuffer, RT/scene.h:15-120, RT/Raytracer.h:34-48).
No torch types cross the boundary: pointers and sizes only.
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "lib", "librt_mi355x.so")

RT_OK = 0
RT_ERROR_INVALID = 1
RT_ERROR_DEVICE = 2
RT_ERROR_OUT_OF_MEMORY = 3
RT_ERROR_CANCELLED = 4
RT_ERROR_NO_DEVICE = 5

RT_MATERIAL_MIRROR = 0x1
RT_MATERIAL_CHECKERS = 0x2
RT_MATERIAL_EMISSIVE = 0x4

RT_PRIMITIVE_NONE, RT_PRIMITIVE_PLANE, RT_PRIMITIVE_SPHERE, RT_PRIMITIVE_BOX, RT_PRIMITIVE_MESH = range(5)
RT_SAMPLING_UNIFORM, RT_SAMPLING_OPTIMIZED_BLUE_NOISE, RT_SAMPLING_STRATIFIED = range(3)
RT_SPLAT_STREAM, RT_SPLAT_EXACT, RT_SPLAT_ATOMIC = range(3)          # rt_splat_mode
RT_SHARD_TILES, RT_SHARD_PASSES = range(2)                           # rt_shard_mode
RT_SHADOW_LAUNCH_AUTO, RT_SHADOW_LAUNCH_SEPARATE, RT_SHADOW_LAUNCH_MERGED = range(3)   # rt_shadow_launch (ABI 8)
# rt_integrator: the reference's g_integrators table indices (RT/integrators.cpp:823-830)
(RT_INTEGRATOR_ADVANCED, RT_INTEGRATOR_WHITTED, RT_INTEGRATOR_GROUND_TRUTH_RECURSIVE,
 RT_INTEGRATOR_GROUND_TRUTH_ITERATIVE, RT_INTEGRATOR_NORMALS, RT_INTEGRATOR_DISTANCES) = range(6)
RT_INTEGRATOR_COUNT = 6
RT_RNG_PER_SAMPLE, RT_RNG_TILE_STREAM = 0, 1
(RT_MESH_TABLE_TRIANGLES, RT_MESH_TABLE_NORMALS, RT_MESH_TABLE_NODES_SRC, RT_MESH_TABLE_NODES, RT_MESH_TABLE_NODES4,
 RT_MESH_TABLE_MID4, RT_MESH_TABLE_BVH4_SOURCES, RT_MESH_TABLE_REFIT_PLAN, RT_MESH_TABLE_COUNT) = range(9)   # rt_mesh_table
RT_HIT_MISS = 0xFFFFFFFF
RT_HIT_PLANE_BIT = 0x80000000
RTH_BVH_MIDPOINT_SPLIT, RTH_BVH_SAH_BINNED, RTH_BVH_SAH_FULL = range(3)
RT_BVH_BUILD_MIDPOINT, RT_BVH_BUILD_SAH_BINNED, RT_BVH_BUILD_SAH_FULL = range(3)   # rt_bvh_build_method

RT_KERNEL_NAMES = ("generate", "extend", "shade", "connect", "splat", "resolve")
RT_KERNEL_COUNT = 6


class V3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def __iter__(self):
        return iter((self.x, self.y, self.z))

    def __repr__(self):
        return f"V3({self.x}, {self.y}, {self.z})"


def v3(x, y=None, z=None):
    if y is None:
        return V3(x, x, x)
    return V3(x, y, z)


class M4x4(C.Structure):
    _fields_ = [("e", (C.c_float * 4) * 4)]


class M4x4Inv(C.Structure):
    _fields_ = [("forward", M4x4), ("inverse", M4x4)]


class Material(C.Structure):          # RT/scene.h:15-29
    _fields_ = [("flags", C.c_uint32), ("albedo", V3), ("checker_color", V3), ("emission_color", V3),
                ("ior", C.c_float), ("metallic", C.c_float), ("roughness", C.c_float),
                ("is_participating_medium", C.c_int32), ("absorb", V3)]


class Primitive(C.Structure):         # RT/primitives.h:92-106
    _fields_ = [("transform_index", C.c_uint32), ("material_id", C.c_uint32), ("type", C.c_uint32),
                ("mesh_index", C.c_uint32), ("p", C.c_float * 4)]


class BvhNode(C.Structure):           # RT/bvh.h:31-37
    _fields_ = [("bv_p", V3), ("bv_r", V3), ("left_first", C.c_uint32), ("count", C.c_uint16),
                ("split_axis", C.c_uint16)]


class Mesh(C.Structure):
    _fields_ = [("triangle_count", C.c_uint32), ("has_normals", C.c_uint32),
                ("triangles", C.POINTER(V3)), ("indices", C.POINTER(C.c_uint32)),
                ("normals", C.POINTER(V3)), ("node_count", C.c_uint32), ("nodes", C.POINTER(BvhNode))]


class SceneDesc(C.Structure):         # RT/scene.h:92-120
    _fields_ = [("material_count", C.c_uint32), ("materials", C.POINTER(Material)),
                ("primitive_count", C.c_uint32), ("primitives", C.POINTER(Primitive)),
                ("plane_count", C.c_uint32), ("planes", C.POINTER(Primitive)),
                ("transform_count", C.c_uint32), ("transforms", C.POINTER(M4x4Inv)),
                ("light_count", C.c_uint32), ("lights", C.POINTER(C.c_uint32)),
                ("mesh_count", C.c_uint32), ("meshes", C.POINTER(Mesh)),
                ("bvh_node_count", C.c_uint32), ("bvh_nodes", C.POINTER(BvhNode)),
                ("bvh_index_count", C.c_uint32), ("bvh_indices", C.POINTER(C.c_uint32)),
                ("top_sky_color", V3), ("bot_sky_color", V3),
                ("skydome_w", C.c_uint32), ("skydome_h", C.c_uint32), ("skydome", C.POINTER(V3))]


class Camera(C.Structure):            # RT/scene.h:31-46
    _fields_ = [("p", V3), ("x", V3), ("y", V3), ("z", V3), ("vfov", C.c_float), ("aspect_ratio", C.c_float),
                ("lens_radius", C.c_float), ("focus_distance", C.c_float), ("film_distance", C.c_float),
                ("half_film_w", C.c_float), ("half_film_h", C.c_float)]


class Settings(C.Structure):          # RT/scene.h:64-82
    _fields_ = [("next_event_estimation", C.c_int32), ("importance_sample_lights", C.c_int32),
                ("importance_sample_diffuse", C.c_int32), ("use_mis", C.c_int32),
                ("russian_roulette", C.c_int32), ("caustics", C.c_int32),
                ("sampling_strategy", C.c_int32), ("use_path_guide", C.c_int32),
                ("vignette_strength", C.c_float), ("lens_distortion", C.c_float), ("f_factor", C.c_float),
                ("diaphragm_edges", C.c_float), ("phi_shutter_max", C.c_float),
                ("samples_per_pixel", C.c_uint32), ("max_bounce_count", C.c_uint32), ("integrator", C.c_int32)]


class FilterCache(C.Structure):       # RT/Raytracer.h:34-40
    _fields_ = [("kernel_size", C.c_uint32), ("cache_size", C.c_uint32), ("cache", C.c_float * 512)]


class AccumulationBuffer(C.Structure):  # RT/Raytracer.h:44-48
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("frame_count", C.c_uint32), ("pixels", C.POINTER(C.c_float))]


class TileSet(C.Structure):
    _fields_ = [("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("shard_index", C.c_uint32), ("shard_count", C.c_uint32)]


TRAVERSAL_FIELDS = ("mesh_intersection_count", "mesh_bvh_traversals", "mesh_node_traversals", "mesh_leaf_traversals")


class TraversalStats(C.Structure):    # TraversalStats RT/intersection.h:33-40 (rt_traversal_stats)
    _fields_ = [(f, C.c_uint64) for f in TRAVERSAL_FIELDS]

    def as_dict(self):
        return {f: getattr(self, f) for f in TRAVERSAL_FIELDS}


class Stats(C.Structure):
    _fields_ = [("closest_hit_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("samples", C.c_uint64),
                ("iterations", C.c_uint64), ("seconds", C.c_double),
                ("kernel_ms", C.c_double * RT_KERNEL_COUNT), ("kernel_launches", C.c_uint64 * RT_KERNEL_COUNT),
                ("traced_rays", C.c_uint64 * 2), ("splat_mode", C.c_int32), ("shadow_launch", C.c_int32),
                ("traversal", TraversalStats * 2), ("trace_steps", C.c_uint64 * 2),
                ("traversal_ref", TraversalStats * 2)]       # ABI 7: rt_scene_config::traversal_ref

    def traversal_total(self):
        """The reference's TraversalStats: both query kinds summed."""
        return {f: getattr(self.traversal[0], f) + getattr(self.traversal[1], f) for f in TRAVERSAL_FIELDS}

    def as_dict(self):
        return {"closest_hit_rays": self.closest_hit_rays, "shadow_rays": self.shadow_rays,
                "samples": self.samples, "iterations": self.iterations, "seconds": self.seconds,
                "kernel_ms": {RT_KERNEL_NAMES[i]: self.kernel_ms[i] for i in range(6)},
                "kernel_launches": {RT_KERNEL_NAMES[i]: self.kernel_launches[i] for i in range(6)},
                "traced_rays": [self.traced_rays[0], self.traced_rays[1]], "splat_mode": self.splat_mode,
                "traversal": [self.traversal[0].as_dict(), self.traversal[1].as_dict()],
                "trace_steps": [self.trace_steps[0], self.trace_steps[1]],
                "traversal_ref": [self.traversal_ref[0].as_dict(), self.traversal_ref[1].as_dict()]}


class RayQuery(C.Structure):
    _fields_ = [("o", V3), ("d", V3), ("max_t", C.c_float), ("ignored_primitive", C.c_uint32)]


class HitRecord(C.Structure):
    _fields_ = [("t", C.c_float), ("primitive", C.c_uint32), ("hit_p", V3), ("n", V3)]


class PostSettings(C.Structure):      # RT/scene.h:84-90
    _fields_ = [("exposure", C.c_float), ("tonemapping", C.c_int32), ("srgb_transform", C.c_int32),
                ("midpoint", C.c_float), ("contrast", C.c_float)]


RT_CONFIG_INHERIT = -1


class SceneConfig(C.Structure):       # rt_scene_config (per-scene schedule and splat settings)
    _fields_ = [("splat_mode", C.c_int32), ("shard_mode", C.c_int32), ("env_sampling", C.c_int32),
                ("partitions", C.c_int32), ("path_pool", C.c_int64), ("fuse_paths", C.c_int64),
                ("splat_chunk", C.c_int32), ("splat_ring", C.c_int32), ("sample_budget_gb", C.c_double),
                ("resolve_tall_pixels", C.c_int64), ("debug_traversal", C.c_int32), ("traversal_ref", C.c_int32),
                ("drain_every", C.c_int32), ("shadow_launch", C.c_int32),  # ABI 8
                ("ramp_shade", C.c_int32),      # 0 auto (on), 1 on, 2 off: the dense ramp-down shade
                ("reserved", C.c_int32 * 3)]


class DenoiseParams(C.Structure):     # rt_denoise_params (the denoise stage)
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_guide", C.c_float * 2),
                ("firefly_clamp", C.c_float), ("reserved", C.c_int32 * 3)]


RT_FEATURE_NORMAL, RT_FEATURE_DISTANCE, RT_FEATURE_ALBEDO = range(3)   # rt_feature (feature frames)
RT_FEATURE_COUNT = 3


class DenoiseFeaturesParams(C.Structure):     # rt_denoise_features_params (the denoise stage with feature frames)
    _fields_ = [("base", DenoiseParams), ("sigma_albedo", C.c_float), ("demodulate", C.c_int32),
                ("albedo_floor", C.c_float), ("reserved", C.c_int32 * 5)]


class TileErrorParams(C.Structure):    # rt_tile_error_params (adaptive sampling: the tile error estimate)
    _fields_ = [("floor", C.c_float), ("reserved", C.c_int32 * 3)]


class AdaptiveParams(C.Structure):     # rt_adaptive_params (adaptive sampling: the driver)
    _fields_ = [("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("step_spp", C.c_uint32), ("threshold", C.c_float),
                ("error", TileErrorParams), ("reserved", C.c_int32 * 4)]


class RobustParams(C.Structure):       # rt_robust_params (the robust estimator: a Gini-adaptive median of means)
    _fields_ = [("buffers", C.c_uint32), ("gini_scale", C.c_float), ("max_trim", C.c_uint32), ("reserved", C.c_int32 * 5)]


class GBufferTexel(C.Structure):       # rt_gbuffer_texel (temporal accumulation: the primary hit of a pixel), 32 bytes
    _fields_ = [("p", V3), ("t", C.c_float), ("n", V3), ("primitive", C.c_uint32)]


# the numpy layout of a G-buffer: np.zeros((h, w), GBUFFER_DTYPE)
GBUFFER_DTYPE = [("p", "<f4", (3,)), ("t", "<f4"), ("n", "<f4", (3,)), ("primitive", "<u4")]


class TemporalParams(C.Structure):     # rt_temporal_params (temporal accumulation: the accumulate stage)
    _fields_ = [("max_history", C.c_float), ("normal_cos", C.c_float), ("plane_tolerance", C.c_float),
                ("snap", C.c_float), ("firefly_clamp", C.c_float), ("reserved", C.c_int32 * 3)]


class TemporalState(C.Structure):      # rt_temporal_state (temporal accumulation: the driver's; all zero = no history)
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("frames", C.c_uint32), ("parity", C.c_uint32),
                ("camera", Camera), ("lens_distortion", C.c_float), ("d_workspace", C.c_void_p)]


class DenoiseVarianceParams(C.Structure):   # rt_denoise_variance_params (variance-guided filtering: the filter), 32 bytes
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_plane", C.c_float), ("variance_epsilon", C.c_float), ("firefly_clamp", C.c_float),
                ("reserved", C.c_int32 * 2)]


class TemporalFilteredState(C.Structure):   # rt_temporal_filtered_state (variance-guided filtering: the driver's)
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("frames", C.c_uint32), ("parity", C.c_uint32),
                ("camera", Camera), ("lens_distortion", C.c_float), ("d_workspace", C.c_void_p)]


RT_TEMPORAL_SPATIAL_BELOW_DEFAULT = 4.0


class MotionEntry(C.Structure):        # rt_motion_entry (moving instances: one primitive's rigid motion), 112 bytes
    _fields_ = [("inv_cur", (C.c_float * 4) * 3), ("fwd_prev", (C.c_float * 4) * 3), ("moved", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


# the numpy layout of a motion table: np.zeros(count, MOTION_DTYPE)
MOTION_DTYPE = [("inv_cur", "<f4", (3, 4)), ("fwd_prev", "<f4", (3, 4)), ("moved", "<u4"), ("reserved", "<u4", (3,))]
# and of rt_m4x4inv arrays: np.zeros(count, M4X4INV_DTYPE)
M4X4INV_DTYPE = [("forward", "<f4", (4, 4)), ("inverse", "<f4", (4, 4))]


class TemporalMotionState(C.Structure):     # rt_temporal_motion_state (moving instances: the driver's)
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("frames", C.c_uint32), ("parity", C.c_uint32),
                ("camera", Camera), ("lens_distortion", C.c_float), ("primitive_count", C.c_uint32),
                ("transform_cap", C.c_uint32), ("d_workspace", C.c_void_p), ("transforms", C.POINTER(M4x4Inv))]


class SurfaceTexel(C.Structure):       # rt_surface_texel (deforming meshes: where on which triangle a pixel's hit lies), 16 bytes
    _fields_ = [("triangle", C.c_uint32), ("v", C.c_float), ("w", C.c_float), ("reserved", C.c_uint32)]


# the numpy layout of a surface buffer: np.zeros((h, w), SURFACE_DTYPE)
SURFACE_DTYPE = [("triangle", "<u4"), ("v", "<f4"), ("w", "<f4"), ("reserved", "<u4")]


class DeformMesh(C.Structure):         # rt_deform_mesh (deforming meshes: one deformed mesh and last frame's vertices)
    _fields_ = [("mesh_index", C.c_uint32), ("reserved", C.c_uint32), ("d_prev_triangles", C.c_void_p),
                ("d_prev_normals", C.c_void_p)]


class DeformEntry(C.Structure):        # rt_deform_entry (deforming meshes: one primitive's entry of the table), 128 bytes
    _fields_ = [("inv_prev", (C.c_float * 4) * 3), ("fwd_prev", (C.c_float * 4) * 3), ("d_prev_triangles", C.c_void_p),
                ("d_prev_normals", C.c_void_p), ("triangle_count", C.c_uint32), ("deformed", C.c_uint32),
                ("has_normals", C.c_uint32), ("reserved", C.c_uint32)]


# the numpy layout of a deform table: np.zeros(count, DEFORM_DTYPE)
DEFORM_DTYPE = [("inv_prev", "<f4", (3, 4)), ("fwd_prev", "<f4", (3, 4)), ("d_prev_triangles", "<u8"),
                ("d_prev_normals", "<u8"), ("triangle_count", "<u4"), ("deformed", "<u4"), ("has_normals", "<u4"),
                ("reserved", "<u4")]


class NeighbourhoodTexel(C.Structure):  # rt_neighbourhood_texel (neighbourhood clipping: a window's statistics), 32 bytes
    _fields_ = [("mean", V3), ("count", C.c_float), ("sigma", V3), ("reserved", C.c_float)]


# the numpy layout of a neighbourhood buffer: np.zeros((h, w), NEIGHBOURHOOD_DTYPE)
NEIGHBOURHOOD_DTYPE = [("mean", "<f4", (3,)), ("count", "<f4"), ("sigma", "<f4", (3,)), ("reserved", "<f4")]


class TemporalClipParams(C.Structure):  # rt_temporal_clip_params (neighbourhood clipping: the driver's), 16 bytes
    _fields_ = [("radius", C.c_uint32), ("gamma", C.c_float), ("min_count", C.c_float), ("reserved", C.c_uint32)]


class SpecularTexel2(C.Structure):     # rt_specular_texel2 (the specular G-buffer's side record), 16 bytes
    _fields_ = [("first_primitive", C.c_uint32), ("first_t", C.c_float), ("chain", C.c_uint32), ("end", C.c_uint32)]


# the numpy layout of a side-record buffer: np.zeros((h, w), SPECULAR_CHAIN_DTYPE)
SPECULAR_CHAIN_DTYPE = [("first_primitive", "<u4"), ("first_t", "<f4"), ("chain", "<u4"), ("end", "<u4")]
# rt_specular_end
(RT_SPECULAR_END_MISS, RT_SPECULAR_END_EMITTER, RT_SPECULAR_END_DIFFUSE, RT_SPECULAR_END_ROUGH, RT_SPECULAR_END_STACK,
 RT_SPECULAR_END_CAP) = range(6)


class GBufferSpecularParams(C.Structure):   # rt_gbuffer_specular_params (the specular G-buffer: the walk's), 16 bytes
    _fields_ = [("max_events", C.c_uint32), ("reflect_threshold", C.c_float), ("roughness_max", C.c_float),
                ("reserved", C.c_uint32)]


class BvhInfo(C.Structure):
    _fields_ = [("node_count", C.c_uint32), ("leaf_count", C.c_uint32), ("max_depth", C.c_uint32),
                ("max_leaf_size", C.c_uint32)]


P = C.POINTER

# name -> (restype, argtypes)
ABI_FUNCTIONS = {
    "rt_abi_version": (C.c_int, []),
    "rt_last_error": (C.c_char_p, []),
    "rt_device_count": (C.c_int, [P(C.c_int)]),
    "rt_integrator_name": (C.c_char_p, [C.c_int]),
    "rt_find_integrator": (C.c_int, [C.c_char_p]),
    "rt_integrator_supported": (C.c_int, [C.c_int]),
    "rt_scene_set_recursive_integrators": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_scene_integrator_supported": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_scene_set_ambient_light": (C.c_int, [C.c_void_p, P(V3)]),
    "rt_scene_upload": (C.c_int, [P(SceneDesc), C.c_int, P(C.c_void_p)]),
    "rt_scene_free": (C.c_int, [C.c_void_p]),
    "rt_render": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                            P(AccumulationBuffer), P(Stats)]),
    "rt_render_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                   C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, P(Stats)]),
    "rt_trace_samples": (C.c_int, [C.c_void_p, P(Camera), P(Settings), C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint32), P(C.c_uint32),
                                   P(C.c_float), P(Stats)]),
    "rt_debug_intersect": (C.c_int, [C.c_void_p, C.c_uint32, P(RayQuery), C.c_int, P(HitRecord)]),
    "rt_debug_mesh_bvh4": (C.c_int, [P(BvhNode), C.c_uint32, P(C.c_float), C.c_uint32, P(C.c_uint32),
                                     P(C.c_uint32)]),
    "rt_debug_top_sequences": (C.c_int, [P(BvhNode), C.c_uint32, C.c_uint32, P(C.c_float), C.c_uint32,
                                         P(C.c_uint32)]),
    "rt_debug_claim_slots": (C.c_int, [P(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint32)]),
    "rt_debug_rank_slots": (C.c_int, [P(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint32)]),
    "rt_scene_ramp_stats": (C.c_int, [C.c_void_p, P(C.c_uint64), P(C.c_uint64)]),
    "rt_debug_verify_rcp": (C.c_int, [C.c_int, P(C.c_uint64), P(C.c_uint32)]),
    "rt_debug_verify_div_pi": (C.c_int, [C.c_int, P(C.c_uint64), P(C.c_uint32)]),
    "rt_debug_verify_div3": (C.c_int, [C.c_int, C.c_uint32, P(C.c_float), P(C.c_uint64), P(C.c_uint32)]),
    "rt_set_profiling": (C.c_int, [C.c_int]),
    "rt_set_profiling_stages": (C.c_int, [C.c_uint32]),
    "rt_set_path_pool": (C.c_int, [C.c_uint32]),
    "rt_set_splat_mode": (C.c_int, [C.c_int]),
    "rt_set_shard_mode": (C.c_int, [C.c_int]),
    "rt_set_env_sampling": (C.c_int, [C.c_int]),
    "rt_build_bvh": (C.c_int, [C.c_int, C.c_uint32, P(V3), P(V3), C.c_int, P(BvhNode), P(C.c_uint32), P(C.c_uint32)]),
    "rt_build_bvh_last_error": (C.c_char_p, []),
    "rt_render_picture": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                    C.c_uint32, C.c_uint32, P(PostSettings), P(C.c_uint32), P(Stats)]),
    "rt_cancel": (C.c_int, [C.c_void_p]),
    "rt_scene_default_config": (C.c_int, [P(SceneConfig)]),
    "rt_scene_get_config": (C.c_int, [C.c_void_p, P(SceneConfig)]),
    "rt_scene_set_config": (C.c_int, [C.c_void_p, P(SceneConfig)]),
    "rt_scene_stack_depth": (C.c_int, [C.c_void_p, P(C.c_uint32), P(C.c_uint32)]),
    "rt_postprocess_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, P(PostSettings), C.c_uint32,
                                        C.c_void_p, C.c_void_p]),
    "rt_postprocess": (C.c_int, [C.c_int, P(AccumulationBuffer), P(PostSettings), C.c_uint32, P(C.c_uint32)]),
    "rt_denoise_default_params": (C.c_int, [P(DenoiseParams)]),
    "rt_denoise_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_denoise_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                    P(DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise": (C.c_int, [C.c_int, P(AccumulationBuffer), P(C.c_float), P(C.c_float), P(DenoiseParams),
                             P(C.c_float)]),
    "rt_render_picture_denoised": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet),
                                             C.c_uint32, C.c_uint32, C.c_uint32, P(PostSettings), P(DenoiseParams),
                                             C.c_uint32, P(C.c_uint32), P(Stats)]),
    "rt_render_feature_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                           C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                           P(Stats)]),
    "rt_render_feature": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                    C.c_int, P(AccumulationBuffer), P(Stats)]),
    "rt_render_features_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, P(Stats)]),
    "rt_render_features": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                     P(AccumulationBuffer), P(AccumulationBuffer), P(AccumulationBuffer), P(Stats)]),
    "rt_denoise_features_default_params": (C.c_int, [P(DenoiseFeaturesParams)]),
    "rt_denoise_features_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_denoise_features_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.c_uint32, P(DenoiseFeaturesParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise_features": (C.c_int, [C.c_int, P(AccumulationBuffer), P(C.c_float), P(C.c_float), P(C.c_float),
                                      P(DenoiseFeaturesParams), P(C.c_float)]),
    "rt_render_picture_features_denoised": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet),
                                                      C.c_uint32, C.c_uint32, C.c_uint32, P(PostSettings),
                                                      P(DenoiseFeaturesParams), C.c_uint32, P(C.c_uint32), P(Stats)]),
    "rt_render_tiles_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), C.c_uint32, C.c_uint32,
                                         P(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p, P(Stats)]),
    "rt_render_tiles": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), C.c_uint32, C.c_uint32,
                                  P(C.c_uint32), C.c_uint32, C.c_uint32, P(AccumulationBuffer), P(Stats)]),
    "rt_tile_error_default_params": (C.c_int, [P(TileErrorParams)]),
    "rt_tile_error_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_uint32, P(TileErrorParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_tile_error": (C.c_int, [C.c_int, P(C.c_float), P(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                P(C.c_uint32), C.c_uint32, P(TileErrorParams), P(C.c_float), P(C.c_uint32)]),
    "rt_adaptive_default_params": (C.c_int, [P(AdaptiveParams)]),
    "rt_adaptive_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "rt_render_adaptive_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(AdaptiveParams),
                                            C.c_void_p, C.c_void_p, P(C.c_uint32), C.c_void_p, P(Stats)]),
    "rt_render_adaptive": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), C.c_uint32, C.c_uint32,
                                     C.c_uint32, P(AdaptiveParams), P(AccumulationBuffer), P(C.c_uint32), P(Stats)]),
    "rt_robust_default_params": (C.c_int, [P(RobustParams)]),
    "rt_robust_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "rt_robust_combine_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, P(RobustParams),
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_robust_combine": (C.c_int, [C.c_int, P(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32, P(RobustParams),
                                    P(C.c_float), P(C.c_float)]),
    "rt_render_robust_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                          C.c_uint32, C.c_uint32, C.c_uint32, P(RobustParams), C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, P(Stats)]),
    "rt_render_robust": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                   C.c_uint32, C.c_uint32, C.c_uint32, P(RobustParams), P(C.c_float), P(C.c_float),
                                   P(Stats)]),
    "rt_render_picture_robust": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                           C.c_uint32, C.c_uint32, P(PostSettings), P(RobustParams),
                                           P(DenoiseFeaturesParams), C.c_uint32, P(C.c_uint32), P(Stats)]),
    "rt_gbuffer_device": (C.c_int, [C.c_void_p, P(Camera), C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_gbuffer": (C.c_int, [C.c_void_p, P(Camera), C.c_float, C.c_uint32, C.c_uint32, P(GBufferTexel)]),
    "rt_temporal_default_params": (C.c_int, [P(TemporalParams)]),
    "rt_temporal_accumulate_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                P(Camera), C.c_float, C.c_uint32, C.c_uint32, P(TemporalParams),
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_temporal_accumulate": (C.c_int, [C.c_int, P(C.c_float), P(GBufferTexel), P(C.c_float), P(C.c_float),
                                         P(GBufferTexel), P(Camera), C.c_float, C.c_uint32, C.c_uint32,
                                         P(TemporalParams), P(C.c_float), P(C.c_float)]),
    "rt_temporal_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_render_temporal_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams), P(TemporalState),
                                            C.c_void_p, C.c_void_p, C.c_void_p, P(Stats)]),
    "rt_render_temporal": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams), P(TemporalState),
                                     P(C.c_float), P(C.c_float), P(Stats)]),
    "rt_temporal_accumulate_moments_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, P(Camera), C.c_float, C.c_uint32, C.c_uint32,
                                                        P(TemporalParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_temporal_accumulate_moments": (C.c_int, [C.c_int, P(C.c_float), P(GBufferTexel), P(C.c_float), P(C.c_float),
                                                 P(GBufferTexel), P(C.c_float), P(Camera), C.c_float, C.c_uint32, C.c_uint32,
                                                 P(TemporalParams), P(C.c_float), P(C.c_float), P(C.c_float)]),
    "rt_temporal_variance_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                              P(TemporalParams), C.c_float, C.c_void_p, C.c_void_p]),
    "rt_temporal_variance": (C.c_int, [C.c_int, P(C.c_float), P(C.c_float), P(GBufferTexel), C.c_uint32, C.c_uint32,
                                       P(TemporalParams), C.c_float, P(C.c_float)]),
    "rt_denoise_variance_default_params": (C.c_int, [P(DenoiseVarianceParams)]),
    "rt_denoise_variance_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_denoise_variance_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                             P(DenoiseVarianceParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise_variance": (C.c_int, [C.c_int, P(C.c_float), P(C.c_float), P(GBufferTexel), C.c_uint32, C.c_uint32,
                                      P(DenoiseVarianceParams), P(C.c_float), P(C.c_float)]),
    "rt_temporal_filtered_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_render_temporal_filtered_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet),
                                                     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams),
                                                     C.c_float, P(DenoiseVarianceParams), P(TemporalFilteredState),
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(Stats)]),
    "rt_render_temporal_filtered": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                              C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams), C.c_float,
                                              P(DenoiseVarianceParams), P(TemporalFilteredState), P(C.c_float),
                                              P(C.c_float), P(C.c_float), P(C.c_float), P(Stats)]),
    "rt_scene_update_instances": (C.c_int, [C.c_void_p, P(SceneDesc)]),
    "rt_scene_primitive_transforms": (C.c_int, [C.c_void_p, C.c_uint32, P(M4x4Inv), P(C.c_uint32)]),
    "rt_scene_update_mesh_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, P(BvhNode)]),
    "rt_scene_update_mesh": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_float), P(C.c_float), P(BvhNode)]),
    "rt_debug_scene_mesh_table": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, P(C.c_size_t)]),
    "rt_motion_table": (C.c_int, [C.c_uint32, P(M4x4Inv), P(M4x4Inv), P(MotionEntry)]),
    "rt_temporal_accumulate_motion_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       P(Camera), C.c_float, C.c_uint32, C.c_uint32, P(TemporalParams),
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_temporal_accumulate_motion": (C.c_int, [C.c_int, P(C.c_float), P(GBufferTexel), P(C.c_float), P(C.c_float),
                                                P(GBufferTexel), P(Camera), C.c_float, C.c_uint32, C.c_uint32,
                                                P(TemporalParams), P(C.c_float), P(C.c_float), P(MotionEntry), C.c_uint32,
                                                P(C.c_float), P(C.c_float), P(C.c_float)]),
    "rt_temporal_motion_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "rt_render_temporal_motion_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet),
                                                   C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams),
                                                   P(TemporalMotionState), C.c_void_p, C.c_void_p, C.c_void_p, P(Stats)]),
    "rt_render_temporal_motion": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams), P(TemporalMotionState),
                                            P(C.c_float), P(C.c_float), P(Stats)]),
    "rt_gbuffer_surface_device": (C.c_int, [C.c_void_p, P(Camera), C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "rt_gbuffer_surface": (C.c_int, [C.c_void_p, P(Camera), C.c_float, C.c_uint32, C.c_uint32, P(GBufferTexel),
                                     P(SurfaceTexel)]),
    "rt_scene_deform_table": (C.c_int, [C.c_void_p, C.c_uint32, P(DeformMesh), C.c_uint32, P(M4x4Inv), P(DeformEntry)]),
    "rt_temporal_accumulate_deform_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       P(Camera), C.c_float, C.c_uint32, C.c_uint32, P(TemporalParams),
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_uint32]),
    "rt_temporal_accumulate_deform": (C.c_int, [C.c_int, P(C.c_float), P(GBufferTexel), P(C.c_float), P(C.c_float),
                                                P(GBufferTexel), P(Camera), C.c_float, C.c_uint32, C.c_uint32,
                                                P(TemporalParams), P(C.c_float), P(C.c_float), P(MotionEntry), C.c_uint32,
                                                P(C.c_float), P(C.c_float), P(C.c_float), P(SurfaceTexel), P(DeformEntry),
                                                C.c_uint32]),
    "rt_temporal_deform_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "rt_render_temporal_deform_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet),
                                                   C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams),
                                                   P(TemporalMotionState), C.c_uint32, P(DeformMesh), C.c_void_p,
                                                   C.c_void_p, C.c_void_p, P(Stats)]),
    "rt_render_temporal_deform": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams), P(TemporalMotionState),
                                            C.c_uint32, P(DeformMesh), P(C.c_float), P(C.c_float), P(Stats)]),
    "rt_temporal_neighbourhood_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                                   C.c_void_p, C.c_void_p]),
    "rt_temporal_neighbourhood": (C.c_int, [C.c_int, P(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                            P(NeighbourhoodTexel)]),
    "rt_temporal_clip_default_params": (C.c_int, [P(TemporalClipParams)]),
    "rt_temporal_accumulate_clip_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     P(Camera), C.c_float, C.c_uint32, C.c_uint32, P(TemporalParams),
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_uint32, C.c_void_p, C.c_float, C.c_float, C.c_void_p]),
    "rt_temporal_accumulate_clip": (C.c_int, [C.c_int, P(C.c_float), P(GBufferTexel), P(C.c_float), P(C.c_float),
                                              P(GBufferTexel), P(Camera), C.c_float, C.c_uint32, C.c_uint32,
                                              P(TemporalParams), P(C.c_float), P(C.c_float), P(MotionEntry), C.c_uint32,
                                              P(C.c_float), P(C.c_float), P(C.c_float), P(SurfaceTexel), P(DeformEntry),
                                              C.c_uint32, P(NeighbourhoodTexel), C.c_float, C.c_float, P(C.c_float)]),
    "rt_temporal_clipped_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "rt_render_temporal_clipped_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet),
                                                    C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams),
                                                    P(TemporalMotionState), C.c_uint32, P(DeformMesh),
                                                    P(TemporalClipParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    P(Stats)]),
    "rt_render_temporal_clipped": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams), P(TemporalMotionState),
                                             C.c_uint32, P(DeformMesh), P(TemporalClipParams), P(C.c_float), P(C.c_float),
                                             P(C.c_float), P(Stats)]),
    "rt_gbuffer_specular_default_params": (C.c_int, [P(GBufferSpecularParams)]),
    "rt_gbuffer_specular_device": (C.c_int, [C.c_void_p, P(Camera), C.c_float, C.c_uint32, C.c_uint32,
                                             P(GBufferSpecularParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_gbuffer_specular": (C.c_int, [C.c_void_p, P(Camera), C.c_float, C.c_uint32, C.c_uint32, P(GBufferSpecularParams),
                                      P(GBufferTexel), P(SpecularTexel2)]),
    "rt_temporal_specular_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_render_temporal_specular_device": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet),
                                                     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams),
                                                     P(TemporalState), P(GBufferSpecularParams), P(TemporalClipParams),
                                                     C.c_void_p, C.c_void_p, C.c_void_p, P(Stats)]),
    "rt_render_temporal_specular": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(TileSet), C.c_uint32,
                                              C.c_uint32, C.c_uint32, C.c_uint32, P(TemporalParams), P(TemporalState),
                                              P(GBufferSpecularParams), P(TemporalClipParams), P(C.c_float), P(C.c_float),
                                              P(Stats)]),
}

HOST_FUNCTIONS = {
    "rth_last_error": (C.c_char_p, []),
    "rth_scene_create": (C.c_void_p, []),
    "rth_scene_destroy": (None, [C.c_void_p]),
    "rth_add_material": (C.c_uint32, [C.c_void_p, P(Material)]),
    "rth_add_diffuse_material": (C.c_uint32, [C.c_void_p, V3, C.c_float, C.c_float, C.c_int32, V3]),
    "rth_add_translucent_material": (C.c_uint32, [C.c_void_p, V3, C.c_float, C.c_float]),
    "rth_add_emissive_material": (C.c_uint32, [C.c_void_p, V3]),
    "rth_add_plane": (C.c_uint32, [C.c_void_p, C.c_uint32, V3, C.c_float]),
    "rth_add_sphere": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_float, P(M4x4Inv)]),
    "rth_add_box": (C.c_uint32, [C.c_void_p, C.c_uint32, V3, P(M4x4Inv)]),
    "rth_add_mesh": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_uint32, P(M4x4Inv)]),
    "rth_create_mesh": (C.c_uint32, [C.c_void_p, C.c_uint32, P(V3), P(V3), C.c_int32]),
    "rth_load_obj_mesh": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, P(C.c_uint32)]),
    "rth_mesh_bvh_info": (C.c_int, [C.c_void_p, C.c_uint32, P(BvhInfo)]),
    "rth_scene_bvh_info": (C.c_int, [C.c_void_p, P(BvhInfo)]),
    "rth_set_sky": (None, [C.c_void_p, V3, V3]),
    "rth_scene_set_ambient_light": (None, [C.c_void_p, V3]),
    "rth_scene_ambient_light": (V3, [C.c_void_p]),
    "rth_load_environment_map": (C.c_int, [C.c_void_p, C.c_char_p]),
    "rth_set_environment_map": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(V3)]),
    "rth_create_scene_bvh": (C.c_int, [C.c_void_p]),
    "rth_set_primitive_transform": (C.c_int, [C.c_void_p, C.c_uint32, P(M4x4Inv)]),
    "rth_update_mesh": (C.c_int, [C.c_void_p, C.c_uint32, P(V3), P(V3)]),
    "rth_set_bvh_device": (None, [C.c_int]),
    "rth_build_bvh_entries": (C.c_int, [C.c_uint32, P(V3), P(V3), C.c_int32, P(BvhNode), P(C.c_uint32), P(C.c_uint32)]),
    "rth_scene_desc": (P(SceneDesc), [C.c_void_p]),
    "rth_transform_identity": (M4x4Inv, []),
    "rth_transform_translate": (M4x4Inv, [V3]),
    "rth_transform_scale": (M4x4Inv, [V3]),
    "rth_transform_rotate_x_axis": (M4x4Inv, [C.c_float]),
    "rth_transform_rotate_y_axis": (M4x4Inv, [C.c_float]),
    "rth_transform_rotate_z_axis": (M4x4Inv, [C.c_float]),
    "rth_transform_mul": (M4x4Inv, [M4x4Inv, M4x4Inv]),
    "rth_aim_camera": (None, [P(Camera), V3]),
    "rth_aim_camera_at": (None, [P(Camera), V3]),
    "rth_recompute_camera": (None, [P(Camera)]),
    "rth_default_settings": (None, [P(Settings), P(PostSettings)]),
    "rth_load_reconstruction_kernel": (None, [C.c_char_p, P(FilterCache)]),
    "rth_load_preset": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, P(C.c_void_p), P(Camera),
                                  P(Settings), P(FilterCache), P(PostSettings)]),
    "rth_generate_mesh": (C.c_uint32, [C.c_uint32, C.c_uint32, P(V3), P(V3)]),
    "rth_write_synthetic_obj": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32]),
    "rth_write_synthetic_hdr": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "rth_resolve_bgra8": (None, [P(AccumulationBuffer), P(PostSettings), P(C.c_uint32)]),
    "rth_write_bitmap": (C.c_int, [C.c_char_p, P(C.c_uint32), C.c_uint32, C.c_uint32]),
    "rth_take_picture": (C.c_int, [C.c_void_p, P(Camera), P(Settings), P(FilterCache), P(PostSettings),
                                   C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_char_p, P(Stats)]),
    "rth_read_bitmap": (C.c_int, [C.c_char_p, P(C.c_uint32), C.c_uint32, C.c_uint32]),
}


def bind(lib, table):
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_LIB = None


def load_library(path=None):
    """Load librt_mi355x.so.  There is no fallback: a missing library is an error.

    RT_MI355X_LIB names another build of the same library (tuning variants)."""
    global _LIB
    if path is None:
        path = os.environ.get("RT_MI355X_LIB") or LIB_PATH
    if _LIB is None:
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run __graft_entry__.build() (make -C buas-pathtracer_amd/csrc)")
        lib = C.CDLL(path)
        bind(lib, ABI_FUNCTIONS)
        bind(lib, HOST_FUNCTIONS)
        _LIB = lib
    return _LIB
