"""MI355X wavefront path tracer — Python host mirror of the reference's interface.

The hot path (render_tile -> advanced_integrator -> intersect_scene /
intersect_shadow_ray -> samplers -> splat_filter, RT/raytracer.cpp:366-495)
runs as gfx950 HIP kernels in lib/librt_mi355x.so behind the C ABI of
include/rt_abi.h.  This module is a thin ctypes host over that ABI and over
the scene model of include/rt_host.h, keeping the reference's names:

    scene = Scene()                         # clear_scene + init_scene
    m = scene.add_diffuse_material(...)     # RT/scene.cpp:23-37
    scene.add_sphere(m, 2.0, translate(...))
    scene.create_scene_bvh()                # RT/scene.cpp:173-242
    dev = DeviceScene(scene, device=0)      # rt_scene_upload
    acc = dev.render(camera, settings, filter_cache, w, h)   # render_all_tiles

There is no CPU fallback: without a visible MI355X, DeviceScene raises.
"""
import ctypes as C
import math

import numpy as np

from . import abi
from .abi import (V3, v3, M4x4Inv, Material, Camera, Settings, FilterCache, PostSettings, TileSet, Stats,
                  AccumulationBuffer, RayQuery, HitRecord, BvhInfo, DenoiseParams, DenoiseFeaturesParams,
                  TileErrorParams, AdaptiveParams, RobustParams, GBufferTexel, TemporalParams, TemporalState,
                  DenoiseVarianceParams, TemporalFilteredState, MotionEntry, TemporalMotionState, SurfaceTexel,
                  DeformMesh, DeformEntry, NeighbourhoodTexel, TemporalClipParams, SpecularTexel2,
                  GBufferSpecularParams)

__all__ = ["Scene", "DeviceScene", "RenderError", "load_preset", "default_settings", "load_reconstruction_kernel",
           "translate", "scale", "rotate_x", "rotate_y", "rotate_z", "identity", "aim_camera", "aim_camera_at",
           "recompute_camera", "resolve_bgra8", "postprocess", "write_bitmap", "lib", "abi", "v3", "PI_32", "DEG_TO_RAD",
           "set_splat_mode", "splat_mode", "take_picture", "read_bitmap", "integrator_name", "find_integrator",
           "integrator_supported", "scene_integrator_supported", "DenoiseParams", "default_denoise_params", "denoise",
           "denoise_workspace_bytes", "DenoiseFeaturesParams", "default_denoise_features_params", "denoise_features",
           "denoise_features_workspace_bytes", "TileErrorParams", "AdaptiveParams", "default_tile_error_params",
           "default_adaptive_params", "adaptive_workspace_bytes", "tile_error", "RobustParams", "default_robust_params",
           "robust_workspace_bytes", "robust_combine", "GBufferTexel", "TemporalParams", "TemporalState",
           "default_temporal_params", "temporal_workspace_bytes", "temporal_accumulate", "temporal_accumulate_device",
           "DenoiseVarianceParams", "TemporalFilteredState", "default_denoise_variance_params",
           "denoise_variance_workspace_bytes", "temporal_filtered_workspace_bytes", "temporal_accumulate_moments",
           "temporal_accumulate_moments_device", "temporal_variance", "temporal_variance_device", "denoise_variance",
           "denoise_variance_device", "MotionEntry", "TemporalMotionState", "motion_table", "temporal_accumulate_motion",
           "temporal_accumulate_motion_device", "temporal_motion_workspace_bytes", "SurfaceTexel", "DeformMesh",
           "DeformEntry", "deform_meshes", "temporal_deform_workspace_bytes", "temporal_accumulate_deform",
           "temporal_accumulate_deform_device", "NeighbourhoodTexel", "TemporalClipParams", "default_temporal_clip_params",
           "temporal_neighbourhood", "temporal_neighbourhood_device", "temporal_accumulate_clip",
           "temporal_accumulate_clip_device", "temporal_clipped_workspace_bytes", "SpecularTexel2",
           "GBufferSpecularParams", "default_gbuffer_specular_params", "temporal_specular_workspace_bytes"]

PI_32 = 3.14159265359
DEG_TO_RAD = 6.28318530717 / 360.0


class RenderError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"rt error {code}: {message}")
        self.code = code


def lib():
    return abi.load_library()


def _check(code):
    if code != abi.RT_OK:
        raise RenderError(code, (lib().rt_last_error() or b"").decode())


def _v(x):
    if isinstance(x, V3):
        return x
    x = tuple(x) if not isinstance(x, (int, float)) else (x, x, x)
    return V3(*[float(c) for c in x])


# ---- transforms (MathLib/my_math.h:1009-1069)
def identity():
    return lib().rth_transform_identity()


def translate(t):
    return lib().rth_transform_translate(_v(t))


def scale(s):
    return lib().rth_transform_scale(_v(s))


def rotate_x(a):
    return lib().rth_transform_rotate_x_axis(float(a))


def rotate_y(a):
    return lib().rth_transform_rotate_y_axis(float(a))


def rotate_z(a):
    return lib().rth_transform_rotate_z_axis(float(a))


def mul(a, b):
    return lib().rth_transform_mul(a, b)


M4x4Inv.__mul__ = lambda a, b: lib().rth_transform_mul(a, b)


# ---- camera (RT/raytracer.cpp:26-59)
def aim_camera(cam, d):
    lib().rth_aim_camera(C.byref(cam), _v(d))


def aim_camera_at(cam, at):
    lib().rth_aim_camera_at(C.byref(cam), _v(at))


def recompute_camera(cam):
    lib().rth_recompute_camera(C.byref(cam))


def default_settings():
    """init_scene defaults (RT/raytracer.cpp:1430-1452) -> (Settings, PostSettings)."""
    st, post = Settings(), PostSettings()
    lib().rth_default_settings(C.byref(st), C.byref(post))
    return st, post


def load_reconstruction_kernel(name="Mitchell Netravali"):
    """load_reconstruction_kernel(find_filter(name)) (RT/raytracer.cpp:164-185)."""
    fc = FilterCache()
    lib().rth_load_reconstruction_kernel(name.encode(), C.byref(fc))
    return fc


class Scene:
    """Host scene (RT/scene.h:92-120): materials, primitives, planes, lights, BVHs."""

    def __init__(self, handle=None):
        self._h = handle if handle is not None else lib().rth_scene_create()
        if not self._h:
            raise MemoryError("rth_scene_create failed")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().rth_scene_destroy(h)
            except Exception:
                pass

    @property
    def handle(self):
        return self._h

    # materials (RT/scene.cpp:9-61)
    def add_material(self, flags=0, albedo=0.0, checker_color=0.0, emission_color=0.0, ior=0.0, metallic=0.0,
                     roughness=0.0, is_participating_medium=False, absorb=0.0):
        m = Material(flags, _v(albedo), _v(checker_color), _v(emission_color), ior, metallic, roughness,
                     int(bool(is_participating_medium)), _v(absorb))
        return lib().rth_add_material(self._h, C.byref(m))

    def add_diffuse_material(self, diffuse_color, ior, roughness=0.0, checkers=False, checker_color=0.1):
        return lib().rth_add_diffuse_material(self._h, _v(diffuse_color), float(ior), float(roughness),
                                              int(bool(checkers)), _v(checker_color))

    def add_translucent_material(self, absorb, ior, roughness=0.0):
        return lib().rth_add_translucent_material(self._h, _v(absorb), float(ior), float(roughness))

    def add_emissive_material(self, emission_color):
        return lib().rth_add_emissive_material(self._h, _v(emission_color))

    # primitives (RT/scene.cpp:70-159)
    def add_plane(self, material_id, n, d):
        return lib().rth_add_plane(self._h, material_id, _v(n), float(d))

    def add_sphere(self, material_id, r, transform=None):
        return lib().rth_add_sphere(self._h, material_id, float(r), C.byref(transform) if transform else None)

    def add_box(self, material_id, r, transform=None):
        return lib().rth_add_box(self._h, material_id, _v(r), C.byref(transform) if transform else None)

    def add_mesh(self, material_id, mesh_id, transform=None):
        return lib().rth_add_mesh(self._h, material_id, mesh_id, C.byref(transform) if transform else None)

    def create_mesh(self, triangles, normals=None, method=abi.RTH_BVH_SAH_BINNED):
        """triangles: float32 array [n,3,3]; normals: optional [n,3,3] (per-vertex)."""
        t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 3)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3, 3)
        mid = lib().rth_create_mesh(self._h, t.shape[0], t.ctypes.data_as(C.POINTER(V3)),
                                    None if n is None else n.ctypes.data_as(C.POINTER(V3)), method)
        if mid == 0xFFFFFFFF:
            raise RuntimeError(f"rth_create_mesh failed: {(lib().rth_last_error() or b'').decode()}")
        return mid

    def load_obj_mesh(self, path, method=abi.RTH_BVH_SAH_BINNED):
        out = C.c_uint32()
        if not lib().rth_load_obj_mesh(self._h, str(path).encode(), method, C.byref(out)):
            raise ValueError(lib().rth_last_error().decode())
        return out.value

    def set_sky(self, top, bot):
        lib().rth_set_sky(self._h, _v(top), _v(bot))

    def set_ambient_light(self, ambient_light):
        """Scene::ambient_light (RT/scene.h:102): added to the Whitted integrator's illumination only.
        DeviceScene passes it on at upload."""
        lib().rth_scene_set_ambient_light(self._h, _v(ambient_light))

    def ambient_light(self):
        a = lib().rth_scene_ambient_light(self._h)
        return (a.x, a.y, a.z)

    def load_environment_map(self, path):
        if not lib().rth_load_environment_map(self._h, str(path).encode()):
            raise ValueError(lib().rth_last_error().decode())

    def set_environment_map(self, pixels):
        """An environment map from an (h, w, 3) float32 array (row 0 = v = 0, the bottom)."""
        a = np.ascontiguousarray(pixels, dtype=np.float32)
        h, w = a.shape[:2]
        if not lib().rth_set_environment_map(self._h, w, h, a.ctypes.data_as(C.POINTER(abi.V3))):
            raise ValueError(lib().rth_last_error().decode())

    def create_scene_bvh(self):
        if not lib().rth_create_scene_bvh(self._h):
            raise RuntimeError(f"rth_create_scene_bvh failed: {(lib().rth_last_error() or b'').decode()}")

    def set_primitive_transform(self, primitive_id, transform):
        """rth_set_primitive_transform: move a sphere, box or mesh instance.  Call create_scene_bvh() again before
        desc() is uploaded or passed to DeviceScene.update_instances."""
        if not lib().rth_set_primitive_transform(self._h, primitive_id, C.byref(transform)):
            raise ValueError((lib().rth_last_error() or b"").decode())

    def update_mesh(self, mesh_id, triangles, normals=None):
        """rth_update_mesh: new vertices for a mesh, [n,3,3] in create_mesh's order (normals likewise, or None to keep
        the stored ones); its BVH is refitted, the topology stays.  Call create_scene_bvh() again before desc() is
        uploaded or passed to DeviceScene.update_instances."""
        t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 3)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3, 3)
        d = self.desc()
        if mesh_id < d.mesh_count and (t.shape[0] != d.meshes[mesh_id].triangle_count or
                                       (n is not None and n.shape[0] != t.shape[0])):
            raise ValueError("update_mesh: the mesh's triangle count cannot change")
        if not lib().rth_update_mesh(self._h, mesh_id, t.ctypes.data_as(C.POINTER(V3)),
                                     None if n is None else n.ctypes.data_as(C.POINTER(V3))):
            raise ValueError((lib().rth_last_error() or b"").decode())

    def bvh_info(self, mesh_id=None):
        info = BvhInfo()
        if mesh_id is None:
            lib().rth_scene_bvh_info(self._h, C.byref(info))
        else:
            lib().rth_mesh_bvh_info(self._h, mesh_id, C.byref(info))
        return {k: getattr(info, k) for k, _ in BvhInfo._fields_}

    def desc(self):
        """The flattened scene (rt_scene_desc).  Its arrays point into this host scene, so the
        returned struct keeps the Scene alive (`Scene(...).desc()` on a temporary is safe)."""
        d = lib().rth_scene_desc(self._h).contents
        d._scene = self
        return d


def load_preset(name, w, h, asset_dir=None):
    """load_scene(g_scenes[...]) or a BASELINE config ('c1'..'c5').
    Returns (Scene, Camera, Settings, FilterCache, PostSettings)."""
    handle = C.c_void_p()
    cam, st, fc, post = Camera(), Settings(), FilterCache(), PostSettings()
    ok = lib().rth_load_preset(name.encode(), w, h, asset_dir.encode() if asset_dir else None, C.byref(handle),
                               C.byref(cam), C.byref(st), C.byref(fc), C.byref(post))
    if not ok:
        why = lib().rth_last_error()
        why = why.decode() if isinstance(why, bytes) else why
        raise ValueError(f"preset {name!r}: " + (why or "unknown preset"))
    return Scene(handle.value), cam, st, fc, post


class DeviceScene:
    """A scene resident on one MI355X (rt_scene_upload)."""

    def __init__(self, scene, device=0):
        self.scene = scene          # keep the host arrays alive
        self.device = device
        h = C.c_void_p()
        _check(lib().rt_scene_upload(C.byref(scene.desc()), device, C.byref(h)))
        self._h = h
        ambient = getattr(scene, "ambient_light", None)     # not part of rt_scene_desc; any object with desc() uploads
        if ambient is not None:
            self.set_ambient_light(ambient())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().rt_scene_free(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def update_instances(self, desc=None):
        """rt_scene_update_instances: replace the transform-dependent tables (transforms, transform indices, the
        top-level BVH) with those of `desc` (default: the host scene's desc() as it is now).  No mesh, material or
        sky array of `desc` is read.  Synchronises the device."""
        if desc is None:
            desc = self.scene.desc()
        _check(lib().rt_scene_update_instances(self._h, C.byref(desc)))

    def _mesh_triangles(self, mesh_index):
        """The mesh's triangle count, or None for an index the scene refuses (the update entry then says so)."""
        size = C.c_size_t()
        if lib().rt_debug_scene_mesh_table(self._h, mesh_index, abi.RT_MESH_TABLE_TRIANGLES, None, 0, C.byref(size)):
            return None
        return size.value // 48

    def update_mesh(self, mesh_index, triangles, normals=None):
        """rt_scene_update_mesh: new vertices for one mesh of the uploaded scene, float32 [n,3,3] in the mesh's
        original triangle order (normals likewise, or None to keep the stored ones); the mesh's BVH is refitted on the
        device.  Returns node 0 (abi.BvhNode).  When its box changed, the scene refuses to trace until
        update_instances() with a top-level BVH over the new bounds: Scene.update_mesh, Scene.create_scene_bvh, then
        DeviceScene.update_instances."""
        t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 3)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3, 3)
        count = self._mesh_triangles(mesh_index)
        if count is not None and (t.shape[0] != count or (n is not None and n.shape[0] != count)):
            raise ValueError(f"update_mesh: mesh {mesh_index} has {count} triangles")
        fp = C.POINTER(C.c_float)
        root = abi.BvhNode()
        _check(lib().rt_scene_update_mesh(self._h, mesh_index, t.ctypes.data_as(fp),
                                          None if n is None else n.ctypes.data_as(fp), C.byref(root)))
        return root

    def update_mesh_device(self, mesh_index, d_triangles, d_normals=None):
        """rt_scene_update_mesh_device: the same from device memory, as pointers (9 float32 per triangle, original
        order) or as contiguous float32 torch tensors on the scene's device."""
        count = self._mesh_triangles(mesh_index)

        def ptr(x):
            if x is None or isinstance(x, int):
                return x
            if str(x.dtype) != "torch.float32" or not x.is_contiguous() or (count is not None and x.numel() != 9*count):
                raise ValueError(f"update_mesh_device: a contiguous float32 tensor of {count} x 3 x 3 is needed")
            if not x.is_cuda or x.device.index != self.device:
                raise ValueError("update_mesh_device: the tensor is not on the scene's device")
            return x.data_ptr()
        root = abi.BvhNode()
        pt, pn = ptr(d_triangles), ptr(d_normals)
        _check(lib().rt_scene_update_mesh_device(self._h, mesh_index, C.c_void_p(pt) if pt else None,
                                                 C.c_void_p(pn) if pn else None, C.byref(root)))
        return root

    def mesh_table(self, mesh_index, which):
        """rt_debug_scene_mesh_table: one mesh's slice of a scene table (abi.RT_MESH_TABLE_*) as a uint8 array."""
        size = C.c_size_t()
        _check(lib().rt_debug_scene_mesh_table(self._h, mesh_index, which, None, 0, C.byref(size)))
        out = np.zeros(size.value, np.uint8)
        _check(lib().rt_debug_scene_mesh_table(self._h, mesh_index, which, out.ctypes.data_as(C.c_void_p), out.size,
                                               C.byref(size)))
        return out

    def primitive_transforms(self):
        """rt_scene_primitive_transforms: the resolved transform of every primitive as of the upload or the last
        update -> a structured array (primitive_count,) of abi.M4X4INV_DTYPE."""
        count = C.c_uint32()
        _check(lib().rt_scene_primitive_transforms(self._h, 0, None, C.byref(count)))
        out = np.zeros(count.value, abi.M4X4INV_DTYPE)
        _check(lib().rt_scene_primitive_transforms(self._h, count.value, out.ctypes.data_as(C.POINTER(M4x4Inv)),
                                                   C.byref(count)))
        return out

    def render(self, camera, settings, filter_cache, w, h, accum=None, frame_count=0, total_frame_index=0,
               tile=64, shard_index=0, shard_count=1):
        """rt_render: adds one frame into `accum` (float32 [h,w,4], host) and returns (accum, stats)."""
        if accum is None:
            accum = np.zeros((h, w, 4), np.float32)
        assert accum.dtype == np.float32 and accum.flags.c_contiguous and accum.shape == (h, w, 4)
        buf = AccumulationBuffer(w, h, frame_count, accum.ctypes.data_as(C.POINTER(C.c_float)))
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        _check(lib().rt_render(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache), C.byref(tiles),
                               total_frame_index, C.byref(buf), C.byref(stats)))
        return accum, stats

    def render_device(self, camera, settings, filter_cache, w, h, d_pixels, stream=None, frame_count=0,
                      total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_device into a device pointer (e.g. torch tensor .data_ptr())."""
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        _check(lib().rt_render_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                      C.byref(tiles), total_frame_index, w, h, frame_count, C.c_void_p(d_pixels),
                                      C.c_void_p(stream) if stream else None, C.byref(stats)))
        return stats

    def trace_samples(self, camera, settings, w, h, pixel_xy, sample_offset, frame_count=0, total_frame_index=0,
                      tile=64):
        xy = np.ascontiguousarray(pixel_xy, np.uint32).reshape(-1, 2)
        s = np.ascontiguousarray(sample_offset, np.uint32).reshape(-1)
        out = np.zeros((xy.shape[0], 5), np.float32)
        stats = Stats()
        _check(lib().rt_trace_samples(self._h, C.byref(camera), C.byref(settings), w, h, tile, tile, frame_count,
                                      total_frame_index, xy.shape[0], xy.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      s.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(stats)))
        return out, stats

    def intersect(self, rays, occlusion=False):
        n = len(rays)
        q = (RayQuery * n)(*rays)
        out = (HitRecord * n)()
        _check(lib().rt_debug_intersect(self._h, n, q, int(bool(occlusion)), out))
        return list(out)

    def cancel(self):
        lib().rt_cancel(self._h)

    def set_recursive_integrators(self, enable=True):
        """rt_scene_set_recursive_integrators: on, the render entries take Whitted and Ground Truth Recursive
        for this scene (a frame stack is allocated on the device); off (the default), they refuse them."""
        _check(lib().rt_scene_set_recursive_integrators(self._h, int(bool(enable))))

    def integrator_supported(self, integrator):
        """rt_scene_integrator_supported: integrator_supported plus Whitted and Ground Truth Recursive when
        this scene has opted in."""
        return bool(lib().rt_scene_integrator_supported(self._h, int(integrator)))

    def set_ambient_light(self, ambient_light):
        """rt_scene_set_ambient_light: Scene::ambient_light, read by the Whitted integrator only."""
        a = _v(ambient_light)
        _check(lib().rt_scene_set_ambient_light(self._h, C.byref(a)))

    def config(self):
        """rt_scene_get_config: this scene's schedule and splat settings (abi.SceneConfig)."""
        c = abi.SceneConfig()
        _check(lib().rt_scene_get_config(self._h, C.byref(c)))
        return c

    def ramp_stats(self):
        """rt_scene_ramp_stats: (shade iterations after the last claim and before the fused drain, paths
        they shaded) of the last frame, summed over its partitions."""
        it, paths = C.c_uint64(0), C.c_uint64(0)
        _check(lib().rt_scene_ramp_stats(self._h, C.byref(it), C.byref(paths)))
        return int(it.value), int(paths.value)

    def stack_depth(self):
        """rt_scene_stack_depth: (entries, entries with traversal_ref's markers) the upload's bound says a
        traversal of this scene can hold; rt_scene_upload requires entries + 2 <= 64."""
        d, r = C.c_uint32(0), C.c_uint32(0)
        _check(lib().rt_scene_stack_depth(self._h, C.byref(d), C.byref(r)))
        return int(d.value), int(r.value)

    def render_guides(self, camera, settings, filter_cache, w, h, spp, total_frame_index=0, tile=64):
        """The two guide frames of the denoise stage: a Normals and a Distances frame (integrators 4 and 5) of
        `spp` samples per pixel with the caller's other settings -> (normals, distances), host float32
        [h, w, 4] accumulation buffers for denoise(accum, normals, distances)."""
        st = Settings.from_buffer_copy(settings)
        st.samples_per_pixel = spp
        out = []
        for integrator in (abi.RT_INTEGRATOR_NORMALS, abi.RT_INTEGRATOR_DISTANCES):
            st.integrator = integrator
            out.append(self.render(camera, st, filter_cache, w, h, total_frame_index=total_frame_index, tile=tile)[0])
        return out[0], out[1]

    def render_feature(self, camera, settings, filter_cache, w, h, feature, accum=None, frame_count=0,
                       total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_feature: adds one feature frame (abi.RT_FEATURE_NORMAL, _DISTANCE or _ALBEDO: what the pixel
        shows at the end of its specular prefix) into `accum` (float32 [h,w,4], host) -> (accum, stats)."""
        if accum is None:
            accum = np.zeros((h, w, 4), np.float32)
        assert accum.dtype == np.float32 and accum.flags.c_contiguous and accum.shape == (h, w, 4)
        buf = AccumulationBuffer(w, h, frame_count, accum.ctypes.data_as(C.POINTER(C.c_float)))
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        _check(lib().rt_render_feature(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache), C.byref(tiles),
                                       total_frame_index, int(feature), C.byref(buf), C.byref(stats)))
        return accum, stats

    def render_feature_device(self, camera, settings, filter_cache, w, h, feature, d_pixels, stream=None,
                              frame_count=0, total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_feature_device into a device pointer (e.g. torch tensor .data_ptr())."""
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        _check(lib().rt_render_feature_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                              C.byref(tiles), total_frame_index, w, h, frame_count, int(feature),
                                              C.c_void_p(d_pixels), C.c_void_p(stream) if stream else None,
                                              C.byref(stats)))
        return stats

    def render_features(self, camera, settings, filter_cache, w, h, accums=None, frame_count=0, total_frame_index=0,
                        tile=64, shard_index=0, shard_count=1):
        """rt_render_features: the NORMAL, DISTANCE and ALBEDO frames in one walk, added into `accums` (three
        float32 [h,w,4] host buffers; fresh ones by default) -> (normal, distance, albedo, stats).  Each buffer
        is what render_feature adds to it; the stats are the one walk's."""
        if accums is None:
            accums = [np.zeros((h, w, 4), np.float32) for _ in range(abi.RT_FEATURE_COUNT)]
        accums = list(accums)
        assert len(accums) == abi.RT_FEATURE_COUNT
        for a in accums:
            assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (h, w, 4)
        bufs = [AccumulationBuffer(w, h, frame_count, a.ctypes.data_as(C.POINTER(C.c_float))) for a in accums]
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        _check(lib().rt_render_features(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache), C.byref(tiles),
                                        total_frame_index, C.byref(bufs[0]), C.byref(bufs[1]), C.byref(bufs[2]),
                                        C.byref(stats)))
        return accums[0], accums[1], accums[2], stats

    def render_features_device(self, camera, settings, filter_cache, w, h, d_normal, d_distance, d_albedo, stream=None,
                               frame_count=0, total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_features_device into three distinct device pointers (e.g. torch tensors' .data_ptr())."""
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        _check(lib().rt_render_features_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                               C.byref(tiles), total_frame_index, w, h, frame_count,
                                               C.c_void_p(d_normal), C.c_void_p(d_distance), C.c_void_p(d_albedo),
                                               C.c_void_p(stream) if stream else None, C.byref(stats)))
        return stats

    def render_picture_features_denoised(self, camera, settings, filter_cache, w, h, post, params=None, guide_spp=0,
                                         total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_picture_features_denoised: rt_render_picture with the denoise stage guided by the three
        feature frames of `guide_spp` samples per pixel (0: the beauty frame's count), demodulated by the
        albedo frame -> (BGRA8 (h, w) u32, the beauty frame's stats)."""
        if params is None:
            params = default_denoise_features_params()
        tiles = TileSet(tile, tile, shard_index, shard_count)
        out = np.zeros((h, w), np.uint32)
        stats = Stats()
        _check(lib().rt_render_picture_features_denoised(self._h, C.byref(camera), C.byref(settings),
                                                         C.byref(filter_cache), C.byref(tiles), total_frame_index, w, h,
                                                         C.byref(post), C.byref(params), guide_spp,
                                                         out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(stats)))
        return out, stats

    def render_picture_denoised(self, camera, settings, filter_cache, w, h, post, params=None, guide_spp=0,
                                total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_picture_denoised: the frame of rt_render_picture with the denoise stage between the
        accumulation buffer and the output pass, guided by a Normals and a Distances frame of `guide_spp`
        samples per pixel (0: the beauty frame's count) -> (BGRA8 (h, w) u32, the beauty frame's stats)."""
        if params is None:
            params = default_denoise_params()
        tiles = TileSet(tile, tile, shard_index, shard_count)
        out = np.zeros((h, w), np.uint32)
        stats = Stats()
        _check(lib().rt_render_picture_denoised(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                                C.byref(tiles), total_frame_index, w, h, C.byref(post),
                                                C.byref(params), guide_spp,
                                                out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(stats)))
        return out, stats

    def render_tiles(self, camera, settings, filter_cache, w, h, tile_ids, accum=None, frame_count=0,
                     total_frame_index=0, tile=64):
        """rt_render_tiles: adds the frame of the listed tiles (strictly ascending indices into the tile grid)
        into `accum` (float32 [h,w,4], host) -> (accum, stats)."""
        if accum is None:
            accum = np.zeros((h, w, 4), np.float32)
        assert accum.dtype == np.float32 and accum.flags.c_contiguous and accum.shape == (h, w, 4)
        ids = np.ascontiguousarray(tile_ids, np.uint32).reshape(-1)
        buf = AccumulationBuffer(w, h, frame_count, accum.ctypes.data_as(C.POINTER(C.c_float)))
        stats = Stats()
        _check(lib().rt_render_tiles(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache), tile, tile,
                                     ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size, total_frame_index,
                                     C.byref(buf), C.byref(stats)))
        return accum, stats

    def render_tiles_device(self, camera, settings, filter_cache, w, h, tile_ids, d_pixels, stream=None, frame_count=0,
                            total_frame_index=0, tile=64):
        """rt_render_tiles_device into a device pointer (e.g. torch tensor .data_ptr()); tile_ids is a host list."""
        ids = np.ascontiguousarray(tile_ids, np.uint32).reshape(-1)
        stats = Stats()
        _check(lib().rt_render_tiles_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache), tile, tile,
                                            ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size, total_frame_index, w, h,
                                            frame_count, C.c_void_p(d_pixels), C.c_void_p(stream) if stream else None,
                                            C.byref(stats)))
        return stats

    def render_adaptive(self, camera, settings, filter_cache, w, h, params=None, accum=None, frame_count=0,
                        total_frame_index=0, tile=64):
        """rt_render_adaptive: adaptive sampling by tiles (settings.samples_per_pixel is ignored, params.max_spp
        rules) added into `accum` (float32 [h,w,4], host) -> (accum, tile_spp, stats), tile_spp the samples each
        tile of the grid took (uint32 [tcy, tcx])."""
        if params is None:
            params = default_adaptive_params()
        if accum is None:
            accum = np.zeros((h, w, 4), np.float32)
        assert accum.dtype == np.float32 and accum.flags.c_contiguous and accum.shape == (h, w, 4)
        tile_spp = np.zeros(((h + tile - 1) // tile, (w + tile - 1) // tile), np.uint32)
        buf = AccumulationBuffer(w, h, frame_count, accum.ctypes.data_as(C.POINTER(C.c_float)))
        stats = Stats()
        _check(lib().rt_render_adaptive(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache), tile, tile,
                                        total_frame_index, C.byref(params), C.byref(buf),
                                        tile_spp.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(stats)))
        return accum, tile_spp, stats

    def render_adaptive_device(self, camera, settings, filter_cache, w, h, params, d_pixels, d_workspace=None,
                               stream=None, frame_count=0, total_frame_index=0, tile=64):
        """rt_render_adaptive_device into a device pointer; d_workspace: adaptive_workspace_bytes(w, h, tile) bytes
        on the device, or None -> (tile_spp, stats)."""
        tile_spp = np.zeros(((h + tile - 1) // tile, (w + tile - 1) // tile), np.uint32)
        stats = Stats()
        _check(lib().rt_render_adaptive_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache), tile,
                                               tile, total_frame_index, w, h, frame_count, C.byref(params),
                                               C.c_void_p(d_workspace) if d_workspace else None, C.c_void_p(d_pixels),
                                               tile_spp.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               C.c_void_p(stream) if stream else None, C.byref(stats)))
        return tile_spp, stats

    def render_robust(self, camera, settings, filter_cache, w, h, params=None, frame_count=0, total_frame_index=0,
                      tile=64, shard_index=0, shard_count=1, want_info=True):
        """rt_render_robust: the frame of settings.samples_per_pixel samples rendered as its params.buffers shards by
        sample passes, combined by the robust estimator -> (out float32 [h,w,4] = {r, g, b, 1}, info float32 [h,w,4] = {G, c, n, weight} or None, stats)."""
        if params is None:
            params = default_robust_params()
        out = np.zeros((h, w, 4), np.float32)
        info = np.zeros((h, w, 4), np.float32) if want_info else None
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        fp = C.POINTER(C.c_float)
        _check(lib().rt_render_robust(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache), C.byref(tiles),
                                      total_frame_index, w, h, frame_count, C.byref(params), out.ctypes.data_as(fp),
                                      info.ctypes.data_as(fp) if want_info else None, C.byref(stats)))
        return out, info, stats

    def render_robust_device(self, camera, settings, filter_cache, w, h, params, d_out, d_info=None, d_workspace=None,
                             stream=None, frame_count=0, total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_robust_device into device pointers (d_out is overwritten); d_workspace:
        robust_workspace_bytes(w, h, params.buffers) bytes on the device, or None -> stats."""
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        _check(lib().rt_render_robust_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                             C.byref(tiles), total_frame_index, w, h, frame_count, C.byref(params),
                                             C.c_void_p(d_workspace) if d_workspace else None, C.c_void_p(d_out),
                                             C.c_void_p(d_info) if d_info else None,
                                             C.c_void_p(stream) if stream else None, C.byref(stats)))
        return stats

    def render_picture_robust(self, camera, settings, filter_cache, w, h, post, params=None, denoise_params=None,
                              guide_spp=0, total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_picture_robust: rt_render_picture with the robust estimator in place of the mean and, with
        `denoise_params` (DenoiseFeaturesParams), the denoise stage with feature frames on its output
        -> (BGRA8 (h, w) u32, the driver's stats)."""
        if params is None:
            params = default_robust_params()
        tiles = TileSet(tile, tile, shard_index, shard_count)
        out = np.zeros((h, w), np.uint32)
        stats = Stats()
        _check(lib().rt_render_picture_robust(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                              C.byref(tiles), total_frame_index, w, h, C.byref(post), C.byref(params),
                                              C.byref(denoise_params) if denoise_params is not None else None, guide_spp,
                                              out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(stats)))
        return out, stats

    def gbuffer(self, camera, w, h, lens_distortion=0.0):
        """rt_gbuffer: the primary hit of every pixel's jitter-free pinhole ray -> a structured array (h, w) of
        abi.GBUFFER_DTYPE {p, t, n, primitive}; a miss is {the ray's direction, 0, 0, RT_HIT_MISS}."""
        out = np.zeros((h, w), abi.GBUFFER_DTYPE)
        _check(lib().rt_gbuffer(self._h, C.byref(camera), float(lens_distortion), w, h,
                                out.ctypes.data_as(C.POINTER(GBufferTexel))))
        return out

    def gbuffer_device(self, camera, w, h, d_out, lens_distortion=0.0, stream=None):
        """rt_gbuffer_device into a device pointer of w*h 32-byte texels (e.g. a torch tensor's .data_ptr())."""
        _check(lib().rt_gbuffer_device(self._h, C.byref(camera), float(lens_distortion), w, h, C.c_void_p(d_out),
                                       C.c_void_p(stream) if stream else None))

    def render_temporal(self, camera, settings, filter_cache, w, h, state, params=None, frame_count=0, total_frame_index=0,
                        tile=64, shard_index=0, shard_count=1, want_length=True):
        """rt_render_temporal: one frame of the loop.  `state` is a TemporalState whose d_workspace points at
        temporal_workspace_bytes(w, h) bytes on the device (all else zero at the start); it is updated in place
        -> (history float32 [h,w,4] = {r, g, b, 1}, length float32 [h,w] or None, the beauty frame's stats)."""
        if params is None:
            params = default_temporal_params()
        out = np.zeros((h, w, 4), np.float32)
        length = np.zeros((h, w), np.float32) if want_length else None
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        fp = C.POINTER(C.c_float)
        _check(lib().rt_render_temporal(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache), C.byref(tiles),
                                        total_frame_index, w, h, frame_count, C.byref(params), C.byref(state),
                                        out.ctypes.data_as(fp), length.ctypes.data_as(fp) if want_length else None,
                                        C.byref(stats)))
        return out, length, stats

    def render_temporal_device(self, camera, settings, filter_cache, w, h, params, state, d_out, d_length_out=None,
                               stream=None, frame_count=0, total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_temporal_device into device pointers (d_out w*h float4, d_length_out w*h floats or None; both
        overwritten); `state` as for render_temporal -> the beauty frame's stats."""
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        _check(lib().rt_render_temporal_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                               C.byref(tiles), total_frame_index, w, h, frame_count, C.byref(params),
                                               C.byref(state), C.c_void_p(d_out),
                                               C.c_void_p(d_length_out) if d_length_out else None,
                                               C.c_void_p(stream) if stream else None, C.byref(stats)))
        return stats

    def render_temporal_motion(self, camera, settings, filter_cache, w, h, state, params=None, frame_count=0,
                               total_frame_index=0, tile=64, shard_index=0, shard_count=1, want_length=True):
        """rt_render_temporal_motion: render_temporal with a history that follows update_instances.  `state` is a
        TemporalMotionState whose d_workspace points at temporal_motion_workspace_bytes(w, h, primitive count) bytes
        on the device and whose transforms / transform_cap name a host array of M4x4Inv (all else zero at the start)
        -> (history float32 [h,w,4], length float32 [h,w] or None, the beauty frame's stats)."""
        if params is None:
            params = default_temporal_params()
        out = np.zeros((h, w, 4), np.float32)
        length = np.zeros((h, w), np.float32) if want_length else None
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        fp = C.POINTER(C.c_float)
        _check(lib().rt_render_temporal_motion(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                               C.byref(tiles), total_frame_index, w, h, frame_count, C.byref(params),
                                               C.byref(state), out.ctypes.data_as(fp),
                                               length.ctypes.data_as(fp) if want_length else None, C.byref(stats)))
        return out, length, stats

    def render_temporal_motion_device(self, camera, settings, filter_cache, w, h, params, state, d_out, d_length_out=None,
                                      stream=None, frame_count=0, total_frame_index=0, tile=64, shard_index=0,
                                      shard_count=1):
        """rt_render_temporal_motion_device into device pointers (as render_temporal_device); `state` as for
        render_temporal_motion -> the beauty frame's stats."""
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        _check(lib().rt_render_temporal_motion_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                                      C.byref(tiles), total_frame_index, w, h, frame_count,
                                                      C.byref(params), C.byref(state), C.c_void_p(d_out),
                                                      C.c_void_p(d_length_out) if d_length_out else None,
                                                      C.c_void_p(stream) if stream else None, C.byref(stats)))
        return stats

    def gbuffer_surface(self, camera, w, h, lens_distortion=0.0):
        """rt_gbuffer_surface: gbuffer() and, beside it, a structured array (h, w) of abi.SURFACE_DTYPE {triangle, v, w,
        reserved}: the mesh-local original triangle index and the barycentrics of a hit on a mesh, {0xFFFFFFFF, 0, 0, 0}
        elsewhere -> (gbuffer, surface)."""
        out = np.zeros((h, w), abi.GBUFFER_DTYPE)
        surface = np.zeros((h, w), abi.SURFACE_DTYPE)
        _check(lib().rt_gbuffer_surface(self._h, C.byref(camera), float(lens_distortion), w, h,
                                        out.ctypes.data_as(C.POINTER(GBufferTexel)),
                                        surface.ctypes.data_as(C.POINTER(SurfaceTexel))))
        return out, surface

    def gbuffer_surface_device(self, camera, w, h, d_out, d_surface, lens_distortion=0.0, stream=None):
        """rt_gbuffer_surface_device into device pointers of w*h 32-byte texels and w*h 16-byte surface records."""
        _check(lib().rt_gbuffer_surface_device(self._h, C.byref(camera), float(lens_distortion), w, h, C.c_void_p(d_out),
                                               C.c_void_p(d_surface) if d_surface else None,
                                               C.c_void_p(stream) if stream else None))

    def deform_table(self, meshes, prev):
        """rt_scene_deform_table (no device work): `meshes` a list of (mesh_index, d_prev_triangles, d_prev_normals or
        None) with device pointers or torch tensors (or a DeformMesh array), `prev` the transforms primitive_transforms()
        returned the frame before -> a structured array of abi.DEFORM_DTYPE."""
        prev = np.ascontiguousarray(prev, abi.M4X4INV_DTYPE)
        arr = deform_meshes(meshes)
        out = np.zeros(prev.shape[0], abi.DEFORM_DTYPE)
        _check(lib().rt_scene_deform_table(self._h, len(arr), arr if len(arr) else None, prev.shape[0],
                                           prev.ctypes.data_as(C.POINTER(M4x4Inv)),
                                           out.ctypes.data_as(C.POINTER(DeformEntry))))
        return out

    def render_temporal_deform(self, camera, settings, filter_cache, w, h, state, meshes=(), params=None, frame_count=0,
                               total_frame_index=0, tile=64, shard_index=0, shard_count=1, want_length=True):
        """rt_render_temporal_deform: render_temporal_motion with a history that also follows update_mesh.  `state` is a
        TemporalMotionState whose d_workspace points at temporal_deform_workspace_bytes(w, h, primitive count) bytes;
        `meshes` lists what was deformed since the previous frame as deform_table() takes it, each with the vertex
        buffer the previous frame was rendered with -> (history, length or None, the beauty frame's stats)."""
        if params is None:
            params = default_temporal_params()
        out = np.zeros((h, w, 4), np.float32)
        length = np.zeros((h, w), np.float32) if want_length else None
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        arr = deform_meshes(meshes)
        fp = C.POINTER(C.c_float)
        _check(lib().rt_render_temporal_deform(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                               C.byref(tiles), total_frame_index, w, h, frame_count, C.byref(params),
                                               C.byref(state), len(arr), arr if len(arr) else None, out.ctypes.data_as(fp),
                                               length.ctypes.data_as(fp) if want_length else None, C.byref(stats)))
        return out, length, stats

    def render_temporal_deform_device(self, camera, settings, filter_cache, w, h, params, state, meshes, d_out,
                                      d_length_out=None, stream=None, frame_count=0, total_frame_index=0, tile=64,
                                      shard_index=0, shard_count=1):
        """rt_render_temporal_deform_device into device pointers (as render_temporal_motion_device); `state` and
        `meshes` as for render_temporal_deform -> the beauty frame's stats."""
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        arr = deform_meshes(meshes)
        _check(lib().rt_render_temporal_deform_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                                      C.byref(tiles), total_frame_index, w, h, frame_count,
                                                      C.byref(params), C.byref(state), len(arr),
                                                      arr if len(arr) else None, C.c_void_p(d_out),
                                                      C.c_void_p(d_length_out) if d_length_out else None,
                                                      C.c_void_p(stream) if stream else None, C.byref(stats)))
        return stats

    def render_temporal_clipped(self, camera, settings, filter_cache, w, h, state, meshes=(), params=None, clip_params=None,
                                frame_count=0, total_frame_index=0, tile=64, shard_index=0, shard_count=1, want_length=True,
                                want_clip_amount=True):
        """rt_render_temporal_clipped: render_temporal_deform with the history clipped to the current frame's
        neighbourhood before the blend.  `state` is a TemporalMotionState whose d_workspace points at
        temporal_clipped_workspace_bytes(w, h, primitive count) bytes; `clip_params` a TemporalClipParams (None: the
        defaults) -> (history, length or None, clip amount (h, w) or None, the beauty frame's stats)."""
        if params is None:
            params = default_temporal_params()
        if clip_params is None:
            clip_params = default_temporal_clip_params()
        out = np.zeros((h, w, 4), np.float32)
        length = np.zeros((h, w), np.float32) if want_length else None
        amount = np.zeros((h, w), np.float32) if want_clip_amount else None
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        arr = deform_meshes(meshes)
        fp = C.POINTER(C.c_float)
        _check(lib().rt_render_temporal_clipped(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                                C.byref(tiles), total_frame_index, w, h, frame_count, C.byref(params),
                                                C.byref(state), len(arr), arr if len(arr) else None, C.byref(clip_params),
                                                out.ctypes.data_as(fp), length.ctypes.data_as(fp) if want_length else None,
                                                amount.ctypes.data_as(fp) if want_clip_amount else None, C.byref(stats)))
        return out, length, amount, stats

    def render_temporal_clipped_device(self, camera, settings, filter_cache, w, h, params, state, meshes, clip_params, d_out,
                                       d_length_out=None, d_clip_amount_out=None, stream=None, frame_count=0,
                                       total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_temporal_clipped_device into device pointers (as render_temporal_deform_device); `clip_params` a
        TemporalClipParams or None (a null pointer, which the entry refuses) -> the beauty frame's stats."""
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        arr = deform_meshes(meshes)
        vp = lambda a: C.c_void_p(a) if a else None
        _check(lib().rt_render_temporal_clipped_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                                       C.byref(tiles), total_frame_index, w, h, frame_count,
                                                       C.byref(params), C.byref(state), len(arr),
                                                       arr if len(arr) else None,
                                                       None if clip_params is None else C.byref(clip_params), vp(d_out),
                                                       vp(d_length_out), vp(d_clip_amount_out), vp(stream), C.byref(stats)))
        return stats

    def gbuffer_specular(self, camera, w, h, params=None, lens_distortion=0.0, want_chain=True):
        """rt_gbuffer_specular: the G-buffer that follows the camera ray through mirrors and glass.  `params` a
        GBufferSpecularParams (None: the defaults) -> (a structured array (h, w) of abi.GBUFFER_DTYPE, and one of
        abi.SPECULAR_CHAIN_DTYPE {first_primitive, first_t, chain, end} or None)."""
        if params is None:
            params = default_gbuffer_specular_params()
        out = np.zeros((h, w), abi.GBUFFER_DTYPE)
        chain = np.zeros((h, w), abi.SPECULAR_CHAIN_DTYPE) if want_chain else None
        _check(lib().rt_gbuffer_specular(self._h, C.byref(camera), float(lens_distortion), w, h, C.byref(params),
                                         out.ctypes.data_as(C.POINTER(GBufferTexel)),
                                         chain.ctypes.data_as(C.POINTER(SpecularTexel2)) if want_chain else None))
        return out, chain

    def gbuffer_specular_device(self, camera, w, h, params, d_out, d_chain=None, lens_distortion=0.0, stream=None):
        """rt_gbuffer_specular_device into device pointers of w*h 32-byte texels and, optionally, w*h 16-byte side
        records; `params` a GBufferSpecularParams or None (a null pointer, which the entry refuses)."""
        vp = lambda a: C.c_void_p(a) if a else None
        _check(lib().rt_gbuffer_specular_device(self._h, C.byref(camera), float(lens_distortion), w, h,
                                                None if params is None else C.byref(params), vp(d_out), vp(d_chain),
                                                vp(stream)))

    def render_temporal_specular(self, camera, settings, filter_cache, w, h, state, params=None, specular_params=None,
                                 clip_params=None, frame_count=0, total_frame_index=0, tile=64, shard_index=0,
                                 shard_count=1, want_length=True):
        """rt_render_temporal_specular: render_temporal over the specular G-buffer.  `state` is a TemporalState whose
        d_workspace points at temporal_specular_workspace_bytes(w, h) bytes; `specular_params` a GBufferSpecularParams
        (None: the defaults); `clip_params` a TemporalClipParams, or None for the plain accumulate stage
        -> (history, length or None, the beauty frame's stats)."""
        if params is None:
            params = default_temporal_params()
        if specular_params is None:
            specular_params = default_gbuffer_specular_params()
        out = np.zeros((h, w, 4), np.float32)
        length = np.zeros((h, w), np.float32) if want_length else None
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        fp = C.POINTER(C.c_float)
        _check(lib().rt_render_temporal_specular(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                                 C.byref(tiles), total_frame_index, w, h, frame_count, C.byref(params),
                                                 C.byref(state), C.byref(specular_params),
                                                 None if clip_params is None else C.byref(clip_params),
                                                 out.ctypes.data_as(fp), length.ctypes.data_as(fp) if want_length else None,
                                                 C.byref(stats)))
        return out, length, stats

    def render_temporal_specular_device(self, camera, settings, filter_cache, w, h, params, state, specular_params,
                                        clip_params, d_out, d_length_out=None, stream=None, frame_count=0,
                                        total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_temporal_specular_device into device pointers (as render_temporal_device); `specular_params` a
        GBufferSpecularParams or None (a null pointer, which the entry refuses), `clip_params` a TemporalClipParams or
        None (the plain accumulate stage) -> the beauty frame's stats."""
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        vp = lambda a: C.c_void_p(a) if a else None
        _check(lib().rt_render_temporal_specular_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                                        C.byref(tiles), total_frame_index, w, h, frame_count,
                                                        C.byref(params), C.byref(state),
                                                        None if specular_params is None else C.byref(specular_params),
                                                        None if clip_params is None else C.byref(clip_params), vp(d_out),
                                                        vp(d_length_out), vp(stream), C.byref(stats)))
        return stats

    def render_temporal_filtered(self, camera, settings, filter_cache, w, h, state, params=None, filter_params=None,
                                 spatial_below=abi.RT_TEMPORAL_SPATIAL_BELOW_DEFAULT, frame_count=0, total_frame_index=0,
                                 tile=64, shard_index=0, shard_count=1, want_extras=True):
        """rt_render_temporal_filtered: one frame of the loop with the variance-guided filter.  `state` is a
        TemporalFilteredState whose d_workspace points at temporal_filtered_workspace_bytes(w, h) bytes on the device
        (all else zero at the start); it is updated in place -> (filtered float32 [h,w,4] = {r, g, b, 1}, then the
        unfiltered history [h,w,4], its length [h,w] and the variance [h,w], or three None, the beauty frame's stats)."""
        if params is None:
            params = default_temporal_params()
        if filter_params is None:
            filter_params = default_denoise_variance_params()
        out = np.zeros((h, w, 4), np.float32)
        hist = np.zeros((h, w, 4), np.float32) if want_extras else None
        length = np.zeros((h, w), np.float32) if want_extras else None
        var = np.zeros((h, w), np.float32) if want_extras else None
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        fp = C.POINTER(C.c_float)
        opt = lambda a: a.ctypes.data_as(fp) if a is not None else None
        _check(lib().rt_render_temporal_filtered(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                                 C.byref(tiles), total_frame_index, w, h, frame_count, C.byref(params),
                                                 float(spatial_below), C.byref(filter_params), C.byref(state),
                                                 out.ctypes.data_as(fp), opt(hist), opt(length), opt(var), C.byref(stats)))
        return out, hist, length, var, stats

    def render_temporal_filtered_device(self, camera, settings, filter_cache, w, h, params, filter_params, state, d_out,
                                        d_history_out=None, d_length_out=None, d_variance_out=None,
                                        spatial_below=abi.RT_TEMPORAL_SPATIAL_BELOW_DEFAULT, stream=None, frame_count=0,
                                        total_frame_index=0, tile=64, shard_index=0, shard_count=1):
        """rt_render_temporal_filtered_device into device pointers (d_out w*h float4; the unfiltered history w*h float4,
        its length and the variance w*h floats each, or None); `state` as for render_temporal_filtered -> the beauty
        frame's stats."""
        tiles = TileSet(tile, tile, shard_index, shard_count)
        stats = Stats()
        vp = lambda a: C.c_void_p(a) if a else None
        _check(lib().rt_render_temporal_filtered_device(self._h, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                                        C.byref(tiles), total_frame_index, w, h, frame_count,
                                                        C.byref(params), float(spatial_below), C.byref(filter_params),
                                                        C.byref(state), vp(d_out), vp(d_history_out), vp(d_length_out),
                                                        vp(d_variance_out), vp(stream), C.byref(stats)))
        return stats

    def configure(self, **fields):
        """rt_scene_set_config with the named fields changed, e.g. configure(partitions=1,
        splat_mode=abi.RT_SPLAT_EXACT).  Returns the previous configuration (pass it to
        set_config to restore it)."""
        old = self.config()
        c = abi.SceneConfig.from_buffer_copy(old)
        for k, v in fields.items():
            if k not in dict(abi.SceneConfig._fields_):
                raise AttributeError(f"rt_scene_config has no field {k!r}")
            setattr(c, k, v)
        self.set_config(c)
        return old

    def set_config(self, c):
        _check(lib().rt_scene_set_config(self._h, C.byref(c)))

    def configured(self, **fields):
        """with dev.configured(partitions=1): ... -- the scene's configuration restored after."""
        dev = self

        class _Ctx:
            def __enter__(self):
                self.old = dev.configure(**fields)
                return dev

            def __exit__(self, *exc):
                dev.set_config(self.old)
                return False
        return _Ctx()


def resolve_bgra8(accum, post):
    h, w, _ = accum.shape
    out = np.zeros((h, w), np.uint32)
    buf = AccumulationBuffer(w, h, 0, accum.ctypes.data_as(C.POINTER(C.c_float)))
    lib().rth_resolve_bgra8(C.byref(buf), C.byref(post), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out


def postprocess(accum, post, total_frame_index=0, device=0):
    """The output pass on the GPU (rt_postprocess; RT/raytracer.cpp:2103-2171): host float4 (h, w, 4) in,
    BGRA8 (h, w) u32 out, with the reference's TPDF blue-noise dither."""
    accum = np.ascontiguousarray(accum, np.float32)
    h, w, _ = accum.shape
    out = np.zeros((h, w), np.uint32)
    buf = AccumulationBuffer(w, h, 0, accum.ctypes.data_as(C.POINTER(C.c_float)))
    _check(lib().rt_postprocess(device, C.byref(buf), C.byref(post), total_frame_index,
                                out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


def default_denoise_params():
    """rt_denoise_default_params (no device needed) -> DenoiseParams."""
    p = DenoiseParams()
    _check(lib().rt_denoise_default_params(C.byref(p)))
    return p


def denoise_workspace_bytes(w, h):
    """rt_denoise_workspace_bytes (no device needed): 64 bytes per pixel."""
    return int(lib().rt_denoise_workspace_bytes(w, h))


def denoise(accum, guide0=None, guide1=None, params=None, device=0):
    """The denoise stage on the GPU (rt_denoise): host float4 accumulation buffers (h, w, 4) in -- the beauty
    frame and up to two guide frames, e.g. DeviceScene.render_guides' -- and the filtered buffer out, which
    postprocess() takes as it is.  params: DenoiseParams; None takes default_denoise_params() with the sigma
    of an absent guide switched off."""
    accum = np.ascontiguousarray(accum, np.float32)
    h, w, _ = accum.shape
    if params is None:
        params = default_denoise_params()
        for k, g in enumerate((guide0, guide1)):
            if g is None:
                params.sigma_guide[k] = 0.0
    fp = C.POINTER(C.c_float)
    guides = []
    for g in (guide0, guide1):
        if g is not None:
            g = np.ascontiguousarray(g, np.float32)
            assert g.shape == accum.shape
        guides.append(g)
    out = np.zeros((h, w, 4), np.float32)
    buf = AccumulationBuffer(w, h, 0, accum.ctypes.data_as(fp))
    _check(lib().rt_denoise(device, C.byref(buf), *[g.ctypes.data_as(fp) if g is not None else None for g in guides],
                            C.byref(params), out.ctypes.data_as(fp)))
    return out


def default_denoise_features_params():
    """rt_denoise_features_default_params (no device needed) -> DenoiseFeaturesParams."""
    p = DenoiseFeaturesParams()
    _check(lib().rt_denoise_features_default_params(C.byref(p)))
    return p


def denoise_features_workspace_bytes(w, h):
    """rt_denoise_features_workspace_bytes (no device needed): 80 bytes per pixel."""
    return int(lib().rt_denoise_features_workspace_bytes(w, h))


def denoise_features(accum, normal=None, distance=None, albedo=None, params=None, device=0):
    """The denoise stage with feature frames on the GPU (rt_denoise_features): host float4 accumulation buffers
    (h, w, 4) in -- the beauty frame and DeviceScene.render_feature's NORMAL, DISTANCE and ALBEDO frames -- and
    the filtered buffer out.  params: DenoiseFeaturesParams; None takes default_denoise_features_params() with
    the terms of an absent frame switched off."""
    accum = np.ascontiguousarray(accum, np.float32)
    h, w, _ = accum.shape
    if params is None:
        params = default_denoise_features_params()
        for k, g in enumerate((normal, distance)):
            if g is None:
                params.base.sigma_guide[k] = 0.0
        if albedo is None:
            params.sigma_albedo, params.demodulate = 0.0, 0
    fp = C.POINTER(C.c_float)
    frames = []
    for g in (normal, distance, albedo):
        if g is not None:
            g = np.ascontiguousarray(g, np.float32)
            assert g.shape == accum.shape
        frames.append(g)
    out = np.zeros((h, w, 4), np.float32)
    buf = AccumulationBuffer(w, h, 0, accum.ctypes.data_as(fp))
    _check(lib().rt_denoise_features(device, C.byref(buf),
                                     *[g.ctypes.data_as(fp) if g is not None else None for g in frames],
                                     C.byref(params), out.ctypes.data_as(fp)))
    return out


def default_tile_error_params():
    """rt_tile_error_default_params (no device needed) -> TileErrorParams."""
    p = TileErrorParams()
    _check(lib().rt_tile_error_default_params(C.byref(p)))
    return p


def default_adaptive_params():
    """rt_adaptive_default_params (no device needed) -> AdaptiveParams."""
    p = AdaptiveParams()
    _check(lib().rt_adaptive_default_params(C.byref(p)))
    return p


def adaptive_workspace_bytes(w, h, tile=64):
    """rt_adaptive_workspace_bytes (no device needed): the two half buffers and the per-tile lists."""
    return int(lib().rt_adaptive_workspace_bytes(w, h, tile, tile))


def tile_error(half_a, half_b, tile=64, tile_ids=None, params=None, device=0):
    """The tile error estimate on the GPU (rt_tile_error): two host float4 accumulation buffers (h, w, 4) holding
    disjoint halves of the samples -> (error float32, valid uint32), per listed tile (None: every tile)."""
    a = np.ascontiguousarray(half_a, np.float32)
    b = np.ascontiguousarray(half_b, np.float32)
    assert a.shape == b.shape
    h, w, _ = a.shape
    if params is None:
        params = default_tile_error_params()
    ids = None if tile_ids is None else np.ascontiguousarray(tile_ids, np.uint32).reshape(-1)
    count = ((w + tile - 1) // tile)*((h + tile - 1) // tile) if ids is None else ids.size
    err = np.zeros(count, np.float32)
    valid = np.zeros(count, np.uint32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    _check(lib().rt_tile_error(device, a.ctypes.data_as(fp), b.ctypes.data_as(fp), w, h, tile, tile,
                               None if ids is None else ids.ctypes.data_as(up), count, C.byref(params),
                               err.ctypes.data_as(fp), valid.ctypes.data_as(up)))
    return err, valid


def default_robust_params():
    """rt_robust_default_params (no device needed) -> RobustParams."""
    p = RobustParams()
    _check(lib().rt_robust_default_params(C.byref(p)))
    return p


def robust_workspace_bytes(w, h, buffers=8):
    """rt_robust_workspace_bytes (no device needed): the stack, buffers*w*h*16 bytes."""
    return int(lib().rt_robust_workspace_bytes(w, h, buffers))


def robust_combine(stack, params=None, device=0, want_info=True):
    """The robust estimator on the GPU (rt_robust_combine): a host stack of K float4 accumulation buffers
    (K, h, w, 4) holding disjoint sample sets of one frame -> (out (h, w, 4), info (h, w, 4) or None)."""
    stack = np.ascontiguousarray(stack, np.float32)
    k, h, w, _ = stack.shape
    if params is None:
        params = default_robust_params()
    out = np.zeros((h, w, 4), np.float32)
    info = np.zeros((h, w, 4), np.float32) if want_info else None
    fp = C.POINTER(C.c_float)
    _check(lib().rt_robust_combine(device, stack.ctypes.data_as(fp), k, w, h, C.byref(params), out.ctypes.data_as(fp),
                                   info.ctypes.data_as(fp) if want_info else None))
    return out, info


def default_temporal_params():
    """rt_temporal_default_params (no device needed) -> TemporalParams."""
    p = TemporalParams()
    _check(lib().rt_temporal_default_params(C.byref(p)))
    return p


def temporal_workspace_bytes(w, h):
    """rt_temporal_workspace_bytes (no device needed): the driver's workspace, 120 bytes per pixel."""
    return int(lib().rt_temporal_workspace_bytes(w, h))


def temporal_accumulate(current, gbuffer, prev=None, prev_camera=None, prev_lens_distortion=0.0, params=None, device=0):
    """The accumulate stage on the GPU (rt_temporal_accumulate): a host accumulation buffer (h, w, 4), its G-buffer
    (h, w) of abi.GBUFFER_DTYPE and, with history, prev = (history (h, w, 4), length (h, w), gbuffer (h, w)) of the
    frame before with its camera and lens distortion -> (history (h, w, 4), length (h, w))."""
    current = np.ascontiguousarray(current, np.float32)
    h, w, _ = current.shape
    gbuffer = np.ascontiguousarray(gbuffer, abi.GBUFFER_DTYPE)
    assert gbuffer.shape == (h, w)
    if params is None:
        params = default_temporal_params()
    fp, gp = C.POINTER(C.c_float), C.POINTER(GBufferTexel)
    ph = pl = pg = None
    if prev is not None:
        ph = np.ascontiguousarray(prev[0], np.float32)
        pl = np.ascontiguousarray(prev[1], np.float32)
        pg = np.ascontiguousarray(prev[2], abi.GBUFFER_DTYPE)
        assert ph.shape == (h, w, 4) and pl.shape == (h, w) and pg.shape == (h, w)
    history = np.zeros((h, w, 4), np.float32)
    length = np.zeros((h, w), np.float32)
    _check(lib().rt_temporal_accumulate(device, current.ctypes.data_as(fp), gbuffer.ctypes.data_as(gp),
                                        None if ph is None else ph.ctypes.data_as(fp),
                                        None if pl is None else pl.ctypes.data_as(fp),
                                        None if pg is None else pg.ctypes.data_as(gp),
                                        None if prev_camera is None else C.byref(prev_camera), float(prev_lens_distortion),
                                        w, h, C.byref(params), history.ctypes.data_as(fp), length.ctypes.data_as(fp)))
    return history, length


def temporal_accumulate_device(d_current, d_gbuffer, d_prev_history, d_prev_length, d_prev_gbuffer, prev_camera,
                               prev_lens_distortion, w, h, params, d_history, d_length, device=0, stream=None):
    """rt_temporal_accumulate_device on device pointers (the three d_prev_* all None for no history)."""
    vp = lambda a: C.c_void_p(a) if a else None
    _check(lib().rt_temporal_accumulate_device(device, vp(d_current), vp(d_gbuffer), vp(d_prev_history), vp(d_prev_length),
                                               vp(d_prev_gbuffer), None if prev_camera is None else C.byref(prev_camera),
                                               float(prev_lens_distortion), w, h, C.byref(params), vp(d_history),
                                               vp(d_length), vp(stream)))


def temporal_motion_workspace_bytes(w, h, primitive_count):
    """rt_temporal_motion_workspace_bytes (no device needed): temporal_workspace_bytes and the motion table."""
    return int(lib().rt_temporal_motion_workspace_bytes(w, h, primitive_count))


def motion_table(cur, prev):
    """rt_motion_table (no device needed): two arrays of abi.M4X4INV_DTYPE (the current and the previous resolved
    transforms, as DeviceScene.primitive_transforms returns them) -> a structured array of abi.MOTION_DTYPE."""
    cur = np.ascontiguousarray(cur, abi.M4X4INV_DTYPE)
    prev = np.ascontiguousarray(prev, abi.M4X4INV_DTYPE)
    assert cur.shape == prev.shape and cur.ndim == 1
    out = np.zeros(cur.shape[0], abi.MOTION_DTYPE)
    mp = C.POINTER(M4x4Inv)
    _check(lib().rt_motion_table(cur.shape[0], cur.ctypes.data_as(mp), prev.ctypes.data_as(mp),
                                 out.ctypes.data_as(C.POINTER(MotionEntry))))
    return out


def temporal_accumulate_motion(current, gbuffer, prev=None, prev_camera=None, prev_lens_distortion=0.0, params=None,
                               motion=None, want_moments=False, want_velocity=False, device=0):
    """The motion-aware accumulate stage on the GPU (rt_temporal_accumulate_motion): temporal_accumulate's arguments,
    `motion` a table of abi.MOTION_DTYPE or None, prev = (history, length, gbuffer) and with want_moments also the
    previous moments (h, w, 2) -> (history, length, moments (h, w, 2) or None, velocity (h, w, 2) or None)."""
    current = np.ascontiguousarray(current, np.float32)
    h, w, _ = current.shape
    gbuffer = np.ascontiguousarray(gbuffer, abi.GBUFFER_DTYPE)
    assert gbuffer.shape == (h, w)
    if params is None:
        params = default_temporal_params()
    fp, gp = C.POINTER(C.c_float), C.POINTER(GBufferTexel)
    ph = pl = pg = pm = None
    if prev is not None:
        ph = np.ascontiguousarray(prev[0], np.float32)
        pl = np.ascontiguousarray(prev[1], np.float32)
        pg = np.ascontiguousarray(prev[2], abi.GBUFFER_DTYPE)
        assert ph.shape == (h, w, 4) and pl.shape == (h, w) and pg.shape == (h, w)
        if want_moments:
            pm = np.ascontiguousarray(prev[3], np.float32)
            assert pm.shape == (h, w, 2)
    count = 0
    if motion is not None:
        motion = np.ascontiguousarray(motion, abi.MOTION_DTYPE)
        count = motion.shape[0]
    history = np.zeros((h, w, 4), np.float32)
    length = np.zeros((h, w), np.float32)
    moments = np.zeros((h, w, 2), np.float32) if want_moments else None
    velocity = np.zeros((h, w, 2), np.float32) if want_velocity else None
    opt = lambda a, t: None if a is None else a.ctypes.data_as(t)
    _check(lib().rt_temporal_accumulate_motion(device, current.ctypes.data_as(fp), gbuffer.ctypes.data_as(gp), opt(ph, fp),
                                               opt(pl, fp), opt(pg, gp),
                                               None if prev_camera is None else C.byref(prev_camera),
                                               float(prev_lens_distortion), w, h, C.byref(params),
                                               history.ctypes.data_as(fp), length.ctypes.data_as(fp),
                                               opt(motion if count else None, C.POINTER(MotionEntry)), count, opt(pm, fp),
                                               opt(moments, fp), opt(velocity, fp)))
    return history, length, moments, velocity


def temporal_accumulate_motion_device(d_current, d_gbuffer, d_prev_history, d_prev_length, d_prev_gbuffer, prev_camera,
                                      prev_lens_distortion, w, h, params, d_history, d_length, d_motion=None, motion_count=0,
                                      d_prev_moments=None, d_moments=None, d_velocity=None, device=0, stream=None):
    """rt_temporal_accumulate_motion_device on device pointers (the d_prev_* all None for no history; d_motion,
    d_moments with d_prev_moments, and d_velocity optional)."""
    vp = lambda a: C.c_void_p(a) if a else None
    _check(lib().rt_temporal_accumulate_motion_device(device, vp(d_current), vp(d_gbuffer), vp(d_prev_history),
                                                      vp(d_prev_length), vp(d_prev_gbuffer),
                                                      None if prev_camera is None else C.byref(prev_camera),
                                                      float(prev_lens_distortion), w, h, C.byref(params), vp(d_history),
                                                      vp(d_length), vp(stream), vp(d_motion), motion_count,
                                                      vp(d_prev_moments), vp(d_moments), vp(d_velocity)))


def deform_meshes(meshes):
    """A list of (mesh_index, d_prev_triangles, d_prev_normals or None), pointers or torch tensors -> a DeformMesh
    array (the tensors must stay alive while it is used); a DeformMesh array passes through."""
    if isinstance(meshes, C.Array):
        return meshes
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
    arr = (DeformMesh*len(meshes))()
    for k, (m, t, n) in enumerate(meshes):
        arr[k] = DeformMesh(m, 0, ptr(t), ptr(n))
    return arr


def temporal_deform_workspace_bytes(w, h, primitive_count):
    """rt_temporal_deform_workspace_bytes (no device needed): temporal_motion_workspace_bytes, the surface records and
    the deform table."""
    return int(lib().rt_temporal_deform_workspace_bytes(w, h, primitive_count))


def temporal_accumulate_deform(current, gbuffer, prev=None, prev_camera=None, prev_lens_distortion=0.0, params=None,
                               motion=None, surface=None, deform=None, want_moments=False, want_velocity=False, device=0):
    """The deform-aware accumulate stage on the GPU (rt_temporal_accumulate_deform): temporal_accumulate_motion's
    arguments, `surface` (h, w) of abi.SURFACE_DTYPE and `deform` a table of abi.DEFORM_DTYPE (its vertex pointers
    device pointers) or None -> (history, length, moments or None, velocity or None)."""
    current = np.ascontiguousarray(current, np.float32)
    h, w, _ = current.shape
    gbuffer = np.ascontiguousarray(gbuffer, abi.GBUFFER_DTYPE)
    assert gbuffer.shape == (h, w)
    if params is None:
        params = default_temporal_params()
    fp, gp = C.POINTER(C.c_float), C.POINTER(GBufferTexel)
    ph = pl = pg = pm = None
    if prev is not None:
        ph = np.ascontiguousarray(prev[0], np.float32)
        pl = np.ascontiguousarray(prev[1], np.float32)
        pg = np.ascontiguousarray(prev[2], abi.GBUFFER_DTYPE)
        assert ph.shape == (h, w, 4) and pl.shape == (h, w) and pg.shape == (h, w)
        if want_moments:
            pm = np.ascontiguousarray(prev[3], np.float32)
            assert pm.shape == (h, w, 2)
    count = dcount = 0
    if motion is not None:
        motion = np.ascontiguousarray(motion, abi.MOTION_DTYPE)
        count = motion.shape[0]
    if deform is not None:
        deform = np.ascontiguousarray(deform, abi.DEFORM_DTYPE)
        dcount = deform.shape[0]
    if surface is not None:
        surface = np.ascontiguousarray(surface, abi.SURFACE_DTYPE)
        assert surface.shape == (h, w)
    history = np.zeros((h, w, 4), np.float32)
    length = np.zeros((h, w), np.float32)
    moments = np.zeros((h, w, 2), np.float32) if want_moments else None
    velocity = np.zeros((h, w, 2), np.float32) if want_velocity else None
    opt = lambda a, t: None if a is None else a.ctypes.data_as(t)
    _check(lib().rt_temporal_accumulate_deform(device, current.ctypes.data_as(fp), gbuffer.ctypes.data_as(gp), opt(ph, fp),
                                               opt(pl, fp), opt(pg, gp),
                                               None if prev_camera is None else C.byref(prev_camera),
                                               float(prev_lens_distortion), w, h, C.byref(params),
                                               history.ctypes.data_as(fp), length.ctypes.data_as(fp),
                                               opt(motion if count else None, C.POINTER(MotionEntry)), count, opt(pm, fp),
                                               opt(moments, fp), opt(velocity, fp), opt(surface, C.POINTER(SurfaceTexel)),
                                               opt(deform if dcount else None, C.POINTER(DeformEntry)), dcount))
    return history, length, moments, velocity


def temporal_accumulate_deform_device(d_current, d_gbuffer, d_prev_history, d_prev_length, d_prev_gbuffer, prev_camera,
                                      prev_lens_distortion, w, h, params, d_history, d_length, d_motion=None, motion_count=0,
                                      d_prev_moments=None, d_moments=None, d_velocity=None, d_surface=None, d_deform=None,
                                      deform_count=0, device=0, stream=None):
    """rt_temporal_accumulate_deform_device on device pointers: temporal_accumulate_motion_device's arguments, the
    surface records and the deform table."""
    vp = lambda a: C.c_void_p(a) if a else None
    _check(lib().rt_temporal_accumulate_deform_device(device, vp(d_current), vp(d_gbuffer), vp(d_prev_history),
                                                      vp(d_prev_length), vp(d_prev_gbuffer),
                                                      None if prev_camera is None else C.byref(prev_camera),
                                                      float(prev_lens_distortion), w, h, C.byref(params), vp(d_history),
                                                      vp(d_length), vp(stream), vp(d_motion), motion_count,
                                                      vp(d_prev_moments), vp(d_moments), vp(d_velocity), vp(d_surface),
                                                      vp(d_deform), deform_count))


def default_temporal_clip_params():
    """rt_temporal_clip_default_params (no device needed) -> TemporalClipParams."""
    p = TemporalClipParams()
    _check(lib().rt_temporal_clip_default_params(C.byref(p)))
    return p


def temporal_clipped_workspace_bytes(w, h, primitive_count):
    """rt_temporal_clipped_workspace_bytes (no device needed): temporal_deform_workspace_bytes, the neighbourhood texels
    and the clip amounts."""
    return int(lib().rt_temporal_clipped_workspace_bytes(w, h, primitive_count))


def default_gbuffer_specular_params():
    """rt_gbuffer_specular_default_params (no device needed) -> GBufferSpecularParams."""
    p = GBufferSpecularParams()
    _check(lib().rt_gbuffer_specular_default_params(C.byref(p)))
    return p


def temporal_specular_workspace_bytes(w, h):
    """rt_temporal_specular_workspace_bytes (no device needed): temporal_workspace_bytes and the neighbourhood texels."""
    return int(lib().rt_temporal_specular_workspace_bytes(w, h))


def temporal_neighbourhood(current, radius, firefly_clamp, device=0):
    """The statistics of the current frame's windows on the GPU (rt_temporal_neighbourhood): a host accumulation buffer
    (h, w, 4) -> a structured array (h, w) of abi.NEIGHBOURHOOD_DTYPE {mean, count, sigma, reserved}."""
    current = np.ascontiguousarray(current, np.float32)
    h, w, _ = current.shape
    out = np.zeros((h, w), abi.NEIGHBOURHOOD_DTYPE)
    _check(lib().rt_temporal_neighbourhood(device, current.ctypes.data_as(C.POINTER(C.c_float)), w, h, int(radius),
                                           float(firefly_clamp), out.ctypes.data_as(C.POINTER(NeighbourhoodTexel))))
    return out


def temporal_neighbourhood_device(d_current, w, h, radius, firefly_clamp, d_out, device=0, stream=None):
    """rt_temporal_neighbourhood_device on device pointers: w*h float4 in, w*h 32-byte texels out."""
    vp = lambda a: C.c_void_p(a) if a else None
    _check(lib().rt_temporal_neighbourhood_device(device, vp(d_current), w, h, int(radius), float(firefly_clamp), vp(d_out),
                                                  vp(stream)))


def temporal_accumulate_clip(current, gbuffer, prev=None, prev_camera=None, prev_lens_distortion=0.0, params=None,
                             motion=None, surface=None, deform=None, neighbourhood=None, gamma=0.5, min_count=2.0,
                             want_moments=False, want_velocity=False, want_clip_amount=True, device=0):
    """The accumulate stage with a clip on the GPU (rt_temporal_accumulate_clip): temporal_accumulate_deform's arguments,
    `neighbourhood` (h, w) of abi.NEIGHBOURHOOD_DTYPE or None, gamma and min_count
    -> (history, length, moments or None, velocity or None, clip amount (h, w) or None)."""
    current = np.ascontiguousarray(current, np.float32)
    h, w, _ = current.shape
    gbuffer = np.ascontiguousarray(gbuffer, abi.GBUFFER_DTYPE)
    assert gbuffer.shape == (h, w)
    if params is None:
        params = default_temporal_params()
    fp, gp = C.POINTER(C.c_float), C.POINTER(GBufferTexel)
    ph = pl = pg = pm = None
    if prev is not None:
        ph = np.ascontiguousarray(prev[0], np.float32)
        pl = np.ascontiguousarray(prev[1], np.float32)
        pg = np.ascontiguousarray(prev[2], abi.GBUFFER_DTYPE)
        assert ph.shape == (h, w, 4) and pl.shape == (h, w) and pg.shape == (h, w)
        if want_moments:
            pm = np.ascontiguousarray(prev[3], np.float32)
            assert pm.shape == (h, w, 2)
    count = dcount = 0
    if motion is not None:
        motion = np.ascontiguousarray(motion, abi.MOTION_DTYPE)
        count = motion.shape[0]
    if deform is not None:
        deform = np.ascontiguousarray(deform, abi.DEFORM_DTYPE)
        dcount = deform.shape[0]
    if surface is not None:
        surface = np.ascontiguousarray(surface, abi.SURFACE_DTYPE)
        assert surface.shape == (h, w)
    if neighbourhood is not None:
        neighbourhood = np.ascontiguousarray(neighbourhood, abi.NEIGHBOURHOOD_DTYPE)
        assert neighbourhood.shape == (h, w)
    history = np.zeros((h, w, 4), np.float32)
    length = np.zeros((h, w), np.float32)
    moments = np.zeros((h, w, 2), np.float32) if want_moments else None
    velocity = np.zeros((h, w, 2), np.float32) if want_velocity else None
    amount = np.zeros((h, w), np.float32) if want_clip_amount else None
    opt = lambda a, t: None if a is None else a.ctypes.data_as(t)
    _check(lib().rt_temporal_accumulate_clip(device, current.ctypes.data_as(fp), gbuffer.ctypes.data_as(gp), opt(ph, fp),
                                             opt(pl, fp), opt(pg, gp),
                                             None if prev_camera is None else C.byref(prev_camera),
                                             float(prev_lens_distortion), w, h, C.byref(params),
                                             history.ctypes.data_as(fp), length.ctypes.data_as(fp),
                                             opt(motion if count else None, C.POINTER(MotionEntry)), count, opt(pm, fp),
                                             opt(moments, fp), opt(velocity, fp), opt(surface, C.POINTER(SurfaceTexel)),
                                             opt(deform if dcount else None, C.POINTER(DeformEntry)), dcount,
                                             opt(neighbourhood, C.POINTER(NeighbourhoodTexel)), float(gamma),
                                             float(min_count), opt(amount, fp)))
    return history, length, moments, velocity, amount


def temporal_accumulate_clip_device(d_current, d_gbuffer, d_prev_history, d_prev_length, d_prev_gbuffer, prev_camera,
                                    prev_lens_distortion, w, h, params, d_history, d_length, d_motion=None, motion_count=0,
                                    d_prev_moments=None, d_moments=None, d_velocity=None, d_surface=None, d_deform=None,
                                    deform_count=0, d_neighbourhood=None, gamma=0.5, min_count=2.0, d_clip_amount=None,
                                    device=0, stream=None):
    """rt_temporal_accumulate_clip_device on device pointers: temporal_accumulate_deform_device's arguments, the
    neighbourhood texels, gamma, min_count and the clip amounts (optional)."""
    vp = lambda a: C.c_void_p(a) if a else None
    _check(lib().rt_temporal_accumulate_clip_device(device, vp(d_current), vp(d_gbuffer), vp(d_prev_history),
                                                    vp(d_prev_length), vp(d_prev_gbuffer),
                                                    None if prev_camera is None else C.byref(prev_camera),
                                                    float(prev_lens_distortion), w, h, C.byref(params), vp(d_history),
                                                    vp(d_length), vp(stream), vp(d_motion), motion_count,
                                                    vp(d_prev_moments), vp(d_moments), vp(d_velocity), vp(d_surface),
                                                    vp(d_deform), deform_count, vp(d_neighbourhood), float(gamma),
                                                    float(min_count), vp(d_clip_amount)))


def default_denoise_variance_params():
    """rt_denoise_variance_default_params (no device needed) -> DenoiseVarianceParams."""
    p = DenoiseVarianceParams()
    _check(lib().rt_denoise_variance_default_params(C.byref(p)))
    return p


def denoise_variance_workspace_bytes(w, h):
    """rt_denoise_variance_workspace_bytes (no device needed): the filter's workspace, 40 bytes per pixel."""
    return int(lib().rt_denoise_variance_workspace_bytes(w, h))


def temporal_filtered_workspace_bytes(w, h):
    """rt_temporal_filtered_workspace_bytes (no device needed): the filtered driver's workspace, 180 bytes per pixel."""
    return int(lib().rt_temporal_filtered_workspace_bytes(w, h))


def temporal_accumulate_moments(current, gbuffer, prev=None, prev_camera=None, prev_lens_distortion=0.0, params=None,
                                device=0):
    """The accumulate stage with moments on the GPU (rt_temporal_accumulate_moments): temporal_accumulate's arguments with
    prev = (history (h, w, 4), length (h, w), gbuffer (h, w), moments (h, w, 2)) -> (history, length, moments (h, w, 2))."""
    current = np.ascontiguousarray(current, np.float32)
    h, w, _ = current.shape
    gbuffer = np.ascontiguousarray(gbuffer, abi.GBUFFER_DTYPE)
    assert gbuffer.shape == (h, w)
    if params is None:
        params = default_temporal_params()
    fp, gp = C.POINTER(C.c_float), C.POINTER(GBufferTexel)
    ph = pl = pg = pm = None
    if prev is not None:
        ph = np.ascontiguousarray(prev[0], np.float32)
        pl = np.ascontiguousarray(prev[1], np.float32)
        pg = np.ascontiguousarray(prev[2], abi.GBUFFER_DTYPE)
        pm = np.ascontiguousarray(prev[3], np.float32)
        assert ph.shape == (h, w, 4) and pl.shape == (h, w) and pg.shape == (h, w) and pm.shape == (h, w, 2)
    history = np.zeros((h, w, 4), np.float32)
    length = np.zeros((h, w), np.float32)
    moments = np.zeros((h, w, 2), np.float32)
    _check(lib().rt_temporal_accumulate_moments(device, current.ctypes.data_as(fp), gbuffer.ctypes.data_as(gp),
                                                None if ph is None else ph.ctypes.data_as(fp),
                                                None if pl is None else pl.ctypes.data_as(fp),
                                                None if pg is None else pg.ctypes.data_as(gp),
                                                None if pm is None else pm.ctypes.data_as(fp),
                                                None if prev_camera is None else C.byref(prev_camera),
                                                float(prev_lens_distortion), w, h, C.byref(params),
                                                history.ctypes.data_as(fp), length.ctypes.data_as(fp),
                                                moments.ctypes.data_as(fp)))
    return history, length, moments


def temporal_accumulate_moments_device(d_current, d_gbuffer, d_prev_history, d_prev_length, d_prev_gbuffer, d_prev_moments,
                                       prev_camera, prev_lens_distortion, w, h, params, d_history, d_length, d_moments,
                                       device=0, stream=None):
    """rt_temporal_accumulate_moments_device on device pointers (the four d_prev_* all None for no history)."""
    vp = lambda a: C.c_void_p(a) if a else None
    _check(lib().rt_temporal_accumulate_moments_device(device, vp(d_current), vp(d_gbuffer), vp(d_prev_history),
                                                       vp(d_prev_length), vp(d_prev_gbuffer), vp(d_prev_moments),
                                                       None if prev_camera is None else C.byref(prev_camera),
                                                       float(prev_lens_distortion), w, h, C.byref(params), vp(d_history),
                                                       vp(d_length), vp(d_moments), vp(stream)))


def temporal_variance(moments, length, gbuffer, params=None, spatial_below=abi.RT_TEMPORAL_SPATIAL_BELOW_DEFAULT, device=0):
    """The variance of the history on the GPU (rt_temporal_variance): moments (h, w, 2), length (h, w) and the frame's
    G-buffer (h, w) -> variance (h, w)."""
    moments = np.ascontiguousarray(moments, np.float32)
    h, w, _ = moments.shape
    length = np.ascontiguousarray(length, np.float32)
    gbuffer = np.ascontiguousarray(gbuffer, abi.GBUFFER_DTYPE)
    assert length.shape == (h, w) and gbuffer.shape == (h, w)
    if params is None:
        params = default_temporal_params()
    fp = C.POINTER(C.c_float)
    out = np.zeros((h, w), np.float32)
    _check(lib().rt_temporal_variance(device, moments.ctypes.data_as(fp), length.ctypes.data_as(fp),
                                      gbuffer.ctypes.data_as(C.POINTER(GBufferTexel)), w, h, C.byref(params),
                                      float(spatial_below), out.ctypes.data_as(fp)))
    return out


def temporal_variance_device(d_moments, d_length, d_gbuffer, w, h, params, spatial_below, d_variance, device=0, stream=None):
    """rt_temporal_variance_device on device pointers."""
    vp = lambda a: C.c_void_p(a) if a else None
    _check(lib().rt_temporal_variance_device(device, vp(d_moments), vp(d_length), vp(d_gbuffer), w, h, C.byref(params),
                                             float(spatial_below), vp(d_variance), vp(stream)))


def denoise_variance(color, variance, gbuffer, params=None, device=0, want_variance=True):
    """The variance-guided filter on the GPU (rt_denoise_variance): a host colour buffer (h, w, 4) (a history {r, g, b, 1}
    or an accumulation buffer), its variance (h, w) and the frame's G-buffer (h, w) -> (out (h, w, 4), the filtered
    variance (h, w) or None)."""
    color = np.ascontiguousarray(color, np.float32)
    h, w, _ = color.shape
    variance = np.ascontiguousarray(variance, np.float32)
    gbuffer = np.ascontiguousarray(gbuffer, abi.GBUFFER_DTYPE)
    assert variance.shape == (h, w) and gbuffer.shape == (h, w)
    if params is None:
        params = default_denoise_variance_params()
    fp = C.POINTER(C.c_float)
    out = np.zeros((h, w, 4), np.float32)
    var_out = np.zeros((h, w), np.float32) if want_variance else None
    _check(lib().rt_denoise_variance(device, color.ctypes.data_as(fp), variance.ctypes.data_as(fp),
                                     gbuffer.ctypes.data_as(C.POINTER(GBufferTexel)), w, h, C.byref(params),
                                     out.ctypes.data_as(fp), var_out.ctypes.data_as(fp) if want_variance else None))
    return out, var_out


def denoise_variance_device(d_color, d_variance, d_gbuffer, w, h, params, d_out, d_variance_out=None, d_workspace=None,
                            device=0, stream=None):
    """rt_denoise_variance_device on device pointers (d_out may be d_color, d_variance_out may be d_variance or None;
    d_workspace None: the call allocates its own)."""
    vp = lambda a: C.c_void_p(a) if a else None
    _check(lib().rt_denoise_variance_device(device, vp(d_color), vp(d_variance), vp(d_gbuffer), w, h, C.byref(params),
                                            vp(d_workspace), vp(d_out), vp(d_variance_out), vp(stream)))


def write_bitmap(path, bgra):
    h, w = bgra.shape
    b = np.ascontiguousarray(bgra, np.uint32)
    if not lib().rth_write_bitmap(str(path).encode(), b.ctypes.data_as(C.POINTER(C.c_uint32)), w, h):
        raise OSError(lib().rth_last_error().decode())


def set_splat_mode(mode):
    """rt_set_splat_mode: abi.RT_SPLAT_STREAM (default), RT_SPLAT_EXACT (the reference's splat
    order, bit-identical frames) or RT_SPLAT_ATOMIC."""
    _check(lib().rt_set_splat_mode(int(mode)))


def set_shard_mode(mode):
    """rt_set_shard_mode: abi.RT_SHARD_TILES (default: tile t to shard t % n) or RT_SHARD_PASSES
    (every tile, a contiguous range of the sample passes per shard)."""
    _check(lib().rt_set_shard_mode(int(mode)))


class splat_mode:
    """with splat_mode(abi.RT_SPLAT_EXACT): ... restores the default (streaming) splat after."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        set_splat_mode(self.mode)
        return self

    def __exit__(self, *exc):
        set_splat_mode(abi.RT_SPLAT_STREAM)
        return False


def set_env_sampling(mode):
    """rt_set_env_sampling: 1 = environment-map importance sampling in the NEE (beyond the
    reference, whose environment CDF is never read), 0 = the reference's estimator (default)."""
    _check(lib().rt_set_env_sampling(int(mode)))


class env_sampling:
    """with env_sampling(1): ... turns environment-map sampling off again after."""

    def __init__(self, mode=1):
        self.mode = mode

    def __enter__(self):
        set_env_sampling(self.mode)
        return self

    def __exit__(self, *exc):
        set_env_sampling(0)
        return False


def read_bitmap(path, w, h):
    """The BGRA8 pixels (h, w) u32 of a bitmap write_bitmap wrote."""
    out = np.zeros((h, w), np.uint32)
    if not lib().rth_read_bitmap(str(path).encode(), out.ctypes.data_as(C.POINTER(C.c_uint32)), w, h):
        raise OSError(lib().rth_last_error().decode())
    return out


def take_picture(scene, camera, settings, filter_cache, post, w, h, spp, path, total_frame_index=0, device=0):
    """rth_take_picture: the reference's "Take picture" (RT/raytracer.cpp:2031-2185) -> BMP at `path`."""
    stats = Stats()
    _check(lib().rth_take_picture(scene.handle, C.byref(camera), C.byref(settings), C.byref(filter_cache),
                                  C.byref(post), w, h, spp, total_frame_index, device, str(path).encode(),
                                  C.byref(stats)))
    return stats


def integrator_name(integrator):
    """rt_integrator_name: the reference's name of a g_integrators index (RT/integrators.cpp:823-830),
    None when out of range."""
    name = lib().rt_integrator_name(int(integrator))
    return None if name is None else name.decode()


def find_integrator(name):
    """rt_find_integrator: the index of a name, 0 (the default integrator) when unknown, as the
    reference's find_integrator (RT/integrators.cpp:835-845)."""
    return int(lib().rt_find_integrator(str(name).encode()))


def integrator_supported(integrator):
    """rt_integrator_supported: True when the render entries take this integrator (Whitted and Ground
    Truth Recursive are refused: they need a per-path recursion stack)."""
    return bool(lib().rt_integrator_supported(int(integrator)))


def scene_integrator_supported(dev, integrator):
    """rt_scene_integrator_supported for a DeviceScene, or None: then it equals integrator_supported."""
    return bool(lib().rt_scene_integrator_supported(dev._h if dev is not None else None, int(integrator)))


def device_count():
    n = C.c_int()
    lib().rt_device_count(C.byref(n))
    return n.value
