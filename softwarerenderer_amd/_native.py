"""ctypes binding of libswr_hip.so (the C ABI declared in include/swr.h).

There is no CPU fallback: if the shared library is missing or no gfx950 device is usable the
import / context creation raises.  PyTorch is optional plumbing (device memory, streams,
torch.distributed); when it is already imported the library binds to the HIP runtime torch
loaded (same SONAME), so both live on one runtime.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SWR_LIB selects another in-tree build of the SAME source (the numerics sensitivity builds libswr_hip_fma.so /
# libswr_hip_dotpw.so of csrc/Makefile, or a test build); there is no non-HIP alternative to select
LIB_PATH = os.path.join(_HERE, os.path.basename(os.environ.get("SWR_LIB", "") or "libswr_hip.so"))

SWR_OK = 0
SWR_PROG_USER_BASE = 256     # ids of user fragment programs (swr_program_create) are >= this
SWR_ABI_EXPECTED = 3
SWR_ERR_INVALID_ARG = -1
SWR_ERR_HIP = -2
SWR_ERR_OOM = -3
SWR_ERR_NO_DEVICE = -4
SWR_ERR_UNSUPPORTED = -5
SWR_TEXTURE_ALPHA_OPAQUE, SWR_TEXTURE_ALPHA_KEEP = 0, 1     # swr_texture_update_from_frame
SWR_TEXTURE_FORMAT_RGBA8, SWR_TEXTURE_FORMAT_DEPTH32F = 0, 1     # swr_texture_format
SWR_DEPTH_REDUCE_MAX, SWR_DEPTH_REDUCE_MIN, SWR_DEPTH_REDUCE_FIRST = 0, 1, 2     # swr_texture_update_from_depth
SWR_POST_RGB32F, SWR_POST_RGB8, SWR_POST_RGBX8 = 0, 3, 4     # swr_readback_post & co: what a post program's result becomes
SWR_POST_TEXTURES = 4                                        # swr_post_set_texture: slots 0 .. 3
SWR_PROGRAM_TEXTURES = 4                                     # user programs: slot 0 the draw's texture, swr_program_set_texture: slots 1 .. 3
SWR_STALE = 1          # swr_present_wait: not an error -- the copied frame predates a replayed batch, present again


class SwrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"swr error {code}: {msg}")
        self.code = code


class Vertex(C.Structure):  # Shaders.VertexInput, Shaders.cs:10-24 (48 bytes)
    _fields_ = [("position", C.c_float * 3), ("uv", C.c_float * 2), ("normal", C.c_float * 3), ("color", C.c_float * 4)]


class PointLight(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("range", C.c_float), ("color", C.c_float * 3), ("intensity", C.c_float)]


class Uniforms(C.Structure):  # swr_uniforms == fields of Renderer.cs:39-44 (+ build-defined Phong block)
    _fields_ = [
        ("light_direction", C.c_float * 3), ("_pad0", C.c_float),
        ("light_color", C.c_float * 4),
        ("fog_color", C.c_float * 4),
        ("fog_start", C.c_float), ("fog_end", C.c_float),
        ("shininess", C.c_float), ("_pad1", C.c_float),
        ("camera_position", C.c_float * 3), ("_pad2", C.c_float),
        ("lights", PointLight * 4),
    ]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "triangles_in", "triangles_setup", "triangles_clipped", "fragments_tested",
        "fragments_shaded", "fragments_written", "tile_pairs", "flushes")]


class Profile(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("vertex_ms", "setup_ms", "bin_ms", "sort_ms", "cover_ms", "raster_ms", "clear_ms", "total_ms")] + \
               [("raster_launches", C.c_uint64), ("flushes", C.c_uint64)]


class Ray(C.Structure):  # swr_ray (24 bytes): Physics.Raycast's rayOrigin, rayDirection
    _fields_ = [("origin", C.c_float * 3), ("direction", C.c_float * 3)]


class RayTarget(C.Structure):  # swr_ray_target (136 bytes): a retained mesh, its model matrix and Transpose(Invert(model))
    _fields_ = [("mesh", C.c_void_p), ("model", C.c_float * 16), ("normal_matrix", C.c_float * 16)]


class RayHit(C.Structure):  # swr_ray_hit (40 bytes)
    _fields_ = [("found", C.c_int32), ("target", C.c_int32), ("triangle", C.c_int32), ("distance", C.c_float),
                ("point", C.c_float * 3), ("normal", C.c_float * 3)]


class CharacterParams(C.Structure):  # swr_character_params (52 bytes): the properties of CharacterController.cs:21-32
    _fields_ = [("gravity", C.c_float * 3)] + [(n, C.c_float) for n in (
        "height", "radius", "step_size", "move_speed", "jump_force", "ground_acceleration", "air_acceleration", "max_air_speed",
        "ground_friction", "air_control")]


class Character(C.Structure):  # swr_character (44 bytes): one controller's state, in and out
    _fields_ = [("position", C.c_float * 3), ("velocity", C.c_float * 3), ("jump_cooldown", C.c_float), ("actual_step_size", C.c_float),
                ("grounded", C.c_int32), ("ceiling", C.c_int32), ("noclip", C.c_int32)]


class CharacterInput(C.Structure):  # swr_character_input (16 bytes)
    _fields_ = [("move", C.c_float * 3), ("jump", C.c_int32)]


class CharacterTrace(C.Structure):  # swr_character_trace (48 bytes)
    _fields_ = [("ground_found", C.c_int32), ("ceiling_found", C.c_int32), ("ground_point", C.c_float * 3), ("ground_normal", C.c_float * 3),
                ("chain_attempts", C.c_int32 * 2), ("chain_stop", C.c_int32 * 2)]


class AnimChannel(C.Structure):  # swr_anim_channel (32 bytes): one glTF animation channel with its sampler
    _fields_ = [("node", C.c_int32), ("path", C.c_int32), ("interpolation", C.c_int32), ("n_keys", C.c_int32),
                ("times", C.c_void_p), ("values", C.c_void_p)]


class PoseRequest(C.Structure):  # swr_pose_request (20 bytes)
    _fields_ = [("clip_a", C.c_int32), ("time_a", C.c_float), ("clip_b", C.c_int32), ("time_b", C.c_float), ("weight", C.c_float)]


SWR_ANIM_PATH_TRANSLATION, SWR_ANIM_PATH_ROTATION, SWR_ANIM_PATH_SCALE = 0, 1, 2
SWR_ANIM_STEP, SWR_ANIM_LINEAR, SWR_ANIM_CUBICSPLINE = 0, 1, 2
SWR_SKELETON_MAX_NODES = 65535

SWR_RAY_FACES_ALL, SWR_RAY_IGNORE_BACKFACES, SWR_RAY_IGNORE_FRONTFACES, SWR_RAY_CROSS_FUSED = 0, 1, 2, 0x100

# every symbol include/swr.h declares; tests/test_abi.py checks the library exports all of them
EXPORTS = [
    "swr_abi_version", "swr_build_info", "swr_numerics_mode", "swr_set_transform_fma", "swr_get_transform_fma", "swr_set_pipelining", "swr_get_pipelining", "swr_last_error", "swr_create", "swr_destroy", "swr_resize", "swr_set_band", "swr_set_band_interleaved",
    "swr_bind_framebuffer", "swr_set_stream", "swr_clear_color", "swr_clear_depth", "swr_get_pixel",
    "swr_set_pixel", "swr_get_depth", "swr_set_depth", "swr_readback", "swr_readback_rgb", "swr_present_rgb_async", "swr_present_wait", "swr_flatten_rgb_device", "swr_flatten_rgb_device_async", "swr_replay_count", "swr_sync_count", "swr_host_register", "swr_host_unregister", "swr_upload", "swr_color_device_ptr",
    "swr_depth_device_ptr", "swr_texture_create", "swr_texture_destroy", "swr_texture_set_filter", "swr_texture_sample",
    "swr_mesh_create", "swr_mesh_destroy", "swr_set_state", "swr_initialize_tile_locks", "swr_render_mesh",
    "swr_render_mesh_arrays", "swr_mesh_bounds", "swr_is_sphere_in_frustum", "swr_render_mesh_culled", "swr_flush", "swr_sync", "swr_interpolate", "swr_get_stats", "swr_reset_stats",
    "swr_profile_enable", "swr_profile_get", "swr_profile_reset", "swr_profile_raster_samples", "swr_device_name", "swr_debug_counters", "swr_selftest_division",
    "swr_program_create", "swr_program_destroy", "swr_program_set_constants", "swr_program_validate",
    "swr_program_set_texture",
    "swr_program_create_vf", "swr_program_validate_vf",
    "swr_raycast", "swr_raycast_nearest", "swr_character_ray_counts", "swr_character_update",
    "swr_resolved_size", "swr_readback_rgb_resolved", "swr_present_rgb_resolved_async", "swr_resolve_rgb_device", "swr_resolve_rgb_device_async",
    "swr_present8_size", "swr_readback_rgb8", "swr_present_rgb8_async", "swr_resolve_rgb8_device", "swr_resolve_rgb8_device_async",
    "swr_texture_create_target", "swr_texture_update_from_frame", "swr_texture_readback",
    "swr_post_create", "swr_post_destroy", "swr_post_set_constants", "swr_post_validate", "swr_post_size",
    "swr_readback_post", "swr_present_post_async", "swr_post_device", "swr_post_device_async",
    "swr_post_set_texture", "swr_texture_update_from_post",
    "swr_texture_create_depth", "swr_texture_update_from_depth", "swr_texture_readback_depth", "swr_texture_sample_depth", "swr_texture_format",
    "swr_texture_generate_mipmaps", "swr_texture_levels", "swr_texture_level_size", "swr_texture_readback_level", "swr_texture_sample_lod", "swr_texture_lod",
    "swr_texture_create_cube", "swr_texture_create_cube_depth", "swr_texture_is_cube", "swr_texture_update_face_from_frame",
    "swr_texture_update_face_from_depth", "swr_texture_update_face_from_post", "swr_texture_readback_face", "swr_cube_face_view",
    "swr_texture_cube_face", "swr_texture_sample_cube", "swr_texture_sample_cube_depth",
    "swr_mesh_create_like", "swr_mesh_readback", "swr_mesh_blend", "swr_mesh_set_skin", "swr_mesh_skin",
    "swr_skeleton_create", "swr_skeleton_destroy", "swr_skeleton_add_clip", "swr_pose_set_create", "swr_pose_set_destroy",
    "swr_pose_set_sample", "swr_pose_set_upload", "swr_pose_set_readback", "swr_mesh_skin_batch",
]

_libs = {}


def load(name: str = None) -> C.CDLL:
    """Load libswr_hip.so (built by __graft_entry__.build()), or another in-tree build of the same source by file name
    (the numerics sensitivity builds, the test build).  Raises if it is absent.  The libraries are linked -Bsymbolic, so
    several builds can live in one process without binding to each other's kernels."""
    path = LIB_PATH if not name else os.path.join(_HERE, os.path.basename(name))
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). softwarerenderer_amd has no CPU fallback.")
    lib = C.CDLL(path, mode=C.RTLD_LOCAL)
    P, I, F = C.c_void_p, C.c_int, C.c_float
    fp = C.POINTER(C.c_float)
    sig = {
        "swr_abi_version": (I, []),
        "swr_build_info": (C.c_char_p, []),
        "swr_numerics_mode": (I, [C.POINTER(I), C.POINTER(I)]),
        "swr_set_transform_fma": (I, [P, I, I]),
        "swr_get_transform_fma": (I, [P, C.POINTER(I), C.POINTER(I)]),
        "swr_set_pipelining": (I, [P, I]),
        "swr_get_pipelining": (I, [P, C.POINTER(I)]),
        "swr_last_error": (C.c_char_p, [P]),
        "swr_create": (I, [I, C.POINTER(P)]),
        "swr_destroy": (None, [P]),
        "swr_resize": (I, [P, I, I]),
        "swr_set_band": (I, [P, I, I]),
        "swr_set_band_interleaved": (I, [P, I, I, I]),
        "swr_bind_framebuffer": (I, [P, P, P]),
        "swr_set_stream": (I, [P, P]),
        "swr_clear_color": (I, [P, fp]),
        "swr_clear_depth": (I, [P]),
        "swr_get_pixel": (I, [P, I, I, fp]),
        "swr_set_pixel": (I, [P, I, I, fp]),
        "swr_get_depth": (I, [P, I, I, fp]),
        "swr_set_depth": (I, [P, I, I, F]),
        "swr_readback": (I, [P, P, P]),
        "swr_readback_rgb": (I, [P, P]),
        "swr_present_rgb_async": (I, [P, P, C.POINTER(C.c_uint64)]),
        "swr_present_wait": (I, [P, C.c_uint64]),
        "swr_flatten_rgb_device": (I, [P, P]),
        "swr_flatten_rgb_device_async": (I, [P, P]),
        "swr_replay_count": (I, [P, C.POINTER(C.c_uint64)]),
        "swr_sync_count": (I, [P, C.POINTER(C.c_uint64)]),
        "swr_host_register": (I, [P, P, C.c_size_t]),
        "swr_host_unregister": (I, [P, P]),
        "swr_upload": (I, [P, P, P]),
        "swr_color_device_ptr": (I, [P, C.POINTER(P)]),
        "swr_depth_device_ptr": (I, [P, C.POINTER(P)]),
        "swr_texture_create": (I, [P, P, I, I, C.POINTER(P)]),
        "swr_texture_destroy": (I, [P, P]),
        "swr_texture_set_filter": (I, [P, P, I]),
        "swr_texture_sample": (I, [P, P, P, I, P]),
        "swr_mesh_create": (I, [P, P, I, P, I, C.POINTER(P)]),
        "swr_mesh_destroy": (I, [P, P]),
        "swr_set_state": (I, [P, F, F, I]),
        "swr_initialize_tile_locks": (I, [P, I, I]),
        "swr_render_mesh": (I, [P, P, fp, fp, fp, I, C.POINTER(Uniforms), P, I, I, I]),
        "swr_render_mesh_arrays": (I, [P, P, I, P, I, fp, fp, fp, I, C.POINTER(Uniforms), P, I, I, I]),
        "swr_mesh_bounds": (I, [P, P, fp]),
        "swr_is_sphere_in_frustum": (I, [P, fp, fp, fp, fp, C.POINTER(I)]),
        "swr_render_mesh_culled": (I, [P, P, fp, fp, fp, I, C.POINTER(Uniforms), P, I, I, I]),
        "swr_flush": (I, [P]),
        "swr_sync": (I, [P]),
        "swr_interpolate": (I, [P, P, P, I, I, P]),
        "swr_get_stats": (I, [P, C.POINTER(Stats)]),
        "swr_reset_stats": (I, [P]),
        "swr_profile_enable": (I, [P, I]),
        "swr_profile_get": (I, [P, C.POINTER(Profile)]),
        "swr_profile_reset": (I, [P]),
        "swr_profile_raster_samples": (I, [P, fp, I, C.POINTER(I)]),
        "swr_device_name": (I, [P, C.c_char_p, I]),
        "swr_debug_counters": (I, [P, C.POINTER(C.c_uint64)]),
        "swr_selftest_division": (I, [P, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
        "swr_program_create": (I, [P, C.c_char_p, C.POINTER(I)]),
        "swr_program_destroy": (I, [P, I]),
        "swr_program_set_constants": (I, [P, I, fp, I]),
        "swr_program_set_texture": (I, [P, I, I, P]),
        "swr_program_validate": (I, [C.c_char_p, C.c_char_p, I]),
        "swr_program_create_vf": (I, [P, C.c_char_p, C.c_char_p, C.POINTER(I)]),
        "swr_program_validate_vf": (I, [C.c_char_p, C.c_char_p, C.c_char_p, I]),
        "swr_raycast": (I, [P, P, I, P, I, I, P]),
        "swr_raycast_nearest": (I, [P, P, I, P, I, I, P]),
        "swr_character_ray_counts": (I, [P, C.POINTER(I), C.POINTER(I)]),
        "swr_character_update": (I, [P, P, P, P, I, F, P, I, P, I, I, P]),
        "swr_resolved_size": (I, [P, I, I, C.POINTER(I), C.POINTER(I)]),
        "swr_readback_rgb_resolved": (I, [P, I, I, P]),
        "swr_present_rgb_resolved_async": (I, [P, I, I, P, C.POINTER(C.c_uint64)]),
        "swr_resolve_rgb_device": (I, [P, I, I, P]),
        "swr_resolve_rgb_device_async": (I, [P, I, I, P]),
        "swr_present8_size": (I, [P, I, I, I, C.POINTER(I), C.POINTER(I), C.POINTER(C.c_size_t)]),
        "swr_readback_rgb8": (I, [P, I, I, I, P]),
        "swr_present_rgb8_async": (I, [P, I, I, I, P, C.POINTER(C.c_uint64)]),
        "swr_resolve_rgb8_device": (I, [P, I, I, I, P]),
        "swr_resolve_rgb8_device_async": (I, [P, I, I, I, P]),
        "swr_texture_create_target": (I, [P, I, I, C.POINTER(P)]),
        "swr_texture_update_from_frame": (I, [P, P, P, I, I, I]),
        "swr_texture_readback": (I, [P, P, P]),
        "swr_post_create": (I, [P, C.c_char_p, C.POINTER(I)]),
        "swr_post_destroy": (I, [P, I]),
        "swr_post_set_constants": (I, [P, I, fp, I]),
        "swr_post_validate": (I, [C.c_char_p, C.c_char_p, I]),
        "swr_post_size": (I, [P, I, I, I, C.POINTER(I), C.POINTER(I), C.POINTER(C.c_size_t)]),
        "swr_readback_post": (I, [P, I, I, I, I, P]),
        "swr_present_post_async": (I, [P, I, I, I, I, P, C.POINTER(C.c_uint64)]),
        "swr_post_device": (I, [P, I, I, I, I, P]),
        "swr_post_device_async": (I, [P, I, I, I, I, P]),
        "swr_post_set_texture": (I, [P, I, I, P]),
        "swr_texture_update_from_post": (I, [P, P, P, I, I, I, I]),
        "swr_texture_create_depth": (I, [P, P, I, I, C.POINTER(P)]),
        "swr_texture_update_from_depth": (I, [P, P, P, I, I, I]),
        "swr_texture_readback_depth": (I, [P, P, P]),
        "swr_texture_sample_depth": (I, [P, P, P, I, P]),
        "swr_texture_format": (I, [P, P, C.POINTER(I)]),
        "swr_texture_generate_mipmaps": (I, [P, P]),
        "swr_texture_levels": (I, [P, P, C.POINTER(I)]),
        "swr_texture_level_size": (I, [P, P, I, C.POINTER(I), C.POINTER(I)]),
        "swr_texture_readback_level": (I, [P, P, I, P]),
        "swr_texture_sample_lod": (I, [P, P, P, I, P]),
        "swr_texture_lod": (I, [P, P, P, I, P]),
        "swr_texture_create_cube": (I, [P, P, I, C.POINTER(P)]),
        "swr_texture_create_cube_depth": (I, [P, P, I, C.POINTER(P)]),
        "swr_texture_is_cube": (I, [P, P, C.POINTER(I)]),
        "swr_texture_update_face_from_frame": (I, [P, P, I, P, I, I, I]),
        "swr_texture_update_face_from_depth": (I, [P, P, I, P, I, I, I]),
        "swr_texture_update_face_from_post": (I, [P, P, I, P, I, I, I, I]),
        "swr_texture_readback_face": (I, [P, P, I, I, P]),
        "swr_cube_face_view": (I, [I, P, P]),
        "swr_texture_cube_face": (I, [P, P, I, P, P]),
        "swr_texture_sample_cube": (I, [P, P, P, I, P]),
        "swr_texture_sample_cube_depth": (I, [P, P, P, I, P]),
        "swr_mesh_create_like": (I, [P, P, C.POINTER(P)]),
        "swr_mesh_readback": (I, [P, P, P]),
        "swr_mesh_blend": (I, [P, P, P, P, F]),
        "swr_mesh_set_skin": (I, [P, P, P, P]),
        "swr_mesh_skin": (I, [P, P, P, fp, I]),
        "swr_skeleton_create": (I, [P, I, P, P, P, P, P, I, P, P, C.POINTER(P)]),
        "swr_skeleton_destroy": (I, [P, P]),
        "swr_skeleton_add_clip": (I, [P, P, P, I, C.POINTER(I)]),
        "swr_pose_set_create": (I, [P, I, I, C.POINTER(P)]),
        "swr_pose_set_destroy": (I, [P, P]),
        "swr_pose_set_sample": (I, [P, P, P, P, I]),
        "swr_pose_set_upload": (I, [P, P, I, I, P]),
        "swr_pose_set_readback": (I, [P, P, P]),
        "swr_mesh_skin_batch": (I, [P, I, P, P, P, P]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name, None)
        if fn is None:
            if os.environ.get("SWR_ABLATE_LIB"):       # tools/ablate.py timing an OLDER build of the library (build_ab/): newer entry points may be absent
                continue
            raise ImportError(f"{path} does not export {name}: rebuild it (ABI {SWR_ABI_EXPECTED})")
        fn.restype = res
        fn.argtypes = args
    _libs[path] = lib
    return lib


def check(ctx, rc: int, lib: C.CDLL = None) -> None:
    if rc != SWR_OK:
        msg = (lib or load()).swr_last_error(ctx)
        raise SwrError(rc, msg.decode() if msg else "")
