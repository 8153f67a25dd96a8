"""Host-side mirror of the reference's raster API over the HIP backend.

Same names, argument meaning and error behaviour as the C# reference so that callers and
tests read like the reference's own code (file:line under OCSYT/SoftwareRenderer):

  Rasterizer.RenderMesh / InitializeTileLocks / Interpolate, enums, statics   Rasterizer.cs:14-50,69,163,566
  Shaders.VertexInput / VertexOutput, shader delegates                        Shaders.cs:10-98
  Texture(pixels) / Width / Height / Sample / Dispose                          Texture.cs:31-68
  MainWindow.RenderWidth/RenderHeight/ColorBuffer/DepthBuffer/Get*/Set*/Clear* MainWindow.cs:25-31,378-436

C# delegates cannot cross the C ABI: a `ShaderProgram` (program id + uniform block + texture)
stands in for the (VertexShader, FragmentShader) delegate pair.  Everything below runs on the
GPU through libswr_hip.so; nothing here computes pixels on the host.
"""
from __future__ import annotations

import ctypes as C
import enum
from typing import Optional

import numpy as np

from . import _native as N

# numpy view of Shaders.VertexInput (Shaders.cs:10-24): 12 consecutive float32 = 48 bytes
VERTEX_DTYPE = np.dtype([("position", "<f4", 3), ("uv", "<f4", 2), ("normal", "<f4", 3), ("color", "<f4", 4)])
assert VERTEX_DTYPE.itemsize == 48 == C.sizeof(N.Vertex)


class DebugMode(enum.IntEnum):      # Rasterizer.cs:14-18
    None_ = 0
    Wireframe = 1


class BlendMode(enum.IntEnum):      # Rasterizer.cs:25-31
    None_ = 0
    Alpha = 1
    Additive = 2
    Multiply = 3


class DepthTest(enum.IntEnum):      # Rasterizer.cs:33-43
    Disabled = 0
    Less = 1
    LessEqual = 2
    Greater = 3
    GreaterEqual = 4
    Equal = 5
    NotEqual = 6
    Always = 7


class CullMode(enum.IntEnum):       # Rasterizer.cs:45-50
    None_ = 0
    Back = 1
    Front = 2


class DepthReduce(enum.IntEnum):    # build-defined: SWR_DEPTH_REDUCE_* of include/swr.h (Texture.UpdateFromDepth)
    Max = 0                         # the block's nearest sample under the default LessEqual test
    Min = 1
    First = 2                       # the block's top-left sample


class Program(enum.IntEnum):        # built-in programs (include/swr.h)
    FlatColor = 0
    Gouraud = 1
    Dust2LambertFog = 2
    Phong4Point = 3
    DebugVaryings = 4               # build-defined: returns Normal / ScreenCoords / Barycentric (the varyings no other built-in reads)


def _f32(a, n=None):
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1))
    if n is not None and arr.size != n:
        raise ValueError(f"expected {n} floats, got {arr.size}")
    return arr


def _fptr(arr):
    return arr.ctypes.data_as(C.POINTER(C.c_float))


def default_uniforms() -> N.Uniforms:
    """Uniform defaults of Renderer.cs:39-44 (FogStart 1, FogEnd 25, FogColor, LightDirection, LightColor)."""
    u = N.Uniforms()
    u.light_direction[:] = euler_to_direction(-45.0, -45.0, 0.0)
    u.light_color[:] = (1.0, 1.0, 1.0, 1.0)
    u.fog_color[:] = (1.0, 0.62, 0.5, 1.0)
    u.fog_start, u.fog_end = 1.0, 25.0
    u.shininess = 16.0
    return u


def euler_to_direction(pitch_deg: float, yaw_deg: float, roll_deg: float):
    """Renderer.EulerToDirection (Renderer.cs:967-972): -UnitZ rotated by CreateFromYawPitchRoll(yaw, pitch, roll),
    normalised.  Host-side input generator (float32); roll does not move the forward axis."""
    p = np.float32(pitch_deg) * np.float32(np.pi) / np.float32(180.0)
    y = np.float32(yaw_deg) * np.float32(np.pi) / np.float32(180.0)
    v = np.array([-np.sin(y) * np.cos(p), np.sin(p), -np.cos(y) * np.cos(p)], dtype=np.float32)
    v = v / np.float32(np.sqrt(np.float32(v @ v)))
    return tuple(float(t) for t in v)


class Device:
    """One swr_context = one GPU (one process per GPU)."""

    def __init__(self, device_id: int = 0, lib: str = None):
        """`lib`: file name of another in-tree build of the backend (e.g. "libswr_hip_fma.so"); default = the product library."""
        self._lib = N.load(lib)
        self._ctx = C.c_void_p()
        rc = self._lib.swr_create(int(device_id), C.byref(self._ctx))
        if rc != N.SWR_OK:
            msg = self._lib.swr_last_error(None)
            raise N.SwrError(rc, msg.decode() if msg else "swr_create failed")

    def close(self):
        if self._ctx:
            self._lib.swr_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        N.check(self._ctx, rc, self._lib)

    @property
    def name(self) -> str:
        buf = C.create_string_buffer(256)
        self._ck(self._lib.swr_device_name(self._ctx, buf, 256))
        return buf.value.decode()

    def pin(self, array: np.ndarray):
        """Page-lock a long-lived host array (swr_host_register): read-backs into it then DMA at PCIe rate."""
        self._ck(self._lib.swr_host_register(self._ctx, C.c_void_p(array.ctypes.data), C.c_size_t(array.nbytes)))

    def unpin(self, array: np.ndarray):
        self._ck(self._lib.swr_host_unregister(self._ctx, C.c_void_p(array.ctypes.data)))

    def stats(self) -> dict:
        s = N.Stats()
        self._ck(self._lib.swr_get_stats(self._ctx, C.byref(s)))
        return {n: int(getattr(s, n)) for n, _ in N.Stats._fields_}

    def reset_stats(self):
        self._ck(self._lib.swr_reset_stats(self._ctx))

    def profile_enable(self, on):
        """False/0 off, True/1 events around every stage, 2 around the raster kernel only, 3 around the raster kernel of every
        4th flush (an event pair costs about 10 us of stream time)."""
        self._ck(self._lib.swr_profile_enable(self._ctx, int(on)))

    def profile(self) -> dict:
        p = N.Profile()
        self._ck(self._lib.swr_profile_get(self._ctx, C.byref(p)))
        return {n: (float(getattr(p, n)) if t is C.c_double else int(getattr(p, n))) for n, t in N.Profile._fields_}

    def raster_samples(self) -> np.ndarray:
        """Duration (ms) of every raster-kernel launch that carried an event pair since profile_reset (swr_profile_raster_samples)."""
        n = C.c_int(0)
        self._ck(self._lib.swr_profile_raster_samples(self._ctx, None, 0, C.byref(n)))
        out = np.zeros(max(int(n.value), 1), dtype=np.float32)
        self._ck(self._lib.swr_profile_raster_samples(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float)), int(out.size), C.byref(n)))
        return out[:int(n.value)]

    def profile_reset(self):
        self._ck(self._lib.swr_profile_reset(self._ctx))

    def selftest_division(self, samples: int = 1 << 30, seed: int = 1) -> dict:
        """swr_selftest_division: the kernels' exact-division / sqrt cores against the compiler's IEEE `/` and sqrtf."""
        out = (C.c_uint64 * 8)()
        self._ck(self._lib.swr_selftest_division(self._ctx, C.c_uint64(samples), C.c_uint64(seed), out))
        keys = ("divisions", "division_mismatches", "sqrts", "sqrt_mismatches", "bad_n_bits", "bad_d_bits", "bad_got_bits", "bad_want_bits")
        return dict(zip(keys, (int(v) for v in out)))

    def replay_count(self) -> int:
        out = C.c_uint64(0)
        self._ck(self._lib.swr_replay_count(self._ctx, C.byref(out)))
        return int(out.value)

    def sync_count(self) -> int:
        """Times an entry point has made the host wait for the stream (swr_sync_count): a steady-state frame loop adds none."""
        out = C.c_uint64(0)
        self._ck(self._lib.swr_sync_count(self._ctx, C.byref(out)))
        return int(out.value)

    def build_info(self) -> str:
        """`hipcc=...; csrc_sha256=...; fma=..; dot=..` of the loaded library (swr_build_info)."""
        return self._lib.swr_build_info().decode()

    def numerics_mode(self):
        """(fma, dot_order) the loaded library was compiled with (SWR_NUMERICS_FMA, SWR_DOT_PAIRWISE)."""
        f, d = C.c_int(0), C.c_int(0)
        self._ck(self._lib.swr_numerics_mode(C.byref(f), C.byref(d)))
        return int(f.value), int(d.value)

    def set_transform_fma(self, transform_fused: bool, transform_normal_fused: bool):
        """The run-time half of the System.Numerics model (swr_set_transform_fma): do Vector4.Transform (Renderer.cs:832-834) /
        Vector3.TransformNormal (:835) fuse their multiply-adds?  Default = the library's compile-time fma for both."""
        self._ck(self._lib.swr_set_transform_fma(self._ctx, int(bool(transform_fused)), int(bool(transform_normal_fused))))

    def transform_fma(self):
        a, b = C.c_int(0), C.c_int(0)
        self._ck(self._lib.swr_get_transform_fma(self._ctx, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    def set_pipelining(self, mode: int):
        """swr_set_pipelining: 0 = one stream (kernel timings are quoted on this), 1 = the front end of flush N+1 beside the raster
        kernel of flush N, every asynchronous batch (default), 2 = the same for small frames / batches only (<= 2^15 tiles or <= 2^17 triangles)."""
        self._ck(self._lib.swr_set_pipelining(self._ctx, int(mode)))

    def pipelining(self) -> int:
        m = C.c_int(0)
        self._ck(self._lib.swr_get_pipelining(self._ctx, C.byref(m)))
        return int(m.value)

    def compile_program(self, source: str, vertex_source: Optional[str] = None) -> int:
        """swr_program_create_vf: compile a user program for this device -- C++ defining `swr_fragment` and, with `vertex_source`,
        `swr_vertex` (contract in include/swr.h); without it the vertex stage is Renderer.VertexShader.  Returns its id
        (>= SWR_PROG_USER_BASE).  A compile error raises SwrError(SWR_ERR_INVALID_ARG) with the log."""
        pid = C.c_int(0)
        vs = vertex_source.encode() if vertex_source is not None else None
        self._ck(self._lib.swr_program_create_vf(self._ctx, vs, source.encode(), C.byref(pid)))
        return pid.value

    def destroy_program(self, program_id: int):
        """Draws recorded with the program still render with it."""
        self._ck(self._lib.swr_program_destroy(self._ctx, int(program_id)))

    def set_program_constants(self, program_id: int, values):
        """Up to 64 floats the program reads as env.constants[i]; each draw captures them when it is recorded."""
        a = _f32(values if values is not None else [], None)
        self._ck(self._lib.swr_program_set_constants(self._ctx, int(program_id), _fptr(a) if a.size else None, int(a.size)))

    def set_program_texture(self, program_id: int, slot: int, texture: Optional["Texture"]):
        """Bind a Texture of this Device to slot 1 .. 3 of a user program (None unbinds; slot 0 is the draw's own texture): both
        halves read it with swr_sample / swr_texel(env, slot, ..).  Each draw captures the slots, and each texture's filter, when
        it is recorded."""
        self._ck(self._lib.swr_program_set_texture(self._ctx, int(program_id), int(slot), texture._h if texture is not None else None))

    def set_stream(self, hip_stream: int):
        self._ck(self._lib.swr_set_stream(self._ctx, C.c_void_p(hip_stream)))

    def flush(self):
        self._ck(self._lib.swr_flush(self._ctx))

    def sync(self):
        self._ck(self._lib.swr_sync(self._ctx))

    def SkinBatch(self, dsts, srcs, pose_set: "PoseSet", instances):
        """swr_mesh_skin_batch: dsts[k] = srcs[k] skinned by the palette of instances[k] of `pose_set`, all jobs in one kernel launch
        (word for word what Mesh.SkinFrom gives with that palette).  Two jobs may share a source or an instance."""
        n = len(dsts)
        if len(srcs) != n or len(instances) != n:
            raise ValueError("dsts, srcs and instances must have equal lengths")
        d = (C.c_void_p * max(n, 1))(*[m._h.value if m is not None else None for m in dsts])
        q = (C.c_void_p * max(n, 1))(*[m._h.value if m is not None else None for m in srcs])
        i = np.ascontiguousarray(instances, dtype=np.int32).reshape(-1)
        self._ck(self._lib.swr_mesh_skin_batch(self._ctx, n, d, q, pose_set._h if pose_set is not None else None, i.ctypes.data if n else None))


class PostProgram:
    """A post-process program (swr_post_create): C++ defining `swr_post` (contract in include/swr.h), compiled for the device at
    run time and run once per output pixel by MainWindow.PostBuffer / PresentPostAsync / PostTo.  A compile error raises
    SwrError(SWR_ERR_INVALID_ARG) with the log, which names the text's lines as post.hip:LINE:."""

    def __init__(self, device: Device, source: str, constants=None):
        self._dev = device
        self._id = None
        pid = C.c_int(0)
        device._ck(device._lib.swr_post_create(device._ctx, source.encode(), C.byref(pid)))
        self._id = pid.value
        if constants is not None:
            self.SetConstants(constants)

    def SetConstants(self, values):
        """Up to 64 floats the program reads as env.constants[i] (the rest read 0); each present captures them when it is called."""
        a = _f32(values if values is not None else [], None)
        self._dev._ck(self._dev._lib.swr_post_set_constants(self._dev._ctx, self._id, _fptr(a) if a.size else None, int(a.size)))

    def SetTexture(self, slot: int, texture: Optional["Texture"]):
        """Bind a Texture of this Device to slot 0 .. 3 (None unbinds): the program reads it with swr_post_sample / swr_post_texel.
        Each present captures the four slots, and each texture's filter, when it is called."""
        self._dev._ck(self._dev._lib.swr_post_set_texture(self._dev._ctx, self._id, int(slot), texture._h if texture is not None else None))

    def close(self):
        """swr_post_destroy: a present already enqueued with the program still completes."""
        if self._id is not None and self._dev._ctx:
            self._dev._ck(self._dev._lib.swr_post_destroy(self._dev._ctx, self._id))
        self._id = None

    Dispose = close


class Texture:
    """Texture(Image<Rgba32>), Texture.cs:31-68: RGBA8 pixels, nearest sampling with wrap."""

    def __init__(self, device: Device, pixels_rgba8: np.ndarray):
        px = np.ascontiguousarray(pixels_rgba8, dtype=np.uint8)
        if px.ndim != 3 or px.shape[2] != 4:
            raise ValueError("pixels must be (height, width, 4) uint8")
        self._dev = device
        self.Height, self.Width = int(px.shape[0]), int(px.shape[1])
        self._h = C.c_void_p()
        device._ck(device._lib.swr_texture_create(device._ctx, px.ctypes.data, self.Width, self.Height, C.byref(self._h)))

    @classmethod
    def Target(cls, device: Device, width: int, height: int) -> "Texture":
        """A texture of zeros without host data (swr_texture_create_target), to be filled by UpdateFrom."""
        t = cls.__new__(cls)
        t._dev = device
        t.Height, t.Width = int(height), int(width)
        t._h = C.c_void_p()
        device._ck(device._lib.swr_texture_create_target(device._ctx, t.Width, t.Height, C.byref(t._h)))
        return t

    def UpdateFrom(self, window: "MainWindow", kx: int = 1, ky: int = 1, keep_alpha: bool = False):
        """Render to texture (swr_texture_update_from_frame; build-defined, the reference has no such link): the texels become the
        window's frame, box-filtered by kx x ky and quantised as the 8-bit present; alpha 255, or the frame's with keep_alpha.  The
        window measures Width * kx by Height * ky and may belong to this texture's Device or to another Device on the same GPU.
        Immediate-mode semantics and no wait for the GPU: draws recorded earlier sample the old texels, later ones the new."""
        window._activate()
        src = window._dev._ctx if window._dev is not self._dev else None
        self._dev._ck(self._dev._lib.swr_texture_update_from_frame(
            self._dev._ctx, self._h, src, int(kx), int(ky), N.SWR_TEXTURE_ALPHA_KEEP if keep_alpha else N.SWR_TEXTURE_ALPHA_OPAQUE))

    def UpdateFromPost(self, window: "MainWindow", post: PostProgram, kx: int = 1, ky: int = 1, keep_alpha: bool = False):
        """A pass's result into the texture (swr_texture_update_from_post): UpdateFrom with `post`, a program of the window's Device,
        between the resolve and the quantiser; alpha 255, or the quantised w of the program's result with keep_alpha.  The texture
        may not be bound to a slot of `post`.  A chain of passes is a sequence of calls: pass 1 writes A, pass 2 samples A."""
        window._activate()
        src = window._dev._ctx if window._dev is not self._dev else None
        self._dev._ck(self._dev._lib.swr_texture_update_from_post(
            self._dev._ctx, self._h, src, post._id, int(kx), int(ky), N.SWR_TEXTURE_ALPHA_KEEP if keep_alpha else N.SWR_TEXTURE_ALPHA_OPAQUE))

    @classmethod
    def Depth(cls, device: Device, width: int, height: int, depth: Optional[np.ndarray] = None) -> "Texture":
        """A depth texture (swr_texture_create_depth; build-defined): float32 depth words as the raster stage stores them, `depth`
        of shape (height, width) or, without it, float.MinValue everywhere -- nothing drawn.  Filled by UpdateFromDepth, read in
        programs through swr_shadow / swr_sample_depth / swr_texel_depth; SetBilinear switches swr_shadow to its 2 x 2 form."""
        t = cls.__new__(cls)
        t._dev = device
        t.Height, t.Width = int(height), int(width)
        t._h = C.c_void_p()
        words = None
        if depth is not None:
            words = np.ascontiguousarray(depth, dtype=np.float32)
            if words.shape != (t.Height, t.Width):
                raise ValueError("depth must be (height, width) float32")
        device._ck(device._lib.swr_texture_create_depth(device._ctx, words.ctypes.data if words is not None else None, t.Width, t.Height, C.byref(t._h)))
        return t

    @property
    def Format(self) -> int:
        """SWR_TEXTURE_FORMAT_RGBA8 (0) or SWR_TEXTURE_FORMAT_DEPTH32F (1) (swr_texture_format)."""
        f = C.c_int(-1)
        self._dev._ck(self._dev._lib.swr_texture_format(self._dev._ctx, self._h, C.byref(f)))
        return f.value

    def UpdateFromDepth(self, window: "MainWindow", kx: int = 1, ky: int = 1, reduce: int = DepthReduce.Max):
        """A frame's depth into this depth texture (swr_texture_update_from_depth): each texel becomes one word of its kx x ky block
        of the window's depth plane -- the nearest (Max, under the default LessEqual test), the farthest (Min) or the top-left one
        (First).  The window measures Width * kx by Height * ky; otherwise UpdateFrom's contract: immediate-mode order, no wait for
        the GPU, the window of this Device or of another on the same GPU."""
        window._activate()
        src = window._dev._ctx if window._dev is not self._dev else None
        self._dev._ck(self._dev._lib.swr_texture_update_from_depth(self._dev._ctx, self._h, src, int(kx), int(ky), int(reduce)))

    def ReadDepth(self) -> np.ndarray:
        """The depth words as (Height, Width) float32 (swr_texture_readback_depth); waits for the GPU."""
        out = np.empty((self.Height, self.Width), dtype=np.float32)
        self._dev._ck(self._dev._lib.swr_texture_readback_depth(self._dev._ctx, self._h, out.ctypes.data))
        return out

    def SampleDepth(self, uv, ref) -> tuple:
        """The device lookups of a depth texture with its filter as it is now (swr_texture_sample_depth), batched: uv of shape
        (..., 2) and ref of shape (...) -> (depth, shadow), each of shape (...).  depth: the word of the texel Texture.Sample's
        addressing picks.  shadow: 1 where ref >= the stored depth, one texel (nearest) or the 2 x 2 footprint blended (bilinear)."""
        a = np.ascontiguousarray(np.asarray(uv, dtype=np.float32))
        r = np.broadcast_to(np.asarray(ref, dtype=np.float32), a.shape[:-1])
        flat = np.ascontiguousarray(np.concatenate([a.reshape(-1, 2), r.reshape(-1, 1)], axis=1))
        out = np.empty((flat.shape[0], 2), dtype=np.float32)
        self._dev._ck(self._dev._lib.swr_texture_sample_depth(self._dev._ctx, self._h, flat.ctypes.data, flat.shape[0], out.ctypes.data))
        return out[:, 0].reshape(a.shape[:-1]), out[:, 1].reshape(a.shape[:-1])

    def Read(self) -> np.ndarray:
        """The texels as (Height, Width, 4) uint8 (swr_texture_readback); waits for the GPU."""
        out = np.empty((self.Height, self.Width, 4), dtype=np.uint8)
        self._dev._ck(self._dev._lib.swr_texture_readback(self._dev._ctx, self._h, out.ctypes.data))
        return out

    def Sample(self, uv) -> np.ndarray:
        """Texture.Sample, Texture.cs:43-63 (batched: uv of shape (..., 2) -> (..., 4)); runs on the GPU."""
        a = np.ascontiguousarray(np.asarray(uv, dtype=np.float32))
        flat = a.reshape(-1, 2)
        out = np.empty((flat.shape[0], 4), dtype=np.float32)
        self._dev._ck(self._dev._lib.swr_texture_sample(self._dev._ctx, self._h, flat.ctypes.data, flat.shape[0], out.ctypes.data))
        return out.reshape(a.shape[:-1] + (4,))

    def GenerateMipmaps(self):
        """Build-defined (the reference's Texture is one level): give the texture its mip chain, or regenerate it
        (swr_texture_generate_mipmaps).  L = 1 + floor(log2(max(Width, Height))) levels, each a 2 x 2 box filter of the one before,
        per byte, rounding half up.  UpdateFrom's order and no wait for the GPU: draws recorded earlier see the old levels, later ones
        the new.  From then on UpdateFrom / UpdateFromPost regenerate the chain in the same call.  Programs read it through
        swr_sample_lod / swr_sample_grad / swr_sample_level; Texture.Sample and the built-in programs stay on level 0."""
        self._dev._ck(self._dev._lib.swr_texture_generate_mipmaps(self._dev._ctx, self._h))

    @property
    def Levels(self) -> int:
        """1, or L once GenerateMipmaps has run (swr_texture_levels)."""
        n = C.c_int(-1)
        self._dev._ck(self._dev._lib.swr_texture_levels(self._dev._ctx, self._h, C.byref(n)))
        return n.value

    def LevelSize(self, level: int) -> tuple:
        """(width, height) of a level of the full chain, generated or not (swr_texture_level_size)."""
        w, h = C.c_int(-1), C.c_int(-1)
        self._dev._ck(self._dev._lib.swr_texture_level_size(self._dev._ctx, self._h, int(level), C.byref(w), C.byref(h)))
        return w.value, h.value

    def ReadLevel(self, level: int) -> np.ndarray:
        """The texels of a level the texture has as (h_l, w_l, 4) uint8 (swr_texture_readback_level); waits for the GPU."""
        w, h = self.LevelSize(level)
        out = np.empty((h, w, 4), dtype=np.uint8)
        self._dev._ck(self._dev._lib.swr_texture_readback_level(self._dev._ctx, self._h, int(level), out.ctypes.data))
        return out

    def SampleLod(self, uv, lod) -> np.ndarray:
        """swr_sample_lod as a program computes it, with the texture's filter as it is now (swr_texture_sample_lod), batched: uv of
        shape (..., 2) and lod of shape (...) -> (..., 4); runs on the GPU."""
        a = np.ascontiguousarray(np.asarray(uv, dtype=np.float32))
        l = np.broadcast_to(np.asarray(lod, dtype=np.float32), a.shape[:-1])
        flat = np.ascontiguousarray(np.concatenate([a.reshape(-1, 2), l.reshape(-1, 1)], axis=1))
        out = np.empty((flat.shape[0], 4), dtype=np.float32)
        self._dev._ck(self._dev._lib.swr_texture_sample_lod(self._dev._ctx, self._h, flat.ctypes.data, flat.shape[0], out.ctypes.data))
        return out.reshape(a.shape[:-1] + (4,))

    def Lod(self, grads) -> np.ndarray:
        """swr_lod as a program computes it (swr_texture_lod), batched: grads of shape (..., 4) = (dudx, dvdx, dudy, dvdy) -> (...);
        runs on the GPU."""
        a = np.ascontiguousarray(np.asarray(grads, dtype=np.float32))
        flat = a.reshape(-1, 4)
        out = np.empty((flat.shape[0],), dtype=np.float32)
        self._dev._ck(self._dev._lib.swr_texture_lod(self._dev._ctx, self._h, flat.ctypes.data, flat.shape[0], out.ctypes.data))
        return out.reshape(a.shape[:-1])

    # ---- cube maps (build-defined; include/swr.h): a cube of side n is a texture n wide and 6 n high, face f
    # (0..5 = +X, -X, +Y, -Y, +Z, -Z) in rows [f n, (f + 1) n); every other method sees that atlas
    @classmethod
    def _cube(cls, device: Device, n: int, data, depth: bool) -> "Texture":
        t = cls.__new__(cls)
        t._dev = device
        t.Width, t.Height = int(n), 6 * int(n)
        t._h = C.c_void_p()
        fn = device._lib.swr_texture_create_cube_depth if depth else device._lib.swr_texture_create_cube
        device._ck(fn(device._ctx, data.ctypes.data if data is not None else None, int(n), C.byref(t._h)))
        return t

    @classmethod
    def Cube(cls, device: Device, faces) -> "Texture":
        """A cube map from six faces (swr_texture_create_cube): `faces` of shape (6, n, n, 4) uint8, in the order +X, -X, +Y, -Y,
        +Z, -Z, each as a camera along that axis sees it (hostmath.cube_face_view).  Read in programs through swr_sample_cube."""
        px = np.ascontiguousarray(faces, dtype=np.uint8)
        if px.ndim != 4 or px.shape[0] != 6 or px.shape[1] != px.shape[2] or px.shape[3] != 4 or px.shape[1] < 1:
            raise ValueError("faces must be (6, n, n, 4) uint8")
        return cls._cube(device, px.shape[1], px, False)

    @classmethod
    def CubeTarget(cls, device: Device, n: int) -> "Texture":
        """A cube map of zeros without host data, to be filled face by face by UpdateFaceFrom / UpdateFaceFromPost."""
        return cls._cube(device, n, None, False)

    @classmethod
    def CubeDepth(cls, device: Device, n: int, words=None) -> "Texture":
        """A depth cube map (swr_texture_create_cube_depth): `words` of shape (6, n, n) float32 or, without it, float.MinValue
        everywhere.  Filled by UpdateFaceFromDepth, read in programs through swr_shadow_cube / swr_sample_cube_depth."""
        w = None
        if words is not None:
            w = np.ascontiguousarray(words, dtype=np.float32)
            if w.shape != (6, int(n), int(n)):
                raise ValueError("words must be (6, n, n) float32")
        return cls._cube(device, n, w, True)

    @property
    def IsCube(self) -> int:
        """n of a cube map, 0 of any other texture (swr_texture_is_cube)."""
        n = C.c_int(-1)
        self._dev._ck(self._dev._lib.swr_texture_is_cube(self._dev._ctx, self._h, C.byref(n)))
        return n.value

    @staticmethod
    def _face(face) -> int:
        f = int(face)
        if not 0 <= f <= 5:
            raise ValueError("face must be 0 .. 5 (+X, -X, +Y, -Y, +Z, -Z)")
        return f

    def UpdateFaceFrom(self, face: int, window: "MainWindow", kx: int = 1, ky: int = 1, keep_alpha: bool = False):
        """UpdateFrom into one face of a cube map (swr_texture_update_face_from_frame): the window measures n * kx by n * ky.  The
        same kernel, order and contract; a cube with a mip chain has it regenerated in the same call."""
        face = self._face(face)
        window._activate()
        src = window._dev._ctx if window._dev is not self._dev else None
        self._dev._ck(self._dev._lib.swr_texture_update_face_from_frame(
            self._dev._ctx, self._h, face, src, int(kx), int(ky), N.SWR_TEXTURE_ALPHA_KEEP if keep_alpha else N.SWR_TEXTURE_ALPHA_OPAQUE))

    def UpdateFaceFromDepth(self, face: int, window: "MainWindow", kx: int = 1, ky: int = 1, reduce: int = DepthReduce.Max):
        """UpdateFromDepth into one face of a depth cube map (swr_texture_update_face_from_depth)."""
        face = self._face(face)
        window._activate()
        src = window._dev._ctx if window._dev is not self._dev else None
        self._dev._ck(self._dev._lib.swr_texture_update_face_from_depth(self._dev._ctx, self._h, face, src, int(kx), int(ky), int(reduce)))

    def UpdateFaceFromPost(self, face: int, window: "MainWindow", post: PostProgram, kx: int = 1, ky: int = 1, keep_alpha: bool = False):
        """UpdateFromPost into one face of a cube map (swr_texture_update_face_from_post)."""
        face = self._face(face)
        window._activate()
        src = window._dev._ctx if window._dev is not self._dev else None
        self._dev._ck(self._dev._lib.swr_texture_update_face_from_post(
            self._dev._ctx, self._h, face, src, post._id, int(kx), int(ky), N.SWR_TEXTURE_ALPHA_KEEP if keep_alpha else N.SWR_TEXTURE_ALPHA_OPAQUE))

    def ReadFace(self, face: int, level: int = 0) -> np.ndarray:
        """One face of a level the cube has (swr_texture_readback_face): (n_l, n_l, 4) uint8, or (n, n) float32 depth words;
        waits for the GPU."""
        face = self._face(face)
        if not 0 <= int(level) < 32 or (self.Width >> int(level)) < 1:
            raise ValueError("the level is outside the cube's chain")
        n = self.Width >> int(level)
        out = np.empty((n, n), dtype=np.float32) if self.Format == N.SWR_TEXTURE_FORMAT_DEPTH32F else np.empty((n, n, 4), dtype=np.uint8)
        self._dev._ck(self._dev._lib.swr_texture_readback_face(self._dev._ctx, self._h, face, int(level), out.ctypes.data))
        return out

    @staticmethod
    def _dirs4(dirs, last) -> tuple:
        a = np.asarray(dirs, dtype=np.float32)
        if a.ndim < 1 or a.shape[-1] != 3:
            raise ValueError("directions must have shape (..., 3)")
        l = np.broadcast_to(np.asarray(last, dtype=np.float32), a.shape[:-1])
        return a.shape[:-1], np.ascontiguousarray(np.concatenate([a.reshape(-1, 3), l.reshape(-1, 1)], axis=1))

    def SampleCube(self, dirs, lod=0.0) -> np.ndarray:
        """swr_sample_cube_lod as a program computes it, with the texture's filter as it is now (swr_texture_sample_cube), batched:
        dirs of shape (..., 3) and lod of shape (...) -> (..., 4); lod 0 is swr_sample_cube; runs on the GPU."""
        shape, flat = self._dirs4(dirs, lod)
        out = np.empty((flat.shape[0], 4), dtype=np.float32)
        self._dev._ck(self._dev._lib.swr_texture_sample_cube(self._dev._ctx, self._h, flat.ctypes.data, flat.shape[0], out.ctypes.data))
        return out.reshape(shape + (4,))

    def SampleCubeDepth(self, dirs, ref) -> tuple:
        """swr_sample_cube_depth and swr_shadow_cube of a depth cube (swr_texture_sample_cube_depth), batched: dirs of shape
        (..., 3) and ref of shape (...) -> (depth, shadow), each of shape (...)."""
        shape, flat = self._dirs4(dirs, ref)
        out = np.empty((flat.shape[0], 2), dtype=np.float32)
        self._dev._ck(self._dev._lib.swr_texture_sample_cube_depth(self._dev._ctx, self._h, flat.ctypes.data, flat.shape[0], out.ctypes.data))
        return out[:, 0].reshape(shape), out[:, 1].reshape(shape)

    @staticmethod
    def CubeFace(device: Device, dirs) -> tuple:
        """swr_cube_face as a program computes it (swr_texture_cube_face), batched: dirs of shape (..., 3) -> (face of shape (...)
        int32, st of shape (..., 2)); runs on the GPU."""
        a = np.asarray(dirs, dtype=np.float32)
        if a.ndim < 1 or a.shape[-1] != 3:
            raise ValueError("directions must have shape (..., 3)")
        flat = np.ascontiguousarray(a.reshape(-1, 3))
        face = np.empty((flat.shape[0],), dtype=np.int32)
        st = np.empty((flat.shape[0], 2), dtype=np.float32)
        device._ck(device._lib.swr_texture_cube_face(device._ctx, flat.ctypes.data, flat.shape[0], face.ctypes.data, st.ctypes.data))
        return face.reshape(a.shape[:-1]), st.reshape(a.shape[:-1] + (2,))

    def SetBilinear(self, on: bool):
        """Build-defined extension (the reference samples nearest): bilinear filter with wrap for later draws."""
        self._dev._ck(self._dev._lib.swr_texture_set_filter(self._dev._ctx, self._h, 1 if on else 0))

    def Dispose(self):
        if self._h:
            self._dev._ck(self._dev._lib.swr_texture_destroy(self._dev._ctx, self._h))
            self._h = C.c_void_p()


class VertexShader:
    def __init__(self, program: "ShaderProgram"):
        self.program = program


class FragmentShader:
    def __init__(self, program: "ShaderProgram"):
        self.program = program


class ShaderProgram:
    """Stands in for the reference's (VertexShader, FragmentShader) delegate pair (Shaders.cs:97-98)."""

    def __init__(self, program: Program, uniforms: Optional[N.Uniforms] = None, texture: Optional[Texture] = None):
        # a built-in Program, or the id of a user fragment program (Device.compile_program, >= SWR_PROG_USER_BASE)
        self.program = Program(program) if int(program) < N.SWR_PROG_USER_BASE else int(program)
        self.uniforms = uniforms if uniforms is not None else default_uniforms()
        self.texture = texture
        self.VertexShader = VertexShader(self)
        self.FragmentShader = FragmentShader(self)

    def _program_for(self, dev: "Device") -> int:
        return int(self.program)


class CustomProgram(ShaderProgram):
    """A user program given as source (Shaders.Custom): the fragment half and, optionally, the vertex half; compiled once per Device
    on first use; `constants` (up to 64 floats, the fields the C# closures capture, read by both halves) and `textures` (up to three
    Textures or None for slots 1 .. 3, the closures' further Texture fields; `texture` is slot 0) are set before every draw, so each
    draw renders with what it was given."""

    def __init__(self, source: str, uniforms: Optional[N.Uniforms] = None, texture: Optional[Texture] = None, constants=None,
                 vertex_source: Optional[str] = None, textures=None):
        super().__init__(Program.FlatColor, uniforms, texture)
        self.source = source
        self.vertex_source = vertex_source
        self.constants = constants
        textures = tuple(textures) if textures is not None else ()
        if len(textures) > N.SWR_PROGRAM_TEXTURES - 1:
            raise ValueError("a user program owns three texture slots (1 .. 3); slot 0 is `texture`")
        self.textures = textures
        self._ids = {}          # id(Device) -> (Device, program id)

    def _program_for(self, dev: "Device") -> int:
        hit = self._ids.get(id(dev))
        if hit is None or hit[0] is not dev:
            hit = (dev, dev.compile_program(self.source, self.vertex_source))
            self._ids[id(dev)] = hit
        pid = hit[1]
        dev.set_program_constants(pid, self.constants)
        for k in range(N.SWR_PROGRAM_TEXTURES - 1):
            dev.set_program_texture(pid, k + 1, self.textures[k] if k < len(self.textures) else None)
        return pid


class Shaders:
    VertexInput = VERTEX_DTYPE      # Shaders.cs:10-24
    Program = Program

    @staticmethod
    def FlatColor():
        return ShaderProgram(Program.FlatColor)

    @staticmethod
    def Gouraud():
        return ShaderProgram(Program.Gouraud)

    @staticmethod
    def Dust2LambertFog(uniforms=None, texture=None):     # Renderer.cs:830-860
        return ShaderProgram(Program.Dust2LambertFog, uniforms, texture)

    @staticmethod
    def DebugVaryings():
        return ShaderProgram(Program.DebugVaryings)

    @staticmethod
    def Phong4Point(uniforms, texture=None):
        return ShaderProgram(Program.Phong4Point, uniforms, texture)

    @staticmethod
    def Custom(source: str, uniforms=None, texture=None, constants=None, vertex_source=None, textures=None):
        """Any Shaders.FragmentShader -- with `vertex_source`, any (Shaders.VertexShader, Shaders.FragmentShader) pair -- restated in
        C++ against the contract of include/swr.h (swr_program_create_vf).  `textures`: slots 1 .. 3 (swr_program_set_texture)."""
        return CustomProgram(source, uniforms, texture, constants, vertex_source, textures)


class MainWindow:
    """Framebuffer part of MainWindow (MainWindow.cs:25-31,378-436); buffers live in HBM."""

    def __init__(self, device: Device, render_width: int = 800, render_height: int = 600):
        self._dev = device
        self.RenderWidth = 0
        self.RenderHeight = 0
        self._band = None
        self._bound = None
        self.Resize(render_width, render_height)

    def _activate(self):
        """A context owns ONE framebuffer (one MainWindow in the reference).  Several MainWindow objects on one Device
        take turns: the one being used re-applies its geometry first; its previous pixels are then undefined.  The window that
        is already active issues only the call for what changed (BindFramebuffer -> swr_bind_framebuffer alone: no flush-and-wait,
        fragment counters keep accumulating); the C side also ignores a resize / band that changes nothing."""
        if getattr(self._dev, "_active_window", None) is self:
            return
        self._apply_size()
        self._apply_band()
        self._apply_binding()
        self._dev._active_window = self

    def _apply_size(self):
        self._dev._ck(self._dev._lib.swr_resize(self._dev._ctx, self.RenderWidth, self.RenderHeight))

    def _apply_band(self):
        lib, ctx = self._dev._lib, self._dev._ctx
        if self._band is not None and len(self._band) == 3:
            self._dev._ck(lib.swr_set_band_interleaved(ctx, *self._band))
        else:
            b = self._band if self._band is not None else (-1, -1)
            self._dev._ck(lib.swr_set_band(ctx, b[0], b[1]))

    def _apply_binding(self):
        cb = self._bound if self._bound is not None else (None, None)
        self._dev._ck(self._dev._lib.swr_bind_framebuffer(self._dev._ctx, C.c_void_p(cb[0]) if cb[0] else None,
                                                          C.c_void_p(cb[1]) if cb[1] else None))

    def _is_active(self):
        return getattr(self._dev, "_active_window", None) is self

    def Resize(self, width: int, height: int):          # HandleResize, MainWindow.cs:320-321
        self.RenderWidth, self.RenderHeight = int(width), int(height)
        if self._is_active():
            self._apply_size()
        else:
            self._activate()

    def SetBand(self, first_tile_row: int, n_tile_rows: int):
        self._band = (int(first_tile_row), int(n_tile_rows)) if first_tile_row >= 0 and n_tile_rows >= 0 else None
        if self._is_active():
            self._apply_band()
        else:
            self._activate()

    def SetBandInterleaved(self, rank: int, world: int, stripe_tile_rows: int):
        """Interleaved stripes instead of one contiguous band: stripe s (stripe_tile_rows tile rows) belongs to rank s % world;
        the window then holds this rank's stripes one after the other (multigpu.stripe_rows gives their frame rows)."""
        self._band = (int(rank), int(world), int(stripe_tile_rows))
        if self._is_active():
            self._apply_band()
        else:
            self._activate()

    def band_pixel_rows(self):
        tiles_y = (self.RenderHeight + 15) // 16
        if self._band is None:
            return 0, max(self.RenderHeight, 0)
        if len(self._band) == 3:
            from . import multigpu
            return 0, len(multigpu.stripe_rows(self.RenderHeight, self._band[1], self._band[2])[self._band[0]])
        t0 = min(max(self._band[0], 0), tiles_y)
        t1 = min(t0 + max(self._band[1], 0), tiles_y)
        y0, y1 = t0 * 16, min(self.RenderHeight, t1 * 16)
        return y0, max(0, y1 - y0)

    def BindFramebuffer(self, color_ptr: int, depth_ptr: int):
        """swr_bind_framebuffer: does not wait for the GPU.  Buffers bound earlier stay referenced until the next validating call
        (Device.sync / read-back / stats): see the lifetime rule in include/swr.h."""
        self._bound = (int(color_ptr), int(depth_ptr)) if color_ptr and depth_ptr else None
        if self._is_active():
            self._apply_binding()
        else:
            self._activate()

    def ClearColorBuffer(self, clear_color):             # MainWindow.cs:400-407
        self._activate()
        c = _f32(clear_color, 4)
        self._dev._ck(self._dev._lib.swr_clear_color(self._dev._ctx, _fptr(c)))

    def ClearDepthBuffer(self):                          # MainWindow.cs:429-436
        self._activate()
        self._dev._ck(self._dev._lib.swr_clear_depth(self._dev._ctx))

    def _read(self, want_color=True, want_depth=True):
        self._activate()
        _, rows = self.band_pixel_rows()
        w = max(self.RenderWidth, 0)
        col = np.empty((rows, w, 4), dtype=np.float32) if want_color else None
        dep = np.empty((rows, w), dtype=np.float32) if want_depth else None
        self._dev._ck(self._dev._lib.swr_readback(self._dev._ctx, col.ctypes.data if want_color else None,
                                                  dep.ctypes.data if want_depth else None))
        return col, dep

    @property
    def ColorBuffer(self) -> np.ndarray:                 # Vector4[W*H], idx = y*W + x
        return self._read(True, False)[0]

    @property
    def DepthBuffer(self) -> np.ndarray:
        return self._read(False, True)[1]

    def _payload_out(self, shape, dtype, out, allow_none=True):
        """The array a present or read-back fills: `out` held to the payload's shape and dtype, or a new one; makes the window current."""
        if out is None and allow_none:
            out = np.empty(shape, dtype=dtype)
        elif out.shape != shape or out.dtype != dtype or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        self._activate()
        return out

    def FlatColorBuffer(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The Vector3[] `flatColorBuffer` of MainWindow.OnRender (MainWindow.cs:234-240), flattened on the GPU.
        `out`: a caller-owned (rows, W, 3) float32 array to fill -- page-lock it once with Device.pin() and the copy runs
        at PCIe rate."""
        out = self._payload_out((self.band_pixel_rows()[1], max(self.RenderWidth, 0), 3), np.float32, out)
        if out.size:
            self._dev._ck(self._dev._lib.swr_readback_rgb(self._dev._ctx, out.ctypes.data))
        return out

    def PresentAsync(self, out: np.ndarray) -> int:
        """Asynchronous FlatColorBuffer (swr_present_rgb_async): flatten on the GPU behind the recorded draws, copy into `out`
        (page-lock it with Device.pin()) on the context's copy stream, return a ticket at once.  The next frame renders while this
        one crosses PCIe; `out` must stay untouched until PresentWait(ticket)."""
        out = self._payload_out((self.band_pixel_rows()[1], max(self.RenderWidth, 0), 3), np.float32, out, allow_none=False)
        t = C.c_uint64(0)
        self._dev._ck(self._dev._lib.swr_present_rgb_async(self._dev._ctx, C.c_void_p(out.ctypes.data), C.byref(t)))
        return int(t.value)

    def PresentWait(self, ticket: int) -> bool:
        """Blocks until the present `ticket` has landed in its array.  True = the array holds the frame; False = a batch was replayed
        meanwhile (SWR_STALE: only while the pair buffers are still growing), present that frame again."""
        rc = self._dev._lib.swr_present_wait(self._dev._ctx, C.c_uint64(ticket))
        if rc == N.SWR_STALE:
            return False
        self._dev._ck(rc)
        return True

    def FlattenTo(self, device_ptr: int):
        """FlatColorBuffer into caller-owned DEVICE memory (band rows x W x 3 floats); completes with Device.sync()."""
        self._activate()
        self._dev._ck(self._dev._lib.swr_flatten_rgb_device(self._dev._ctx, C.c_void_p(device_ptr)))

    def FlattenToAsync(self, device_ptr: int):
        """FlattenTo without the validation sync (swr_flatten_rgb_device_async): for frame loops that chain render -> flatten
        -> gather in stream order and validate later with Device.sync() + Device.replay_count()."""
        self._activate()
        self._dev._ck(self._dev._lib.swr_flatten_rgb_device_async(self._dev._ctx, C.c_void_p(device_ptr)))

    def ResolvedSize(self, kx: int, ky: int) -> tuple:
        """(rows, width) of the supersampled present's payload: band rows / ky and W / kx, the arithmetic of swr_resolved_size
        restated on the host (as FlatColorBuffer's shape is).  kx, ky in {1, 2, 4, 8}; the window's width must be a multiple of kx
        and its height of ky -- then every band's and stripe's rows are a multiple of ky."""
        if kx not in (1, 2, 4, 8) or ky not in (1, 2, 4, 8):
            raise ValueError("resolve factors must be 1, 2, 4 or 8")
        w, h = self.RenderWidth, self.RenderHeight
        if w <= 0 or h <= 0:
            return 0, 0
        if w % kx or h % ky:
            raise ValueError(f"a {w} x {h} window does not divide by the resolve factors ({kx}, {ky})")
        return self.band_pixel_rows()[1] // ky, w // kx

    def _resolved_out(self, kx, ky, out):
        return self._payload_out(self.ResolvedSize(kx, ky) + (3,), np.float32, out)

    def ResolvedColorBuffer(self, kx: int, ky: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """FlatColorBuffer of a window rendered at kx x ky times its size: every kx x ky block of the band box-filtered on the GPU
        (swr_readback_rgb_resolved; the arithmetic is in include/swr.h), (rows / ky, W / kx, 3) floats."""
        out = self._resolved_out(kx, ky, out)
        if out.size:
            self._dev._ck(self._dev._lib.swr_readback_rgb_resolved(self._dev._ctx, int(kx), int(ky), out.ctypes.data))
        return out

    def PresentResolvedAsync(self, out: np.ndarray, kx: int, ky: int) -> int:
        """PresentAsync with the resolved payload (swr_present_rgb_resolved_async): 1 / (kx * ky) of the bytes cross PCIe.  Shares
        PresentAsync's two slots; PresentWait serves the ticket."""
        out = self._resolved_out(kx, ky, out)
        t = C.c_uint64(0)
        self._dev._ck(self._dev._lib.swr_present_rgb_resolved_async(self._dev._ctx, int(kx), int(ky), C.c_void_p(out.ctypes.data), C.byref(t)))
        return int(t.value)

    def ResolveTo(self, device_ptr: int, kx: int, ky: int):
        """ResolvedColorBuffer into caller-owned DEVICE memory (ResolvedSize x 3 floats); completes with Device.sync()."""
        self._activate()
        self._dev._ck(self._dev._lib.swr_resolve_rgb_device(self._dev._ctx, int(kx), int(ky), C.c_void_p(device_ptr)))

    def ResolveToAsync(self, device_ptr: int, kx: int, ky: int):
        """ResolveTo without the validation sync (swr_resolve_rgb_device_async), as FlattenToAsync."""
        self._activate()
        self._dev._ck(self._dev._lib.swr_resolve_rgb_device_async(self._dev._ctx, int(kx), int(ky), C.c_void_p(device_ptr)))

    def Present8Size(self, kx: int = 1, ky: int = 1, channels: int = 3) -> tuple:
        """(rows, width, channels) of the 8-bit present's payload (swr_present8_size restated on the host): ResolvedSize, and 3
        (R, G, B) or 4 (R, G, B, 255) bytes per pixel, rows tightly packed."""
        if channels not in (3, 4):
            raise ValueError("channels must be 3 (RGB8) or 4 (RGBX8)")
        return self.ResolvedSize(kx, ky) + (channels,)

    def _present8_out(self, kx, ky, channels, out):
        return self._payload_out(self.Present8Size(kx, ky, channels), np.uint8, out)

    def ColorBuffer8(self, kx: int = 1, ky: int = 1, channels: int = 3, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The frame as the window's 8-bit framebuffer will hold it, quantised on the GPU (swr_readback_rgb8; the rule is in
        include/swr.h): FlatColorBuffer under (1, 1), ResolvedColorBuffer otherwise, clamped to [0, 1], times 255, rounded to nearest
        even; (rows / ky, W / kx, channels) uint8.  A quarter (channels = 3) or a third (channels = 4) of the float payload's bytes."""
        out = self._present8_out(kx, ky, channels, out)
        if out.size:
            self._dev._ck(self._dev._lib.swr_readback_rgb8(self._dev._ctx, int(kx), int(ky), int(channels), out.ctypes.data))
        return out

    def Present8Async(self, out: np.ndarray, kx: int = 1, ky: int = 1) -> int:
        """PresentAsync with the 8-bit payload (swr_present_rgb8_async); out.shape[-1] (3 or 4) selects the format.  Shares
        PresentAsync's two slots; PresentWait serves the ticket."""
        if getattr(out, "ndim", 0) != 3:
            raise ValueError("out must be a uint8 array of shape (rows, width, 3 or 4)")
        channels = int(out.shape[-1])
        out = self._present8_out(kx, ky, channels, out)
        t = C.c_uint64(0)
        self._dev._ck(self._dev._lib.swr_present_rgb8_async(self._dev._ctx, int(kx), int(ky), channels, C.c_void_p(out.ctypes.data), C.byref(t)))
        return int(t.value)

    def Quantise8To(self, device_ptr: int, kx: int = 1, ky: int = 1, channels: int = 3):
        """ColorBuffer8 into caller-owned DEVICE memory (Present8Size bytes, 4-byte aligned); completes with Device.sync()."""
        self._activate()
        self._dev._ck(self._dev._lib.swr_resolve_rgb8_device(self._dev._ctx, int(kx), int(ky), int(channels), C.c_void_p(device_ptr)))

    def Quantise8ToAsync(self, device_ptr: int, kx: int = 1, ky: int = 1, channels: int = 3):
        """Quantise8To without the validation sync (swr_resolve_rgb8_device_async), as FlattenToAsync."""
        self._activate()
        self._dev._ck(self._dev._lib.swr_resolve_rgb8_device_async(self._dev._ctx, int(kx), int(ky), int(channels), C.c_void_p(device_ptr)))

    @staticmethod
    def _post_format(channels, dtype) -> int:
        dt = np.dtype(dtype)
        if dt == np.float32 and channels == 3:
            return N.SWR_POST_RGB32F
        if dt == np.uint8 and channels in (3, 4):
            return N.SWR_POST_RGB8 if channels == 3 else N.SWR_POST_RGBX8
        raise ValueError("a post program delivers (3, float32), (3, uint8) or (4, uint8)")

    def PostBuffer(self, post: PostProgram, kx: int = 1, ky: int = 1, channels: int = 3, dtype=np.uint8,
                   out: Optional[np.ndarray] = None) -> np.ndarray:
        """The frame after `post` (swr_readback_post): the program runs once per pixel of the resolved frame and its result is
        delivered as ResolvedColorBuffer delivers (float32, unclamped) or as ColorBuffer8 does (uint8, 3 or 4 channels)."""
        fmt = self._post_format(channels, dtype)
        out = self._payload_out(self.ResolvedSize(kx, ky) + (channels,), np.dtype(dtype), out)
        if out.size:
            self._dev._ck(self._dev._lib.swr_readback_post(self._dev._ctx, post._id, int(kx), int(ky), fmt, out.ctypes.data))
        return out

    def PresentPostAsync(self, post: PostProgram, out: np.ndarray, kx: int = 1, ky: int = 1) -> int:
        """PresentAsync with the program's result (swr_present_post_async); out's dtype and last axis select the format.  Shares
        PresentAsync's two slots; PresentWait serves the ticket.  The program's constants are captured by this call."""
        if getattr(out, "ndim", 0) != 3:
            raise ValueError("out must be a float32 array of shape (rows, width, 3) or a uint8 one of (rows, width, 3 or 4)")
        fmt = self._post_format(int(out.shape[-1]), out.dtype)
        out = self._payload_out(self.ResolvedSize(kx, ky) + (int(out.shape[-1]),), out.dtype, out, allow_none=False)
        t = C.c_uint64(0)
        self._dev._ck(self._dev._lib.swr_present_post_async(self._dev._ctx, post._id, int(kx), int(ky), fmt, C.c_void_p(out.ctypes.data), C.byref(t)))
        return int(t.value)

    def PostTo(self, post: PostProgram, device_ptr: int, kx: int = 1, ky: int = 1, channels: int = 3, dtype=np.uint8, wait: bool = True):
        """PostBuffer into caller-owned DEVICE memory (4-byte aligned; swr_post_device); completes with Device.sync().  wait=False:
        without the validation sync (swr_post_device_async), as FlattenToAsync."""
        fmt = self._post_format(channels, dtype)
        self._activate()
        fn = self._dev._lib.swr_post_device if wait else self._dev._lib.swr_post_device_async
        self._dev._ck(fn(self._dev._ctx, post._id, int(kx), int(ky), fmt, C.c_void_p(device_ptr)))

    def Upload(self, color=None, depth=None):
        self._activate()
        c = np.ascontiguousarray(color, dtype=np.float32) if color is not None else None
        d = np.ascontiguousarray(depth, dtype=np.float32) if depth is not None else None
        self._dev._ck(self._dev._lib.swr_upload(self._dev._ctx, c.ctypes.data if c is not None else None,
                                                d.ctypes.data if d is not None else None))

    def GetPixel(self, x: int, y: int) -> np.ndarray:    # MainWindow.cs:391-398
        self._activate()
        out = np.zeros(4, dtype=np.float32)
        self._dev._ck(self._dev._lib.swr_get_pixel(self._dev._ctx, int(x), int(y), _fptr(out)))
        return out

    def SetPixel(self, x: int, y: int, color):           # MainWindow.cs:382-388
        self._activate()
        c = _f32(color, 4)
        self._dev._ck(self._dev._lib.swr_set_pixel(self._dev._ctx, int(x), int(y), _fptr(c)))

    def GetDepth(self, x: int, y: int) -> float:         # MainWindow.cs:420-426
        self._activate()
        out = C.c_float(0.0)
        self._dev._ck(self._dev._lib.swr_get_depth(self._dev._ctx, int(x), int(y), C.byref(out)))
        return float(np.float32(out.value))

    def SetDepth(self, x: int, y: int, depth: float):    # MainWindow.cs:411-417
        self._activate()
        self._dev._ck(self._dev._lib.swr_set_depth(self._dev._ctx, int(x), int(y), float(depth)))


class Mesh:
    """Retained mesh: Mesh.Vertices / Mesh.Indices (ModelLoader.cs:45-47) uploaded once."""

    def __init__(self, device: Device, vertices: np.ndarray, indices: np.ndarray):
        v = as_vertex_array(vertices)
        i = np.ascontiguousarray(indices, dtype=np.uint16).reshape(-1)
        self._dev = device
        self.n_vertices, self.n_indices = int(v.shape[0]), int(i.shape[0])
        self._h = C.c_void_p()
        device._ck(device._lib.swr_mesh_create(device._ctx, v.ctypes.data, self.n_vertices, i.ctypes.data, self.n_indices, C.byref(self._h)))

    @property
    def SphereBounds(self) -> np.ndarray:
        """Mesh.SphereBounds = FrustumCuller.CalculateBoundingSphere(vertices) (ModelLoader.cs:291): {cx, cy, cz, r}, on the GPU."""
        out = np.zeros(4, dtype=np.float32)
        self._dev._ck(self._dev._lib.swr_mesh_bounds(self._dev._ctx, self._h, _fptr(out)))
        return out

    # ---- deforming meshes (build-defined)
    def Like(self) -> "Mesh":
        """swr_mesh_create_like: a retained mesh with this one's vertices and indices, copied on the GPU -- a deform target."""
        m = Mesh.__new__(Mesh)
        m._dev, m.n_vertices, m.n_indices, m._h = self._dev, self.n_vertices, self.n_indices, C.c_void_p()
        self._dev._ck(self._dev._lib.swr_mesh_create_like(self._dev._ctx, self._h, C.byref(m._h)))
        return m

    def Read(self) -> np.ndarray:
        """swr_mesh_readback: the vertices as the device holds them (VERTEX_DTYPE); flushes nothing."""
        out = np.zeros(self.n_vertices, dtype=VERTEX_DTYPE)
        self._dev._ck(self._dev._lib.swr_mesh_readback(self._dev._ctx, self._h, out.ctypes.data))
        return out

    def BlendFrom(self, a: "Mesh", b: "Mesh", t: float) -> "Mesh":
        """swr_mesh_blend: this mesh's vertices = a * (1 - t) + b * t, every scalar, in the build's Lerp model; t is not clamped."""
        self._dev._ck(self._dev._lib.swr_mesh_blend(self._dev._ctx, self._h, a._h if a is not None else None,
                                                    b._h if b is not None else None, C.c_float(float(np.float32(t)))))
        return self

    def SetSkin(self, joints, weights) -> "Mesh":
        """swr_mesh_set_skin: four joint indices (uint16) and four weights (float32) per vertex, retained; (None, None) removes them."""
        if joints is None and weights is None:
            self._dev._ck(self._dev._lib.swr_mesh_set_skin(self._dev._ctx, self._h, None, None))
            return self
        j = np.ascontiguousarray(joints, dtype=np.uint16).reshape(-1)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if j.size != 4 * self.n_vertices or w.size != 4 * self.n_vertices:
            raise ValueError("joints and weights must hold four entries per vertex")
        self._dev._ck(self._dev._lib.swr_mesh_set_skin(self._dev._ctx, self._h, j.ctypes.data, w.ctypes.data))
        return self

    def SkinFrom(self, src: "Mesh", palette) -> "Mesh":
        """swr_mesh_skin: this mesh's vertices = src's, skinned by `palette` (n_joints x 4 x 4, row-major for row vectors: glTF's
        jointMatrix, the caller's) with src's skin attributes, under the device's Transform / TransformNormal model."""
        p = np.ascontiguousarray(palette, dtype=np.float32).reshape(-1, 16)
        self._dev._ck(self._dev._lib.swr_mesh_skin(self._dev._ctx, self._h, src._h if src is not None else None, _fptr(p), int(p.shape[0])))
        return self

    def Dispose(self):
        if self._h:
            self._dev._ck(self._dev._lib.swr_mesh_destroy(self._dev._ctx, self._h))
            self._h = C.c_void_p()


# ---- skeletal animation (build-defined; include/swr.h "SKELETAL ANIMATION")
ANIM_PATHS = {"translation": N.SWR_ANIM_PATH_TRANSLATION, "rotation": N.SWR_ANIM_PATH_ROTATION, "scale": N.SWR_ANIM_PATH_SCALE}
ANIM_INTERPOLATIONS = {"STEP": N.SWR_ANIM_STEP, "LINEAR": N.SWR_ANIM_LINEAR, "CUBICSPLINE": N.SWR_ANIM_CUBICSPLINE}
POSE_REQUEST_DTYPE = np.dtype([("clip_a", "<i4"), ("time_a", "<f4"), ("clip_b", "<i4"), ("time_b", "<f4"), ("weight", "<f4")])


class Skeleton:
    """swr_skeleton: nodes in topological order (parent[i] < i, -1 for a root) with their rest matrices and rest T / R / S, the joints
    (the node each is, its inverse bind matrix) and the clips added to it.  Matrices are 4 x 4, row-major for row vectors."""

    def __init__(self, device: Device, parent, rest_local, rest_t, rest_r, rest_s, joint_node, inverse_bind):
        self._dev = device
        par = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
        n = int(par.size)
        loc, t, r, sc = _f32(rest_local, 16 * n), _f32(rest_t, 3 * n), _f32(rest_r, 4 * n), _f32(rest_s, 3 * n)
        jn = np.ascontiguousarray(joint_node, dtype=np.int32).reshape(-1)
        ib = _f32(inverse_bind, 16 * int(jn.size))
        self.n_nodes, self.n_joints, self.n_clips = n, int(jn.size), 0
        self._h = C.c_void_p()
        device._ck(device._lib.swr_skeleton_create(device._ctx, n, par.ctypes.data, loc.ctypes.data, t.ctypes.data, r.ctypes.data, sc.ctypes.data,
                                                   self.n_joints, jn.ctypes.data, ib.ctypes.data, C.byref(self._h)))

    def AddClip(self, channels) -> int:
        """swr_skeleton_add_clip: `channels` is a sequence of (node, path, interpolation, times, values) -- path one of "translation",
        "rotation", "scale" (or SWR_ANIM_PATH_*), interpolation "STEP" or "LINEAR" (or SWR_ANIM_*), times n_keys floats, values
        n_keys x 3 (x 4 for a rotation, xyzw).  Returns the clip's index.  A load-time call: it may wait for the device."""
        keep, recs = [], (N.AnimChannel * max(len(channels), 1))()
        for k, (node, path, interp, times, values) in enumerate(channels):
            path = ANIM_PATHS.get(path, path) if isinstance(path, str) else int(path)
            interp = ANIM_INTERPOLATIONS.get(interp, interp) if isinstance(interp, str) else int(interp)
            if isinstance(path, str) or isinstance(interp, str):
                raise ValueError(f"unknown animation path or interpolation: {path!r}, {interp!r}")
            tm = np.ascontiguousarray(times, dtype=np.float32).reshape(-1)
            va = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
            if va.size != tm.size * (4 if path == N.SWR_ANIM_PATH_ROTATION else 3):
                raise ValueError("a channel's values must hold 3 floats per key (4 for a rotation)")
            keep += [tm, va]
            recs[k] = N.AnimChannel(int(node), path, interp, int(tm.size), tm.ctypes.data, va.ctypes.data)
        idx = C.c_int(-1)
        self._dev._ck(self._dev._lib.swr_skeleton_add_clip(self._dev._ctx, self._h, recs, len(channels), C.byref(idx)))
        self.n_clips = idx.value + 1
        return idx.value

    def Dispose(self):
        if self._h:
            self._dev._ck(self._dev._lib.swr_skeleton_destroy(self._dev._ctx, self._h))
            self._h = C.c_void_p()


class PoseSet:
    """swr_pose_set: n_instances x n_joints joint matrices on the device -- sampled from a skeleton's clips on the GPU (Sample) or made
    on the host (Upload) -- that Device.SkinBatch skins a crowd from."""

    def __init__(self, device: Device, n_instances: int, n_joints: int):
        self._dev, self.n_instances, self.n_joints = device, int(n_instances), int(n_joints)
        self._h = C.c_void_p()
        device._ck(device._lib.swr_pose_set_create(device._ctx, self.n_instances, self.n_joints, C.byref(self._h)))

    @staticmethod
    def Requests(clip_a, time_a, clip_b=-1, time_b=0.0, weight=0.0) -> np.ndarray:
        """POSE_REQUEST_DTYPE records from scalars or arrays (broadcast against clip_a)."""
        ca = np.atleast_1d(np.asarray(clip_a, dtype=np.int32))
        r = np.zeros(ca.shape[0], dtype=POSE_REQUEST_DTYPE)
        r["clip_a"], r["time_a"], r["clip_b"], r["time_b"], r["weight"] = ca, time_a, clip_b, time_b, weight
        return r

    def Sample(self, skeleton: Skeleton, requests) -> "PoseSet":
        """swr_pose_set_sample: instance i from requests[i] (POSE_REQUEST_DTYPE: clip_a, time_a, clip_b or -1, time_b, weight) for
        i < len(requests) <= n_instances, on the GPU; no host wait."""
        r = np.ascontiguousarray(requests, dtype=POSE_REQUEST_DTYPE).reshape(-1)
        self._dev._ck(self._dev._lib.swr_pose_set_sample(self._dev._ctx, self._h, skeleton._h if skeleton is not None else None,
                                                         r.ctypes.data if r.size else None, int(r.size)))
        return self

    def Upload(self, first: int, palettes) -> "PoseSet":
        """swr_pose_set_upload: host-made palettes (n x n_joints x 4 x 4) into instances first .. first + n - 1; no host wait."""
        p = np.ascontiguousarray(palettes, dtype=np.float32).reshape(-1, self.n_joints * 16)
        self._dev._ck(self._dev._lib.swr_pose_set_upload(self._dev._ctx, self._h, int(first), int(p.shape[0]), p.ctypes.data if p.size else None))
        return self

    def Read(self) -> np.ndarray:
        """swr_pose_set_readback: (n_instances, n_joints, 4, 4) as the device holds them; waits for the set's last write only."""
        out = np.zeros((self.n_instances, self.n_joints, 4, 4), dtype=np.float32)
        self._dev._ck(self._dev._lib.swr_pose_set_readback(self._dev._ctx, self._h, out.ctypes.data))
        return out

    def Dispose(self):
        if self._h:
            self._dev._ck(self._dev._lib.swr_pose_set_destroy(self._dev._ctx, self._h))
            self._h = C.c_void_p()


class FrustumCuller:
    """public static class FrustumCuller (FrustumCuller.cs:57): the two members the frame loop uses."""

    @staticmethod
    def CalculateBoundingSphere(mesh: "Mesh") -> np.ndarray:          # FrustumCuller.cs:59-151
        return mesh.SphereBounds

    @staticmethod
    def IsSphereInFrustum(window: "MainWindow", bounds, modelMatrix, viewMatrix, projectionMatrix) -> bool:   # :201-218
        b, m, v, p = _f32(bounds, 4), _f32(modelMatrix, 16), _f32(viewMatrix, 16), _f32(projectionMatrix, 16)
        out = C.c_int(0)
        dev = window._dev
        dev._ck(dev._lib.swr_is_sphere_in_frustum(dev._ctx, _fptr(b), _fptr(m), _fptr(v), _fptr(p), C.byref(out)))
        return bool(out.value)


class RaycastFaceMask(enum.IntFlag):      # Physics.cs:8-14
    None_ = 0
    IgnoreBackfaces = 1
    IgnoreFrontfaces = 2


# numpy views of swr_ray (24 B) and swr_ray_hit (40 B)
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3)])
RAY_HIT_DTYPE = np.dtype([("found", "<i4"), ("target", "<i4"), ("triangle", "<i4"), ("distance", "<f4"), ("point", "<f4", 3), ("normal", "<f4", 3)])
assert RAY_DTYPE.itemsize == 24 == C.sizeof(N.Ray) and RAY_HIT_DTYPE.itemsize == 40 == C.sizeof(N.RayHit)


class Physics:
    """public static class Physics (Physics.cs:16) over retained meshes: every ray-triangle test runs on the GPU."""

    @staticmethod
    def _rays(origins, directions) -> np.ndarray:
        o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("origins and directions must have the same shape (n, 3)")
        rays = np.empty(o.shape[0], dtype=RAY_DTYPE)
        rays["origin"], rays["direction"] = o, d
        return rays

    @staticmethod
    def _targets(targets):
        """targets = [(Mesh, model)] or [(Mesh, model, normal_matrix)]; without a normal matrix it is hostmath.normal_matrix(model),
        and a model that does not invert leaves the target out (Physics.cs:30-36).  Returns (ctypes array, kept indices, device)."""
        from . import hostmath
        rows, kept, dev = [], [], None
        for k, t in enumerate(targets):
            mesh, model = t[0], _f32(t[1], 16)
            nm = t[2] if len(t) > 2 and t[2] is not None else hostmath.normal_matrix(model)
            if nm is None:
                continue
            if dev is not None and mesh._dev is not dev:
                raise ValueError("the meshes of one query must live on one Device")
            dev = mesh._dev
            rows.append((mesh, model, _f32(nm, 16))); kept.append(k)
        arr = (N.RayTarget * max(len(rows), 1))()
        for a, (mesh, model, nm) in zip(arr, rows):
            a.mesh = mesh._h.value
            a.model[:] = model.tolist()
            a.normal_matrix[:] = nm.tolist()
        return arr, kept, dev

    @staticmethod
    def _query(fn_name, rays, targets, faceMask, crossFused, per_pair):
        arr, kept, dev = Physics._targets(targets)
        n_out = rays.shape[0] * (len(kept) if per_pair else 1)
        out = np.zeros(n_out, dtype=RAY_HIT_DTYPE)
        if per_pair or not kept:
            out["target"] = np.tile(np.asarray(kept, dtype=np.int32), rays.shape[0]) if per_pair else -1
            out["triangle"], out["distance"] = -1, np.finfo(np.float32).max
        if kept and rays.shape[0]:
            flags = int(faceMask) | (N.SWR_RAY_CROSS_FUSED if crossFused else 0)
            dev._ck(getattr(dev._lib, fn_name)(dev._ctx, rays.ctypes.data, int(rays.shape[0]), C.addressof(arr), len(kept), flags, out.ctypes.data))
            tgt = out["target"]
            out["target"] = np.where(tgt >= 0, np.asarray(kept, dtype=np.int32)[np.maximum(tgt, 0)], tgt)    # index into the CALLER's list
        return out, kept

    @staticmethod
    def Raycast(rayOrigin, rayDirection, mesh: "Mesh", model, faceMask=RaycastFaceMask.IgnoreBackfaces, crossFused: bool = False):
        """Physics.Raycast (Physics.cs:19-52) against a retained mesh: (hit, hitDistance, hitPoint, hitNormal); a model that does not
        invert gives the reference's (False, float.MaxValue, zero, zero)."""
        out, _ = Physics._query("swr_raycast", Physics._rays(rayOrigin, rayDirection), [(mesh, model)], faceMask, crossFused, True)
        if out.shape[0] == 0:
            return False, float(np.finfo(np.float32).max), np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
        h = out[0]
        return bool(h["found"]), float(h["distance"]), h["point"].copy(), h["normal"].copy()

    @staticmethod
    def RaycastBatch(origins, directions, targets, faceMask=RaycastFaceMask.IgnoreBackfaces, crossFused: bool = False) -> np.ndarray:
        """swr_raycast: Physics.Raycast for every (ray, target) pair; targets = [(Mesh, model[, normal_matrix])].  Returns a
        (n_rays, n_kept) array of RAY_HIT_DTYPE whose `target` is the index into `targets` (targets whose model does not invert are
        left out, as the reference returns false for them)."""
        rays = Physics._rays(origins, directions)
        out, kept = Physics._query("swr_raycast", rays, targets, faceMask, crossFused, True)
        return out.reshape(rays.shape[0], len(kept))

    @staticmethod
    def RaycastNearest(origins, directions, targets, faceMask=RaycastFaceMask.IgnoreBackfaces, crossFused: bool = False) -> np.ndarray:
        """swr_raycast_nearest: per ray, the nearest hit over the targets in target order under strict `<` (the callers' lock blocks,
        CharacterController.cs:260-301,308-389); (n_rays,) of RAY_HIT_DTYPE, target = -1 where a ray misses everything."""
        rays = Physics._rays(origins, directions)
        return Physics._query("swr_raycast_nearest", rays, targets, faceMask, crossFused, False)[0]


# numpy views of swr_character_params (52 B), swr_character (44 B), swr_character_input (16 B) and swr_character_trace (48 B)
CHARACTER_PARAMS_DTYPE = np.dtype([("gravity", "<f4", 3), ("height", "<f4"), ("radius", "<f4"), ("step_size", "<f4"), ("move_speed", "<f4"),
                                   ("jump_force", "<f4"), ("ground_acceleration", "<f4"), ("air_acceleration", "<f4"), ("max_air_speed", "<f4"),
                                   ("ground_friction", "<f4"), ("air_control", "<f4")])
CHARACTER_DTYPE = np.dtype([("position", "<f4", 3), ("velocity", "<f4", 3), ("jump_cooldown", "<f4"), ("actual_step_size", "<f4"),
                            ("grounded", "<i4"), ("ceiling", "<i4"), ("noclip", "<i4")])
CHARACTER_INPUT_DTYPE = np.dtype([("move", "<f4", 3), ("jump", "<i4")])
CHARACTER_TRACE_DTYPE = np.dtype([("ground_found", "<i4"), ("ceiling_found", "<i4"), ("ground_point", "<f4", 3), ("ground_normal", "<f4", 3),
                                  ("chain_attempts", "<i4", 2), ("chain_stop", "<i4", 2)])
assert CHARACTER_PARAMS_DTYPE.itemsize == 52 == C.sizeof(N.CharacterParams) and CHARACTER_DTYPE.itemsize == 44 == C.sizeof(N.Character)
assert CHARACTER_INPUT_DTYPE.itemsize == 16 == C.sizeof(N.CharacterInput) and CHARACTER_TRACE_DTYPE.itemsize == 48 == C.sizeof(N.CharacterTrace)


class CharacterController:
    """public class CharacterController (CharacterController.cs:7-45) over retained meshes: Update runs whole on the GPU, in one
    call (swr_character_update).  collisionModels = one list of Mesh per model, modelMatrices = one matrix per model, as the
    reference's constructor takes them; they are flattened model-major, mesh-minor, and a model that does not invert is left out.

    The ring table -- (cos, sin) of the float32 angle 2 * pi * hStep / horizontalRays (:348-353) -- is the CALLER's: .NET's
    MathF.Cos / MathF.Sin are the C runtime's and the device cannot reproduce them, so this class computes the table with
    math.cos / math.sin of the float32 angle, rounded to float32, and a C# caller computes it with MathF (csharp/RasterizerNative.cs).
    CamOffset is kept for the caller's camera and takes no part in Update."""

    JumpCooldownDuration = 0.25

    def __init__(self, initialPosition, collisionModels, modelMatrices, crossFused: bool = False):
        self.Position = np.asarray(initialPosition, dtype=np.float32).reshape(3).copy()
        self.Velocity = np.zeros(3, dtype=np.float32)
        self.IsGrounded = False
        self.IsCeiling = False
        self.IsNoClipEnabled = False
        self.Gravity = np.array([0.0, -14.0, 0.0], dtype=np.float32)
        self.Height = 0.5
        self.Radius = 0.15
        self.StepSize = 0.3
        self.ActualStepSize = np.float32(0.03)
        self.MoveSpeed = 5.0
        self.JumpForce = 4.0
        self.GroundAcceleration = 3.5
        self.AirAcceleration = 0.35
        self.MaxAirSpeed = 6.0
        self.GroundFriction = 6.0
        self.AirControl = 0.2
        self.CamOffset = np.array([0.0, 0.15, 0.0], dtype=np.float32)
        self.JumpCooldownTimer = np.float32(0.0)
        self.CrossFused = bool(crossFused)
        self.CollisionModels = [list(m) for m in collisionModels] if collisionModels is not None else None
        self.ModelMatrices = [np.asarray(m, dtype=np.float32).reshape(4, 4) for m in modelMatrices] if modelMatrices is not None else None
        self.LastTrace = None
        self._flat = None
        self._ring_key, self._ring = None, None

    # ---- what the caller supplies
    def Params(self) -> np.ndarray:
        p = np.zeros((), dtype=CHARACTER_PARAMS_DTYPE)
        p["gravity"] = self.Gravity
        for name, v in (("height", self.Height), ("radius", self.Radius), ("step_size", self.StepSize), ("move_speed", self.MoveSpeed),
                        ("jump_force", self.JumpForce), ("ground_acceleration", self.GroundAcceleration),
                        ("air_acceleration", self.AirAcceleration), ("max_air_speed", self.MaxAirSpeed),
                        ("ground_friction", self.GroundFriction), ("air_control", self.AirControl)):
            p[name] = v
        return p

    @staticmethod
    def RayCounts(params) -> tuple:
        """(verticalSteps, horizontalRays) of MoveWithSlide (:327-328) for a CHARACTER_PARAMS_DTYPE record (swr_character_ray_counts)."""
        p = np.ascontiguousarray(params, dtype=CHARACTER_PARAMS_DTYPE).reshape(1)
        v, h = C.c_int(0), C.c_int(0)
        rc = N.load().swr_character_ray_counts(p.ctypes.data, C.byref(v), C.byref(h))
        if rc != N.SWR_OK:
            raise N.SwrError(rc, "ray counts of these parameters are not numbers or beyond the limits")
        return v.value, h.value

    @staticmethod
    def Ring(horizontalRays: int) -> np.ndarray:
        """(horizontalRays, 2) float32: cos and sin of the float32 angle 2 * MathF.PI * hStep / horizontalRays (:348), through the C
        runtime's double cos / sin rounded to float32 -- this caller's table."""
        import math
        two_pi = np.float32(2.0) * np.float32(math.pi)
        out = np.empty((horizontalRays, 2), dtype=np.float32)
        for h in range(horizontalRays):
            angle = np.float32(np.float32(two_pi * np.float32(h)) / np.float32(horizontalRays))
            out[h] = np.float32(math.cos(float(angle))), np.float32(math.sin(float(angle)))
        return out

    def _ring_table(self, params) -> np.ndarray:
        key = float(np.float32(self.Radius)), float(np.float32(self.Height))
        if self._ring_key != key:
            self._ring_key, self._ring = key, CharacterController.Ring(CharacterController.RayCounts(params)[1])
        return self._ring

    def _targets(self):
        if self.CollisionModels is None or self.ModelMatrices is None or len(self.CollisionModels) != len(self.ModelMatrices):
            return []                                                          # :233, :314: every query answers "nothing"
        if self._flat is None:
            self._flat = [(mesh, m) for meshes, m in zip(self.CollisionModels, self.ModelMatrices) for mesh in meshes]
        return self._flat

    @staticmethod
    def _same_targets(a, b) -> bool:
        """the same Mesh objects under equal matrices, in the same order"""
        ta, tb = a._targets(), b._targets()
        return len(ta) == len(tb) and all(x[0] is y[0] and np.array_equal(x[1], y[1]) for x, y in zip(ta, tb))

    def State(self) -> np.ndarray:
        s = np.zeros((), dtype=CHARACTER_DTYPE)
        s["position"], s["velocity"] = self.Position, self.Velocity
        s["jump_cooldown"], s["actual_step_size"] = self.JumpCooldownTimer, self.ActualStepSize
        s["grounded"], s["ceiling"], s["noclip"] = int(self.IsGrounded), int(self.IsCeiling), int(self.IsNoClipEnabled)
        return s

    def _take(self, s, trace):
        self.Position, self.Velocity = s["position"].copy(), s["velocity"].copy()
        self.JumpCooldownTimer, self.ActualStepSize = np.float32(s["jump_cooldown"]), np.float32(s["actual_step_size"])
        self.IsGrounded, self.IsCeiling = bool(s["grounded"]), bool(s["ceiling"])
        self.LastTrace = trace

    def Update(self, DeltaTime: float, MoveInput, JumpRequested: bool) -> None:
        """CharacterController.Update (:50-140)."""
        CharacterController.UpdateBatch([self], DeltaTime, [MoveInput], [JumpRequested])

    @staticmethod
    def UpdateRaw(device, params, states, inputs, DeltaTime, ring, targets, crossFused=False, trace=True):
        """swr_character_update on arrays: states (CHARACTER_DTYPE) is updated in place; returns the CHARACTER_TRACE_DTYPE array or None.
        targets = [(Mesh, model[, normal_matrix])] as Physics.RaycastBatch takes them."""
        p = np.ascontiguousarray(params, dtype=CHARACTER_PARAMS_DTYPE).reshape(1)
        if states.dtype != CHARACTER_DTYPE or not states.flags.c_contiguous:
            raise ValueError("states must be a C-contiguous CHARACTER_DTYPE array")
        inp = np.ascontiguousarray(inputs, dtype=CHARACTER_INPUT_DTYPE).reshape(-1)
        if inp.shape[0] != states.shape[0]:
            raise ValueError("one input per controller")
        r = np.ascontiguousarray(ring, dtype=np.float32).reshape(-1, 2)
        arr, kept, dev = Physics._targets(targets)
        dev = dev or device
        tr = np.zeros(states.shape[0], dtype=CHARACTER_TRACE_DTYPE) if trace else None
        flags = N.SWR_RAY_CROSS_FUSED if crossFused else 0
        dev._ck(dev._lib.swr_character_update(dev._ctx, p.ctypes.data, states.ctypes.data, inp.ctypes.data, int(states.shape[0]),
                                              float(DeltaTime), r.ctypes.data, int(r.shape[0]), C.addressof(arr), len(kept), flags,
                                              tr.ctypes.data if trace else None))
        return tr

    @staticmethod
    def UpdateBatch(controllers, DeltaTime: float, MoveInputs, JumpRequests, device=None) -> None:
        """Update for many controllers in one call.  They share the first one's properties, collision models and Cross model (the
        call has one swr_character_params and one target list); position, velocity, timers and flags are each controller's own."""
        if not controllers:
            return
        first = controllers[0]
        params = first.Params()
        for c in controllers[1:]:
            if c.Params().tobytes() != params.tobytes() or c.CrossFused != first.CrossFused or not CharacterController._same_targets(c, first):
                raise ValueError("the controllers of one batch share their properties, collision models and Cross model")
        states = np.array([c.State() for c in controllers], dtype=CHARACTER_DTYPE)
        inputs = np.zeros(len(controllers), dtype=CHARACTER_INPUT_DTYPE)
        inputs["move"] = np.asarray(MoveInputs, dtype=np.float32).reshape(len(controllers), 3)
        inputs["jump"] = [1 if j else 0 for j in JumpRequests]
        targets = first._targets()
        if device is None:
            if not targets:
                raise ValueError("a controller without collision meshes needs the `device` argument")
            device = targets[0][0]._dev
        trace = CharacterController.UpdateRaw(device, params, states, inputs, DeltaTime, first._ring_table(params), targets, first.CrossFused)
        for c, s, t in zip(controllers, states, trace):
            c._take(s, t)


def as_vertex_array(vertices) -> np.ndarray:
    v = np.asarray(vertices)
    if v.dtype == VERTEX_DTYPE:
        return np.ascontiguousarray(v).reshape(-1)
    v = np.ascontiguousarray(v, dtype=np.float32)
    if v.ndim != 2 or v.shape[1] != 12:
        raise ValueError("vertices must have dtype VERTEX_DTYPE or shape (n, 12) float32")
    return v.view(VERTEX_DTYPE).reshape(-1)


class Rasterizer:
    """public static class Rasterizer (Rasterizer.cs:12): statics + enums + RenderMesh."""

    DebugMode = DebugMode
    BlendMode = BlendMode
    DepthTest = DepthTest
    CullMode = CullMode

    NearClip = 0.1                       # Rasterizer.cs:20
    FarClip = 1000.0                     # Rasterizer.cs:21
    RenderDebugMode = DebugMode.None_    # Rasterizer.cs:22

    @staticmethod
    def InitializeTileLocks(window: MainWindow, width: int, height: int):
        """Rasterizer.cs:69-93; non-positive sizes raise (C#: ArgumentException)."""
        try:
            window._dev._ck(window._dev._lib.swr_initialize_tile_locks(window._dev._ctx, int(width), int(height)))
        except N.SwrError as e:
            if e.code == N.SWR_ERR_INVALID_ARG:
                raise ValueError("Width and height must be positive non-zero values.") from e
            raise

    @classmethod
    def RenderMesh(cls, window: MainWindow, vertices, indices, model, view, projection,
                   vertexShader: VertexShader, fragmentShader: FragmentShader,
                   cullMode: CullMode = CullMode.Back, depthTest: DepthTest = DepthTest.LessEqual,
                   blendMode: BlendMode = BlendMode.Alpha, frustumCull: bool = False):
        """Rasterizer.RenderMesh, Rasterizer.cs:163-174.  frustumCull=True (retained meshes only) prepends the
        reference's `if (!FrustumCuller.IsSphereInFrustum(mesh.SphereBounds, ...)) return;` (Renderer.cs:446), evaluated on the GPU.  `vertices` may be a retained `Mesh`
        (then `indices` is ignored) or the VertexInput[] / ushort[] arrays of the C# signature."""
        prog = fragmentShader.program
        if vertexShader.program is not prog:
            raise ValueError("vertexShader and fragmentShader must come from the same ShaderProgram")
        window._activate()
        dev = window._dev
        dev._ck(dev._lib.swr_set_state(dev._ctx, float(cls.NearClip), float(cls.FarClip), int(cls.RenderDebugMode)))
        m, v, p = _f32(model, 16), _f32(view, 16), _f32(projection, 16)
        tex = prog.texture._h if prog.texture is not None else None
        pid = prog._program_for(dev)
        if isinstance(vertices, Mesh):
            fn = dev._lib.swr_render_mesh_culled if frustumCull else dev._lib.swr_render_mesh
            rc = fn(dev._ctx, vertices._h, _fptr(m), _fptr(v), _fptr(p), pid,
                                          C.byref(prog.uniforms), tex, int(cullMode), int(depthTest), int(blendMode))
        else:
            va = as_vertex_array(vertices)
            ia = np.ascontiguousarray(indices, dtype=np.uint16).reshape(-1)
            rc = dev._lib.swr_render_mesh_arrays(dev._ctx, va.ctypes.data, int(va.shape[0]), ia.ctypes.data, int(ia.shape[0]),
                                                 _fptr(m), _fptr(v), _fptr(p), pid, C.byref(prog.uniforms), tex,
                                                 int(cullMode), int(depthTest), int(blendMode))
        if rc == N.SWR_ERR_INVALID_ARG:
            msg = dev._lib.swr_last_error(dev._ctx).decode()
            if "index out of range" in msg:
                raise IndexError(msg)      # C#: IndexOutOfRangeException
        dev._ck(rc)

    @staticmethod
    def Interpolate(window: MainWindow, a, b, c, w, interpolate: bool = True) -> np.ndarray:
        """Rasterizer.Interpolate (public, Rasterizer.cs:566-640), batched over n weight triples.
        a, b, c: 20-float vertex records {clip4,color4,uv2,normal3,screen2,worldNormal3,pad2};
        returns (n, 24): {clip4,color4,uv2,normal3,screen2,worldNormal3,bary3,pad3}."""
        verts = np.concatenate([_f32(a, 20), _f32(b, 20), _f32(c, 20)])
        wts = np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1, 3))
        out = np.empty((wts.shape[0], 24), dtype=np.float32)
        dev = window._dev
        dev._ck(dev._lib.swr_interpolate(dev._ctx, verts.ctypes.data, wts.ctypes.data, wts.shape[0], 1 if interpolate else 0, out.ctypes.data))
        return out
