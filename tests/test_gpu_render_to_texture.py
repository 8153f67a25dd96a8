"""Render to texture on the GPU (include/swr.h, csrc/swr_deliver.hip.h): k_frame_to_texture against the numpy
restatement of tests/render_to_texture_cases.py byte for byte, its block-linear copy through the bilinear filter, and the ordering of
swr_texture_update_from_frame against the draws around it -- within one context and between two -- without a host synchronisation."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import render_to_texture_cases as T
from softwarerenderer_amd import (BlendMode, CullMode, DepthTest, Device, MainWindow, Rasterizer, Shaders, Texture, _native,
                                  default_uniforms, hostmath as hm, scenes)
from test_gpu_parity import run_both

pytestmark = pytest.mark.gpu

# a user fragment program with two dependent-free fetches of the draw's texture
TWO_FETCHES = r"""
__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {
    const float4 a = swr_sample(env, in.tex_coord);
    const float4 b = swr_sample(env, make_float2(in.tex_coord.y + 0.25f, in.tex_coord.x));
    return make_float4(a.x * in.color.x, b.y * in.color.y, a.z * b.x, 1.0f);
}
"""


@pytest.fixture(scope="module")
def other():
    """A second context on the same GPU: the camera whose frame becomes the first context's texture."""
    dev = Device(0)
    yield dev
    dev.close()


@functools.lru_cache(maxsize=None)
def plane(width, height, seed):
    p = T.pool_plane(height, width, seed)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def want(width, height, seed, kx, ky, keep):
    w = T.texels(plane(width, height, seed), kx, ky, keep_alpha=keep)
    w.setflags(write=False)
    return w


def same_bytes(got, expect, what=""):
    assert got.dtype == np.uint8 and got.shape == expect.shape, (what, got.dtype, got.shape, expect.shape)
    bad = np.argwhere(got != expect)
    assert bad.size == 0, (what, f"{len(bad)} bytes differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {expect[tuple(bad[0])]}")


def same_words(got, expect, what=""):
    assert got.shape == expect.shape, (what, got.shape, expect.shape)
    g, e = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32), np.ascontiguousarray(expect, dtype=np.float32).view(np.uint32)
    bad = np.argwhere(g != e)
    assert bad.size == 0, (what, f"{len(bad)} words differ, first at {tuple(bad[0])}")


# ------------------------------------------------------------------------------------------------------------------ 1. bytes
@pytest.mark.parametrize("tex_size,factors", T.GPU_SHAPES)
def test_texels_equal_the_restatement_under_both_alpha_modes(device, tex_size, factors):
    (w, h), (kx, ky) = tex_size, factors
    fw, fh = T.source_size(tex_size, factors)
    seed = 100 + w
    win = MainWindow(device, fw, fh)
    win.Upload(color=plane(fw, fh, seed))
    tex = Texture.Target(device, w, h)
    try:
        for keep in (False, True):
            tex.UpdateFrom(win, kx, ky, keep_alpha=keep)
            got = tex.Read()
            expect = want(fw, fh, seed, kx, ky, keep)
            same_bytes(got, expect, (tex_size, factors, keep))
            if not keep:
                same_bytes(got, win.ColorBuffer8(kx, ky, 4), (tex_size, factors, "swr_readback_rgb8"))
            else:
                assert len(np.unique(got[..., 3])) > 2, "alpha was not kept"
            sampled = tex.Sample(T.texel_centres(w, h))
            same_words(sampled, expect.astype(np.float32) * np.float32(1.0 / 255.0), (tex_size, factors, keep, "Sample"))
    finally:
        tex.Dispose()


# --------------------------------------------------------------------------------------------------- 2. block-linear copy
QUAD = scenes.make_vertices([(-0.9, -0.8, 0.0), (0.95, -0.85, 0.0), (0.9, 0.9, 0.0), (-0.85, 0.8, 0.0)],
                            uv=[(-0.6, -0.4), (1.7, -0.3), (1.6, 1.5), (-0.5, 1.4)],
                            color=[(1, 0.9, 0.8, 1), (0.7, 1, 0.9, 1), (0.9, 0.8, 1, 1), (1, 1, 1, 1)])
QUAD_IDX = np.array([0, 1, 2, 0, 2, 3], dtype=np.uint16)


def draw_quad(win, tex, clear=(0.1, 0.2, 0.3, 1.0)):
    """One textured quad with wrapping uv under DUST2's program; the frame as (colour, depth)."""
    I = hm.identity()
    prog = Shaders.Dust2LambertFog(default_uniforms(), tex)
    win.ClearDepthBuffer()
    win.ClearColorBuffer(clear)
    Rasterizer.RenderMesh(win, QUAD, QUAD_IDX, I, I, I, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.Alpha)
    return win._read(True, True)


@pytest.mark.parametrize("tex_size,factors", T.BLOCKED_SHAPES)
@pytest.mark.parametrize("filter_first", [True, False])
def test_the_bilinear_copy_is_written_by_the_update_and_refreshed_by_the_next(device, other, tex_size, factors, filter_first):
    (w, h), (kx, ky) = tex_size, factors
    fw, fh = T.source_size(tex_size, factors)
    cam = MainWindow(other, fw, fh)
    win = MainWindow(device, 96, 64)
    tex = Texture.Target(device, w, h)
    frames = []
    try:
        if filter_first:
            tex.SetBilinear(True)                     # the block-linear copy exists (of zeros) before the first update
        for seed, keep in ((200 + w, False), (300 + w, True)):
            cam.Upload(color=plane(fw, fh, seed))
            tex.UpdateFrom(cam, kx, ky, keep_alpha=keep)
            if not filter_first:
                tex.SetBilinear(True)                 # first time: built from the texels the update left; then a no-op
            got = draw_quad(win, tex)
            ref_tex = Texture(device, want(fw, fh, seed, kx, ky, keep))
            ref_tex.SetBilinear(True)
            ref = draw_quad(win, ref_tex)
            ref_tex.Dispose()
            same_words(got[0], ref[0], (tex_size, factors, filter_first, seed, "colour"))
            same_words(got[1], ref[1], (tex_size, factors, filter_first, seed, "depth"))
            same_bytes(tex.Read(), want(fw, fh, seed, kx, ky, keep), "row-major texels")
            frames.append(got[0])
        assert not np.array_equal(frames[0], frames[1]), "the second update changed nothing on screen"
    finally:
        tex.Dispose()


# --------------------------------------------------------------------------------------------- 3. end to end, two contexts
def camera_scene():
    return scenes.cfg3(128, 96, (2, 2), (12, 8), tex_size=32, seed=5)


def screen_scene(program=None, width=160, height=112):
    s = scenes.cfg3(width, height, (2, 2), (10, 6), tex_size=8, seed=9)
    if program is not None:
        s = dataclasses.replace(s, draws=[dataclasses.replace(d, program=program) for d in s.draws])
    return s


def render_with(device, scene, texture=None, texels=None, window=None):
    """The scene with every draw's texture replaced: by `texture`, or by a host-created texture of `texels`."""
    made = Texture(device, texels) if texture is None else None
    r = scenes.SceneRenderer(device, scene, window=window)
    for p in r.programs:
        p.texture = texture if texture is not None else made
    device.reset_stats()
    color, depth = r.render()
    st = device.stats()
    r.close()
    if made is not None:
        made.Dispose()
    return color, depth, st


@pytest.mark.parametrize("user_program", [False, True])
def test_a_camera_in_one_context_feeds_a_screen_in_another(device, other, user_program):
    program = device.compile_program(TWO_FETCHES) if user_program else None
    cam = scenes.SceneRenderer(other, camera_scene())
    tex = Texture.Target(device, 64, 48)
    try:
        cam.window.Upload(color=np.zeros((96, 128, 4), dtype=np.float32))      # (whatever an earlier test left there is gone)
        cam.submit_frame()                            # recorded, not flushed: the update completes the frame
        tex.UpdateFrom(cam.window, 2, 2)
        got = render_with(device, screen_scene(program), texture=tex)
        host_bytes = cam.window.ColorBuffer8(2, 2, 4)
        assert len(np.unique(host_bytes[..., :3])) > 50, "the camera's frame is empty"
        same_bytes(tex.Read(), host_bytes, "texels against swr_readback_rgb8")
        ref = render_with(device, screen_scene(program), texels=host_bytes)
        same_words(got[0], ref[0], "colour"); same_words(got[1], ref[1], "depth")
        assert got[2] == ref[2] and got[2]["fragments_written"] > 0
        blank = render_with(device, screen_scene(program), texels=np.zeros((48, 64, 4), dtype=np.uint8))
        assert not np.array_equal(blank[0], ref[0]), "the screen does not show its texture"
    finally:
        if program is not None:
            device.destroy_program(program)
        tex.Dispose(); cam.close()


@pytest.mark.parametrize("user_program", [False, True])
def test_a_context_feeds_itself_frame_then_clear_then_draw(device, user_program):
    program = device.compile_program(TWO_FETCHES) if user_program else None
    cam = scenes.SceneRenderer(device, camera_scene())
    tex = Texture.Target(device, 64, 48)
    try:
        cam.window.Upload(color=np.zeros((96, 128, 4), dtype=np.float32))
        cam.submit_frame()                            # recorded, not flushed
        tex.UpdateFrom(cam.window, 2, 2)              # src == NULL: the context's own frame
        got = render_with(device, screen_scene(program, 128, 96), texture=tex, window=cam.window)      # clears, then draws over it
        cam.submit_frame()
        host_bytes = cam.window.ColorBuffer8(2, 2, 4)
        same_bytes(tex.Read(), host_bytes, "texels against swr_readback_rgb8")
        ref = render_with(device, screen_scene(program, 128, 96), texels=host_bytes, window=cam.window)
        same_words(got[0], ref[0], "colour"); same_words(got[1], ref[1], "depth")
        assert got[2] == ref[2] and got[2]["fragments_written"] > 0
    finally:
        if program is not None:
            device.destroy_program(program)
        tex.Dispose(); cam.close()


# ------------------------------------------------------------------------------------- 4. order, no host synchronisation
W, H = 128, 96


def feedback_frames(device, win, soups, use_update):
    """Three frames of a feedback loop on one context.  Per frame: clear; a full-screen quad with the texture (frame N - 1's image),
    flushed on odd frames; a triangle soup, recorded and NOT flushed; the texture becomes the frame; a second, smaller quad with the
    texture (frame N's image).  use_update: swr_texture_update_from_frame and nothing else; otherwise the host route of the parent
    commit with a swr_sync after every step.  Returns (colour, depth, texels) after the third frame and the sync counts seen."""
    I = hm.identity()
    tex = Texture.Target(device, W // 2, H // 2)
    prog = Shaders.Dust2LambertFog(default_uniforms(), tex)
    gouraud = Shaders.Gouraud()
    moved = []
    step = (lambda: None) if use_update else device.sync
    for n in range(3):
        big = QUAD.copy()
        big["uv"] += np.float32(0.13 * n)
        small = QUAD.copy()
        small["position"][:, :2] *= np.float32(0.5)
        small["uv"] = small["uv"] * np.float32(0.5) + np.float32(0.25)
        win.ClearDepthBuffer(); win.ClearColorBuffer((0.2 * n, 0.9 - 0.3 * n, 0.5, 1.0)); step()
        Rasterizer.RenderMesh(win, big, QUAD_IDX, I, I, I, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.Always, BlendMode.Alpha)
        if n & 1:
            device.flush()
        step()
        d = soups[n].draws[0]
        Rasterizer.RenderMesh(win, d.vertices, d.indices, d.model, d.view, d.projection, gouraud.VertexShader, gouraud.FragmentShader,
                              d.cull, d.depth_test, d.blend)
        step()
        if use_update:
            before = device.sync_count()
            tex.UpdateFrom(win, 2, 2, keep_alpha=bool(n & 1))
            moved.append(device.sync_count() - before)
        else:
            texels = T.texels(win.ColorBuffer, 2, 2, keep_alpha=bool(n & 1)) if n & 1 else win.ColorBuffer8(2, 2, 4)
            old, tex = tex, Texture(device, texels)
            prog = Shaders.Dust2LambertFog(default_uniforms(), tex)
            old.Dispose(); step()
        Rasterizer.RenderMesh(win, small, QUAD_IDX, I, I, I, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.Always, BlendMode.Alpha)
        step()
    color, depth = win._read(True, True)
    texels = tex.Read() if use_update else texels
    tex.Dispose()
    return color, depth, texels, moved


@pytest.mark.parametrize("pipelining", [0, 1, 2])
def test_draws_before_the_update_see_the_old_texels_and_draws_after_it_the_new(device, pipelining):
    soups = [scenes.cfg2(W, H, 60, seed=40 + n, min_area=30.0, max_area=900.0) for n in range(3)]
    win = MainWindow(device, W, H)
    was = device.pipelining()
    device.set_pipelining(pipelining)
    try:
        feedback_frames(device, win, soups, use_update=True)              # sizes the pair buffers of every raster set in use
        device.sync()
        replays = device.replay_count()
        color, depth, texels, moved = feedback_frames(device, win, soups, use_update=True)
        assert moved == [0, 0, 0], "swr_texture_update_from_frame made the host wait"
        assert device.replay_count() == replays, "a batch was replayed: the comparison below would not be about ordering"
        ref = feedback_frames(device, win, soups, use_update=False)
        same_words(color, ref[0], "colour after three frames"); same_words(depth, ref[1], "depth after three frames")
        same_bytes(texels, ref[2], "texels after three frames")
        assert len(np.unique(texels[..., :3])) > 50 and len(np.unique(texels[..., 3])) == 1      # the last frame's mode was opaque
    finally:
        device.set_pipelining(was)


# ---------------------------------------------------------------------------------------------------------------- 5. errors
def hip_device_count():
    n = C.c_int(0)
    assert C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(n)) == 0
    return n.value


def test_refusals_leave_the_texture_and_the_context_alone(device, other):
    lib, ctx = device._lib, device._ctx
    win = MainWindow(device, 64, 32)
    win.Upload(color=plane(64, 32, 7))
    tex = Texture.Target(device, 32, 16)
    assert tex.Read().shape == (16, 32, 4) and not tex.Read().any(), "a new target is not zero-filled"

    def refused(code, words, t, src, kx, ky, mode):
        syncs = device.sync_count()
        assert lib.swr_texture_update_from_frame(ctx, t, src, kx, ky, mode) == code, words
        assert words in lib.swr_last_error(ctx).decode(), (words, lib.swr_last_error(ctx).decode())
        assert device.sync_count() == syncs
    try:
        refused(_native.SWR_ERR_INVALID_ARG, "texture width * kx by texture height * ky", tex._h, None, 1, 1, 0)       # 32 x 16 from 64 x 32
        refused(_native.SWR_ERR_INVALID_ARG, "texture width * kx by texture height * ky", tex._h, None, 2, 4, 0)
        refused(_native.SWR_ERR_INVALID_ARG, "factors must be 1, 2, 4 or 8", tex._h, None, 3, 2, 0)
        refused(_native.SWR_ERR_INVALID_ARG, "factors must be 1, 2, 4 or 8", tex._h, None, 2, 0, 0)
        refused(_native.SWR_ERR_INVALID_ARG, "factors must be 1, 2, 4 or 8", tex._h, None, 16, 2, 0)
        refused(_native.SWR_ERR_INVALID_ARG, "alpha_mode", tex._h, None, 2, 2, 2)
        refused(_native.SWR_ERR_INVALID_ARG, "alpha_mode", tex._h, None, 2, 2, -1)
        refused(_native.SWR_ERR_INVALID_ARG, "texture is null", None, None, 2, 2, 0)
        # a source that holds a band of its frame: a contiguous band, then interleaved stripes
        cam = MainWindow(other, 64, 32)
        cam.SetBand(1, 1)
        refused(_native.SWR_ERR_UNSUPPORTED, "only a band", tex._h, other._ctx, 2, 2, 0)
        cam.SetBandInterleaved(0, 2, 1)
        refused(_native.SWR_ERR_UNSUPPORTED, "only a band", tex._h, other._ctx, 2, 2, 0)
        cam.SetBand(-1, -1)
        if hip_device_count() > 1:
            far = Device(1)
            try:
                MainWindow(far, 64, 32)
                refused(_native.SWR_ERR_UNSUPPORTED, "another device", tex._h, far._ctx, 2, 2, 0)
            finally:
                far.close()
        with pytest.raises(_native.SwrError) as e:
            tex.UpdateFrom(win, 4, 2)
        assert e.value.code == _native.SWR_ERR_INVALID_ARG
        h = C.c_void_p()
        for bad in ((0, 4), (4, -1)):
            assert lib.swr_texture_create_target(ctx, bad[0], bad[1], C.byref(h)) == _native.SWR_ERR_INVALID_ARG and not h.value
        assert lib.swr_texture_create_target(ctx, 4, 4, None) == _native.SWR_ERR_INVALID_ARG
        assert lib.swr_texture_create_target(ctx, 1 << 15, 1 << 15, C.byref(h)) == _native.SWR_ERR_UNSUPPORTED and not h.value
        assert lib.swr_texture_readback(ctx, tex._h, None) == _native.SWR_ERR_INVALID_ARG
        assert not tex.Read().any(), "a refused update wrote texels"
        # ... and both contexts still work: the refused call, accepted; then a parity frame
        cam.Upload(color=plane(64, 32, 7))
        tex.UpdateFrom(cam, 2, 2, keep_alpha=True)
        same_bytes(tex.Read(), want(64, 32, 7, 2, 2, True), "after the refusals, from the other context")
        tex.UpdateFrom(win, 2, 2)
        same_bytes(tex.Read(), want(64, 32, 7, 2, 2, False), "after the refusals, own frame")
    finally:
        tex.Dispose()
    run_both(device, scenes.cfg2(160, 120, 200, seed=3))
