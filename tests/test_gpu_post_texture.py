"""Post programs with textures on the GPU (include/swr.h, csrc/swr_post.hip.h): swr_post_set_texture and the four
helpers against the oracle's samplers and the numpy twins of tests/post_texture_cases.py, word for word and byte for byte; what a
present captures when it is called; swr_texture_update_from_post, its block-linear copy, chains of passes within one context and
between two, its order against draws, and its refusals."""
import ctypes as C

import numpy as np
import pytest

import post_cases as P
import post_texture_cases as X
from resolve_cases import assert_same_words
from softwarerenderer_amd import (BlendMode, CullMode, DepthTest, Device, MainWindow, PostProgram, Rasterizer, Shaders, Texture, _native,
                                  default_uniforms, hostmath as hm, scenes)
from test_gpu_present8 import DeviceBytes
from test_gpu_render_to_texture import QUAD, QUAD_IDX, same_bytes, same_words

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = _native.SWR_ERR_INVALID_ARG, _native.SWR_ERR_UNSUPPORTED
NAMES = ("SAMPLE", "FOUR", "DYNAMIC", "TEXEL", "SIZES", "BLUR_H", "BLUR_V", "ACCUM")


def programs_of(dev):
    progs = {name: PostProgram(dev, X.TEXTS[name]) for name in NAMES}
    progs["IDENTITY"] = PostProgram(dev, P.IDENTITY)
    return progs


@pytest.fixture(scope="module")
def posts(device, oracle_lib):
    progs = programs_of(device)
    yield progs
    for p in progs.values():
        p.close()


@pytest.fixture(scope="module")
def other():
    """A second context on the same GPU: the camera."""
    dev = Device(0)
    yield dev
    dev.close()


@pytest.fixture(scope="module")
def textures(device):
    """The three textures of the cases, once nearest and once under the filter (8 x 8 then has a block-linear copy, 5 x 3 cannot)."""
    made = {}
    for size in X.TEXTURE_SIZES:
        for bilinear in (False, True):
            t = Texture(device, X.texture(size))
            t.SetBilinear(bilinear)
            made[size, bilinear] = t
    yield made
    for t in made.values():
        t.Dispose()


def bind(post, textures, keys):
    """keys: four entries, None or (size, bilinear).  Returns the twin's slots."""
    for slot, key in enumerate(keys):
        post.SetTexture(slot, textures[key] if key is not None else None)
    return tuple((X.texture(key[0]), key[1]) if key is not None else None for key in keys)


def run(win, post, constants, factors=(1, 1)):
    post.SetConstants(constants)
    return win.PostBuffer(post, *factors, 3, np.float32)


# ------------------------------------------------------------------------------------------------------------- 1. the samplers
@pytest.mark.parametrize("out_size", P.OUT_SIZES)
def test_sampling_equals_the_oracle_word_for_word(device, posts, textures, out_size):
    for factors in ((1, 1), (4, 2)):
        w, h = P.frame_size(out_size, factors)
        win = MainWindow(device, w, h)
        win.Upload(color=P.planes(out_size, factors, "pool")[0])
        for size in X.TEXTURE_SIZES:
            for bilinear in (False, True):
                slots = bind(posts["SAMPLE"], textures, [(size, bilinear), None, None, None])
                for reverse in (False, True):
                    k = X.uv_constants(out_size, reverse=reverse)
                    got = run(win, posts["SAMPLE"], k, factors)
                    want = X.sample_twin(np.zeros((out_size[1], out_size[0], 4), dtype=np.float32), k, slots)[..., :3]
                    assert_same_words(got, want, (out_size, factors, size, bilinear, reverse))


# ------------------------------------------------------------------------------------------------------------ 2. four slots
@pytest.mark.parametrize("out_size", P.OUT_SIZES)
def test_four_slots_at_once_and_a_slot_that_varies_by_lane(device, posts, textures, out_size):
    win = MainWindow(device, *out_size)
    k = X.uv_constants(out_size)
    res = np.zeros((out_size[1], out_size[0], 4), dtype=np.float32)
    full = [((8, 8), True), ((5, 3), False), ((1, 1), False), ((5, 3), True)]
    for keys in (full, [None, ((5, 3), False), None, ((8, 8), True)], [((8, 8), False), None, None, None], [None] * 4):
        for name in ("FOUR", "DYNAMIC"):
            slots = bind(posts[name], textures, keys)
            assert_same_words(run(win, posts[name], k), X.TWINS[name](res, k, slots)[..., :3], (name, out_size, keys))
    if out_size != (1, 1):
        slots = bind(posts["FOUR"], textures, full)
        assert not np.array_equal(run(win, posts["FOUR"], k), X.four_slots_swapped(res, k, slots)[..., :3])


# ------------------------------------------------------------------------------------------------------- 3. texels and sizes
@pytest.mark.parametrize("out_size", [(65, 5), (130, 9)])
def test_texel_and_texture_size_at_the_corners_and_beyond(device, posts, textures, out_size):
    win = MainWindow(device, *out_size)
    res = np.zeros((out_size[1], out_size[0], 4), dtype=np.float32)
    for size in X.TEXTURE_SIZES:
        for bilinear in (False, True):                                 # (8 x 8 under the filter: the texel comes out of the block-linear copy)
            slots = bind(posts["TEXEL"], textures, [(size, bilinear), None, None, None])
            for shift in ((0, 0), (-2, -1), (3, 2), (-60, 4), (1000, -1000), (-100000, 100000)):
                k = P.constants64(shift)
                assert_same_words(run(win, posts["TEXEL"], k), X.texel_twin(res, k, slots)[..., :3], (size, bilinear, shift))
    slots = bind(posts["TEXEL"], textures, [None] * 4)
    assert np.all(run(win, posts["TEXEL"], P.constants64()) == 1.0)
    for keys in ([((8, 8), True), ((5, 3), False), None, ((1, 1), False)], [None, None, ((8, 8), False), ((5, 3), True)], [None] * 4):
        slots = bind(posts["SIZES"], textures, keys)
        got = win.PostBuffer(posts["SIZES"], 1, 1, 3, np.float32)
        assert_same_words(got, X.sizes_twin(res, P.constants64(), slots)[..., :3], keys)
    # w (the bound slots as bits) through the KEEP mode's alpha: bits / 64 quantised
    slots = bind(posts["SIZES"], textures, [((8, 8), True), None, None, ((1, 1), False)])
    t = Texture.Target(device, *out_size)
    try:
        t.UpdateFromPost(win, posts["SIZES"], keep_alpha=True)
        same_bytes(t.Read(), X.texels(X.sizes_twin(res, P.constants64(), slots), keep_alpha=True), "SIZES")
        assert t.Read()[0, 0, 3] == round((2 + 16) / 64 * 255)
    finally:
        t.Dispose()


# ------------------------------------------------------------------------------------------------- 4. captured at the call
def test_two_presents_in_flight_keep_their_own_slots_and_filters():
    dev = Device(0)                                                    # a fresh context: its staging buffers start empty
    out_size = (65, 5)
    win = MainWindow(dev, *out_size)
    win.Upload(color=np.zeros((5, 65, 4), dtype=np.float32))
    post = PostProgram(dev, X.SAMPLE)
    k = X.uv_constants(out_size)
    post.SetConstants(k)
    ta, tb = Texture(dev, X.texture((8, 8))), Texture(dev, X.texture((8, 8), seed=1))
    ta.SetBilinear(True); ta.SetBilinear(False)                       # the block-linear copy exists: the switch below allocates nothing
    res = np.zeros((5, 65, 4), dtype=np.float32)
    outs = [np.zeros((5, 65, 3), dtype=np.float32) for _ in range(4)]
    for o in outs:
        dev.pin(o)
    try:
        post.SetTexture(0, tb)
        assert win.PresentWait(win.PresentPostAsync(post, outs[3]))   # first use allocates a staging buffer
        assert win.PresentWait(win.PresentPostAsync(post, outs[3]))   # ... and the other slot's
        s0 = dev.sync_count()
        post.SetTexture(0, ta)
        t0 = win.PresentPostAsync(post, outs[0])                      # ta, nearest
        post.SetTexture(0, tb)                                        # rebound between the calls
        t1 = win.PresentPostAsync(post, outs[1])                      # tb
        post.SetTexture(0, ta)
        ta.SetBilinear(True)                                          # the filter switched between the calls
        assert win.PresentWait(t0)
        t2 = win.PresentPostAsync(post, outs[2])                      # ta, bilinear
        ta.SetBilinear(False)                                         # too late for the present just made
        post.SetTexture(0, None)
        assert dev.sync_count() == s0
        assert win.PresentWait(t1) and win.PresentWait(t2)
        wants = [((X.texture((8, 8)), False),), ((X.texture((8, 8), seed=1), False),), ((X.texture((8, 8)), True),)]
        for i, slot0 in enumerate(wants):
            assert_same_words(outs[i], X.sample_twin(res, k, slot0 + (None, None, None))[..., :3], ("present", i))
        # the wrong twin: the filter as it was at bind time
        assert not np.array_equal(outs[2], X.sample_twin(res, k, ((X.texture((8, 8)), False), None, None, None))[..., :3])
    finally:
        dev.sync()
        for o in outs:
            dev.unpin(o)
    post.close(); ta.Dispose(); tb.Dispose(); dev.close()


def test_a_present_sees_the_texture_updates_enqueued_before_it_and_not_those_after(device, posts):
    out_size = (65, 5)
    win = MainWindow(device, *out_size)
    first, second = P.planes(out_size, (1, 1), "pool")[0], P.planes((65, 5), (2, 1), "pool")[0][:5, :65]
    tex = Texture.Target(device, *out_size)
    nbytes = 65 * 5 * 4
    a, b = DeviceBytes(nbytes), DeviceBytes(nbytes)
    try:
        posts["TEXEL"].SetConstants([0, 0])
        posts["TEXEL"].SetTexture(0, tex)
        for s in (1, 2, 3):
            posts["TEXEL"].SetTexture(s, None)
        win.Upload(color=first)
        tex.UpdateFrom(win, keep_alpha=True)
        win.Upload(color=second)
        s0 = device.sync_count()
        win.PostTo(posts["TEXEL"], a.ptr.value, 1, 1, 4, np.uint8, wait=False)       # enqueued before the update: the old texels
        tex.UpdateFrom(win, keep_alpha=True)
        win.PostTo(posts["TEXEL"], b.ptr.value, 1, 1, 4, np.uint8, wait=False)       # after it: the new
        assert device.sync_count() == s0
        device.sync()
        old, new = X.T.texels(first, 1, 1, keep_alpha=True), X.T.texels(second, 1, 1, keep_alpha=True)
        assert not np.array_equal(old, new)
        for buf, texels in ((a, old), (b, new)):
            want = P.deliver(X.texel_twin(np.zeros((5, 65, 4), dtype=np.float32), P.constants64(), ((texels, False), None, None, None))[..., :3], P.RGBX8)
            same_bytes(buf.read().reshape(5, 65, 4), want, "old" if buf is a else "new")
    finally:
        posts["TEXEL"].SetTexture(0, None)
        a.free(); b.free(); tex.Dispose()


# ------------------------------------------------------------------------------------------------------------- 5. destroy
def test_destroying_a_bound_texture_unbinds_it_everywhere(device, posts):
    win = MainWindow(device, 65, 5)
    k = X.uv_constants((65, 5))
    res = np.zeros((5, 65, 4), dtype=np.float32)
    t = Texture(device, X.texture((5, 3)))
    keep = Texture(device, X.texture((8, 8)))
    try:
        for slot, tex in enumerate((t, keep, t, None)):
            posts["FOUR"].SetTexture(slot, tex)
        posts["SAMPLE"].SetTexture(0, t)
        slots = ((X.texture((5, 3)), False), (X.texture((8, 8)), False), (X.texture((5, 3)), False), None)
        assert_same_words(run(win, posts["FOUR"], k), X.four_twin(res, k, slots)[..., :3], "before")
        t.Dispose()
        assert np.all(run(win, posts["SAMPLE"], k) == 1.0)            # "no texture" there
        assert_same_words(run(win, posts["FOUR"], k), X.four_twin(res, k, (None, slots[1], None, None))[..., :3], "after")
        again = Texture(device, X.texture((5, 3)))                    # the context is usable, the slot can be bound again
        posts["SAMPLE"].SetTexture(0, again)
        assert_same_words(run(win, posts["SAMPLE"], k), X.sample_twin(res, k, (slots[0], None, None, None))[..., :3], "rebound")
        again.Dispose()
    finally:
        keep.Dispose()
        for s in range(4):
            posts["FOUR"].SetTexture(s, None)


# ------------------------------------------------------------------------------------------------ 6. a pass into a texture
@pytest.mark.parametrize("out_size", P.OUT_SIZES)
def test_the_texels_of_a_pass_equal_the_twin_under_both_alpha_modes(device, posts, textures, out_size):
    w, h = out_size
    tex, ref = Texture.Target(device, w, h), Texture.Target(device, w, h)
    k = X.uv_constants(out_size, reverse=True)
    slots = bind(posts["SAMPLE"], textures, [((5, 3), True), None, None, None])
    posts["SAMPLE"].SetConstants(k)
    try:
        for factors in P.FACTORS:
            color, depth = P.planes(out_size, factors, "pool")
            win = MainWindow(device, color.shape[1], color.shape[0])
            win.Upload(color=color, depth=depth)
            for keep in (False, True):
                for name, constants, s in (("BLUR_H", (), X.NO_SLOTS), ("SAMPLE", k, slots), ("IDENTITY", (), X.NO_SLOTS)):
                    tex.UpdateFromPost(win, posts[name], *factors, keep_alpha=keep)
                    got = tex.Read()
                    r = X.result(name, color, *factors, constants, s)
                    same_bytes(got, X.texels(r, keep_alpha=keep), (name, out_size, factors, keep))
                    if name == "BLUR_H":
                        same_bytes(got[..., :3], win.PostBuffer(posts[name], *factors, 4, np.uint8)[..., :3], "RGBX8's bytes")
                        if keep and out_size != (1, 1):                # the wrong twin: alpha from the frame
                            assert not np.array_equal(got, X.texels_alpha_from_frame(r, color, *factors))
                    if name == "IDENTITY":
                        ref.UpdateFrom(win, *factors, keep_alpha=keep)
                        same_bytes(got, ref.Read(), ("against swr_texture_update_from_frame", out_size, factors, keep))
    finally:
        tex.Dispose(); ref.Dispose()


@pytest.mark.parametrize("tex_size", [(64, 4), (8, 8), (136, 12)])
@pytest.mark.parametrize("filter_first", [True, False])
def test_the_block_linear_copy_is_fresh_after_a_pass(device, posts, tex_size, filter_first):
    w, h = tex_size
    view = MainWindow(device, 65, 5)
    k = X.uv_constants((65, 5))
    res = np.zeros((5, 65, 4), dtype=np.float32)
    tex = Texture.Target(device, w, h)
    try:
        if filter_first:
            tex.SetBilinear(True)                                      # the copy exists (of zeros) before the first pass
        for n, (factors, keep) in enumerate((((1, 1), False), ((2, 2), True))):
            color = P.planes(tex_size, factors, "pool")[0] if tex_size in P.OUT_SIZES else P.color_plane(w * factors[0], h * factors[1], 50 + n, "pool")
            cam = MainWindow(device, w * factors[0], h * factors[1])
            cam.Upload(color=color)
            posts["SAMPLE"].SetTexture(0, None)
            tex.UpdateFromPost(cam, posts["BLUR_H"], *factors, keep_alpha=keep)
            if not filter_first:
                tex.SetBilinear(True)                                  # first time: built from the texels the pass left; then a no-op
            texels = tex.Read()
            same_bytes(texels, X.texels(X.result("BLUR_H", color, *factors), keep_alpha=keep), (tex_size, factors))
            posts["SAMPLE"].SetTexture(0, tex)
            got = run(view, posts["SAMPLE"], k)
            assert_same_words(got, X.sample_twin(res, k, ((texels, True), None, None, None))[..., :3], (tex_size, filter_first, n))
    finally:
        posts["SAMPLE"].SetTexture(0, None)
        tex.Dispose()


# ---------------------------------------------------------------------------------------------------------------- 7. chains
@pytest.mark.parametrize("out_size,factors", [((65, 5), (2, 1)), ((130, 9), (1, 1)), ((64, 4), (4, 2))])
@pytest.mark.parametrize("two_contexts", [False, True])
def test_a_separable_blur_is_two_calls(device, other, posts, out_size, factors, two_contexts):
    w, h = out_size
    color = P.planes(out_size, factors, "pool")[0]
    cam_dev = other if two_contexts else device
    cam = MainWindow(cam_dev, color.shape[1], color.shape[0])
    cam.Upload(color=color)
    blur_h = PostProgram(other, X.BLUR_H) if two_contexts else posts["BLUR_H"]
    a, t = Texture.Target(device, w, h), Texture.Target(device, w, h)
    try:
        if two_contexts:
            screen = MainWindow(device, w, h)                          # pass 2 runs over the screen context's own frame
            screen.Upload(color=np.zeros((h, w, 4), dtype=np.float32))
        syncs = device.sync_count(), other.sync_count()
        a.UpdateFromPost(cam, blur_h, *factors, keep_alpha=True)       # pass 1: the camera's frame, blurred along x, into A
        posts["BLUR_V"].SetTexture(0, a)
        if two_contexts:
            t.UpdateFromPost(screen, posts["BLUR_V"])                  # pass 2: A, blurred along y, into T
        else:
            t.UpdateFromPost(cam, posts["BLUR_V"], *factors)
        assert (device.sync_count(), other.sync_count()) == syncs      # nothing waited for the GPU
        want_a, want_t = X.blur_chain(color, *factors)
        same_bytes(t.Read(), want_t, ("T", out_size, factors, two_contexts))
        same_bytes(a.Read(), want_a, ("A", out_size, factors, two_contexts))
        if two_contexts:                                               # the camera's next frame waits for the pass that read this one
            cam.Upload(color=np.zeros_like(color))
            same_bytes(a.Read(), want_a, "A after the camera moved on")
    finally:
        posts["BLUR_V"].SetTexture(0, None)
        if two_contexts:
            blur_h.close()
        a.Dispose(); t.Dispose()


def test_ping_pong_accumulation_over_three_frames(device, posts):
    out_size = (65, 5)
    frames = [P.planes(out_size, f, "pool")[0][:5, :65] for f in ((1, 1), (2, 1), (1, 2))]
    win = MainWindow(device, *out_size)
    tex = [Texture.Target(device, *out_size), Texture.Target(device, *out_size)]
    try:
        for n, f in enumerate(frames):
            win.Upload(color=f)
            posts["ACCUM"].SetTexture(0, tex[(n + 1) % 2])
            with pytest.raises(_native.SwrError) as e:                 # a pass may not sample the texture it writes
                tex[(n + 1) % 2].UpdateFromPost(win, posts["ACCUM"], keep_alpha=True)
            assert e.value.code == INVALID
            tex[n % 2].UpdateFromPost(win, posts["ACCUM"], keep_alpha=True)
        want = X.accumulate(frames)
        same_bytes(tex[0].Read(), want[0], "texture 0"); same_bytes(tex[1].Read(), want[1], "texture 1")
        assert len(np.unique(want[0])) > 50
    finally:
        posts["ACCUM"].SetTexture(0, None)
        tex[0].Dispose(); tex[1].Dispose()


# ------------------------------------------------------------------------------------- 8. order against draws, no host wait
W, H = 128, 96


def feedback_frames(device, win, soups, post, use_update):
    """Three frames on one context.  Per frame: clear; a full-screen quad with the texture (the pass over frame N - 1), flushed on odd
    frames; a triangle soup, recorded and NOT flushed; the texture becomes the pass over the frame; a smaller quad with the texture (the
    pass over frame N).  use_update: swr_texture_update_from_post and nothing else; otherwise the host route -- the frame read back, the
    twin, a new texture -- with a swr_sync after every step."""
    I = hm.identity()
    tex = Texture.Target(device, W // 2, H // 2)
    prog = Shaders.Dust2LambertFog(default_uniforms(), tex)
    gouraud = Shaders.Gouraud()
    moved, texels = [], None
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
            tex.UpdateFromPost(win, post, 2, 2, keep_alpha=bool(n & 1))
            moved.append(device.sync_count() - before)
        else:
            texels = X.texels(X.result("BLUR_H", win.ColorBuffer, 2, 2), keep_alpha=bool(n & 1))
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
def test_draws_before_the_pass_see_the_old_texels_and_draws_after_it_the_new(device, posts, pipelining):
    soups = [scenes.cfg2(W, H, 60, seed=40 + n, min_area=30.0, max_area=900.0) for n in range(3)]
    win = MainWindow(device, W, H)
    was = device.pipelining()
    device.set_pipelining(pipelining)
    try:
        feedback_frames(device, win, soups, posts["BLUR_H"], use_update=True)        # sizes the pair buffers and the resolved plane
        device.sync()
        replays = device.replay_count()
        color, depth, texels, moved = feedback_frames(device, win, soups, posts["BLUR_H"], use_update=True)
        assert moved == [0, 0, 0], "swr_texture_update_from_post made the host wait"
        assert device.replay_count() == replays, "a batch was replayed: the comparison below would not be about ordering"
        ref = feedback_frames(device, win, soups, posts["BLUR_H"], use_update=False)
        same_words(color, ref[0], "colour after three frames"); same_words(depth, ref[1], "depth after three frames")
        same_bytes(texels, ref[2], "texels after three frames")
        assert len(np.unique(texels[..., :3])) > 50 and len(np.unique(texels[..., 3])) == 1      # the last frame's mode was opaque
    finally:
        device.set_pipelining(was)


# -------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_write_nothing_and_leave_everything_usable(device, other, posts, textures):
    lib, ctx = device._lib, device._ctx
    color = P.planes((64, 4), (1, 1), "pool")[0]
    win = MainWindow(device, 64, 4)
    win.Upload(color=color)
    tex = Texture.Target(device, 32, 2)
    good = posts["BLUR_H"]._id
    foreign = PostProgram(other, X.BLUR_H)
    gone = PostProgram(device, X.BLUR_H)
    gone_id = gone._id
    gone.close()

    def refused(code, words, t, src, pid, kx, ky, mode):
        syncs = device.sync_count(), other.sync_count()
        assert lib.swr_texture_update_from_post(ctx, t, src, pid, kx, ky, mode) == code, words
        assert words in lib.swr_last_error(ctx).decode(), (words, lib.swr_last_error(ctx).decode())
        assert (device.sync_count(), other.sync_count()) == syncs
    try:
        # the slots: a bad slot or id changes nothing
        slots = bind(posts["FOUR"], textures, [((8, 8), False), ((5, 3), False), None, ((1, 1), False)])
        for slot in (-1, 4, 5, 1 << 20):
            assert lib.swr_post_set_texture(ctx, posts["FOUR"]._id, slot, textures[(8, 8), True]._h) == INVALID
        for pid in (0, -1, 999999, gone_id, foreign._id):
            assert lib.swr_post_set_texture(ctx, pid, 0, textures[(8, 8), True]._h) == INVALID
        assert lib.swr_post_set_texture(None, posts["FOUR"]._id, 0, None) == INVALID
        k = X.uv_constants((64, 4))
        assert_same_words(run(win, posts["FOUR"], k), X.four_twin(np.zeros((4, 64, 4), dtype=np.float32), k, slots)[..., :3], "slots as they were")
        # a target bound to the program that would write it
        posts["SAMPLE"].SetTexture(3, tex)
        refused(INVALID, "may not sample the texture it writes", tex._h, None, posts["SAMPLE"]._id, 2, 2, 0)
        posts["SAMPLE"].SetTexture(3, None)
        # ids: unknown, destroyed, another context's (and this context's id with another context as the source)
        for pid in (0, -1, 999999, gone_id, foreign._id):
            refused(INVALID, "unknown or destroyed post program id", tex._h, None, pid, 2, 2, 0)
        cam = MainWindow(other, 64, 4)
        cam.Upload(color=color)
        refused(INVALID, "unknown or destroyed post program id", tex._h, other._ctx, good, 2, 2, 0)
        # whatever swr_texture_update_from_frame refuses
        refused(INVALID, "texture width * kx by texture height * ky", tex._h, None, good, 1, 1, 0)
        refused(INVALID, "texture width * kx by texture height * ky", tex._h, None, good, 2, 4, 0)
        for kx, ky in ((3, 2), (2, 0), (16, 2), (-1, 2)):
            refused(INVALID, "factors must be 1, 2, 4 or 8", tex._h, None, good, kx, ky, 0)
        for mode in (2, -1):
            refused(INVALID, "alpha_mode", tex._h, None, good, 2, 2, mode)
        refused(INVALID, "texture is null", None, None, good, 2, 2, 0)
        assert lib.swr_texture_update_from_post(None, tex._h, None, good, 2, 2, 0) == INVALID
        big = MainWindow(other, 64, 32)                                # two tile rows: a band of one of them
        big.SetBand(1, 1)
        wide = Texture.Target(device, 32, 16)
        refused(UNSUPPORTED, "only a band", wide._h, other._ctx, foreign._id, 2, 2, 0)
        big.SetBandInterleaved(0, 2, 1)
        refused(UNSUPPORTED, "only a band", wide._h, other._ctx, foreign._id, 2, 2, 0)
        big.SetBand(-1, -1)
        assert not wide.Read().any()
        wide.Dispose()
        assert not tex.Read().any(), "a refused pass wrote texels"
        # ... and both contexts still work: the refused calls, accepted, without a host wait
        cam = MainWindow(other, 64, 4)
        cam.Upload(color=color)
        win._activate()
        syncs = device.sync_count(), other.sync_count()
        tex.UpdateFromPost(cam, foreign, 2, 2, keep_alpha=True)
        tex.UpdateFromPost(cam, foreign, 2, 2, keep_alpha=True)
        assert (device.sync_count(), other.sync_count()) == syncs
        want = X.texels(X.result("BLUR_H", color, 2, 2), keep_alpha=True)
        same_bytes(tex.Read(), want, "from the other context")
        syncs = device.sync_count(), other.sync_count()
        tex.UpdateFromPost(win, posts["BLUR_H"], 2, 2)
        assert (device.sync_count(), other.sync_count()) == syncs
        same_bytes(tex.Read(), X.texels(X.result("BLUR_H", color, 2, 2)), "own frame")
    finally:
        for s in range(4):
            posts["FOUR"].SetTexture(s, None)
        posts["SAMPLE"].SetTexture(3, None)
        foreign.close()
        tex.Dispose()
