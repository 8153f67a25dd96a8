"""Depth textures on the GPU (include/swr.h, csrc/swr_deliver.hip.h, csrc/swr_device.h): k_depth_to_texture
against the numpy restatement of tests/depth_texture_cases.py, its block-linear copy through the host-callable lookups, the three
lookups in both halves of a user program and in a post program, a cast shadow between two contexts, the ordering of
swr_texture_update_from_depth against the draws around it without a host synchronisation, and the refusals.  No tolerance anywhere:
every comparison is made on 32-bit words (a NaN that went through a program's result is matched by any NaN)."""
import ctypes as C

import numpy as np
import pytest

import depth_texture_cases as D
import post_cases as P
import post_texture_cases as X
import program_probe_cases as PC
import program_texture_cases as PT
from softwarerenderer_amd import (BlendMode, CullMode, DepthReduce, DepthTest, Device, MainWindow, PostProgram, Rasterizer, Shaders,
                                  Texture, _native, hostmath as hm, scenes)
from softwarerenderer_amd.rasterizer import ShaderProgram
from test_gpu_parity import run_both
from test_gpu_program_probe import assert_words
from test_gpu_program_textures import render as render_probe
from test_gpu_render_to_texture import QUAD, QUAD_IDX, hip_device_count

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, UNSUPPORTED = _native.SWR_ERR_INVALID_ARG, _native.SWR_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def other():
    """A second context on the same GPU: the light, or the camera whose depth becomes the first context's texture."""
    dev = Device(0)
    yield dev
    dev.close()


@pytest.fixture(scope="module")
def programs(device):
    """name -> program id, compiled when a test first asks for it."""
    class Compiled(dict):
        def __missing__(self, name):
            vertex, fragment = D.TEXTS[name]
            self[name] = device.compile_program(fragment, vertex_source=vertex)
            return self[name]
    ids = Compiled()
    yield ids
    for pid in ids.values():
        device.destroy_program(pid)


@pytest.fixture(scope="module")
def post_probe(device):
    p = PostProgram(device, D.POST_PROBE)
    yield p
    p.close()


def same_words(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(D.words(got) != D.words(want))
    assert bad.size == 0, (what, f"{len(bad)} words differ, first at {tuple(bad[0])}: got {D.words(got)[tuple(bad[0])]:08x} "
                                 f"want {D.words(want)[tuple(bad[0])]:08x}")


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("tex_size,factors", D.GPU_SHAPES)
def test_texels_equal_the_restatement_under_every_reduction(device, post_probe, tex_size, factors):
    (w, h), (kx, ky) = tex_size, factors
    fw, fh = D.source_size(tex_size, factors)
    plane = D.depth_pool_plane(fh, fw, 100 + w)
    win = MainWindow(device, fw, fh)
    win.Upload(depth=plane)
    tex = Texture.Depth(device, w, h)
    host = Texture.Depth(device, w, h, D.reduce(plane, kx, ky, D.MIN))
    try:
        assert tex.Format == D.DEPTH32F and (D.words(tex.ReadDepth()) == 0xff7fffff).all(), "a new depth texture is not float.MinValue"
        same_words(host.ReadDepth(), D.reduce(plane, kx, ky, D.MIN), "a host-created texture reads back its input")
        got = {}
        for mode in D.REDUCTIONS:
            tex.UpdateFromDepth(win, kx, ky, DepthReduce(mode))
            got[mode] = tex.ReadDepth()
            same_words(got[mode], D.reduce(plane, kx, ky, mode), (tex_size, factors, mode))
        k = P.constants64().copy()
        k[6] = 1.0                                     # the post probe's other mode: swr_post_depth at its own pixel
        post_probe.SetConstants(k)
        same_words(win.PostBuffer(post_probe, kx, ky, 3, np.float32)[..., 0], got[D.FIRST], "FIRST is the word swr_post_depth reads")
        if (kx, ky) != (1, 1):
            assert (D.words(got[D.MAX]) != D.words(got[D.MIN])).any() and (D.words(got[D.MAX]) != D.words(got[D.FIRST])).any()
    finally:
        tex.Dispose(); host.Dispose()


# --------------------------------------------------------------------------------------------------- 2. the block-linear copy
def check_lookups(tex, depth, bilinear, what):
    """SampleDepth under the texture's present filter against the restatement, at centres, corners, wraps and negatives."""
    h, w = depth.shape
    uv = D.lookup_uvs(w, h)
    ref = D.lookup_refs(len(uv), seed=w)
    slots = ((depth, bilinear), None, None, None)
    got_depth, got_shadow = tex.SampleDepth(uv, ref)
    same_words(got_depth, D.depth_sample(slots, 0, uv), what + ("depth",))
    want = D.shadow(slots, 0, uv, ref)
    same_words(got_shadow, want, what + ("shadow",))
    assert (want == 0).any() and (want == 1).any()
    if bilinear:
        assert ((want > 0) & (want < 1)).any()
    centres = D.texel_centres(w, h)
    same_words(tex.SampleDepth(centres, F32(0.5))[0], depth, what + ("centres",))


@pytest.mark.parametrize("tex_size,factors", D.BLOCKED_SHAPES)
@pytest.mark.parametrize("filter_first", [True, False])
def test_the_bilinear_copy_is_written_by_the_update_and_refreshed_by_the_next(device, other, tex_size, factors, filter_first):
    (w, h), (kx, ky) = tex_size, factors
    fw, fh = D.source_size(tex_size, factors)
    cam = MainWindow(other, fw, fh)                    # the source in another context
    tex = Texture.Depth(device, w, h)
    seen = []
    try:
        if filter_first:
            tex.SetBilinear(True)                     # the block-linear copy exists (of float.MinValue) before the first update
        for seed, mode in ((200 + w, D.MAX), (300 + w, D.MIN)):
            plane = D.depth_pool_plane(fh, fw, seed)
            want = D.reduce(plane, kx, ky, mode)
            cam.Upload(depth=plane)
            tex.UpdateFromDepth(cam, kx, ky, mode)
            tex.SetBilinear(True)                     # the first time without filter_first: built from the texels the update left
            check_lookups(tex, want, True, (tex_size, factors, filter_first, seed))          # through the block-linear copy
            tex.SetBilinear(False)
            check_lookups(tex, want, False, (tex_size, factors, filter_first, seed))         # row-major
            same_words(tex.ReadDepth(), want, "row-major texels")
            tex.SetBilinear(True)
            seen.append(want)
        assert (D.words(seen[0]) != D.words(seen[1])).any()
    finally:
        tex.Dispose()


# ------------------------------------------------------------------------------------------------------ 3. the program contract
@pytest.fixture(scope="module")
def depth_textures(device):
    """name -> (live Texture, its words).  "12x20": a 24 x 40 pool plane through the kernel under (2, 2) MAX; "12x20min": the same plane
    under MIN; "8x8", "5x3": host-created from pool planes; "f12x20", "f8x8": finite words, for values that meet the interpolator."""
    win = MainWindow(device, 24, 40)
    plane = D.depth_pool_plane(40, 24, 7)
    win.Upload(depth=plane)
    made = {}
    for name, mode in (("12x20", D.MAX), ("12x20min", D.MIN)):
        t = Texture.Depth(device, 12, 20)
        t.UpdateFromDepth(win, 2, 2, mode)
        made[name] = (t, D.reduce(plane, 2, 2, mode))
    for name, words in (("8x8", D.depth_pool_plane(8, 8, 8)), ("5x3", D.depth_pool_plane(3, 5, 9)),
                        ("f12x20", D.finite_plane(20, 12, 1)), ("f8x8", D.finite_plane(8, 8, 2))):
        made[name] = (Texture.Depth(device, words.shape[1], words.shape[0], words), words)
    yield made
    for t, _ in made.values():
        t.Dispose()


def bind(depth_textures, spec, bilinear):
    """spec: four names or None -> (the live Textures under that filter, the twin's slots)."""
    for n in spec:
        if n is not None:
            depth_textures[n][0].SetBilinear(bilinear)
    return (tuple(None if n is None else depth_textures[n][0] for n in spec),
            tuple(None if n is None else (depth_textures[n][1], bilinear) for n in spec))


def probe_frame(device, pid, scene, k, tex, slots, what):
    want, n = PT.expected_frame(scene, lambda j, xs, ys: D.fragment_probe_twin(k, slots, xs, ys))
    c, st = render_probe(device, scene, pid, [(k, tex)] * len(scene.draws))
    assert_words(c, want, what)
    assert st["fragments_written"] == n > 0, (what, st["fragments_written"], n)
    return c


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "2x2"])
@pytest.mark.parametrize("slot", [0, 2, PT.PER_PIXEL], ids=["slot0", "slot2", "per_pixel"])
def test_the_fragment_half_reads_depth_words_and_shadows(device, programs, depth_textures, slot, bilinear):
    s = PC.wide()
    k = PT.constants(s.width, s.height, slot=slot)
    spec = ("12x20", None, "8x8", "5x3")               # slot 1 unbound; per pixel: slot 4 out of range as well
    tex, slots = bind(depth_textures, spec, bilinear)
    c = probe_frame(device, programs["FRAGMENT_PROBE"], s, k, tex, slots, f"fragment/{slot}/{bilinear}")
    covered = PT.coverage(s)[1] > 0
    assert len(np.unique(c[covered][:, 1].view(np.uint32))) > 20, "the probe saw no texture"
    # unbound: float.MinValue, and every fragment lit
    u = probe_frame(device, programs["FRAGMENT_PROBE"], s, k, (None,) * 4, D.NO_SLOTS, f"fragment/{slot}/{bilinear}/unbound")
    assert (u[covered][:, 0] == 1).all() and (u[covered][:, 1:3].view(np.uint32) == 0xff7fffff).all()
    if slot == 0:
        # the reduction shows through the program: the MIN texture in the MAX texture's place is another frame
        tex2, slots2 = bind(depth_textures, ("12x20min",) + spec[1:], bilinear)
        m = probe_frame(device, programs["FRAGMENT_PROBE"], s, k, tex2, slots2, f"fragment/{slot}/{bilinear}/min")
        assert (c.view(np.uint32) != m.view(np.uint32)).any()


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "2x2"])
def test_the_vertex_half_reads_the_same_words(device, programs, depth_textures, bilinear):
    from vertex_probe_cases import nm_flags
    scene = PT.vertex_scene()
    flags = nm_flags(*device.transform_fma())
    tex, slots = bind(depth_textures, ("f12x20", "f8x8", None, None), bilinear)
    stages = [D.vertex_probe_stage(d, flags, slots) for d in scene.draws]
    drawn = np.concatenate([st["data4"][np.unique(d.indices)] for st, d in zip(stages, scene.draws)])
    assert len(drawn) == len(PT.VERTEX_UVS) and len(np.unique(drawn[:, 0])) > 1 and len(np.unique(drawn[:, 1])) > 4
    planes, count = PC.expected_planes(scene, tris=PC.probe_tris(scene, lambda j, d: stages[j]))
    covered = int((count > 0).sum())
    assert count.max() == 1 and covered > 0 and D.VERTEX_GROUPS
    for g in D.VERTEX_GROUPS:
        k = PC.selector_constants(g)
        c, st = render_probe(device, scene, programs["VERTEX_PROBE"], [(k, tex)] * 2)
        assert_words(c, PC.expected_colour(scene, PC.group_names(g), planes, count), f"vertex/{bilinear}/{'+'.join(PC.group_names(g))}")
        assert st["fragments_written"] == covered


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "2x2"])
def test_a_post_program_reads_the_same_words(device, post_probe, depth_textures, bilinear):
    out_size = (65, 5)
    win = MainWindow(device, *out_size)
    spec = ("12x20", None, "8x8", "5x3")
    tex, slots = bind(depth_textures, spec, bilinear)
    try:
        for slot in (0, 2, PT.PER_PIXEL, 1, -1):
            for bound in (True, False):
                for i in range(4):
                    post_probe.SetTexture(i, tex[i] if bound else None)
                k = X.uv_constants(out_size).copy()
                k[4], k[5], k[D.SLOT] = -2, 1, slot
                post_probe.SetConstants(k)
                got = win.PostBuffer(post_probe, 1, 1, 3, np.float32)
                want = D.post_probe_twin(out_size[1], out_size[0], k, slots if bound else D.NO_SLOTS)
                assert_words(got, want, f"post/{slot}/{bilinear}/{bound}")
                if not bound or slot in (1, -1):
                    assert (got[..., 0] == 1).all() and (got[..., 1:].view(np.uint32) == 0xff7fffff).all()
    finally:
        for i in range(4):
            post_probe.SetTexture(i, None)


# ------------------------------------------------------------------------------------------------------ 4. a shadow, end to end
LIGHT, TEXELS = 128, 64                                # the light's frame; its depth texture under (2, 2)
FLOOR_Z, OCCLUDER_Z = 0.5, -0.5                        # stored depth -(z + 1) / 2: -0.75 and -0.25 -- the larger is the nearer
OCCLUDER = (-0.3125, 0.1875, -0.25, 0.375)             # x0, x1, y0, y1 in the light's clip space: on pixel edges of its 128 x 128 frame
LIT, DARK = (1.0, 0.75, 0.5), (0.25, 0.25, 0.5)        # LIT - DARK is exact, and DARK + (LIT - DARK) is LIT


def quad(x0, x1, y0, y1, z):
    return scenes.make_vertices([(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)])


FLOOR = quad(-0.875, 0.875, -0.875, 0.875, FLOOR_Z)
# the screen's camera: the floor turned by 30 degrees and shrunk, so that texels and screen pixels do not line up
CAMERA = np.array([[0.8 * np.cos(np.pi / 6), 0.8 * np.sin(np.pi / 6), 0, 0], [-0.8 * np.sin(np.pi / 6), 0.8 * np.cos(np.pi / 6), 0, 0],
                   [0, 0, 1, 0], [0.05, -0.1, 0, 1]], dtype=F32)


def light_frame(win):
    """The floor and the occluder as the light sees them (its clip space is the world: identity matrices)."""
    I = hm.identity()
    g = Shaders.Gouraud()
    win.ClearDepthBuffer(); win.ClearColorBuffer((0, 0, 0, 1))
    for mesh in (FLOOR, quad(*OCCLUDER, OCCLUDER_Z)):
        Rasterizer.RenderMesh(win, mesh, QUAD_IDX, I, I, I, g.VertexShader, g.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.Alpha)


def screen_frame(device, win, pid, shadow_map):
    """The floor under the recipe program with `shadow_map` in slot 1; (colour, depth, stats)."""
    I = hm.identity()
    k = np.zeros(64, dtype=F32)
    k[:16] = I.reshape(-1)                             # the light's view * projection
    k[16] = 1.0 / 1024.0                               # the bias
    k[17:20], k[20:23] = LIT, DARK
    device.set_program_constants(pid, k)
    device.set_program_texture(pid, 1, shadow_map)
    prog = ShaderProgram(pid)
    win.ClearDepthBuffer(); win.ClearColorBuffer((0, 0, 0, 1))
    device.reset_stats()
    Rasterizer.RenderMesh(win, FLOOR, QUAD_IDX, I, CAMERA, I, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.None_)
    c, z = win._read(True, True)
    st = device.stats()
    device.set_program_texture(pid, 1, None)
    return c, z, st


def test_a_light_in_one_context_shadows_a_floor_in_another(device, other, programs):
    W, H = 160, 112
    light = MainWindow(other, LIGHT, LIGHT)
    screen = MainWindow(device, W, H)
    tex = Texture.Depth(device, TEXELS, TEXELS)
    tex.SetBilinear(True)
    try:
        light_frame(light)                              # recorded, not flushed: the update completes the frame
        tex.UpdateFromDepth(light, 2, 2, DepthReduce.Max)
        got = screen_frame(device, screen, programs["SHADOW"], tex)
        host_map = D.reduce(light.DepthBuffer.reshape(LIGHT, LIGHT), 2, 2, D.MAX)
        same_words(tex.ReadDepth(), host_map, "texels against swr_readback's depth through the restatement")
        assert (D.words(host_map) == 0xff7fffff).any() and list(np.unique(np.round(host_map[host_map > D.MINVALUE], 3))) == [-0.75, -0.25]
        ref_tex = Texture.Depth(device, TEXELS, TEXELS, host_map)
        ref_tex.SetBilinear(True)
        ref = screen_frame(device, screen, programs["SHADOW"], ref_tex)
        ref_tex.Dispose()
        same_words(got[0], ref[0], "colour"); same_words(got[1], ref[1], "depth")
        assert got[2] == ref[2] and got[2]["fragments_written"] > 0
        # where is each screen pixel in the light's texture?  In float64, through the inverse of the camera (w = 1 throughout)
        ys, xs = np.mgrid[0:H, 0:W]
        ndc = np.stack([(xs + 0.5) / W * 2 - 1, 1 - (ys + 0.5) / H * 2, np.zeros((H, W)), np.ones((H, W))], axis=-1)
        world = ndc @ np.linalg.inv(CAMERA.astype(np.float64))
        tx, ty = (world[..., 0] * 0.5 + 0.5) * TEXELS, (1 - (world[..., 1] * 0.5 + 0.5)) * TEXELS
        ox0, ox1 = (OCCLUDER[0] * 0.5 + 0.5) * TEXELS, (OCCLUDER[1] * 0.5 + 0.5) * TEXELS
        oy0, oy1 = (1 - (OCCLUDER[3] * 0.5 + 0.5)) * TEXELS, (1 - (OCCLUDER[2] * 0.5 + 0.5)) * TEXELS
        on_floor = (np.abs(world[..., 0]) < 0.875 - 3 * 2 / TEXELS) & (np.abs(world[..., 1]) < 0.875 - 3 * 2 / TEXELS)
        inside = (tx > ox0 + 3) & (tx < ox1 - 3) & (ty > oy0 + 3) & (ty < oy1 - 3)
        outside = on_floor & ((tx < ox0 - 3) | (tx > ox1 + 3) | (ty < oy0 - 3) | (ty > oy1 + 3))
        assert inside.sum() > 200 and outside.sum() > 2000
        assert (got[0][inside] == np.array(DARK + (1.0,), dtype=F32)).all(), "a pixel well inside the occluder's shadow is not the shadowed colour"
        assert (got[0][outside] == np.array(LIT + (1.0,), dtype=F32)).all(), "a pixel well outside the shadow is not the lit colour"
        rim = got[0][on_floor & ~inside & ~outside][:, 0]
        assert ((rim > DARK[0]) & (rim < LIT[0])).any(), "no pixel between lit and shadowed: the 2 x 2 filter shows nowhere"
    finally:
        tex.Dispose()


# ------------------------------------------------------------------------------------- 5. order, no host synchronisation
W, H = 128, 96


def feedback_frames(device, win, pid, soups, use_update):
    """Three frames of a feedback loop on one context.  Per frame: clear; a quad under the fragment probe reading the depth texture
    (frame N - 1's depth) in slot 0, flushed on odd frames; a triangle soup, recorded and NOT flushed; the texture becomes the frame's
    depth under (2, 2); a second, smaller and nearer quad under the probe (frame N's depth).  use_update:
    swr_texture_update_from_depth and nothing else; otherwise the host route -- swr_readback, the restatement,
    swr_texture_create_depth -- with a swr_sync after every step.  Returns (colour, depth, texels) after the third frame and the sync
    counts seen."""
    I = hm.identity()
    tex = Texture.Depth(device, W // 2, H // 2)
    gouraud = Shaders.Gouraud()
    k = PT.constants(W, H, slot=0, texel_span=(W // 2 + 4, H // 2 + 4), lo=-0.5, hi=1.5)
    moved = []
    step = (lambda: None) if use_update else device.sync
    for n in range(3):
        big = QUAD.copy()
        big["position"][:, 2] = -0.5
        small = QUAD.copy()
        small["position"][:, :2] *= F32(0.5)
        small["position"][:, 2] = -0.9
        device.set_program_constants(pid, k)
        probe = ShaderProgram(pid, None, tex)
        win.ClearDepthBuffer(); win.ClearColorBuffer((0.2 * n, 0.9 - 0.3 * n, 0.5, 1.0)); step()
        Rasterizer.RenderMesh(win, big, QUAD_IDX, I, I, I, probe.VertexShader, probe.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.None_)
        if n & 1:
            device.flush()
        step()
        d = soups[n].draws[0]
        Rasterizer.RenderMesh(win, d.vertices, d.indices, d.model, d.view, d.projection, gouraud.VertexShader, gouraud.FragmentShader,
                              d.cull, d.depth_test, d.blend)
        step()
        mode = D.REDUCTIONS[n]
        if use_update:
            before = device.sync_count()
            tex.UpdateFromDepth(win, 2, 2, mode)
            moved.append(device.sync_count() - before)
        else:
            texels = D.reduce(win.DepthBuffer.reshape(H, W), 2, 2, mode)
            old, tex = tex, Texture.Depth(device, W // 2, H // 2, texels)
            old.Dispose(); step()
        probe = ShaderProgram(pid, None, tex)
        Rasterizer.RenderMesh(win, small, QUAD_IDX, I, I, I, probe.VertexShader, probe.FragmentShader, CullMode.None_, DepthTest.Always, BlendMode.None_)
        step()
    color, depth = win._read(True, True)
    texels = tex.ReadDepth() if use_update else texels
    tex.Dispose()
    return color, depth, texels, moved


@pytest.mark.parametrize("pipelining", [0, 1, 2])
def test_draws_before_the_update_see_the_old_depth_and_draws_after_it_the_new(device, programs, pipelining):
    soups = [scenes.cfg2(W, H, 60, seed=40 + n, min_area=30.0, max_area=900.0) for n in range(3)]
    win = MainWindow(device, W, H)
    pid = programs["FRAGMENT_PROBE"]
    was = device.pipelining()
    device.set_pipelining(pipelining)
    try:
        feedback_frames(device, win, pid, soups, use_update=True)          # sizes the pair buffers of every raster set in use
        device.sync()
        replays = device.replay_count()
        color, depth, texels, moved = feedback_frames(device, win, pid, soups, use_update=True)
        assert moved == [0, 0, 0], "swr_texture_update_from_depth made the host wait"
        assert device.replay_count() == replays, "a batch was replayed: the comparison below would not be about ordering"
        ref = feedback_frames(device, win, pid, soups, use_update=False)
        assert_words(color, ref[0], "colour after three frames")
        same_words(depth, ref[1], "depth after three frames")
        same_words(texels, ref[2], "texels after three frames")
        assert len(np.unique(texels)) > 50
    finally:
        device.set_pipelining(was)


# ------------------------------------------------------------------------------------------------------------ a plain-C caller
def test_a_plain_c_caller_reduces_and_looks_up_through_the_abi():
    """tests/c/depth_texture_smoke.c: gcc + dlopen, no C++ / HIP headers."""
    import os
    import spawner
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c")
    spawner.run(["make", "-C", here, "-f", "depth_texture_smoke.mk", "-s"], check=True)
    out = spawner.run([os.path.join(here, "depth_texture_smoke"), _native.LIB_PATH], timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wrong=0 refused=-1" in out.stdout


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_textures_and_the_context_alone(device, other):
    lib, ctx = device._lib, device._ctx
    win = MainWindow(device, 64, 32)
    plane = D.depth_pool_plane(32, 64, 7)
    win.Upload(depth=plane, color=np.full((32, 64, 4), 0.5, dtype=F32))
    first = D.depth_pool_plane(16, 32, 11)
    tex = Texture.Depth(device, 32, 16, first)
    rgba = Texture.Target(device, 32, 16)
    out4, out1, uv = np.zeros((16, 32, 4), dtype=np.uint8), np.zeros((16, 32), dtype=F32), np.zeros(3, dtype=F32)

    def refused(code, words, rc):
        assert rc == code, (words, rc)
        assert words in lib.swr_last_error(ctx).decode(), (words, lib.swr_last_error(ctx).decode())

    def update(t, src, kx, ky, reduce):
        syncs = device.sync_count()
        rc = lib.swr_texture_update_from_depth(ctx, t, src, kx, ky, reduce)
        assert device.sync_count() == syncs
        return rc
    try:
        refused(INVALID, "texture width * kx by texture height * ky", update(tex._h, None, 1, 1, 0))       # 32 x 16 from 64 x 32
        refused(INVALID, "texture width * kx by texture height * ky", update(tex._h, None, 2, 4, 0))
        for kx, ky in ((3, 2), (2, 0), (16, 2)):
            refused(INVALID, "factors must be 1, 2, 4 or 8", update(tex._h, None, kx, ky, 0))
        for reduce in (3, -1):
            refused(INVALID, "reduce must be", update(tex._h, None, 2, 2, reduce))
        refused(INVALID, "texture is null", update(None, None, 2, 2, 0))
        # the format, in both directions: depth calls on an RGBA8 texture ...
        refused(INVALID, "not a depth texture", update(rgba._h, None, 2, 2, 0))
        refused(INVALID, "not a depth texture", lib.swr_texture_readback_depth(ctx, rgba._h, out1.ctypes.data))
        refused(INVALID, "not a depth texture", lib.swr_texture_sample_depth(ctx, rgba._h, uv.ctypes.data, 1, out1.ctypes.data))
        # ... and colour calls on a depth texture
        refused(INVALID, "is a depth texture", lib.swr_texture_update_from_frame(ctx, tex._h, None, 2, 2, 0))
        identity = PostProgram(device, P.IDENTITY)
        refused(INVALID, "is a depth texture", lib.swr_texture_update_from_post(ctx, tex._h, None, identity._id, 2, 2, 0))
        identity.close()
        refused(INVALID, "is a depth texture", lib.swr_texture_readback(ctx, tex._h, out4.ctypes.data))
        refused(INVALID, "is a depth texture", lib.swr_texture_sample(ctx, tex._h, uv.ctypes.data, 1, out1.ctypes.data))
        assert not out4.any() and not out1.any(), "a refused read wrote its destination"
        # a source that holds a band of its frame: a contiguous band, then interleaved stripes
        cam = MainWindow(other, 64, 32)
        cam.SetBand(1, 1)
        refused(UNSUPPORTED, "only a band", update(tex._h, other._ctx, 2, 2, 0))
        cam.SetBandInterleaved(0, 2, 1)
        refused(UNSUPPORTED, "only a band", update(tex._h, other._ctx, 2, 2, 0))
        cam.SetBand(-1, -1)
        if hip_device_count() > 1:
            far = Device(1)
            try:
                MainWindow(far, 64, 32)
                refused(UNSUPPORTED, "another device", update(tex._h, far._ctx, 2, 2, 0))
            finally:
                far.close()
        with pytest.raises(_native.SwrError) as e:
            tex.UpdateFromDepth(win, 4, 2)
        assert e.value.code == INVALID
        # creation: the limits of swr_texture_create; the other arguments
        h = C.c_void_p()
        for bad in ((0, 4), (4, -1)):
            assert lib.swr_texture_create_depth(ctx, None, bad[0], bad[1], C.byref(h)) == INVALID and not h.value
        assert lib.swr_texture_create_depth(ctx, None, 4, 4, None) == INVALID
        assert lib.swr_texture_create_depth(ctx, None, 1 << 15, 1 << 15, C.byref(h)) == UNSUPPORTED and not h.value
        assert lib.swr_texture_readback_depth(ctx, tex._h, None) == INVALID
        assert lib.swr_texture_sample_depth(ctx, tex._h, None, 1, out1.ctypes.data) == INVALID
        assert lib.swr_texture_format(ctx, None, C.byref(C.c_int())) == INVALID and lib.swr_texture_format(ctx, tex._h, None) == INVALID
        assert (tex.Format, rgba.Format) == (D.DEPTH32F, D.RGBA8)
        # nothing was written
        same_words(tex.ReadDepth(), first, "a refused update wrote texels")
        assert not rgba.Read().any(), "a refused update wrote texels"
        # ... and both contexts still work: the refused calls, accepted; then a parity frame
        cam.Upload(depth=plane)
        tex.UpdateFromDepth(cam, 2, 2, DepthReduce.Min)
        same_words(tex.ReadDepth(), D.reduce(plane, 2, 2, D.MIN), "after the refusals, from the other context")
        tex.UpdateFromDepth(win, 2, 2)
        same_words(tex.ReadDepth(), D.reduce(plane, 2, 2, D.MAX), "after the refusals, own frame")
        rgba.UpdateFrom(win, 2, 2)
        assert (rgba.Read()[..., :3] == 128).all()
    finally:
        tex.Dispose(); rgba.Dispose()
    run_both(device, scenes.cfg2(160, 120, 200, seed=3))
