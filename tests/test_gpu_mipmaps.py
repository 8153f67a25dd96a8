"""Mip chains on the GPU (include/swr.h, csrc/swr_deliver.hip.h, csrc/swr_device.h): k_mip_downsample against
the integer restatement of tests/mipmap_cases.py, the chain kept up to date by the texture updates, the lookups by level, lod and
gradient through the host-callable batches, in both halves of a user program and in a post program, the ordering of
swr_texture_generate_mipmaps against the draws around it without a host synchronisation, and the refusals.  No tolerance anywhere:
bytes are compared as bytes and floats as 32-bit words."""
import ctypes as C

import numpy as np
import pytest

import mipmap_cases as M
import post_cases as P
import post_texture_cases as X
import program_probe_cases as PC
import program_texture_cases as PT
from softwarerenderer_amd import (BlendMode, CullMode, DepthTest, MainWindow, PostProgram, Rasterizer, Texture, _native, hostmath as hm,
                                  scenes)
from softwarerenderer_amd.rasterizer import ShaderProgram
from test_gpu_parity import run_both
from test_gpu_program_probe import assert_words, render as render_scene
from test_gpu_program_textures import render as render_probe
from test_gpu_render_to_texture import QUAD, QUAD_IDX

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = _native.SWR_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def programs(device):
    """name -> program id, compiled when a test first asks for it."""
    class Compiled(dict):
        def __missing__(self, name):
            if name == "VERTEX_PROBE":
                self[name] = device.compile_program(PC.PROBE_ALL, vertex_source=M.VERTEX_PROBE)
            else:
                self[name] = device.compile_program(M.FRAGMENT_TEXTS[name])
            return self[name]
    ids = Compiled()
    yield ids
    for pid in ids.values():
        device.destroy_program(pid)


def same_bytes(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, f"{len(bad)} bytes differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def check_chain(tex, level0, what):
    """every level the texture has against the restatement of `level0`"""
    levels = M.chain(level0)
    assert tex.Levels == len(levels) == M.full_levels(tex.Width, tex.Height), (what, tex.Levels, len(levels))
    for l, want in enumerate(levels):
        assert tex.LevelSize(l) == (want.shape[1], want.shape[0]), (what, l)
        same_bytes(tex.ReadLevel(l), want, what + (l,))
    return levels


# ------------------------------------------------------------------------------------------------------------------ 1. the bytes
@pytest.mark.parametrize("size", M.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_level_equals_the_restatement(device, size):
    w, h = size
    texels = M.texture(size)
    tex = Texture(device, texels)
    try:
        assert tex.Levels == 1 and tex.LevelSize(M.full_levels(w, h) - 1) == (1, 1)
        same_bytes(tex.ReadLevel(0), texels, (size, "level 0 before"))
        tex.GenerateMipmaps()
        levels = check_chain(tex, texels, (size,))
        same_bytes(tex.Read(), texels, (size, "level 0 after"))
        tex.GenerateMipmaps()                            # nothing changed: the same bytes again
        check_chain(tex, texels, (size, "again"))
        if size != (1, 1):
            assert len(levels) >= 2 and levels[-1].shape == (1, 1, 4)
    finally:
        tex.Dispose()


def test_a_targets_levels_are_zero(device):
    tex = Texture.Target(device, 33, 17)
    try:
        tex.GenerateMipmaps()
        assert tex.Levels == 6
        for l in range(6):
            assert not tex.ReadLevel(l).any(), l
    finally:
        tex.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 2. updates
def frame_plane(width, height, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.1, 1.1, (height, width, 4)).astype(F32)


def test_updates_regenerate_the_chain_without_a_host_wait(device):
    win = MainWindow(device, 64, 64)
    chained, plain = Texture.Target(device, 32, 32), Texture.Target(device, 32, 32)
    identity = PostProgram(device, P.IDENTITY)
    try:
        chained.GenerateMipmaps()
        seen = []
        for step, keep in ((0, False), (1, True), (2, False)):
            win.Upload(color=frame_plane(64, 64, 70 + step))
            syncs, replays = device.sync_count(), device.replay_count()
            for t in (chained, plain):
                if step < 2:
                    t.UpdateFrom(win, 2, 2, keep_alpha=keep)
                else:
                    t.UpdateFromPost(win, identity, 2, 2, keep_alpha=keep)
            assert device.sync_count() == syncs and device.replay_count() == replays, "an update of a chained texture made the host wait"
            level0 = plain.Read()                       # today's bytes: the texture without a chain
            assert plain.Levels == 1 and level0.any()
            check_chain(chained, level0, ("update", step))
            seen.append(level0)
        assert (seen[0] != seen[1]).any() and (seen[1] != seen[2]).any()
        with pytest.raises(_native.SwrError):
            plain.ReadLevel(1)
    finally:
        identity.close(); chained.Dispose(); plain.Dispose()


@pytest.mark.parametrize("filter_first", [True, False])
def test_the_block_linear_copy_names_the_same_chain(device, filter_first):
    size = (68, 8)
    texels = M.texture(size)
    tex = Texture(device, texels)
    try:
        if filter_first:
            tex.SetBilinear(True)                       # the copy and its header exist before the chain does
        tex.GenerateMipmaps()
        tex.SetBilinear(True)                           # otherwise: the copy is made now and gets a copy of the header
        levels = check_chain(tex, texels, (size, filter_first))
        uv = M.lookup_uvs(*size)
        lods = M.lods_for(len(levels))
        got = tex.SampleLod(uv[:, None, :].repeat(len(lods), 1), lods[None, :].repeat(len(uv), 0))
        assert_words(got, M.sample_lod(levels, True, uv[:, None, :].repeat(len(lods), 1), lods[None, :].repeat(len(uv), 0)), f"blocked/{filter_first}")
    finally:
        tex.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 3. SampleLod
@pytest.mark.parametrize("filtered", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("size", M.SAMPLE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sample_lod_matches_the_restatement_word_for_word(device, size, filtered):
    texels = M.texture(size)
    tex = Texture(device, texels)
    try:
        tex.SetBilinear(filtered)
        uv = M.lookup_uvs(*size)
        L = M.full_levels(*size)
        lods = M.lods_for(L)
        uvs, ls = uv[:, None, :].repeat(len(lods), 1), lods[None, :].repeat(len(uv), 0)
        levels = M.chain(texels)
        # without a chain every lod gives level 0: swr_texture_sample's words under the nearest filter
        assert tex.Levels == 1
        flat = tex.SampleLod(uvs, ls)
        assert_words(flat, M.sample_lod(levels, filtered, uvs, ls, have=1), f"{size}/{filtered}/no chain")
        if not filtered:
            assert_words(flat, tex.Sample(uvs), f"{size}/no chain against swr_texture_sample")
        tex.GenerateMipmaps()
        got = tex.SampleLod(uvs, ls)
        want = M.sample_lod(levels, filtered, uvs, ls)
        assert_words(got, want, f"{size}/{filtered}")
        assert (got.view(np.uint32) != flat.view(np.uint32)).any(), "the chain shows nowhere"
        # the ends of the definition, through the GPU: NaN and -1 are lod 0; L and +Inf are lod L - 1; 1 is level 1 alone
        nanl, neg, zero, one, top, above, inf = (got[:, i] for i in (0, 1, 2, 5, 7, 8, 9))
        for a, b in ((nanl, zero), (neg, zero), (above, top), (inf, top)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert_words(one, M.sample_level(levels, filtered, 1, uv), "lod 1 is level 1")
    finally:
        tex.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 4. Lod
@pytest.mark.parametrize("size", [(12, 20), (68, 8), (5, 7), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lod_matches_the_restatement_word_for_word(device, size):
    w, h = size
    L = M.full_levels(w, h)
    g = M.gradient_ladder(w, h, L)
    tex = Texture(device, M.texture(size))
    try:
        assert_words(tex.Lod(g), M.lod(w, h, g, 1), f"{size}/no chain")          # one level: every lod clamps to 0
        assert (tex.Lod(g).view(np.uint32) == 0).all()
        tex.GenerateMipmaps()
        got = tex.Lod(g)
        assert_words(got, M.lod(w, h, g, L), f"{size}", exact_nan=True)
        assert not np.isnan(got).any() and (got == L - 1).any() and ((got > 0) & (got < L - 1)).any()
        # rho exactly 1, 2, 4, 2^(L - 1), axis-aligned, four ways each: the integers (where 1 / w and 1 / h are exact)
        if size == (64, 64):
            assert np.array_equal(got[1:17].reshape(4, 4), np.array([0, 1, 2, L - 1], dtype=F32)[:, None].repeat(4, 1))
    finally:
        tex.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 5. the field
SCENES = {"cells": PC.cells, "clipped": PC.clipped, "wide": PC.wide}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_gradient_field_matches_the_restatement_word_for_word(device, programs, name):
    scene = SCENES[name]()
    planes, count = PC.expected_planes(scene)
    planes = dict(planes, **M.grad_planes(scene))
    covered = int((count > 0).sum())
    assert count.max() == 1 and covered > 0
    for text, names in (("GRAD_XYZ", ("grad.x", "grad.y", "grad.z")), ("GRAD_WXY", ("grad.w", "grad.x", "grad.y"))):
        c, _, st = render_scene(device, scene, programs[text])
        assert_words(c, PC.expected_colour(scene, names, planes, count), f"{name}/{text}")
        assert st["fragments_written"] == covered
    g = np.stack([planes[n][count > 0] for n in M.GRAD_NAMES], axis=1)
    assert len(np.unique(g.view(np.uint32), axis=0)) > covered // 20 or name == "wide", "the gradient is the same everywhere"


@pytest.fixture(scope="module")
def chained(device):
    """name -> (live Texture, chain, filtered, levels it has): 12 x 20 nearest and 68 x 8 bilinear (block-linear level 0) with chains,
    5 x 7 without one"""
    made = {}
    for name, size, filtered, generate in (("12x20", (12, 20), False, True), ("68x8", (68, 8), True, True), ("5x7", (5, 7), False, False)):
        t = Texture(device, M.texture(size))
        t.SetBilinear(filtered)
        if generate:
            t.GenerateMipmaps()
        made[name] = (t, M.chain(M.texture(size)), filtered, M.full_levels(*size) if generate else 1)
    yield made
    for t, *_ in made.values():
        t.Dispose()


@pytest.mark.parametrize("slot", [0, 2, 3, 1, 7, M.PER_PIXEL], ids=["slot0", "slot2", "slot3_no_chain", "unbound", "out_of_range", "per_pixel"])
def test_lod_levels_and_sample_grad_through_a_program(device, programs, chained, slot):
    scene = PC.wide()
    spec = ("12x20", None, "68x8", "5x7")
    tex = tuple(None if n is None else chained[n][0] for n in spec)
    planes, count = PC.expected_planes(scene)
    grads = M.grad_planes(scene)
    k = np.zeros(64, dtype=F32)
    k[M.SLOT] = slot

    def words_of(j, xs, ys):
        uv = np.stack([planes["tex_coord.x"][ys, xs], planes["tex_coord.y"][ys, xs]], axis=1)
        g = np.stack([grads[n][ys, xs] for n in M.GRAD_NAMES], axis=1)
        out = np.zeros((len(xs), 3), dtype=F32)
        which = (xs + ys) % 5 if slot == M.PER_PIXEL else np.full(len(xs), int(slot))
        for s in np.unique(which):
            m = which == s
            name = spec[s] if 0 <= s < 4 else None
            if name is None:
                out[m] = (0.0, 0.0, 1.0)                # lod 0, 0 levels, sample 1
                continue
            t, levels, filtered, have = chained[name]
            lod = M.lod(t.Width, t.Height, g[m], have)
            out[m] = np.stack([lod, np.full(m.sum(), have, dtype=F32), M.sample_lod(levels, filtered, uv[m], lod, have)[:, 0]], axis=1)
        return out
    want, n = PT.expected_frame(scene, words_of)
    c, st = render_probe(device, scene, programs["CHAIN_PROBE"], [(k, tex)] * len(scene.draws))
    assert_words(c, want, f"chain probe/{slot}")
    assert st["fragments_written"] == n > 0
    cov = count > 0
    if slot in (1, 7):
        assert (c[cov][:, :3] == np.array([0, 0, 1], dtype=F32)).all()
    if slot == 2:
        assert len(np.unique(c[cov][:, 0])) > 3 and (c[cov][:, 1] == 7).all(), "the lod does not vary over the frame"


# ------------------------------------------------------------------------------------------------------------------ 6. a receding checkerboard
def ground_scene():
    """One ground triangle at y = -1 under a perspective camera at the origin, 128 x 128: uv = (x, z) / 2 repeats the 64 x 64
    checkerboard; a texel is about a pixel wide at the bottom of the frame and hundreds of texels share a pixel at the horizon."""
    v = scenes.make_vertices([(-8.0, -1.0, -1.5), (8.0, -1.0, -1.5), (0.0, -1.0, -60.0)], uv=[(-4.0, 0.75), (4.0, 0.75), (0.0, 30.0)])
    d = scenes.Draw(v, np.array([0, 1, 2], dtype=np.uint16), hm.identity(), hm.identity(),
                    hm.create_perspective_fov(np.pi / 3, 1.0, 0.1, 100.0), cull=CullMode.None_, blend=BlendMode.None_)
    return scenes.Scene("mip_ground", 128, 128, [d], clear_color=PC.CLEAR, near_clip=0.1)


def draw_ground(device, scene, pid, tex):
    win = MainWindow(device, scene.width, scene.height)
    Rasterizer.NearClip, Rasterizer.FarClip = scene.near_clip, scene.far_clip
    win.ClearDepthBuffer(); win.ClearColorBuffer(scene.clear_color)
    d = scene.draws[0]
    device.set_program_constants(pid, np.zeros(64, dtype=F32))
    prog = ShaderProgram(pid, None, tex)
    Rasterizer.RenderMesh(win, d.vertices, d.indices, d.model, d.view, d.projection, prog.VertexShader, prog.FragmentShader, d.cull, d.depth_test, d.blend)
    return win._read(True, False)[0]


def test_a_receding_checkerboard_settles_on_its_last_level(device, programs):
    scene = ground_scene()
    board = M.checkerboard(64)
    levels = M.chain(board)
    L = len(levels)
    planes, count = PC.expected_planes(scene)
    grads = M.grad_planes(scene)
    cov = count > 0
    assert count.max() == 1 and cov.sum() > 2000
    uv = np.stack([planes["tex_coord.x"], planes["tex_coord.y"]], axis=-1)
    lod = M.lod(64, 64, np.stack([grads[n] for n in M.GRAD_NAMES], axis=-1), L)
    far, near = cov & (lod == L - 1), cov & (lod == 0)
    assert far.sum() > 50 and near.sum() > 50 and (cov & (lod > 0) & (lod < L - 1)).sum() > 200      # (the camera was chosen for this)
    tex = Texture(device, board)
    try:
        tex.GenerateMipmaps()
        got = draw_ground(device, scene, programs["RECIPE"], tex)
        plain = draw_ground(device, scene, programs["PLAIN"], tex)
        last = (levels[-1][0, 0].astype(F32) * M.INV255).astype(F32)
        assert np.array_equal(levels[-1][0, 0], (128, 128, 128, 255))
        assert (got[far][:, :3] == last[:3]).all(), "a pixel whose lod is the top level is not the last level's texel"
        assert np.array_equal(got[near].view(np.uint32), plain[near].view(np.uint32)), "a pixel of lod 0 differs from swr_sample"
        assert set(np.unique(plain[cov][:, 0])) == {F32(0.0), F32(1.0)} and (plain[far][:, 0] != last[0]).all()     # it aliases without the chain
        want = np.empty_like(got)
        want[...] = np.asarray(scene.clear_color, dtype=F32)
        s = M.sample_lod(levels, False, uv[cov], lod[cov])
        want[cov] = np.concatenate([s[:, :3], np.ones((int(cov.sum()), 1), dtype=F32)], axis=1)
        assert_words(got, want, "the whole frame")
    finally:
        tex.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 7. the other halves
def test_the_vertex_half_samples_levels(device, programs, chained):
    from vertex_probe_cases import _empty, nm_flags, renderer_clip
    scene = PT.vertex_scene()
    flags = nm_flags(*device.transform_fma())
    t, levels, filtered, have = chained["12x20"]
    tex = (None, t, None, None)
    groups = [g for g in PC.FS_IN_GROUPS if any(n.split(".")[0] == "data4" for n in PC.group_names(g))]
    assert groups
    for level, lod in ((1, 0.5), (3, 2.25), (9, 1.0)):
        stages = []
        for d in scene.draws:
            o = _empty(d.vertices.shape[0])
            for i in range(d.vertices.shape[0]):
                o["clip"][i] = renderer_clip(d, i, flags)
            uv = d.vertices["uv"].astype(F32)
            s = M.sample_level(levels, filtered, level, uv)
            o["data4"][:, 0], o["data4"][:, 1], o["data4"][:, 2] = s[:, 0], s[:, 1], have
            o["data4"][:, 3] = M.sample_lod(levels, filtered, uv, F32(lod))[:, 2]
            stages.append(o)
        planes, count = PC.expected_planes(scene, tris=PC.probe_tris(scene, lambda j, d: stages[j]))
        covered = int((count > 0).sum())
        assert count.max() == 1 and covered > 0
        for g in groups:
            k = PC.selector_constants(g)
            k[0], k[1] = level, lod
            c, st = render_probe(device, scene, programs["VERTEX_PROBE"], [(k, tex)] * len(scene.draws))
            assert_words(c, PC.expected_colour(scene, PC.group_names(g), planes, count), f"vertex/{level}/{lod}/{'+'.join(PC.group_names(g))}")
            assert st["fragments_written"] == covered


def test_a_post_program_samples_levels_as_floats_and_into_a_texture(device, chained):
    out_size = (65, 5)
    win = MainWindow(device, *out_size)
    win.Upload(color=frame_plane(out_size[0], out_size[1], 5))
    post = PostProgram(device, M.POST_PROBE)
    target = Texture.Target(device, *out_size)
    target.GenerateMipmaps()
    try:
        for name, other in (("12x20", "5x7"), ("68x8", None)):
            t, levels, filtered, have = chained[name]
            post.SetTexture(0, t)
            post.SetTexture(1, chained[other][0] if other else None)
            for lod, level, dudx in ((0.75, 2, 4.0 / t.Width), (2.5, 0, 0.0), (float("nan"), 99, 3.0 / t.Width)):
                k = X.uv_constants(out_size).copy()
                k[5], k[6], k[7] = lod, level, dudx
                post.SetConstants(k)
                uv = X.pixel_uv(out_size[1], out_size[0], k)
                a = M.sample_lod(levels, filtered, uv, F32(lod))
                b = M.sample_level(levels, filtered, level, uv)
                z = F32(chained[other][3] if other else 0) + M.lod(t.Width, t.Height, np.array([dudx, 0, 0, 0], dtype=F32), have)
                want = np.stack([a[..., 0], b[..., 1], np.broadcast_to(F32(z), a.shape[:-1]), a[..., 3]], axis=-1).astype(F32)
                assert_words(win.PostBuffer(post, 1, 1, 3, np.float32), want[..., :3], f"post/{name}/{lod}/{level}")
                target.UpdateFromPost(win, post, 1, 1, keep_alpha=True)
                texels = X.texels(want, keep_alpha=True)
                same_bytes(target.Read(), texels, ("post into a texture", name, lod))
                check_chain(target, texels, ("post into a chained texture", name, lod))
    finally:
        post.close(); target.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 8. order
def order_frames(device, win, pid, texels, synced):
    """A big quad sampling slot 1 at lod 1, left unflushed; GenerateMipmaps; a smaller, nearer quad under the same program.  synced: a
    swr_sync after every step.  Returns (colour, sync counts moved by GenerateMipmaps)."""
    I = hm.identity()
    tex = Texture(device, texels)
    step = device.sync if synced else (lambda: None)
    try:
        small = QUAD.copy()
        small["position"][:, :2] *= F32(0.5)
        small["position"][:, 2] = -0.9
        k = np.zeros(64, dtype=F32)
        k[0] = 1.0
        device.set_program_constants(pid, k)
        device.set_program_texture(pid, 1, tex)
        prog = ShaderProgram(pid)
        win.ClearDepthBuffer(); win.ClearColorBuffer((0.1, 0.2, 0.3, 1.0)); step()
        Rasterizer.RenderMesh(win, QUAD, QUAD_IDX, I, I, I, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.None_)
        step()
        before = device.sync_count()
        tex.GenerateMipmaps()
        moved = device.sync_count() - before
        step()
        Rasterizer.RenderMesh(win, small, QUAD_IDX, I, I, I, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.Always, BlendMode.None_)
        step()
        color = win._read(True, False)[0]
    finally:
        device.set_program_texture(pid, 1, None)
        tex.Dispose()
    return color, moved


def one_level_frame(device, win, pid, texels, generate, which):
    """the big quad (which = 0), both quads (1) or the small one alone (2), every draw at lod 1 of a texture that has (generate) or has
    not got its chain"""
    I = hm.identity()
    tex = Texture(device, texels)
    try:
        if generate:
            tex.GenerateMipmaps()
        k = np.zeros(64, dtype=F32)
        k[0] = 1.0
        device.set_program_constants(pid, k)
        device.set_program_texture(pid, 1, tex)
        prog = ShaderProgram(pid)
        win.ClearDepthBuffer(); win.ClearColorBuffer((0.1, 0.2, 0.3, 1.0))
        small = QUAD.copy()
        small["position"][:, :2] *= F32(0.5)
        small["position"][:, 2] = -0.9
        for mesh, test in ((QUAD, DepthTest.LessEqual), (small, DepthTest.Always))[which // 2:which % 2 + 1 + which // 2]:
            Rasterizer.RenderMesh(win, mesh, QUAD_IDX, I, I, I, prog.VertexShader, prog.FragmentShader, CullMode.None_, test, BlendMode.None_)
        return win._read(True, False)[0]
    finally:
        device.set_program_texture(pid, 1, None)
        tex.Dispose()


@pytest.mark.parametrize("pipelining", [0, 1, 2])
def test_draws_before_generate_see_one_level_and_draws_after_it_the_chain(device, programs, pipelining):
    W, H = 128, 96
    win = MainWindow(device, W, H)
    pid = programs["LOD_CONSTANT"]
    texels = M.texture((12, 20), seed=3).copy()
    texels[..., 3] = 255                                 # (a result with w = 0 writes nothing: every fragment of both quads is written)
    was = device.pipelining()
    device.set_pipelining(pipelining)
    try:
        order_frames(device, win, pid, texels, synced=False)               # sizes the pair buffers of every raster set in use
        device.sync()
        replays = device.replay_count()
        color, moved = order_frames(device, win, pid, texels, synced=False)
        assert moved == 0, "swr_texture_generate_mipmaps made the host wait"
        assert device.replay_count() == replays, "a batch was replayed: the comparison below would not be about ordering"
        ref, _ = order_frames(device, win, pid, texels, synced=True)
        assert_words(color, ref, "against the same sequence with a swr_sync after every step")
        # the first draw holds level-0 words (the texture had one level when it ran), the second level-1 words
        level0 = one_level_frame(device, win, pid, texels, False, 1)
        level1 = one_level_frame(device, win, pid, texels, True, 1)
        big_only = one_level_frame(device, win, pid, texels, False, 0)
        clear = np.array((0.1, 0.2, 0.3, 1.0), dtype=F32)
        inner = (one_level_frame(device, win, pid, texels, False, 2) != clear).any(axis=-1)           # where the small quad shows
        outer = (big_only != clear).any(axis=-1) & ~inner
        assert inner.sum() > 500 and outer.sum() > 500
        assert np.array_equal(color[outer].view(np.uint32), level0[outer].view(np.uint32)), "the draw recorded before GenerateMipmaps saw the chain"
        changed = (level0[inner].view(np.uint32) != level1[inner].view(np.uint32)).any(axis=-1)
        assert changed.mean() > 0.5
        assert np.array_equal(color[inner][changed].view(np.uint32), level1[inner][changed].view(np.uint32)), "the draw recorded after GenerateMipmaps saw one level"
    finally:
        device.set_pipelining(was)


# ------------------------------------------------------------------------------------------------------------------ 9. refusals
def test_a_plain_c_caller_generates_and_reads_levels_through_the_abi():
    """tests/c/mipmap_smoke.c: gcc + dlopen, no C++ / HIP headers."""
    import os
    import spawner
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c")
    spawner.run(["make", "-C", here, "-f", "mipmap_smoke.mk", "-s"], check=True)
    out = spawner.run([os.path.join(here, "mipmap_smoke"), _native.LIB_PATH], timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wrong=0 refused=-1" in out.stdout


def test_refusals_leave_the_textures_and_the_context_alone(device):
    lib, ctx = device._lib, device._ctx
    texels = M.texture((12, 20))
    tex = Texture(device, texels)
    flat = Texture(device, texels)
    depth = Texture.Depth(device, 8, 8)
    out = np.zeros((20, 12, 4), dtype=np.uint8)
    f4, n, wh = np.zeros(8, dtype=F32), C.c_int(-7), (C.c_int(-7), C.c_int(-7))

    def refused(words, rc):
        assert rc == INVALID, (words, rc)
        assert words in lib.swr_last_error(ctx).decode(), (words, lib.swr_last_error(ctx).decode())
    try:
        tex.GenerateMipmaps()
        syncs = device.sync_count()
        refused("texture is null", lib.swr_texture_generate_mipmaps(ctx, None))
        refused("is a depth texture", lib.swr_texture_generate_mipmaps(ctx, depth._h))
        assert device.sync_count() == syncs
        refused("is a depth texture", lib.swr_texture_readback_level(ctx, depth._h, 0, out.ctypes.data))
        refused("is a depth texture", lib.swr_texture_sample_lod(ctx, depth._h, f4.ctypes.data, 1, f4.ctypes.data))
        refused("is a depth texture", lib.swr_texture_lod(ctx, depth._h, f4.ctypes.data, 1, f4.ctypes.data))
        assert depth.Levels == 1
        for level in (-1, 5, 99):
            refused("outside the levels the texture has", lib.swr_texture_readback_level(ctx, tex._h, level, out.ctypes.data))
            refused("outside the texture's full chain", lib.swr_texture_level_size(ctx, tex._h, level, C.byref(wh[0]), C.byref(wh[1])))
        refused("outside the levels the texture has", lib.swr_texture_readback_level(ctx, flat._h, 1, out.ctypes.data))
        assert flat.LevelSize(4) == (1, 1) and flat.Levels == 1               # the full chain's sizes, generated or not
        assert lib.swr_texture_levels(ctx, None, C.byref(n)) == INVALID and lib.swr_texture_levels(ctx, tex._h, None) == INVALID
        assert lib.swr_texture_level_size(ctx, tex._h, 0, None, C.byref(wh[1])) == INVALID
        assert lib.swr_texture_level_size(ctx, None, 0, C.byref(wh[0]), C.byref(wh[1])) == INVALID
        assert lib.swr_texture_readback_level(ctx, tex._h, 0, None) == INVALID and lib.swr_texture_readback_level(ctx, None, 0, out.ctypes.data) == INVALID
        for fn in (lib.swr_texture_sample_lod, lib.swr_texture_lod):
            assert fn(ctx, None, f4.ctypes.data, 1, f4.ctypes.data) == INVALID and fn(ctx, tex._h, None, 1, f4.ctypes.data) == INVALID
            assert fn(ctx, tex._h, f4.ctypes.data, 1, None) == INVALID and fn(ctx, tex._h, f4.ctypes.data, -1, f4.ctypes.data) == INVALID
            assert fn(ctx, tex._h, f4.ctypes.data, 0, f4.ctypes.data) == _native.SWR_OK
        assert not out.any() and not f4.any() and (n.value, wh[0].value, wh[1].value) == (-7, -7, -7), "a refused call wrote its destination"
        # nothing was written, and a 1 x 1 texture has its chain of one level
        check_chain(tex, texels, ("after the refusals",))
        same_bytes(flat.Read(), texels, "after the refusals")
        one = Texture(device, M.texture((1, 1)))
        one.GenerateMipmaps()
        assert one.Levels == 1
        one.Dispose()
    finally:
        tex.Dispose(); flat.Dispose(); depth.Dispose()
    run_both(device, scenes.cfg2(160, 120, 200, seed=3))
