"""Cube maps on the GPU (include/swr.h, csrc/swr_device.h, csrc/swr_api.hip): the batched lookups against the
numpy restatement of tests/cubemap_cases.py word for word, the same functions in both halves of a user program and in a post
program, face updates through the existing kernels with a face's offset, their ordering without a host synchronisation, the
orientation of the face cameras and the point-light shadow recipe end to end, chains, and the refusals.  No tolerance anywhere:
bytes are compared as bytes and floats as 32-bit words."""
import ctypes as C

import numpy as np
import pytest

import cubemap_cases as K
import depth_texture_cases as D
import mipmap_cases as M
import program_probe_cases as PC
import program_texture_cases as PT
import render_to_texture_cases as T
from softwarerenderer_amd import (BlendMode, CullMode, DepthReduce, DepthTest, MainWindow, PostProgram, Rasterizer, Texture, _native,
                                  hostmath as hm, scenes)
from softwarerenderer_amd.rasterizer import ShaderProgram
from test_gpu_parity import run_both
from test_gpu_program_probe import assert_words
from test_gpu_program_textures import render as render_probe
from test_gpu_render_to_texture import QUAD, QUAD_IDX, same_bytes

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, UNSUPPORTED = _native.SWR_ERR_INVALID_ARG, _native.SWR_ERR_UNSUPPORTED
I4 = hm.identity()
PLAIN_COLOUR = PC.HEAD + "    return make_float4(in.color.x, in.color.y, in.color.z, 1.0f);\n}\n"
# the centre of face +X, halved: the order test's two draws
ORDER = PC.HEAD + """    const float4 c = swr_sample_cube(env, 1, make_float3(1.0f, 0.0f, 0.0f));
    return make_float4(c.x * 0.5f, c.y * 0.5f, c.z * 0.5f, 1.0f);
}
"""


@pytest.fixture(scope="module")
def programs(device):
    """name -> program id, compiled when a test first asks for it."""
    texts = dict(K.FRAGMENT_TEXTS, PLAIN_COLOUR=(None, PLAIN_COLOUR), ORDER=(None, ORDER))

    class Compiled(dict):
        def __missing__(self, name):
            vertex, fragment = texts[name]
            self[name] = device.compile_program(fragment) if vertex is None else device.compile_program(fragment, vertex_source=vertex)
            return self[name]
    ids = Compiled()
    yield ids
    for pid in ids.values():
        device.destroy_program(pid)


def same_words(got, want, what):
    """32-bit words, NaN payloads included"""
    g, w = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
    assert bad.size == 0, (what, f"{len(bad)} words differ, first at {tuple(bad[0])}: got {g[tuple(bad[0])]!r} want {w[tuple(bad[0])]!r}")


# ------------------------------------------------------------------------------------------------------------------ 1. the batches
def test_cube_face_matches_the_restatement_word_for_word(device):
    dirs = np.concatenate([K.directions(n) for n in (0, 2, 4, 8, 16)])
    face, st = Texture.CubeFace(device, dirs)
    want_face, want_st = K.cube_face(dirs)
    assert np.array_equal(face, want_face), np.argwhere(face != want_face)[:4]
    same_words(st, want_st, "st")
    assert set(face.tolist()) == {0, 1, 2, 3, 4, 5} and (st == 0).any() and (st == 1).any()


@pytest.mark.parametrize("filtered", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("n", K.SIDES)
def test_sample_cube_and_the_depth_lookups_match_the_restatement_word_for_word(device, n, filtered):
    dirs = K.directions(n)
    faces, words = K.colour_faces(n), K.depth_faces(n)
    cube, depth = Texture.Cube(device, faces), Texture.CubeDepth(device, n, words)
    try:
        assert cube.IsCube == n and depth.IsCube == n and (cube.Width, cube.Height) == (n, 6 * n)
        assert depth.Format == _native.SWR_TEXTURE_FORMAT_DEPTH32F and cube.Levels == 1
        cube.SetBilinear(filtered); depth.SetBilinear(filtered)
        a, w = K.atlas(faces), K.atlas(words)
        same_bytes(cube.Read(), a, (n, "the atlas"))
        same_words(depth.ReadDepth(), w, (n, "the depth atlas"))
        for f in range(6):
            same_bytes(cube.ReadFace(f), faces[f], (n, f))
            same_words(depth.ReadFace(f), words[f], (n, f))
        same_words(cube.SampleCube(dirs), K.sample_cube(a, filtered, dirs), (n, filtered, "sample_cube"))
        same_words(cube.SampleCube(dirs, 2.5), K.sample_cube(a, filtered, dirs), (n, filtered, "a lod without a chain is level 0"))
        for seed in (0, 1):
            refs = K.refs_for(w, dirs, seed)
            got_d, got_s = depth.SampleCubeDepth(dirs, refs)
            same_words(got_d, K.depth_sample(w, dirs), (n, filtered, "depth"))
            same_words(got_s, K.shadow_cube(w, filtered, dirs, refs), (n, filtered, "shadow"))
            assert set(np.unique(got_s)) >= {F32(0.0), F32(1.0)}
        # every existing call sees the n x 6 n atlas
        uv = T.texel_centres(n, 6 * n)
        cube.SetBilinear(False)
        same_words(cube.Sample(uv), (a.astype(F32) * K.INV255).astype(F32), (n, "Sample over the atlas"))
        if n in K.CHAIN_SIDES:
            cube.SetBilinear(filtered)
            cube.GenerateMipmaps()
            levels = K.chain(a)
            assert cube.Levels == len(levels) == 1 + n.bit_length() - 1
            lods = K.lods_for(len(levels))
            every = np.broadcast_to(dirs[:, None, :], (len(dirs), len(lods), 3))
            got = cube.SampleCube(every, lods)
            want = K.sample_cube_lod(levels, filtered, every, np.broadcast_to(lods, (len(dirs), len(lods))))
            same_words(got, want, (n, filtered, "lod"))
    finally:
        cube.Dispose(); depth.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 2. programs
SCREEN_TRIANGLE = scenes.make_vertices([(-1.0, -1.0, 0.0), (3.0, -1.0, 0.0), (-1.0, 3.0, 0.0)], uv=[(0, 0), (1, 0), (0, 1)])
SCREEN_IDX = np.array([0, 1, 2], dtype=np.uint16)
CLEAR = (0.25, 0.5, 0.75, 0.125)


def run_fragment_probe(device, win, pid, k, slots):
    win.ClearDepthBuffer(); win.ClearColorBuffer(CLEAR)
    device.reset_stats()
    device.set_program_constants(pid, k)
    for s in (1, 2, 3):
        device.set_program_texture(pid, s, slots[s])
    prog = ShaderProgram(pid)
    Rasterizer.RenderMesh(win, SCREEN_TRIANGLE, SCREEN_IDX, I4, I4, I4, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.Always, BlendMode.None_)
    color = win._read(True, False)[0].reshape(K.PROBE_H, K.PROBE_W, 4)
    assert device.stats()["fragments_written"] == K.PROBE_PIXELS
    for s in (1, 2, 3):
        device.set_program_texture(pid, s, None)
    return color


def probe_rounds(n):
    """rounds of PROBE_PIXELS directions from the pool: the lattice, the degenerate set, then the texel boundaries of n"""
    pool = K.directions(n)
    picked = np.concatenate([np.arange(26), np.arange(104, 104 + len(K.degenerate())), np.arange(len(pool) - 40, len(pool))])
    return [pool[picked[i:i + K.PROBE_PIXELS]] for i in range(0, len(picked) - K.PROBE_PIXELS + 1, K.PROBE_PIXELS)]


@pytest.mark.parametrize("filtered", [False, True], ids=["nearest", "bilinear"])
def test_a_fragment_and_a_post_program_agree_with_the_batches(device, programs, filtered):
    n = 8
    faces, words = K.colour_faces(n, 1), K.depth_faces(n, 1, finite=True)
    cube, depth = Texture.Cube(device, faces), Texture.CubeDepth(device, n, words)
    flat = Texture(device, M.texture((5, 7)))
    post = PostProgram(device, K.POST_PROBE)
    win = MainWindow(device, K.PROBE_W, K.PROBE_H)
    try:
        cube.SetBilinear(filtered); depth.SetBilinear(filtered)
        cube.GenerateMipmaps()
        levels, w = K.chain(K.atlas(faces)), K.atlas(words)
        pid = programs["FRAGMENT_PROBE"]
        post.SetTexture(0, cube); post.SetTexture(1, depth)
        for r, dirs in enumerate(probe_rounds(n)):
            refs = K.refs_for(w, dirs, r)
            lasts = {0: refs, 1: refs, 3: K.lods_for(len(levels))[np.arange(len(dirs)) % 11], 4: (np.arange(len(dirs)) % 6 - 1).astype(F32)}
            for mode in (0, 1, 3, 4):
                k = K.probe_constants(dirs, lasts[mode], mode)
                want = K.probe_twin(k, (levels, filtered), (w, filtered), None)
                # the twin IS the batch: the same restatement the batched lookups were held to, and the batch itself
                if mode == 0:
                    same_words(cube.SampleCube(dirs)[:, :3].reshape(want.shape), want, ("batch", r))
                if mode == 1:
                    same_words(depth.SampleCubeDepth(dirs, refs)[1].reshape(want.shape[:2]), want[..., 1], ("batch shadow", r))
                got = run_fragment_probe(device, win, pid, k, (None, cube, depth, None))
                same_words(got[..., :3], want, ("fragment", filtered, r, mode))
                assert (got[..., 3] == 1).all()
                post.SetConstants(k)
                win.Upload(color=np.zeros((K.PROBE_H, K.PROBE_W, 4), dtype=F32))
                same_words(win.PostBuffer(post, 1, 1, 3, np.float32), want, ("post", filtered, r, mode))
        # a slot that is not a cube, and an unbound one: the defined values, before any load
        k = K.probe_constants(K.directions(n)[:K.PROBE_PIXELS], 0.5, 2)
        want = K.probe_twin(k, (levels, filtered), (w, filtered), None)
        for other in (flat, None):
            same_words(run_fragment_probe(device, win, pid, k, (None, cube, depth, other))[..., :3], want, ("not a cube", other is None))
            post.SetTexture(2, other)
            post.SetConstants(k)
            same_words(win.PostBuffer(post, 1, 1, 3, np.float32), want, ("post, not a cube", other is None))
        assert (want == K.NOT_A_CUBE).all()
    finally:
        post.close(); cube.Dispose(); depth.Dispose(); flat.Dispose()


def test_the_vertex_half_agrees_with_the_batches(device, programs):
    from vertex_probe_cases import _empty, nm_flags, renderer_clip
    n = 4
    scene = PT.vertex_scene()
    pool = K.directions(n)
    at = 0
    for d in scene.draws:                                    # (vertex_scene hands out copies: a direction of its own per drawn vertex)
        for v in np.unique(d.indices):
            d.vertices["normal"][v] = pool[[3, 30, 60, 107, 130, 400, 410, 420, 430][at]]
            at += 1
    flags = nm_flags(*device.transform_fma())
    faces, words = K.colour_faces(n, 2), K.depth_faces(n, 2, finite=True)
    cube, depth = Texture.Cube(device, faces), Texture.CubeDepth(device, n, words)
    groups = [g for g in PC.FS_IN_GROUPS if any(name.split(".")[0] == "data4" for name in PC.group_names(g))]
    try:
        for filtered in (False, True):
            cube.SetBilinear(filtered); depth.SetBilinear(filtered)
            stages = []
            for d in scene.draws:
                o = _empty(d.vertices.shape[0])
                for i in range(d.vertices.shape[0]):
                    o["clip"][i] = renderer_clip(d, i, flags)
                dirs, ref = d.vertices["normal"].astype(F32), d.vertices["uv"][:, 1].astype(F32)
                c = K.sample_cube(K.atlas(faces), filtered, dirs)
                same_words(cube.SampleCube(dirs), c, "the batch")
                o["data4"][:, 0] = c[:, 0]
                o["data4"][:, 1] = K.shadow_cube(K.atlas(words), filtered, dirs, ref)
                o["data4"][:, 2] = K.depth_sample(K.atlas(words), dirs)
                o["data4"][:, 3] = (c[:, 3] + F32(n)).astype(F32)
                stages.append(o)
            planes, count = PC.expected_planes(scene, tris=PC.probe_tris(scene, lambda j, d: stages[j]))
            covered = int((count > 0).sum())
            assert count.max() == 1 and covered > 0
            for g in groups:
                k = PC.selector_constants(g)
                c, st = render_probe(device, scene, programs["VERTEX_PROBE"], [(k, (None, cube, depth, cube))] * len(scene.draws))
                assert_words(c, PC.expected_colour(scene, PC.group_names(g), planes, count), f"vertex/{filtered}/{'+'.join(PC.group_names(g))}")
                assert st["fragments_written"] == covered
    finally:
        for s in (1, 2, 3):
            device.set_program_texture(programs["VERTEX_PROBE"], s, None)
        cube.Dispose(); depth.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 3. face updates
@pytest.mark.parametrize("k", [1, 2])
def test_face_updates_write_one_face_through_the_existing_kernels(device, k):
    n = 16
    win = MainWindow(device, n * k, n * k)
    cube, depth = Texture.CubeTarget(device, n), Texture.CubeDepth(device, n)
    identity = PostProgram(device, "__device__ float4 swr_post(const swr_post_in& in, const swr_post_env& env) {\n    return in.color;\n}\n")
    try:
        cube.SetBilinear(True); depth.SetBilinear(True)      # n % 4 == 0: the block-linear copies exist
        want, want_d = np.zeros((6, n, n, 4), dtype=np.uint8), np.full((6, n, n), D.MINVALUE, dtype=F32)
        dirs = K.directions(n)
        for f in (3, 0, 5, 1, 4, 2, 3):                     # each face in turn, one of them twice
            colour, plane = T.pool_plane(n * k, n * k, 600 + 10 * f + k), D.depth_pool_plane(n * k, n * k, 700 + 10 * f + k)
            win.Upload(color=colour, depth=plane)
            keep, mode = bool(f & 1), (DepthReduce.Max, DepthReduce.Min, DepthReduce.First)[f % 3]
            syncs = device.sync_count()
            if f == 4:
                cube.UpdateFaceFromPost(f, win, identity, k, k, keep_alpha=keep)
            else:
                cube.UpdateFaceFrom(f, win, k, k, keep_alpha=keep)
            depth.UpdateFaceFromDepth(f, win, k, k, mode)
            assert device.sync_count() == syncs, "a face update made the host wait"
            want[f] = T.texels(colour, k, k, keep_alpha=keep)
            want_d[f] = D.reduce(plane, k, k, int(mode))
            if not keep:
                same_bytes(cube.ReadFace(f), win.ColorBuffer8(k, k, 4), (f, "swr_readback_rgb8"))
            for g in range(6):                               # this face is the source's, the other five keep their bytes
                same_bytes(cube.ReadFace(g), want[g], (k, f, g))
                same_words(depth.ReadFace(g), want_d[g], (k, f, g))
            # the block-linear copies agree: the bilinear lookups read them
            same_words(cube.SampleCube(dirs), K.sample_cube(K.atlas(want), True, dirs), (k, f, "bilinear SampleCube"))
            refs = K.refs_for(K.atlas(want_d), dirs, f)
            same_words(depth.SampleCubeDepth(dirs, refs)[1], K.shadow_cube(K.atlas(want_d), True, dirs, refs), (k, f, "bilinear shadow"))
        same_bytes(cube.Read(), K.atlas(want), "the atlas")
    finally:
        identity.close(); cube.Dispose(); depth.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 4. order
def order_frames(device, win, pid, faces, synced):
    """A big quad showing half the centre of face +X, left unflushed; face +X becomes the frame; a smaller quad under the same
    program.  Returns (colour, sync counts moved by the update)."""
    cube = Texture.Cube(device, faces)
    step = device.sync if synced else (lambda: None)
    try:
        small = QUAD.copy()
        small["position"][:, :2] *= F32(0.5)
        small["position"][:, 2] = -0.9
        device.set_program_texture(pid, 1, cube)
        prog = ShaderProgram(pid)
        win.ClearDepthBuffer(); win.ClearColorBuffer(CLEAR); step()
        Rasterizer.RenderMesh(win, QUAD, QUAD_IDX, I4, I4, I4, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.None_)
        step()
        before = device.sync_count()
        cube.UpdateFaceFrom(0, win, 2, 2)
        moved = device.sync_count() - before
        step()
        Rasterizer.RenderMesh(win, small, QUAD_IDX, I4, I4, I4, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.Always, BlendMode.None_)
        step()
        return win._read(True, False)[0].reshape(32, 32, 4), moved
    finally:
        device.set_program_texture(pid, 1, None)
        cube.Dispose()


@pytest.mark.parametrize("pipelining", [0, 1, 2])
def test_a_draw_before_a_face_update_sees_the_old_face_and_a_draw_after_it_the_new(device, programs, pipelining):
    n = 16
    win = MainWindow(device, 2 * n, 2 * n)
    faces = K.colour_faces(n, 3).copy()
    faces[0, 7:9, 7:9] = (200, 100, 50, 255)
    pid = programs["ORDER"]
    was = device.pipelining()
    device.set_pipelining(pipelining)
    try:
        order_frames(device, win, pid, faces, synced=False)      # sizes the buffers of every raster set in use
        device.sync()
        replays = device.replay_count()
        color, moved = order_frames(device, win, pid, faces, synced=False)
        assert moved == 0, "swr_texture_update_face_from_frame made the host wait"
        assert device.replay_count() == replays, "a batch was replayed: the comparison below would not be about ordering"
        ref, _ = order_frames(device, win, pid, faces, synced=True)
        same_words(color, ref, "against the same sequence with a swr_sync after every step")
        old = np.append(((np.array((200, 100, 50), dtype=F32) * K.INV255).astype(F32) * F32(0.5)).astype(F32), F32(1.0))
        frame = np.broadcast_to(old, (2, 2, 4)).astype(F32)
        new = np.append(((T.texels(frame, 2, 2)[0, 0, :3].astype(F32) * K.INV255).astype(F32) * F32(0.5)).astype(F32), F32(1.0))
        is_old, is_new = (color == old).all(axis=-1), (color == new).all(axis=-1)
        is_clear = (color == np.array(CLEAR, dtype=F32)).all(axis=-1)
        assert not np.array_equal(old, new) and is_old.sum() > 200 and is_new.sum() > 100 and (is_old | is_new | is_clear).all()
        assert is_new[16, 16] and is_old[4, 16]
    finally:
        device.set_pipelining(was)


# ------------------------------------------------------------------------------------------------------------------ 5. orientation
def front_facing(tri, view, proj):
    """Rasterizer.cs:367-414 for one world triangle in submission order: outputs = {v2, v1, v0}, the screen mapping, area < 0"""
    clip = np.concatenate([np.asarray(tri, dtype=np.float64), np.ones((3, 1))], axis=1) @ view.astype(np.float64) @ proj.astype(np.float64)
    ndc = clip[:, :3] / clip[:, 3:]
    sx, sy = ndc[:, 0] * 0.5 + 0.5, 1.0 - (ndc[:, 1] * 0.5 + 0.5)
    (ax, ay), (bx, by), (cx, cy) = ((sx[i], sy[i]) for i in (2, 1, 0))
    return (cx - ax) * (by - ay) - (cy - ay) * (bx - ax) < 0


def room():
    """Six walls one unit from the origin, each of four quadrant quads of a colour of their own; every triangle faces the origin by
    the rasterizer's own rule, decided under hostmath.create_look_at -- not under the face cameras this test is about.
    Returns (vertices, indices, {(face, su, sv): (direction of the quadrant's centre, colour bytes)})"""
    proj = hm.create_perspective_fov(np.pi / 3, 1.0, 0.1, 10.0)
    pos, col, idx, quadrants = [], [], [], {}
    for f, axis in enumerate(np.array(hm.CUBE_FACE_AXIS, dtype=np.float64)):
        u, v = np.roll(axis, 1), np.roll(axis, 2)            # two world axes in the wall, whatever their signs
        up = v
        view = hm.create_look_at((0, 0, 0), axis, up)
        for su in (-1, 1):
            for sv in (-1, 1):
                q = 2 * (su > 0) + (sv > 0)
                colour = (51 * (1 + f // 2), 51 * (1 + 2 * (f % 2) + q // 2), 51 * (1 + 3 * (q % 2)), 255)      # multiples of 51: exact bytes
                corners = [axis + a * u + b * v for a, b in ((0, 0), (su, 0), (su, sv), (0, sv))]
                base = len(pos)
                pos += corners
                col += [np.array(colour, dtype=np.float64) / 255.0] * 4
                for tri in ((0, 1, 2), (0, 2, 3)):
                    t = [base + i for i in tri]
                    if not front_facing([pos[i] for i in t], view, proj):
                        t = t[::-1]
                    assert front_facing([pos[i] for i in t], view, proj)
                    idx += t
                quadrants[(f, su, sv)] = (axis + 0.5 * su * u + 0.5 * sv * v, colour)
    assert len({c for _, c in quadrants.values()}) == 24, "the quadrants' colours are not distinct"
    return scenes.make_vertices([tuple(p) for p in pos], uv=[(0, 0)] * len(pos), color=[tuple(c) for c in col]), np.array(idx, dtype=np.uint16), quadrants


def render_faces(device, win, draw, eye, near, far):
    """the six face cameras at `eye`: draw(view, projection), then yield the face for the caller's update"""
    Rasterizer.NearClip, Rasterizer.FarClip = near, far
    proj = hm.create_perspective_fov(np.pi / 2, 1.0, near, far)
    view, eye32 = np.zeros(16, dtype=F32), np.ascontiguousarray(eye, dtype=F32)
    for f in range(6):
        assert device._lib.swr_cube_face_view(f, eye32.ctypes.data, view.ctypes.data) == 0
        assert np.array_equal(view.reshape(4, 4), hm.cube_face_view(f, eye))
        win.ClearDepthBuffer(); win.ClearColorBuffer((0.0, 0.0, 0.0, 1.0))
        draw(view.reshape(4, 4).copy(), proj)
        yield f


def test_the_face_cameras_render_a_room_the_lookup_reads_back_unmirrored(device, programs):
    n = 16
    vertices, indices, quadrants = room()
    win = MainWindow(device, n, n)
    cube = Texture.CubeTarget(device, n)
    prog = ShaderProgram(programs["PLAIN_COLOUR"])
    was = (Rasterizer.NearClip, Rasterizer.FarClip)
    try:
        def draw(view, proj):
            Rasterizer.RenderMesh(win, vertices, indices, I4, view, proj, prog.VertexShader, prog.FragmentShader, CullMode.Back, DepthTest.LessEqual, BlendMode.None_)
        for f in render_faces(device, win, draw, (0.0, 0.0, 0.0), 0.1, 10.0):
            cube.UpdateFaceFrom(f, win)
        for filtered in (False, True):
            cube.SetBilinear(filtered)
            keys = sorted(quadrants)
            got = cube.SampleCube(np.array([quadrants[k][0] for k in keys], dtype=F32))
            want = (np.array([quadrants[k][1] for k in keys], dtype=F32) * K.INV255).astype(F32)
            face, _ = K.cube_face(np.array([quadrants[k][0] for k in keys], dtype=F32))
            assert face.tolist() == [k[0] for k in keys]
            bad = [(k, g, w) for k, g, w in zip(keys, got.tolist(), want.tolist()) if g != w]
            assert not bad, (filtered, bad[:3])
        assert not (cube.Read()[..., :3] == 0).all(axis=-1).any(), "a wall was culled or missed: some texel kept the clear colour"
    finally:
        Rasterizer.NearClip, Rasterizer.FarClip = was
        cube.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 6. a point light
def quad_y(y, half, colour=(1, 1, 1, 1)):
    return scenes.make_vertices([(-half, y, -half), (half, y, -half), (half, y, half), (-half, y, half)], uv=[(0, 0)] * 4, color=[colour] * 4)


@pytest.mark.parametrize("filtered", [False, True], ids=["nearest", "bilinear"])
def test_a_point_lights_shadow_falls_where_the_occluder_hides_the_light(device, programs, filtered):
    n, near, far, bias = 16, 0.5, 20.0, 0.02
    light = (0.0, 0.0, 0.0)
    floor, occluder = quad_y(-2.0, 6.0), quad_y(-1.0, 0.5)
    win = MainWindow(device, n, n)
    screen = MainWindow(device, 64, 64)
    cube = Texture.CubeDepth(device, n)
    plain = ShaderProgram(programs["PLAIN_COLOUR"])
    pid = programs["SHADOW"]
    was = (Rasterizer.NearClip, Rasterizer.FarClip)
    try:
        cube.SetBilinear(filtered)

        def draw(view, proj):
            for mesh in (floor, occluder):
                Rasterizer.RenderMesh(win, mesh, QUAD_IDX, I4, view, proj, plain.VertexShader, plain.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.None_)
        for f in render_faces(device, win, draw, light, near, far):
            cube.UpdateFaceFromDepth(f, win)
        down = cube.ReadFace(3)
        assert (down > D.MINVALUE).all() and (down[6:10, 6:10] > down[0, 0] + 0.1).all(), "the light's -Y face should hold the floor and, nearer, the occluder"
        # the screen pass, by the recipe's program
        r = F32(far) / (F32(near) - F32(far))
        k = np.zeros(64, dtype=F32)
        k[0:3], k[3], k[4], k[5] = light, r, F32(near) * r, bias
        k[6:9], k[9:12] = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
        view = hm.create_look_at((5.0, 1.0, 0.0), (0.0, -2.0, 0.0), (0.0, 1.0, 0.0))
        proj = hm.create_perspective_fov(np.pi / 3, 1.0, 0.5, 30.0)
        Rasterizer.NearClip, Rasterizer.FarClip = 0.5, 30.0
        screen.ClearDepthBuffer(); screen.ClearColorBuffer((0.5, 0.5, 0.5, 1.0))
        device.set_program_constants(pid, k)
        device.set_program_texture(pid, 1, cube)
        prog = ShaderProgram(pid)
        for mesh in (floor, occluder):
            Rasterizer.RenderMesh(screen, mesh, QUAD_IDX, I4, view, proj, prog.VertexShader, prog.FragmentShader, CullMode.None_, DepthTest.LessEqual, BlendMode.None_)
        color = screen._read(True, False)[0].reshape(64, 64, 4)

        def pixel(p):
            clip = np.array([p[0], p[1], p[2], 1.0]) @ view.astype(np.float64) @ proj.astype(np.float64)
            return int((1 - (clip[1] / clip[3] * 0.5 + 0.5)) * 64), int((clip[0] / clip[3] * 0.5 + 0.5) * 64)
        shadowed = [(0.3, -2.0, 0.0), (0.4, -2.0, 0.4), (0.0, -2.0, -0.4), (-0.3, -2.0, 0.3), (0.0, -2.0, 0.0)]
        lit = [(1.6, -2.0, 0.0), (0.0, -2.0, -1.6), (-1.5, -2.0, 1.5), (1.7, -2.0, -1.7), (0.0, -1.0, 0.0), (0.3, -1.0, -0.3)]
        for p in shadowed:
            y, x = pixel(p)
            assert color[y, x].tolist() == [0.0, 0.0, 0.0, 1.0], (filtered, p, (x, y), color[y, x])
        for p in lit:
            y, x = pixel(p)
            assert color[y, x].tolist() == [1.0, 1.0, 1.0, 1.0], (filtered, p, (x, y), color[y, x])
    finally:
        Rasterizer.NearClip, Rasterizer.FarClip = was
        device.set_program_texture(pid, 1, None)
        cube.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 7. chains
def check_cube_chain(cube, faces, what):
    n = faces.shape[1]
    L = n.bit_length()
    assert cube.Levels == L == 1 + int(np.log2(n)), (what, cube.Levels)
    above = [np.asarray(f) for f in faces]
    for l in range(L):
        assert cube.LevelSize(l) == (n >> l, 6 * (n >> l)), (what, l)
        got = [cube.ReadFace(f, l) for f in range(6)]
        for f in range(6):
            same_bytes(got[f], above[f] if l == 0 else M.downsample(above[f]), what + (l, f))
        same_bytes(cube.ReadLevel(l), K.atlas(np.stack(got)), what + (l, "the level's atlas"))
        above = got


@pytest.mark.parametrize("n", [2, 8, 16])
def test_every_level_of_every_face_is_the_downsample_of_the_face_above(device, n):
    faces = K.colour_faces(n, 4)
    cube = Texture.Cube(device, faces)
    win = MainWindow(device, n, n)
    try:
        assert cube.Levels == 1
        cube.GenerateMipmaps()
        check_cube_chain(cube, faces, (n,))
        # a face update regenerates the chain in the same call, without a host wait
        colour = T.pool_plane(n, n, 800 + n)
        win.Upload(color=colour)
        syncs = device.sync_count()
        cube.UpdateFaceFrom(4, win, 1, 1, keep_alpha=True)
        assert device.sync_count() == syncs
        updated = faces.copy()
        updated[4] = T.texels(colour, 1, 1, keep_alpha=True)
        check_cube_chain(cube, updated, (n, "after a face update"))
    finally:
        cube.Dispose()


@pytest.mark.parametrize("n", [3, 5])
def test_a_side_that_is_no_power_of_two_has_no_chain(device, n):
    faces = K.colour_faces(n, 5)
    cube = Texture.Cube(device, faces)
    try:
        with pytest.raises(_native.SwrError) as e:
            cube.GenerateMipmaps()
        assert e.value.code == UNSUPPORTED
        assert cube.Levels == 1
        same_bytes(cube.Read(), K.atlas(faces), "after the refusal")
        same_words(cube.SampleCube(K.directions(), 1.5), K.sample_cube(K.atlas(faces), False, K.directions()), "one level")
    finally:
        cube.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 8. refusals
def test_a_plain_c_caller_uses_cube_maps_through_the_abi():
    """tests/c/cubemap_smoke.c: gcc + dlopen, no C++ / HIP headers."""
    import os
    import spawner
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c")
    spawner.run(["make", "-C", here, "-f", "cubemap_smoke.mk", "-s"], check=True)
    out = spawner.run([os.path.join(here, "cubemap_smoke"), _native.LIB_PATH], timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wrong=0 refused=-1" in out.stdout


def test_refusals_leave_the_texels_and_the_context_alone(device):
    from test_gpu_render_to_texture import hip_device_count
    from softwarerenderer_amd import Device
    lib, ctx = device._lib, device._ctx
    n = 8
    faces, words = K.colour_faces(n, 6), K.depth_faces(n, 6)
    cube, depth, flat = Texture.Cube(device, faces), Texture.CubeDepth(device, n, words), Texture.Target(device, n, 6 * n)
    win = MainWindow(device, 2 * n, 2 * n)
    win.Upload(color=T.pool_plane(2 * n, 2 * n, 9), depth=D.depth_pool_plane(2 * n, 2 * n, 9))
    post = PostProgram(device, "__device__ float4 swr_post(const swr_post_in& in, const swr_post_env& env) {\n    return in.color;\n}\n")
    other = Device(0)
    out = np.zeros((n, n, 4), dtype=np.uint8)
    f4, i4, h = np.zeros(16, dtype=F32), np.full(4, -7, dtype=np.int32), C.c_void_p()
    from_frame, from_depth, from_post = lib.swr_texture_update_face_from_frame, lib.swr_texture_update_face_from_depth, lib.swr_texture_update_face_from_post

    def refused(code, words_, rc):
        assert rc == code, (words_, rc)
        assert words_ in lib.swr_last_error(ctx).decode(), (words_, lib.swr_last_error(ctx).decode())
    try:
        syncs = device.sync_count()
        refused(INVALID, "texture is null", from_frame(ctx, None, 0, None, 2, 2, 0))
        refused(INVALID, "texture is null", from_depth(ctx, None, 0, None, 2, 2, 0))
        for face in (-1, 6, 1 << 20):
            refused(INVALID, "face must be 0 .. 5", from_frame(ctx, cube._h, face, None, 2, 2, 0))
            refused(INVALID, "face must be 0 .. 5", from_depth(ctx, depth._h, face, None, 2, 2, 0))
            refused(INVALID, "face must be 0 .. 5", from_post(ctx, cube._h, face, None, post._id, 2, 2, 0))
            refused(INVALID, "face must be 0 .. 5", lib.swr_texture_readback_face(ctx, cube._h, face, 0, out.ctypes.data))
        refused(INVALID, "not a cube map", from_frame(ctx, flat._h, 0, None, 2, 2, 0))
        refused(INVALID, "not a cube map", lib.swr_texture_readback_face(ctx, flat._h, 0, 0, out.ctypes.data))
        refused(INVALID, "not a cube map", lib.swr_texture_sample_cube(ctx, flat._h, f4.ctypes.data, 1, f4.ctypes.data))
        refused(INVALID, "is a depth texture", from_frame(ctx, depth._h, 0, None, 2, 2, 0))
        refused(INVALID, "is a depth texture", from_post(ctx, depth._h, 0, None, post._id, 2, 2, 0))
        refused(INVALID, "is not a depth texture", from_depth(ctx, cube._h, 0, None, 2, 2, 0))
        refused(INVALID, "is a depth texture", lib.swr_texture_sample_cube(ctx, depth._h, f4.ctypes.data, 1, f4.ctypes.data))
        refused(INVALID, "is not a depth texture", lib.swr_texture_sample_cube_depth(ctx, cube._h, f4.ctypes.data, 1, f4.ctypes.data))
        for kx, ky in ((3, 2), (2, 0), (16, 2)):
            refused(INVALID, "factors must be 1, 2, 4 or 8", from_frame(ctx, cube._h, 0, None, kx, ky, 0))
            refused(INVALID, "factors must be 1, 2, 4 or 8", from_depth(ctx, depth._h, 0, None, kx, ky, 0))
        for kx, ky in ((1, 1), (2, 4), (4, 2)):
            refused(INVALID, "n * kx by n * ky", from_frame(ctx, cube._h, 0, None, kx, ky, 0))
            refused(INVALID, "n * kx by n * ky", from_depth(ctx, depth._h, 0, None, kx, ky, 0))
        refused(INVALID, "alpha_mode", from_frame(ctx, cube._h, 0, None, 2, 2, 2))
        refused(INVALID, "reduce must be", from_depth(ctx, depth._h, 0, None, 2, 2, 3))
        refused(INVALID, "unknown or destroyed post program", from_post(ctx, cube._h, 0, None, 1 << 20, 2, 2, 0))
        refused(INVALID, "outside the levels", lib.swr_texture_readback_face(ctx, cube._h, 0, 1, out.ctypes.data))
        refused(INVALID, "outside the levels", lib.swr_texture_readback_face(ctx, cube._h, 0, -1, out.ctypes.data))
        # creation: n < 1, and 6 n^2 at or above the limit of 2^30 texels
        for bad in (0, -3, 13378):
            assert lib.swr_texture_create_cube(ctx, None, bad, C.byref(h)) == INVALID and not h.value, bad
            assert lib.swr_texture_create_cube_depth(ctx, None, bad, C.byref(h)) == INVALID and not h.value, bad
        assert lib.swr_texture_create_cube(ctx, None, 4, None) == INVALID
        assert 6 * 13378 ** 2 >= 1 << 30 > 6 * 13377 ** 2
        # NULL pointers and negative counts of the batches
        assert lib.swr_texture_is_cube(ctx, None, i4.ctypes.data_as(C.POINTER(C.c_int))) == INVALID and lib.swr_texture_is_cube(ctx, cube._h, None) == INVALID
        assert lib.swr_texture_readback_face(ctx, cube._h, 0, 0, None) == INVALID and lib.swr_texture_readback_face(ctx, None, 0, 0, out.ctypes.data) == INVALID
        assert lib.swr_texture_cube_face(ctx, None, 1, i4.ctypes.data, f4.ctypes.data) == INVALID
        assert lib.swr_texture_cube_face(ctx, f4.ctypes.data, 1, None, f4.ctypes.data) == INVALID
        assert lib.swr_texture_cube_face(ctx, f4.ctypes.data, -1, i4.ctypes.data, f4.ctypes.data) == INVALID
        assert lib.swr_texture_cube_face(ctx, f4.ctypes.data, 0, i4.ctypes.data, f4.ctypes.data) == _native.SWR_OK
        for fn, t in ((lib.swr_texture_sample_cube, cube), (lib.swr_texture_sample_cube_depth, depth)):
            assert fn(ctx, None, f4.ctypes.data, 1, f4.ctypes.data) == INVALID and fn(ctx, t._h, None, 1, f4.ctypes.data) == INVALID
            assert fn(ctx, t._h, f4.ctypes.data, 1, None) == INVALID and fn(ctx, t._h, f4.ctypes.data, -1, f4.ctypes.data) == INVALID
            assert fn(ctx, t._h, f4.ctypes.data, 0, f4.ctypes.data) == _native.SWR_OK
        assert device.sync_count() == syncs
        # a source that holds a band of its frame, and one on another device
        cam = MainWindow(other, 8 * n, 8 * n)
        cam.SetBand(1, 1)
        refused(UNSUPPORTED, "only a band", from_frame(ctx, cube._h, 0, other._ctx, 8, 8, 0))
        refused(UNSUPPORTED, "only a band", from_depth(ctx, depth._h, 0, other._ctx, 8, 8, 0))
        cam.SetBand(-1, -1)
        if hip_device_count() > 1:
            far = Device(1)
            try:
                MainWindow(far, 8 * n, 8 * n)
                refused(UNSUPPORTED, "another device", from_frame(ctx, cube._h, 0, far._ctx, 8, 8, 0))
            finally:
                far.close()
        assert not out.any() and not f4.any() and (i4 == -7).all(), "a refused call wrote its destination"
        same_bytes(cube.Read(), K.atlas(faces), "after the refusals")
        same_words(depth.ReadDepth(), K.atlas(words), "after the refusals")
        assert not flat.Read().any() and cube.Levels == 1
        # ... and both contexts still work: a refused call, accepted, from the other context
        colour = T.pool_plane(8 * n, 8 * n, 11)
        cam.Upload(color=colour)
        cube.UpdateFaceFrom(2, cam, 8, 8)
        same_bytes(cube.ReadFace(2), T.texels(colour, 8, 8), "from the other context")
        same_bytes(cube.ReadFace(1), faces[1], "the neighbour")
    finally:
        post.close(); cube.Dispose(); depth.Dispose(); flat.Dispose(); other.close()
    run_both(device, scenes.cfg2(160, 120, 200, seed=3))
