"""User vertex programs and the user varying data4 (swr_program_create_vf, include/swr.h) on the GPU.

The oracle knows the built-in programs only, so every new path is tied BIT FOR BIT -- depth words, colour words, swr_stats -- to a
path the oracle covers, as tests/test_gpu_custom_program.py does for the fragment half: the restated Renderer.VertexShader against the
built-in vertex stage, a displacing vertex program against the built-in stage on a mesh displaced on the host (one IEEE add has the
same bits in numpy), data4 against Data["WorldNormal"], which the raster stage sums the same way before it renormalises."""
import dataclasses
import os

import numpy as np
import pytest

from softwarerenderer_amd import Device, _native, scenes
from softwarerenderer_amd import _native as N
from softwarerenderer_amd import hostmath as hm
from softwarerenderer_amd.rasterizer import (BlendMode, CullMode, DebugMode, DepthTest, MainWindow, Mesh, Program, Rasterizer,
                                             Shaders)
from softwarerenderer_amd.modelloader import Model
from test_gpu_custom_program import DUST2, VARYINGS, VERTEX_COLOUR, assert_identical, render, with_programs
from util import assert_frame_parity, render_oracle
from vertex_program_texts import (DATA4_PLUS_FS, DATA4_VS, DATA4_XYW_FS, DATA4_XYZ_FS, DISPLACE_VS, QUARTERS_FS, RENDERER_VS,
                                  WORLD_NORMAL_FS)

pytestmark = pytest.mark.gpu

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")


@pytest.fixture(scope="module")
def device():
    dev = Device(0)
    yield dev
    dev.close()


def dust2_scenes():
    yield scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=64, seed=5)
    yield scenes.from_model(Model().LoadModel(os.path.join(MODELS, "dust2", "scene.gltf")), 320, 240, name="dust2")
    yield scenes.near_clip_scene()


def displaced(scene, offset):
    """`scene` with every mesh's positions moved by `offset` on the host, in float32 (what DISPLACE_VS adds on the device)."""
    off = np.asarray(offset, dtype=np.float32)
    draws = []
    for d in scene.draws:
        v = d.vertices.copy()
        v["position"] = v["position"] + off            # float32 + float32: one correctly rounded add per component
        draws.append(dataclasses.replace(d, vertices=v))
    return dataclasses.replace(scene, draws=draws)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,tn", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_restated_vertex_and_fragment_shaders_equal_the_builtin_program(device, tr, tn):
    from oracle import binding as ob
    pid = device.compile_program(DUST2, vertex_source=RENDERER_VS)
    assert pid >= N.SWR_PROG_USER_BASE
    default = device.transform_fma()
    device.set_transform_fma(tr, tn)
    try:
        for scene in dust2_scenes():
            want = render(device, scene)
            got = render(device, with_programs(scene, [pid]))
            assert got[2]["fragments_written"] > 0
            assert_identical(got, want, f"t{tr}n{tn}/{scene.name}")
            o = ob.OracleRenderer(scene.width, scene.height, transform_fma=(tr, tn))
            rc, rd = o.render_scene(scene); o.close()
            assert_frame_parity(got[0], got[1], rc, rd, color_ulp=1, what=f"vertex program/t{tr}n{tn}/{scene.name}")
    finally:
        device.set_transform_fma(*default)
        device.destroy_program(pid)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_normal_travels_through_the_user_vertex_kernel_and_the_clipper(device):
    pid = device.compile_program(VARYINGS, vertex_source=RENDERER_VS)
    for scene in (scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=32, seed=71, program=Program.DebugVaryings),
                  scenes.near_clip_scene(program=Program.DebugVaryings),
                  scenes.state_scene(program=Program.DebugVaryings, blend=BlendMode.None_, seed=72)):
        got = render(device, with_programs(scene, [pid]))
        assert_identical(got, render(device, scene), scene.name)
        rc, rd, _ = render_oracle(scene)
        assert_frame_parity(got[0], got[1], rc, rd, color_ulp=1, what=f"vertex program/{scene.name}")
    assert got[2]["fragments_written"] > 0
    device.destroy_program(pid)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_displacement_equals_the_builtin_stage_on_a_displaced_mesh(device):
    pid = device.compile_program(DUST2, vertex_source=DISPLACE_VS)
    for scene, offset in ((scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=64, seed=5), (0.75, -0.5, 1.25)),
                          (scenes.near_clip_scene(), (0.0625, 0.03, -0.11))):
        device.set_program_constants(pid, offset)
        got = render(device, with_programs(scene, [pid]))
        plain = render(device, scene)
        want = render(device, displaced(scene, offset))
        assert got[2]["fragments_written"] > 0
        assert_identical(got, want, f"displaced/{scene.name}")
        assert not np.array_equal(got[1].view(np.uint32), plain[1].view(np.uint32)), "the displacement moved nothing"
        rc, rd, _ = render_oracle(displaced(scene, offset))
        assert_frame_parity(got[0], got[1], rc, rd, color_ulp=1, what=f"displaced/{scene.name}")
    device.destroy_program(pid)


def test_the_vertex_stage_reads_the_constants_each_draw_captured(device):
    s = scenes.cfg2(160, 120, 300, seed=21)
    d = s.draws[0]
    offsets = [(0.5, 0.25, -1.0), (-0.75, -0.5, -3.0)]

    def begin():
        w = MainWindow(device, s.width, s.height)
        w.ClearDepthBuffer(); w.ClearColorBuffer(s.clear_color)
        device.reset_stats()
        return w

    # two draws of ONE retained mesh with ONE program, other constants set between them ...
    custom = Shaders.Custom(VERTEX_COLOUR, vertex_source=DISPLACE_VS)
    mesh = Mesh(device, d.vertices, d.indices)
    w = begin()
    for k in offsets:
        custom.constants = k
        Rasterizer.RenderMesh(w, mesh, None, d.model, d.view, d.projection, custom.VertexShader, custom.FragmentShader,
                              CullMode.None_, DepthTest.LessEqual, BlendMode.Alpha)
    device.set_program_constants(custom._program_for(device), (9.0, 9.0, 9.0))       # ... and once more after recording: changes nothing
    c, z = w._read(True, True)
    got = (c, z, device.stats())
    mesh.Dispose()
    # ... equal two meshes displaced on the host, through the built-in vertex stage
    w = begin()
    gouraud = Shaders.Gouraud()
    for k in offsets:
        v = d.vertices.copy()
        v["position"] = v["position"] + np.asarray(k, dtype=np.float32)
        Rasterizer.RenderMesh(w, v, d.indices, d.model, d.view, d.projection, gouraud.VertexShader, gouraud.FragmentShader,
                              CullMode.None_, DepthTest.LessEqual, BlendMode.Alpha)
    c, z = w._read(True, True)
    want = (c, z, device.stats())
    assert got[2]["fragments_written"] > 0
    assert_identical(got, want, "per-draw constants in the vertex stage")


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_data4_is_lerped_by_the_clipper_and_summed_by_the_raster_stage(device):
    b = device.compile_program(WORLD_NORMAL_FS, vertex_source=DATA4_VS)
    for name, text in (("xyz", DATA4_XYZ_FS), ("xyw", DATA4_XYW_FS)):
        a = device.compile_program(text, vertex_source=DATA4_VS)
        for scene in (scenes.near_clip_scene(), scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=64, seed=5)):
            got, want = render(device, with_programs(scene, [a])), render(device, with_programs(scene, [b]))
            assert got[2]["fragments_written"] > 0
            if scene.name.startswith("nearclip"):
                assert got[2]["triangles_clipped"] > 0              # the clipper's lerp of data4 is exercised
            assert_identical(got, want, f"data4.{name}/{scene.name}")
        device.destroy_program(a)
    # and Data["WorldNormal"] itself is what the built-in stage delivers: B equals the same fragment text over the built-in vertex stage
    f = device.compile_program(WORLD_NORMAL_FS)
    scene = scenes.near_clip_scene()
    assert_identical(render(device, with_programs(scene, [b])), render(device, with_programs(scene, [f])), "world normal")
    device.destroy_program(b); device.destroy_program(f)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_data4_reads_zero_without_a_vertex_half(device):
    a, b = device.compile_program(DATA4_PLUS_FS), device.compile_program(QUARTERS_FS)
    for scene in (scenes.near_clip_scene(), scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=64, seed=5)):
        got, want = render(device, with_programs(scene, [a])), render(device, with_programs(scene, [b]))
        assert got[2]["fragments_written"] > 0
        assert_identical(got, want, f"data4 = 0/{scene.name}")
    # ... and with a vertex half that leaves it alone (new Shaders.VertexOutput(): zeros), through the k_vertex_user path
    c = device.compile_program(DATA4_PLUS_FS, vertex_source=RENDERER_VS)
    scene = scenes.near_clip_scene()
    assert_identical(render(device, with_programs(scene, [c])), render(device, with_programs(scene, [b])), "data4 untouched")
    for p in (a, b, c):
        device.destroy_program(p)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def band_scene(offset_y=0.0):
    """256 x 256 (16 tile rows): a fan of triangles given in clip space (identity matrices) whose box covers NDC y in [0.5, 0.9] --
    pixel rows 12 .. 64, tile rows 0 .. 4.  Moved by -1.2 in y it covers NDC y in [-0.7, -0.3]: pixel rows 166 .. 218, all inside
    the band of tile rows 10 .. 13 (pixel rows 160 .. 223)."""
    rng = np.random.default_rng(31)
    n = 24
    x0 = np.linspace(-0.9, 0.8, n)
    pos = np.empty((n, 3, 3), dtype=np.float32)
    pos[:, 0] = np.stack([x0, np.full(n, 0.5), rng.uniform(-0.5, 0.5, n)], axis=1)
    pos[:, 1] = np.stack([x0 + 0.1, np.full(n, 0.5), rng.uniform(-0.5, 0.5, n)], axis=1)
    pos[:, 2] = np.stack([x0 + 0.05, np.full(n, 0.9), rng.uniform(-0.5, 0.5, n)], axis=1)
    pos[..., 1] += np.float32(offset_y)
    col = np.concatenate([rng.uniform(0.2, 1.0, (3 * n, 3)), np.ones((3 * n, 1))], axis=1)
    v = scenes.make_vertices(pos.reshape(-1, 3), color=col)
    I = hm.identity()
    d = scenes.Draw(v, np.arange(3 * n, dtype=np.uint16), I, I, I, program=Program.Gouraud, cull=CullMode.None_,
                    depth_test=DepthTest.LessEqual, blend=BlendMode.Alpha)
    return scenes.Scene("band", 256, 256, [d])


BAND = (10, 4)          # tile rows 10 .. 13


def test_a_vertex_program_draw_is_not_dropped_from_a_band_by_the_mesh_box(device):
    offset = (0.0, -1.2, 0.0)
    pid = device.compile_program(VERTEX_COLOUR, vertex_source=DISPLACE_VS)
    device.set_program_constants(pid, offset)
    scene = with_programs(band_scene(), [pid])
    whole = render(device, scene)
    y0, y1 = BAND[0] * 16, (BAND[0] + BAND[1]) * 16
    # the whole frame is the built-in stage's frame of the mesh displaced on the host, and that one writes into the band's rows
    want = render(device, band_scene(np.float32(-1.2)))
    assert_identical(whole, want, "band/whole frame")
    assert (want[1][y0:y1] != want[1][0, 0]).any() and not (want[1][:y0] != want[1][0, 0]).any()
    rc, rd, _ = render_oracle(band_scene(np.float32(-1.2)))
    assert_frame_parity(whole[0], whole[1], rc, rd, color_ulp=1, what="band/whole frame")
    # the band alone (retained mesh: it carries the box band_rejects reads -- a box that lies wholly above this band)
    w = MainWindow(device, scene.width, scene.height)
    w.SetBand(*BAND)
    try:
        device.reset_stats()
        r = scenes.SceneRenderer(device, scene, window=w)
        c, z = r.render()
        st = device.stats()
        r.close()
        assert c.shape[0] == y1 - y0
        assert st["fragments_written"] > 0
        assert np.array_equal(z.view(np.uint32), whole[1][y0:y1].view(np.uint32))
        assert np.array_equal(c.view(np.uint32), whole[0][y0:y1].view(np.uint32))
        # the built-in stage on the undisplaced mesh IS dropped here (the box test this draw must not take), and writes nothing
        device.reset_stats()
        r = scenes.SceneRenderer(device, band_scene(), window=w)
        r.render()
        assert device.stats()["triangles_in"] == 0
        r.close()
    finally:
        w.SetBand(-1, -1)
    device.destroy_program(pid)


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_frames_in_flight_mix_builtin_fragment_only_and_vertex_program_draws(device):
    f_only = device.compile_program(DUST2)
    vf = device.compile_program(DUST2, vertex_source=DISPLACE_VS)
    base = scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=64, seed=17)
    tex = scenes.random_texture(64, 117, alpha=None)                 # random alpha: blending makes the order of draws AND frames matter
    base = dataclasses.replace(base, textures=[tex], clear_color=None, clear_depth=True)
    mixes = [[Program.Dust2LambertFog, f_only, vf, Program.Dust2LambertFog], [vf, Program.Dust2LambertFog, f_only, vf],
             [f_only, vf, vf, Program.Gouraud]]
    offsets = [(0.5, 0.0, 0.0), (0.0, -0.4, 0.3), (-0.3, 0.2, 0.6)]
    frames = {}
    try:
        for mode in (0, 1, 2):
            device.set_pipelining(mode)
            w = MainWindow(device, base.width, base.height)
            w.ClearColorBuffer(scenes.CLEAR_COLOR)
            device.reset_stats()
            before = device.replay_count()
            renderers = []
            for mix, off in zip(mixes, offsets):                   # three frames back to back, colour kept: nothing read in between
                device.set_program_constants(vf, off)
                r = scenes.SceneRenderer(device, with_programs(base, mix), window=w)
                r.submit_frame(); device.flush()
                renderers.append(r)
            c, z = w._read(True, True)
            frames[mode] = (c, z, device.stats())
            print(f"pipelining {mode}: swr_replay_count +{device.replay_count() - before}")
            for r in renderers:
                r.close()
    finally:
        device.set_pipelining(1)
    assert frames[0][2]["fragments_written"] > 0
    assert_identical(frames[1], frames[0], "pipelining 1 vs 0")
    assert_identical(frames[2], frames[0], "pipelining 2 vs 0")
    device.destroy_program(f_only); device.destroy_program(vf)


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_render_mesh_culled_keeps_the_mesh_bounds_test(device):
    scene = scenes.cfg3(256, 192, (1, 1), (12, 8), tex_size=32, seed=9)
    d = scene.draws[0]
    away = hm.multiply(d.model, hm.create_translation(500.0, 0.0, 0.0)).astype(np.float32)     # far outside the frustum
    vf = Shaders.Custom(DUST2, uniforms=d.uniforms, vertex_source=RENDERER_VS)
    f_only = Shaders.Custom(DUST2, uniforms=d.uniforms)
    mesh = Mesh(device, d.vertices, d.indices)

    def frame(prog, draws):             # [(model, frustumCull)]
        w = MainWindow(device, scene.width, scene.height)
        w.ClearDepthBuffer(); w.ClearColorBuffer(scene.clear_color)
        device.reset_stats()
        for model, cull in draws:
            Rasterizer.RenderMesh(w, mesh, None, model, d.view, d.projection, prog.VertexShader, prog.FragmentShader,
                                  d.cull, d.depth_test, d.blend, frustumCull=cull)
        c, z = w._read(True, True)
        return c, z, device.stats()

    outside = frame(vf, [(away, True)])
    assert outside[2]["fragments_written"] == 0 and outside[2]["triangles_in"] == 0
    assert (outside[1] == outside[1][0, 0]).all()
    assert_identical(outside, frame(f_only, [(away, True)]), "culled, outside")
    # a visible and a culled draw in ONE batch: k_vertex_user's visible[] return beside blocks that run
    both = frame(vf, [(away, True), (d.model, True)])
    assert both[2]["fragments_written"] > 0
    assert_identical(both, frame(f_only, [(away, True), (d.model, True)]), "culled, mixed batch")
    assert_identical(frame(vf, [(d.model, True)]), frame(vf, [(d.model, False)]), "culled, inside")
    mesh.Dispose()


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors(device):
    lib, ctx = device._lib, device._ctx
    pid = N.C.c_int(0)
    bad_vs = RENDERER_VS.replace("out.color = in.color;", "out.color = in.colr;")
    line = bad_vs.splitlines().index("    out.color = in.colr;") + 1
    rc = lib.swr_program_create_vf(ctx, bad_vs.encode(), VERTEX_COLOUR.encode(), N.C.byref(pid))
    assert rc == N.SWR_ERR_INVALID_ARG
    err = lib.swr_last_error(ctx).decode()
    assert "colr" in err and f"vertex.hip:{line}:" in err, err
    rc = lib.swr_program_create_vf(ctx, b"__device__ void nothing() {}\n", VERTEX_COLOUR.encode(), N.C.byref(pid))
    assert rc == N.SWR_ERR_INVALID_ARG and "swr_vertex" in lib.swr_last_error(ctx).decode()
    # the context renders correctly afterwards
    scene = scenes.cfg3(192, 128, (1, 1), (8, 6), tex_size=32, seed=3)
    c, d, _ = render(device, scene)
    rc_, rd_, _ = render_oracle(scene)
    assert_frame_parity(c, d, rc_, rd_, color_ulp=1, what="after a vertex compile error")

    # DebugMode.Wireframe
    live = device.compile_program(VERTEX_COLOUR, vertex_source=RENDERER_VS)
    mesh = scenes.SceneRenderer(device, scene)
    I = np.eye(4, dtype=np.float32).reshape(-1).ctypes.data_as(N.C.POINTER(N.C.c_float))
    lib.swr_set_state(ctx, 0.1, 1000.0, int(DebugMode.Wireframe))
    assert lib.swr_render_mesh(ctx, mesh.meshes[0]._h, I, I, I, live, None, None, 0, 2, 1) == N.SWR_ERR_UNSUPPORTED
    lib.swr_set_state(ctx, 0.1, 1000.0, int(DebugMode.None_))
    mesh.close()

    # destroyed after recording: its draws still render, vertex kernel included
    user = with_programs(scene, [live])
    r = scenes.SceneRenderer(device, user)
    device.reset_stats()
    r.submit_frame()
    device.destroy_program(live)
    got = r.window._read(True, True)
    st = device.stats()
    r.close()
    want = render(device, with_programs(scene, [Program.Gouraud]))
    assert_identical((got[0], got[1], st), want, "destroyed after recording")


# 10 --------------------------------------------------------------------------------------------------------------------------------
def test_fma_build_vertex_program_equals_its_own_builtin():
    lib = "libswr_hip_fma.so"
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it")
    dev = Device(0, lib=lib)
    try:
        assert dev.numerics_mode()[0] == 1
        pid = dev.compile_program(DUST2, vertex_source=RENDERER_VS)
        a, b = dev.compile_program(DATA4_XYW_FS, vertex_source=DATA4_VS), dev.compile_program(WORLD_NORMAL_FS, vertex_source=DATA4_VS)
        for scene in (scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=64, seed=5), scenes.near_clip_scene()):
            assert_identical(render(dev, with_programs(scene, [pid])), render(dev, scene), f"fma/{scene.name}")
            assert_identical(render(dev, with_programs(scene, [a])), render(dev, with_programs(scene, [b])), f"fma/data4/{scene.name}")
    finally:
        dev.close()
