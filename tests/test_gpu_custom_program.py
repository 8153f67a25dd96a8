"""User fragment programs (swr_program_create, include/swr.h) on the GPU.

Each program restates a built-in one against the source contract (csrc/swr_program.hip.h) and must reproduce it BIT FOR BIT --
depth words, colour words and swr_stats -- which also ties it to the oracle through the built-in's own parity."""
import dataclasses
import os

import numpy as np
import pytest

from softwarerenderer_amd import Device, _native, scenes
from softwarerenderer_amd import _native as N
from softwarerenderer_amd.rasterizer import BlendMode, CullMode, DebugMode, DepthTest, MainWindow, Program, Rasterizer, Shaders
from softwarerenderer_amd.modelloader import Model
from util import assert_frame_parity, render_oracle

pytestmark = pytest.mark.gpu

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")

# Renderer.FragmentShader, Renderer.cs:848-860
DUST2 = r"""
__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {
    const swr_uniforms& u = env.uniforms;
    const float3 to_light = make_float3(-u.light_direction[0], -u.light_direction[1], -u.light_direction[2]);
    const float diffuse = swr_max(0.25f, swr_dot3(in.world_normal, to_light));
    const float4 tc = swr_sample(env, in.tex_coord);
    const float4 base = make_float4(in.color.x * tc.x, in.color.y * tc.y, in.color.z * tc.z, in.color.w * tc.w);
    const float depth = in.clip_position.z;
    float fog = swr_clamp((u.fog_end - depth) / (u.fog_end - u.fog_start), 0.0f, 1.0f);
    fog = fog * fog * (3.0f - 2.0f * fog);
    const float s = 0.1f + 0.9f * diffuse;
    return make_float4(swr_lerp(u.fog_color[0], base.x * s * u.light_color[0], fog),
                       swr_lerp(u.fog_color[1], base.y * s * u.light_color[1], fog),
                       swr_lerp(u.fog_color[2], base.z * s * u.light_color[2], fog), base.w);
}
"""
# the same, but a texel whose alpha is below 0.5 discards the fragment
DUST2_DISCARD = DUST2.replace("const float4 base =", "if (tc.w < 0.5f) return swr_discard();\n    const float4 base =")
VERTEX_COLOUR = "__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) { return in.color; }\n"
# shade_debug_varyings (csrc/swr_raster.hip.h) = SWR_PROG_DEBUG_VARYINGS
VARYINGS = r"""
__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {
    return make_float4(in.screen_coords.x + in.normal.x, in.screen_coords.y + in.normal.y,
                       in.barycentric.x + in.normal.z, in.barycentric.y + 0.5f);
}
"""
CONSTANT_COLOUR = r"""
__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {
    return make_float4(env.constants[0], env.constants[1], env.constants[2], env.constants[3]);
}
"""


@pytest.fixture(scope="module")
def device():
    dev = Device(0)
    yield dev
    dev.close()


def with_programs(scene, programs):
    """A copy of `scene` whose draw i uses programs[i % len(programs)] (built-in enum or user id)."""
    draws = [dataclasses.replace(d, program=programs[i % len(programs)]) for i, d in enumerate(scene.draws)]
    return dataclasses.replace(scene, draws=draws)


def render(dev, scene):
    dev.reset_stats()
    r = scenes.SceneRenderer(dev, scene)
    c, d = r.render()
    st = dev.stats()
    r.close()
    return c, d, st


def assert_identical(a, b, what, stats=True):
    (ca, da, sa), (cb, db, sb) = a, b
    assert np.array_equal(da.view(np.uint32), db.view(np.uint32)), f"{what}: depth words differ"
    diff = ca.view(np.uint32) != cb.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} colour words differ"
    if stats:
        assert sa == sb, f"{what}: stats differ {sa} vs {sb}"
    else:
        for k in ("fragments_tested", "fragments_shaded", "fragments_written", "triangles_setup"):
            assert sa[k] == sb[k], f"{what}: {k} {sa[k]} vs {sb[k]}"


def dust2_scenes():
    yield scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=64, seed=5)
    yield scenes.from_model(Model().LoadModel(os.path.join(MODELS, "dust2", "scene.gltf")), 320, 240, name="dust2")
    yield scenes.near_clip_scene()


def test_dust2_restatement_equals_the_builtin_and_the_oracle(device):
    pid = device.compile_program(DUST2)
    assert pid >= N.SWR_PROG_USER_BASE
    for scene in dust2_scenes():
        want = render(device, scene)
        got = render(device, with_programs(scene, [pid]))
        assert got[2]["fragments_written"] > 0
        assert_identical(got, want, scene.name)
        rc, rd, _ = render_oracle(scene)
        assert_frame_parity(got[0], got[1], rc, rd, color_ulp=1, what=f"custom/{scene.name}")
    device.destroy_program(pid)


def test_bilinear_texture_is_sampled_as_the_builtin_does(device):
    pid = device.compile_program(DUST2)
    scene = scenes.cfg3(256, 192, (2, 2), (12, 8), tex_size=64, seed=9, bilinear=True)
    assert_identical(render(device, with_programs(scene, [pid])), render(device, scene), "bilinear")
    device.destroy_program(pid)


@pytest.mark.parametrize("depth_test", list(DepthTest))
def test_vertex_colour_equals_gouraud_under_every_depth_test_and_blend(device, depth_test):
    pid = device.compile_program(VERTEX_COLOUR)
    for blend in BlendMode:
        base = scenes.cfg2(200, 150, 600, seed=3)
        base.draws[0] = dataclasses.replace(base.draws[0], program=Program.Gouraud, depth_test=depth_test, blend=blend)
        assert_identical(render(device, with_programs(base, [pid])), render(device, base), f"{depth_test.name}/{blend.name}")
    device.destroy_program(pid)


def test_varyings_restatement_equals_debug_varyings(device):
    pid = device.compile_program(VARYINGS)
    for scene in (scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=32, seed=71, program=Program.DebugVaryings),
                  scenes.near_clip_scene(program=Program.DebugVaryings),
                  scenes.state_scene(program=Program.DebugVaryings, blend=BlendMode.None_, seed=72)):
        got = render(device, with_programs(scene, [pid]))
        assert_identical(got, render(device, scene), scene.name)
        rc, rd, _ = render_oracle(scene)
        assert_frame_parity(got[0], got[1], rc, rd, color_ulp=1, what=f"custom/{scene.name}")
    device.destroy_program(pid)


@pytest.mark.parametrize("blend", [BlendMode.Alpha, BlendMode.None_])
def test_discard_equals_the_builtin_on_a_binary_alpha_texture(device, blend):
    scene = scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=64, seed=13)
    tex = scene.textures[0].copy()
    tex[..., 3] = np.where(np.random.default_rng(4).uniform(size=tex.shape[:2]) < 0.5, 0, 255).astype(np.uint8)
    scene = dataclasses.replace(scene, textures=[tex], draws=[dataclasses.replace(d, blend=blend) for d in scene.draws])
    pid = device.compile_program(DUST2_DISCARD)
    got, want = render(device, with_programs(scene, [pid])), render(device, scene)
    assert want[2]["fragments_written"] < want[2]["fragments_shaded"]      # the texture's zero alpha does reject fragments
    assert_identical(got, want, f"discard/{blend.name}")
    device.destroy_program(pid)


def _two_triangles():
    s = scenes.cfg2(160, 120, 300, seed=21)
    d = s.draws[0]
    n = d.indices.size // 2 // 3 * 3
    return s, d, [d.indices[:n], d.indices[n:]]


def test_constants_are_captured_per_draw(device):
    s, d, halves = _two_triangles()
    consts = [(0.25, 0.5, 0.75, 1.0), (0.9, 0.1, 0.3, 0.6)]

    def frame(draws):             # [(vertices, indices, ShaderProgram)]
        w = MainWindow(device, s.width, s.height)
        w.ClearDepthBuffer(); w.ClearColorBuffer(s.clear_color)
        device.reset_stats()
        for v, idx, prog in draws:
            Rasterizer.RenderMesh(w, v, idx, d.model, d.view, d.projection, prog.VertexShader, prog.FragmentShader,
                                  CullMode.None_, DepthTest.LessEqual, BlendMode.Alpha)
        c, z = w._read(True, True)
        return c, z, device.stats()

    # two draws of ONE program, other constants set between them (Shaders.Custom sets them before each draw) ...
    custom = Shaders.Custom(CONSTANT_COLOUR)
    pid = custom._program_for(device)
    w = MainWindow(device, s.width, s.height)
    w.ClearDepthBuffer(); w.ClearColorBuffer(s.clear_color)
    device.reset_stats()
    for idx, k in zip(halves, consts):
        custom.constants = k
        Rasterizer.RenderMesh(w, d.vertices, idx, d.model, d.view, d.projection, custom.VertexShader, custom.FragmentShader,
                              CullMode.None_, DepthTest.LessEqual, BlendMode.Alpha)
    device.set_program_constants(pid, (0.0, 0.0, 0.0, 0.0))         # ... and once more after recording: changes nothing
    c, z = w._read(True, True)
    got = (c, z, device.stats())
    flat = []
    for idx, k in zip(halves, consts):
        v = d.vertices.copy()
        v["color"][:] = np.asarray(k, dtype=np.float32)
        flat.append((v, idx, Shaders.FlatColor()))
    want = frame(flat)
    assert_identical(got, want, "constants")
    assert got[2]["fragments_written"] > 0


@pytest.mark.parametrize("pipelining", [0, 1])
def test_mixed_frame_equals_the_builtin_twins(device, pipelining):
    a, b = device.compile_program(DUST2), device.compile_program(VERTEX_COLOUR)
    scene = scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=64, seed=17)
    device.set_pipelining(pipelining)
    try:
        for _ in range(2):              # (a second frame: pipelined flushes alternate raster sets)
            got = render(device, with_programs(scene, [Program.Dust2LambertFog, a, b, Program.Dust2LambertFog]))
            want = render(device, with_programs(scene, [Program.Dust2LambertFog, Program.Dust2LambertFog, Program.Gouraud,
                                                        Program.Dust2LambertFog]))
            assert_identical(got, want, f"mixed/pipelining={pipelining}", stats=False)
    finally:
        device.set_pipelining(1)
    device.destroy_program(a); device.destroy_program(b)


def test_errors(device):
    lib, ctx = device._lib, device._ctx
    pid = N.C.c_int(0)
    rc = lib.swr_program_create(ctx, b"__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) { return in.colr; }\n",
                                N.C.byref(pid))
    assert rc == N.SWR_ERR_INVALID_ARG
    assert "colr" in lib.swr_last_error(ctx).decode()
    # the context renders correctly afterwards
    scene = scenes.cfg3(192, 128, (1, 1), (8, 6), tex_size=32, seed=3)
    c, d, _ = render(device, scene)
    rc_, rd_, _ = render_oracle(scene)
    assert_frame_parity(c, d, rc_, rd_, color_ulp=1, what="after a compile error")

    good = device.compile_program(VERTEX_COLOUR)
    device.destroy_program(good)
    mesh = scenes.SceneRenderer(device, scene)
    I = np.eye(4, dtype=np.float32).reshape(-1).ctypes.data_as(N.C.POINTER(N.C.c_float))
    for bad in (good, N.SWR_PROG_USER_BASE + 100000):
        assert lib.swr_render_mesh(ctx, mesh.meshes[0]._h, I, I, I, bad, None, None, 0, 2, 1) == N.SWR_ERR_INVALID_ARG
        assert lib.swr_program_destroy(ctx, bad) == N.SWR_ERR_INVALID_ARG
        assert lib.swr_program_set_constants(ctx, bad, None, 0) == N.SWR_ERR_INVALID_ARG

    # DebugMode.Wireframe
    live = device.compile_program(VERTEX_COLOUR)
    lib.swr_set_state(ctx, 0.1, 1000.0, int(DebugMode.Wireframe))
    assert lib.swr_render_mesh(ctx, mesh.meshes[0]._h, I, I, I, live, None, None, 0, 2, 1) == N.SWR_ERR_UNSUPPORTED
    lib.swr_set_state(ctx, 0.1, 1000.0, int(DebugMode.None_))
    mesh.close()

    # destroyed after recording: its draws still render
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


def test_fma_build_restatement_equals_its_own_builtin():
    lib = "libswr_hip_fma.so"
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it")
    dev = Device(0, lib=lib)
    try:
        assert dev.numerics_mode()[0] == 1
        pid = dev.compile_program(DUST2)
        for scene in (scenes.cfg3(320, 256, (2, 2), (16, 12), tex_size=64, seed=5), scenes.near_clip_scene()):
            assert_identical(render(dev, with_programs(scene, [pid])), render(dev, scene), f"fma/{scene.name}")
    finally:
        dev.close()
