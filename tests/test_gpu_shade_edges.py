"""The shading edge families of tests/shade_edge_scenes.py on the GPU.

Every scene: the product library against the oracle at the project's bar (depth words bit-exact, colour <= 1 ULP, six counters
equal).  Then, with NO tolerance, word for word: the pure scene (specialised kernel: shade_dust2_fast / shade_phong4_fast, ballot,
re-shade) against the diluted one (generic kernel: shade_fragment only), both from the product library, and both against the
fenced general test build libswr_hip_test.so.  The design's claim is that a verified speculative value IS the guarded one, so the
same frame through the two kernels of one library must not differ in a single bit -- a check the 1 ULP oracle bar cannot make.

Colour words that are NaN in both frames are compared as NaN-ness only.  That is enough: a lane's speculative value is used only
when every lane of its chunk is verified, and a verified lane has no NaN among the operands of the substituted v_max / v_med3
(the normal's length, the fog quotient and the light direction are finite), so a NaN in a frame never comes out of the
substitution; it comes from NaN inputs (colours, uniforms, UVs) through the same + and * in both kernels, where only the payload
-- which the hardware may pick from either operand -- is free.

tests/test_shade_edges_host.py shows on the CPU that these scenes put fragments on both sides of every guard, and that every
`safe` term fails ALONE in some whole triangle that is alone in its tile (the verification is per chunk, so only that is a test).

Mutant builds (kernel sources changed on a scratch copy, one change each, run once through this file; the suite as it was before
this file passed under every one of the first nine, the others were not run through it):
  caught   texel index term dropped (S2 1x7, 7x1, 37x53, 16x16: pure != oracle);  `len_sq > 1e-6` dropped (S3 special);
           dust2_fast_applies without `fog_r1 != 0` (S4) and without finite_l (S5);  need_exact forced false (17 cases);
           shade_phong4_fast without unit()'s condition and without the range condition (S6 cores);
           representatives not barred by `frustum_cull` (S8: a material shared with a culled draw has fog_den = 0)
  not caught, because the term is sufficient and not necessary -- the cores ARE the IEEE operation on a wider range than the
  guard states, and where they are not, another term fails too:
    fastdiv, weights, fog_num (division core): v_div_scale rescales only for an exponent difference >= 96, a denormal operand or
        quotient, or |n| < 2^-103.  S1 "perw" has clip.w = 2^+-90 .. 2^+-127 and S1 "far" weights down to 1e-15 with identical
        frames; a fog quotient that small or that large is clamped to 0 or 1 before it is used, and a weight of exactly 0 gives
        the quotient 0 from either sequence.
    |inv_sum| >= 2^-40 (both shaders): with clip.w and weights in range a cancelled sum is 0 or above 2^-87, where recip_core is
        still the division; at exactly 0 the weights are infinite and `len_sq` fails its own term.
    len_sq <= 1e12 (both shaders): sqrt_core needs no scaling up to FLT_MAX and its result is inside recip_core's range; +Inf
        comes only with inv_sum == 0.
    re-shade of unsafe lanes only: equal by design -- a verified lane's speculative value is the guarded one, which is what
        pure == diluted asserts; the whole-chunk re-shade is a choice of control flow, not of values.
    frag_reps cap removed: the cap bounds host time only; draws past it represent themselves (S8 crosses it both ways).
    `n_verts > 0` removed: unreachable through the API -- record_draw drops a draw without triangles, and a mesh with indices has
        vertices (make_mesh checks every index); the condition is kept as a statement of what a representative needs.
  These terms stay: they are the ranges for which the cores' exactness is PROVED (swr_device.h), and they cost one compare."""
import dataclasses
import os
import time

import numpy as np
import pytest

import shade_edge_scenes as S
from softwarerenderer_amd import Device, _native, scenes
from softwarerenderer_amd.rasterizer import Rasterizer
from test_gpu_custom_program import DUST2 as DUST2_SOURCE
from test_gpu_parity import run_both
from util import assert_frame_parity

pytestmark = pytest.mark.gpu

PAIRS = S.pairs(0)
T0 = time.time()


@pytest.fixture(scope="module")
def testlib_device():
    lib = "libswr_hip_test.so"
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it (make -C softwarerenderer_amd/csrc variants)")
    dev = Device(0, lib=lib)
    yield dev
    dev.close()


def _render(dev, scene):
    dev.reset_stats()
    r = scenes.SceneRenderer(dev, scene)
    c, d = r.render()
    st = dev.stats()
    r.close()
    return c, d, st


def assert_same_words(a, b, what):
    (ca, da, sa), (cb, db, sb) = a, b
    bad = da.view(np.uint32) != db.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} depth words differ, first at (y, x) = {tuple(np.argwhere(bad)[0])}"
    nan = np.isnan(ca) & np.isnan(cb)
    bad = (ca.view(np.uint32) != cb.view(np.uint32)) & ~nan
    if bad.any():
        y, x, ch = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} colour words differ, first at (x={x}, y={y}, channel {ch}): "
                             f"{ca[y, x, ch]!r} against {cb[y, x, ch]!r}")
    for k in ("fragments_tested", "fragments_shaded", "fragments_written"):
        assert sa[k] == sb[k], (what, k, sa[k], sb[k])


@pytest.mark.parametrize("idx", range(len(PAIRS)), ids=[p.name[len("shade_"):-len("_pure")] for p, _ in PAIRS])
def test_pure_and_diluted_match_the_oracle_and_each_other_word_for_word(device, testlib_device, idx):
    pure, diluted = PAIRS[idx]
    assert S.predicted_kernel(pure) in ("dust2_default", "phong_default") and S.predicted_kernel(diluted).startswith("generic")
    _, st = run_both(device, pure)
    run_both(device, diluted)
    assert st["fragments_written"] > 0, f"{pure.name}: nothing was drawn"
    p, d = _render(device, pure), _render(device, diluted)
    assert_same_words(p, d, f"{pure.name}: specialised against generic kernel")
    assert_same_words(p, _render(testlib_device, pure), f"{pure.name}: product against test build")
    assert_same_words(d, _render(testlib_device, diluted), f"{diluted.name}: product against test build")


def test_user_program_restating_dust2_equals_the_builtin_on_s2_to_s5(device):
    """S2-S5 (DUST2 scenes) through a user fragment program that restates Renderer.FragmentShader: word for word the built-in's
    frame, as tests/test_gpu_custom_program.py asserts for ordinary scenes."""
    pid = device.compile_program(DUST2_SOURCE)
    try:
        n = 0
        for pure, _ in S.pairs(0, ("s2", "s3", "s4", "s5")):
            if pure.draws[0].program != S.DUST2:
                continue
            user = dataclasses.replace(pure, draws=[dataclasses.replace(d, program=pid) for d in pure.draws])
            assert_same_words(_render(device, user), _render(device, pure), f"{pure.name}: user program against built-in")
            n += 1
        assert n >= 10
    finally:
        device.destroy_program(pid)


def test_fused_lerp_build_matches_the_oracle_built_alike_on_s1_to_s5():
    """S1-S5 once through libswr_hip_fma.so (nm_lerp, the fast shader's last line, fused) against the oracle built with the same
    switch: depth bit-exact, colour <= 1 ULP."""
    from oracle import binding as ob
    lib = "libswr_hip_fma.so"
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it (make -C softwarerenderer_amd/csrc variants)")
    ob.load(variant="fma")
    dev = Device(0, lib=lib)
    try:
        for pure, _ in S.pairs(0, ("s1", "s2", "s3", "s4", "s5")):
            c, d, st = _render(dev, pure)
            o = ob.OracleRenderer(pure.width, pure.height, variant="fma")
            rc, rd = o.render_scene(pure)
            ost = o.stats(); o.close()
            assert_frame_parity(c, d, rc, rd, color_ulp=1, what=f"fma/{pure.name}")
            assert st["fragments_written"] == ost["fragments_written"] > 0
    finally:
        dev.close()


def _submit_with_frustum_flags(dev, scene):
    """The frame through Rasterizer.RenderMesh on retained meshes, each draw with its own frustumCull flag, as ONE batch."""
    r = scenes.SceneRenderer(dev, scene)
    w = r.window
    dev.reset_stats()
    w.ClearDepthBuffer(); w.ClearColorBuffer(scene.clear_color)
    for d, prog, mesh in zip(scene.draws, r.programs, r.meshes):
        Rasterizer.RenderMesh(w, mesh, None, d.model, d.view, d.projection, prog.VertexShader, prog.FragmentShader,
                              d.cull, d.depth_test, d.blend, frustumCull=d.frustum_cull)
    c, dz = w._read()
    st = dev.stats()
    r.close()
    return c, dz, st


def test_s8_material_identity_across_the_representative_cap(device, testlib_device, oracle_lib):
    """S8: 72 materials one bit apart in one batch, behind three decoys that must not become representatives (no vertices;
    frustum-culled and culled; frustum-culled and kept).  The oracle frame holds the draws the host-side decision keeps."""
    from oracle.binding import OracleRenderer
    scene = S.s8_material_identity(0)
    assert S.predicted_kernel(scene) == "dust2_default"
    o = OracleRenderer(scene.width, scene.height)
    o.clear_depth(); o.clear_color(scene.clear_color)
    culled = 0
    for d in scene.draws:
        if d.frustum_cull:
            v = np.ascontiguousarray(d.vertices)
            sph = np.zeros(4, np.float32)
            oracle_lib.oswr_bounding_sphere(v.ctypes.data, v.shape[0], sph.ctypes.data)
            m_, v_, p_ = (np.ascontiguousarray(a, dtype=np.float32) for a in (d.model, d.view, d.projection))
            if not oracle_lib.oswr_is_sphere_in_frustum(sph.ctypes.data, m_.ctypes.data, v_.ctypes.data, p_.ctypes.data):
                culled += 1
                continue
        tex = scene.textures[d.texture] if d.texture is not None else None
        o.render_mesh(d.vertices, d.indices, d.model, d.view, d.projection, int(d.program), d.uniforms, tex,
                      int(d.cull), int(d.depth_test), int(d.blend))
    assert culled == 1
    rst = o.stats()
    got = _submit_with_frustum_flags(device, scene)
    assert_frame_parity(got[0], got[1], o.color, o.depth, 1, scene.name)
    for k in ("triangles_setup", "fragments_tested", "fragments_shaded", "fragments_written"):
        assert got[2][k] == rst[k] > 0, (k, got[2][k], rst[k])
    o.close()
    assert_same_words(got, _submit_with_frustum_flags(testlib_device, scene), f"{scene.name}: product against test build")


def test_report_wall_time():
    print(f"tests/test_gpu_shade_edges.py: {time.time() - T0:.1f} s from import to here ({len(PAIRS)} scene pairs)")
