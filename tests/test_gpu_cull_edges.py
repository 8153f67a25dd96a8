"""The frustum-culler edge cases of tests/cull_edge_cases.py on the GPU: k_bounding_sphere, sphere_in_frustum behind k_frustum_test
and k_frustum_cull (csrc/swr_cull.hip.h) against the oracle, with no tolerance anywhere.

  - spheres: every family B1-B6 on the product build, B1 / B2 / B6 on the five System.Numerics sensitivity builds against the oracle
    built alike -- the same 32-bit words (cull_edge_cases.same_words: a NaN word of the oracle must be a NaN word here);
  - threshold decisions: every F case at its threshold radius r* and 1, 2, 8 ULP either side: rejected below, accepted from r* on,
    and equal to the oracle at each radius; product build under the run-time Transform flags (0,0), (1,1), (1,0), each
    sensitivity build under its default flags; F3's degenerate decisions everywhere;
  - batch: ONE flush of 130 RenderMesh draws (three blocks of k_frustum_cull, the last with two threads) at threshold translations,
    every third without the cull request; the pattern and its complement, pipelining 0 and 1;
  - flags captured per draw: one batch whose draws were recorded under alternating Transform flags at translations where the two
    flags decide differently.

A sphere tangent to a frustum plane from outside holds nothing visible, so in the batch tests the decisions are read from
triangles_in (a culled draw's triangles never enter); the frame is compared as well and must stay the oracle's.

tests/test_cull_edges_host.py shows on the CPU that the cases are what they claim to be.

Device mutant (one change in a scratch copy of csrc/, the product library rebuilt, this file run once on it): `>=` for `>` in
sphere_in_frustum fails test_threshold_decisions_on_the_product_build under all three flag settings and all four cases of
test_batch_of_130_draws_at_threshold_translations (7 of the 14 product tests).  The same change in the oracle moves 83 of the 84
thresholds (42 cases x 2 flags): at almost every case the radius below r* gives dist == -worldRadius exactly.

What B6 found: DistanceSquared / Distance are Dot(d, d), and the kernel's dist_sq3 had the sequential order written out, so
libswr_hip_dotpw.so and libswr_hip_fma_dotpw.so returned the DEFAULT order's sphere: 17 of the 51 spheres of B1 / B2 / B6 differed
from the dotpw oracle (all 15 of B6 and two pass-1 ties of B2).  For b6_cfg3_patch_seed1 both builds gave
c0f470cc c0a6d288 c1a36965 41d019f3 where the dotpw oracle gives c0f470cf c0a6d286 c1a36965 41d019f4; with dist_sq3 routed
through dot3 they give the oracle's words and 0 of 51 differ."""
import os

import numpy as np
import pytest

import cull_edge_cases as K
from oracle import binding as ob
from softwarerenderer_amd import Device, _native
from softwarerenderer_amd.rasterizer import (BlendMode, CullMode, DepthTest, FrustumCuller, MainWindow, Mesh, Program, Rasterizer,
                                              ShaderProgram)
from util import assert_frame_parity

pytestmark = pytest.mark.gpu

MODES = [("libswr_hip_fma.so", "fma"), ("libswr_hip_dotpw.so", "dotpw"), ("libswr_hip_fma_dotpw.so", "fma_dotpw"),
         ("libswr_hip_dpps.so", "dpps"), ("libswr_hip_fma_dpps.so", "fma_dpps")]
CLEAR = (0.125, 0.25, 0.5, 1.0)


@pytest.fixture(scope="module", params=MODES, ids=[m[1] for m in MODES])
def mode(request):
    lib, variant = request.param
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it (make -C softwarerenderer_amd/csrc variants)")
    olib = ob.load(variant=variant)
    dev = Device(0, lib=lib)
    assert dev.numerics_mode() == (olib.oswr_numerics_fma(), olib.oswr_dot_pairwise())
    yield dev, olib, variant
    dev.close()


def gpu_sphere(dev, vertices):
    n = vertices.shape[0]
    mesh = Mesh(dev, vertices, np.zeros(3 if n else 0, dtype=np.uint16))
    try:
        return FrustumCuller.CalculateBoundingSphere(mesh)
    finally:
        mesh.Dispose()


def check_spheres(dev, olib, families, what):
    bad = []
    for f in families:
        for c in K.SPHERE_FAMILIES[f]():
            got, want = gpu_sphere(dev, c.vertices), K.oracle_sphere(olib, c.vertices)
            if not K.same_words(got, want):
                bad.append(f"{c.name}: got {K.words(got)} want {K.words(want)}")
    assert not bad, f"{what}: {len(bad)} spheres differ from the oracle:\n" + "\n".join(bad)


@pytest.mark.parametrize("family", list(K.SPHERE_FAMILIES))
def test_spheres_on_the_product_build(device, oracle_lib, family):
    check_spheres(device, oracle_lib, [family], "product")


def test_spheres_on_a_sensitivity_build_match_the_oracle_built_alike(mode):
    dev, olib, variant = mode
    check_spheres(dev, olib, K.VARIANT_FAMILIES, variant)


def check_thresholds(dev, olib, oracle_flag, what):
    """`dev` has its flags set already; oracle_flag = the Transform flag of the oracle (None = its default)."""
    win = MainWindow(dev, 16, 16)
    bad = []
    for c in K.f1_cases():
        r = K.threshold_radius(olib, c, oracle_flag)
        assert r is not None, c.name
        for k in K.ULP_OFFSETS:
            s = c.sphere(K.ulp_step(r, k))
            with K.oracle_flags(olib, oracle_flag):
                want = K.oracle_inside(olib, s, c.model, c.view, c.proj)
            assert want == (k >= 0), (c.name, k)                   # (the host test's condition, once more where it is used)
            got = FrustumCuller.IsSphereInFrustum(win, s, c.model, c.view, c.proj)
            if got != want:
                bad.append(f"{c.name}: r* {r!r} {k:+d} ULP: got {got}, want {want}")
    assert not bad, f"{what}: {len(bad)} decisions differ from the oracle:\n" + "\n".join(bad)


def check_degenerate(dev, olib, oracle_flag, what):
    win = MainWindow(dev, 16, 16)
    for c in K.f3_degenerate():
        with K.oracle_flags(olib, oracle_flag):
            want = K.oracle_inside(olib, c.sphere, c.model, c.view, c.proj)
        assert FrustumCuller.IsSphereInFrustum(win, c.sphere, c.model, c.view, c.proj) == want, (what, c.name, want)


@pytest.mark.parametrize("flags", [(0, 0), (1, 1), (1, 0)], ids=["t0n0", "t1n1", "t1n0"])
def test_threshold_decisions_on_the_product_build(device, oracle_lib, flags):
    """The culler reads the Transform flag alone (Vector3.Transform, Matrix4x4.Multiply): (1, 0) decides as (1, 1)."""
    default = device.transform_fma()
    try:
        device.set_transform_fma(*flags)
        check_thresholds(device, oracle_lib, flags[0], f"product, flags {flags}")
        check_degenerate(device, oracle_lib, flags[0], f"product, flags {flags}")
    finally:
        device.set_transform_fma(*default)


def test_threshold_decisions_on_a_sensitivity_build(mode):
    dev, olib, variant = mode
    assert dev.transform_fma() == (bool(olib.oswr_numerics_fma()),) * 2
    check_thresholds(dev, olib, None, variant)
    check_degenerate(dev, olib, None, variant)


# ------------------------------------------------------------------------------------------------ batch
def _render_batch(dev, meshes, draws):
    """draws = [(mesh index, model, cull request, flags or None)]: one batch, flushed by the read-back.  Returns colour, depth, stats."""
    Rasterizer.NearClip, Rasterizer.FarClip = 0.1, 1000.0
    win = MainWindow(dev, K.BATCH_SIZE, K.BATCH_SIZE)
    prog = ShaderProgram(Program.Gouraud)
    retained = [Mesh(dev, v, i) for v, i in meshes]
    try:
        dev.reset_stats()
        win.ClearDepthBuffer(); win.ClearColorBuffer(CLEAR)
        for mesh, model, request, flags in draws:
            if flags is not None:
                dev.set_transform_fma(*flags)
            Rasterizer.RenderMesh(win, retained[mesh], None, model, K.BATCH_VIEW, K.BATCH_PROJ, prog.VertexShader, prog.FragmentShader,
                                  CullMode.None_, DepthTest.LessEqual, BlendMode.Alpha, frustumCull=request)
        c, d = win._read()
        st = dev.stats()
        assert st["flushes"] == 1                                    # the draws went as ONE batch
        return c, d, st
    finally:
        for m in retained:
            m.Dispose()


def _oracle_batch(meshes, kept):
    """The frame and counters of the kept draws [(mesh index, model, flag)] on the oracle."""
    o = ob.OracleRenderer(K.BATCH_SIZE, K.BATCH_SIZE)
    o.set_state(0.1, 1000.0, 0)
    o.clear_depth(); o.clear_color(CLEAR)
    for mesh, model, flag in kept:
        o.transform_fma = (bool(flag), bool(flag))
        v, i = meshes[mesh]
        assert o.render_mesh(v, i, model, K.BATCH_VIEW, K.BATCH_PROJ, int(Program.Gouraud), None, None,
                             int(CullMode.None_), int(DepthTest.LessEqual), int(BlendMode.Alpha)) == 0
    c, d, st = o.color.copy(), o.depth.copy(), o.stats()
    o.close()
    default = int(o.lib.oswr_numerics_fma())
    o.lib.oswr_set_transform_fma(default, default)                   # (global per library instance)
    return c, d, st


@pytest.mark.parametrize("pipelining", [0, 1])
@pytest.mark.parametrize("complement", [False, True], ids=["pattern", "complement"])
def test_batch_of_130_draws_at_threshold_translations(device, oracle_lib, complement, pipelining):
    meshes = K.batch_meshes()
    pattern = K.batch_pattern(oracle_lib, complement)
    spheres = [K.oracle_sphere(oracle_lib, v) for v, _ in meshes]
    kept = []
    for d in pattern:
        inside = K.oracle_inside(oracle_lib, spheres[d.mesh], d.model, K.BATCH_VIEW, K.BATCH_PROJ)
        assert inside == (d.step < 0)
        d.keep = inside or not d.cull_request
        if d.keep:
            kept.append((d.mesh, d.model, 0))
    assert 0 < len(kept) < len(pattern)
    rc, rd, rst = _oracle_batch(meshes, kept)
    want_in = sum(d.mesh + 1 for d in pattern if d.keep)
    assert rst["triangles_in"] == want_in
    was = device.pipelining()
    try:
        device.set_pipelining(pipelining)
        c, dz, st = _render_batch(device, meshes, [(d.mesh, d.model, d.cull_request, None) for d in pattern])
    finally:
        device.set_pipelining(was)
    print(f"batch: {len(kept)} of {len(pattern)} draws kept, triangles_in {st['triangles_in']} (want {want_in}), "
          f"triangles_setup {st['triangles_setup']} (want {rst['triangles_setup']})")
    assert st["triangles_in"] == want_in
    assert st["triangles_setup"] == rst["triangles_setup"]
    assert_frame_parity(c, dz, rc, rd, 1, "batch at threshold translations")


def test_every_draw_is_decided_under_the_flags_it_was_recorded_with(device, oracle_lib):
    """Twin meshes: the vertices (so the sphere, so the threshold) of a batch mesh, with 2^j triangles for draw j -- triangles_in then
    spells out which draws were kept.  Each case is recorded under (0,0) and under (1,1) at the smaller of its two thresholds: culled
    under one flag, kept under the other."""
    cases = K.flag_sensitive_batch_draws()
    assert len(cases) >= 2
    base_meshes = K.batch_meshes()
    meshes, draws, kept, want_in, alt = [], [], [], 0, {0: 0, 1: 0}
    for j, (mesh, base, t0, t1) in enumerate(cases):
        model = K.with_translation(base, min(t0, t1))
        sphere = K.oracle_sphere(oracle_lib, base_meshes[mesh][0])
        for flag in ((0, 1) if j % 2 == 0 else (1, 0)):              # the switch goes both ways between neighbours
            weight = 1 << len(meshes)
            meshes.append((base_meshes[mesh][0], np.tile(np.arange(3, dtype=np.uint16), weight)))
            draws.append((len(meshes) - 1, model, True, (flag, flag)))
            with K.oracle_flags(oracle_lib, flag):
                inside = K.oracle_inside(oracle_lib, sphere, model, K.BATCH_VIEW, K.BATCH_PROJ)
            assert inside == (min(t0, t1) < (t0, t1)[flag])
            if inside:
                kept.append((len(meshes) - 1, model, flag))
                want_in += weight
            for f in (0, 1):                                          # what one flag for the whole batch would give
                alt[f] += weight * (min(t0, t1) < (t0, t1)[f])
    assert len(kept) == len(cases) and want_in not in alt.values()
    rc, rd, rst = _oracle_batch(meshes, kept)
    assert rst["triangles_in"] == want_in
    default = device.transform_fma()
    try:
        c, dz, st = _render_batch(device, meshes, draws)
    finally:
        device.set_transform_fma(*default)
    assert st["triangles_in"] == want_in, (bin(st["triangles_in"]), bin(want_in))
    assert st["triangles_setup"] == rst["triangles_setup"]
    assert_frame_parity(c, dz, rc, rd, 1, "flags captured per draw")
