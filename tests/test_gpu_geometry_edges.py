"""The geometry edge families of tests/geometry_edge_scenes.py on the GPU: k_vertex, both copies of k_setup and band_rejects at
the branches of the near clipper, the fan and DrawTriangle's discards.

Every scene goes through run_both: depth words exact, colour <= 1 ULP, the six counters equal to the oracle's.  G1-G5 then again
  - in DebugMode.Wireframe against the oracle's (six slots per clipped triangle, the truncating line bbox);
  - on libswr_hip_test.so, word for word with the product, and on libswr_hip_fma.so against the oracle built alike (a fused lerp
    moves exactly the zero-w and tie cases);
  - through the k_setup that is compiled at run time for a program with a vertex half (RENDERER_VS restates the built-in vertex
    stage, so the frame must be the built-in path's bit for bit), with a data4 program for the lerp of data4.w;
  - G3 and G5 in 2 and 3 bands and in stripes (want[] of odd slots under a band clamp): the union is the single frame.
G7 holds band_rejects to its margin: per band, triangles_in is exactly what the restated decision keeps.

tests/test_geometry_edges_host.py shows on the CPU that the scenes reach every branch, and ties the oracle's clipper to an
independent float32 restatement word for word, with the table of oracle-side mutants (all caught there but one that needs
pixels).

Device mutants: one-change builds of libswr_hip.so from a scratch copy of csrc/ (selected with SWR_LIB; the run-time k_setup is
compiled from the same mutated header), each run once through this file and, where listed, through the GPU suite as it was
before this file (330 tests).  family[..] = test_family_matches_the_oracle, wire[..] = test_family_in_wireframe_matches_the_oracle,
runtime = test_the_run_time_k_setup_equals_the_builtin_one, bands = test_bands_and_stripes_union_is_the_single_frame, g7 =
test_g7_band_rejection_holds_its_margin.  test_test_build_equals_the_product_word_for_word also fails under every mutant of the
shared clipper code, but only because libswr_hip_test.so was left unmutated: it is not counted.  In the right column
test_build_identity_matches_the_verified_pair (which any rebuilt library fails) is left out; "-" = not run.
  mutant                                         this file fails in                               earlier GPU suite
  `>=` -> `>` in the inside test                 family[g1], wire[g1]                             all pass
  the same in the run-time copy alone            runtime                                          -
  threshold 1e-6 -> 1e-5                         family[g2], wire[g2]                             -
  fallback 0.5 -> 0                              family[g2, g5], wire[g2, g5]                     -
  clamp removed                                  family[g1, g4], wire[g1, g4]                     all pass
  `w <= 0` -> `w < 0`                            family[g5], wire[g5]                             -
  fan (0,2,3) -> (0,1,3)                         family[g1..g6], wire[g1..g5]                     -
  second fan triangle's vertices swapped         family[g1..g6], wire[g1..g5]                     -
  `n >= 3` -> `n > 3`                            family[g1..g4, g6], wire[g1..g4]                 -
  triangles_clipped only when n >= 3             family[g2, g3, g6], wire[g2, g3]                 -
  INTERP from v0 instead of outputs[0]           family[g3, g6], wire[g3]                         11 fail (near_clip[FlatColor], 8 random scenes, kat, depth hashes)
  `r.interp = a.interp` in svert_lerp            family[g3, g6], wire[g3]                         11 fail (the same kinds)
  d4w lerp dropped in the run-time k_setup       runtime                                          test_data4_is_lerped_by_the_clipper_...
  odd slot's record index less one               family[g1..g6], runtime, bands[g3, g5]           82 fail
  band_rejects margin 2 -> -3                    g7[2], g7[3]                                     all pass
So the inside test, the clamp and the band margin (and, on the CPU, the threshold and the fallback: tests/test_geometry_edges_host.py)
were held by nothing before; the fan, the counters, INTERP and the record index were already pinned by the random near-clip scenes.
"""
import os

import numpy as np
import pytest

import geometry_edge_scenes as G
from softwarerenderer_amd import Device, _native, multigpu, scenes
from softwarerenderer_amd.rasterizer import DebugMode, MainWindow, Program, Rasterizer
from test_gpu_custom_program import DUST2, VARYINGS, VERTEX_COLOUR, assert_identical, render, with_programs
from test_gpu_parity import run_both
from util import assert_frame_parity
from vertex_program_texts import DATA4_VS, DATA4_XYW_FS, DATA4_XYZ_FS, RENDERER_VS, WORLD_NORMAL_FS

pytestmark = pytest.mark.gpu

COUNTERS = ("triangles_in", "triangles_setup", "triangles_clipped", "fragments_tested", "fragments_shaded", "fragments_written")
RESTATED = {f: G.FAMILIES[f](0) for f in G.RESTATED}
ALL_RESTATED = [s for f in G.RESTATED for s in RESTATED[f]]


def assert_same_words(a, b, what):
    """No tolerance: depth and colour words (NaN against NaN counts as equal: the payload is the hardware's choice)."""
    (ca, da, _), (cb, db, _) = a, b
    bad = da.view(np.uint32) != db.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} depth words differ, first at (y, x) = {tuple(np.argwhere(bad)[0])}"
    bad = (ca.view(np.uint32) != cb.view(np.uint32)) & ~(np.isnan(ca) & np.isnan(cb))
    assert not bad.any(), f"{what}: {int(bad.sum())} colour words differ, first at (y, x, channel) = {tuple(np.argwhere(bad)[0])}"


def _variant_device(lib):
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it (make -C softwarerenderer_amd/csrc variants)")
    return Device(0, lib=lib)


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_family_matches_the_oracle(device, family):
    """Depth words exact, colour <= 1 ULP, six counters equal; every scene draws."""
    for scene in (RESTATED[family] if family in RESTATED else G.FAMILIES[family](0)):
        _, st = run_both(device, scene)
        assert st["fragments_written"] > 0, f"{scene.name}: nothing was drawn"
        if family in RESTATED:
            assert st["triangles_clipped"] > 0, scene.name


@pytest.mark.parametrize("family", G.RESTATED)
def test_family_in_wireframe_matches_the_oracle(device, family):
    """Three DrawLine records per fan triangle, six slots per clipped triangle.  (DebugVaryings is refused in wireframe --
    tests/test_gpu_parity.py::test_debug_varyings_in_wireframe_is_refused_not_wrong -- so that one G3 scene is drawn as Gouraud.)"""
    from oracle.binding import OracleRenderer
    for scene in RESTATED[family]:
        if scene.draws[0].program == Program.DebugVaryings:
            scene = with_programs(scene, [Program.Gouraud])
        o = OracleRenderer(scene.width, scene.height)
        rc, rd = o.render_scene(scene, debug_mode=1)
        rst = o.stats(); o.close()
        Rasterizer.RenderDebugMode = DebugMode.Wireframe
        try:
            c, d, st = render(device, scene)
        finally:
            Rasterizer.RenderDebugMode = DebugMode.None_
        assert_frame_parity(c, d, rc, rd, 1, "wireframe " + scene.name)
        for k in COUNTERS:
            assert st[k] == rst[k], (scene.name, k, st[k], rst[k])
        assert st["fragments_written"] > 0 and st["triangles_clipped"] > 0, scene.name


def test_test_build_equals_the_product_word_for_word(device):
    dev = _variant_device("libswr_hip_test.so")
    try:
        for scene in ALL_RESTATED:
            a, b = render(device, scene), render(dev, scene)
            assert_same_words(a, b, f"{scene.name}: product against test build")
            for k in COUNTERS:
                assert a[2][k] == b[2][k], (scene.name, k)
    finally:
        dev.close()


def test_fused_lerp_build_matches_the_oracle_built_alike():
    from oracle import binding as ob
    ob.load(variant="fma")
    dev = _variant_device("libswr_hip_fma.so")
    try:
        assert dev.numerics_mode()[0] == 1
        for scene in ALL_RESTATED:
            c, d, st = render(dev, scene)
            o = ob.OracleRenderer(scene.width, scene.height, variant="fma")
            rc, rd = o.render_scene(scene)
            ost = o.stats(); o.close()
            assert_frame_parity(c, d, rc, rd, color_ulp=1, what=f"fma/{scene.name}")
            for k in COUNTERS:
                assert st[k] == ost[k], (scene.name, k, st[k], ost[k])
    finally:
        dev.close()


def _builtin_twin(program):
    """(fragment text, built-in program) pairs of tests/test_gpu_custom_program.py: the text restates the built-in.  User programs
    always interpolate (FlatColor's INTERP = 0 has no user counterpart), so FlatColor scenes are compared as Gouraud ones; the Phong
    scene is compared as Dust2LambertFog (the world-normal lerp)."""
    if program == Program.DebugVaryings:
        return VARYINGS, Program.DebugVaryings
    if program == Program.Phong4Point:
        return DUST2, Program.Dust2LambertFog
    return VERTEX_COLOUR, Program.Gouraud


def test_the_run_time_k_setup_equals_the_builtin_one(device):
    """RENDERER_VS + a restated fragment text: the module's own k_vertex_user / k_setup (SWR_USER_VERTEX) against the built-in
    kernels, bit for bit, stats included.  Both copies come from one header, so this test sees only what differs between them
    (test_family_matches_the_oracle holds the shared code to the oracle).  What each text reads of the clipper's lerps: VERTEX_COLOUR
    the colour, VARYINGS the Normal, DUST2 the world normal, the uv (white texture: no effect) and clip.z -- NOT the world position,
    which a user program does not have: its slots carry data4.xyz.  So the wpos lerp and the d4w lerp of the module are read through
    data4: DATA4_VS hands the world normal over in data4 (z once more in .w, lerped on its own in the module's clipper), and
    DATA4_XYZ_FS (the three wpos slots) and DATA4_XYW_FS (x, y and the d4w lerp) must both equal WORLD_NORMAL_FS over the BUILT-IN
    vertex stage.  The run-time copy never sees INTERP = 0 (user programs always interpolate)."""
    pids = {}
    xyw = device.compile_program(DATA4_XYW_FS, vertex_source=DATA4_VS)
    xyz = device.compile_program(DATA4_XYZ_FS, vertex_source=DATA4_VS)
    wn = device.compile_program(WORLD_NORMAL_FS)
    try:
        for scene in ALL_RESTATED:
            text, builtin = _builtin_twin(scene.draws[0].program)
            if text not in pids:
                pids[text] = device.compile_program(text, vertex_source=RENDERER_VS)
            want = render(device, with_programs(scene, [builtin]))
            got = render(device, with_programs(scene, [pids[text]]))
            assert got[2]["triangles_clipped"] > 0
            assert_identical(got, want, f"run-time k_setup/{scene.name}")
            want = render(device, with_programs(scene, [wn]))
            assert_identical(render(device, with_programs(scene, [xyw])), want, f"data4.xyw/{scene.name}")
            assert_identical(render(device, with_programs(scene, [xyz])), want, f"data4.xyz/{scene.name}")
    finally:
        for p in list(pids.values()) + [xyw, xyz, wn]:
            device.destroy_program(p)


def _banded(device, scene, set_band):
    win = MainWindow(device, scene.width, scene.height)
    set_band(win)
    device.reset_stats()
    r = scenes.SceneRenderer(device, scene, window=win)
    c, d = r.render()
    st = device.stats()
    r.close()
    return c, d, st


@pytest.mark.parametrize("family", ["g3", "g5"])
def test_bands_and_stripes_union_is_the_single_frame(device, family):
    for scene in RESTATED[family]:
        whole = render(device, scene)
        try:
            for world in (2, 3):
                parts = [_banded(device, scene, lambda w, b=band: w.SetBand(*b)) for band in multigpu.band_partition(scene.height, world)]
                c, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
                assert np.array_equal(d.view(np.uint32), whole[1].view(np.uint32)), f"{scene.name}: {world} bands, depth"
                assert np.array_equal(c.view(np.uint32), whole[0].view(np.uint32)), f"{scene.name}: {world} bands, colour"
                assert sum(p[2]["fragments_written"] for p in parts) == whole[2]["fragments_written"]
            world, k = 2, 1
            parts = [_banded(device, scene, lambda w, r=rank: w.SetBandInterleaved(r, world, k)) for rank in range(world)]
            c = multigpu.assemble_stripes([p[0] for p in parts], scene.height, world, k)
            d = multigpu.assemble_stripes([p[1] for p in parts], scene.height, world, k)
            assert np.array_equal(d.view(np.uint32), whole[1].view(np.uint32)), f"{scene.name}: stripes, depth"
            assert np.array_equal(c.view(np.uint32), whole[0].view(np.uint32)), f"{scene.name}: stripes, colour"
            assert sum(p[2]["fragments_written"] for p in parts) == whole[2]["fragments_written"]
        finally:
            MainWindow(device, scene.width, scene.height).SetBand(-1, -1)


def _kept_triangles(scene, band):
    """triangles_in of a band by band_rejects' rule, guards included, restated in double (G.band_keeps): the scene's boxes end a whole
    pixel from either threshold, so double against double decides alike."""
    y0, rows = multigpu.band_pixel_rows(scene.height, band)
    return sum(d.indices.size // 3 for d in scene.draws if G.band_keeps(d, scene.height, y0, y0 + rows))


@pytest.mark.parametrize("world", [2, 3])
def test_g7_band_rejection_holds_its_margin(device, world):
    scene, borders = G.g7_band_margin()
    run_both(device, scene)
    whole = render(device, scene)
    total = scene.n_triangles
    try:
        bands = multigpu.band_partition(scene.height, world)
        assert {b[0] * 16 for b in bands if b[0] > 0} <= set(borders)
        parts = [_banded(device, scene, lambda w, b=band: w.SetBand(*b)) for band in bands]
    finally:
        MainWindow(device, scene.width, scene.height).SetBand(-1, -1)
    c, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert np.array_equal(d.view(np.uint32), whole[1].view(np.uint32)), f"{world} bands, depth"
    assert np.array_equal(c.view(np.uint32), whole[0].view(np.uint32)), f"{world} bands, colour"
    tin = [p[2]["triangles_in"] for p in parts]
    print(f"g7: {world} bands, triangles_in per rank {tin} of {total}")
    assert all(0 < t < total for t in tin), tin                        # every rank rejects some meshes and keeps some
    assert tin == [_kept_triangles(scene, b) for b in bands]
    # fragments on the border rows, from meshes on either side
    for b in bands[1:]:
        y = b[0] * 16
        assert (whole[1][y - 1] != whole[1][0, 0]).any() and (whole[1][y] != whole[1][0, 0]).any(), y
