"""DebugMode.Wireframe at DrawLine's boundaries -- the families W1-W9 of tests/wireframe_edge_scenes.py -- against the oracle, at the
project's bar: depth words bit-exact, colour within 1 ULP, the six counters equal; the product build and the fenced test build
word for word the same; tile_pairs equal to the bbox tiles the restatement (and, for W8 and W9, front_end_scenes.plan) counts.
That every family reaches what it is for, and that the restatement is the oracle's frame, is asserted on the CPU in
tests/test_wireframe_edges_host.py.  What each test caught when the kernels were changed on purpose: profiles/r11_wireframe_tests.md.

  test_scene                    every scene, both builds
  test_numerics_builds          W1 and W5 on the five System.Numerics sensitivity builds against the oracle built alike: line_test uses
                                no dot3 and no Lerp, so the lit pixels are the default build's
  test_in_parts                 W9 and W7 (four tiles) in 2 and 3 tile-row bands and in (3, 2) interleaved stripes
  test_flush_modes              W7 and W8 with synchronous flushes and with frames in flight, two frames each, both equal
  test_mode_switch_in_a_frame   filled, wireframe, filled without a clear between: a flush per change of mode"""
import functools
import os
import time

import numpy as np
import pytest

import front_end_scenes as F
import wireframe_edge_scenes as Wf
from oracle import binding as ob
from softwarerenderer_amd import Device, MainWindow, _native, multigpu, scenes
from softwarerenderer_amd.rasterizer import BlendMode, DebugMode, DepthTest, Mesh, Rasterizer, ShaderProgram
from test_gpu_parity import COLOR_ULP
from util import assert_frame_parity

pytestmark = pytest.mark.gpu

T0 = time.time()
COUNTERS = ("triangles_in", "triangles_setup", "triangles_clipped", "fragments_tested", "fragments_shaded", "fragments_written")
FRAGMENTS = ("fragments_tested", "fragments_shaded", "fragments_written")
TEST_LIB = "libswr_hip_test.so"
MODES = [("libswr_hip_fma.so", "fma"), ("libswr_hip_dotpw.so", "dotpw"), ("libswr_hip_fma_dotpw.so", "fma_dotpw"),
         ("libswr_hip_dpps.so", "dpps"), ("libswr_hip_fma_dpps.so", "fma_dpps")]
SCENES = Wf.all_scenes()
PLANNED = tuple(s.name for f in ("w8", "w9") for s in Wf.family(f))
# W9 (16 tile rows) and the W7 scenes with more than one tile row: the four-tile ones (six rows) and the clipped quads (four rows).
# W7's one-tile scenes are 16 x 16, a single tile row: there is nothing to cut.
IN_PARTS = tuple(s.name for s in Wf.family("w9")) + tuple(s.name for s in Wf.family("w7") if "one_tile" not in s.name)
NUMERICS = tuple(s.name for f in ("w1", "w5") for s in Wf.family(f))
FLUSHED = tuple(s.name for f in ("w7", "w8") for s in Wf.family(f))


def _need(lib):
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it (make -C softwarerenderer_amd/csrc variants)")


@pytest.fixture(scope="module")
def testlib_device():
    _need(TEST_LIB)
    dev = Device(0, lib=TEST_LIB)
    yield dev
    dev.close()


@pytest.fixture(scope="module", params=MODES, ids=[m[1] for m in MODES])
def mode(request):
    lib, variant = request.param
    _need(lib)
    olib = ob.load(variant=variant)
    dev = Device(0, lib=lib)
    assert dev.numerics_mode() == (olib.oswr_numerics_fma(), olib.oswr_dot_pairwise())
    yield dev, variant
    dev.close()


@functools.lru_cache(maxsize=None)
def _want(name, variant=None):
    """The oracle's wireframe colour, depth and stats: computed once, shared, never changed."""
    scene = SCENES[name]
    o = ob.OracleRenderer(scene.width, scene.height, variant=variant)
    c, d = o.render_scene(scene, debug_mode=1)
    st = o.stats()
    o.close()
    return c, d, st


@functools.lru_cache(maxsize=None)
def _restated(name):
    return Wf.restate(SCENES[name])


def _render(dev, scene, window=None, frames=1, every=False):
    """Colour, depth and stats of the LAST of `frames` identical wireframe frames (every=True: of each)."""
    r = scenes.SceneRenderer(dev, scene, window=window)
    out = []
    Rasterizer.RenderDebugMode = DebugMode.Wireframe
    try:
        for _ in range(frames):
            dev.reset_stats()
            r.submit_frame()
            c, d = r.window._read(True, True)
            st = dev.stats()
            assert st["flushes"] == 1, f"{scene.name}: {len(scene.draws)} draws went as {st['flushes']} batches"
            out.append((c, d, st))
    finally:
        Rasterizer.RenderDebugMode = DebugMode.None_
        r.close()
    return out if every else out[-1]


def _check(what, got, want, counters=COUNTERS):
    c, d, st = got
    rc, rd, rst = want
    for k in counters + ("tile_pairs",):
        print(f"{what}: {k} gpu={st[k]} oracle={rst.get(k)}")
    assert_frame_parity(c, d, rc, rd, COLOR_ULP, what)
    for k in counters:
        assert st[k] == rst[k], f"{what}: stats[{k}] gpu={st[k]} oracle={rst[k]}"


def _same_words(a, b, what):
    (ca, da, sa), (cb, db, sb) = a, b
    bad = da.view(np.uint32) != db.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} depth words differ, first at (y, x) = {tuple(np.argwhere(bad)[0])}"
    bad = (ca.view(np.uint32) != cb.view(np.uint32)) & ~(np.isnan(ca) & np.isnan(cb))      # (a NaN's payload is the hardware's choice)
    assert not bad.any(), f"{what}: {int(bad.sum())} colour words differ, first at (y, x, channel) = {tuple(np.argwhere(bad)[0])}"
    for k in COUNTERS + ("tile_pairs",):
        assert sa[k] == sb[k], (what, k, sa[k], sb[k])


def _check_pairs(name, pairs):
    want = _restated(name).tile_pairs
    assert pairs == want, f"{name}: tile_pairs={pairs}, the lines' bboxes hold {want} tiles"
    if name in PLANNED:
        p = F.plan(SCENES[name], wireframe=True)
        assert p.exact and pairs == int(p.lo.sum()), f"{name}: tile_pairs={pairs}, the planner counts {int(p.lo.sum())}"


# ------------------------------------------------------------------------------------------------ 1: every scene, both builds
@pytest.mark.parametrize("name", list(SCENES))
def test_scene(device, testlib_device, name):
    scene, want = SCENES[name], _want(name)
    got = _render(device, scene)
    _check(name, got, want)
    _check_pairs(name, got[2]["tile_pairs"])
    test = _render(testlib_device, scene)
    _check(f"{name} on the test build", test, want)
    _same_words(got, test, f"{name}: product against test build")


# ------------------------------------------------------------------------------------------------ 2: the numerics builds
@pytest.mark.parametrize("name", NUMERICS)
def test_numerics_builds(mode, name):
    dev, variant = mode
    scene = SCENES[name]
    got = _render(dev, scene)
    _check(f"{variant}/{name}", got, _want(name, variant))
    lit, default_lit = got[1] != Wf.FLOAT_MIN, _want(name)[1] != Wf.FLOAT_MIN
    assert np.array_equal(lit, default_lit), f"{variant}/{name}: line_test has no dot3 and no Lerp, yet the lit pixels differ"
    assert np.array_equal(got[1].view(np.uint32), _want(name)[1].view(np.uint32)), f"{variant}/{name}: nor has the depth"


# ------------------------------------------------------------------------------------------------ 3: bands and stripes
def _in_parts(device, scene, windows, assemble):
    cols, deps, tot = [], [], dict.fromkeys(FRAGMENTS + ("tile_pairs",), 0)
    try:
        for setup in windows:
            win = MainWindow(device, scene.width, scene.height)
            setup(win)
            c, d, st = _render(device, scene, window=win, frames=2)
            cols.append(c); deps.append(d)
            for k in tot:
                tot[k] += st[k]
    finally:
        MainWindow(device, scene.width, scene.height).SetBand(-1, -1)
    return assemble(cols), assemble(deps), tot


# (3, 2) stripes need at least five tile rows for every rank to hold one: the clipped quads (four rows) are cut into bands only
PARTS = [(n, p) for n in IN_PARTS for p in ("bands2", "bands3", "stripes3x2") if not (p == "stripes3x2" and SCENES[n].height < 80)]


@pytest.mark.parametrize("name,parts", PARTS, ids=[f"{n}-{p}" for n, p in PARTS])
def test_in_parts(device, name, parts):
    scene = SCENES[name]
    rc, rd, rst = _want(name)
    if parts.startswith("bands"):
        bands = multigpu.band_partition(scene.height, int(parts[-1]))
        assert all(b[1] > 0 for b in bands) and sum(b[1] for b in bands) * 16 == scene.height, "the union is the whole frame"
        c, d, tot = _in_parts(device, scene, [functools.partial(lambda b, w: w.SetBand(*b), b) for b in bands], np.concatenate)
    else:
        rows = multigpu.stripe_rows(scene.height, 3, 2)
        assert all(len(r) for r in rows) and sorted(np.concatenate(rows).tolist()) == list(range(scene.height))
        c, d, tot = _in_parts(device, scene, [functools.partial(lambda r, w: w.SetBandInterleaved(r, 3, 2), r) for r in range(3)],
                              lambda p: multigpu.assemble_stripes(p, scene.height, 3, 2))
    assert_frame_parity(c, d, rc, rd, COLOR_ULP, f"{name} in {parts}")
    for k in FRAGMENTS:
        assert tot[k] == rst[k], f"{name} in {parts}: summed {k} gpu={tot[k]} oracle={rst[k]}"
    _check_pairs(name, tot["tile_pairs"])


# ------------------------------------------------------------------------------------------------ 4: flush modes, two frames
@pytest.mark.parametrize("flush", ["synchronous", "in_flight"])
@pytest.mark.parametrize("name", FLUSHED)
def test_flush_modes(device, monkeypatch, name, flush):
    scene, want = SCENES[name], _want(name)
    if flush == "synchronous":
        monkeypatch.setenv("SWR_SYNC_FLUSH", "1")           # read when the context is created
        dev = Device(0)
        monkeypatch.delenv("SWR_SYNC_FLUSH")
    else:
        dev = device
        assert dev.pipelining() == 1, "the default: the front end of a flush beside the raster kernel of the one before"
    try:
        first, second = _render(dev, scene, frames=2, every=True)
    finally:
        if dev is not device:
            dev.close()
    _check(f"{name} {flush} first frame", first, want)
    _check(f"{name} {flush} second frame", second, want)
    _same_words(first, second, f"{name} {flush}: first against second frame")
    _check_pairs(name, second[2]["tile_pairs"])


# ------------------------------------------------------------------------------------------------ 5: the mode changes inside a frame
def test_mode_switch_in_a_frame(device):
    """Filled, wireframe, filled on one frame without a clear between.  swr_set_state flushes what is recorded when the mode
    changes (a batch is all lines or all triangles), so the frame takes one flush per change plus the last."""
    wire = Wf.family("w9")[0]
    a = scenes.cfg2(256, 256, 150, seed=71, min_area=200.0, max_area=6000.0).draws[0]
    b = wire.draws[0]
    c = scenes.state_scene(256, 256, 120, seed=72, depth_test=DepthTest.LessEqual, blend=BlendMode.Alpha, alpha_range=(0.3, 0.7)).draws[0]
    plan = [(a, DebugMode.None_), (b, DebugMode.Wireframe), (c, DebugMode.None_)]
    changes = sum(m0 != m1 for (_, m0), (_, m1) in zip(plan, plan[1:]))
    assert changes == 2
    o = ob.OracleRenderer(256, 256)
    o.set_state(0.1, 1000.0, 0)
    o.clear_depth(); o.clear_color(Wf.CLEAR)
    for d, m in plan:
        o.set_state(0.1, 1000.0, int(m))
        assert o.render_mesh(d.vertices, d.indices, d.model, d.view, d.projection, int(d.program), d.uniforms, None,
                             int(d.cull), int(d.depth_test), int(d.blend)) == 0
    rc, rd, rst = o.color.copy(), o.depth.copy(), o.stats()
    o.close()
    win = MainWindow(device, 256, 256)
    meshes = [Mesh(device, d.vertices, d.indices) for d, _ in plan]
    try:
        device.reset_stats()
        Rasterizer.NearClip, Rasterizer.FarClip = 0.1, 1000.0
        win.ClearDepthBuffer(); win.ClearColorBuffer(Wf.CLEAR)
        for (d, m), mesh in zip(plan, meshes):
            Rasterizer.RenderDebugMode = m
            prog = ShaderProgram(d.program, d.uniforms, None)
            Rasterizer.RenderMesh(win, mesh, None, d.model, d.view, d.projection, prog.VertexShader, prog.FragmentShader, d.cull, d.depth_test, d.blend)
        col, dep = win._read(True, True)
        st = device.stats()
    finally:
        Rasterizer.RenderDebugMode = DebugMode.None_
        for m in meshes:
            m.Dispose()
    assert_frame_parity(col, dep, rc, rd, COLOR_ULP, "filled, wireframe, filled")
    for k in COUNTERS:
        assert st[k] == rst[k], f"mode switch: stats[{k}] gpu={st[k]} oracle={rst[k]}"
    assert st["flushes"] == changes + 1, f"{st['flushes']} flushes for {changes} changes of mode"
    assert rst["triangles_setup"] > 0 and rst["fragments_written"] > 3000


# ------------------------------------------------------------------------------------------------ 6
def test_report_wall_time():
    print(f"tests/test_gpu_wireframe_edges.py: {time.time() - T0:.1f} s from import to here ({len(SCENES)} scenes)")
