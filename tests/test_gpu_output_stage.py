"""The filled path's output stage -- depth function, `W > 0` gate, blend, conditional Z write and the BlendMode.None row early-out of
k_raster_c -- on the families O1-O6 of tests/output_stage_scenes.py, against the oracle at the project's bar: depth words bit-exact,
colour within 1 ULP, the six counters equal; the product build and the fenced test build word for word the same.  That every family
reaches what it is for (which lane of which chunk a failing fragment lands on, which word a vertex sample stores), and that the
restatement is the oracle's frame, is asserted on the CPU in tests/test_output_stage_host.py.  What each test caught when the kernel
was changed on purpose: profiles/r12_output_stage_tests.md.

  test_scene                    every scene, both builds
  test_kernel_variants          O7: every O1 / O2 scene diluted into generic_none and generic_phong, word for word the pure frame
  test_user_program             O7: O3 and O4 through a user fragment program (user_none), bit for bit the built-in Gouraud frame
  test_numerics_builds          O1 and O2 on the five System.Numerics sensitivity builds against the oracle built alike; FlatColor
                                scenes (no Lerp, no dot3): the default build's words
  test_in_bands                 the O3 two-tile scene and the O5 stacks in 2 tile-row bands
  test_flush_modes              O3 and O5 with synchronous flushes and with frames in flight, two frames each, both equal"""
import functools
import os
import time

import numpy as np
import pytest

import output_stage_scenes as O
import shade_edge_scenes as S
from oracle import binding as ob
from softwarerenderer_amd import Device, MainWindow, _native, multigpu, scenes
from softwarerenderer_amd.rasterizer import BlendMode, Program
from test_gpu_custom_program import VERTEX_COLOUR, with_programs
from test_gpu_parity import COLOR_ULP
from util import assert_frame_parity

pytestmark = pytest.mark.gpu

T0 = time.time()
COUNTERS = ("triangles_in", "triangles_setup", "triangles_clipped", "fragments_tested", "fragments_shaded", "fragments_written")
FRAGMENTS = ("fragments_tested", "fragments_shaded", "fragments_written")
TEST_LIB = "libswr_hip_test.so"
MODES = [("libswr_hip_fma.so", "fma"), ("libswr_hip_dotpw.so", "dotpw"), ("libswr_hip_fma_dotpw.so", "fma_dotpw"),
         ("libswr_hip_dpps.so", "dpps"), ("libswr_hip_fma_dpps.so", "fma_dpps")]
SCENES = O.all_scenes()
VARIANTS = tuple(s.name for f in ("o1", "o2") for s in O.family(f))                     # O7's dilutions; the numerics builds
USER = tuple(s.name for f in ("o3", "o4") for s in O.family(f))
FLAT = tuple(n for n in VARIANTS if all(d.program == Program.FlatColor for d in SCENES[n].draws))
IN_BANDS = tuple(s.name for f in ("o3", "o5") for s in O.family(f) if s.height == 32)
FLUSHED = {f: tuple(s.name for s in O.family(f)) for f in ("o3", "o5")}


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


@pytest.fixture(scope="module")
def vertex_colour(device):
    pid = device.compile_program(VERTEX_COLOUR)
    yield pid
    device.destroy_program(pid)


@functools.lru_cache(maxsize=None)
def _want(name, variant=None):
    """The oracle's colour, depth and stats: computed once, shared, never changed."""
    scene = SCENES[name]
    o = ob.OracleRenderer(scene.width, scene.height, variant=variant)
    c, d = o.render_scene(scene)
    st = o.stats()
    o.close()
    return c, d, st


def _render(dev, scene, window=None, frames=1, every=False):
    """Colour, depth and stats of the LAST of `frames` identical frames (every=True: of each)."""
    r = scenes.SceneRenderer(dev, scene, window=window)
    out = []
    try:
        for _ in range(frames):
            dev.reset_stats()
            r.submit_frame()
            c, d = r.window._read(True, True)
            st = dev.stats()
            assert st["flushes"] == 1, f"{scene.name}: {len(scene.draws)} draws went as {st['flushes']} batches"
            out.append((c, d, st))
    finally:
        r.close()
    return out if every else out[-1]


_DEFAULT = {}


def _default_frame(device, name):
    """The product build's frame of a scene: rendered once, shared, never changed."""
    if name not in _DEFAULT:
        _DEFAULT[name] = _render(device, SCENES[name])
    return _DEFAULT[name]


def _check(what, got, want, counters=COUNTERS):
    c, d, st = got
    rc, rd, rst = want
    for k in counters:
        print(f"{what}: {k} gpu={st[k]} oracle={rst.get(k)}")
    assert_frame_parity(c, d, rc, rd, COLOR_ULP, what)
    for k in counters:
        assert st[k] == rst[k], f"{what}: stats[{k}] gpu={st[k]} oracle={rst[k]}"


def _same_words(a, b, what, counters=COUNTERS):
    (ca, da, sa), (cb, db, sb) = a, b
    bad = da.view(np.uint32) != db.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} depth words differ, first at (y, x) = {tuple(np.argwhere(bad)[0])}"
    bad = (ca.view(np.uint32) != cb.view(np.uint32)) & ~(np.isnan(ca) & np.isnan(cb))      # (a NaN's payload is the hardware's choice)
    assert not bad.any(), f"{what}: {int(bad.sum())} colour words differ, first at (y, x, channel) = {tuple(np.argwhere(bad)[0])}"
    for k in counters:
        assert sa[k] == sb[k], (what, k, sa[k], sb[k])


# ------------------------------------------------------------------------------------------------ 1: every scene, both builds
@pytest.mark.parametrize("name", list(SCENES))
def test_scene(device, testlib_device, name):
    scene, want = SCENES[name], _want(name)
    got = _default_frame(device, name)
    _check(name, got, want)
    test = _render(testlib_device, scene)
    _check(f"{name} on the test build", test, want)
    _same_words(got, test, f"{name}: product against test build")


# ------------------------------------------------------------------------------------------------ 2: O7, the other kernels
@pytest.mark.parametrize("name", VARIANTS)
def test_kernel_variants(device, name):
    scene = SCENES[name]
    pure = _default_frame(device, name)
    assert S.predicted_kernel(scene) == O.expected_kernel(scene)
    for dil, with_phong in (("none", False), ("phong", True)):
        d = O.diluted(scene, with_phong)
        assert S.predicted_kernel(d) == O.expected_kernel(scene, dil), d.name
        got = _render(device, d)
        # (the off-screen triangle is set up nowhere and covers nothing)
        _same_words(pure, got, f"{name}: {S.predicted_kernel(scene)} against {S.predicted_kernel(d)}", counters=FRAGMENTS + ("triangles_setup",))


@pytest.mark.parametrize("name", USER)
def test_user_program(device, vertex_colour, name):
    scene = SCENES[name]
    user = with_programs(scene, [vertex_colour])
    # select_raster_kernel (csrc/swr_raster_select.h): a program id >= SWR_PROG_USER_BASE sets `user`, a BlendMode.None draw sets `none`
    assert all(d.program >= _native.SWR_PROG_USER_BASE for d in user.draws) and any(d.blend == BlendMode.None_ for d in user.draws), "user_none"
    _same_words(_render(device, user), _default_frame(device, name), f"{name}: user program (user_none) against built-in Gouraud")


# ------------------------------------------------------------------------------------------------ 3: the numerics builds
@pytest.mark.parametrize("name", VARIANTS)
def test_numerics_builds(device, mode, name):
    dev, variant = mode
    got = _render(dev, SCENES[name])
    _check(f"{variant}/{name}", got, _want(name, variant))
    if name in FLAT:
        _same_words(got, _default_frame(device, name), f"{variant}/{name}: FlatColor has no Lerp and no dot3, yet the words differ")


# ------------------------------------------------------------------------------------------------ 4: bands
@pytest.mark.parametrize("name", IN_BANDS)
def test_in_bands(device, name):
    scene = SCENES[name]
    rc, rd, rst = _want(name)
    bands = multigpu.band_partition(scene.height, 2)
    assert all(b[1] > 0 for b in bands) and sum(b[1] for b in bands) * 16 == scene.height, "the union is the whole frame"
    cols, deps, tot = [], [], dict.fromkeys(FRAGMENTS, 0)
    try:
        for b in bands:
            win = MainWindow(device, scene.width, scene.height)
            win.SetBand(*b)
            c, d, st = _render(device, scene, window=win, frames=2)
            cols.append(c); deps.append(d)
            for k in tot:
                tot[k] += st[k]
    finally:
        MainWindow(device, scene.width, scene.height).SetBand(-1, -1)
    assert_frame_parity(np.concatenate(cols), np.concatenate(deps), rc, rd, COLOR_ULP, f"{name} in 2 bands")
    for k in FRAGMENTS:
        assert tot[k] == rst[k], f"{name} in 2 bands: summed {k} gpu={tot[k]} oracle={rst[k]}"


# ------------------------------------------------------------------------------------------------ 5: flush modes, two frames
@pytest.mark.parametrize("flush", ["synchronous", "in_flight"])
@pytest.mark.parametrize("fam", list(FLUSHED))
def test_flush_modes(device, monkeypatch, fam, flush):
    if flush == "synchronous":
        monkeypatch.setenv("SWR_SYNC_FLUSH", "1")           # read when the context is created
        dev = Device(0)
        monkeypatch.delenv("SWR_SYNC_FLUSH")
    else:
        dev = device
        assert dev.pipelining() == 1, "the default: the front end of a flush beside the raster kernel of the one before"
    try:
        for name in FLUSHED[fam]:
            want = _want(name)
            first, second = _render(dev, SCENES[name], frames=2, every=True)
            _check(f"{name} {flush} first frame", first, want)
            _check(f"{name} {flush} second frame", second, want)
            _same_words(first, second, f"{name} {flush}: first against second frame")
    finally:
        if dev is not device:
            dev.close()


# ------------------------------------------------------------------------------------------------ 6
def test_report_wall_time():
    print(f"tests/test_gpu_output_stage.py: {time.time() - T0:.1f} s from import to here ({len(SCENES)} scenes)")
