"""The front end where its paths switch -- k_bin's crowded hash table, tpw and the ragged last wave, bin_big's four-at-a-time and
strided paths at 9 / 64 / 65 tiles, k_sort_tiles' four paths mixed inside a wave, the scan's seams at 255 / 256 / 257 tiles,
tile_place_block's 16 x 16 regions -- against the oracle, at the project's bar: depth words bit-exact, colour within 1 ULP, the six
counters equal.  The scenes and the planner are tests/front_end_scenes.py; that each scene reaches its path, and that the counters
of a staircase scene see an inversion, a lost or a duplicated pair ANYWHERE in a list (which the colours do not), is asserted on the
CPU in tests/test_front_end_host.py.  What each test caught when the kernels were broken on purpose: profiles/r10_front_end_tests.md.

Every family is rendered twice and the second frame checked (the optimistic, pipelined flush, with the first frame's fragment counts
in the tile order), then once more on a fresh context with SWR_SYNC_FLUSH=1; tile_pairs must agree between the two and with the
planner -- exactly where the scene consists of certain primitives, within its bounds elsewhere."""
import functools
import os

import numpy as np
import pytest

import front_end_scenes as F
from softwarerenderer_amd import Device, MainWindow, _native, multigpu, scenes
from softwarerenderer_amd.rasterizer import DebugMode, Rasterizer
from util import assert_frame_parity, render_oracle

pytestmark = pytest.mark.gpu

COUNTERS = ("triangles_in", "triangles_setup", "triangles_clipped", "fragments_tested", "fragments_shaded", "fragments_written")
FRAGMENTS = ("fragments_tested", "fragments_shaded", "fragments_written")
TEST_LIB = "libswr_hip_test.so"

FAMILIES = {"sort_ladder": lambda: F.sort_ladder()[0], "crowded_table": F.crowded_table, "big_slots": lambda: F.big_slots()[0]}
FAMILIES.update({f"tpw_{n}": functools.partial(F.tpw_ladder, n) for n in F.TPW_LADDER_T})
FAMILIES.update({f"tiling_{x}x{y}": functools.partial(lambda x, y: F.tiling_ladder(x, y)[0], x, y) for x, y in F.TILING_LADDER})
FAMILIES["tiling_%dx%dpx" % F.TILING_ODD_PIXELS] = lambda: F.tiling_ladder(pixels=F.TILING_ODD_PIXELS)[0]
WIREFRAME = "tpw_8193"              # the member of the tpw ladder that also runs with 6 slots per triangle


@functools.lru_cache(maxsize=None)
def _case(name, wireframe=False):
    """(scene, plan, oracle's colour, depth, stats): computed once, shared, never changed."""
    scene = FAMILIES[name]()
    return scene, F.plan(scene, wireframe=wireframe), render_oracle(scene, debug_mode=1 if wireframe else 0)


def _render(dev, scene, window=None, wireframe=False, frames=2):
    """Colour, depth and stats of the LAST of `frames` identical frames."""
    r = scenes.SceneRenderer(dev, scene, window=window)
    Rasterizer.RenderDebugMode = DebugMode.Wireframe if wireframe else DebugMode.None_
    try:
        for _ in range(frames):
            dev.reset_stats()
            r.submit_frame()
            c, d = r.window._read(True, True)
            st = dev.stats()
            # plan() takes all draws of a scene as ONE batch (T, tpw, the k_bin blocks follow from that): hold the library to it
            assert st["flushes"] == 1, f"{scene.name}: {len(scene.draws)} draws went as {st['flushes']} batches, plan() is for one"
    finally:
        Rasterizer.RenderDebugMode = DebugMode.None_
        r.close()
    return c, d, st


def _check(what, got, want, counters=COUNTERS):
    c, d, st = got
    rc, rd, rst = want
    for k in counters + ("tile_pairs",):
        print(f"{what}: {k} gpu={st[k]} oracle={rst.get(k)}")
    assert_frame_parity(c, d, rc, rd, 1, what)
    for k in counters:
        assert st[k] == rst[k], f"{what}: stats[{k}] gpu={st[k]} oracle={rst[k]}"


def _check_pairs(what, pairs, plan):
    lo, hi = int(plan.lo.sum()), int(plan.hi.sum())
    print(f"{what}: tile_pairs={pairs} planner lo={lo} hi={hi} exact={plan.exact}")
    if plan.exact:
        assert pairs == lo, f"{what}: tile_pairs={pairs}, the planner counts exactly {lo}"
    else:
        assert lo <= pairs <= hi, f"{what}: tile_pairs={pairs} outside the planner's bounds [{lo}, {hi}]"


def _sync_device(monkeypatch, lib=None):
    """SWR_SYNC_FLUSH=1 is read when the context is created: every flush then reads the pair total back between COUNT and FILL."""
    monkeypatch.setenv("SWR_SYNC_FLUSH", "1")
    dev = Device(0, lib=lib)
    monkeypatch.delenv("SWR_SYNC_FLUSH")
    return dev


def _both_modes(device, monkeypatch, name, wireframe=False):
    scene, plan, want = _case(name, wireframe)
    got = _render(device, scene, wireframe=wireframe)
    _check(f"{name} second frame", got, want)
    _check_pairs(name, got[2]["tile_pairs"], plan)
    dev = _sync_device(monkeypatch)
    try:
        sync = _render(dev, scene, wireframe=wireframe)
    finally:
        dev.close()
    _check(f"{name} synchronous flushes", sync, want)
    assert sync[2]["tile_pairs"] == got[2]["tile_pairs"], "the pipelined and the synchronous flush bin different pairs"


@pytest.mark.parametrize("name", list(FAMILIES))
def test_family(device, monkeypatch, name):
    _both_modes(device, monkeypatch, name)


def test_tpw_ladder_in_wireframe(device, monkeypatch):
    """spt = 6: a thread walks six slots, three DrawLine edges per fan triangle, every tile of an edge's box kept."""
    _both_modes(device, monkeypatch, WIREFRAME, wireframe=True)


def _in_parts(device, scene, windows, assemble):
    """The frame rendered part by part (bands or stripes): assembled colour and depth, the fragment counters and tile_pairs summed."""
    cols, deps, tot = [], [], dict.fromkeys(FRAGMENTS + ("tile_pairs",), 0)
    try:
        for setup in windows:
            win = MainWindow(device, scene.width, scene.height)
            setup(win)
            c, d, st = _render(device, scene, window=win)
            cols.append(c); deps.append(d)
            for k in tot:
                tot[k] += st[k]
    finally:
        MainWindow(device, scene.width, scene.height).SetBand(-1, -1)
    return assemble(cols), assemble(deps), tot


def _check_parts(what, got, want, plan):
    c, d, tot = got
    rc, rd, rst = want
    assert_frame_parity(c, d, rc, rd, 1, what)
    for k in FRAGMENTS:
        assert tot[k] == rst[k], f"{what}: summed {k} gpu={tot[k]} oracle={rst[k]}"
    _check_pairs(what, tot["tile_pairs"], plan)


def test_sort_ladder_in_two_bands(device):
    """Tile rows 0-4 and 5-8: 35 and 28 tiles, other groupings of the lists into sort waves, another scan length."""
    scene, plan, want = _case("sort_ladder")
    bands = multigpu.band_partition(scene.height, 2)
    assert [b[1] * plan.tiles_x for b in bands] == [35, 28]
    got = _in_parts(device, scene, [functools.partial(lambda b, w: w.SetBand(*b), b) for b in bands], np.concatenate)
    _check_parts("sort ladder in two bands", got, want, plan)


@pytest.mark.parametrize("name", ["crowded_table", "big_slots"])
def test_interleaved_stripes(device, name):
    """SetBandInterleaved(rank, 2, 1): the tile box stays the frame's, band_local_row is negative for every other row -- in the
    direct path of the crowded table and in both paths of bin_big."""
    scene, plan, want = _case(name)
    got = _in_parts(device, scene, [functools.partial(lambda r, w: w.SetBandInterleaved(r, 2, 1), r) for r in range(2)],
                    lambda parts: multigpu.assemble_stripes(parts, scene.height, 2, 1))
    _check_parts(f"{name} in stripes", got, want, plan)


@pytest.mark.parametrize("name", ["sort_ladder", "crowded_table"])
def test_test_build_is_bit_equal(device, name):
    """libswr_hip_test.so (real fences at the lane-to-lane LDS hand-offs, the general select): the same frame bit for bit."""
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), TEST_LIB)):
        pytest.fail(f"{TEST_LIB} is missing: __graft_entry__.build() makes it (make -C softwarerenderer_amd/csrc variants)")
    scene, plan, want = _case(name)
    c, d, st = _render(device, scene)
    dev = Device(0, lib=TEST_LIB)
    try:
        tc, td, tst = _render(dev, scene)
    finally:
        dev.close()
    assert np.array_equal(td.view(np.uint32), d.view(np.uint32)) and np.array_equal(tc.view(np.uint32), c.view(np.uint32))
    _check(f"{name} on the test build", (tc, td, tst), want)
    assert tst["tile_pairs"] == st["tile_pairs"]
