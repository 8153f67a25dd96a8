"""The front end's record layout and the moved binning decision, against the oracle (depth words bit-exact, colour within 1 ULP,
the counters equal).

Two things changed places and nothing a pixel needs changed value:
  * where the TriRec of a primitive slot lives (rec_index, csrc/swr_device.h): filled batches store even slots densely and the odd
    slots -- second fan triangles of near-clipped quads -- in a region of their own; wireframe batches keep one record per slot;
  * who decides which tiles of a small (<= 8 tiles) slot are binned: k_setup writes the byte want[slot] (small_want_mask), both
    k_bin passes replay it.  The tile bbox is clamped to the context's band first, so the band changes which bit means which tile.
A wrong record address shows as a swapped or stale triangle (translucent layers under BlendMode.Alpha make the order and the
identity of every triangle visible); a disagreement about the bits shows as a dropped or duplicated (triangle, tile) pair, i.e. in
the frame, in fragments_tested / fragments_written, and in tile_pairs -- which is the sum of the want decisions (plus the big
slots' own tests) and must come out the same however the frame is cut into bands or flushed.

What the scenes are built to contain (asserted in test_the_scene_contains_what_it_is_for, on the host):
  (a) several draws whose near-clipped quads -- odd slots -- sit BETWEEN unclipped neighbours;  (e) a frustum-culled draw in the
  middle of the batch;  (f) per-draw triangle counts that are no multiples of 64 and an odd batch total (wave tails; the border
  between the two record regions);  (c) triangles of 2-8 tiles across every band border.
The split of one slot range into several MODE_SYNC rounds needs more than 2^30 pairs and cannot be forced at test sizes; it is
argued from the code in profiles/r07_front_end_records.md."""
import os

import numpy as np
import pytest

import edge_scenes as E
import softwarerenderer_amd.hostmath as hm
from softwarerenderer_amd import Device, MainWindow, _native, multigpu, scenes
from softwarerenderer_amd.rasterizer import BlendMode, CullMode, DebugMode, DepthTest, Program, Rasterizer
from util import assert_frame_parity

pytestmark = pytest.mark.gpu

W, H = 208, 176                      # 13 x 11 tiles: 2 bands = rows 0-5 | 6-10, 3 bands = 0-3 | 4-7 | 8-10
NEAR = 0.9                           # Rasterizer.NearClip of the scene: the clipper cuts at view distance ~1, where triangles are small
DRAW_TRIS = (67, 131, 45, 70, 33, 1)  # per draw; draw 2 is the frustum-culled one.  None a multiple of 64, total 347 (odd)
CULLED_DRAW = 2
COUNTERS = ("triangles_in", "triangles_setup", "triangles_clipped", "fragments_tested", "fragments_shaded", "fragments_written")


def _soup(rng, n):
    """n triangles in view space (camera at the origin looking down -Z, fov 90): two of every three a small triangle at distance
    1.5-4 (a few pixels to a few tiles), every third a needle from BEHIND the camera (w <= 0 -> the clipper runs) to distance
    1.3-1.8, which the near plane cuts into a quad (one vertex outside) or a triangle (two outside) of ordinary screen size."""
    pos = np.empty((n, 3, 3))
    for i in range(n):
        if i % 3 == 1:
            x0, y0 = rng.uniform(-0.8, 0.8), rng.uniform(-0.7, 0.7)
            behind = 1 if rng.uniform() < 0.7 else 2                      # vertices behind the camera: 1 -> quad, 2 -> triangle
            for k in range(3):
                d = -rng.uniform(0.1, 0.3) if k < behind else rng.uniform(1.3, 1.8)
                pos[i, k] = (x0 + rng.uniform(-0.25, 0.25), y0 + rng.uniform(-0.25, 0.25), -d)
            pos[i] = pos[i][rng.permutation(3)]
        else:
            d = rng.uniform(1.5, 4.0)
            c = np.array([rng.uniform(-1, 1) * d, rng.uniform(-0.85, 0.85) * d, -d])
            pos[i] = c + rng.uniform(-0.22, 0.22, (3, 3)) * d * np.array([1.0, 1.0, 0.3])
    return pos


def dense_scene(seed=0):
    """Returns (scene as submitted, oracle's scene = the same without the frustum-culled draw)."""
    rng = np.random.default_rng(100 + seed)
    proj = scenes._perspective(W, H)
    I = hm.identity()
    draws = []
    for di, n in enumerate(DRAW_TRIS):
        pos = _soup(rng, n)
        col = np.concatenate([rng.uniform(0, 1, (3 * n, 3)), rng.uniform(0.25, 0.8, (3 * n, 1))], axis=1)      # translucent: order shows
        v = scenes.make_vertices(pos.reshape(-1, 3), uv=rng.uniform(-2, 3, (3 * n, 2)), color=col)
        model = hm.create_translation(900.0, 0.0, 0.0) if di == CULLED_DRAW else I         # far outside the frustum
        draws.append(scenes.Draw(v, np.arange(3 * n, dtype=np.uint16), model, I, proj, program=Program.Gouraud, cull=CullMode.None_,
                                 depth_test=DepthTest.LessEqual if di % 2 == 0 else DepthTest.Always, blend=BlendMode.Alpha))
    sub = scenes.Scene(f"dense_records_{seed}", W, H, draws, near_clip=NEAR)
    ora = scenes.Scene(sub.name, W, H, [d for i, d in enumerate(draws) if i != CULLED_DRAW], near_clip=NEAR)
    return sub, ora


def _oracle(scene, wireframe=False):
    from oracle.binding import OracleRenderer
    o = OracleRenderer(scene.width, scene.height)
    c, d = o.render_scene(scene, debug_mode=1 if wireframe else 0)
    st = o.stats()
    o.close()
    return c, d, st


def _render(dev, scene, window=None, wireframe=False, frames=1):
    """The scene through RenderMesh, draw CULLED_DRAW with the device-side frustum test; returns colour, depth and the stats of the
    LAST of `frames` identical frames."""
    r = scenes.SceneRenderer(dev, scene, window=window)
    w = r.window
    Rasterizer.RenderDebugMode = DebugMode.Wireframe if wireframe else DebugMode.None_
    try:
        for _ in range(frames):
            dev.reset_stats()
            w._activate()
            Rasterizer.NearClip, Rasterizer.FarClip = scene.near_clip, scene.far_clip
            w.ClearDepthBuffer(); w.ClearColorBuffer(scene.clear_color)
            for i, (d, prog, mesh) in enumerate(zip(scene.draws, r.programs, r.meshes)):
                Rasterizer.RenderMesh(w, mesh, None, d.model, d.view, d.projection, prog.VertexShader, prog.FragmentShader,
                                      d.cull, d.depth_test, d.blend, frustumCull=(len(scene.draws) == len(DRAW_TRIS) and i == CULLED_DRAW))
            c, dz = w._read(True, True)
            st = dev.stats()
    finally:
        Rasterizer.RenderDebugMode = DebugMode.None_
        r.close()
    return c, dz, st


def _check(what, got, want, counters=COUNTERS):
    c, d, st = got
    rc, rd, rst = want
    assert_frame_parity(c, d, rc, rd, 1, what)
    for k in counters:
        assert st[k] == rst[k], f"{what}: stats[{k}] gpu={st[k]} oracle={rst[k]}"


def _clip_counts(scene):
    """Per draw: for every triangle, how many vertices the clipper keeps -- or 3 where it does not run (no vertex with w <= 0)."""
    out = []
    for d in scene.draws:
        p = d.vertices["position"].astype(np.float64)
        clip = np.concatenate([p, np.ones((p.shape[0], 1))], axis=1) @ np.asarray(d.model, np.float64) @ np.asarray(d.view, np.float64) \
            @ np.asarray(d.projection, np.float64)
        clip = clip[d.indices.astype(np.int64)].reshape(-1, 3, 4)
        runs = (clip[:, :, 3] <= 0).any(axis=1) & ~(clip[:, :, 3] <= 0).all(axis=1)
        inside = (clip[:, :, 2] >= scene.near_clip * clip[:, :, 3]).sum(axis=1)
        out.append(np.where(runs, inside, 3))
    return out


def _tile_boxes(scene):
    """(tminx, tmaxx, tminy, tmaxy) of every triangle the clipper leaves alone and that touches the frame."""
    out = []
    for d in scene.draws:
        p = d.vertices["position"].astype(np.float64)
        clip = np.concatenate([p, np.ones((p.shape[0], 1))], axis=1) @ np.asarray(d.model, np.float64) @ np.asarray(d.view, np.float64) \
            @ np.asarray(d.projection, np.float64)
        clip = clip[d.indices.astype(np.int64)].reshape(-1, 3, 4)
        clip = clip[(clip[:, :, 3] > 0).all(axis=1)]
        sx = (clip[:, :, 0] / clip[:, :, 3] * 0.5 + 0.5) * scene.width
        sy = (1.0 - (clip[:, :, 1] / clip[:, :, 3] * 0.5 + 0.5)) * scene.height
        x0, x1 = np.maximum(np.floor(sx.min(axis=1)), 0), np.minimum(np.ceil(sx.max(axis=1)), scene.width - 1)
        y0, y1 = np.maximum(np.floor(sy.min(axis=1)), 0), np.minimum(np.ceil(sy.max(axis=1)), scene.height - 1)
        ok = (x0 <= x1) & (y0 <= y1)
        out.append(np.stack([x0[ok] // 16, x1[ok] // 16, y0[ok] // 16, y1[ok] // 16], axis=1).astype(np.int64))
    return np.concatenate(out)


def test_the_scene_contains_what_it_is_for():
    sub, ora = dense_scene()
    assert all(n % 64 for n in DRAW_TRIS) and sum(DRAW_TRIS) % 2 == 1 and sub.n_triangles == sum(DRAW_TRIS)
    kept = _clip_counts(sub)
    for di, k in enumerate(kept):
        if DRAW_TRIS[di] < 8:
            continue
        quads = np.nonzero(k == 2)[0]               # two vertices inside + two cuts = a quad: its second fan triangle is an odd slot
        assert len(quads) >= 5, (di, len(quads))
        assert quads.min() < len(k) // 3 and quads.max() > 2 * len(k) // 3, "odd slots sit between unclipped neighbours, over the whole draw"
        assert (k == 1).any() or di > 1             # (one vertex inside: clipped, but still one triangle)
    _, _, st = _oracle(ora)
    assert st["triangles_clipped"] >= 60 and st["triangles_setup"] > st["triangles_in"] - 40 and st["fragments_written"] > 20000
    # unclipped triangles of 2-8 tiles across EVERY tile-row border: whichever way the frame is cut, the clamp renumbers some bits
    tb = _tile_boxes(ora)
    small = tb[((tb[:, 1] - tb[:, 0] + 1) * (tb[:, 3] - tb[:, 2] + 1) >= 2) & ((tb[:, 1] - tb[:, 0] + 1) * (tb[:, 3] - tb[:, 2] + 1) <= 8)]
    for border in range(1, (H + 15) // 16):
        assert ((small[:, 2] < border) & (small[:, 3] >= border)).sum() >= 2, f"no small triangle crosses tile row border {border}"


@pytest.fixture(scope="module")
def frames():
    sub, ora = dense_scene()
    return sub, ora, _oracle(ora), _oracle(ora, wireframe=True)


def test_filled_whole_frame(device, frames):
    sub, ora, want, _ = frames
    got = _render(device, sub, frames=2)              # (the second frame is an optimistic, pipelined flush)
    _check("dense filled", got, want)
    assert got[2]["tile_pairs"] > 0


def test_wireframe_whole_frame(device, frames):
    sub, ora, _, want = frames
    _check("dense wireframe", _render(device, sub, wireframe=True, frames=2), want)


@pytest.mark.parametrize("wireframe", [False, True], ids=["filled", "wireframe"])
@pytest.mark.parametrize("world", [2, 3])
def test_tile_row_bands(device, frames, world, wireframe):
    sub, ora, want_f, want_w = frames
    rc, rd, rst = want_w if wireframe else want_f
    whole = _render(device, sub, wireframe=wireframe, frames=2)[2]
    cols, deps, tot = [], [], dict.fromkeys(("fragments_tested", "fragments_shaded", "fragments_written", "tile_pairs"), 0)
    try:
        for band in multigpu.band_partition(H, world):
            win = MainWindow(device, W, H)
            win.SetBand(*band)
            c, d, st = _render(device, sub, window=win, wireframe=wireframe, frames=2)
            assert c.shape[0] == multigpu.band_pixel_rows(H, band)[1]
            cols.append(c); deps.append(d)
            for k in tot:
                tot[k] += st[k]
    finally:
        MainWindow(device, W, H).SetBand(-1, -1)
    assert_frame_parity(np.concatenate(cols), np.concatenate(deps), rc, rd, 1, f"dense bands{world}")
    for k in ("fragments_tested", "fragments_shaded", "fragments_written"):
        assert tot[k] == rst[k], (k, tot[k], rst[k])
    assert tot["tile_pairs"] == whole["tile_pairs"], "the bands' pairs are the frame's pairs: none dropped, none twice"


@pytest.mark.parametrize("wireframe", [False, True], ids=["filled", "wireframe"])
@pytest.mark.parametrize("world,k", [(2, 1), (3, 2)])
def test_interleaved_stripes(device, frames, world, k, wireframe):
    sub, ora, want_f, want_w = frames
    rc, rd, rst = want_w if wireframe else want_f
    whole = _render(device, sub, wireframe=wireframe, frames=2)[2]
    cols, deps, tot = [], [], dict.fromkeys(("fragments_tested", "fragments_shaded", "fragments_written", "tile_pairs"), 0)
    try:
        for rank in range(world):
            win = MainWindow(device, W, H)
            win.SetBandInterleaved(rank, world, k)
            c, d, st = _render(device, sub, window=win, wireframe=wireframe, frames=2)
            cols.append(c); deps.append(d)
            for key in tot:
                tot[key] += st[key]
    finally:
        MainWindow(device, W, H).SetBand(-1, -1)
    c = multigpu.assemble_stripes(cols, H, world, k)
    d = multigpu.assemble_stripes(deps, H, world, k)
    assert_frame_parity(c, d, rc, rd, 1, f"dense stripes world={world} k={k}")
    for key in ("fragments_tested", "fragments_shaded", "fragments_written"):
        assert tot[key] == rst[key], (key, tot[key], rst[key])
    assert tot["tile_pairs"] == whole["tile_pairs"]


@pytest.mark.parametrize("wireframe", [False, True], ids=["filled", "wireframe"])
def test_synchronous_flushes(device, frames, monkeypatch, wireframe):
    """SWR_SYNC_FLUSH=1 (read when the context is created): every flush reads the pair total back between COUNT and FILL."""
    sub, ora, want_f, want_w = frames
    pairs = _render(device, sub, wireframe=wireframe, frames=2)[2]["tile_pairs"]
    monkeypatch.setenv("SWR_SYNC_FLUSH", "1")
    dev = Device(0)
    monkeypatch.delenv("SWR_SYNC_FLUSH")
    try:
        got = _render(dev, sub, wireframe=wireframe, frames=2)
        _check("dense sync", got, want_w if wireframe else want_f)
        assert got[2]["tile_pairs"] == pairs
    finally:
        dev.close()


def test_replay_after_a_fill_overflow(frames, monkeypatch):
    """SWR_DEBUG_FILL_CAPACITY (test build): k_bin<FILL> of the optimistic second frame overflows, the batch poisons itself and the host
    replays it -- k_setup writes slot_tb, want and the records again, the synchronous round bins from them."""
    sub, ora, want, _ = frames
    lib = "libswr_hip_test.so"
    if not os.path.exists(os.path.join(os.path.dirname(_native.LIB_PATH), lib)):
        pytest.fail(f"{lib} is missing: __graft_entry__.build() makes it (make -C softwarerenderer_amd/csrc variants)")
    monkeypatch.setenv("SWR_DEBUG_FILL_CAPACITY", "300")
    dev = Device(0, lib=lib)
    monkeypatch.delenv("SWR_DEBUG_FILL_CAPACITY")
    try:
        r0 = dev.replay_count() if hasattr(dev, "replay_count") else None
        got = _render(dev, sub, frames=2)
        _check("dense replay", got, want)
        if r0 is not None:
            assert dev.replay_count() > r0, "the second frame was not replayed: the hook did not bite"
    finally:
        dev.close()


EDGE = {s.name: s for f in (E.f1_lattice_edges, E.f3_magnitude_ladder, E.f4_slivers) for s in f(0)}


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_families_at_the_binning_margin_in_two_bands(device, name):
    """The families that sit at pair_may_cover's margin (exact lattice edges, the 1e15 magnitude guard, slivers), whole-frame in
    tests/test_gpu_raster_edges.py, here with the decision taken in k_setup under a band clamp."""
    scene = EDGE[name]
    rc, rd, rst = _oracle(scene)
    cols, deps, frag = [], [], 0
    try:
        for band in multigpu.band_partition(scene.height, 2):
            win = MainWindow(device, scene.width, scene.height)
            win.SetBand(*band)
            device.reset_stats()
            r = scenes.SceneRenderer(device, scene, window=win)
            c, d = r.render()
            frag += device.stats()["fragments_written"]
            r.close()
            cols.append(c); deps.append(d)
    finally:
        MainWindow(device, scene.width, scene.height).SetBand(-1, -1)
    assert_frame_parity(np.concatenate(cols), np.concatenate(deps), rc, rd, 1, name + " in two bands")
    assert frag == rst["fragments_written"] > 0
