"""Scenes that put the front end (k_bin<COUNT>, k_scan_sums / k_scan_apply, k_bin<FILL> with tile_place_block, k_sort_tiles: all in
csrc/swr_binning.hip.h, steered by bin_and_raster in csrc/swr_flush.h) where its size-dependent paths switch, and a planner -- plain
numpy, a restatement of the host's decisions -- that says which path a scene reaches.  tests/test_front_end_host.py asserts every
such claim on the CPU; tests/test_gpu_front_end.py renders the scenes.

Geometry.  Identity matrices and clip-space positions (as scenes.cfg1), w = 1: a vertex given in pixels lands on that pixel
coordinate up to float32 rounding.  The reference samples a pixel at its INTEGER coordinate (Rasterizer.cs:481-483) and forms the
pixel box as floor(min) .. ceil(max), the tile box as that / 16: so a vertex coordinate whose fraction lies in [0.25, 0.75] -- every
vertex here sits at .5 -- is a quarter pixel away from everything that decides a box or a tile, and plan() asserts it on the
float32 screen coordinates it recomputes the way DrawTriangle does.

The staircase.  All triangles of one tile's list have the same vertices in x and y (they cover the same few pixels) and a depth
that passes DepthTest.Less against every earlier one (the reference's Less is `new > old`, the clear value is -FLT_MAX, and its
barycentric weights sum to -1 -- edge values over an area of the other sign convention --, so a filled triangle's depth is
-(z + 1) / 2: z FALLS along the list).  In submission order every fragment passes: fragments_written == fragments_tested.  An
inversion ANYWHERE in the list makes the overtaken triangle fail on all its pixels: fragments_written drops.  A lost pair lowers
fragments_tested, a duplicated one raises it.  Alpha blending alone sees only the tail of a long list (test_front_end_host.py shows that).
A tile's triangles are spread evenly over the whole batch, so k_bin<FILL>'s cursors hand out list positions in no particular order.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

import softwarerenderer_amd.hostmath as hm
from softwarerenderer_amd import scenes
from softwarerenderer_amd.rasterizer import BlendMode, CullMode, DepthTest, Program

TILE = 16
SWR_SMALL_TILES = 8            # csrc/swr_device.h
SWR_BIN_TABLE = 256            # csrc/swr_binning.hip.h: entries of k_bin's hash table
SWR_SORT_TPW = 4               # tiles per sort wave
SWR_SORT_LDS = 2048            # longest list sorted in LDS
SWR_SCAN_BLOCK = 256           # tiles per scan block
MAX_DRAW_TRIS = 21845          # 16-bit indices, unshared vertices
MARGIN = 0.25                  # px: every vertex is at least this far from an integer coordinate
EDGE_MARGIN = 1.0 / 64.0       # px: a pixel counts as covered for certain only this far inside all three edges
SORT_LADDER_COUNTS = (0, 1, 2, 3, 33, 63, 64, 65, 96, 127, 128, 129, 1023, 2047, 2048, 2049)
TPW_LADDER_T = (8191, 8193, 16385, 32769, 65537)
TILING_LADDER = ((1, 1), (257, 1), (1, 33), (16, 16), (17, 15), (17, 17), (27, 19), (33, 2))
TILING_ODD_PIXELS = (100, 75)  # 7 x 5 tiles, the last column 4 px wide, the last row 11 px high


# ----------------------------------------------------------------------------------------------- building
def _scene(name, width, height, tri_px, z, rgba, depth_test, blend=BlendMode.Alpha) -> scenes.Scene:
    """tri_px: (T, 3, 2) pixel coordinates, z: (T,) clip-space z of all three vertices, rgba: (T, 4).  One batch of as many draws as
    16-bit indices need, all with the same state."""
    tri_px = np.asarray(tri_px, np.float64)
    T = tri_px.shape[0]
    pos = np.empty((T, 3, 3))
    pos[:, :, 0] = tri_px[:, :, 0] / width * 2.0 - 1.0
    pos[:, :, 1] = 1.0 - tri_px[:, :, 1] / height * 2.0
    pos[:, :, 2] = np.asarray(z, np.float64)[:, None]
    col = np.repeat(np.asarray(rgba, np.float64), 3, axis=0)
    I = hm.identity()
    draws = []
    for lo in range(0, T, MAX_DRAW_TRIS):
        hi = min(T, lo + MAX_DRAW_TRIS)
        v = scenes.make_vertices(pos[lo:hi].reshape(-1, 3), color=col[3 * lo:3 * hi])
        draws.append(scenes.Draw(v, np.arange(3 * (hi - lo), dtype=np.uint16), I, I, I, program=Program.Gouraud, cull=CullMode.None_,
                                 depth_test=depth_test, blend=blend))
    return scenes.Scene(name, width, height, draws, clear_color=(0.0, 0.0, 0.0, 1.0))


def _colours(rng, n):
    return np.concatenate([rng.uniform(0.05, 1.0, (n, 3)), rng.uniform(0.3, 0.7, (n, 1))], axis=1)


def _corner(x, y, lx, ly):
    """Right triangle with its right angle at (x, y) and legs lx, ly (signed) along the axes."""
    return [(x, y), (x + lx, y), (x, y + ly)]


def _spread(counts, rng):
    """Submission order for lists of counts[i] triangles each: list i's k-th triangle goes to position (k + phase_i) / counts[i] of
    the batch, so every list is scattered over the whole batch and stays in its own order.  Returns (list index, k) per triangle."""
    counts = np.asarray(counts, np.int64)
    which = np.repeat(np.arange(len(counts)), counts)
    k = np.concatenate([np.arange(c) for c in counts]) if counts.sum() else np.zeros(0, np.int64)
    phase = rng.uniform(0.05, 0.95, len(counts))
    key = (k + phase[which]) / np.maximum(counts[which], 1)
    o = np.argsort(key, kind="stable")
    return which[o], k[o]


def _stair_z(k):
    """z of the k-th triangle of a list: steps of 2^-11 in z = 2^-12 in depth, thousands of float32 ULPs apart."""
    return 0.0625 - np.asarray(k, np.float64) / 2048.0


# ----------------------------------------------------------------------------------------------- families
def sort_ladder(counts_per_tile=None, tiles_x=7, tiles_y=9, seed=0, name="sort_ladder"):
    """k_sort_tiles' four paths in one launch.  63 tiles (no multiple of SWR_SORT_TPW) whose list lengths are SORT_LADDER_COUNTS,
    each once, on the first tiles of a random permutation; of the other tiles two in three have lengths of 66-200 (LDS path), the
    rest of 0-5, so that a wave -- which takes entries w, w + 16, w + 32, w + 48 of the heaviest-first order -- sorts several lists
    on the LDS path one after the other in its one LDS slice, after a long first one, and ends with lists of n < 2 or in registers.
    Every triangle is a one-tile staircase primitive of 10 pixels.  Returns (scene, per-tile counts)."""
    rng = np.random.default_rng(1000 + seed)
    n_tiles = tiles_x * tiles_y
    if counts_per_tile is None:
        rest = [int(rng.integers(66, 200)) if i % 3 != 2 else int(rng.integers(0, 6)) for i in range(n_tiles - len(SORT_LADDER_COUNTS))]
        counts = np.array(list(SORT_LADDER_COUNTS) + rest, np.int64)[rng.permutation(n_tiles)]
    else:
        counts = np.asarray(counts_per_tile, np.int64)
        assert counts.shape == (n_tiles,)
    tile, k = _spread(counts, rng)
    tx, ty = tile % tiles_x, tile // tiles_x
    tri = np.array([_corner(4.5, 4.5, 5.0, 4.0)] * len(tile)) + np.stack([tx * TILE, ty * TILE], axis=1)[:, None, :]
    return _scene(name, tiles_x * TILE, tiles_y * TILE, tri, _stair_z(k), _colours(rng, len(tile)), DepthTest.Less), counts


def crowded_table(n_tris=16384 + 37, seed=0):
    """k_bin's "crowded table: go direct" branch, in COUNT and in FILL.  tpw = 16: a block bins 64 consecutive triangles.  64 x 64
    tiles; triangle i is a sliver 5 px high over the 8 tiles of span i % 512 (8 spans per tile row, 64 rows), with a pixel in each
    of them: the 64 triangles of a block want 512 distinct tiles, twice what the table holds.  A span comes round every 8 blocks, so
    a tile collects a pair from each of 32 (33) blocks: a staircase."""
    rng = np.random.default_rng(2000 + seed)
    i = np.arange(n_tris)
    span = i % 512
    row, seg = span // 8, span % 8
    x0, y0 = seg * 128 + 0.5, row * TILE + 4.5
    tri = np.stack([np.stack([x0, y0], 1), np.stack([x0 + 120.0, y0], 1), np.stack([x0 + 120.0, y0 + 5.0], 1)], axis=1)
    return _scene("crowded_table", 64 * TILE, 64 * TILE, tri, _stair_z(i // 512), _colours(rng, n_tris), DepthTest.Less)


def tpw_ladder(n_tris, seed=0):
    """tpw = 4, 8, 16, 32, 64 for TPW_LADDER_T, each with a ragged last wave and last block: random translucent triangles of a few
    pixels at random depths under LessEqual (order and depth both decide a pixel), 20 x 13 tiles."""
    rng = np.random.default_rng(3000 + seed + n_tris)
    W, H = 20 * TILE, 13 * TILE
    c = np.stack([rng.integers(4, W - 4, n_tris), rng.integers(4, H - 4, n_tris)], axis=1) + 0.5
    tri = c[:, None, :] + rng.integers(-3, 4, (n_tris, 3, 2))
    return _scene(f"tpw_ladder_{n_tris}", W, H, tri, rng.uniform(-0.9, 0.9, n_tris), _colours(rng, n_tris), DepthTest.LessEqual)


# big slots: tile boxes (nx, ny) by class
BIG_SMALL = ((8, 1), (2, 4), (4, 2), (1, 8), (1, 1), (3, 2))
BIG_MEDIUM = ((3, 3), (8, 8), (64, 1), (1, 17), (9, 1), (4, 16), (16, 4), (1, 9))
BIG_LARGE = ((65, 1), (13, 5), (5, 13), (66, 17), (33, 2))
BIG_GROUPS = ((1, 2, 5), (2, 2, 4), (3, 1, 4), (4, 3, 1), (5, 1, 2), (7, 1, 0))      # (medium, large, small) slots of a wave: 8 each
BIG_TPW = 8
BIG_T = 8192 + 5


def _box_triangle(tx, ty, nx, ny, flip):
    """A right triangle whose tile box is exactly nx x ny tiles from tile (tx, ty); right angle at the bottom right (the LAST tile of
    the row-major walk is covered) or, flipped, at the top left."""
    x0, x1, y0, y1 = tx * TILE + 0.5, (tx + nx - 1) * TILE + 14.5, ty * TILE + 0.5, (ty + ny - 1) * TILE + 14.5
    return [(x0, y0), (x1, y0), (x0, y1)] if flip else [(x1, y1), (x0, y1), (x1, y0)]


def big_slots(seed=0):
    """bin_big's two paths at their limits.  66 x 17 tiles; tile boxes of exactly 8 (small), 9 and 64 (medium: four at a time) and 65
    and more (large: strided loop).  At tpw = 8 a wave bins 8 consecutive triangles; the waves listed in the returned `groups`
    hold k = 1, 2, 3, 4, 5, 7 medium slots beside large and small ones over the same tiles (BIG_GROUPS); the batch is padded with tiny
    triangles to 8192 + 5.  Everything at one depth under LessEqual and translucent: order inside the shared tiles shows.
    Returns (scene, {wave index: (medium, large, small)})."""
    rng = np.random.default_rng(4000 + seed)
    TX, TY = 66, 17
    W, H = TX * TILE, TY * TILE
    c = np.stack([rng.integers(4, W - 4, BIG_T), rng.integers(4, H - 4, BIG_T)], axis=1) + 0.5
    tri = c[:, None, :] + rng.integers(-2, 3, (BIG_T, 3, 2))
    groups: Dict[int, tuple] = {}
    im = il = ism = 0
    waves = BIG_T // BIG_TPW
    for rep in range(3):                                        # each group three times, at the start, the middle and the end of the batch
        for gi, (m, l, s) in enumerate(BIG_GROUPS):
            wave = (3 + 7 * gi, waves // 2 + 5 * gi, waves - 40 + 6 * gi)[rep]
            kinds = ["m"] * m + ["l"] * l + ["s"] * s
            kinds = [kinds[j] for j in rng.permutation(len(kinds))]
            assert len(kinds) == BIG_TPW
            for j, kd in enumerate(kinds):
                if kd == "m":
                    nx, ny = BIG_MEDIUM[im % len(BIG_MEDIUM)]; im += 1
                elif kd == "l":
                    nx, ny = BIG_LARGE[il % len(BIG_LARGE)]; il += 1
                else:
                    nx, ny = BIG_SMALL[ism % len(BIG_SMALL)]; ism += 1
                # all over the tiles around (32, 8): the boxes are placed so that they contain it where their size allows
                tx = int(np.clip(32 - rng.integers(0, nx), 0, TX - nx))
                ty = int(np.clip(8 - rng.integers(0, ny), 0, TY - ny))
                tri[wave * BIG_TPW + j] = _box_triangle(tx, ty, nx, ny, flip=(kd != "m" and (im + il + ism) % 3 == 0))
            groups[wave] = (m, l, s)
    return _scene("big_slots", W, H, tri, np.zeros(BIG_T), _colours(rng, BIG_T), DepthTest.LessEqual), groups


def tiling_stair_tiles(n_tiles):
    """Tile 0, the last tile and the tiles on both sides of every seam between two scan blocks."""
    t = {0, n_tiles - 1}
    for seam in range(SWR_SCAN_BLOCK, n_tiles, SWR_SCAN_BLOCK):
        t |= {seam - 1, seam}
    return sorted(t)


def tiling_ladder(tiles_x=None, tiles_y=None, pixels=None, stair=37, seed=0):
    """The scan's seams and tile_place_block's regions.  One marker triangle of 3 pixels in EVERY tile (a lost or misplaced tile is a
    missing marker, and every tile has a pair), and a staircase of `stair` more on the marker's pixels in tiling_stair_tiles().
    Returns (scene, per-tile counts)."""
    W, H = pixels if pixels else (tiles_x * TILE, tiles_y * TILE)
    tiles_x, tiles_y = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rng = np.random.default_rng(5000 + seed + 100 * tiles_x + tiles_y)
    n_tiles = tiles_x * tiles_y
    counts = np.ones(n_tiles, np.int64)
    counts[tiling_stair_tiles(n_tiles)] += stair
    tile, k = _spread(counts, rng)
    tri = np.array([_corner(0.5, 0.5, 3.0, 2.0)] * len(tile)) + np.stack([tile % tiles_x * TILE, tile // tiles_x * TILE], axis=1)[:, None, :]
    return _scene(f"tiling_{W}x{H}", W, H, tri, _stair_z(k), _colours(rng, len(tile)), DepthTest.Less), counts


# ----------------------------------------------------------------------------------------------- the planner
def host_tpw(n_tris):
    """bin_and_raster: triangles per k_bin wave."""
    tpw = 64
    while tpw > 4 and n_tris < tpw * 1024:
        tpw >>= 1
    return tpw


@dataclass
class Plan:
    n_tris: int
    tiles_x: int
    tiles_y: int
    spt: int
    tpw: int
    bin_blocks: int
    last_wave_tris: int            # triangles in the last, ragged wave (tpw: it is full)
    last_block_tris: int
    box: np.ndarray                # (T, 4) tminx, tmaxx, tminy, tmaxy; -1 where the triangle is off the frame or degenerate
    box_tiles: np.ndarray          # (T,) tiles of the box
    cls: np.ndarray                # (T,) 0 nothing, 1 small (<= 8 tiles), 2 medium (9-64), 3 large (> 64)
    pixels: np.ndarray             # (T,) pixels covered for certain
    near_edge: np.ndarray          # (T,) pixels of the box within EDGE_MARGIN of an edge (0 everywhere: `pixels` is exact)
    lo: np.ndarray                 # (n_tiles,) pairs at least: triangles with a pixel of that tile covered for certain
    hi: np.ndarray                 # (n_tiles,) pairs at most: tile boxes
    block_small_tiles: List[int]   # per k_bin block: distinct tiles certainly wanted by its small slots
    sx: np.ndarray                 # (T, 3) float32 screen coordinates
    sy: np.ndarray
    pairs: Optional[np.ndarray] = None      # (n, 2) (triangle, tile) with a pixel covered for certain

    @property
    def exact(self):
        """Built from certain primitives only: every tile of every box is covered, and no pixel is in doubt."""
        return bool((self.lo == self.hi).all() and not self.near_edge.any())


def screen_coordinates(scene):
    """float32 screen coordinates of every triangle of the batch, computed as DrawTriangle does (Rasterizer.cs:371-386) for w = 1."""
    sx, sy = [], []
    f = np.float32
    for d in scene.draws:
        for m in (d.model, d.view, d.projection):
            assert np.array_equal(np.asarray(m, np.float64), np.eye(4)), "the planner is for identity matrices"
        p = d.vertices["position"][d.indices.astype(np.int64)].reshape(-1, 3, 3).astype(np.float32)
        sx.append((p[:, :, 0] * f(0.5) + f(0.5)) * f(scene.width))
        sy.append((f(1.0) - (p[:, :, 1] * f(0.5) + f(0.5))) * f(scene.height))
    return np.concatenate(sx), np.concatenate(sy)


def _coverage(sx, sy, x0, x1, y0, y1, tiles_x):
    """For triangles (float64 coordinates) with pixel boxes [x0, x1] x [y0, y1]: per triangle the pixels covered for certain, the
    pixels in doubt, and the (triangle, tile) pairs with a certain pixel.  Vectorised per box size."""
    T = len(sx)
    pixels, doubt = np.zeros(T, np.int64), np.zeros(T, np.int64)
    pair_tri, pair_tile = [], []
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    valid = (bw > 0) & (bh > 0)
    keys = np.where(valid, bw * 100000 + bh, -1)
    for key in np.unique(keys[valid]):
        idx_all = np.nonzero(keys == key)[0]
        w, h = int(key // 100000), int(key % 100000)
        step = max(1, (1 << 22) // (w * h))
        for s in range(0, len(idx_all), step):
            idx = idx_all[s:s + step]
            X = (x0[idx, None, None] + np.arange(w)[None, None, :]).astype(np.float64)
            Y = (y0[idx, None, None] + np.arange(h)[None, :, None]).astype(np.float64)
            dmin, dmax = None, None
            for a, b in ((0, 1), (1, 2), (2, 0)):
                ex, ey = (sx[idx, b] - sx[idx, a])[:, None, None], (sy[idx, b] - sy[idx, a])[:, None, None]
                d = (ex * (Y - sy[idx, a][:, None, None]) - ey * (X - sx[idx, a][:, None, None])) / np.sqrt(ex * ex + ey * ey)
                dmin = d if dmin is None else np.minimum(dmin, d)
                dmax = d if dmax is None else np.maximum(dmax, d)
            inside = (dmin > EDGE_MARGIN) | (dmax < -EDGE_MARGIN)
            maybe = ((dmin >= -EDGE_MARGIN) | (dmax <= EDGE_MARGIN)) & ~inside
            pixels[idx] = inside.sum(axis=(1, 2))
            doubt[idx] = maybe.sum(axis=(1, 2))
            tile = ((Y.astype(np.int64) // TILE) * tiles_x + X.astype(np.int64) // TILE) + np.zeros_like(inside, np.int64)
            pk = np.unique(idx[:, None, None] * (1 << 24) + np.where(inside, tile, (1 << 24) - 1))
            pk = pk[(pk & ((1 << 24) - 1)) != (1 << 24) - 1]
            pair_tri.append(pk >> 24); pair_tile.append(pk & ((1 << 24) - 1))
    cat = lambda l: np.concatenate(l) if l else np.zeros(0, np.int64)
    return pixels, doubt, cat(pair_tri), cat(pair_tile)


def plan(scene, wireframe=False, rows=None) -> Plan:
    """What the host and the kernels decide for this scene as ONE batch.  rows = (first tile row, tile rows): a contiguous band --
    tile boxes are clamped to it before they are classified, as slot_tiles does."""
    W, H = scene.width, scene.height
    tiles_x, tiles_y = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    sx, sy = screen_coordinates(scene)
    T = len(sx)
    for s in (sx, sy):
        frac = s.astype(np.float64) - np.floor(s.astype(np.float64))
        assert ((frac >= MARGIN) & (frac <= 1.0 - MARGIN)).all(), "a vertex within a quarter pixel of a pixel centre / tile border"
    x0 = np.maximum(np.floor(sx.min(axis=1)), 0).astype(np.int64); x1 = np.minimum(np.ceil(sx.max(axis=1)), W - 1).astype(np.int64)
    y0 = np.maximum(np.floor(sy.min(axis=1)), 0).astype(np.int64); y1 = np.minimum(np.ceil(sy.max(axis=1)), H - 1).astype(np.int64)
    sx64, sy64 = sx.astype(np.float64), sy.astype(np.float64)
    # EdgeFunction(screen of v2, v1, v0) in float32, as DrawTriangle forms it (Rasterizer.cs:396, 562): a triangle is dropped where THAT
    # is zero -- vertices that are collinear on the half-pixel lattice stay so here although their float32 coordinates are not exactly
    area = (sx[:, 0] - sx[:, 2]) * (sy[:, 1] - sy[:, 2]) - (sy[:, 0] - sy[:, 2]) * (sx[:, 1] - sx[:, 2])
    assert area.dtype == np.float32
    ok = (x0 <= x1) & (y0 <= y1) & (area != 0)
    x1 = np.where(ok, x1, x0 - 1)
    ty_lo, ty_hi = (0, tiles_y) if rows is None else (rows[0], rows[0] + rows[1])
    box = np.stack([x0 // TILE, x1 // TILE, np.maximum(y0 // TILE, ty_lo), np.minimum(y1 // TILE, ty_hi - 1)], axis=1)
    ok &= box[:, 2] <= box[:, 3]
    box[~ok] = -1
    box_tiles = np.where(ok, (box[:, 1] - box[:, 0] + 1) * (box[:, 3] - box[:, 2] + 1), 0)
    cls = np.where(box_tiles == 0, 0, np.where(box_tiles <= SWR_SMALL_TILES, 1, np.where(box_tiles <= 64, 2, 3)))
    # pixels and pairs, inside the band's rows
    py0, py1 = np.maximum(y0, ty_lo * TILE), np.minimum(y1, ty_hi * TILE - 1)
    pixels, doubt, ptri, ptile = _coverage(sx64, sy64, x0, np.where(ok, x1, x0 - 1), py0, py1, tiles_x)
    n_tiles = tiles_x * tiles_y
    lo = np.bincount(ptile, minlength=n_tiles)
    hi = np.zeros(n_tiles, np.int64)
    for nx_ny in np.unique(np.stack([box[ok, 1] - box[ok, 0], box[ok, 3] - box[ok, 2]], axis=1), axis=0) if ok.any() else []:
        sel = ok & (box[:, 1] - box[:, 0] == nx_ny[0]) & (box[:, 3] - box[:, 2] == nx_ny[1])
        gx = box[sel, 0][:, None, None] + np.arange(nx_ny[0] + 1)[None, None, :]
        gy = box[sel, 2][:, None, None] + np.arange(nx_ny[1] + 1)[None, :, None]
        hi += np.bincount((gy * tiles_x + gx).reshape(-1), minlength=n_tiles)
    if wireframe:
        # DrawLine (Rasterizer.cs:242-257): per edge the box of the two end points, truncated, every tile of it kept
        lo = np.zeros(n_tiles, np.int64)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            ex0 = np.maximum(np.minimum(sx[:, a], sx[:, b]), 0).astype(np.int64); ex1 = np.minimum(np.maximum(sx[:, a], sx[:, b]), W - 1).astype(np.int64)
            ey0 = np.maximum(np.minimum(sy[:, a], sy[:, b]), 0).astype(np.int64); ey1 = np.minimum(np.maximum(sy[:, a], sy[:, b]), H - 1).astype(np.int64)
            for t in np.nonzero(ok & (ex0 <= ex1) & (ey0 <= ey1))[0]:
                for ty in range(max(ey0[t] // TILE, ty_lo), min(ey1[t] // TILE, ty_hi - 1) + 1):
                    lo[ty * tiles_x + ex0[t] // TILE: ty * tiles_x + ex1[t] // TILE + 1] += 1
        hi = lo.copy()
        pixels, doubt = np.zeros(T, np.int64), np.zeros(T, np.int64)     # (of filled triangles: not this mode's)
    tpw = host_tpw(T)
    per_block = 4 * tpw
    bin_blocks = (T + per_block - 1) // per_block
    small_pair = cls[ptri] == 1
    blk = ptri[small_pair] // per_block
    block_small_tiles = np.bincount(np.unique(blk * (1 << 24) + ptile[small_pair]) >> 24, minlength=bin_blocks).tolist() if T else []
    return Plan(T, tiles_x, tiles_y, 6 if wireframe else 2, tpw, bin_blocks, T - (T - 1) // tpw * tpw, T - (bin_blocks - 1) * per_block,
                box, box_tiles, cls, pixels, doubt, lo, hi, block_small_tiles, sx, sy, np.stack([ptri, ptile], axis=1))


def sort_path(n):
    """k_sort_tiles / sort_tile: which of the four paths a list of n pairs takes."""
    return "none" if n < 2 else "registers" if n <= 64 else "lds" if n <= SWR_SORT_LDS else "global"


def order_bucket(w):
    """order_bucket of csrc/swr_binning.hip.h."""
    if w == 0:
        return 0
    e = int(w).bit_length() - 1
    m = ((w >> (e - 3)) & 7) if e >= 3 else ((w << (3 - e)) & 7)
    return min(e * 8 + m + 1, 255)


def sort_wave_paths(counts, frags_per_pair=0):
    """For per-tile pair counts, the sort paths each wave of k_sort_tiles takes, in the order it takes them -- for ONE order that the
    counting sort may produce (inside a bucket the kernel's order is arbitrary; here it is by tile index).  Weight of a tile =
    fragments of the previous flush (frags_per_pair each; 0: first frame) + 16 per pair."""
    counts = np.asarray(counts, np.int64)
    b = np.array([order_bucket(int(c) * (16 + frags_per_pair)) for c in counts])
    order = np.argsort(-b, kind="stable")
    waves = (len(counts) + SWR_SORT_TPW - 1) // SWR_SORT_TPW
    return [[sort_path(int(counts[order[e]])) for e in range(w, len(counts), waves)] for w in range(waves)], b


def with_edit(scene, swap=None, drop=None, twice=None):
    """A copy of a one-draw scene with triangles swap = (i, j) exchanged in submission order, triangle `drop` left out, or triangle
    `twice` submitted a second time right after itself (what a wrong front end would do to a tile's list)."""
    assert len(scene.draws) == 1
    d = scene.draws[0]
    order = list(range(d.indices.size // 3))
    if swap is not None:
        order[swap[0]], order[swap[1]] = order[swap[1]], order[swap[0]]
    if drop is not None:
        order.remove(drop)
    if twice is not None:
        order.insert(order.index(twice) + 1, twice)
    idx = d.indices.reshape(-1, 3)[order].reshape(-1).astype(np.uint16)
    nd = scenes.Draw(d.vertices, idx, d.model, d.view, d.projection, program=d.program, cull=d.cull, depth_test=d.depth_test, blend=d.blend)
    return scenes.Scene(scene.name + "_edited", scene.width, scene.height, [nd], clear_color=scene.clear_color)
