"""The claims tests/test_gpu_front_end.py rests on, on the CPU: that each scene of tests/front_end_scenes.py reaches the path it is
for (planner against the constants of csrc/swr_binning.hip.h and the loop of bin_and_raster), that the planner's pair and pixel
counts are the oracle's, that a staircase scene writes every fragment it tests, and -- on the oracle, with the edits a wrong front
end would make to a tile's list -- that the counters see an inversion, a lost and a duplicated pair anywhere in a list, where the
colours do not."""
import re
import os

import numpy as np
import pytest

import front_end_scenes as F
from util import render_oracle, ulp_distance

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "softwarerenderer_amd", "csrc")


def _define(text, name):
    return re.search(r"#define\s+" + name + r"\s+(.+?)\s*(?://.*)?$", text, re.M).group(1)


def test_the_constants_are_the_kernels():
    b = open(os.path.join(CSRC, "swr_binning.hip.h")).read()
    d = open(os.path.join(CSRC, "swr_device.h")).read()
    f = open(os.path.join(CSRC, "swr_flush.h")).read()
    assert 1 << int(_define(b, "SWR_BIN_TABLE_LOG2")) == F.SWR_BIN_TABLE
    assert int(_define(b, "SWR_SORT_TPW")) == F.SWR_SORT_TPW and int(_define(b, "SWR_SORT_LDS")) == F.SWR_SORT_LDS
    assert int(_define(b, "SWR_SCAN_BLOCK")) == F.SWR_SCAN_BLOCK and int(_define(d, "SWR_SMALL_TILES")) == F.SWR_SMALL_TILES
    assert int(_define(b, "SWR_SORT_TPB")) == 1
    assert "while (ba.tpw > 4u && bin_threads < ba.tpw * 1024u) ba.tpw >>= 1;" in f and "ba.tpw = 64u;" in f
    assert "(bin_threads + 4u * ba.tpw - 1u) / (4u * ba.tpw)" in f and "ba.spt = b.wireframe ? 6u : 2u;" in f
    assert "if (n <= 64) {" in b and "if (n < 2) return;" in b and "nt <= 64" in b and "nt > 64" in b


@pytest.fixture(scope="module")
def ladder():
    scene, counts = F.sort_ladder()
    return scene, counts, F.plan(scene), render_oracle(scene)


def test_sort_ladder_reaches_every_path_and_mixes_them_in_a_wave(ladder):
    scene, counts, p, _ = ladder
    assert (p.tiles_x, p.tiles_y) == (7, 9) and (p.tiles_x * p.tiles_y) % F.SWR_SORT_TPW != 0
    assert set(F.SORT_LADDER_COUNTS) <= set(counts.tolist())
    assert p.exact and np.array_equal(p.lo, counts), "one pair per triangle, in its own tile"
    assert {F.sort_path(int(c)) for c in counts} == {"none", "registers", "lds", "global"}
    assert (p.cls == 1).all() and (p.box_tiles == 1).all()
    # Whatever order the counting sort produces inside a bucket: 16 waves of at most 4 lists each, and more lists that go through
    # the wave's LDS slice (or past it, in global memory) than waves -- so at least (heavy - 16) / 3 waves sort a second such list
    # in the slice the first one used, and 16 lists of n <= 64 or n < 2 cannot all sit in waves of their own.
    heavy = sum(F.sort_path(int(c)) in ("lds", "global") for c in counts)
    assert (len(counts) + F.SWR_SORT_TPW - 1) // F.SWR_SORT_TPW == 16 and -((16 - heavy) // 3) >= 7
    assert sum(F.sort_path(int(c)) in ("none", "registers") for c in counts) >= 20
    # ... and in the order the sort produces when ties inside a bucket fall by tile index, for the first frame (weights: pairs alone)
    # and the second (+ fragments tested, 10 per pair):
    for frags in (0, 10):
        waves, buckets = F.sort_wave_paths(counts, frags)
        assert len(waves) == 16 and all(w[0] in ("lds", "global") for w in waves)
        assert sum(sum(x == "lds" for x in w) >= 2 for w in waves) >= 8
        assert sum(("registers" in w[1:] or "none" in w[1:]) for w in waves) >= 8
        assert any(w[0] == "global" and "lds" in w[1:] for w in waves)
    # a tile's triangles are scattered over the whole batch
    first_tile = int(np.argmax(counts))
    mine = np.nonzero((p.box[:, 0] + p.box[:, 2] * p.tiles_x) == first_tile)[0]
    assert mine[0] < 20 and mine[-1] > p.n_tris - 20 and np.diff(mine).max() <= 16
    assert p.tpw == 8


def test_crowded_table_overflows_the_hash_table_in_every_full_block():
    scene = F.crowded_table()
    p = F.plan(scene)
    assert p.n_tris == 16384 + 37 and p.tpw == 16 and (p.tiles_x, p.tiles_y) == (64, 64)
    assert (p.box_tiles == 8).all() and (p.cls == 1).all() and (p.box[:, 2] == p.box[:, 3]).all()
    assert p.exact, "every sliver has a pixel in each of its 8 tiles"
    full = p.n_tris // 64
    assert p.bin_blocks == full + 1 and p.last_block_tris == 37 and p.last_wave_tris == 37 % 16
    surplus = np.array(p.block_small_tiles[:full]) - F.SWR_BIN_TABLE
    assert (surplus == 256).all(), "512 distinct wanted tiles per block: at least 256 pairs cannot enter the table"
    assert p.lo.min() >= 32 and p.lo.max() == 33, "every tile collects pairs from 32 or 33 different blocks"
    c, d, st = render_oracle(scene)
    assert st["fragments_written"] == st["fragments_tested"] == int(p.pixels.sum())


@pytest.mark.parametrize("n_tris,tpw", list(zip(F.TPW_LADDER_T, (4, 8, 16, 32, 64))))
def test_tpw_ladder(n_tris, tpw):
    assert F.host_tpw(n_tris) == tpw
    if tpw > 4:
        assert F.host_tpw(tpw * 1024 - 1) == tpw // 2 and F.host_tpw(tpw * 1024) == tpw, "T sits right above the threshold"
    assert n_tris % tpw != 0 and n_tris % (4 * tpw) != 0, "ragged last wave and last block"
    p = F.plan(F.tpw_ladder(n_tris))
    assert p.tpw == tpw and p.n_tris == n_tris and 0 < p.last_wave_tris < tpw and 0 < p.last_block_tris < 4 * tpw
    assert p.bin_blocks == (n_tris + 4 * tpw - 1) // (4 * tpw)
    assert (p.cls[p.box_tiles > 0] == 1).all() and p.lo.sum() <= p.hi.sum() and p.lo.min() > 0
    if n_tris == 8193:              # the one that also runs in wireframe: a thread walks 6 slots, every tile of an edge's box is kept
        pw = F.plan(F.tpw_ladder(n_tris), wireframe=True)
        assert pw.spt == 6 and pw.tpw == tpw and pw.exact and pw.lo.sum() > p.hi.sum()


def test_big_slots_hold_the_boundaries_and_the_group_sizes():
    scene, groups = F.big_slots()
    p = F.plan(scene)
    assert p.tpw == F.BIG_TPW == 8 and (p.tiles_x, p.tiles_y) == (66, 17) and p.n_tris % 8 != 0
    assert {9, 64} <= set(p.box_tiles[p.cls == 2].tolist()) and {65} <= set(p.box_tiles[p.cls == 3].tolist()) and 8 in p.box_tiles[p.cls == 1]
    shapes = {(int(b[1] - b[0] + 1), int(b[3] - b[2] + 1)) for b in p.box[p.cls >= 2]}
    assert {(3, 3), (8, 8), (64, 1), (1, 17), (65, 1), (13, 5), (5, 13)} <= shapes
    seen = set()
    for wave, (m, l, s) in groups.items():
        cls = p.cls[wave * 8:(wave + 1) * 8]
        assert ((cls == 2).sum(), (cls == 3).sum(), (cls == 1).sum()) == (m, l, s), (wave, cls)
        seen.add(m)
        # the slots of the wave meet in tiles: every big one shares a tile with another slot of the wave
        b = p.box[wave * 8:(wave + 1) * 8]
        for i in np.nonzero(cls >= 2)[0]:
            assert any(j != i and b[i, 0] <= b[j, 1] and b[j, 0] <= b[i, 1] and b[i, 2] <= b[j, 3] and b[j, 2] <= b[i, 3] for j in range(8))
    assert seen == {1, 2, 3, 4, 5, 7}
    # no other wave holds a big slot: the padding is small
    big_waves = set((np.nonzero(p.cls >= 2)[0] // 8).tolist())
    assert big_waves == set(groups)
    # the last tile of every medium box (row-major: what the last lane of the four-at-a-time path bins) is covered for certain
    med = np.nonzero(p.cls == 2)[0]
    assert len(med) == 3 * (1 + 2 + 3 + 4 + 5 + 7)
    certain = set(map(tuple, p.pairs.tolist()))
    assert all((int(i), int(p.box[i, 3] * p.tiles_x + p.box[i, 1])) in certain for i in med)
    assert (p.lo <= p.hi).all() and p.lo.sum() < p.hi.sum()


def test_big_slots_hand_the_register_sort_lists_that_are_out_of_order():
    """bin_block_slots bins a block's small slots through the table and calls bin_big after the table's barriers: a big slot
    submitted BEFORE a small slot of its own k_bin block takes its list position after it, whatever the hardware does with the
    atomics.  In every tile where the two meet the list reaches k_sort_tiles out of order by construction; here such tiles with 2 to
    64 pairs (the register network) are counted.  Its early steps change nothing on a list that arrives sorted."""
    scene, _ = F.big_slots()
    p = F.plan(scene)
    per_block = 4 * p.tpw
    tri, tile = p.pairs[:, 0], p.pairs[:, 1]
    in_registers = (p.lo >= 2) & (p.hi <= 64)
    assert all(F.sort_path(int(n)) == "registers" for n in (p.lo[in_registers].min(), p.hi[in_registers].max()))
    out_of_order = set()
    for t in np.unique(tile[p.cls[tri] >= 2]):
        if in_registers[t]:
            here = tri[tile == t]
            big, small = here[p.cls[here] >= 2], here[p.cls[here] == 1]
            if any(((small > b) & (small // per_block == b // per_block)).any() for b in big):
                out_of_order.add(int(t))
    assert len(out_of_order) >= 32, len(out_of_order)


def _tiling_cases():
    return [dict(tiles_x=x, tiles_y=y) for x, y in F.TILING_LADDER] + [dict(pixels=F.TILING_ODD_PIXELS)]


@pytest.mark.parametrize("kw", _tiling_cases(), ids=lambda kw: "x".join(str(v) for v in kw.values()).replace(", ", "x"))
def test_tiling_ladder(kw):
    scene, counts = F.tiling_ladder(**kw)
    p = F.plan(scene)
    n_tiles = p.tiles_x * p.tiles_y
    assert p.exact and np.array_equal(p.lo, counts) and counts.min() >= 1, "a pair in every tile"
    stairs = F.tiling_stair_tiles(n_tiles)
    assert 0 in stairs and n_tiles - 1 in stairs and all(counts[t] == 38 for t in stairs) and (counts > 1).sum() == len(stairs)
    for seam in range(256, n_tiles, 256):
        assert seam - 1 in stairs and seam in stairs
    if "pixels" in kw:
        assert scene.width % 16 and scene.height % 16
    c, d, st = render_oracle(scene)
    assert st["fragments_written"] == st["fragments_tested"] == int(p.pixels.sum()) == 3 * int(counts.sum())
    # every tile's marker is in the frame
    assert all((c[ty * 16 + 1, tx * 16 + 1, :3] != 0).any() for ty in range(p.tiles_y) for tx in range(p.tiles_x))


def test_tiling_ladder_sizes():
    sizes = {x * y for x, y in F.TILING_LADDER}
    assert {1, 255, 256, 257, 289, 513} <= sizes
    assert any(x == 17 for x, _ in F.TILING_LADDER) and any(y == 17 for _, y in F.TILING_LADDER) and (1, 33) in F.TILING_LADDER and (257, 1) in F.TILING_LADDER


def test_staircase_scenes_write_every_fragment(ladder):
    scene, counts, p, (c, d, st) = ladder
    assert st["fragments_written"] == st["fragments_tested"] == int(p.pixels.sum()) == 10 * int(counts.sum())
    assert st["triangles_setup"] == p.n_tris


# ---- sensitivity: what a wrong front end does to a tile's list, done to the submission order of a reduced sort ladder ----
@pytest.fixture(scope="module")
def reduced():
    """Three tiles: the list of 2049, one of 65, one empty."""
    scene, counts = F.sort_ladder(counts_per_tile=[2049, 65, 0], tiles_x=3, tiles_y=1, name="sort_ladder_reduced")
    p = F.plan(scene)
    mine = np.nonzero(p.box[:, 0] == 0)[0]              # the 2049 list, in submission order
    assert len(mine) == 2049
    return scene, mine, render_oracle(scene)


def _adjacent(mine, k):
    return int(mine[k]), int(mine[k + 1])


@pytest.mark.parametrize("where,k", [("early", 5), ("middle", 1024), ("late", 2046)])
def test_a_swap_in_the_long_list_shows_in_the_counters(reduced, where, k):
    scene, mine, (c, d, st) = reduced
    assert st["fragments_written"] == st["fragments_tested"]
    c2, d2, st2 = render_oracle(F.with_edit(scene, swap=_adjacent(mine, k)))
    assert st2["fragments_tested"] == st["fragments_tested"]
    assert st2["fragments_written"] == st["fragments_written"] - 10, "the overtaken triangle fails the depth test on all its pixels"
    if where == "early":
        # ... and that is the reason the staircase exists: 2000 translucent layers later the colours no longer know
        assert int(ulp_distance(c2, c).max()) <= 1
        assert np.array_equal(d2.view(np.uint32), d.view(np.uint32))


def test_a_lost_pair_shows_in_the_counters(reduced):
    scene, mine, (c, d, st) = reduced
    c2, d2, st2 = render_oracle(F.with_edit(scene, drop=int(mine[7])))
    assert st2["fragments_tested"] == st["fragments_tested"] - 10
    assert int(ulp_distance(c2, c).max()) <= 1, "the colours alone would not have seen it"


def test_a_duplicated_pair_shows_in_the_counters(reduced):
    scene, mine, (c, d, st) = reduced
    c2, d2, st2 = render_oracle(F.with_edit(scene, twice=int(mine[7])))
    assert st2["fragments_tested"] == st["fragments_tested"] + 10
    assert st2["fragments_written"] == st["fragments_written"], "the copy fails Less against itself"
