"""The edge families of tests/edge_scenes.py on the CPU: the oracle against an independent float32 restatement of setup and the
tile chain, and proof that each family really reaches the bound it is meant to test (non-vacuity).  No GPU."""
import copy

import numpy as np
import pytest

import edge_scenes as E
from softwarerenderer_amd.rasterizer import BlendMode, CullMode, DepthTest, Program

K = 5            # the least number of pairs / rows a family must put at its bound


def _single(scene, draw, tri_index):
    """A scene of one triangle of `draw`: FlatColor (alpha 1), blend None, depth Always, cull None, cleared to alpha 0, so the
    frame's alpha is the coverage and its depth words are the fragments' depths."""
    d = copy.copy(draw)
    d.indices = draw.indices[3 * tri_index:3 * tri_index + 3].copy()
    d.vertices = draw.vertices.copy()
    d.vertices["color"][:, 3] = 1.0
    d.program, d.blend, d.depth_test, d.cull = Program.FlatColor, BlendMode.None_, DepthTest.Always, CullMode.None_
    d.texture = None
    return E.scenes.Scene("single", scene.width, scene.height, [d], clear_color=(0.0, 0.0, 0.0, 0.0))


def _oracle_frame(o, scene):
    o.reset_stats()
    c, d = o.render_scene(scene)
    return c[..., 3] == 1.0, d, o.stats()


@pytest.fixture(scope="module")
def oracle():
    from oracle import binding
    binding.build()
    binding.load()
    made = {}
    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = binding.OracleRenderer(w, h)
        return made[(w, h)]
    yield get
    for o in made.values():
        o.close()


def _family_triangles(fam, seed=0, draws=slice(0, 1)):
    for s in E.FAMILIES[fam](seed):
        for d in s.draws[draws]:
            for i, t in enumerate(E.triangles(d, s.width, s.height)):
                yield s, d, i, t


@pytest.mark.parametrize("fam", ["f1", "f2", "f3", "f4", "f5"])
def test_oracle_equals_the_float32_restatement(oracle, fam):
    """Coverage and depth words of every triangle of the family, one at a time: the oracle (C) against Tri (numpy float32).
    Where the depth is NaN only NaN-ness is compared (x86 and numpy agree on the bits, but that is not what is tested)."""
    n = covered = 0
    for s, d, i, t in _family_triangles(fam, draws=slice(0, 1)):
        o = oracle(s.width, s.height)
        cov, dep, st = _oracle_frame(o, _single(s, d, i))
        with np.errstate(all="ignore"):
            rcov, rdep = t.frame() if t.ok else (np.zeros_like(cov), np.full_like(dep, E.FLOAT_MIN))
        assert np.array_equal(cov, rcov), f"{s.name} triangle {i}: coverage differs ({int((cov != rcov).sum())} pixels)"
        assert st["fragments_tested"] == int(rcov.sum())
        nan = np.isnan(rdep)
        assert np.array_equal(nan, np.isnan(dep)), f"{s.name} triangle {i}: NaN depths differ"
        assert np.array_equal(dep.view(np.uint32)[~nan], rdep.view(np.uint32)[~nan]), f"{s.name} triangle {i}: depth words differ"
        n += 1
        covered += int(rcov.any())
    print(f"{fam}: {n} triangles, {covered} cover pixels")
    assert covered >= K


def test_f1_reaches_the_binning_margin():
    """F1: pairs that pair_may_cover with margin 0 would drop although the chain covers a sample of bbox /\\ tile."""
    pairs = at_bound = kept = 0
    for s, d, i, t in _family_triangles("f1"):
        for tx, ty, r in t.tiles():
            pairs += 1
            inside, _, _ = t.cover(r)
            if inside.any():
                assert t.pair_may_cover(r), f"{s.name} triangle {i} tile {(tx, ty)}: the margin of record drops a covered pair"
                at_bound += not t.pair_may_cover(r, margin=0.0)
            else:
                kept += t.pair_may_cover(r)
    print(f"f1: {pairs} pairs, {at_bound} covered pairs that margin 0 drops, {kept} empty pairs kept")
    assert at_bound >= K


def _triangles_and_stored(oracle, s):
    """(draw, triangle, depth buffer before that triangle) of every triangle of s, the depth taken from the oracle."""
    o = oracle(s.width, s.height)
    for j, d in enumerate(s.draws):
        for i, t in enumerate(E.triangles(d, s.width, s.height)):
            part = copy.copy(d)
            part.indices = d.indices[:3 * i]
            _, stored = o.render_scene(E.scenes.Scene("prefix", s.width, s.height, s.draws[:j] + [part]))
            yield d, t, stored


def _hiz_pairs(oracle, fams):
    """Per pair with the whole tile written before: (family name, U at margin 0, U of record, U before the underflow term,
    largest fragment depth, tile minimum of the stored depth, whether some fragment passes the draw's test)."""
    for s in fams:
        for d, t, stored in _triangles_and_stored(oracle, s):
            for tx, ty, r in t.tiles():
                x0, y0 = tx * E.TILE, ty * E.TILE
                tile = stored[y0:y0 + E.TILE, x0:x0 + E.TILE]
                zmin = tile.min()
                if not zmin > E.FLOAT_MIN:
                    continue
                with np.errstate(all="ignore"):
                    inside, depth, _ = t.cover(r)
                if not inside.any():
                    continue
                sX, eX, sY, eY = r
                frag = depth[inside]
                old = stored[sY:eY + 1, sX:eX + 1][inside]
                passes = (frag >= old).any() if d.depth_test == DepthTest.LessEqual else (frag > old).any()
                yield (s.name, t.hiz_bound(r, 0.0, False), t.hiz_bound(r), t.hiz_bound(r, 64.0, False), frag.max(), zmin, passes)


def test_f2_reaches_the_hiz_bound_and_the_bound_of_record_holds(oracle):
    """F2: pairs where the zero-margin bound is below the largest fragment depth and at or below the tile's stored minimum (a
    margin-0 build would drop them), per case; the bound of record is never below a fragment depth.  The bound before the
    underflow term (k_cover before this test existed) is shown to fail on the huge-triangle case: it would drop pairs of which
    a fragment passes the depth test."""
    counts = {}
    for name, u0, u, u_old, fmax, zmin, passes in _hiz_pairs(oracle, E.f2_hiz_near_ties(0)):
        case = name.split("_")[2]
        case = "huge" if case.startswith("huge") else "S" if case.startswith("S1e") else "plane"
        c = counts.setdefault(case, [0, 0, 0, 0])
        c[0] += 1
        c[1] += bool(u0 < fmax and u0 <= zmin)
        c[2] += bool(u_old < fmax)
        c[3] += bool(u_old < zmin and passes)
        assert u >= fmax, f"{name}: the hi-Z bound {u!r} is below a fragment depth {fmax!r}"
    for case, (n, at0, old_below, old_drop) in sorted(counts.items()):
        print(f"f2 {case}: {n} pairs over written tiles, {at0} at the margin-0 bound; old bound below a fragment {old_below}, "
              f"old bound drops a passing pair {old_drop}")
    assert counts["plane"][1] >= K and counts["huge"][1] >= K
    assert counts["huge"][3] >= 1          # the finding: without the underflow term the bound drops fragments that pass
    assert counts["S"][0] >= K


def test_f3_populates_every_magnitude_band():
    bands = {"<1e15": 0, "1e15..1e30": 0, ">=1e30": 0, "chain non-finite": 0, "slow walk": 0}
    for s, d, i, t in _family_triangles("f3", draws=slice(0, 1)):
        if not t.ok:
            continue
        with np.errstate(all="ignore"):
            tiles = [(r, *t.cover(r)) for _, _, r in t.tiles()]
            if not any(inside.any() for _, inside, _, _ in tiles):
                continue
            big = float(max(np.abs(t.sx).max(), np.abs(t.sy).max()))
            bands["<1e15" if big < 1e15 else "1e15..1e30" if big < 1e30 else ">=1e30"] += 1
            bands["chain non-finite"] += any(inside.any() and not np.isfinite(w).all() for _, inside, _, w in tiles)
            bands["slow walk"] += any(inside.any() and not t.fast_walk(r) for r, inside, _, _ in tiles)
    print("f3 visible triangles per band:", bands)
    assert all(v >= 2 for v in bands.values()), bands


def test_f4_every_row_of_a_triangle_is_one_run():
    """F4 cannot reach its bound, and this says why.  The run select (pairs flagged SWR_INFO_SIMPLE) assumes a row's covered
    samples are one run.  Along a row each edge value is stepped by its constant a (:527-529), so it is monotone (fl(w + a) >= w
    for a > 0), +-Inf stays put and NaN, once there, stays.  The a of a triangle cannot all have one sign (a01 + a12 + a20 = 0,
    and the smallest is an exact difference of nearby floats), and a zero a makes the other two opposite.  So "all >= 0" and
    "all <= 0" are intervals [max of the rising crossings, min of the falling] and [max falling, min rising]; both non-empty
    and apart needs a falling edge that is 0 at two samples, i.e. a = 0.  Every row is one run and SWR_INFO_SIMPLE is never
    wrong for triangles: the needles of F4 (and 17k random slivers at 1..1e8 px, 1e-8..1 px wide, in a one-off search) have
    no other row.  The test keeps the invariant: it fails the day a row of a triangle is not one run."""
    rows = multi = 0
    for s, d, i, t in _family_triangles("f4", draws=slice(0, 1)):
        for _, _, r in t.tiles():
            inside, _, _ = t.cover(r)
            for row in inside:
                x = row.astype(np.int8)
                rows += bool(x.any())
                multi += int(np.count_nonzero(np.diff(x) == 1) + x[0] > 1)
    print(f"f4: {rows} covered rows of needles, {multi} that are not one run")
    assert rows >= 200
    assert multi == 0


def test_f5_puts_operands_on_both_sides_of_every_guard():
    """Interpolate's operands of every covered fragment of F5 (float64 is enough here: the counts only need each side of each
    guard populated, far from rounding distance): clip.w and inv_sum against the division cores' [2^-40, 2^40] and the
    reciprocal's 2^83, the world normal's squared length against the sqrt core's [2^-40, 2^40] and the 1e-6 threshold."""
    sides = {}
    def note(name, lo_side, in_side, hi_side=None):
        c = sides.setdefault(name, [0, 0, 0])
        c[0] += int(lo_side); c[1] += int(in_side); c[2] += int(hi_side or 0)
    for s in E.f5_guard_scale(0):
        d = s.draws[0]
        nrm = d.vertices["normal"].astype(np.float64)
        nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
        for j, t in enumerate(E.triangles(d, s.width, s.height)):
            if not t.ok:
                continue
            cw = t.clip_w.astype(np.float64)
            wn = nrm[[3 * j + 2, 3 * j + 1, 3 * j]]                 # outputs = { v2, v1, v0 }
            for _, _, r in t.tiles():
                with np.errstate(all="ignore"):
                    inside, _, w = t.cover(r)
                if not inside.any():
                    continue
                wf = (w * t.inv_area).astype(np.float64)[:, inside]
                ra = wf / cw[:, None]
                inv_sum = ra.sum(axis=0)
                aw = np.abs(cw)
                note("clip.w vs 2^+-40", (aw < 2 ** -40).any(), ((aw >= 2 ** -40) & (aw <= 2 ** 40)).any(), (aw > 2 ** 40).any())
                ai = np.abs(inv_sum)
                note("inv_sum vs 2^-40, 2^83", (ai < 2 ** -40).any(), ((ai >= 2 ** -40) & (ai <= 2 ** 83)).any(), (ai > 2 ** 83).any())
                note("clip.w vs 2^+-126", (aw < 2 ** -126).any(), ((aw >= 2 ** -126) & (aw < 2 ** 126)).any(), (aw >= 2 ** 126).any())
                wb = ra / inv_sum
                v = (wb[:, :, None] * wn[:, None, :]).sum(axis=0)
                ls = (v * v).sum(axis=1)
                note("|N|^2 vs 1e-6", (ls <= 1e-6).any(), (ls > 1e-6).any())
                note("|N|^2 vs 2^-40", ((ls > 0) & (ls < 2 ** -40)).any(), ((ls >= 2 ** -40) & (ls <= 1e-6)).any())
    print("f5 tiles on each side (below, inside, above):", sides)
    for name, (lo, mid, hi) in sides.items():
        assert lo > 0 and mid > 0, name
        if "clip.w" in name or "inv_sum" in name:
            assert hi > 0, name
