"""The shading edge families of tests/shade_edge_scenes.py on the CPU: the oracle against an independent numpy float32 restatement
of Interpolate + fs_dust2 / fs_phong4, and proof that the families put shaded fragments on both sides of every `safe` term of
shade_dust2_fast / shade_phong4_fast and of the per-draw predicates (non-vacuity).  Everything here is a statement about the
INPUTS, computed from the restatement, never from the kernel.  No GPU."""
import copy
import functools

import numpy as np
import pytest

import shade_edge_scenes as S
from softwarerenderer_amd.rasterizer import BlendMode, CullMode, DepthTest

N_SIDE = 16          # shaded fragments a family set must put on each side of a guard


def _pure(families=None):
    return [p for p, _ in S.pairs(0, families) if not any(tag in p.name for tag in S.NOT_RESTATED)]


@functools.lru_cache(maxsize=None)
def _fragments(families=None):
    """[(scene, draw index, triangle index, rect, Shaded)] of the pure scenes (the diluted ones hold the same draws)."""
    return [(s, j, i, r, sh) for s in _pure(families) for j, i, _, r, sh in S.shaded_fragments(s)]


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


def _single(scene, draw, tri_index):
    """One triangle of `draw` with its own program, uniforms and texture, under BlendMode.Multiply over a frame cleared to
    (1, 1, 1, 1) with depth test Always: a written pixel holds src * 1 = the fragment program's value word for word (NaN and -0
    included), an unwritten one (alpha not > 0) keeps the clear values, and no row ends early (only BlendMode.None does that)."""
    d = copy.copy(draw)
    d.indices = draw.indices[3 * tri_index:3 * tri_index + 3].copy()
    d.blend, d.depth_test, d.cull = BlendMode.Multiply, DepthTest.Always, CullMode.None_
    return S.scenes.Scene("single", scene.width, scene.height, [d], textures=scene.textures, bilinear=scene.bilinear,
                          clear_color=(1.0, 1.0, 1.0, 1.0))


@pytest.mark.parametrize("fam", [f for f in S.FAMILIES])
def test_oracle_equals_the_float32_restatement(oracle, fam):
    """Every triangle of every pure scene, one at a time: depth words and colour words of the oracle (C) against Shaded (numpy).
    The bar is 0 ULP for depth and colour: both sides are IEEE float32 on the same CPU, every operation of Interpolate and of the
    two programs is a single correctly rounded + - * / sqrt in a stated order, and the oracle is compiled without contraction, so
    there is no rounding left to differ in.  Where a word is NaN on both sides only NaN-ness is compared (payload and sign of a
    NaN are not part of the reference's semantics)."""
    n = written = 0
    for s in _pure((fam,)):
        o = oracle(s.width, s.height)
        by_tri = {}
        for j, i, t, r, sh in S.shaded_fragments(s):
            by_tri.setdefault((j, i), []).append((r, sh))
        for j, d in enumerate(s.draws):
            for i in range(d.indices.size // 3):
                want_c = np.ones((s.height, s.width, 4), np.float32)
                want_d = np.full((s.height, s.width), S.E.FLOAT_MIN, np.float32)
                for (sX, eX, sY, eY), sh in by_tri.get((j, i), []):
                    with np.errstate(all="ignore"):
                        wr = sh.color[:, 3] > 0
                    m = sh.inside.copy()
                    m[sh.inside] = wr
                    want_c[sY:eY + 1, sX:eX + 1][m] = sh.color[wr]
                    want_d[sY:eY + 1, sX:eX + 1][m] = sh.depth[sh.inside][wr]
                    written += int(wr.sum())
                o.reset_stats()
                got_c, got_d = o.render_scene(_single(s, d, i))
                what = f"{s.name} draw {j} triangle {i}"
                for name, got, want in (("depth", got_d, want_d), ("colour", got_c, want_c)):
                    nan = np.isnan(want)
                    assert np.array_equal(nan, np.isnan(got)), f"{what}: NaN {name} words differ"
                    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
                    assert not bad.any(), (f"{what}: {int(bad.sum())} {name} words differ; first {got[bad][0]!r} "
                                           f"against the restatement's {want[bad][0]!r}")
                n += 1
    print(f"{fam}: {n} triangles, {written} written fragments, oracle == restatement word for word")
    assert written >= 100


def _count_sides(program, families=None):
    """Per `safe` term: [fragments where it holds, fragments where it fails, (triangle, tile) groups where it ALONE fails: some
    fragment of the group fails it, every fragment of the group passes every other term, and the per-draw predicate holds].  The
    kernel verifies per chunk of up to 64 consecutive fragments of a tile; a cell triangle is alone in its tile, so such a group
    is a chunk that a kernel without the term would not shade again."""
    sides = {}
    for s, j, i, r, sh in _fragments(families):
        d = s.draws[j]
        if d.program != program:
            continue
        tex = s.textures[d.texture] if d.texture is not None else None
        applies = all(S.draw_applies(d, tex, s.bilinear).values())
        terms = sh.terms(program)
        allok = np.logical_and.reduce(list(terms.values()))
        for name, ok in terms.items():
            others = np.logical_and.reduce([v for k, v in terms.items() if k != name])
            c = sides.setdefault(name, [0, 0, 0])
            c[0] += int(ok.sum()); c[1] += int((~ok).sum()); c[2] += int(applies and (~ok).any() and others.all())
        c = sides.setdefault("every term (safe)", [0, 0, 0])
        c[0] += int(allok.sum()) if applies else 0; c[1] += int((~allok).sum())
    return sides


@pytest.mark.parametrize("program", [S.DUST2, S.PHONG], ids=["dust2", "phong4"])
def test_every_safe_term_has_fragments_on_both_sides(program):
    """Both sides of every `safe` term hold at least N_SIDE shaded fragments of the pure scenes, and for every term at least one
    whole (triangle, tile) group fails that term ALONE: a kernel that dropped the term would keep its speculative values there.

    `len_sq <= 1e12` needs a construction of its own, and this says why.  With three positive clip.w the normalised weights wa, wb, wc are >= 0
    and sum to 1 within rounding, so |N| <= max |n_i| <= 1 (+ rounding) and len_sq stays below 2.  Only a negative clip.w that
    the near clipper keeps (S1 "cancel") makes ra, rb, rc cancel, and then len_sq grows like 1 / inv_sum^2: it passes 1e12 where
    |inv_sum| is below about 1e-6 of the weights.  Those fragments exist (counted below), and some of them fail no other term."""
    sides = _count_sides(program)
    for name, (ok, bad, alone) in sides.items():
        print(f"{program.name}: {name}: holds {ok}, fails {bad}, fails alone in {alone} groups")
    for name, (ok, bad, alone) in sides.items():
        assert ok >= N_SIDE and bad >= N_SIDE, (name, ok, bad)
        if name != "every term (safe)":
            assert alone >= 1, f"{name}: no group fails this term alone"


def test_per_draw_predicates_have_draws_on_both_sides():
    """dust2_fast_applies: texture bound / fog range in [2^-40, 2^40] (fog_r1 != 0) / light direction finite; phong4_fast_applies:
    texture bound.  Each condition holds for, and ALONE fails for, draws with at least N_SIDE shaded fragments."""
    sides = {}
    for s, j, i, r, sh in _fragments():
        d = s.draws[j]
        tex = s.textures[d.texture] if d.texture is not None else None
        t = S.draw_applies(d, tex, s.bilinear)
        n = sh.wf.shape[1]
        for name, ok in t.items():
            others = all(v for k, v in t.items() if k != name)
            c = sides.setdefault((d.program.name, name), [0, 0])
            c[0] += n if ok else 0
            c[1] += n if (not ok and others) else 0
    for key, (ok, alone) in sides.items():
        print(f"{key}: holds for {ok} fragments, alone fails for {alone}")
        assert ok >= N_SIDE and alone >= N_SIDE, key
    assert len(sides) == 4


def test_the_exact_cases_occur():
    """The inputs named "exactly" occur, as exact float32 statements: a weight of 0 (sample on an edge), two weights of 0 (sample on
    a vertex), inv_sum == 0, texel index == texture width and == height, fog_end - clip_z == 0, fog quotient exactly 0 and
    exactly 1 and on either side of both, camera on the fragment (Vd == 0), light on the fragment (dist == 0), Ln + Vn == 0, a
    zero component of a light vector on a whole wall."""
    seen = dict.fromkeys(["weight 0", "two weights 0", "inv_sum 0", "tx == tex_w", "ty == tex_h", "fog_num 0", "fog_q 1", "fog_q < 0",
                          "fog_q > 1", "0 < fog_q < 1", "Vd 0", "dist 0", "Ln + Vn 0", "Ld.z 0 on a whole triangle", "|N|^2 0",
                          "|N|^2 > 1e12 finite", "|N|^2 NaN", "alpha <= 0", "alpha NaN", "subnormal colour"], 0)
    for s, j, i, r, sh in _fragments():
        d = s.draws[j]
        with np.errstate(all="ignore"):
            zeros = (sh.wf == 0).sum(axis=0)
            seen["weight 0"] += int((zeros == 1).sum())
            seen["two weights 0"] += int((zeros == 2).sum())
            seen["inv_sum 0"] += int((sh.inv_sum == 0).sum())
            seen["|N|^2 0"] += int((sh.len_sq == 0).sum())
            seen["|N|^2 > 1e12 finite"] += int(((sh.len_sq > 1e12) & np.isfinite(sh.len_sq)).sum())
            seen["|N|^2 NaN"] += int(np.isnan(sh.len_sq).sum())
            seen["alpha <= 0"] += int((sh.color[:, 3] <= 0).sum())
            seen["alpha NaN"] += int(np.isnan(sh.color[:, 3]).sum())
            a = np.abs(sh.color[:, :3])
            seen["subnormal colour"] += int(((a > 0) & (a < 2.0 ** -126)).sum())
            if d.texture is not None and not s.bilinear:
                seen["tx == tex_w"] += int((sh.tx == sh.tex_w).sum())
                seen["ty == tex_h"] += int((sh.ty == sh.tex_h).sum())
            if d.program == S.DUST2:
                q = sh.fog_num / sh.fog_den
                seen["fog_num 0"] += int((sh.fog_num == 0).sum())
                seen["fog_q 1"] += int((q == 1).sum())
                seen["fog_q < 0"] += int((q < 0).sum())
                seen["fog_q > 1"] += int((q > 1).sum())
                seen["0 < fog_q < 1"] += int(((q > 0) & (q < 1)).sum())
            else:
                seen["Vd 0"] += int((sh.units[0][0] == 0).sum())
                for l in range(4):
                    ll, v = sh.units[1 + 2 * l]
                    seen["dist 0"] += int((ll == 0).sum())
                    seen["Ld.z 0 on a whole triangle"] += int((v[2] == 0).all())
                    hl, hv = sh.units[2 + 2 * l]
                    seen["Ln + Vn 0"] += int(((hv[0] == 0) & (hv[1] == 0) & (hv[2] == 0)).sum())
    print(seen)
    for name, n in seen.items():
        assert n >= 1, name


def test_s7_tiles_hold_safe_and_unsafe_fragments_of_one_draw():
    """At least 16 tiles of each S7 scene hold both safe and unsafe fragments of the same draw -- and at least 16 single triangles
    do (a triangle's fragments are consecutive in the tile's stream, so they share a chunk)."""
    for s in _pure(("s7",)):
        tiles, tris = {}, {}
        for j, i, t, r, sh in S.shaded_fragments(s):
            safe = np.logical_and.reduce(list(sh.terms(s.draws[j].program).values()))
            key = (j, r[0] // S.TILE, r[2] // S.TILE)
            for dct, k in ((tiles, key), (tris, (j, i))):
                c = dct.setdefault(k, [0, 0])
                c[0] += int(safe.sum()); c[1] += int((~safe).sum())
            assert sh.wf.shape[1] <= 32
        mixed_tiles = sum(1 for a, b in tiles.values() if a and b)
        mixed_tris = sum(1 for a, b in tris.values() if a and b)
        print(f"{s.name}: {mixed_tiles} of {len(tiles)} tiles and {mixed_tris} of {len(tris)} triangles hold safe and unsafe fragments")
        assert mixed_tiles >= 16 and mixed_tris >= 16


def test_pure_scenes_select_the_specialised_kernel_and_diluted_ones_the_generic():
    for pure, diluted in S.pairs(0):
        prog = pure.draws[0].program
        assert S.predicted_kernel(pure) == ("dust2_default" if prog == S.DUST2 else "phong_default"), pure.name
        assert S.predicted_kernel(diluted) == ("generic" if prog == S.DUST2 else "generic_phong"), diluted.name
        assert diluted.draws[:-1] == pure.draws
        assert all(d.depth_test == DepthTest.LessEqual for d in diluted.draws)          # depth_only_grows stays set


def test_s8_crosses_the_representative_cap_behind_three_decoys():
    """S8 as execute_batch sees it: more than 64 distinct materials in one batch, every one a single bit away from the defaults
    in a single field; the first three draws (no vertices / frustum-culled) have the materials of draws 3, 4, 5; repeats of
    materials from before and from after the cap come last."""
    s = S.s8_material_identity(0)
    assert S.predicted_kernel(s) == "dust2_default"
    keys = [S.material_key(d) for d in s.draws]
    order = list(dict.fromkeys(keys))
    assert len(order) > 64 + 6
    assert keys[0] == keys[3] and keys[1] == keys[4] and keys[2] == keys[5]
    assert s.draws[0].vertices.shape[0] == 0 and s.draws[1].frustum_cull and s.draws[2].frustum_cull
    assert not any(d.frustum_cull for d in s.draws[3:])
    tail = [order.index(k) for k in keys[-4:]]
    assert min(tail) < 64 <= max(tail)
    base = np.frombuffer(bytes(S.scenes.default_uniforms()), np.uint32)
    one_bit = 0
    for k in order:
        diff = np.frombuffer(k[4], np.uint32) ^ base
        one_bit += int(np.count_nonzero(diff) == 1 and bin(int(diff[diff != 0][0])).count("1") == 1)
    assert one_bit >= 60          # (the light-direction materials also replace x and y by signed zeros)
