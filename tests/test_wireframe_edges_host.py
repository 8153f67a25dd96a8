"""The claims tests/test_gpu_wireframe_edges.py rests on, on the CPU: that the numpy-float32 restatement of DrawLine in
tests/wireframe_edge_scenes.py IS the oracle's wireframe frame for every scene (depth words, the written pixels, the three
fragment counters) -- without which no count below says anything about what the GPU is compared with --, and that every family
W1-W9 reaches what it is for, counted with the restatement.  Each test prints the figures it asserts on
(profiles/r11_wireframe_tests.md records them)."""
import numpy as np
import pytest

import front_end_scenes as F
import wireframe_edge_scenes as Wf
from softwarerenderer_amd.rasterizer import BlendMode, DepthTest, Program
from util import render_oracle

F32 = np.float32
QUARTER = F32(0.25)
BELOW_QUARTER = float(np.nextafter(QUARTER, F32(0.0)))          # dist_sq <= this  <=>  dist_sq < 0.25f
SCENES = Wf.all_scenes()


@pytest.fixture(scope="module")
def restated():
    """name -> Restated, computed once and never changed."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Wf.restate(SCENES[name])
        return cache[name]
    return get


def _lit_differs(scene, lines, **kw):
    a, b = Wf.restate(scene, lines=lines), Wf.restate(scene, lines=lines, **kw)
    return int(((a.hits > 0) != (b.hits > 0)).sum()), a, b


# ------------------------------------------------------------------------------------------------ the restatement is the oracle
@pytest.mark.parametrize("name", list(SCENES))
def test_restatement_is_the_oracles_wireframe_frame(restated, name):
    scene, r = SCENES[name], restated(name)
    c, d, st = render_oracle(scene, debug_mode=1)
    bad = d.view(np.uint32) != r.depth.view(np.uint32)
    assert not bad.any(), f"{name}: {int(bad.sum())} depth words differ, first at (y, x) = {tuple(np.argwhere(bad)[0])}"
    for k, v in r.counters().items():
        assert st[k] == v, (name, k, st[k], v)
    assert st["triangles_setup"] == 0, "the oracle counts filled triangles only"
    changed = (d != Wf.FLOAT_MIN) | (c != np.asarray(Wf.CLEAR, F32)).any(axis=2)
    assert not (changed & (r.written == 0)).any(), f"{name}: the oracle wrote a pixel the restatement does not light"
    if all(dr.depth_test != DepthTest.Disabled for dr in scene.draws):
        assert np.array_equal(changed, r.written > 0), f"{name}: written pixels differ"


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_keeps_within_one_batch(name):
    """What the GPU tests rely on (record_draw, csrc/swr_flush.h): built-in programs of one kernel class, at most 65535 vertices per
    draw, vertices + 4 x triangles of the frame far below 2^26; and frames of at most 256 x 256."""
    s = SCENES[name]
    assert s.width <= 256 and s.height <= 256
    assert all(d.vertices.shape[0] <= 65535 and d.indices.size % 3 == 0 for d in s.draws)
    assert all(d.program in (Program.FlatColor, Program.Gouraud, Program.Dust2LambertFog) for d in s.draws)
    assert sum(d.vertices.shape[0] + 4 * (d.indices.size // 3) for d in s.draws) < 1 << 16


def test_the_scalars_are_dotnets():
    nan = F32(np.nan)
    assert [Wf.f2i(v) for v in (nan, 3e9, -3e9, -0.9, 0.9, -1.0, 249.99998)] == [0, 2 ** 31 - 1, -2 ** 31, 0, 0, -1, 249]
    assert np.isnan(Wf.mathf_min(F32(1), nan)) and np.isnan(Wf.mathf_min(nan, F32(1))) and np.isnan(Wf.mathf_max(F32(0), nan))
    assert np.signbit(Wf.mathf_min(F32(0.0), F32(-0.0))) and not np.signbit(Wf.mathf_max(F32(0.0), F32(-0.0)))
    assert not np.signbit(Wf.mathf_max(F32(-0.0), F32(0.0)))
    # fmaf: one rounding -- 1 + 2^-24 + 2^-48 rounds up where the two-step product-then-sum rounds to even
    a = F32(1.0 + 2.0 ** -12)
    assert Wf.fma32(a, a, F32(-1.0))[()] == F32(2.0 ** -11 + 2.0 ** -24) and F32(F32(a * a) - F32(1.0)) == F32(2.0 ** -11)
    assert Wf.exact_distance_sq((10.0, 6.0), (16.0, 14.0), 10, 6) == Wf.Fraction(1, 100)


# ------------------------------------------------------------------------------------------------ W1
def _w1_counts(segments):
    n_exact = n_in = n_out = n_flip = n_equal = 0
    flips = []
    for name, p0, p1 in segments:
        x0, x1, y0, y1 = Wf.line_bbox(p0, p1, 64, 64)
        ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        lit, t, dist = Wf.line_test(p0, p1, xs, ys)
        lit_f, _, _ = Wf.line_test(p0, p1, xs, ys, fused=True)
        for (i, j) in np.ndindex(xs.shape):
            if Wf.exact_distance_sq(p0, p1, int(xs[i, j]), int(ys[i, j])) == Wf.Fraction(1, 4):
                n_exact += 1
                n_in += bool(lit[i, j]); n_out += not lit[i, j]
                n_equal += bool(dist[i, j] == QUARTER)
                if lit[i, j] != lit_f[i, j]:
                    n_flip += 1
                    flips.append(name)
    return n_exact, n_in, n_out, n_flip, n_equal, flips


def test_w1_centres_at_exactly_half_a_pixel_fall_on_both_sides():
    n_exact, n_in, n_out, n_flip, n_equal, flips = _w1_counts(Wf.w1_segments()[:18])
    print(f"W1: {n_exact} centres at exactly 0.5 px: {n_in} inside, {n_out} outside, {n_equal} with dist_sq == 0.25f, "
          f"{n_flip} change under fused=True {flips}")
    assert n_exact >= 40 and n_in >= 5 and n_out >= 5 and n_flip >= 1
    assert (n_exact, n_in, n_out) == (60, 49, 11) and flips == ["w1_5_12_at_10.5_6"], "the counts these segments were chosen for"
    assert n_equal >= 5, "`dist_sq < 0.25f` must change a pixel"


def test_w1_far_end_points_round_the_chain():
    n_exact, n_in, n_out, n_flip, n_equal, flips = _w1_counts(Wf.w1_segments()[18:])
    print(f"W1 from 1e3 px: {n_exact} centres at exactly 0.5 px: {n_in} inside, {n_out} outside, {n_equal} with dist_sq == 0.25f, "
          f"{n_flip} change under fused=True {flips}")
    assert n_exact >= 20 and n_in >= 5 and n_out >= 5
    for name, p0, p1 in Wf.w1_segments()[18:]:
        assert max(abs(v) for v in (*p0, *p1)) >= 800.0


def test_w1_the_ties_show_in_the_frames(restated):
    """In the scenes themselves: under `<`, and under fusing, lit pixels change that no other edge of the triangle lights."""
    strict = fused = 0
    for s in Wf.family("w1"):
        r = restated(s.name)
        strict += _lit_differs(s, r.lines, threshold=BELOW_QUARTER)[0]
        fused += _lit_differs(s, r.lines, fused=True)[0]
    print(f"W1 scenes: {strict} lit pixels change under dist_sq < 0.25f, {fused} under fused=True")
    assert strict >= 5 and fused >= 1, "as many as the ties must have on each side of the comparison; one under fusing"


def test_fusing_the_numerator_alone_shows_in_depth_words(restated):
    """On W1's half-pixel lattice px * dx and py * dy are exact, so fmaf(px, dx, py * dy) is the unfused sum: a fused numerator
    moves no pixel there.  Where the coordinates carry more bits (W3's 1/64 fractions on steep segments, W4's 1e6, the clipper's
    vertices of W7) it moves t by an ULP, and with it the depth word."""
    changed = []
    for s in SCENES.values():
        r = restated(s.name)
        b = Wf.restate(s, lines=r.lines, fused="numerator")
        n = int((b.depth.view(np.uint32) != r.depth.view(np.uint32)).sum())
        if n or ((b.hits > 0) != (r.hits > 0)).any():
            changed.append((s.name, n))
    print(f"fused numerator alone: depth words change in {changed}")
    assert len(changed) >= 3 and not any(name.startswith("wire_w1") for name, _ in changed)


# ------------------------------------------------------------------------------------------------ W2
def test_w2_truncation_at_the_restatements_functions():
    """The tolerance-free discriminators that no vertex can reach (see the scenes' docstring): x = -1e-9 and x = -0.0."""
    W, H = Wf.W2_SIZE
    for x in (-1e-9, -0.0):
        p0, p1 = (F32(x), F32(20.5)), (F32(x), F32(60.5))
        assert Wf.line_bbox(p0, p1, W, H) == (0, 0, 20, 60)
        ys = np.arange(21, 60)
        lit, _, dist = Wf.line_test(p0, p1, np.zeros_like(ys), ys)
        assert lit.all() and (dist == QUARTER).all(), "column 0 is at exactly 0.5 px: lit"
    b = Wf.line_bbox((F32(-1e-9), F32(20.5)), (F32(-1e-9), F32(60.5)), W, H, floor_bbox=True)
    assert b[0] > b[1], "a floor skips the line"
    b = Wf.line_bbox((F32(30.5), F32(-1e-9)), (F32(200.5), F32(-1e-9)), W, H, floor_bbox=True)
    assert b[2] > b[3]


def test_w2_what_each_scene_is_for(restated):
    W, H = Wf.W2_SIZE
    assert W % 16 and H % 16
    r = {s.name[len("wire_w2_"):]: restated(s.name) for s in Wf.family("w2")}
    first = lambda k: (r[k].lines[0], r[k].boxes[0])
    ln, box = first("x_just_negative")
    assert -2.0 ** -24 * W == ln.p0[0] == ln.p1[0] and box[:2] == (0, 0), "the largest negative x there is; truncated to column 0"
    assert not (r["x_just_negative"].frags["line"] == 0).any(), "... and half a pixel plus 1.5e-5 from its centres"
    f, ln = r["x_just_negative"].frags, r["x_just_negative"].lines[2]
    assert ln.p0[0] < -256 and ln.p1[0] == -2.0 ** -24 * W and F32(ln.p0[0] + F32(ln.p1[0] - ln.p0[0])) == 0
    assert [(int(x), int(y)) for x, y in zip(f["x"][f["line"] == 2], f["y"][f["line"] == 2])] == [(0, 20)], "the cap of the edge from afar"
    ln, box = first("y_just_negative")
    assert -2.0 ** -23 * H == ln.p0[1] == ln.p1[1] and box[2:] == (0, 0)
    f = r["y_just_negative"].frags
    assert [(int(x), int(y)) for x, y in zip(f["x"][f["line"] == 2], f["y"][f["line"] == 2])] == [(30, 0)]
    ln, box = first("x_zero")
    assert ln.p0[0] == 0 and not np.signbit(ln.p0[0]) and box[:2] == (0, 0)
    f = r["x_zero"].frags
    assert set(f["y"][(f["line"] == 0) & (f["x"] == 0)].tolist()) >= set(range(21, 60)), "column 0 at exactly 0.5 px: lit"
    ln, box = first("x_125")
    assert ln.p0[0] == 125 and box[:2] == (125, 125)
    assert Wf.exact_distance_sq(ln.p0, ln.p1, 124, 50) == Wf.Fraction(1, 4) and not r["x_125"].lit[30:80, 124].any(), "outside the bbox: dark"
    assert r["x_125"].lit[30:80, 125].all()
    ln, box = first("y_65")
    assert ln.p0[1] == 65 and box[2:] == (65, 65) and not r["y_65"].lit[64, 30:180].any() and r["y_65"].lit[65, 30:180].all()
    for k, size, axis in (("x_W", W, 0), ("y_H", H, 1)):
        lo = 2 * axis
        ln, box = first(k + "m1_below")
        assert size - 1.01 < ln.p0[axis] < size - 1 and box[lo + 1] == size - 2, "just below size - 1: the cast gives size - 2"
        ln, box = first(k + "m1")
        assert size - 1 <= ln.p0[axis] < size - 0.99 and box[lo:lo + 2] == (size - 1, size - 1)
        ln, box = first(k + "mhalf")
        assert size - 0.5 <= ln.p0[axis] < size - 0.49 and box[lo:lo + 2] == (size - 1, size - 1)
        ln, box = first(k + "m0_below")
        assert size - 0.01 < ln.p0[axis] < size and box[lo:lo + 2] == (size - 1, size - 1)
        assert (r[k + "m0_below"].frags["line"] == 0).sum() >= 60, "the last column / row is lit"
        ln, box = first(k + "m0")
        assert ln.p0[axis] == size and box is None, "min > max: DrawLine returns"
    assert r["beyond"].boxes[:12] == [None] * 12 and all(b is not None for b in r["beyond"].boxes[12:])
    ln, box = first("crossing")
    assert box == (0, W - 1, 0, H - 1) and min(ln.p0) < 0 and ln.p1[0] > W and ln.p1[1] > H
    assert (r["crossing"].frags["line"] == 0).sum() >= 200


def test_w2_a_floor_changes_lit_pixels_and_pairs(restated):
    changed_pairs, changed_lit = [], []
    for s in Wf.family("w2"):
        r = restated(s.name)
        n, _, fl = _lit_differs(s, r.lines, floor_bbox=True)
        if n:
            changed_lit.append((s.name, n))
        if fl.tile_pairs != r.tile_pairs:
            changed_pairs.append((s.name, r.tile_pairs, fl.tile_pairs))
    print(f"W2: floor_bbox=True changes lit pixels in {changed_lit} and tile_pairs in {changed_pairs}")
    assert len(changed_lit) >= 3 and len(changed_pairs) >= 3


# ------------------------------------------------------------------------------------------------ W3
def test_w3_end_caps(restated):
    t0 = t1 = dark = exact0 = exact1 = 0
    for s in Wf.family("w3"):
        r = restated(s.name)
        f = r.frags
        first = np.isin(f["line"], [i for i, ln in enumerate(r.lines) if ln.edge == 0])
        t0 += int((first & (f["t"] == 0)).sum()); t1 += int((first & (f["t"] == 1)).sum())
        for li, (ln, b) in enumerate(zip(r.lines, r.boxes)):
            if ln.edge or b is None:
                continue
            ys, xs = np.mgrid[b[2]:b[3] + 1, b[0]:b[1] + 1]
            lit, t, dist = Wf.line_test(ln.p0, ln.p1, xs, ys)
            dark += int((((t == 0) | (t == 1)) & ~lit).sum())
            exact0 += int((lit & (t == 0) & (dist == 0)).sum()); exact1 += int((lit & (t == 1) & (dist == 0)).sum())
    print(f"W3 first edges: {t0} lit pixels with t clamped to 0, {t1} to 1; {dark} pixels of a bbox with clamped t stay dark; "
          f"{exact0} / {exact1} end points on a pixel centre (distance 0)")
    assert t0 >= 8 and t1 >= 8 and dark >= 8 and exact0 >= 8 and exact1 >= 8


# ------------------------------------------------------------------------------------------------ W4
def test_w4_magnitude_ladder(restated):
    inf_len_t0 = nan_t = lit_by_dropped_nan = 0
    scenes_lit_by_dropped_nan = []
    with np.errstate(all="ignore"):
        for s in Wf.family("w4"):
            r = restated(s.name)
            nan_t += r.t_nan_in_box
            for li, ln in enumerate(r.lines):
                dx, dy = F32(ln.p1[0] - ln.p0[0]), F32(ln.p1[1] - ln.p0[1])
                if np.isposinf(F32(dx * dx + dy * dy)) and np.isfinite([dx, dy]).all():
                    m = r.frags["line"] == li
                    inf_len_t0 += int((m & (r.frags["t"] == 0)).sum())
                    assert (r.frags["t"][m] == 0).all(), "len_sq = +Inf with a finite numerator: only p0's cap"
            n = _lit_differs(s, r.lines, clamp_drops_nan=True)[0]
            lit_by_dropped_nan += n
            if n:
                scenes_lit_by_dropped_nan.append(s.name)
    sizes = sorted({float(max(abs(v) for v in (*ln.p0, *ln.p1))) for s in Wf.family("w4") for ln in restated(s.name).lines[:1]})
    print(f"W4: first edges reach {sizes}; {inf_len_t0} lit pixels with len_sq = +Inf and t = 0; {nan_t} bbox pixels with t NaN; "
          f"a clamp that drops NaN lights {lit_by_dropped_nan} more pixels in {scenes_lit_by_dropped_nan}")
    assert inf_len_t0 >= 4 and nan_t >= 1000 and len(scenes_lit_by_dropped_nan) >= 1
    assert np.isinf(sizes[-1]) and any(9e19 < v < 2e20 for v in sizes) and any(9e36 < v < 2e37 for v in sizes)


# ------------------------------------------------------------------------------------------------ W5
def _w5_by_depth_test():
    return [s for s in Wf.family("w5") if "negative_w" not in s.name]


def test_w5_depth_words(restated):
    for s in _w5_by_depth_test():
        r = restated(s.name)
        dep, den = r.frags["depth"].astype(F32), r.frags["den"].astype(F32)
        tiny = np.finfo(F32).tiny
        n = dict(pos_inf=int(np.isposinf(dep).sum()), negative=int((dep < 0).sum()), huge_pos=int((np.isfinite(dep) & (dep > 1e6)).sum()),
                 huge_neg=int((np.isfinite(dep) & (dep < -1e6)).sum()), subnormal_word=int(((dep != 0) & (np.abs(dep) < tiny)).sum()),
                 neg_inf=int(np.isneginf(dep).sum()), nan=int(np.isnan(dep).sum()),
                 subnormal_den_pos=int(((den > 0) & (den < tiny)).sum()), subnormal_den_neg=int(((den < 0) & (den > -tiny)).sum()),
                 subnormal_den_finite_word=int(((den != 0) & (np.abs(den) < tiny) & np.isfinite(dep)).sum()))
        t = r.frags["t"].astype(F32)
        n["subnormal_t"] = int(((t > 0) & (t < tiny)).sum())
        n["t_underflows_den"] = int(((t > 0) & (t < tiny) & (den == 0) & ~np.signbit(den)).sum())
        print(f"{s.name}: {len(dep)} fragments, {r.counters()['fragments_shaded']} pass; {n}")
        assert n["pos_inf"] >= 3 and n["negative"] >= 50 and n["huge_pos"] >= 3 and n["huge_neg"] >= 3 and n["subnormal_word"] >= 10
        assert n["neg_inf"] >= 1 and n["subnormal_den_pos"] >= 2 and n["subnormal_den_neg"] >= 1 and n["subnormal_den_finite_word"] >= 1
        assert n["subnormal_t"] >= 4 and n["t_underflows_den"] >= 1
        # what (nz + 1) * 0.5 cannot produce (the scenes' docstring): a NaN word needs a NaN, -0.0 or infinite depth operand
        assert n["nan"] == 0
        d = np.array([[ln.d0, ln.d1] for ln in r.lines], F32)
        assert np.isfinite(d).all() and ((d == 0) | (np.abs(d) >= 2.0 ** -25)).all() and not np.signbit(d[d == 0]).any()
    shaded = {s.name: restated(s.name).counters()["fragments_shaded"] for s in _w5_by_depth_test()}
    assert len(set(shaded.values())) >= 6, f"the depth tests decide differently: {shaded}"


def test_w5_negative_w_goes_through_the_clipper(restated):
    s = SCENES["wire_w5_negative_w"]
    r = restated(s.name)
    c, d, st = render_oracle(s, debug_mode=1)
    assert st["triangles_clipped"] == 3 and len(r.lines) == 9, "w <= 0 at one vertex: the clipper runs and keeps the triangle whole"
    assert all(ln.w0 == -1 and ln.w1 == 1 for ln in r.lines)
    assert [(float(ln.d0), float(ln.d1)) for ln in r.lines[::3]] == [(0.25, 0.75), (0.0, 1.0), (-1.0, 2.0)]
    dep = r.frags["depth"].astype(F32)
    print(f"{s.name}: {len(dep)} fragments, {int(np.isposinf(dep).sum())} with +Inf, {int((dep < 0).sum())} negative")
    assert np.isposinf(dep).sum() >= 1 and (dep < 0).sum() >= 10


def test_w5_the_restatement_knows_the_words_the_pipeline_cannot_make():
    t = np.array([0.0, 0.5, 1.0], F32)
    assert np.isneginf(Wf.line_depth(-0.0, -0.0, t)[0]).all()
    assert np.isnan(Wf.line_depth(np.inf, 1.0, t)[0][2]) and Wf.line_depth(np.inf, 1.0, t)[0][0] == 0
    assert np.isposinf(Wf.line_depth(1e-40, 1e-40, t)[0]).all() and np.isneginf(Wf.line_depth(-1e-40, -1e-40, t)[0]).all()


# ------------------------------------------------------------------------------------------------ W6
def test_w6_alpha(restated):
    for s in Wf.family("w6"):
        r = restated(s.name)
        f = r.frags
        a, wr = f["alpha"].astype(F32), f["written"].astype(bool)
        n_neg, n_nan = int((wr & (a < 0)).sum()), int((wr & np.isnan(a)).sum())
        n_zero = int((~wr).sum())
        print(f"{s.name}: written with alpha < 0: {n_neg}, with NaN alpha: {n_nan}; lit and not written (alpha +-0): {n_zero}")
        assert n_neg >= 30 and n_nan >= 30 and n_zero >= 30
        assert ((a == 0) == ~wr).all(), "DepthTest.Always: alpha != 0 alone decides"
        flat = s.draws[0].program == Program.FlatColor
        if not flat and not s.name.startswith("wire_w6_w_"):
            # the row of `crossing` goes on behind its one pixel of alpha exactly 0 (t = 0.5): no early-out
            row = (f["line"] == 0)
            zero_x = f["x"][row & (a == 0)]
            assert len(zero_x) == 1 and (wr & row & (f["x"] > zero_x[0])).sum() >= 15 and (a[row & (f["x"] > zero_x[0])] < 0).all()
        if s.draws[0].blend == BlendMode.None_:
            c, d, st = render_oracle(s, debug_mode=1)
            cf, df, stf = render_oracle(s, debug_mode=0)
            assert (c[..., 3] < 0).sum() >= 30 and np.isnan(c[..., 3]).sum() >= 30
            assert not (cf[..., 3] < 0).any() and not np.isnan(cf[..., 3]).any(), "filled mode writes on alpha > 0 only"
            assert stf["fragments_written"] > 0
    # both sides of the raster kernel's per-record guard div_operands_safe3(clip.w of outputs[0], [1], [0]).  (For a line the third
    # weight is exactly 0, so shade_fragment's per-fragment `fast` -- div_operands_safe3_arith of the weights -- is false whatever
    # the record's flag says: every line fragment takes the full division sequence, and the flag only has to be computed right.)
    outcomes = {}
    for tag, w0, w1 in Wf.W6_CLIP_W:
        ws = {(float(ln.w0), float(ln.w1)) for ln in restated(f"wire_w6_{tag}").lines}
        assert ws == {(w0, w1)}
        outcomes[tag] = Wf.div_operands_safe3(w0, w1, w0)
    print(f"W6 div_operands_safe3 by scene: {outcomes}")
    assert outcomes == {"w_up": True, "w_down": True, "w_both": True, "w_up_out": False, "w_down_out": False, "w_both_out": False}


def test_w6_edges_two_and_three_carry_the_first_edges_varyings():
    """A triangle whose three colours differ, FlatColor aside: the oracle's frame along edges 2 and 3 shows a blend of s0's and s1's
    colours only -- the third vertex's pure blue appears nowhere."""
    s = Wf.family("w6")[0]
    assert s.draws[0].blend == BlendMode.None_ and s.draws[0].program == Program.Gouraud
    import dataclasses
    v = s.draws[0].vertices.copy()
    v["color"][0::3] = (0.0, 0.0, 1.0, 1.0)           # submitted v0 = s2
    v["color"][1::3] = (0.0, 1.0, 0.0, 1.0)           # v1 = s1
    v["color"][2::3] = (1.0, 0.0, 0.0, 1.0)           # v2 = s0
    c, d, st = render_oracle(dataclasses.replace(s, draws=[dataclasses.replace(s.draws[0], vertices=v)]), debug_mode=1)
    lit = d != Wf.FLOAT_MIN
    assert lit.sum() > 200 and (c[lit][:, 2] == 0).all() and (c[lit][:, 0] > 0).any() and (c[lit][:, 1] > 0).any()


# ------------------------------------------------------------------------------------------------ W7
def test_w7_pixels_are_hit_again_inside_a_chunk(restated):
    for s in Wf.family("w7"):
        r = restated(s.name)
        thrice = int((r.hits >= 3).sum())
        tiles = {(int(x) // 16, int(y) // 16) for x, y in zip(r.frags["x"], r.frags["y"])}
        windows = 0
        for tx, ty in tiles:
            pix, _ = Wf.tile_stream(r, tx, ty)
            for lo in range(0, max(1, len(pix) - Wf.CHUNK + 1)):
                w = pix[lo:lo + Wf.CHUNK]
                windows += len(np.unique(w)) < len(w)
        print(f"{s.name}: {len(r.lines)} lines in {len(tiles)} tiles, {thrice} pixels hit three times or more (max {int(r.hits.max())}), "
              f"{windows} windows of {Wf.CHUNK} consecutive fragments hold a pixel twice")
        assert thrice >= 100 and windows >= 1
        if "clipped" in s.name:
            assert sum(ln.fan == 1 for ln in r.lines) >= 3 * 12, "quads: a second fan triangle, six records"
            by_tri = {}
            for ln in r.lines:
                by_tri.setdefault(ln.triangle, []).append(ln)
            twice = [t for t in by_tri.values() if len(t) == 6 and t[2].p0 == t[4].p1 and t[2].p1 == t[4].p0 and (t[2].d0, t[2].d1) != (t[4].d0, t[4].d1)]
            assert len(twice) >= 12, "the shared diagonal, drawn twice with different depths[0..1]"
        else:
            assert len(r.lines) == 3 * Wf.W7_TRIS >= 600 and len(tiles) == (1 if "one_tile" in s.name else 4)


def test_w7_second_hits_at_equal_depth_fail_pass_pass(restated):
    sh = {dt: restated(f"wire_w7_one_tile_Alpha_{dt}").counters()["fragments_shaded"] for dt in ("Less", "LessEqual", "Always")}
    tested = restated("wire_w7_one_tile_Alpha_Less").counters()["fragments_tested"]
    assert sh["Less"] < tested // 4 and sh["LessEqual"] == sh["Always"] == tested


# ------------------------------------------------------------------------------------------------ W8
@pytest.mark.parametrize("N", Wf.W8_RUNS)
def test_w8_a_run_of_empty_pairs_then_one_that_covers(restated, N):
    s = SCENES[f"wire_w8_{N}_empty"]
    r = restated(s.name)
    lst = Wf.tile_list(r, *Wf.W8_TILE)
    counts = [n for _, n in lst]
    print(f"{s.name}: tile {Wf.W8_TILE} gets {len(lst)} pairs with {counts[:3]} ... {counts[-4:]} fragments; tile_pairs {r.tile_pairs}")
    assert counts[:N] == [0] * N and len(counts) == N + 3 and counts[-1] > 0 and all(c > 0 for c in counts[N:])
    assert N in (Wf.SWR_WINDOW - 1, Wf.SWR_WINDOW, Wf.SWR_WINDOW + 1, 2 * Wf.SWR_WINDOW, 100)
    p = F.plan(s, wireframe=True)
    assert p.exact and int(p.lo.sum()) == r.tile_pairs == int(p.hi.sum())
    tile = Wf.W8_TILE[1] * p.tiles_x + Wf.W8_TILE[0]
    assert int(p.lo[tile]) == N + 3


def test_the_window_is_the_kernels():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "softwarerenderer_amd", "csrc", "swr_raster_c.hip.h")).read()
    assert int(re.search(r"#define\s+SWR_WINDOW\s+(\d+)", src).group(1)) == Wf.SWR_WINDOW


# ------------------------------------------------------------------------------------------------ W9
def test_w9_long_lines(restated):
    s = Wf.family("w9")[0]
    r = restated(s.name)
    p = F.plan(s, wireframe=True)
    assert p.exact and int(p.lo.sum()) == r.tile_pairs
    firsts = [i for i, ln in enumerate(r.lines) if ln.edge == 0]
    for li in firsts:
        b = r.boxes[li]
        n_tiles = (b[1] // 16 - b[0] // 16 + 1) * (b[3] // 16 - b[2] // 16 + 1)
        m = r.frags["line"] == li
        nonempty = len({(int(x) // 16, int(y) // 16) for x, y in zip(r.frags["x"][m], r.frags["y"][m])})
        print(f"{s.name}: line {li} bbox {n_tiles} tiles, {nonempty} with a pixel, {int(m.sum())} fragments")
        assert n_tiles == 256 > F.SWR_SMALL_TILES and 16 <= nonempty <= 48
    ln = r.lines[0]
    assert (float(ln.p0[0]), float(ln.p0[1]), float(ln.p1[0]), float(ln.p1[1])) == (0.5, 0.5, 255.5, 255.5), "slope 1 through the tile corners"
    assert int(r.hits.max()) >= 3 and r.counters()["fragments_tested"] > r.counters()["fragments_shaded"]
