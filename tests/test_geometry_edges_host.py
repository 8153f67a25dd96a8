"""The geometry edge families of tests/geometry_edge_scenes.py on the CPU: the float32 restatement of the near clipper against
the oracle's (oswr_clip_triangle), word for word, for EVERY triangle of G1-G5, in the default and in the fused-lerp oracle; the
restatement's counters against the oracle's rendered ones; and the reach of every family, counted with the restatement.

Words that are NaN on both sides count as equal (the payload is the hardware's choice); every other word must be the same bits.

Mutants of the oracle's clipper (one change each in a scratch copy of oracle/swr_oracle.c, both oracle builds remade; "words" =
test_restatement_equals_the_oracle_word_for_word_on_every_triangle, "counters" = test_counters_of_every_scene_..., each in both
variants).  Right column: the CPU tests of the oracle as they were before this file (test_oracle_kat, test_oracle_golden and the
two earlier edge host files: 61 tests).
  mutant                                      this file fails in        the 61 earlier CPU tests
  `>=` -> `>` in the inside test              words, counters           all pass
  threshold 1e-6 -> 1e-5                      words                     all pass
  fallback 0.5 -> 0                           words, counters           all pass
  clamp removed                               words, counters           all pass
  `w <= 0` -> `w < 0` (RenderMesh :208-210)   counters                  golden[degenerate]
  fan (0,2,3) -> (0,1,3)                      counters                  kat near_plane_clip..., golden[nearclip x2, degenerate]
  second fan triangle's vertices swapped      counters                  golden[nearclip x2, degenerate]
  `n >= 3` -> `n > 3`                         counters                  golden[nearclip x2]
  triangles_clipped only when n >= 3          counters                  golden[nearclip x2]
  `r.interpolate = a->interpolate` in Lerp    words                     kat near_plane_clip..., golden[nearclip_FlatColor]
  INTERP from v0 instead of outputs[0]        (not this file: it renders no pixels; the GPU file does)   kat, golden[nearclip_FlatColor]
The golden frames pin the ORACLE against such changes; nothing pinned the two device copies of the clipper at these branches: the
device-side table is in tests/test_gpu_geometry_edges.py.

Equivalent mutants, argued and not killed:
  the `clip.w == 0` test of DrawTriangle (:393, setup_triangle's second return): with w == 0, 1 / w is +-Inf and each of nx, ny, nz is
      +-Inf or NaN (0 * Inf), so the non-finite return of :378-380 is always taken first.  G5 w_zero reaches it all the same.
  t written as -(z0 - near * w0) / denom: denom = (z1 - z0) - near (w1 - w0) and the reference's divisor near (w1 - w0) - (z1 - z0)
      are fl(a - b) and fl(b - a) of the same two float32, which negate exactly (round-to-nearest is symmetric), so the two
      quotients are the same bits, signed zeros included.

t < 0 before the clamp: the seeded search of g4_search (20 000 edges with an end within 0..4 ulp of the plane, half of them at
w ~ 1e2..1e4 where an ulp of z exceeds 1e-6) finds none, and test_g4_reach keeps the count.  The numerator fl(z0 - fl(near w0))
has the sign of the inside test of `cur` by construction (the test compares the same two float32 it subtracts), the true divisor
has that sign too, and for the computed divisor to flip it would have to be smaller than the rounding of near * (w1 - w0), i.e.
far below 1e-6 -- where the fallback is taken instead.  `if (t < 0) t = 0` is therefore kept as the reference has it, untested."""
import ctypes as C

import numpy as np
import pytest

import edge_scenes as E
import geometry_edge_scenes as G
from oracle import binding as ob

F32 = np.float32
VARIANTS = ("", "fma")
FIELDS = (("clip", "clips"), ("color", "color"), ("texcoord", "uv"), ("normal", "normal"), ("world_normal", "wn"), ("world_pos", "wpos"))


@pytest.fixture(scope="module")
def libs():
    ob.build()
    return {v: ob.load(variant=v) for v in VARIANTS}


def same_words(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def oracle_vertices(lib, draw):
    """The three VertexOutputs of a one-triangle draw, from the oracle's vertex shader."""
    v = np.ascontiguousarray(draw.vertices)
    out = (ob.OVertexOutput * 3)()
    m, vw, p = (np.ascontiguousarray(a, dtype=F32).reshape(-1) for a in (draw.model, draw.view, draw.projection))
    for i in range(3):
        lib.oswr_vertex_shader(v.ctypes.data + i * v.dtype.itemsize, m.ctypes.data, vw.ctypes.data, p.ctypes.data, int(draw.program),
                               C.byref(out[i]))
    return out


def as_arrays(vo, n):
    return {mine: np.array([list(getattr(vo[i], theirs)) for i in range(n)], dtype=F32).reshape(n, len(getattr(vo[0], theirs)))
            for theirs, mine in FIELDS}


def all_triangles():
    for s in G.restated_scenes(0):
        for t, d in zip(s.tris, s.draws):
            yield s, t, d


@pytest.mark.parametrize("variant", VARIANTS, ids=["default", "fma"])
def test_restatement_equals_the_oracle_word_for_word_on_every_triangle(libs, variant):
    lib = libs[variant]
    fused = bool(lib.oswr_numerics_fma())
    assert fused == (variant == "fma")
    n_tris = n_clipped = n_lerped = 0
    for transform_fma in (0, 1):
        lib.oswr_set_transform_fma(transform_fma, transform_fma)
        for s, t, d in all_triangles():
            vin = oracle_vertices(lib, d)
            a = as_arrays(vin, 3)
            # the construction: the clip vectors are the rows, whichever way the transform sums
            # (the NaN patterns' third vertex is Inf - Inf unfused and fma(-2^100, 2^100, Inf) = Inf fused: both are kept as patterns)
            if t.pos is None or transform_fma == 0:
                assert same_words(a["clips"], G.clips_of_T(t)), (s.name, t.tag, "clip vectors are not the rows")
            if transform_fma == 0:
                assert same_words(a["clips"], G.clips_of(d)), (s.name, t.tag)
            n_tris += 1
            ec = G.enters_clipper(a["clips"])
            assert ec is not None, (s.name, t.tag, "a family triangle with every w <= 0 tests nothing")
            if not ec:
                assert t.tag == "plain" or "nan" in t.tag, (s.name, t.tag)
                continue
            n_clipped += 1
            out = (ob.OVertexOutput * 4)()
            n = lib.oswr_clip_triangle(F32(s.near_clip), vin, out)
            vary = {k: a[k] for k in G.VARYING_KEYS}
            got = G.clip_near(a["clips"], vary, F32(s.near_clip), fused)
            assert got.n == n, (s.name, t.tag, got.n, n, got.edges)
            want = as_arrays(out, n)
            assert same_words(got.clips, want["clips"]), (s.name, t.tag, "clip", got.clips, want["clips"], got.edges)
            for k in G.VARYING_KEYS:
                assert same_words(got.vary[k].reshape(want[k].shape), want[k]), (s.name, t.tag, k, got.vary[k], want[k], got.edges)
            for i in range(n):
                assert out[i].interpolate == (1 if got.lerped[i] else vin[0].interpolate), (s.name, t.tag, i)
            n_lerped += sum(got.lerped)
    lib.oswr_set_transform_fma(int(fused), int(fused))
    print(f"{variant or 'default'}: {n_tris} triangles, {n_clipped} through the clipper, {n_lerped} lerped vertices")
    assert n_clipped > 2000 and n_lerped > 3000


@pytest.mark.parametrize("variant", VARIANTS, ids=["default", "fma"])
def test_counters_of_every_scene_equal_the_rendered_oracle_and_every_scene_draws(libs, variant):
    for s in G.restated_scenes(0):
        o = ob.OracleRenderer(s.width, s.height, variant=variant)
        o.render_scene(s)
        st = o.stats(); o.close()
        clipped, setup = G.scene_counts(s, fused=variant == "fma")
        assert st["triangles_in"] == len(s.tris)
        assert (clipped, setup) == (st["triangles_clipped"], st["triangles_setup"]), (s.name, clipped, setup, st)
        assert st["fragments_written"] > 0, f"{s.name}: nothing was drawn"


def test_g1_reach():
    """Every near, both signs of w, each of the seven ulp offsets: the vertex is inside exactly from offset 0 upwards."""
    seen = set()
    for s in G.g1_plane_ties(0):
        for t in s.tris:
            _, sign, k, rot = t.tag.split("/")
            i = (1 - int(rot[3:])) % 3                                  # where B went
            z, w = t.rows[i][2], t.rows[i][3]
            assert (w > 0) == (sign == "+")
            assert z == G.ulp_step(F32(s.near_clip) * w, int(k))
            c = G.clip_near(G.clips_of_T(t), {}, F32(s.near_clip), False)
            assert c.edges[i][0] == (int(k) >= 0), (s.name, t.tag)
            seen.add((s.near_clip, sign, int(k), c.edges[i][0]))
    assert len(seen) == len(G.NEARS) * 2 * 7
    assert {k for _, _, k, inside in seen if inside} == {0, 1, 2, 3} and {k for _, _, k, inside in seen if not inside} == {-3, -2, -1}


def _edges(scenes_):
    for s in scenes_:
        for t in s.tris:
            clips = G.clips_of_T(t)
            if G.enters_clipper(clips):
                for e in G.clip_near(clips, {}, F32(s.near_clip), False).edges:
                    if e[2] is not None:
                        yield s, t, e


def test_g2_reach():
    """Cut edges on both sides of |denom| = 1e-6, and at fl(1e-6) and its two neighbours, with either sign of denom."""
    below = above = 0
    at = set()
    per_scene = {}
    for s, t, e in _edges(G.g2_denominator(0)):
        d = abs(e[2])
        below += d < G.EPSILON
        above += d >= G.EPSILON
        assert (e[3] is None) == (d < G.EPSILON)
        for k in (-1, 0, 1):
            if d == G.ulp_step(G.EPSILON, k):
                at.add((k, bool(e[2] > 0)))
        per_scene.setdefault(s.name, [0, 0])[int(d < G.EPSILON)] += 1
    assert below >= 100 and above >= 100
    assert at == {(k, sgn) for k in (-1, 0, 1) for sgn in (False, True)}
    # the ladder crosses the threshold inside its dense part: scenes wholly above, wholly below, and mixed
    kinds = {(a > 0, b > 0) for a, b in per_scene.values()}
    assert kinds == {(True, False), (False, True), (True, True)}, per_scene


def test_g3_reach():
    """Every in/out mask x every sign pattern that enters the clipper, n = 0, 3 and 4, the NaN patterns, in every scene."""
    for s in G.g3_shapes(0):
        seen, ns = set(), set()
        nan_z = nan_w = 0
        for t in s.tris:
            clips = G.clips_of_T(t)
            if "nan" in t.tag:
                nan_z += bool(np.isnan(clips[:, 2]).any()); nan_w += bool(np.isnan(clips[:, 3]).any())
                if not G.enters_clipper(clips):
                    continue
            assert G.enters_clipper(clips) is True
            c = G.clip_near(clips, {}, F32(s.near_clip), False)
            mask = tuple(e[0] for e in c.edges)
            seen.add((mask, tuple(bool(x > 0) for x in clips[:, 3])))
            ns.add(c.n)
            assert c.n == {0: 0, 1: 3, 2: 4, 3: 3}[sum(mask)]
        assert len({m for m, _ in seen}) == 8 and len(seen) >= 48, s.name
        assert ns == {0, 3, 4} and nan_z >= 4 and nan_w >= 3, (s.name, ns, nan_z, nan_w)
    assert {s.tris[0].cull for s in G.g3_shapes(0)} == set(G.CullMode)
    assert {s.tris[0].program for s in G.g3_shapes(0)} >= {G.Program.FlatColor, G.Program.DebugVaryings, G.Program.Phong4Point}


def test_g4_reach():
    """At least 8 edges in each reachable clamp class; the search for t < 0 is kept with its count (module docstring)."""
    found, counts = G.g4_search(0)
    print("g4_search: edges met per class in 20000 candidates:", counts)
    got = {c: 0 for c in G.G4_CLASSES}
    for s, t, e in _edges(G.g4_clamp(0)):
        c = G.clamp_class(e[3])
        if c is not None:
            got[c] += 1
            assert e[4] == (1.0 if c in ("t>1", "t==1") else 0.0)
    for c in G.G4_CLASSES:
        if counts[c] > 0:
            assert got[c] >= 8, (c, got, counts)
    assert all(counts[c] > 0 for c in ("t>1", "t==1", "t==0")), counts
    assert got["t<0"] == len(found["t<0"])


def test_g5_reach():
    """Each discard reason, and both orders of 'one fan triangle dies, the other is drawn'."""
    reasons, pairs = set(), set()
    for s in G.g5_after_the_cut(0):
        assert [t.tag == "plain" for t in s.tris] == [i % 2 == 1 for i in range(len(s.tris))]       # interleaved
        for t in s.tris:
            if t.tag == "plain":
                continue
            clips = G.clips_of_T(t)
            c = G.clip_near(clips, {}, F32(s.near_clip), False)
            v = G.verdicts(t, F32(s.near_clip), s.width, s.height)
            if len(v) == 2:
                pairs.add(tuple(x == "drawn" for x in v))
            reasons |= set(v)
            for i, lerped in enumerate(c.lerped):
                w = c.clips[i][3]
                if lerped and w == 0:
                    reasons.add("w_zero")
                with np.errstate(all="ignore"):
                    if lerped and w != 0 and abs(w) < 2.0 ** -126:
                        reasons.add("inv_w_infinite" if np.isinf(F32(1.0) / w) else "w_subnormal")
            for f, verdict in zip(c.fans, v):
                with np.errstate(all="ignore"):
                    tri = E.Tri([c.clips[i] for i in f], s.width, s.height, clipper_keeps=True)
                if hasattr(tri, "sx") and np.isinf(tri.sx).any():
                    reasons.add("sx_overflow")
                if verdict == "drawn" and any(c.lerped[i] and 0 < abs(c.clips[i][3]) < 2.0 ** -126 for i in f):
                    reasons.add("w_subnormal_drawn")
    assert reasons >= {"w_zero", "w_subnormal", "w_subnormal_drawn", "inv_w_infinite", "sx_overflow", "nonfinite", "zero_area",
                       "culled", "offscreen", "drawn"}, reasons
    assert pairs >= {(False, True), (True, False), (False, False), (True, True)}
    order = {tuple(G.verdicts(t, F32(s.near_clip), 64, 64)) for s in G.g5_after_the_cut(0) for t in s.tris}
    for dead in ("nonfinite", "zero_area", "culled", "offscreen"):
        assert (dead, "drawn") in order and ("drawn", dead) in order, (dead, order)


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    """fma32 against a double evaluation where that is exact, and on hand-picked double-rounding / underflow / overflow cases."""
    rng = np.random.default_rng(5)
    for _ in range(2000):
        a, b = F32(rng.normal()), F32(rng.normal())
        c = F32(-(np.float64(a) * np.float64(b))) if rng.uniform() < 0.3 else F32(rng.normal() * 10 ** rng.uniform(-8, 2))
        exact = np.float64(a) * np.float64(b) + np.float64(c)           # the product is exact in double; the sum rounds to 53 bits
        r = G.fma32(a, b, c)
        lo, hi = np.nextafter(r, F32(-np.inf)), np.nextafter(r, F32(np.inf))
        assert abs(np.float64(r) - exact) <= min(abs(np.float64(lo) - exact), abs(np.float64(hi) - exact))
    one, u = F32(1.0), F32(2.0 ** -24)
    assert G.fma32(F32(1.0 + 2.0 ** -23), F32(1.0 + 2.0 ** -23), F32(0.0)) == F32(1.0 + 2.0 ** -22)      # 1 + 2^-22 + 2^-46 rounds down
    assert G.fma32(u, one, one) == one and G.fma32(F32(u * (1 + 2.0 ** -23)), one, one) == F32(1.0 + 2.0 ** -23)   # tie to even; above the tie
    assert G.fma32(F32(2.0 ** -100), F32(2.0 ** -49), F32(0.0)) == F32(2.0 ** -149)
    assert G.fma32(F32(2.0 ** -100), F32(2.0 ** -50), F32(0.0)) == 0.0 and G.fma32(F32(2.0 ** 100), F32(2.0 ** 100), F32(0.0)) == np.inf
    assert np.isnan(G.fma32(F32(np.inf), F32(0.0), one)) and G.fma32(F32(2.0), F32(3.0), F32(-6.0)) == 0.0
