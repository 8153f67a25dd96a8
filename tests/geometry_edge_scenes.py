"""Adversarial scene families for the geometry stage: near clipper, fan, setup discards (test helper; not part of the package).

tests/edge_scenes.py and tests/shade_edge_scenes.py stop in front of ClipTriangleAgainstNearPlane ("the families never need the
near clipper").  The families here live inside it, at the branches of k_setup (swr_geometry.hip.h) that random positions never land
on: the inside test `clip.z >= near * clip.w` at a tie, `|denom|` on either side of 1e-6, `t` outside [0, 1] before the clamp, a
lerped clip.w that is 0 / subnormal / too small for 1 / w, and polygons whose two fan triangles meet different ends.

  G1  plane ties: a vertex with clip.z at fl(near * clip.w) and 1..3 ulp on either side, both signs of that w, every near
  G2  denominator threshold: G3's shapes scaled by 2^k (k dense in -16..-24), hand-placed edges with |denom| = fl(1e-6) +- 1 ulp
  G3  shapes: every in/out pattern x every sign pattern of w that enters the clipper, both windings, every CullMode, NaN patterns
  G4  clamp: edges with t > 1, t == 1, t == 0 (and t < 0, if any exists) before the clamp, found by seeded search
  G5  after the cut: lerped w = 0, subnormal, 1 / w infinite, sx overflowing, one fan triangle dying while the other is drawn
  G6  vertex-count ladder: indexed meshes of 1 .. 65 535 vertices around SWR_GEOM_BLOCK = 128 and the wave size 64
  G7  band rejection margin: meshes whose box ends within margin +- 1 px of a band border (band_rejects, swr_flush.h)

EXACT CLIP VECTORS (G1-G5).  Every triangle is its own draw.  Its vertices sit at (1,0,0), (0,1,0), (0,0,1), model = view = I, and
the projection's rows 0..2 are the three wanted clip vectors, row 3 is zero: clip_i = 1 * row_i + 0 * row_j + 0 * row_k + 1 * 0 is
row i bit for bit, in the unfused and in the fused transform alike (every other term is a zero).  A -0 entry arrives as +0
(-0 + 0 = +0): harmless, no family needs a negative zero in a clip vector (near * w may still be -0: that is computed).  A non-finite
entry would poison its whole column (0 * NaN), so the NaN patterns of G3 use a third vertex at (2^100, 2^100, 0) instead, whose
clip.z (or clip.w) is 2^100 * 2^100 - 2^100 * 2^100 = Inf - Inf while the other two vertices keep finite rows (under the fused
transform it is fma(-2^100, 2^100, Inf) = +Inf: a non-finite pattern of its own, restated from the oracle's clip vectors).

The second half restates ClipTriangleAgainstNearPlane and Shaders.Lerp in numpy float32 (clip_near, shaders_lerp), after
Rasterizer.cs:95-160, 200-229 and Shaders.cs:50-95; the fan triangles go to edge_scenes.Tri for DrawTriangle's verdict."""
from __future__ import annotations

import dataclasses
import functools
from fractions import Fraction

import numpy as np

import edge_scenes as E
from softwarerenderer_amd import hostmath as hm
from softwarerenderer_amd import scenes
from softwarerenderer_amd.rasterizer import BlendMode, CullMode, DepthTest, Program

F32 = np.float32
NEARS = (0.1, 0.5, 0.01, 0.0, 0.9)
EPSILON = F32(1e-6)
UNIT = np.eye(3, dtype=F32)
BIG = 2.0 ** 100


# ============================================================================ construction helpers
@dataclasses.dataclass
class T:
    """One triangle = one draw: three clip vectors (rows), free varyings, the draw's state."""
    rows: np.ndarray                    # (3, 4) float32: the wanted clip vectors (NaN patterns: the projection's rows, see nan_triangles)
    color: np.ndarray                   # (3, 4)
    uv: np.ndarray                      # (3, 2)
    normal: np.ndarray                  # (3, 3)
    program: Program = Program.Gouraud
    cull: CullMode = CullMode.None_
    depth_test: DepthTest = DepthTest.LessEqual
    blend: BlendMode = BlendMode.Alpha
    pos: np.ndarray = None              # (3, 3) positions; None = the unit vectors
    tag: str = ""


def ulp_step(x, k):
    """x moved k float32 steps along the number line (k < 0: towards -Inf)."""
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def phong_uniforms():
    u = scenes.default_uniforms()
    u.camera_position[:] = (0.0, 0.0, 0.0)
    for i in range(4):
        u.lights[i].position[:] = (2.0 * i - 3.0, 1.0, -2.0)
        u.lights[i].range = 20.0
        u.lights[i].color[:] = (1.0, 0.8, 0.6)
        u.lights[i].intensity = 1.0
    return u


def draw_of(t: T):
    proj = np.zeros((4, 4), dtype=F32)
    proj[:3] = t.rows
    v = scenes.make_vertices(UNIT if t.pos is None else t.pos, uv=t.uv, normal=t.normal, color=t.color)
    I = hm.identity()
    uni = phong_uniforms() if t.program == Program.Phong4Point else scenes.default_uniforms()
    return scenes.Draw(v, np.arange(3, dtype=np.uint16), I, I, proj, program=t.program, uniforms=uni, cull=t.cull,
                       depth_test=t.depth_test, blend=t.blend)


def make_scene(name, tris, near, W=64, H=64):
    s = scenes.Scene(name, W, H, [draw_of(t) for t in tris], clear_color=(0.1, 0.2, 0.3, 1.0), near_clip=float(near))
    s.tris = list(tris)                 # (not a dataclass field: copies made with dataclasses.replace do not carry it)
    return s


def _varyings(rng, alpha=0.7):
    col = np.concatenate([rng.uniform(0.05, 1.0, (3, 3)), np.full((3, 1), alpha)], axis=1).astype(F32)
    nrm = rng.normal(size=(3, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return col, rng.uniform(-2, 3, (3, 2)).astype(F32), nrm.astype(F32)


def _xy(rng, w, spread=0.85):
    """clip.x, clip.y that land on screen for a positive w (ndc in +-spread), and somewhere nearby for the others."""
    s = abs(float(w)) if w > 0 else max(abs(float(w)), 0.5)
    return [F32(rng.uniform(-spread, spread) * s), F32(rng.uniform(-spread, spread) * s)]


def tri_from_zw(rng, zw, tag="", spread=0.85, **state):
    """A triangle whose (clip.z, clip.w) are given per vertex; x, y and the varyings are drawn from rng."""
    rows = np.array([_xy(rng, w, spread) + [F32(z), F32(w)] for z, w in zw], dtype=F32)
    col, uv, nrm = _varyings(rng)
    return T(rows, col, uv, nrm, tag=tag, **state)


def reversed_twin(t: T):
    """The same three vertices in the other winding."""
    r = lambda a: None if a is None else np.ascontiguousarray(a[::-1])
    rows = r(t.rows) if t.pos is None else t.rows      # (with explicit positions the rows are the matrix: the positions are the vertices)
    return dataclasses.replace(t, rows=rows, color=r(t.color), uv=r(t.uv), normal=r(t.normal), pos=r(t.pos), tag=t.tag + "/rev")


def rotated(t: T, k):
    r = lambda a: None if a is None else np.ascontiguousarray(np.roll(a, -k, axis=0))
    rows = r(t.rows) if t.pos is None else t.rows
    return dataclasses.replace(t, rows=rows, color=r(t.color), uv=r(t.uv), normal=r(t.normal), pos=r(t.pos), tag=f"{t.tag}/rot{k}")


def plain_triangle(rng, alpha=0.5):
    """An unclipped, visible triangle (every w = 1)."""
    zw = [(float(rng.uniform(-0.6, 0.6)), 1.0) for _ in range(3)]
    t = tri_from_zw(rng, zw, tag="plain")
    t.color[:, 3] = alpha
    return t


def _vertex(rng, near, inside, w_positive):
    w = F32(rng.uniform(0.5, 2.0) * (1.0 if w_positive else -1.0))
    plane = float(F32(near) * w)
    return (F32(plane + rng.uniform(0.2, 1.5) * (1.0 if inside else -1.0)), w)


# ============================================================================ G1: plane ties
G1_OFFSETS = (-3, -2, -1, 0, 1, 2, 3)


def g1_plane_ties(seed=0, W=64, H=64):
    """Per near: for both signs of w_B and each of the seven offsets k, in each of the three rotations, a triangle with A (w = -1:
    the clipper runs), B with clip.z = fl(near * w_B) moved k ulp, C well inside.  tag = g1/<sign>/<k>."""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for near in NEARS:
        tris = []
        for sign in (1.0, -1.0):
            for k in G1_OFFSETS:
                for rot in range(3):
                    wb = F32(sign * rng.uniform(0.5, 2.0))
                    zb = ulp_step(F32(near) * wb, k)
                    za = -2.0 if rng.uniform() < 0.6 else 0.5               # A outside, or inside with a negative w
                    t = tri_from_zw(rng, [(za, -1.0), (zb, wb), (1.5, 1.5)], tag=f"g1/{'+' if sign > 0 else '-'}/{k}")
                    tris.append(rotated(t, rot))
        out.append(make_scene(f"geom_g1_near{near:g}_{seed}", tris, near, W, H))
    return out


# ============================================================================ G3: shapes
def nan_triangles(rng, near, **state):
    """NaN patterns.  (a) third vertex at (2^100, 2^100, 0) with rows 0, 1 holding +-2^100 in the z column: its clip.z is Inf - Inf,
    the other two keep their rows; (b) the same in the w column; (c) a NaN in the z column of every vertex (all out, n = 0)."""
    out = []
    for col_ in (2, 3):
        rows = np.zeros((3, 4), dtype=F32)
        rows[0] = [0.3, 0.2, 1.0, 1.0]
        rows[1] = [-0.4, 0.5, -2.0, -1.0]
        rows[0, col_], rows[1, col_] = BIG, -BIG
        if col_ == 3:
            rows[0, 2], rows[1, 2] = 2.0 * BIG, -2.0 * BIG              # z >= near * w for vertex 0, below it for vertex 1
        pos = np.array([[1, 0, 0], [0, 1, 0], [BIG, BIG, 0]], dtype=F32)
        c, uv, n = _varyings(rng)
        t = T(rows, c, uv, n, pos=pos, tag=f"g3/nan_col{col_}", **state)
        out += [t, rotated(t, 1), rotated(t, 2)]
    t = tri_from_zw(rng, [(0.0, 1.0), (0.0, -1.0), (0.0, 1.0)], tag="g3/nan_allz", **state)
    t.rows[:, 2] = np.nan
    out.append(t)
    return out


def g3_shapes_tris(rng, near, twins=True, **state):
    """Every in/out mask (8) x every sign pattern of w with one to two w <= 0 (6): 48 triangles, each with its reversed twin."""
    tris = []
    for mask in range(8):
        for signs in range(1, 7):           # bit i set: w_i > 0; 0 (all skipped) and 7 (not clipped) are not the clipper's
            if bin(signs).count("1") == 3 or signs == 0:
                continue
            zw = [_vertex(rng, near, bool(mask >> i & 1), bool(signs >> i & 1)) for i in range(3)]
            t = tri_from_zw(rng, zw, tag=f"g3/mask{mask:03b}/w{signs:03b}", **state)
            tris.append(t)
            if twins:
                tris.append(reversed_twin(t))
    return tris


def g3_shapes(seed=0, W=64, H=64):
    """FlatColor with three distinct vertex colours under every CullMode (the INTERP flag comes from outputs[0], the LAST vertex of
    a fan triangle: lerped and original last vertices shade differently), DebugVaryings (the Normal lerp), Phong4Point (the
    world-position lerp), Gouraud; plus the NaN patterns."""
    rng = np.random.default_rng(3000 + seed)
    out = []
    for cull in CullMode:
        st = dict(program=Program.FlatColor, cull=cull)
        tris = g3_shapes_tris(rng, 0.1, **st) + nan_triangles(rng, 0.1, **st)
        out.append(make_scene(f"geom_g3_flat_{cull.name}_{seed}", tris, 0.1, W, H))
    for prog, near, cull in ((Program.DebugVaryings, 0.5, CullMode.None_), (Program.Phong4Point, 0.01, CullMode.Back),
                             (Program.Gouraud, 0.9, CullMode.Front)):
        st = dict(program=prog, cull=cull)
        tris = g3_shapes_tris(rng, near, twins=False, **st) + nan_triangles(rng, near, **st)
        out.append(make_scene(f"geom_g3_{prog.name}_{cull.name}_{seed}", tris, near, W, H))
    return out


# ============================================================================ G2: denominator threshold
G2_LADDER = (-10, -14, -16, -17, -18, -19, -20, -21, -22, -23, -24, -26, -40, -100, -126)


def g2_hand_placed(rng):
    """near = 0, w_B = w_C = 1: denom = (z_C - z_B) - 0 * 0 is the difference of the two z exactly.  z_B = -2^-21 (outside),
    z_C = E - 2^-21 with E = fl(1e-6) and its two neighbours (all three differences are exact: E has 2^-43 as its ulp, the sum lies
    in [2^-21, 2^-20)).  A is inside with w = -1 (the clipper runs, and the polygon is more than a sliver at C).  Both edge directions (denom = +E and -E) and every rotation."""
    tris = []
    for k in (-1, 0, 1):
        e = ulp_step(EPSILON, k)
        zb = F32(-2.0 ** -21)
        zc = F32(e + zb)
        assert F32(zc - zb) == e
        for rev in (False, True):
            for rot in range(3):
                t = tri_from_zw(rng, [(0.5, -1.0), (zb, 1.0), (zc, 1.0)], tag=f"g2/hand/{k}")
                t = reversed_twin(t) if rev else t
                tris.append(rotated(t, rot))
    return tris


def g2_denominator(seed=0, W=64, H=64):
    """G3's shapes with every clip vector scaled by 2^k: the picture stays while denom >= 1e-6; below, every cut edge takes the
    t = 0.5 fallback and the picture changes.  Plus the hand-placed edges at the threshold (near = 0)."""
    rng = np.random.default_rng(2000 + seed)
    base = g3_shapes_tris(np.random.default_rng(2500 + seed), 0.1, twins=False)[::2]
    out = []
    for k in G2_LADDER:
        tris = [dataclasses.replace(t, rows=(t.rows * F32(2.0 ** k)).astype(F32), tag=f"g2/2^{k}/" + t.tag) for t in base]
        out.append(make_scene(f"geom_g2_2^{k}_{seed}", tris, 0.1, W, H))
    out.append(make_scene(f"geom_g2_hand_{seed}", g2_hand_placed(rng), 0.0, W, H))
    return out


# ============================================================================ G4: clamp
G4_CLASSES = ("t>1", "t==1", "t==0", "t<0")
G4_WANTED = 10


def clamp_class(t_raw):
    if t_raw is None or t_raw != t_raw:
        return None
    return "t>1" if t_raw > 1 else "t==1" if t_raw == 1 else "t<0" if t_raw < 0 else "t==0" if t_raw == 0 else None


@functools.lru_cache(maxsize=4)
def g4_search(seed=0, tries=20000):
    """Seeded search, the restatement below as the judge.  One vertex of the cut edge sits 0..4 ulp from the plane: the inside one
    (numerator 0 or a few ulp) or the outside one (numerator ~ denominator).  Returns ({class: [(near, triangle)]}, {class: edges met in
    `tries` candidates}).  Large w (ulp(z) above 1e-6) is tried too: only there can both ends sit within ulps of the plane and the
    edge still take the division."""
    rng = np.random.default_rng(4000 + seed)
    found = {c: [] for c in G4_CLASSES}
    counts = {c: 0 for c in G4_CLASSES}
    for _ in range(tries):
        near = NEARS[int(rng.integers(0, len(NEARS)))]
        scale = 1.0 if rng.uniform() < 0.5 else 10 ** rng.uniform(2, 4)
        w0, w1 = F32(rng.uniform(0.3, 3.0) * scale), F32(rng.uniform(0.3, 3.0) * scale)
        kind = int(rng.integers(0, 3))
        k_in, k_out = int(rng.integers(0, 5)), -int(rng.integers(1, 5))
        z0 = ulp_step(F32(near) * w0, k_in) if kind != 1 else F32(float(F32(near) * w0) + rng.uniform(0.2, 1.5) * scale)
        z1 = ulp_step(F32(near) * w1, k_out) if kind != 0 else F32(float(F32(near) * w1) - rng.uniform(0.2, 1.5) * scale)
        if rng.uniform() < 0.5:                     # the edge runs from the outside vertex to the inside one
            z0, w0, z1, w1 = z1, w1, z0, w0
        _, _, denom, t_raw, t = edge_cut(z0, w0, z1, w1, F32(near))
        c = clamp_class(t_raw)
        if c is None:
            continue
        counts[c] += 1
        if len(found[c]) < G4_WANTED:
            za = (0.5 if rng.uniform() < 0.6 else -2.0) * scale            # A: w < 0, inside (a fat polygon) or outside
            tr = tri_from_zw(rng, [(za, -1.0 * scale), (z0, w0), (z1, w1)], tag=f"g4/{c}")
            found[c].append((near, rotated(tr, int(rng.integers(0, 3)))))
    return found, counts


def g4_clamp(seed=0, W=64, H=64):
    found, _ = g4_search(seed)
    out = []
    for near in NEARS:
        tris = [t for c in G4_CLASSES for n, t in found[c] if n == near]
        if tris:
            out.append(make_scene(f"geom_g4_near{near:g}_{seed}", tris, near, W, H))
    return out


# ============================================================================ G5: after the cut
G5_REASONS = ("w_zero", "w_subnormal_drawn", "inv_w_infinite", "sx_overflow", "zero_area", "culled", "offscreen")


def _g5_fixed(rng):
    """Hand-placed triangles, near = 0 (t = 0.5 exactly on an edge from z = -d to z = +d: d / 2d).  poly = [A, B, P_BC, P_CA] for
    the mask (in, in, out): the fan is (A, B, P_BC), (A, P_BC, P_CA), so P_CA belongs to the second triangle only and B to the
    first only."""
    tris = []
    def add(rows, tag):
        c, uv, n = _varyings(rng)
        tris.append(T(np.array(rows, dtype=F32), c, uv, n, tag="g5/" + tag))
    s = 2.0 ** -127
    # lerped w exactly 0 on C -> A (second triangle dies), and on B -> C as well (both die)
    add([[0.5, 0.5, 1.0, 1.0], [-0.6, 0.3, 0.5, 1.0], [0.1, -0.7, -1.0, -1.0]], "w_zero/second")
    add([[0.5, 0.5, 0.5, 1.0], [-0.6, 0.3, 1.0, 1.0], [0.1, -0.7, -1.0, -1.0]], "w_zero/first+second")
    # an ORIGINAL vertex with w = 0 that is inside (z >= 0): B -> the first triangle dies, the second lives
    add([[0.5, 0.5, 0.5, 1.0], [-0.6, 0.3, 0.25, 0.0], [0.1, -0.7, -1.0, 1.0]], "w_zero/first")
    # lerped w = 2^-127 (subnormal, 1 / w = 2^127 finite) on C -> A; the whole edge lives at that scale and is DRAWN
    add([[0.9 * s, 0.6 * s, 2 * s, 3 * s], [-0.6, 0.3, 0.5, 1.0], [0.1 * s, -0.8 * s, -2 * s, -1 * s]], "w_subnormal_drawn")
    # lerped w = 2^-130: 1 / w overflows
    a = 2.0 ** -126                      # A keeps a normal w (1 / w = 2^126); a / 2 - 7 a / 16 = 2^-130 exactly, also fused
    add([[0.5 * a, 0.5 * a, 2 * a, a], [-0.6, 0.3, 0.5, 1.0], [0.1 * a, -0.7 * a, -2 * a, -0.875 * a]], "inv_w_infinite")
    # lerped x = 2^126 with w = 1 (from the outside vertex's 2^127): nx is finite, sx = (nx / 2 + 1 / 2) * W overflows
    add([[0.5, 0.5, 1.0, 3.0], [-0.6, 0.3, 0.5, 1.0], [2.0 ** 127, -0.7, -1.0, -1.0]], "sx_overflow")
    return tris


def _g5_zero_area(rng, near=0.5):
    """First triangle of zero area: B exactly on the plane, t = 0 on B -> C, P_BC = B * 1 + C * 0 = B.  Second triangle of zero
    area: C (w < 0) so close below the plane that B -> C ends at t = 1 (P_BC = C) and C -> A starts at t ~ 1e-8, where
    P_CA = C * 1 + A * t rounds to C: (A, C, C).  Found by search, the restatement as the judge."""
    tris = []
    wb = F32(1.25)
    t = tri_from_zw(rng, [(1.5, 1.5), (F32(near) * wb, wb), (-1.0, -0.25)], tag="g5/zero_area/first")
    tris.append(t)
    for _ in range(4000):
        wc = F32(-rng.uniform(0.5, 2.0))
        zc = ulp_step(F32(near) * wc, -int(rng.integers(1, 4)))
        t = tri_from_zw(rng, [(1.5, F32(rng.uniform(1.0, 1.5))), (1.2, 1.0), (zc, wc)], tag="g5/zero_area/second")
        if verdicts(t, near, 64, 64) == ["drawn", "zero_area"]:
            tris.append(t)
            break
    return tris


def _g5_search(rng, near, cull, want, tries=4000):
    """Triangles of the mask (in, in, out) whose B is inside with a NEGATIVE w (it projects through the eye): the polygon is not
    convex on screen, and the fan's two triangles can differ in orientation and in whether their box meets the target."""
    got = {}
    for _ in range(tries):
        if len(got) == len(want):
            break
        zw = [_vertex(rng, near, True, True), _vertex(rng, near, True, False), _vertex(rng, near, False, bool(rng.uniform() < 0.5))]
        t = tri_from_zw(rng, zw, spread=2.5, cull=cull)
        v = verdicts(t, near, 64, 64)
        if len(v) == 2 and tuple(v) in want and tuple(v) not in got:
            got[tuple(v)] = dataclasses.replace(t, tag=f"g5/{v[0]}+{v[1]}")
    return list(got.values())


def g5_after_the_cut(seed=0, W=64, H=64):
    """Every G5 triangle is followed by an unclipped one-triangle draw, all translucent (Alpha): a second fan triangle whose record
    landed in another slot's place shows as a wrong or missing layer."""
    rng = np.random.default_rng(5000 + seed)
    def interleave(tris):
        out = []
        for t in tris:
            out += [t, plain_triangle(rng)]
        return out
    fixed = _g5_fixed(rng)
    s0 = make_scene(f"geom_g5_fixed_{seed}", interleave(fixed + [rotated(t, 1) for t in fixed] + [reversed_twin(t) for t in fixed]), 0.0, W, H)
    s1 = make_scene(f"geom_g5_zero_area_{seed}", interleave(_g5_zero_area(rng)), 0.5, W, H)
    back = _g5_search(rng, 0.1, CullMode.Back, {("culled", "drawn"), ("drawn", "culled")})
    front = _g5_search(rng, 0.1, CullMode.Front, {("culled", "drawn"), ("drawn", "culled")})
    off = _g5_search(rng, 0.1, CullMode.None_, {("offscreen", "drawn"), ("drawn", "offscreen")})
    assert len(back) == 2 and len(front) == 2 and len(off) == 2, "G5: a wanted (dies, lives) pair was not found for this seed"
    assert len(s1.tris) == 4, "G5: the zero-area search found nothing for this seed"
    s2 = make_scene(f"geom_g5_mixed_fans_{seed}", interleave(back + front + off), 0.1, W, H)
    return [s0, s1, s2]


# ============================================================================ G6: vertex-count ladder
G6_COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 257, 65535)


def g6_mesh(rng, n, program):
    """An indexed mesh of n vertices under an ordinary projection: triangles (i, i+1, i+2) of neighbouring vertices, one across the
    border of the first 128-vertex block, the last one ending at vertex n - 1.  n < 3: one degenerate triangle (0, n-1, n-1)."""
    groups = rng.uniform([-2.0, -2.0, -4.0], [2.0, 2.0, 0.3], (n // 8 + 1, 3))          # some vertices behind the eye: clipped
    pos = groups[np.arange(n) // 8] + rng.uniform(-0.3, 0.3, (n, 3))
    col = np.concatenate([rng.uniform(0.05, 1.0, (n, 3)), np.full((n, 1), 0.6)], axis=1)
    v = scenes.make_vertices(pos, uv=rng.uniform(-2, 3, (n, 2)), normal=rng.normal(size=(n, 3)) + [0, 0, 3.0], color=col)
    if n < 3:
        idx = [(0, n - 1, n - 1)]
    else:
        step = max(1, (n - 2) // 400)
        first = sorted(set(range(0, n - 2, step)) | {n - 3} | ({126, 127} if n > 129 else set()) | ({62, 63} if n > 65 else set()))
        idx = [(i, i + 1, i + 2) for i in first]
    idx = np.asarray(idx, dtype=np.uint16).reshape(-1)
    assert int(idx.max()) == n - 1
    I = hm.identity()
    return scenes.Draw(v, idx, I, I, scenes._perspective(256, 256), program=program, uniforms=scenes.default_uniforms(),
                       cull=CullMode.None_, depth_test=DepthTest.LessEqual, blend=BlendMode.Alpha)


def g6_vertex_ladder(seed=0, W=256, H=256):
    """All twelve meshes in ONE flush (vert_base of every draw after the first is then not a multiple of 128), in two orders."""
    rng = np.random.default_rng(6000 + seed)
    draws = [g6_mesh(rng, n, Program.Gouraud if i % 2 else Program.FlatColor) for i, n in enumerate(G6_COUNTS)]
    return [scenes.Scene(f"geom_g6_ladder_{seed}", W, H, draws, near_clip=0.1),
            scenes.Scene(f"geom_g6_ladder_reversed_{seed}", W, H, draws[::-1], near_clip=0.1)]


# ============================================================================ G7: band rejection margin
def band_box(draw, H):
    """What band_rejects (swr_flush.h) derives from a draw's exact box, restated in double: (smin, smax, margin) of the eight
    projected corners, or None where one of its guards keeps the draw whatever the band: a corner that is not finite or not in
    front (`cw > 0`), a float32 w that may not be safely positive (`wmin - ew > 1e-6 wmin`), a margin that is not finite.
    margin = 2 px + the float32 running-error term of the three chained transforms."""
    mv = draw.model.astype(np.float64) @ draw.view.astype(np.float64)
    amv = np.abs(draw.model.astype(np.float64)) @ np.abs(draw.view.astype(np.float64))
    M, A = mv @ draw.projection.astype(np.float64), amv @ np.abs(draw.projection.astype(np.float64))
    p = draw.vertices["position"].astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    u16 = 16.0 / 16777216.0
    ey = ew = ndc_abs = 0.0
    wmin, smin, smax = 1e300, 1e300, -1e300
    for corner in range(8):
        c = np.array([hi[i] if corner >> i & 1 else lo[i] for i in range(3)] + [1.0])
        cy, cw = float(c @ M[:, 1]), float(c @ M[:, 3])
        sy_abs, sw_abs = float(np.abs(c) @ A[:, 1]), float(np.abs(c) @ A[:, 3])
        if not all(np.isfinite(x) for x in (cy, cw, sy_abs, sw_abs)):
            return None
        ey, ew = max(ey, u16 * sy_abs), max(ew, u16 * sw_abs)
        if not cw > 0:
            return None
        wmin = min(wmin, cw)
        ndc = cy / cw
        ndc_abs = max(ndc_abs, abs(ndc))
        sy = (1.0 - (ndc * 0.5 + 0.5)) * H
        if not np.isfinite(sy):
            return None
        smin, smax = min(smin, sy), max(smax, sy)
    if not wmin - ew > 1e-6 * wmin:
        return None
    margin = 2.0 + 0.5 * H * (ey + ndc_abs * ew) / (wmin - ew)
    return (smin, smax, margin) if np.isfinite(margin) else None


def band_margin(draw, H):
    return band_box(draw, H)[2]


def band_keeps(draw, H, y0, y1):
    """Does the band of pixel rows [y0, y1) record the draw?  (band_rejects' last line.)"""
    b = band_box(draw, H)
    return b is None or not (b[1] + b[2] < y0 or b[0] - b[2] > y1)


G7_OFFSETS = ("-margin-1", "-margin+1", "-1", "0", "+1", "+2.5")


def g7_band_margin(worlds=(2, 3), seed=0, W=256, H=256):
    """Per band border Y (of the 2- and the 3-band partition of 16 tile rows) and per side, six small meshes in clip space
    (identity matrices, w = 1) whose exact box ends at Y - margin - 1, Y - margin + 1, Y - 1, Y, Y + 1, Y + 2.5 (mirrored below the
    border): the first is rejected by the band beyond the border, the second must be kept, the last three put fragments on the
    border rows from the far side.  Two meshes with a corner at w barely positive: one kept by its huge projected box, one by the `wmin - ew` guard.  Returns (scene, borders)."""
    from softwarerenderer_amd import multigpu
    rng = np.random.default_rng(7000 + seed)
    borders = sorted({b[0] * 16 for w in worlds for b in multigpu.band_partition(H, w) if b[0] > 0})
    ny = lambda sy: 1.0 - 2.0 * sy / H
    I = hm.identity()
    draws = []
    x0 = -0.95

    def quad(end, far, x0):
        pos = [(x0, ny(end), 0.1), (x0 + 0.07, ny(end), -0.2), (x0 + 0.035, ny(far), 0.3), (x0 + 0.1, ny(far), 0.0)]
        col = np.concatenate([rng.uniform(0.2, 1.0, (4, 3)), np.full((4, 1), 0.7)], axis=1)
        return scenes.Draw(scenes.make_vertices(np.asarray(pos), color=col), np.array([0, 1, 2, 1, 3, 2], dtype=np.uint16), I, I, I,
                           program=Program.Gouraud, cull=CullMode.None_, depth_test=DepthTest.LessEqual, blend=BlendMode.Alpha)

    for Y in borders:
        for side in (-1.0, 1.0):        # -1: the mesh lies above the border (smaller rows); o = how far its box reaches past Y
            for off in G7_OFFSETS:
                m = band_margin(quad(Y, Y + 7.0 * side, x0), H)          # (the margin depends on the box only through |ndc y| <= 1)
                o = {"-margin-1": -m - 1.0, "-margin+1": -m + 1.0}.get(off)
                o = float(off) if o is None else o
                end = Y - side * o
                draws.append(quad(end, end + 7.0 * side, x0))
                x0 = x0 + 0.105 if x0 < 0.8 else -0.95
    v = scenes.make_vertices(np.array([(0.0005, 0.0002, 0.001), (0.3, -0.2, 1.0), (-0.4, 0.1, 1.0)]),
                             color=np.array([(1.0, 0.2, 0.2, 0.7), (0.2, 1.0, 0.2, 0.7), (0.2, 0.2, 1.0, 0.7)]))
    draws.append(scenes.Draw(v, np.arange(3, dtype=np.uint16), I, I, E.w_projection(0.2), program=Program.Gouraud,
                             cull=CullMode.None_, depth_test=DepthTest.LessEqual, blend=BlendMode.Alpha))
    # ... and one whose nearest corner has w = 5e-7, below the float32 error of w at the far corners (the `wmin - ew` guard keeps it)
    v = scenes.make_vertices(np.array([(2.5e-7, -1e-7, 5e-7), (-0.5, -0.6, 1.0), (0.6, -0.3, 1.0)]),
                             color=np.array([(0.9, 0.9, 0.2, 0.7), (0.2, 0.9, 0.9, 0.7), (0.9, 0.2, 0.9, 0.7)]))
    draws.append(scenes.Draw(v, np.arange(3, dtype=np.uint16), I, I, E.w_projection(0.2), program=Program.Gouraud,
                             cull=CullMode.None_, depth_test=DepthTest.LessEqual, blend=BlendMode.Alpha))
    assert band_box(draws[-2], H) is not None and band_box(draws[-1], H) is None
    return scenes.Scene(f"geom_g7_bands_{seed}", W, H, draws, near_clip=0.1), borders


FAMILIES = {"g1": g1_plane_ties, "g2": g2_denominator, "g3": g3_shapes, "g4": g4_clamp, "g5": g5_after_the_cut,
            "g6": g6_vertex_ladder}
RESTATED = ("g1", "g2", "g3", "g4", "g5")


def restated_scenes(seed=0):
    return [s for f in RESTATED for s in FAMILIES[f](seed)]


# ============================================================================ float32 restatement
def _round_f32(s: Fraction):
    """The float32 nearest to the nonzero rational s (ties to even, gradual underflow, overflow to Inf)."""
    sign, m = (-1.0, -s) if s < 0 else (1.0, s)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1
    e = max(e, -126)
    q = Fraction(2) ** (e - 23)
    k = m / q
    n = k.numerator // k.denominator
    r = k - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    val = n * q
    if val >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * float(val))


def fma32(a, b, c):
    """fmaf(a, b, c): a * b + c rounded once."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))           # (the product of two float32 never overflows a double)
    # fast path: the product is exact in double and the sum rounds once to 53 bits; that decides the float32 rounding unless the
    # double lands within a few of its own ulps of a float32 tie (or in the subnormal / overflow range): then exact rationals
    d = a * b + c
    with np.errstate(over="ignore"):
        r = F32(d)
    if d != 0.0 and np.isfinite(r) and abs(float(r)) >= 2.0 ** -125:
        other = np.nextafter(r, F32(np.inf) if d > float(r) else F32(-np.inf))
        tie = 0.5 * (float(r) + float(other))                          # exact in double
        if abs(d - tie) > abs(d) * 2.0 ** -50:
            return r
    s = Fraction(a) * Fraction(b) + Fraction(c)
    if s == 0:
        return F32(np.float64(a) * np.float64(b) + np.float64(c))               # exact product (no underflow in double): IEEE sign of the sum
    return _round_f32(s)


def shaders_lerp(a, b, t, fused):
    """VectorN.Lerp(a, b, t) = a * (1 - t) + b * t per component (Shaders.cs:50-95 lerps every varying so), each operation rounded
    to float32; fused: fmaf(a, 1 - t, b * t), the model of liboswr_fma.so and libswr_hip_fma.so."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    t = F32(t)
    with np.errstate(all="ignore"):
        u = F32(F32(1.0) - t)
        y = (b * t).astype(F32)
        if not fused:
            return ((a * u).astype(F32) + y).astype(F32)
        return np.array([fma32(x, u, yy) for x, yy in zip(a.reshape(-1), y.reshape(-1))], dtype=F32).reshape(a.shape)


def edge_cut(z0, w0, z1, w1, near):
    """(cur_in, nxt_in, denom, t_raw, t) of the edge cur -> nxt (Rasterizer.cs:112-142).  denom / t_raw are None where the
    reference does not compute them; t_raw is None on the |denom| < 1e-6 fallback (t = 0.5)."""
    with np.errstate(all="ignore"):
        z0, w0, z1, w1, near = F32(z0), F32(w0), F32(z1), F32(w1), F32(near)
        cur_in, nxt_in = bool(z0 >= F32(near * w0)), bool(z1 >= F32(near * w1))
        if cur_in == nxt_in:
            return cur_in, nxt_in, None, None, None
        denom = F32(F32(z1 - z0) - F32(near * F32(w1 - w0)))
        if abs(denom) < EPSILON:
            return cur_in, nxt_in, denom, None, F32(0.5)
        t_raw = F32(F32(z0 - F32(near * w0)) / F32(F32(near * F32(w1 - w0)) - F32(z1 - z0)))
        t = F32(0.0) if t_raw < 0 else F32(1.0) if t_raw > 1 else t_raw
        return cur_in, nxt_in, denom, t_raw, t


VARYING_KEYS = ("color", "uv", "normal", "wn", "wpos")


@dataclasses.dataclass
class Clipped:
    n: int
    clips: np.ndarray           # (n, 4)
    vary: dict                  # key -> (n, k)
    lerped: list                # per polygon vertex: made by Shaders.Lerp (Interpolate = true) or copied
    fans: list                  # index triples into the polygon, in DrawTriangle call order ([] when n < 3)
    edges: list                 # per edge i -> (i + 1) % 3: edge_cut's tuple


def clip_near(clips, varyings, near, fused):
    """ClipTriangleAgainstNearPlane (Rasterizer.cs:95-160) and the fan of RenderMesh (:219-223) for one triangle."""
    clips = np.asarray(clips, dtype=F32)
    pc, pv, lerped, edges = [], {k: [] for k in varyings}, [], []
    for i in range(3):
        j = (i + 1) % 3
        e = edge_cut(clips[i][2], clips[i][3], clips[j][2], clips[j][3], near)
        edges.append(e)
        if e[0]:
            pc.append(clips[i].copy()); lerped.append(False)
            for k in varyings:
                pv[k].append(np.asarray(varyings[k][i], dtype=F32))
        if e[0] != e[1]:
            pc.append(shaders_lerp(clips[i], clips[j], e[4], fused)); lerped.append(True)
            for k in varyings:
                pv[k].append(shaders_lerp(varyings[k][i], varyings[k][j], e[4], fused))
    n = len(pc)
    fans = [(0, k, k + 1) for k in range(1, n - 1)] if n >= 3 else []
    return Clipped(n, np.array(pc, dtype=F32).reshape(n, 4), {k: np.array(v, dtype=F32) for k, v in pv.items()}, lerped, fans, edges)


def enters_clipper(clips):
    """RenderMesh :208-217: None = skipped (every w <= 0), False = drawn as it is, True = clipped."""
    b = [bool(c[3] <= 0) for c in clips]
    return None if all(b) else any(b)


def setup_verdict(clips3, W, H, cull):
    """What DrawTriangle + RasterizeTriangle's prologue do with one triangle (v0, v1, v2): 'nonfinite' (:378-380, which also
    returns first for every clip.w == 0 of :393), 'zero_area' (:396), 'culled' (:414-417), 'offscreen' (:442) or 'drawn'
    (counted in triangles_setup)."""
    with np.errstate(all="ignore"):
        t = E.Tri(list(clips3), W, H, clipper_keeps=True)
    if not hasattr(t, "sx"):
        return "nonfinite"
    if not hasattr(t, "area"):
        return "zero_area"
    front = bool(t.area < 0)
    if (cull == CullMode.Back and not front) or (cull == CullMode.Front and front):
        return "culled"
    # (the bbox clamps of :437-440 with MathF.Min / Max, NaN-propagating: Tri computes them with Python's min / max, which differ
    # for NaN only; a NaN screen coordinate needs a non-finite ndc, which has returned above)
    return "drawn" if (t.minX <= t.maxX and t.minY <= t.maxY) else "offscreen"


def clips_of(draw, fused=False):
    """The three clip vectors of a one-triangle draw through E.clip_of (unfused).  For the unit positions both transforms give
    the rows themselves; the NaN patterns give Inf - Inf either way."""
    with np.errstate(all="ignore"):
        return np.array([E.clip_of(draw, i) for i in range(3)], dtype=F32)


def clips_of_T(t: T):
    """The same without the transform where it is the identity on the rows (x + 0 turns a -0 into +0, as the transform does);
    tests/test_geometry_edges_host.py holds this against clips_of and the oracle's vertex shader for every triangle."""
    return (t.rows + F32(0.0)).astype(F32) if t.pos is None else clips_of(draw_of(t))


def verdicts(t: T, near, W, H, fused=False):
    """Setup verdicts of the fan triangles of one T (its own verdict when it is not clipped, [] when skipped or n < 3)."""
    clips = clips_of_T(t)
    ec = enters_clipper(clips)
    if ec is None:
        return []
    if not ec:
        return [setup_verdict(clips, W, H, t.cull)]
    c = clip_near(clips, {}, near, fused)
    return [setup_verdict([c.clips[i] for i in f], W, H, t.cull) for f in c.fans]


def scene_counts(scene, fused=False):
    """(triangles_clipped, triangles_setup) of a G1-G5 scene in filled mode, from the restatement alone."""
    clipped = setup = 0
    for t in scene.tris:
        clips = clips_of_T(t)
        clipped += 1 if enters_clipper(clips) else 0
        setup += sum(v == "drawn" for v in verdicts(t, F32(scene.near_clip), scene.width, scene.height, fused))
    return clipped, setup
