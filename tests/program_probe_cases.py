"""Probes of the user fragment contract, field by field (test helper; not part of the package).

A run-time compiled fragment program (csrc/swr_program.hip.h) is fed by a branch of k_raster_c of its own, shade_user: VOut rows at
fixed offsets, the Normal side array, the screen positions out of the TriRec, interpolate_fs_in, and an swr_fs_env built by hand.  The
twin tests (test_gpu_custom_program.py, test_gpu_vertex_program.py) see of that only what a built-in program happens to read.  A
PROBE is a fragment program that returns three contract scalars unchanged, `make_float4(a, b, c, 1.0f)` (w is 1 because the raster
stage writes only results with w > 0: no field may sit in w), drawn with BlendMode.None and DepthTest.LessEqual on a cleared frame in
a scene where no sample is covered twice: the colour plane's x, y, z at a covered pixel ARE the three words, every other pixel
keeps the clear colour.

One table, TABLE, of (name, C++ expression) generates the texts (grouped in threes) and names the reference's planes, so the two
cannot drift apart.  Every group exists twice: NARROW[g], a text that reads only its group (everything else is dead code: the
kernel loads only what the group reads), and PROBE_ALL, one text that picks the group with `switch ((int)env.constants[63])`, so
that every load of shade_user is live in one kernel.

The reference, fs_in_reference, is Rasterizer.Interpolate (Rasterizer.cs:566-693) in numpy float32 in the operation order of
interpolate_fs_in, built on edge_scenes.Tri (coverage and weights), shade_edge_scenes.vertex_stage / Weights (shared with Shaded) and
geometry_edge_scenes.clip_near (the clipper and its fan).  tests/test_program_probe_host.py holds it against the oracle's
oswr_interpolate word for word.

Scenes: `cells` (64 x 64, one triangle per tile, three different clip.w and clip.z per triangle, half of them on the pixel lattice),
`clipped` (64 x 64, four triangles the near clipper cuts into 3 and into 4 vertices) and `wide` (144 x 80 = 9 x 5 tiles, for
env.x / env.y)."""
from __future__ import annotations

import copy
import dataclasses
import functools
import itertools

import numpy as np

import edge_scenes as E
import geometry_edge_scenes as G
import shade_edge_scenes as S
from edge_scenes import F32, TILE
from softwarerenderer_amd import scenes
from softwarerenderer_amd.rasterizer import BlendMode, CullMode, DepthTest, Program

NAN = float("nan")
CLEAR = (0.1, 0.2, 0.3, 1.0)
NEAR = 0.1


# ============================================================================ the table and the texts
def _members(member, comps):
    return [(f"{member}.{c}", f"in.{member}.{c}") for c in comps]


FS_IN = (_members("clip_position", "xyzw") + _members("color", "xyzw") + _members("tex_coord", "xy") + _members("normal", "xyz") +
         _members("screen_coords", "xy") + _members("barycentric", "xyz") + _members("world_normal", "xyz") + _members("data4", "xyzw"))
assert len(FS_IN) == 4 + 4 + 2 + 3 + 2 + 3 + 3 + 4 == 25
# (env.constants[k] has texts of its own below: CONSTANTS3 reaches all 64)
ENV = [("env.x", "(float)env.x"), ("env.y", "(float)env.y"),
       ("env.tex_w", "(float)env.tex_w"), ("env.tex_h", "(float)env.tex_h"), ("has_texture", "swr_has_texture(env) ? 1.0f : 0.0f")]
TABLE = FS_IN + ENV
assert len(TABLE) % 3 == 0 and len({n for n, _ in TABLE}) == len(TABLE)
GROUPS = [TABLE[i:i + 3] for i in range(0, len(TABLE), 3)]
SELECTOR = 63                       # PROBE_ALL reads its group number from env.constants[63]
ENV_XY_GROUP = next(g for g, grp in enumerate(GROUPS) if "env.x" in [n for n, _ in grp])
TEXTURE_GROUPS = [g for g, grp in enumerate(GROUPS) if any(n == "env.tex_w" for n, _ in grp)]
FS_IN_GROUPS = [g for g in range(len(GROUPS)) if g not in TEXTURE_GROUPS]

HEAD = "__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {\n"


def group_names(g):
    return [n for n, _ in GROUPS[g]]


def _ret(exprs):
    return "return make_float4(" + ", ".join(exprs) + ", 1.0f);"


NARROW = [HEAD + "    " + _ret([e for _, e in grp]) + "\n}\n" for grp in GROUPS]
# (an unknown selector discards: a constant that arrives wrong shows as an uncovered pixel, not as another group's words)
PROBE_ALL = (HEAD + f"    switch ((int)env.constants[{SELECTOR}]) {{\n" +
             "".join(f"    case {g}: {_ret([e for _, e in grp])}\n" for g, grp in enumerate(GROUPS)) +
             "    }\n    return swr_discard();\n}\n")

# constants[3 g .. 3 g + 2] (indices beyond 63 read 63) with g = the triangle's flat vertex colour .x rounded: 22 values of g reach
# every constant, and one draw can hold triangles of several g
N_CONSTANT_GROUPS = 22
CONSTANTS3 = (HEAD + "    int i = 3 * (int)(in.color.x + 0.5f);\n    i = i < 0 ? 0 : i > 63 ? 63 : i;\n"
              "    const int j = i + 1 > 63 ? 63 : i + 1, k = i + 2 > 63 ? 63 : i + 2;\n"
              "    " + _ret(["env.constants[i]", "env.constants[j]", "env.constants[k]"]) + "\n}\n")


def constants3_indices(g):
    i = min(3 * g, 63)
    return i, min(i + 1, 63), min(i + 2, 63)


# fragment identity: 1 / c tells -0 from +0, a bit copy keeps a NaN's payload, c[2] carries one ULP
IDENTITY_CONSTANTS = HEAD + "    " + _ret(["1.0f / env.constants[0]", "__uint_as_float(__float_as_uint(env.constants[1]))",
                                           "env.constants[2]"]) + "\n}\n"
IDENTITY_UNIFORMS = HEAD + "    " + _ret(["1.0f / env.uniforms.fog_start", "__uint_as_float(__float_as_uint(env.uniforms.fog_end))",
                                          "env.uniforms.shininess"]) + "\n}\n"
# Texture.Sample at a uv the program computes itself
SAMPLE_UV = "make_float2(in.tex_coord.y * 3.0f - 1.0f, -in.tex_coord.x)"
SAMPLE_GROUPS = [["sample.x", "sample.y", "sample.z"], ["sample.w", "sample.x", "sample.y"]]
SAMPLE = [HEAD + f"    const float4 s = swr_sample(env, {SAMPLE_UV});\n    " + _ret(["s" + n[6:] for n in grp]) + "\n}\n"
          for grp in SAMPLE_GROUPS]


def all_texts():
    """name -> text of every probe (one compile each)."""
    t = {f"narrow{g}": s for g, s in enumerate(NARROW)}
    t.update(all=PROBE_ALL, constants3=CONSTANTS3, identity_constants=IDENTITY_CONSTANTS, identity_uniforms=IDENTITY_UNIFORMS,
             sample0=SAMPLE[0], sample1=SAMPLE[1])
    return t


# ============================================================================ scenes
def _probe_state(d):
    d.blend, d.depth_test, d.cull, d.texture = BlendMode.None_, DepthTest.LessEqual, CullMode.None_, None
    return d


def _tilted(d, zc):
    """zw_projection with clip.z = zc + x / 8 + y / 16: another clip.z at every vertex (|x|, |y| <= 4: clip.z stays above NEAR * 4)."""
    d.projection = S.zw_projection(zc)
    d.projection[0, 2], d.projection[1, 2] = 0.125, 0.0625
    return d


CELL_W = list(itertools.permutations((1.0, 2.0, 4.0)))
NAN_CELL, CANCEL_CELL = 6, 9
_U = (0.6, 0.0, 0.8)


def _cells_scene(seed, cancel):
    rng = np.random.default_rng(seed)
    c = S.Cells(64, 64, rng, zc=2.0)
    for k in range(c.n_cells):
        kw = dict(half=bool((k + k // 4) & 1), cw=CELL_W[k % 6])
        if k == NAN_CELL:
            kw["nrm"] = [(NAN, 1.0, 0.0), (0.3, -0.2, 0.9), (-0.1, 0.4, 0.7)]
        if k == CANCEL_CELL:                # u at one vertex, -u at the others: N = (2 w - 1) u vanishes where that vertex's weight is 1/2
            cw, j = cancel
            kw.update(half=False, cw=cw, nrm=[_U if i == j else tuple(-v for v in _U) for i in range(3)])
            c.cell(k, **kw)
            continue
        # every other cell is skewed: three different screen x and three different screen y, so that no two vertices can change
        # places unseen (a cell of Cells.cell has two equal x and two equal y)
        q = 0.25 if kw.pop("half") else 0.0
        x0, y0 = TILE * (k % 4) + 4 + q, TILE * (k // 4) + 4 + q
        c.tri_px([(x0, y0 + 1), (x0 + 8, y0), (x0 + 2, y0 + 8)], **kw)
    d = _tilted(_probe_state(c.draw(S.DUST2)), 2.0)
    return scenes.Scene(f"probe_cells_{seed}", 64, 64, [d], clear_color=CLEAR, near_clip=NEAR)


@functools.lru_cache(maxsize=None)
def cells(seed=0):
    """16 one-tile triangles of shade_edge_scenes.Cells, 8 px wide and high: clip.w a permutation of (1, 2, 4), clip.z tilted, half
    on the lattice (vertices and some edge points are samples: a weight of exactly 0) and half a quarter pixel off, three different
    screen x and y per triangle; random distinct colours, uvs and normals; cell NAN_CELL
    has a NaN normal component, cell CANCEL_CELL a world normal that cancels (len_sq <= 1e-6 at a sample: which vertex carries +u
    under which clip.w is found by search, the reference as the judge)."""
    for cancel in itertools.product(CELL_W, range(3)):
        s = _cells_scene(seed, cancel)
        pt = [t for t in probe_tris(s) if t.index == CANCEL_CELL]
        if any((fs_in_reference(s, 0, t, r)["len_sq"] <= F32(1e-6)).any() for t in pt for r in t.rects()):
            return s
    raise AssertionError("cells: no clip.w / normal assignment makes the world normal cancel at a sample")


@functools.lru_cache(maxsize=None)
def clipped(seed=0):
    """Four triangles, one per 32 x 32 quadrant, that enter the near clipper (one or two vertices with w < 0, outside): two leave it
    with 3 vertices, two with 4 (a fan of two).  geometry_edge_scenes.T / draw_of: every triangle is its own draw whose projection
    rows ARE the clip vectors.  Found by seeded search: every fan triangle is drawn, stays inside its quadrant, and no sample is
    covered twice (the fan's shared edge included)."""
    rng = np.random.default_rng(100 + seed)
    W = H = 64
    tris = []
    for q in range(4):
        cx, cy = (-0.5, 0.5)[q % 2], (0.5, -0.5)[q // 2]
        x0, y0 = 32 * (q % 2), 32 * (q // 2)
        n_in = 1 if q in (0, 3) else 2
        for _ in range(20000):
            rows = []
            for i in range(3):
                sign = 1.0 if i < n_in else -1.0
                w = F32(rng.uniform(0.5, 2.0) * sign)
                z = F32(float(F32(NEAR) * w) + rng.uniform(0.2, 1.5) * sign)
                rows.append([F32((cx + rng.uniform(-0.4, 0.4)) * w), F32((cy + rng.uniform(-0.4, 0.4)) * w), z, w])
            col, uv, nrm = G._varyings(rng)
            t = G.rotated(G.T(np.array(rows, dtype=F32), col, uv, nrm, program=Program.Dust2LambertFog, blend=BlendMode.None_,
                              tag=f"probe/n{n_in + 2}"), int(rng.integers(0, 3)))
            c = G.clip_near(G.clips_of_T(t), {}, F32(NEAR), False)
            if c.n != n_in + 2 or G.verdicts(t, F32(NEAR), W, H) != ["drawn"] * (c.n - 2):
                continue
            count = np.zeros((H, W), dtype=np.int32)
            with np.errstate(all="ignore"):
                fans = [E.Tri([c.clips[i] for i in f], W, H, clipper_keeps=True) for f in c.fans]
            for f in fans:
                count += f.frame()[0]
            inside_q = np.zeros((H, W), dtype=bool)
            inside_q[y0 + 1:y0 + 31, x0 + 1:x0 + 31] = True
            if count.max() == 1 and not (count > 0)[~inside_q].any() and all(f.frame()[0].sum() >= 12 for f in fans):
                tris.append(t)
                break
        else:
            raise AssertionError(f"clipped: no triangle found for quadrant {q}")
    return G.make_scene(f"probe_clipped_{seed}", tris, NEAR, W, H)


@functools.lru_cache(maxsize=None)
def wide(seed=0):
    """144 x 80 (9 x 5 tiles: more than one wave of tiles wide, neither side a power of two), two triangles per tile a quarter pixel
    off the lattice, hypotenuses one pixel apart: most of every tile is covered, nothing twice."""
    rng = np.random.default_rng(200 + seed)
    W, H = 144, 80
    c = S.Cells(W, H, rng)
    for ty in range(H // TILE):
        for tx in range(W // TILE):
            x, y = TILE * tx, TILE * ty
            c.tri_px([(x + 0.25, y + 0.25), (x + 15.25, y + 0.25), (x + 0.25, y + 15.25)], z=float(rng.uniform(-0.5, 0.5)))
            c.tri_px([(x + 15.75, y + 15.75), (x + 0.75, y + 15.75), (x + 15.75, y + 0.75)], z=float(rng.uniform(-0.5, 0.5)))
    return scenes.Scene(f"probe_wide_{seed}", W, H, [_probe_state(c.draw(S.DUST2))], clear_color=CLEAR, near_clip=NEAR)


def tile_scene(name, W, H, groups, constants=None, uniforms=None):
    """One batch of one-triangle draws, draw i in tile i of a W x H frame, every vertex coloured (groups[i], 0.5, 0.5, 0.7):
    CONSTANTS3 reads its group number there.  Draw i carries constants[i] (64 floats) / uniforms[i] where given."""
    rng = np.random.default_rng(300)
    draws = []
    for i, g in enumerate(groups):
        c = S.Cells(W, H, rng)
        c.cell(i, half=bool(i & 1), col=[(float(g), 0.5, 0.5, 0.7)] * 3, z=float(rng.uniform(-0.5, 0.5)))
        d = _probe_state(c.draw(S.DUST2))
        if constants is not None:
            d.constants = np.asarray(constants[i], dtype=F32).reshape(64)
        if uniforms is not None:
            d.uniforms = uniforms[i]
        draws.append(d)
    return scenes.Scene(name, W, H, draws, clear_color=CLEAR, near_clip=NEAR)


def constants_scene(W=192, H=96):
    """One batch of three draws of 22 one-tile triangles each (colour .x = g = 0 .. 21), each draw under 64 distinct constants of
    its own: CONSTANTS3 shows constants[3 g .. 3 g + 2] of the draw in triangle g."""
    rng = np.random.default_rng(400)
    draws = []
    for j in range(3):
        c = S.Cells(W, H, rng)
        for g in range(N_CONSTANT_GROUPS):
            k = N_CONSTANT_GROUPS * j + g
            c.cell(k, half=bool(k & 1), col=[(float(g), 0.5, 0.5, 0.7)] * 3, z=float(rng.uniform(-0.5, 0.5)))
        d = _probe_state(c.draw(S.DUST2))
        d.constants = (np.arange(64, dtype=F32) * F32(0.5) + F32(1000.0 * (j + 1))).astype(F32)
        draws.append(d)
    return scenes.Scene("probe_constants", W, H, draws, clear_color=CLEAR, near_clip=NEAR)


def expected_flat(scene, words_of, tris=None):
    """(colour, covered samples) of a frame in which every covered pixel of a triangle shows the three words words_of(ProbeTri) (bit
    patterns kept, NaN payloads included) and w = 1, every other pixel the clear colour."""
    out = np.empty((scene.height, scene.width, 4), dtype=F32)
    out[...] = np.asarray(scene.clear_color, dtype=F32)
    bits = out.view(np.uint32)
    count = np.zeros((scene.height, scene.width), dtype=np.int32)
    for t in (probe_tris(scene) if tris is None else tris):
        w = np.concatenate([np.asarray(words_of(t), dtype=F32).reshape(3), np.ones(1, F32)]).view(np.uint32)
        for sX, eX, sY, eY in t.rects():
            with np.errstate(all="ignore"):
                inside = t.tri.cover((sX, eX, sY, eY))[0]
            bits[sY:eY + 1, sX:eX + 1][inside] = w
            count[sY:eY + 1, sX:eX + 1] += inside
    return out, count


# a 12 x 20 texture (both sides multiples of 4: switched to bilinear it gets a block-linear copy) and a 5 x 7 one (never does)
TEX_12x20, TEX_5x7 = S._texture(12, 20, 7), S._texture(5, 7, 7)
TEXTURE_SETTINGS = (("none", None, False), ("nearest12x20", TEX_12x20, False), ("bilinear12x20", TEX_12x20, True), ("bilinear5x7", TEX_5x7, True))


def with_texture(scene, tex, bilinear=False):
    """A copy of a one-draw scene whose draw samples `tex` (None: no texture)."""
    d = copy.copy(scene.draws[0])
    d.texture = None if tex is None else 0
    return dataclasses.replace(scene, draws=[d], textures=[] if tex is None else [tex], bilinear=bilinear)


def with_constants(scene, constants):
    """A copy of `scene` whose every draw was recorded under `constants`."""
    draws = []
    for d in scene.draws:
        d = copy.copy(d)
        d.constants = np.asarray(constants, dtype=F32).reshape(64)
        draws.append(d)
    return dataclasses.replace(scene, draws=draws)


def selector_constants(g):
    """64 distinct values with PROBE_ALL's selector set to group g."""
    c = (np.arange(64, dtype=F32) * F32(0.25) + F32(100.0)).astype(F32)
    c[SELECTOR] = g
    return c


# ============================================================================ the reference
VARYINGS = ("color", "uv", "normal", "wn")


@dataclasses.dataclass
class ProbeTri:
    """One triangle as DrawTriangle receives it.  `out` = its three outputs IN THE ORDER outputs[0..2] = (v2, v1, v0) (:367), per
    member a (3, k) float32 array: clip, color, uv, normal, wn and, from a user vertex stage, data4.  fan = None for a triangle the
    clipper never saw, else the index triple (0, k, k + 1) into the clipped polygon of `n_poly` vertices."""
    draw: int
    index: int                  # triangle number inside the draw
    vid: tuple
    fan: object
    n_poly: int
    tri: E.Tri
    out: dict

    def rects(self):
        with np.errstate(all="ignore"):
            return [r for _, _, r in self.tri.tiles() if self.tri.cover(r)[0].any()]


def probe_tris(scene, vertex_stage=None, fused=False):
    """Every triangle of the scene that is drawn, after the near clipper and its fan (0, k, k + 1) (Rasterizer.cs:200-223).
    vertex_stage: None = Renderer.VertexShader (S.vertex_stage and the input arrays), else a callable (draw index, draw) -> the
    per-vertex outputs {clip, color, uv, normal, wn, data4} of a user vertex program (tests/vertex_probe_cases.py): data4 then goes
    through the clipper as one more varying.  fused: the clipper's lerp of a SWR_NUMERICS_FMA build."""
    out = []
    near = F32(scene.near_clip)
    for j, d in enumerate(scene.draws):
        if vertex_stage is None:
            clip, wn, _ = S.vertex_stage(d)
            V = d.vertices
            stage = {"clip": clip, "color": V["color"].astype(F32), "uv": V["uv"].astype(F32), "normal": V["normal"].astype(F32), "wn": wn}
        else:
            stage = {k: np.asarray(v, dtype=F32) for k, v in vertex_stage(j, d).items()}
        keys = [k for k in stage if k != "clip"]
        for i, vid in enumerate(d.indices.reshape(-1, 3)):
            vid = [int(v) for v in vid]
            poly = {k: v[vid] for k, v in stage.items()}
            ec = G.enters_clipper(poly["clip"])
            if ec is None:
                continue
            fans, n_poly = [None], 0
            if ec:
                c = G.clip_near(poly["clip"], {k: poly[k] for k in keys}, near, fused)
                poly = dict(c.vary, clip=c.clips)
                fans, n_poly = c.fans, c.n
            for f in fans:
                idx = list(f) if f is not None else [0, 1, 2]
                if G.setup_verdict([poly["clip"][k] for k in idx], scene.width, scene.height, d.cull) != "drawn":
                    continue
                with np.errstate(all="ignore"):
                    t = E.Tri([poly["clip"][k] for k in idx], scene.width, scene.height, clipper_keeps=True)
                o = idx[::-1]
                out.append(ProbeTri(j, i, tuple(vid), f, n_poly, t, {k: np.asarray(v, dtype=F32)[o] for k, v in poly.items()}))
    return out


def texture_words(scene, d):
    """(env.tex_w, env.tex_h, has_texture, width, height) of a draw: the raw words are the layout texture_fetch reads -- tex_h < 0
    for a bilinear texture, tex_w < 0 when its block-linear copy is bound (made for textures whose sides are both multiples of 4)."""
    if d.texture is None:
        return 0, 0, 0, 0, 0
    h, w = scene.textures[d.texture].shape[:2]
    blocked = scene.bilinear and w % 4 == 0 and h % 4 == 0
    return (-w if blocked else w), (-h if scene.bilinear else h), 1, w, h


# wrong restatements of what a user vertex stage hands over (tests/test_vertex_probe_host.py)
VERTEX_MUTANTS = ("data4_w_from_z", "normal_world_normal_swapped", "tex_y_from_wn_x", "data4_renormalised")
MUTANTS = ("clip_w_affine", "barycentric_z_from_sum", "screen_y_from_x", "normal_from_world_normal", "world_normal_always_renormalised")


def fs_in_reference(scene, draw, tri, rect, mutant=None):
    """name -> float32 array over the covered samples of (tri, rect), row-major, for every name of TABLE; plus `inside` (the rect's
    coverage mask), `depth`, `weights` (3, n), `len_sq`, `affine_tex_coord.x` and, with a texture, sample.x .. sample.w.
    Rasterizer.Interpolate (Rasterizer.cs:566-693) in the operation order of interpolate_fs_in (csrc/swr_program.hip.h).
    data4: the outputs' own (tri.out["data4"], from a user vertex stage) summed as (a wa + b wb) + c wc, zeros without one.
    mutant: one of MUTANTS or VERTEX_MUTANTS, a deliberately wrong restatement (tests/test_program_probe_host.py,
    tests/test_vertex_probe_host.py)."""
    assert mutant is None or mutant in MUTANTS + VERTEX_MUTANTS
    d = scene.draws[draw]
    t, o = tri.tri, tri.out
    if mutant in VERTEX_MUTANTS:
        o = {k: v.copy() for k, v in o.items()}
        if mutant == "data4_w_from_z":
            o["data4"][:, 3] = o["data4"][:, 2]
        elif mutant == "normal_world_normal_swapped":
            o["normal"], o["wn"] = o["wn"], o["normal"]
        elif mutant == "tex_y_from_wn_x":
            o["uv"][:, 1] = o["wn"][:, 0]
    one = F32(1.0)
    with np.errstate(all="ignore"):
        k = S.Weights(t, rect, o["clip"][:, 3])                            # :576-585
        n = k.wf.shape[1]

        def member(a):                                                     # Vector2/3/4 members: ((a ra + b rb) + c rc) w, :587-640
            return [k.persp(a[0, i], a[1, i], a[2, i]) for i in range(a.shape[1])]

        def affine(a, b, c):
            return (a * k.wf[0] + b * k.wf[1]) + c * k.wf[2]
        r = {"inside": k.inside, "depth": k.depth[k.inside], "weights": k.wf}
        clip = member(o["clip"])
        if mutant == "clip_w_affine":
            clip[3] = affine(*o["clip"][:, 3])
        normal = member(o["wn"] if mutant == "normal_from_world_normal" else o["normal"])
        # outputs[i].ScreenCoords = screenCoords[i] * (invWidth, invHeight), :362-363, :390
        inv_w, inv_h = one / F32(scene.width - 1), one / F32(scene.height - 1)
        screen = member(np.stack([t.sx * inv_w, (t.sx if mutant == "screen_y_from_x" else t.sy) * inv_h], axis=1).astype(F32))
        bary = [k.wa, k.wb, (one - k.wa) - k.wb if mutant == "barycentric_z_from_sum" else k.wc]              # :583-585, :638
        wn, len_sq = k.world_normal(o["wn"])                               # :680-688
        if mutant == "world_normal_always_renormalised":
            raw = [k.bary(o["wn"][0][i], o["wn"][1][i], o["wn"][2][i]) for i in range(3)]
            wn = [c * (one / np.sqrt(len_sq)) for c in raw]
        uv = member(o["uv"])
        if "data4" in o:                                                   # Vector4 key: weighted sum, nothing else (:690-693)
            data4 = [k.bary(o["data4"][0][i], o["data4"][1][i], o["data4"][2][i]) for i in range(4)]
            if mutant == "data4_renormalised":
                data4[:3] = [c * (one / np.sqrt(S.dot3(data4[:3], data4[:3]))) for c in data4[:3]]
        else:
            data4 = [np.zeros(n, F32)] * 4                                 # no vertex half
        values = clip + member(o["color"]) + uv + normal + screen + bary + wn + data4
        for (name, _), v in zip(FS_IN, values):
            r[name] = np.asarray(v, dtype=F32)
        r["len_sq"] = len_sq
        r["affine_tex_coord.x"] = affine(*o["uv"][:, 0])
        sX, eX, sY, eY = rect
        xs, ys = np.meshgrid(np.arange(sX, eX + 1), np.arange(sY, eY + 1))
        r["env.x"], r["env.y"] = xs[k.inside].astype(F32), ys[k.inside].astype(F32)      # the WINDOW's column and row
        tw = texture_words(scene, d)
        for name, v in zip(("env.tex_w", "env.tex_h", "has_texture"), tw):
            r[name] = np.full(n, v, dtype=F32)
        # swr_sample at SAMPLE_UV (Texture.Sample, Texture.cs:43-63; without a texture Vector4.One)
        su, sv = uv[1] * F32(3.0) - one, -uv[0]
        r["sample_uv"] = np.stack([su, sv], axis=1).astype(F32)
        if d.texture is None:
            s = np.ones((n, 4), F32)
        elif scene.bilinear:
            s = S.texture_bilinear(scene.textures[d.texture], su, sv)
        else:
            s = S.texture_nearest(scene.textures[d.texture], su, sv)[0]
        for i, c in enumerate("xyzw"):
            r["sample." + c] = np.asarray(s[:, i], dtype=F32)
    return r


def expected_planes(scene, mutant=None, tris=None):
    """({name: (H, W) float32 plane}, count): every reference value at its pixel (0 where nothing is covered) and how many
    triangles cover each sample."""
    H, W = scene.height, scene.width
    planes, count = {}, np.zeros((H, W), dtype=np.int32)
    for t in (probe_tris(scene) if tris is None else tris):
        for rect in t.rects():
            r = fs_in_reference(scene, t.draw, t, rect, mutant)
            sX, eX, sY, eY = rect
            count[sY:eY + 1, sX:eX + 1] += r["inside"]
            for name, v in r.items():
                if name in ("inside", "weights", "sample_uv"):
                    continue
                p = planes.setdefault(name, np.zeros((H, W), dtype=F32))
                p[sY:eY + 1, sX:eX + 1][r["inside"]] = v
    return planes, count


def expected_colour(scene, names, planes, count):
    """The colour plane a probe of `names` (three of them) leaves: the words at covered pixels, w = 1, the clear colour elsewhere."""
    out = np.empty((scene.height, scene.width, 4), dtype=F32)
    out[...] = np.asarray(scene.clear_color, dtype=F32)
    cov = count > 0
    for i, n in enumerate(names):
        out[..., i][cov] = planes[n][cov]
    out[..., 3][cov] = 1.0
    return out
