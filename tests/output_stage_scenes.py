"""Scenes that put the OUTPUT STAGE of filled triangles -- what RasterizeTriangle does with a fragment once it is shaded
(Rasterizer.cs:502-523): the depth function, the `W > 0` gate, the blend, the conditional Z write and, under BlendMode.None, the
`break` that ends the row -- where its decisions fall; a numpy-float32 restatement of that stage that says, per fragment, whether
it was visited, failed the depth test, failed the gate or was never visited; and a planner that says on which lane of which
64-fragment chunk of k_raster_c (csrc/swr_raster_c.hip.h) a fragment lands.  tests/test_output_stage_host.py asserts on the CPU that
the restatement IS the oracle's frame and that every family reaches what it is for; tests/test_gpu_output_stage.py renders the scenes.

  O1  depth ties: a writer cell stores an exact word at its vertex samples, a tester cell puts the same word, one ulp beside it,
      33 / 34 steps of 2^-25 beside it (|nd - od| on either side of 1e-6) and a far value there under each of the eight depth
      tests, and a probe cell under LessEqual shows whether the tester wrote Z; nz = -FLT_MAX over the clear (nd - od = +Inf)
  O2  the gate and the blend: vertex alphas +-0, +-1e-45, -1, 1, 2, +-Inf, NaN on Gouraud vertex samples and whole FlatColor
      cells under the four blend modes x {LessEqual, Always}, each followed by a farther LessEqual probe; non-finite, negative,
      > 1 and subnormal source colours over ordinary and non-finite destinations; random 24-bit mantissas under Alpha
  O3  row kills at chunk seams (BlendMode.None, one draw, one tile, no shared pixel): prefix cells shift a target cell so that the
      failing fragment of its row lands on stream position 62, 63, 64 or 65
  O4  kills and the depth test: an alpha failure on a fragment that fails depth must not kill, one that passes depth must
  O5  shared pixels: twin cells, up to 130 one-pixel triangles on one pixel, depth staircases, every depth test
  O6  draw boundaries inside the early-out kernel: None / Alpha / Additive / None draws over neighbouring rows

Geometry.  A `cell` is a right triangle with its right angle on an integer pixel and legs of `leg` px along +x and +y
(edge_scenes.clip_pos, identity matrices, clip.w = 1): it covers the (leg + 1)(leg + 2) / 2 samples with i + j <= leg, its three
vertices are samples whose weights are exactly (-1, 0, 0) -- the reference's edge values and its area have opposite signs for
every triangle, Rasterizer.cs:427, :481-483 -- so the depth stored there is the vertex's own word NEGATED, -((nz + 1) * 0.5): a
larger nz is a SMALLER stored word.  Triangles are given in OUTPUTS order (s0, s1, s2) = (right angle, +x end, +y end), as in wireframe_edge_scenes.

What the filled path cannot reach (asserted in the host tests):
  * a non-finite fragment depth below the magnitudes edge_scenes' F3 covers: after setup the depth is d0 w0 + d1 w1 + d2 w2 with
    finite depths[i] of at most 2^127 in magnitude ((nz + 1) * 0.5, nz finite) and weights of one sign that sum to -1 within
    rounding; there is no division.  The largest depths that exist (nz = +-FLT_MAX) give finite fragment depths everywhere (O1's
    `inf` rung), so NaN / Inf depths need overflowing edge values, i.e. screen coordinates beyond 1e19: F3's ground.
  * |nd - od| EXACTLY equal to float32(1e-6) (0x358637bd, an odd multiple of 2^-43) at a vertex sample or inside a cell: vertex
    depths are multiples of 2^-25 and a cell's weights are eighths.  The seeded search over interpolated samples of cells comes
    within 2e-9 on either side and never onto it; the `exactly_epsilon` scenes reach it with a triangle of doubled area 5^6.
"""
from __future__ import annotations

import dataclasses
import functools
import os
import re
from dataclasses import dataclass
from typing import List

import numpy as np

import edge_scenes as E
import shade_edge_scenes as S
import wireframe_edge_scenes as Wf
from softwarerenderer_amd import scenes
from softwarerenderer_amd.rasterizer import BlendMode, DepthTest, Program
from wireframe_edge_scenes import V

F32 = np.float32
TILE = 16
CHUNK = 64
CLEAR = (0.1, 0.2, 0.3, 0.75)
FLOAT_MIN = E.FLOAT_MIN
FLT_MAX = S.FLT_MAX
EPSILON = Wf.EPSILON
NAN, INF = float("nan"), float("inf")
SUB = 1e-45                                     # the smallest subnormal, 2^-149
ALL_DEPTH_TESTS = tuple(DepthTest)
ALL_BLENDS = tuple(BlendMode)
VISITED, DEPTH_FAILED, GATE_FAILED, KILLED = 0, 1, 2, 3         # per-fragment flags (VISITED = shaded and written)
RASTER_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "softwarerenderer_amd", "csrc", "swr_raster_c.hip.h")


def kernel_constants():
    """SWR_BATCH, SWR_BATCH_FRAGS, SWR_WINDOW as csrc/swr_raster_c.hip.h defines them."""
    text = open(RASTER_HEADER).read()
    return tuple(int(re.search(rf"^#define {k}\s+(\d+)", text, re.M).group(1)) for k in ("SWR_BATCH", "SWR_BATCH_FRAGS", "SWR_WINDOW"))


# =============================================================================================== building
def cell(x, y, leg=8, z=0.0, rgba=(1.0, 1.0, 1.0, 1.0)):
    """z: one nz or three (right angle, +x end, +y end); rgba: one colour or a list of three."""
    zs = list(z) if isinstance(z, (list, tuple)) else [z] * 3
    cs = list(rgba) if isinstance(rgba, list) else [rgba] * 3
    return (V(x, y, zs[0], tuple(cs[0])), V(x + leg, y, zs[1], tuple(cs[1])), V(x, y + leg, zs[2], tuple(cs[2])))


def pixel(x, y, z=0.0, rgba=(1.0, 1.0, 1.0, 1.0)):
    """A triangle that covers the one sample (x, y): quarter-pixel vertices, exact on a power-of-two target."""
    return (V(x - 0.25, y - 0.25, z, tuple(rgba)), V(x + 0.5, y - 0.25, z, tuple(rgba)), V(x - 0.25, y + 0.5, z, tuple(rgba)))


def draw(tris, W, H, depth_test, blend, program=Program.Gouraud):
    return Wf._triangle_draw(list(tris), W, H, program=program, depth_test=depth_test, blend=blend)


def _scene(name, W, H, draws):
    assert W <= 64 and H <= 64
    return scenes.Scene("out_" + name, W, H, list(draws), clear_color=CLEAR)


def _rgb(rng, a=1.0):
    return (*(float(v) for v in rng.uniform(0.1, 0.9, 3)), a)


def nz_of_depth_steps(nz0, steps):
    """nz whose depth word is `steps` depth-ulps of 2^-25 away from that of nz0 (nz0 in [-1, -0.5): nz moves in 2^-24)."""
    return float(F32(F32(nz0) + F32(steps * 2.0 ** -24)))


def depth_word(nz):
    """The word a vertex sample with this nz stores: the weights there are (-1, 0, 0)."""
    return F32(-F32(F32(F32(nz) + F32(1.0)) * F32(0.5)))


# =============================================================================================== O1
O1_NZ0 = -1.0 + 2.0 ** -10                      # writer of the 2^-25 ladder: word -2^-11, vertex words move in steps of 2^-25
O1_NZ1 = -0.375                                 # writer of the 1-ulp rungs: word -0.3125, whose neighbours -0.3125 +- 2^-25 exist
# rung -> (writer nz or None for the cleared word, tester nz).  above / below: the tester's STORED word against the writer's (a
# smaller nz is a larger word); `far`: 2^-4 away.
O1_RUNGS = {
    "same": (O1_NZ1, O1_NZ1), "ulp_above": (O1_NZ1, O1_NZ1 - 2.0 ** -24), "ulp_below": (O1_NZ1, O1_NZ1 + 2.0 ** -24),
    "33_above": (O1_NZ0, nz_of_depth_steps(O1_NZ0, -33)), "33_below": (O1_NZ0, nz_of_depth_steps(O1_NZ0, 33)),
    "34_above": (O1_NZ0, nz_of_depth_steps(O1_NZ0, -34)), "34_below": (O1_NZ0, nz_of_depth_steps(O1_NZ0, 34)),
    "far_above": (O1_NZ0, O1_NZ0 - 2.0 ** -11), "far_below": (O1_NZ0, O1_NZ0 + 0.125),
    "inf": (None, -FLT_MAX),
}
# tile -> the rungs at the tester's (right angle, +x end, +y end)
O1_TILES = (("same", "ulp_above", "ulp_below"), ("33_above", "33_below", "34_above"), ("34_below", "far_above", "far_below"), ("inf", "inf", "inf"))
O1_AT = (3, 3)                                  # the cells' right angle inside their tile


def o1_vertex_pixels():
    """rung -> (x, y) of the vertex sample that carries it."""
    out = {}
    for k, rungs in enumerate(O1_TILES):
        x, y = TILE * (k % 2) + O1_AT[0], TILE * (k // 2) + O1_AT[1]
        for r, (dx, dy) in zip(rungs, ((0, 0), (8, 0), (0, 8))):
            out.setdefault(r, (x + dx, y + dy))
    return out


def _o1_scene(name, dt, rng, writer_state=(DepthTest.Always, BlendMode.None_), tester_z=None, writer_z=None):
    W = H = 32
    writers, testers, probes = [], [], []
    for k, rungs in enumerate(O1_TILES):
        x, y = TILE * (k % 2) + O1_AT[0], TILE * (k // 2) + O1_AT[1]
        wz = O1_RUNGS[rungs[0]][0] if writer_z is None else writer_z
        tz = [O1_RUNGS[r][1] for r in rungs] if tester_z is None else list(tester_z[k])
        if wz is not None:
            writers.append(cell(x, y, z=wz, rgba=_rgb(rng)))
        testers.append(cell(x, y, z=tz, rgba=[_rgb(rng, 0.5) for _ in range(3)]))
        # the probe passes LessEqual (nd >= od) at a vertex exactly when the tester wrote there (tester below the writer) or
        # did not (tester above it): its word is the smaller of the two, i.e. its nz the larger; over the clear: any finite word
        pz = [max(t, wz) if wz is not None else 0.0 for t in tz]
        probes.append(cell(x, y, z=pz, rgba=[_rgb(rng, 0.5) for _ in range(3)]))
    draws = [draw(writers, W, H, *writer_state), draw(testers, W, H, dt, BlendMode.Alpha), draw(probes, W, H, DepthTest.LessEqual, BlendMode.Alpha)]
    return _scene(name, W, H, draws)


def o1_search(seed=0, trials=4000):
    """Seeded search over INTERPOLATED samples for |nd - od| nearer to float32(1e-6) than the 33 / 34-step rungs: the writer is the
    constant O1_NZ0 cell, the tester's three nz are random within +-3e-6 of it.  Returns (below, above, hit): the nearest |nd - od|
    found on each side with the tester's nz triple, and whether a difference equal to float32(1e-6) was met."""
    rng = np.random.default_rng(9100 + seed)
    W = H = 32
    x, y = O1_AT
    def tri(zs):
        pts = ((x, y + 8), (x + 8, y), (x, y))                     # submission order v0 = s2, v1 = s1, v2 = s0
        return E.Tri([np.array([*E.clip_pos(px, py, W, H), z, 1.0], dtype=F32) for (px, py), z in zip(pts, zs[::-1])], W, H)
    wt = tri([O1_NZ0] * 3)
    rect = wt.rect(0, 0)
    ins, od, _ = wt.cover(rect)
    vertex = np.zeros(ins.shape, bool)
    for (vx, vy) in ((x, y), (x + 8, y), (x, y + 8)):
        vertex[vy - rect[2], vx - rect[0]] = True
    best = {"below": (F32(0.0), None), "above": (F32(np.inf), None)}
    hit = False
    for _ in range(trials):
        zs = [float(F32(O1_NZ0 + s * rng.uniform(1.2e-6, 3.0e-6))) for s in rng.choice([-1.0, 1.0], 3)]
        _, nd, _ = tri(zs).cover(rect)
        diff = np.abs((nd - od).astype(F32))[ins & ~vertex]
        hit = hit or bool((diff == EPSILON).any())
        lo = diff[diff < EPSILON]
        hi = diff[diff >= EPSILON]
        if lo.size and lo.max() > best["below"][0]:
            best["below"] = (lo.max(), tuple(zs))
        if hi.size and hi.min() < best["above"][0]:
            best["above"] = (hi.min(), tuple(zs))
    return best["below"], best["above"], hit


# |nd - od| EXACTLY float32(1e-6).  1e-6 = (2^19 / 5^6) 2^-25, so with vertex words m 2^-25 the difference is 1e-6 in real arithmetic
# where (sum m_i a_i) / A - k = 2^19 / 5^6 for integer weights a_i / A: a triangle of doubled area A = 15625 = 125 x 125.  This one --
# (-30, -20), (95, -20), (-29, 105), words 80, 79, 84 over a constant 47 -- has a solution at pixel (53, 18), and there the float32
# roundings of both depths leave the difference on float32(1e-6) itself (found by a directed search, asserted in the host tests).
O1_EXACT_TRIANGLE = ((-30.0, -20.0), (95.0, -20.0), (-29.0, 105.0))
O1_EXACT_WORDS = (80, 79, 84)
O1_EXACT_WRITER = 47
O1_EXACT_PIXEL = (53, 18)


def _o1_exact_scene(dt, rng):
    W = H = 64
    nz = lambda m: float(F32(F32(-1.0) + F32(m * 2.0 ** -24)))
    def tri(ms, a):
        return tuple(V(x, y, nz(m), _rgb(rng, a)) for (x, y), m in zip(O1_EXACT_TRIANGLE, ms))
    return _scene(f"o1_exactly_epsilon_{dt.name}", W, H, [draw([tri([O1_EXACT_WRITER] * 3, 1.0)], W, H, DepthTest.Always, BlendMode.None_),
                                                           draw([tri(O1_EXACT_WORDS, 0.5)], W, H, dt, BlendMode.Alpha)])


@functools.lru_cache(maxsize=None)
def o1_depth_ties(seed=0):
    rng = np.random.default_rng(9000 + seed)
    out = [_o1_scene(f"o1_{dt.name}", dt, rng) for dt in ALL_DEPTH_TESTS]
    # everything Alpha / LessEqual: the compile-time BLEND / DT kernel (gouraud_default); the writer passes over the clear
    out.append(_o1_scene("o1_LessEqual_default", DepthTest.LessEqual, rng, writer_state=(DepthTest.LessEqual, BlendMode.Alpha)))
    below, above, _ = o1_search(seed)
    for dt in (DepthTest.Equal, DepthTest.NotEqual):
        tz = [below[1], above[1], below[1], above[1]]
        out.append(_o1_scene(f"o1_searched_{dt.name}", dt, rng, tester_z=tz, writer_z=O1_NZ0))     # the writer the search ran against
        out.append(_o1_exact_scene(dt, rng))
    return out


# =============================================================================================== O2
O2_ALPHAS = (("plus_zero", 0.0), ("minus_zero", -0.0), ("plus_sub", SUB), ("minus_sub", -SUB), ("minus_one", -1.0), ("one", 1.0),
             ("two", 2.0), ("plus_inf", INF), ("minus_inf", -INF), ("nan", NAN))
O2_COLOURS = (("nan", (NAN, 0.5, NAN)), ("plus_inf", (INF, 0.5, INF)), ("minus_inf", (-INF, 0.25, -INF)), ("above_one", (1.5, 7.0, 3.0e38)),
              ("negative", (-0.5, -2.0, -0.0)), ("subnormal", (1e-38, 2e-45, 1e-30)))
O2_DST = (("ordinary", None), ("nonfinite", (NAN, INF, -INF, 0.5)), ("zero", (0.0, -0.0, 0.0, 0.0)))


def _o2_tile(k, off=(1, 1)):
    return TILE * (k % 4) + off[0], TILE * (k // 4) + off[1]


def _o2_alpha_scene(blend, dt, flat, rng):
    """One tile per alpha.  Gouraud: the alpha sits at the right angle's vertex sample (0.5 and 0.75 at the others); FlatColor: on
    all three vertices, the cell's 45 fragments carry the word as it is.  Then the probe: the same cells, farther, LessEqual."""
    W = H = 64
    prog = Program.FlatColor if flat else Program.Gouraud
    cells, probes = [], []
    for k, (_, a) in enumerate(O2_ALPHAS):
        x, y = _o2_tile(k)
        al = [a, a, a] if flat else [a, 0.5, 0.75]
        cells.append(cell(x, y, z=0.0, rgba=[(*_rgb(rng)[:3], al[i]) for i in range(3)]))
        probes.append(cell(x, y, z=0.5, rgba=[_rgb(rng, 0.5) for _ in range(3)]))
    return _scene(f"o2_alpha_{'flat' if flat else 'gouraud'}_{blend.name}_{dt.name}", W, H,
                  [draw(cells, W, H, dt, blend, prog), draw(probes, W, H, DepthTest.LessEqual, BlendMode.Alpha, prog)])


def _o2_colour_scenes():
    """Per blend mode two scenes (four and two columns of O2_COLOURS).  Tile (row = destination, column = source colour): a first
    FlatColor / None / Always layer leaves the destination, the second layer brings the source colour with alpha 0.5 (Alpha:
    both products; Multiply: Inf * 0 over the `zero` destination)."""
    out = []
    for blend in ALL_BLENDS:
        for half, colours in enumerate((O2_COLOURS[:4], O2_COLOURS[4:])):
            first, second = [], []
            for r, (_, dst) in enumerate(O2_DST):
                for c, (_, rgb) in enumerate(colours):
                    x, y = TILE * c + 1, TILE * r + 1
                    if dst is not None:
                        first.append(cell(x, y, z=0.5, rgba=dst[:3] + (1.0,)))    # (alpha 1 passes the gate; None writes rgb as it is)
                    second.append(cell(x, y, z=0.0, rgba=(*rgb, 0.5)))
            out.append(_scene(f"o2_colour_{blend.name}_{half}", 64, 64,
                              [draw(first, 64, 64, DepthTest.Always, BlendMode.None_, Program.FlatColor),
                               draw(second, 64, 64, DepthTest.LessEqual, blend, Program.FlatColor)]))
    return out


def _mantissa(rng, lo=-2, hi=1):
    """A float32 with a random 24-bit significand and an exponent in [lo, hi)."""
    return float(np.ldexp(F32((1 << 23) + int(rng.integers(0, 1 << 23))) , int(rng.integers(lo, hi)) - 23))


def _o2_random_alpha(rng):
    """Sixteen FlatColor cells over a first layer of random 24-bit significands.  Cells 0..7: random sources, where a contracted
    s * a + d * ia moves the last bit.  Cells 8..15: sources s = -(d * ia) / a, so that the two products cancel and the rounding
    error of s * a, which fmaf does not make, is most of the result: many ULPs, far outside the colour bar."""
    W = H = 64
    first, second = [], []
    for k in range(16):
        x, y = _o2_tile(k)
        dst = [_mantissa(rng) for _ in range(3)]
        a = _mantissa(rng, -2, 0)
        if k < 8:
            src = [_mantissa(rng) for _ in range(3)]
        else:
            ia = F32(F32(1.0) - F32(a))
            src = [float(F32(-F32(F32(d) * ia) / F32(a))) for d in dst]
        first.append(cell(x, y, z=0.5, rgba=(*dst, 1.0)))
        second.append(cell(x, y, z=0.0, rgba=(*src, a)))
    return _scene("o2_random_mantissas_Alpha", W, H, [draw(first, W, H, DepthTest.Always, BlendMode.None_, Program.FlatColor),
                                                      draw(second, W, H, DepthTest.LessEqual, BlendMode.Alpha, Program.FlatColor)])


@functools.lru_cache(maxsize=None)
def o2_gate_and_blend(seed=0):
    rng = np.random.default_rng(9200 + seed)
    out = [_o2_alpha_scene(b, dt, flat, rng) for b in ALL_BLENDS for dt in (DepthTest.LessEqual, DepthTest.Always) for flat in (False, True)]
    out += _o2_colour_scenes()
    out.append(_o2_random_alpha(rng))
    return out


# =============================================================================================== O3
LEG_FRAGS = {leg: (leg + 1) * (leg + 2) // 2 for leg in range(1, 9)}        # 3, 6, 10, 15, 21, 28, 36, 45
O3_DEPTH_TESTS = (DepthTest.Always, DepthTest.Disabled, DepthTest.LessEqual)
# how the target's alpha fails: name -> (alphas at (right angle, +x end, +y end), stream index of row 0's failing fragment in a leg-8 cell)
O3_FAIL = {"first": ((0.0, 1.0, 1.0), 0),           # +0 at the right angle: the row's first covered pixel, the whole row unvisited
           "last": ((1.0, 0.0, 1.0), 8),            # +0 at the +x end: the row's last covered pixel, nothing killed
           "apex": ((1.0, 1.0, 0.0), 44),           # +0 at the +y end: the pair's last fragment, a one-pixel row
           "sign": ((3.0, -5.0, 3.0), 3)}           # alpha = 3 - i along every row: exactly 0 at i = 3, negative beyond
# rung -> (legs of the prefix cells in stream order, kind of failure, lane the failing fragment must land on)
O3_RUNGS = {
    "first_on_62": ((6, 6, 2), "first", 62), "first_on_63_victims_next_chunk": ((8, 4, 1), "first", 63),
    "first_on_0": ((8, 3, 2, 1), "first", 0), "first_on_1": ((8, 3, 3), "first", 1),
    "last_on_62": ((8, 2, 1), "last", 62), "last_on_63": ((8, 3), "last", 63), "last_on_0": ((7, 3, 3), "last", 0), "last_on_1": ((7, 5), "last", 1),
    "sign_on_62": ((6, 5, 3), "sign", 62), "sign_on_63": ((8, 4), "sign", 63), "sign_on_0": ((8, 3, 2), "sign", 0), "sign_on_1": ((6, 6, 2), "sign", 1),
    # the dead row 0 ends exactly on lane 63 (P + 8 = 63); row 1 of the same pair starts on lane 0 and must live
    "dead_row_ends_on_63_new_row_on_0": ((8, 3), "first", 55),
    # the dead row goes on across the seam: failure on lane 60, victims on 61..63 and on 0..4 of the next chunk
    "dead_row_crosses_the_seam": ((8, 4), "first", 60),
}


def _pack(items, W=TILE, H=TILE):
    """Positions for cells of the given legs (right angle top left) so that no two share a pixel: `items` are (leg, fixed (x, y) or
    None); fixed ones first, the others first-fit, row by row."""
    taken = np.zeros((H, W), bool)
    pos = [None] * len(items)
    def shape(leg):
        return [(i, j) for j in range(leg + 1) for i in range(leg + 1 - j)]
    def fits(x, y, leg):
        return x + leg < W and y + leg < H and not any(taken[y + j, x + i] for i, j in shape(leg))
    def take(x, y, leg):
        for i, j in shape(leg):
            taken[y + j, x + i] = True
    order = [k for k, it in enumerate(items) if it[1] is not None] + sorted((k for k, it in enumerate(items) if it[1] is None), key=lambda k: -items[k][0])
    for k in order:
        leg, at = items[k]
        if at is not None:
            assert fits(*at, leg), (items, k)
            pos[k] = at
        else:
            pos[k] = next(((x, y) for y in range(H) for x in range(W) if fits(x, y, leg)), None)
            assert pos[k] is not None, f"no room for a cell of leg {leg}: {items}"
        take(*pos[k], leg)
    return pos


def _o3_cells(rng, items, alphas):
    """items: (leg, fixed position or None) in stream order; alphas: per item the three vertex alphas (None: all 1)."""
    W = max(TILE, max((it[1][0] + it[0] + 1 for it in items if it[1] is not None), default=TILE))
    H = max(TILE, max((it[1][1] + it[0] + 1 for it in items if it[1] is not None), default=TILE))
    W, H = TILE * ((W + TILE - 1) // TILE), TILE * ((H + TILE - 1) // TILE)
    pos = _pack(items, W=W, H=H)
    tris = []
    for (leg, _), (x, y), al in zip(items, pos, alphas):
        al = al or (1.0, 1.0, 1.0)
        tris.append(cell(x, y, leg, z=float(rng.uniform(-0.5, 0.5)), rgba=[(*_rgb(rng)[:3], float(a)) for a in al]))
    return tris, W


def _o3_scene(name, dt, tris, W=TILE, H=None, program=Program.Gouraud):
    H = H or W                                              # (one tile, or the 32 x 32 frame of the two-tile rung)
    return _scene(name, W, H, [draw(tris, W, H, dt, BlendMode.None_, program)])


def o3_configs(rng):
    """name -> (triangles in stream order, width, index of the target triangle(s) whose rows are looked at)."""
    out = {}
    for rung, (legs, kind, lane) in O3_RUNGS.items():
        items = [(leg, None) for leg in legs] + [(8, None)]
        tris, W = _o3_cells(rng, items, [None] * len(legs) + [O3_FAIL[kind][0]])
        out[rung] = (tris, W, len(legs))
    # the pair's last fragment (its apex, tile row y + 8) fails on lane 63; the NEXT pair's first row is the same tile row, on lane 0
    items = [(3, None), (2, None), (1, None), (8, (0, 0)), (3, (9, 8))]
    tris, W = _o3_cells(rng, items, [None, None, None, O3_FAIL["apex"][0], None])
    out["same_row_number_in_the_next_pair_on_0"] = (tris, W, 3)
    # a row that dies in the left tile of a triangle spanning two: columns 10..15 in tile 0, 16..18 in tile 1; once per tile row
    # (a 32 x 32 frame: it can be cut into two bands)
    items = [(8, (10, 2)), (4, None), (8, (10, 18))]
    tris, W = _o3_cells(rng, items, [O3_FAIL["first"][0], None, O3_FAIL["first"][0]])
    assert W == 32
    out["row_dies_in_the_left_tile"] = (tris, W, 0)
    return out


def _o3_batch_scenes(rng, dt):
    """(a) 16-pair batch: 15 cells of leg 1, then a leg-2 cell whose apex (its last fragment, the batch's last) fails, then -- first
    pair of the next batch -- a cell whose first row is the same tile row and must live, with a sign change further down.
    (b) 2048-fragment batch: eight triangles over the whole tile (8 x 256 fragments; pixels shared, so plan.exact is false, but a
    chunk of 64 never holds two of them), the eighth with alpha 3 - x / 2 (dead from column 6 in every row, row 15 to the batch's
    end); the ninth pair starts the next batch in tile row 15."""
    items = [(1, None)] * 15 + [(2, (0, 5)), (6, (1, 7))]
    tris, W = _o3_cells(rng, items, [None] * 15 + [O3_FAIL["apex"][0], (3.0, -3.0, 3.0)])
    a = _o3_scene(f"o3_batch_of_16_pairs_{dt.name}", dt, tris)
    big = []
    for k in range(8):
        al = (3.0, -13.0, 3.0) if k == 7 else (1.0, 1.0, 1.0)            # 32 px legs: alpha = 3 - x / 2 at column x
        big.append(cell(0, 0, 32, z=0.5 - 0.1 * k, rgba=[(*_rgb(rng)[:3], a_) for a_ in al]))
    big.append(cell(3, 15, 8, z=-0.5, rgba=_rgb(rng)))
    b = _o3_scene(f"o3_batch_of_2048_fragments_{dt.name}", dt, big)
    return [a, b]


@functools.lru_cache(maxsize=None)
def o3_row_kills(seed=0):
    out = []
    for dt in O3_DEPTH_TESTS:
        rng = np.random.default_rng(9300 + seed)
        for rung, (tris, W, _) in o3_configs(rng).items():
            out.append(_o3_scene(f"o3_{rung}_{dt.name}", dt, tris, W))
        out += _o3_batch_scenes(rng, dt)
    return out


# =============================================================================================== O4
O4_DEPTH_TESTS = (DepthTest.Less, DepthTest.LessEqual, DepthTest.Greater, DepthTest.GreaterEqual, DepthTest.NotEqual, DepthTest.Equal)
O4_OCCLUDERS = 9                                # 9 x 256 fragments > SWR_BATCH_FRAGS: the testers meet a written tile at batch start


def _o4_scene(dt, rng):
    """Two tiles.  The occluder: nine triangles over the whole frame at depth -0.5 (None; under Always, but in the Less and LessEqual
    scenes under LessEqual -- level words pass at ties, the frame is the same -- so that EVERY draw of the batch is Less / LessEqual,
    depth_only_grows is 1 and generic_none runs with hi-Z on).  Testers (None, `dt`): leg-8 cells
    whose stored depth runs from -0.75 to -0.25 along x (-0.5 exactly at i = 4; Greater / GreaterEqual: from -0.25 to -0.75), so part of each
    row is in front of the stored depth and part behind; their alpha is linear in x as well (weights in eighths: all exact):
      A  alpha = i / 2 - 1 (<= 0 for i <= 2): the failures sit where the depth test fails -- no kill, the rest of the row is written
      B  alpha = 3 - i / 2 (<= 0 for i >= 6): the failure at i = 6 passes depth -- i = 7, 8 are never visited
      C  alpha = 4 - i: 0 at i = 4 (the tie) and negative beyond -- Equal passes only at i = 4 and dies there, NotEqual fails at
         i = 4 (no kill) and dies at i = 5
      D  entirely behind the occluder (depth -0.875), alpha 1: in the Less / LessEqual scenes its batch starts over a tile whose minimum
         is -0.5 (eight of the nine occluders fill the batch before), k_cover's bound of D lies below that, and hi-Z drops the pair:
         its 15 fragments must still count as tested.  (Under the other four tests an Always draw is in the batch: hi-Z is off.)"""
    W, H = 2 * TILE, TILE
    occ = [cell(0, 0, 64, z=0.0, rgba=_rgb(rng)) for _ in range(O4_OCCLUDERS)]
    grows = dt in (DepthTest.Less, DepthTest.LessEqual)
    zl, zr = (0.5, -0.5) if dt not in (DepthTest.Greater, DepthTest.GreaterEqual) else (-0.5, 0.5)
    def tester(x, y, a0, a1):
        return cell(x, y, 8, z=[zl, zr, zl], rgba=[(*_rgb(rng)[:3], a0), (*_rgb(rng)[:3], a1), (*_rgb(rng)[:3], a0)])
    testers = [tester(0, 0, -1.0, 3.0), tester(7, 2, 3.0, -1.0), tester(16, 0, 4.0, -4.0)]
    behind = cell(23, 9, 4, z=0.75, rgba=_rgb(rng))
    return _scene(f"o4_{dt.name}", W, H, [draw(occ, W, H, DepthTest.LessEqual if grows else DepthTest.Always, BlendMode.None_),
                                               draw(testers + [behind], W, H, dt, BlendMode.None_)])


@functools.lru_cache(maxsize=None)
def o4_kills_and_depth(seed=0):
    rng = np.random.default_rng(9400 + seed)
    return [_o4_scene(dt, rng) for dt in O4_DEPTH_TESTS]


# =============================================================================================== O5
O5_STACKS = (2, 63, 64, 65)
O5_BIG_STACK = 130


def _staircase(kind, n, k):
    """nz of copy k of n: stored words going up from -0.75 to the background's -0.5, down from -0.25 to it, level with it, or from it
    down to -0.75 (`deeper`: every copy passes Greater / GreaterEqual)."""
    return {"up": 0.5 - k / (2.0 * n), "down": -0.5 + k / (2.0 * n), "level": 0.0, "deeper": k / (2.0 * n)}[kind]


def _o5_background(rng, W, H):
    """Always / Alpha over the whole frame at depth -0.5: without it Greater, GreaterEqual and Equal pass nothing over the clear."""
    return draw([cell(0, 0, 64, z=0.0, rgba=_rgb(rng, 0.5))], W, H, DepthTest.Always, BlendMode.Alpha)


def _o5_tris(rng, alphas=lambda k: 0.6):
    tris = []
    for copies, (x, y), kind in ((5, (0, 0), "up"), (3, (7, 2), "down"), (2, (0, 9), "level")):
        leg = 8 if copies != 2 else 6
        for k in range(copies):
            a = alphas(k)
            tris.append(cell(x, y, leg, z=_staircase(kind, copies, k), rgba=[(*_rgb(rng)[:3], a), (*_rgb(rng)[:3], alphas(k + 1)), (*_rgb(rng)[:3], a)]))
    for n, (x, y), kind in zip(O5_STACKS, ((12, 12), (13, 13), (14, 14), (15, 15)), ("level", "up", "down", "level")):
        for k in range(n):
            tris.append(pixel(x, y, z=_staircase(kind, n, k), rgba=(*_rgb(rng)[:3], alphas(k))))
    return tris


@functools.lru_cache(maxsize=None)
def o5_shared_pixels(seed=0):
    W = H = TILE
    out = []
    for dt in ALL_DEPTH_TESTS:
        rng = np.random.default_rng(9500 + seed)
        out.append(_scene(f"o5_Alpha_{dt.name}", W, H, [_o5_background(rng, W, H), draw(_o5_tris(rng), W, H, dt, BlendMode.Alpha)]))
    for dt in (DepthTest.Always, DepthTest.LessEqual, DepthTest.Equal):
        rng = np.random.default_rng(9550 + seed)
        alt = lambda k: 1.0 if k % 2 == 0 else 0.0                          # every other copy fails the gate
        out.append(_scene(f"o5_None_alternating_{dt.name}", W, H, [_o5_background(rng, W, H), draw(_o5_tris(rng, alt), W, H, dt, BlendMode.None_)]))
    for blend, dt in ((BlendMode.Alpha, DepthTest.LessEqual), (BlendMode.Additive, DepthTest.Always), (BlendMode.None_, DepthTest.GreaterEqual)):
        rng = np.random.default_rng(9560 + seed)
        H = 2 * TILE                                        # a stack in each of two tile rows: the frame can be cut into two bands
        tris = [pixel(5, 6 + 16 * (k % 2), z=_staircase("level" if blend != BlendMode.None_ else "deeper", O5_BIG_STACK, k),
                      rgba=(*_rgb(rng)[:3], 0.0 if (blend == BlendMode.None_ and k % 3 == 1) else 0.6)) for k in range(2 * O5_BIG_STACK)]
        out.append(_scene(f"o5_stack_of_{O5_BIG_STACK}_{blend.name}_{dt.name}", W, H, [_o5_background(rng, W, H), draw(tris, W, H, dt, blend)]))
    return out


# =============================================================================================== O6
O6_BLENDS = (BlendMode.None_, BlendMode.Alpha, BlendMode.Additive, BlendMode.None_, BlendMode.Multiply)


@functools.lru_cache(maxsize=None)
def o6_draw_boundaries(seed=0):
    """Five draws of one leg-3 cell each down the diagonal of one tile, None / Alpha / Additive / None / Multiply.  Every cell has
    alpha 3 - 2 i - j: its rows 0 and 1 fail one pixel before their end, its apex (its last fragment) fails too, so a None draw ends
    dead (carry_dead set); every cell's first row is the tile row of the previous cell's apex.  The Alpha / Additive / Multiply
    fragments with alpha <= 0 fail the gate and kill nothing."""
    out = []
    for dt in (DepthTest.Always, DepthTest.LessEqual, DepthTest.Disabled):
        rng = np.random.default_rng(9600 + seed)
        W = H = TILE
        draws = []
        for k, blend in enumerate(O6_BLENDS):
            tri = cell(3 * k, 3 * k, 3, z=float(rng.uniform(-0.5, 0.5)), rgba=[(*_rgb(rng)[:3], 3.0), (*_rgb(rng)[:3], -3.0), (*_rgb(rng)[:3], 0.0)])
            draws.append(draw([tri], W, H, dt, blend))
        out.append(_scene(f"o6_{dt.name}", W, H, draws))
    return out


FAMILIES = {"o1": o1_depth_ties, "o2": o2_gate_and_blend, "o3": o3_row_kills, "o4": o4_kills_and_depth, "o5": o5_shared_pixels,
            "o6": o6_draw_boundaries}


def family(tag, seed=0) -> List[scenes.Scene]:
    return list(FAMILIES[tag](seed))


@functools.lru_cache(maxsize=None)
def all_scenes(seed=0):
    return {s.name: s for f in FAMILIES for s in family(f, seed)}


# =============================================================================================== O7: the same scene in another kernel
def diluted(scene, with_phong=False):
    """The scene plus one triangle entirely off screen: BlendMode.None (-> generic_none) or Phong4Point (-> generic_phong).  It
    uses LessEqual, so depth_only_grows and every visible word stay."""
    prog = S.PHONG if with_phong else S.GOURAUD
    off = E._draw([(5.0, 5.0, 0.0), (6.0, 5.0, 0.0), (5.0, 6.0, 0.0)], [(1.0, 1.0, 1.0, 1.0)] * 3, program=prog,
                  blend=BlendMode.Alpha if with_phong else BlendMode.None_)
    off.uniforms = S.uniforms_for(prog)
    return dataclasses.replace(scene, name=scene.name + ("_phong" if with_phong else "_none"), draws=list(scene.draws) + [off])


def expected_kernel(scene, dilution=None):
    """What select_raster_kernel must pick for an O1 / O2 scene and its dilutions, from the scene's state alone."""
    none = any(d.blend == BlendMode.None_ for d in scene.draws)
    if dilution == "none" or none:
        return "generic_none"
    if dilution == "phong":
        return "generic_phong"
    default = all(d.blend == BlendMode.Alpha and d.depth_test == DepthTest.LessEqual for d in scene.draws)
    gouraud = all(d.program == Program.Gouraud for d in scene.draws)
    return "gouraud_default" if default and gouraud else "generic"


# =============================================================================================== the restatement
def _depth_passes(test, nd, od, eq_threshold, eq_strict):
    test = DepthTest(test)
    if test in (DepthTest.Equal, DepthTest.NotEqual) and (eq_threshold != EPSILON or not eq_strict):
        diff = np.abs(F32(nd - od))
        eq = diff < F32(eq_threshold) if eq_strict else diff <= F32(eq_threshold)
        return bool(eq) if test == DepthTest.Equal else not bool(eq)
    return bool(Wf.depth_func(test, nd, od))


GATES = {"gt": lambda a: bool(a > 0), "ge": lambda a: bool(a >= 0), "ne": lambda a: bool(a != 0)}


def blend32(src, dst, mode, additive_fmin=False, alpha_fused=False):
    """Rasterizer.cs:58-75 on float32 4-vectors, one rounding per operation."""
    mode = BlendMode(mode)
    src, dst = np.asarray(src, F32), np.asarray(dst, F32)
    if mode == BlendMode.Alpha:
        a = src[3]
        ia = F32(F32(1.0) - a)
        if alpha_fused:
            return Wf.fma32(src, np.full(4, a, F32), (dst * ia).astype(F32))
        return ((src * a).astype(F32) + (dst * ia).astype(F32)).astype(F32)
    if mode == BlendMode.Additive:
        s = (src + dst).astype(F32)
        if additive_fmin:
            return np.fmin(s, F32(1.0)).astype(F32)
        return np.array([Wf.mathf_min(v, F32(1.0)) for v in s], F32)
    if mode == BlendMode.Multiply:
        return (src * dst).astype(F32)
    return src.copy()


@dataclass
class Restated:
    color: np.ndarray               # (H, W, 4) float32
    depth: np.ndarray               # (H, W) float32
    stats: dict                     # the six counters
    frags: dict                     # per fragment in the reference's order (killed ones included): draw, tri, x, y, flag, alpha, nd, od
    pairs: list                     # (tri, draw, tx, ty, fragments) of every (triangle, tile) whose bbox meets the tile, in order

    def of(self, **kw):
        """Boolean mask over the fragments: of(tri=3, flag=KILLED)."""
        m = np.ones(self.frags["x"].shape, bool)
        for k, v in kw.items():
            m &= self.frags[k] == v
        return m


def restate(scene, eq_threshold=EPSILON, eq_strict=True, gate="gt", z_before_gate=False, additive_fmin=False, alpha_fused=False) -> Restated:
    """The scene's frame from the restatement alone: RasterizeTriangle per triangle, tile and row from edge_scenes.Tri.cover, with
    the `break`; Interpolate and the vertex stage are shade_edge_scenes'.  The keyword arguments are the mutants."""
    W, H = scene.width, scene.height
    color = np.empty((H, W, 4), F32)
    color[:] = np.asarray(scene.clear_color, F32)
    depth = np.full((H, W), FLOAT_MIN, F32)
    st = dict.fromkeys(("triangles_in", "triangles_setup", "triangles_clipped", "fragments_tested", "fragments_shaded", "fragments_written"), 0)
    cols = {k: [] for k in ("draw", "tri", "x", "y", "flag", "alpha", "nd", "od")}
    pairs = []
    passes_gate = GATES[gate]
    tri_no = 0
    with np.errstate(all="ignore"):
        for j, d in enumerate(scene.draws):
            stage = S.vertex_stage(d)
            writes_z = d.depth_test != DepthTest.Disabled
            for vid in d.indices.reshape(-1, 3):
                st["triangles_in"] += 1
                this, tri_no = tri_no, tri_no + 1
                cl = [stage[0][int(v)] for v in vid]
                assert all(c[3] > 0 for c in cl), "the families never need the near clipper"
                t = E.Tri(cl, W, H)
                if not t.ok:
                    continue
                st["triangles_setup"] += 1
                for tx, ty, r in t.tiles():
                    inside = t.cover(r)[0]
                    pairs.append((this, j, tx, ty, int(inside.sum())))
                    if not inside.any():
                        continue
                    sh = S.Shaded(d, stage, vid, t, r, None, False)
                    src = sh.color
                    if d.program == Program.FlatColor:               # Interpolate's flat branch: outputs[0]'s colour as it is
                        src = np.broadcast_to(d.vertices["color"][int(vid[2])].astype(F32), src.shape)
                    k = 0
                    for yy in range(inside.shape[0]):
                        dead = False
                        for xx in range(inside.shape[1]):
                            if not inside[yy, xx]:
                                continue
                            X, Y, a, nd, od = r[0] + xx, r[2] + yy, src[k, 3], sh.depth[yy, xx], depth[r[2] + yy, r[0] + xx]
                            s4 = src[k]
                            k += 1
                            if dead:
                                flag = KILLED
                            else:
                                st["fragments_tested"] += 1
                                if not _depth_passes(d.depth_test, nd, od, eq_threshold, eq_strict):
                                    flag = DEPTH_FAILED
                                else:
                                    st["fragments_shaded"] += 1
                                    ok = passes_gate(a)
                                    if z_before_gate and writes_z:
                                        depth[Y, X] = nd
                                    if ok:
                                        color[Y, X] = blend32(s4, color[Y, X], d.blend, additive_fmin, alpha_fused)
                                        if writes_z:
                                            depth[Y, X] = nd
                                        st["fragments_written"] += 1
                                        flag = VISITED
                                    else:
                                        flag = GATE_FAILED
                                        dead = d.blend == BlendMode.None_
                            for key, v in (("draw", j), ("tri", this), ("x", X), ("y", Y), ("flag", flag), ("alpha", a), ("nd", nd), ("od", od)):
                                cols[key].append(v)
    frags = {k: np.asarray(v, F32 if k in ("alpha", "nd", "od") else np.int64) for k, v in cols.items()}
    return Restated(color, depth, st, frags, pairs)


# =============================================================================================== the planner
@dataclass
class TilePlan:
    exact: bool                     # no two fragments of one window share a pixel and nothing else can move a cut
    batches: list                   # per batch: [(tri, draw, fragments)] of its non-empty pairs
    chunks: list                    # (batch, first position in the batch, length, draw); inexact tiles: cut at 64, draws and batch ends only
    index: np.ndarray               # indices into Restated.frags of the tile's fragments, in stream order
    batch: np.ndarray               # per fragment of the tile: its batch ...
    pos: np.ndarray                 # ... its position in the batch's stream ...
    chunk: np.ndarray               # ... its chunk (index into `chunks`) ...
    lane: np.ndarray                # ... and its lane there


def plan(scene, r: Restated = None):
    """(tx, ty) -> TilePlan: k_raster_c's schedule for every tile of the scene, as the kernel's comments state it.  The stream of a
    tile is its pairs in submission order, each pair's fragments its inside pixels row-major (visited or not).  A batch takes
    the first non-empty pairs of a window of SWR_WINDOW list entries, at most SWR_BATCH of them and at most SWR_BATCH_FRAGS
    fragments (the first always fits), and consumes the list up to the first non-empty pair it left out.  Inside a batch chunks
    are 64 positions, cut at a change of draw and at the batch's end -- and at a fragment whose pixel is already claimed in the
    chunk, which the planner cannot place (the election's winner is not guaranteed): such a tile is not `exact`."""
    BATCH, BATCH_FRAGS, WINDOW = kernel_constants()
    r = r or restate(scene)
    f = r.frags
    grows = all(d.depth_test in (DepthTest.Less, DepthTest.LessEqual) for d in scene.draws)
    out = {}
    tiles = sorted({(p[2], p[3]) for p in r.pairs})
    for (tx, ty) in tiles:
        entries = [(p[0], p[1], p[4]) for p in r.pairs if (p[2], p[3]) == (tx, ty)]
        idx = np.nonzero((f["x"] // TILE == tx) & (f["y"] // TILE == ty))[0]
        assert idx.size == sum(e[2] for e in entries)
        n, base, batches = len(entries), 0, []
        while base < n:
            win = entries[base:base + WINDOW]
            taken, frags, consumed = [], 0, len(win)
            for i, e in enumerate(win):
                if e[2] == 0:
                    continue
                if len(taken) >= BATCH or frags + e[2] > BATCH_FRAGS:
                    consumed = i
                    break
                taken.append(e)
                frags += e[2]
            base += consumed
            if taken:
                batches.append(taken)
        # binning may or may not keep a pair without a fragment (it is conservative): that moves window ends only past WINDOW entries
        exact = not (any(e[2] == 0 for e in entries) and n > WINDOW)
        # hi-Z (all draws Less / LessEqual) drops a pair at batch start only when the whole tile has been written by earlier batches
        if grows and len(batches) > 1:
            px = f["x"][idx] % TILE + TILE * (f["y"][idx] % TILE)
            exact = exact and np.unique(px).size < min(TILE, scene.width - TILE * tx) * min(TILE, scene.height - TILE * ty)
        chunks, b_of, p_of, c_of, l_of = [], [], [], [], []
        k = 0
        for bi, taken in enumerate(batches):
            pos, start, cur = 0, 0, None
            seen = set()
            for (tri, dr, cnt) in taken:
                for _ in range(cnt):
                    pix = (int(f["x"][idx[k]]), int(f["y"][idx[k]]))
                    if pix in seen:
                        exact = False
                    seen.add(pix)
                    if cur is None or dr != cur or pos - start == CHUNK:
                        if cur is not None:
                            chunks.append((bi, start, pos - start, cur))
                        start, cur = pos, dr
                    b_of.append(bi); p_of.append(pos); c_of.append(len(chunks)); l_of.append(pos - start)
                    pos += 1
                    k += 1
            chunks.append((bi, start, pos - start, cur))
        out[(tx, ty)] = TilePlan(exact, batches, chunks, idx, *(np.asarray(v, np.int64) for v in (b_of, p_of, c_of, l_of)))
    return out
