"""Scenes that put DebugMode.Wireframe -- DrawLine, Rasterizer.cs:232-340: the records of k_setup's wireframe branch
(csrc/swr_geometry.hip.h), line_test (csrc/swr_device.h), k_cover<true> and the LINES branches of k_raster_c
(csrc/swr_raster_c.hip.h) -- where its decisions fall, and a numpy-float32 restatement of DrawLine that says which pixel is
lit, with which t and which depth word.  tests/test_wireframe_edges_host.py asserts on the CPU what every family reaches and that
the restatement IS the oracle's wireframe frame; tests/test_gpu_wireframe_edges.py renders the scenes.

  W1  half-pixel ties: segments along Pythagorean directions, pixel centres at exactly 0.5 px in real arithmetic
  W2  the truncating bbox and the frame's edges on a 250 x 130 target (partial tiles right and below)
  W3  end caps: pixels that project before p0 / beyond p1 (t clamped) within half a pixel of the end point
  W4  magnitude ladder: p1 at 1e3 .. 1e19, 1e20 (len_sq = +Inf, t = 0), 1e37 (t NaN) and +Inf
  W5  the depth of a line, 1 / (d0 (1 - t) + d1 t), at zero and cancelling denominators, under all eight depth tests; once with
      a negative clip.w that the near clipper keeps
  W6  alpha != 0 (negative, NaN, +-0) and the varyings of outputs[0..1] under the four blend modes
  W7  many short lines in one tile / in four: one pixel hit several times inside a 64-fragment chunk, near-clipped quads
  W8  N = 31, 32, 33, 64, 100 empty pairs in a tile's list, then one that covers (SWR_WINDOW = 32 candidate pairs)
  W9  lines across the whole 256 x 256 frame: 256-tile boxes (bin_big), about 31 non-empty pairs each

Geometry.  A triangle is given by its three screen points in the order of `outputs` (Rasterizer.cs:367: outputs = {v2, v1, v0}),
so the first edge DrawLine receives is (s0, s1) and EVERY edge carries depths[0..1] and outputs[0..1], i.e. those of s0 and s1.
Exact screen positions come from edge_scenes.clip_pos on power-of-two targets with clip.w = 1.

What the pipeline cannot reach (each is asserted in the host tests, so the day it becomes reachable a test says so):
  * a screen coordinate in (-2^-24 * size, 0) in x, (-2^-23 * size, 0) in y, or equal to -0.0: screen = (n * 0.5 + 0.5) * size,
    and n * 0.5 + 0.5 is a multiple of 2^-24 near n = -1 (1 - that: of 2^-23), and x + 0.5 never rounds to -0.  A
    vertical edge at x = -1e-9 (column 0 at exactly 0.5 px) therefore does not exist: the nearest one, at -1.5e-5, gets the bbox
    column 0 by truncation and lights nothing.  What does exist is as free of tolerance: an edge that ENDS at such a vertex and
    starts more than 256 px (x; 512 px in y) off the frame has dx = p1x - p0x rounded so that p0x + 1 * dx is exactly 0.0, and the
    end cap lights the one pixel of column 0 (row 0) whose centre is then at exactly 0.5 px.  A floor skips that line.  W2 holds
    three such scenes; the -1e-9 / -0.0 discriminators are kept at the level of the restatement's functions.
  * a depth operand that is subnormal, -0.0, infinite or NaN: depths[i] = (nz + 1) * 0.5 with nz finite (:378-380) is +0.0 or at
    least 2^-25 in magnitude and at most 2^127.  So a NaN depth word (Inf * 0, or a NaN operand) does not exist.  Everything
    else does, because t itself can be subnormal: with px exactly 0 the numerator is py * dy alone, and over len_sq = 1e38 that
    is 6.25e-40.  With d0 = 0 the denominator d1 * t is then subnormal of either sign (the reciprocal overflows to +Inf or -Inf,
    or stays finite near 2e38) or underflows to +0.  W5's W5_SUBNORMAL_T kinds are these.
  * len_sq == 0 with distinct end points needs both within about 1e-23 of the origin; the nearest pixel centre is then 0.707 px
    away, so line_test's `len_sq > 0` guard cannot change a pixel.  No family aims at it.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass
from fractions import Fraction
from typing import List

import numpy as np

import edge_scenes as E
import shade_edge_scenes as S
import softwarerenderer_amd.hostmath as hm
from oracle import binding as ob
from softwarerenderer_amd import scenes
from softwarerenderer_amd.rasterizer import BlendMode, CullMode, DepthTest, Program

F32 = np.float32
TILE = 16
SWR_WINDOW = 32                     # csrc/swr_raster_c.hip.h: candidate pairs per batch
CHUNK = 64                          # fragments per chunk of a tile's stream
EPSILON = F32(1e-6)                 # Rasterizer.cs:52
CLEAR = (0.0, 0.0, 0.0, 1.0)
FLOAT_MIN = F32(-3.40282347e38)     # the depth buffer's clear value
PYTHAGOREAN = ((3, 4), (4, 3), (5, 12), (12, 5), (8, 15), (7, 24))
W1_P0 = ((10.0, 6.0), (10.5, 6.0), (13.0, 13.5))
W4_MAGNITUDES = (1e3, 1e6, 1e10, 1e15, 1e19, 1e20, 1e37, float("inf"))
W8_RUNS = (31, 32, 33, 64, 100)
ALL_DEPTH_TESTS = tuple(DepthTest)
ALL_BLENDS = tuple(BlendMode)


# =============================================================================================== building
@dataclass
class V:
    """One vertex of a triangle, in screen terms."""
    x: float
    y: float
    z: float = 0.0                          # clip.z / clip.w: depth = (z + 1) / 2
    rgba: tuple = (1.0, 1.0, 1.0, 1.0)
    w: float = 1.0                          # clip.w (a power of two keeps the screen position exact)
    ndc: tuple = None                       # (nx, ny) given directly instead of (x, y): for positions off every lattice


def _triangle_draw(tris, W, H, *, program=Program.Gouraud, depth_test=DepthTest.LessEqual, blend=BlendMode.Alpha, uniforms=None):
    """tris: triples of V in OUTPUTS order (s0, s1, s2); submitted as v0 = s2, v1 = s1, v2 = s0.  clip = (x w, y w, z w, w)
    through edge_scenes.w_projection when any w differs from 1 (then every z of the draw must be equal: it is the constant nz)."""
    pos, col = [], []
    perw = any(v.w != 1.0 for t in tris for v in t)
    zs = {v.z for t in tris for v in t}
    assert not perw or len(zs) == 1
    for t in tris:
        for v in (t[2], t[1], t[0]):
            nx, ny = v.ndc if v.ndc is not None else E.clip_pos(v.x, v.y, W, H)
            pos.append((nx * v.w, ny * v.w, v.w) if perw else (nx, ny, v.z))
            col.append(v.rgba)
    vtx = scenes.make_vertices(np.asarray(pos, np.float64), color=np.asarray(col, np.float64))
    assert vtx.shape[0] <= 65535
    I = hm.identity()
    proj = E.w_projection(zs.pop()) if perw else I
    return scenes.Draw(vtx, np.arange(vtx.shape[0], dtype=np.uint16), I, I, proj, program=program,
                       uniforms=uniforms if uniforms is not None else scenes.default_uniforms(), cull=CullMode.None_,
                       depth_test=depth_test, blend=blend)


def _scene(name, W, H, draws, **kw):
    return scenes.Scene("wire_" + name, W, H, list(draws), clear_color=CLEAR, **kw)


def _rgb(rng, a=0.6):
    return (*rng.uniform(0.1, 1.0, 3), a)


def _far_third(p0, p1, far=600.0):
    """A third vertex `far` px to the side of p0: the edges to it leave the segment at its end points and never come back."""
    d = np.array([p1[0] - p0[0], p1[1] - p0[1]], float)
    n = np.array([d[1], -d[0]]) / np.hypot(*d)
    return float(round(p0[0] + far * n[0])) + 0.5, float(round(p0[1] + far * n[1])) + 0.5


# =============================================================================================== W1
def w1_segments():
    """(name, p0, p1) of every W1 segment: six directions from three start points, each two triples long; and, per direction, one
    LONG segment through (10.5, 6) + (16, 32) whose end points lie 40 to 200 triples (about 1e3 px) before and behind the 64 x 64
    frame, so that x + 0.5 - p0x is of the order 1e3 and its products round.  The long ones stand in for `the short segments
    translated by a tile multiple plus 1e3 px`: a frame of at most 256 px cannot see a short segment 1e3 px away, and the renderer
    has no viewport offset; what a translation is for -- large, rounding operands at pixels that are still ties -- the long segment has."""
    out = []
    for (a, b) in PYTHAGOREAN:
        for p0 in W1_P0:
            out.append((f"w1_{a}_{b}_at_{p0[0]:g}_{p0[1]:g}", p0, (p0[0] + 2 * a, p0[1] + 2 * b)))
    for (a, b) in PYTHAGOREAN:
        n = int(round(1000.0 / np.hypot(a, b)))
        q = (10.5 + 16.0, 6.0 + 32.0)
        out.append((f"w1_{a}_{b}_from_1e3px", (q[0] - n * a, q[1] - n * b), (q[0] + n * a, q[1] + n * b)))
    return out


@functools.lru_cache(maxsize=None)
def w1_half_pixel_ties(seed=0):
    rng = np.random.default_rng(7100 + seed)
    out = []
    for name, p0, p1 in w1_segments():
        s2 = _far_third(p0, p1)
        tri = (V(*p0, 0.0, _rgb(rng)), V(*p1, 0.25, _rgb(rng)), V(*s2, 0.5, _rgb(rng)))
        out.append(_scene(name, 64, 64, [_triangle_draw([tri], 64, 64)]))
    return out


# =============================================================================================== W2
W2_SIZE = (250, 130)


def ndc_with_screen(pred, X, size, flip=False, reach=1 << 16):
    """The float32 NDC nearest to that of screen coordinate X whose screen coordinate -- computed as DrawTriangle does,
    (n * 0.5 + 0.5) * size, or (1 - (n * 0.5 + 0.5)) * size for y -- satisfies pred."""
    def screen(n):
        s = F32(F32(n * F32(0.5)) + F32(0.5))
        return F32((F32(1.0) - s if flip else s) * F32(size))
    n0 = F32(2.0 * X / size - 1.0)
    n0 = F32(-n0) if flip else n0
    up, dn = n0, n0
    for _ in range(reach):
        for n in (up, dn):
            if pred(screen(n)):
                return float(n)
        up, dn = np.nextafter(up, F32(np.inf)), np.nextafter(dn, F32(-np.inf))
    raise AssertionError(f"no float32 NDC near screen coordinate {X} of {size} satisfies the predicate")


def _w2v(x, y, z, rgba, xpred=None, ypred=None):
    W, H = W2_SIZE
    nx = ndc_with_screen(xpred, x, W) if xpred else float(F32(2.0 * x / W - 1.0))
    ny = ndc_with_screen(ypred, y, H, flip=True) if ypred else -float(F32(2.0 * y / H - 1.0))
    return V(x, y, z, rgba, ndc=(nx, ny))


@functools.lru_cache(maxsize=None)
def w2_bbox_and_frame_edges(seed=0):
    rng = np.random.default_rng(7200 + seed)
    W, H = W2_SIZE
    c = lambda: _rgb(rng)
    neg = lambda s: -1.0 < s < 0.0                  # the negative screen coordinate nearest to 0 that exists
    zero = lambda s: s == 0.0
    eq = lambda v: (lambda s: s == F32(v))
    cases = {
        # a vertical edge at the largest negative x, at x = 0.0, and a horizontal one at the largest negative y
        "x_just_negative": [(_w2v(-1e-9, 20.5, 0, c(), xpred=neg), _w2v(-1e-9, 60.5, 0, c(), xpred=neg), _w2v(-300.5, 40.5, 0, c()))],
        "x_zero": [(_w2v(0, 20.5, 0, c(), xpred=zero), _w2v(0, 60.5, 0, c(), xpred=zero), _w2v(-300.5, 40.5, 0, c()))],
        "y_just_negative": [(_w2v(30.5, -1e-9, 0, c(), ypred=neg), _w2v(200.5, -1e-9, 0, c(), ypred=neg), _w2v(100.5, -600.5, 0, c()))],
        "x_and_y_just_negative": [(_w2v(-1e-9, 70.5, 0, c(), xpred=neg), _w2v(-1e-9, 100.5, 0, c(), xpred=neg), _w2v(-400.5, 90.5, 0, c())),
                                  (_w2v(130.5, -1e-9, 0, c(), ypred=neg), _w2v(220.5, -1e-9, 0, c(), ypred=neg), _w2v(180.5, -700.5, 0, c()))],
        # x = 125.0 exactly (6.0 does not exist on 250 columns: 6 / 250 is no float32 product): bbox column 125 only; column 124's
        # centres are at 0.5 px and stay dark
        "x_125": [(_w2v(125, 20.5, 0, c(), xpred=eq(125)), _w2v(125, 90.5, 0, c(), xpred=eq(125)), _w2v(400.5, 60.5, 0, c()))],
        "y_65": [(_w2v(20.5, 65, 0, c(), ypred=eq(65)), _w2v(190.5, 65, 0, c(), ypred=eq(65)), _w2v(100.5, 500.5, 0, c()))],
        # a line with both ends off the frame that crosses it
        "crossing": [(_w2v(-40.5, -30.5, 0, c()), _w2v(300.5, 170.5, 0.5, c()), _w2v(-400.5, 500.5, 0, c()))],
        # lines entirely beyond each of the four edges (minX > maxX or minY > maxY), and one small visible marker
        "beyond": [(_w2v(-90.5, 10.5, 0, c()), _w2v(-20.5, 100.5, 0, c()), _w2v(-50.5, 60.5, 0.5, c())),
                   (_w2v(260.5, 10.5, 0, c()), _w2v(300.5, 100.5, 0, c()), _w2v(270.5, 60.5, 0.5, c())),
                   (_w2v(10.5, -90.5, 0, c()), _w2v(200.5, -20.5, 0, c()), _w2v(60.5, -50.5, 0.5, c())),
                   (_w2v(10.5, 140.5, 0, c()), _w2v(200.5, 190.5, 0, c()), _w2v(60.5, 150.5, 0.5, c())),
                   (_w2v(100.5, 60.5, 0, c()), _w2v(110.5, 60.5, 0, c()), _w2v(100.5, 70.5, 0.5, c()))],
    }
    # extremes at size - 1 (the nearest coordinates that exist below it -- the cast gives size - 2 -- and from it upwards), at
    # size - 0.5, at the last coordinate below size (clamped to size - 1: the last column, lit) and at size itself (minX > maxX)
    below = lambda v: (lambda s: F32(v - 0.01) < s < F32(v))
    from_ = lambda v: (lambda s: F32(v) <= s < F32(v + 0.01))
    for k, off, mk in (("m1_below", 1.0, below), ("m1", 1.0, from_), ("mhalf", 0.5, from_), ("m0_below", 0.0, below), ("m0", 0.0, eq)):
        x, y = W - off, H - off
        cases[f"x_W{k}"] = [(_w2v(x, 20.5, 0, c(), xpred=mk(x)), _w2v(x, 100.5, 0, c(), xpred=mk(x)), _w2v(W + 300.5, 60.5, 0, c()))]
        cases[f"y_H{k}"] = [(_w2v(20.5, y, 0, c(), ypred=mk(y)), _w2v(200.5, y, 0, c(), ypred=mk(y)), _w2v(100.5, H + 300.5, 0, c()))]
    return [_scene("w2_" + k, W, H, [_triangle_draw(t, W, H)]) for k, t in cases.items()]


# =============================================================================================== W3
@functools.lru_cache(maxsize=None)
def w3_end_caps(seed=0):
    """Steep and shallow segments whose end points sit off-centre in their pixels (fractions 1/64 .. 63/64), so that the bbox
    holds centres that project before p0 and beyond p1; and segments whose end points ARE pixel centres (t = 0 and 1, distance 0)."""
    rng = np.random.default_rng(7300 + seed)
    W = H = 128
    out = []
    for kind in ("shallow", "steep", "centres"):
        tris = []
        for i in range(8):
            cx, cy = 16 + 32 * (i % 4) , 24 + 64 * (i // 4)
            lng, sht = int(rng.integers(9, 14)), int(rng.integers(1, 5))
            sx, sy = (1, -1)[int(rng.integers(0, 2))], (1, -1)[int(rng.integers(0, 2))]
            dx, dy = (lng, sht) if kind != "steep" else (sht, lng)
            if kind == "centres":
                f0 = f1 = (0.5, 0.5)
                if i % 2:
                    dx, dy = dy, dx
            else:
                f0, f1 = rng.integers(1, 64, 2) / 64.0, rng.integers(1, 64, 2) / 64.0
            p0 = (cx + f0[0], cy + f0[1])
            p1 = (cx + sx * dx + f1[0], cy + sy * dy + f1[1])
            s2 = _far_third(p0, p1, far=300.0)
            tris.append((V(*p0, 0.0, _rgb(rng)), V(*p1, 0.5, _rgb(rng)), V(*s2, 0.0, _rgb(rng))))
        out.append(_scene("w3_" + kind, W, H, [_triangle_draw(tris, W, H)]))
    return out


# =============================================================================================== W4
W4_P0 = ((20.25, 30.5, 1.0, 0.0), (44.25, 12.5, -1.0, 0.0), (20.25, 40.75, 1.0, 0.5), (44.75, 50.25, -1.0, -0.5))   # x, y, direction


def _w4_ndc(X, size):
    """NDC of a screen coordinate of any magnitude; +-Inf means `the largest finite NDC`, whose screen coordinate overflows."""
    if np.isinf(X):
        return float(np.sign(X) * F32(3.0e38))
    return float(F32(2.0 * X / size - 1.0))


@functools.lru_cache(maxsize=None)
def w4_magnitude_ladder(seed=0):
    """Four triangles per scene (along +x, -x, and two diagonals), p0 on the 64 x 64 frame, p1 = p0 + M * direction; and the same
    with p0 and p1 exchanged.  The third vertex is on the frame, so one more edge of each triangle is as long."""
    rng = np.random.default_rng(7400 + seed)
    W = H = 64
    out = []
    for M in W4_MAGNITUDES:
        for swapped in (False, True):
            tris = []
            for (x, y, ux, uy) in W4_P0:
                far = V(0, 0, 0.5, _rgb(rng), ndc=(_w4_ndc(x + M * ux if ux else x, W), -_w4_ndc(y + M * uy, H) if uy else E.clip_pos(x, y, W, H)[1]))
                near = V(x, y, 0.0, _rgb(rng))
                third = V(x + 3.0, y + 9.0, 0.25, _rgb(rng))
                tris.append((far, near, third) if swapped else (near, far, third))
            tag = "inf" if np.isinf(M) else f"1e{int(round(np.log10(M)))}"
            out.append(_scene(f"w4_{tag}" + ("_swapped" if swapped else ""), W, H, [_triangle_draw(tris, W, H)]))
    return out


# =============================================================================================== W5
TINY_NEG_Z = float(np.nextafter(F32(-1.0), F32(-2.0)))      # depth -2^-24
TINY_POS_Z = float(np.nextafter(F32(-1.0), F32(0.0)))       # depth +2^-25
W5_DEPTHS = (("equal", -0.5, -0.5), ("d0_zero", -1.0, 0.0), ("d1_zero", 0.25, -1.0), ("opposite", -1.5, -0.5),
             ("tiny_opposite", TINY_NEG_Z, TINY_POS_Z), ("tiny_and_zero", -1.0, TINY_POS_Z), ("huge", 3.0e38, -3.0e38))
# d0 = 0 on a line whose t is subnormal at one lit pixel: denominators d1 * t of 6.25e-40 (1 / it overflows: +Inf), -6.25e-40 (-Inf),
# 5e-39 (subnormal, the reciprocal 2e38 is finite) and 2^-25 * t (underflows to +0: +Inf)
W5_SUBNORMAL_T = (("sub_plus", -1.0, 1.0), ("sub_minus", -1.0, -3.0), ("sub_finite", -1.0, 15.0), ("sub_to_zero", -1.0, TINY_POS_Z))
W5_FAR_X = 1e19


@functools.lru_cache(maxsize=None)
def w5_line_depth(seed=0):
    """One scene per depth test.  Per kind of (d0, d1) a background triangle at depth 0.5 under Always, then the test triangle on the
    same first edge (49 pixels: t = 0.5 exactly at the middle one) under the scene's depth test.  The W5_SUBNORMAL_T kinds have
    another first edge: p0 = (20.5, r + 0.25) -- its x on a pixel centre -- and p1 = (1e19, r + 0.5).  At pixel (20, r) px is exactly
    0, so the numerator is py * dy = 0.0625, len_sq is 1e38 and t = 6.25e-40, a subnormal; the pixel is lit (0.25 px from p0)."""
    rng = np.random.default_rng(7500 + seed)
    W, H = 64, 128
    out = []
    for dt in ALL_DEPTH_TESTS:
        draws = []
        for i, (kind, z0, z1) in enumerate(W5_DEPTHS):
            y = 4.5 + 8 * i
            p0, p1, p2 = (8.5, y), (56.5, y + 3.0), (8.5, y + 5.0)
            bg = (V(*p0, 0.0, _rgb(rng, 1.0)), V(*p1, 0.0, _rgb(rng, 1.0)), V(*p2, 0.0, _rgb(rng, 1.0)))
            fg = (V(*p0, z0, _rgb(rng)), V(*p1, z1, _rgb(rng)), V(*p2, 0.0, _rgb(rng)))
            draws.append(_triangle_draw([bg], W, H, depth_test=DepthTest.Always))
            draws.append(_triangle_draw([fg], W, H, depth_test=dt))
        for i, (kind, z0, z1) in enumerate(W5_SUBNORMAL_T, start=len(W5_DEPTHS)):
            r = 4 + 8 * i
            far = (float(F32(2.0 * W5_FAR_X / W - 1.0)), E.clip_pos(0.0, r + 0.5, W, H)[1])
            for z, a, test in ((0.0, 1.0, DepthTest.Always), (None, 0.6, dt)):
                tri = (V(20.5, r + 0.25, 0.0 if z == 0.0 else z0, _rgb(rng, a)), V(0, 0, 0.0 if z == 0.0 else z1, _rgb(rng, a), ndc=far),
                       V(24.5, r + 5.5, 0.0, _rgb(rng, a)))
                draws.append(_triangle_draw([tri], W, H, depth_test=test))
        out.append(_scene(f"w5_{dt.name}", W, H, draws))
    out.append(w5_negative_w(seed))
    return out


W5_NEGATIVE_W_ZC = (0.5, 1.0, 3.0)      # (d0, d1) = ((1 - zc) / 2, (1 + zc) / 2): ordinary, d0 = 0, opposite signs


def w5_negative_w(seed=0):
    """The same depths by another road: shade_edge_scenes.zw_projection (clip = (x, y, zc, z)) with clip.w = -1 at s0 and +1 at s1
    and s2.  A w <= 0 sends the triangle through the near clipper, which keeps all three vertices (zc >= near * w), and nz = zc / w
    changes sign with w."""
    rng = np.random.default_rng(7550 + seed)
    W = H = 64
    draws = []
    I = hm.identity()
    for i, zc in enumerate(W5_NEGATIVE_W_ZC):
        y = 8.5 + 16 * i
        pts = ((8.5, y, -1.0), (56.5, y + 3.0, 1.0), (8.5, y + 5.0, 1.0))                  # s0, s1, s2 with their clip.w
        pos, col = [], []
        for (x, yy, w) in (pts[2], pts[1], pts[0]):                                       # submitted as v0 = s2, v1 = s1, v2 = s0
            nx, ny = E.clip_pos(x, yy, W, H)
            pos.append((nx * w, ny * w, w))
            col.append(_rgb(rng))
        v = scenes.make_vertices(np.asarray(pos, np.float64), color=np.asarray(col, np.float64))
        draws.append(scenes.Draw(v, np.arange(3, dtype=np.uint16), I, I, S.zw_projection(zc), program=Program.Gouraud,
                                 uniforms=scenes.default_uniforms(), cull=CullMode.None_, depth_test=DepthTest.LessEqual, blend=BlendMode.Alpha))
    return _scene("w5_negative_w", W, H, draws)


# =============================================================================================== W6
NAN = float("nan")
W6_ALPHAS = (("crossing", 0.75, -0.75, 0.5), ("negative", -0.5, -0.5, 0.5), ("zeros", -0.0, 0.0, 1.0), ("nan", NAN, NAN, 0.5),
             ("to_zero", 0.5, 0.0, 1.0))


# clip.w of s0 (and s2) and of s1: the raster kernel's guard div_operands_safe3 (csrc/swr_device.h) holds for magnitudes in
# [2^-40, 2^40], both ends included -- the first three sit on its ends and inside, the last three one binade outside
W6_CLIP_W = (("w_up", 1.0, 2.0 ** 40), ("w_down", 1.0, 2.0 ** -40), ("w_both", 2.0 ** 40, 2.0 ** -40),
             ("w_up_out", 1.0, 2.0 ** 41), ("w_down_out", 1.0, 2.0 ** -41), ("w_both_out", 2.0 ** 41, 2.0 ** -41))


def div_operands_safe3(a, b, c):
    """div_operands_safe3 of csrc/swr_device.h: every |v| in [2^-40, 2^40], compared as bit patterns."""
    u = [int(np.array(v, F32).view(np.uint32)) & 0x7FFFFFFF for v in (a, b, c)]
    return min(u) >= 0x2B800000 and max(u) <= 0x53800000


def _w6_triangles(rng, w0=1.0, w1=1.0):
    tris = []
    for i, (kind, a0, a1, a2) in enumerate(W6_ALPHAS):
        y = 6.5 + 11 * i
        # 33 pixels on the first edge: t = 0.5 exactly in the middle, where `crossing` has alpha exactly 0 on a row that goes on
        tris.append((V(12.5, y, 0.0, (*rng.uniform(0.1, 1.0, 3), a0), w0), V(44.5, y, 0.0, (*rng.uniform(0.1, 1.0, 3), a1), w1),
                     V(20.5, y + 7.0, 0.0, (*rng.uniform(0.1, 1.0, 3), a2), w0)))
    return tris


@functools.lru_cache(maxsize=None)
def w6_alpha_and_varyings(seed=0):
    """Every triangle has three different vertex colours; edges 2 and 3 must show those of s0 and s1 all the same.  DepthTest.Always:
    every lit pixel whose alpha is not 0 is written."""
    rng = np.random.default_rng(7600 + seed)
    W = H = 64
    out = []
    for prog in (Program.Gouraud, Program.Dust2LambertFog, Program.FlatColor):
        for blend in ALL_BLENDS:
            d = _triangle_draw(_w6_triangles(rng), W, H, program=prog, depth_test=DepthTest.Always, blend=blend)
            out.append(_scene(f"w6_{prog.name}_{blend.name}", W, H, [d]))
    for tag, w0, w1 in W6_CLIP_W:
        d = _triangle_draw(_w6_triangles(rng, w0, w1), W, H, program=Program.Gouraud, depth_test=DepthTest.Always, blend=BlendMode.Alpha)
        out.append(_scene(f"w6_{tag}", W, H, [d]))
    return out


# =============================================================================================== W7
W7_ONE_TILE = (16, 16)
W7_FOUR_TILES = (16, 96)            # six tile rows, triangles in rows 0, 2, 3 and 5: bands and stripes all hold some, two tiles stay empty
W7_ROWS = (0, 2, 3, 5)
W7_TRIS = 208


def _w7_triangles(rng, n, tiles):
    tris = []
    for i in range(n):
        ty = tiles[i % len(tiles)]
        lx, ly = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        x, y = int(rng.integers(1, 15 - lx)) + 0.5, int(rng.integers(1, 15 - ly)) + 0.5 + TILE * ty
        sx, sy = (1, -1)[int(rng.integers(0, 2))], (1, -1)[int(rng.integers(0, 2))]
        if sx < 0:
            x += lx
        if sy < 0:
            y += ly
        tris.append((V(x, y, 0.0, _rgb(rng, rng.uniform(0.3, 0.7))), V(x + sx * lx, y, 0.0, _rgb(rng, rng.uniform(0.3, 0.7))),
                     V(x, y + sy * ly, 0.0, _rgb(rng, rng.uniform(0.3, 0.7)))))
    return tris


@functools.lru_cache(maxsize=None)
def w7_shared_pixels(seed=0):
    """208 right triangles with legs of 1 to 4 px, all at depth 0.5: the three records of a triangle meet at its vertices and
    neighbours overlap.  Under Additive and Alpha (order shows) x Less, LessEqual, Always (a second hit at equal depth fails, passes,
    passes), in one tile and over four.  Last: needles from behind the camera that the near plane cuts into quads -- two fan
    triangles, six records, the shared diagonal drawn twice with the depths and outputs of each fan triangle's first two vertices."""
    out = []
    for (W, H), tiles, tag in ((W7_ONE_TILE, (0,), "one_tile"), (W7_FOUR_TILES, W7_ROWS, "four_tiles")):
        for blend in (BlendMode.Additive, BlendMode.Alpha):
            for dt in (DepthTest.Less, DepthTest.LessEqual, DepthTest.Always):
                rng = np.random.default_rng(7700 + seed)
                d = _triangle_draw(_w7_triangles(rng, W7_TRIS, tiles), W, H, depth_test=dt, blend=blend)
                out.append(_scene(f"w7_{tag}_{blend.name}_{dt.name}", W, H, [d]))
    out.append(w7_clipped_quads(seed))
    return out


def w7_clipped_quads(seed=0, n=24):
    rng = np.random.default_rng(7750 + seed)
    W = H = 64
    pos = np.empty((n, 3, 3))
    for i in range(n):
        x0, y0 = rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)
        for k in range(3):
            d = -rng.uniform(0.1, 0.3) if k == 0 else rng.uniform(1.2, 1.6)             # one vertex behind the camera: a quad
            pos[i, k] = (x0 + rng.uniform(-0.2, 0.2), y0 + rng.uniform(-0.2, 0.2), -d)
        pos[i] = pos[i][rng.permutation(3)]
    col = np.concatenate([rng.uniform(0.1, 1.0, (3 * n, 3)), rng.uniform(0.3, 0.7, (3 * n, 1))], axis=1)
    v = scenes.make_vertices(pos.reshape(-1, 3), color=col)
    I = hm.identity()
    d = scenes.Draw(v, np.arange(3 * n, dtype=np.uint16), I, I, scenes._perspective(W, H), program=Program.Gouraud,
                    uniforms=scenes.default_uniforms(), cull=CullMode.None_, depth_test=DepthTest.LessEqual, blend=BlendMode.Alpha)
    return _scene("w7_clipped_quads", W, H, [d], near_clip=0.9)


# =============================================================================================== W8
W8_TILE = (3, 0)                    # the corner tile of the 4 x 4-tile frame that no diagonal touches


@functools.lru_cache(maxsize=None)
def w8_empty_pairs(seed=0):
    """N triangles whose first edge is a diagonal from the top left to the bottom right tile (its bbox is the whole frame, the top
    right tile gets a pair without a pixel) and whose other edges run along the left and the bottom; then one small triangle inside
    the top right tile.  Every vertex at a half-pixel position: front_end_scenes.plan counts the pairs."""
    out = []
    for N in W8_RUNS:
        rng = np.random.default_rng(7800 + seed + N)
        tris = []
        for i in range(N):
            a, b = float(i % 5), float((i // 5) % 4)
            tris.append((V(2.5 + a, 1.5 + b, 0.0, _rgb(rng, 0.4)), V(62.5 - b, 61.5 - a, 0.0, _rgb(rng, 0.4)), V(2.5 + a, 61.5 - a, 0.0, _rgb(rng, 0.4))))
        tris.append((V(52.5, 4.5, 0.0, _rgb(rng, 0.4)), V(58.5, 4.5, 0.0, _rgb(rng, 0.4)), V(52.5, 9.5, 0.0, _rgb(rng, 0.4))))
        out.append(_scene(f"w8_{N}_empty", 64, 64, [_triangle_draw(tris, 64, 64)]))
    return out


# =============================================================================================== W9
@functools.lru_cache(maxsize=None)
def w9_long_lines(seed=0):
    """Lines across the whole 256 x 256 frame: slope exactly 1 through every tile corner of the diagonal (both diagonals), and
    shallower and steeper ones; each has a 256-tile bbox (bin_big's strided path) of which about 31 tiles hold a pixel."""
    rng = np.random.default_rng(7900 + seed)
    c = lambda: _rgb(rng, 0.5)
    tris = [
        (V(0.5, 0.5, 0.0, c()), V(255.5, 255.5, 0.5, c()), V(0.5, 255.5, 0.0, c())),
        (V(255.5, 0.5, -0.5, c()), V(0.5, 255.5, 0.5, c()), V(255.5, 255.5, 0.0, c())),
        (V(0.5, 0.5, 0.25, c()), V(255.5, 250.5, 0.0, c()), V(255.5, 0.5, 0.0, c())),
        (V(2.5, 255.5, 0.0, c()), V(250.5, 0.5, 0.75, c()), V(128.5, 0.5, 0.0, c())),
        (V(0.5, 15.5, 0.0, c()), V(255.5, 240.5, -0.25, c()), V(0.5, 240.5, 0.0, c())),
    ]
    return [_scene("w9_long_lines", 256, 256, [_triangle_draw(tris, 256, 256)])]


FAMILIES = {"w1": w1_half_pixel_ties, "w2": w2_bbox_and_frame_edges, "w3": w3_end_caps, "w4": w4_magnitude_ladder, "w5": w5_line_depth,
            "w6": w6_alpha_and_varyings, "w7": w7_shared_pixels, "w8": w8_empty_pairs, "w9": w9_long_lines}


def family(tag, seed=0) -> List[scenes.Scene]:
    return list(FAMILIES[tag](seed))


@functools.lru_cache(maxsize=None)
def all_scenes(seed=0):
    return {s.name: s for f in FAMILIES for s in family(f, seed)}


# =============================================================================================== the restatement: .NET scalars
def f2i(f):
    """(int)float of .NET 9 on x64: saturating, NaN -> 0, truncating."""
    f = F32(f)
    if f != f:
        return 0
    if f >= F32(2147483648.0):
        return 2 ** 31 - 1
    if f <= F32(-2147483648.0):
        return -2 ** 31
    return int(f)


def _neg(f):
    return bool(np.signbit(f))


def mathf_min(a, b):
    """MathF.Min: NaN-propagating, -0 < +0."""
    a, b = F32(a), F32(b)
    if a != b:
        return (a if a < b else b) if a == a else a
    return a if _neg(a) else b


def mathf_max(a, b):
    a, b = F32(a), F32(b)
    if a != b:
        return (a if b < a else b) if a == a else a
    return a if _neg(b) else b


def line_bbox(p0, p1, W, H, floor_bbox=False):
    """DrawLine's pixel bbox (Rasterizer.cs:242-247): truncating casts of the clamped extremes; (minX, maxX, minY, maxY).
    floor_bbox: what a rasteriser that floors before the cast would take."""
    cast = (lambda f: f2i(np.floor(f))) if floor_bbox else f2i
    return (cast(mathf_max(mathf_min(p0[0], p1[0]), F32(0.0))), cast(mathf_min(mathf_max(p0[0], p1[0]), F32(W - 1))),
            cast(mathf_max(mathf_min(p0[1], p1[1]), F32(0.0))), cast(mathf_min(mathf_max(p0[1], p1[1]), F32(H - 1))))


def _f32_of_fraction(q):
    """The float32 nearest to the rational q (ties to even): for the few fused results that float64 cannot round in one step."""
    c = F32(float(q))
    best = None
    for cand in (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - q)
        even = (int(np.array(cand, F32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    return best[1]


def fma32(a, b, c):
    """fmaf on float32 arrays: a * b is exact in float64; the sum is rounded once to float64 and again to float32, which is the
    single rounding unless the float64 sum sits exactly half way between two float32 values -- those elements are redone exactly."""
    a, b, c = (np.asarray(v, F32) for v in np.broadcast_arrays(a, b, c))
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    r = s.astype(F32)
    half = np.isfinite(s) & ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000))
    if half.any():
        r = r.copy()
        for i in zip(*np.nonzero(half)):
            r[i] = _f32_of_fraction(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return r


def line_test(p0, p1, xs, ys, threshold=0.25, fused=False, clamp_drops_nan=False):
    """Rasterizer.cs:257-259, 296-313 for pixel arrays xs, ys (integers): (lit, t, dist_sq), every intermediate rounded to float32,
    one multiply and one add at a time.  fused: the numerator's second multiply-add and the two of the closest point as fmaf
    (fused="numerator": the numerator's alone).
    clamp_drops_nan: t clamped with fminf / fmaxf, which return the other operand for a NaN, instead of MathF.Min / MathF.Max."""
    with np.errstate(all="ignore"):
        p0x, p0y, p1x, p1y = F32(p0[0]), F32(p0[1]), F32(p1[0]), F32(p1[1])
        dx, dy = F32(p1x - p0x), F32(p1y - p0y)
        len_sq = F32(F32(dx * dx) + F32(dy * dy))
        cxs = np.asarray(xs).astype(F32) + F32(0.5)
        cys = np.asarray(ys).astype(F32) + F32(0.5)
        px, py = cxs - p0x, cys - p0y
        t = np.zeros(px.shape, F32)
        if len_sq > 0:
            num = fma32(px, dx, py * dy) if fused else px * dx + py * dy
            t = (num / len_sq).astype(F32)
        if clamp_drops_nan:
            t = np.fmax(F32(0.0), np.fmin(F32(1.0), t))
        else:
            t = np.where(np.isnan(t), t, np.maximum(F32(0.0), np.minimum(F32(1.0), t)))      # (+-0 cannot meet here: 0 <= 1)
            t = np.where(t == 0, np.where(np.signbit(t), F32(0.0), t), t)                      # MathF.Max(0, -0) = +0
        t = t.astype(F32)
        cx = fma32(t, dx, p0x) if fused is True else p0x + t * dx
        cy = fma32(t, dy, p0y) if fused is True else p0y + t * dy
        ddx, ddy = cxs - cx, cys - cy
        dist_sq = (ddx * ddx + ddy * ddy).astype(F32)
        return dist_sq <= F32(threshold), t, dist_sq


def line_depth(d0, d1, t):
    """Rasterizer.cs:315."""
    with np.errstate(all="ignore"):
        t = np.asarray(t, F32)
        den = (F32(d0) * (F32(1.0) - t) + F32(d1) * t).astype(F32)
        return (F32(1.0) / den).astype(F32), den


def line_alpha(a0, a1, w0, w1, t, interp=True):
    """The alpha the built-in programs without a texture return for a line fragment: Rasterizer.Interpolate (:576-585) with the
    weights (1 - t, t, 0) on outputs[0], outputs[1], outputs[0]; flat: outputs[0]'s."""
    with np.errstate(all="ignore"):
        t = np.asarray(t, F32)
        if not interp:
            return np.full(t.shape, F32(a0), F32)
        ra, rb, rc = (F32(1.0) - t) / F32(w0), t / F32(w1), np.zeros(t.shape, F32) / F32(w0)
        w = F32(1.0) / ((ra + rb) + rc)
        return (((F32(a0) * ra + F32(a1) * rb) + F32(a0) * rc) * w).astype(F32)


def exact_distance_sq(p0, p1, x, y):
    """Squared distance, as a Fraction, of the centre of pixel (x, y) from the segment between the (float32) points p0, p1."""
    p0x, p0y, p1x, p1y = (Fraction(float(F32(v))) for v in (*p0, *p1))
    dx, dy = p1x - p0x, p1y - p0y
    px, py = Fraction(x) + Fraction(1, 2) - p0x, Fraction(y) + Fraction(1, 2) - p0y
    L = dx * dx + dy * dy
    t = max(Fraction(0), min(Fraction(1), (px * dx + py * dy) / L)) if L else Fraction(0)
    ex, ey = px - t * dx, py - t * dy
    return ex * ex + ey * ey


def depth_func(test, nd, od):
    """GetDepthTestFunction, Rasterizer.cs:543-559 (names inverted as written)."""
    with np.errstate(all="ignore"):
        test = DepthTest(test)
        if test == DepthTest.LessEqual:
            return nd >= od
        if test == DepthTest.Less:
            return nd > od
        if test == DepthTest.Greater:
            return nd < od
        if test == DepthTest.GreaterEqual:
            return nd <= od
        if test == DepthTest.Equal:
            return np.abs((nd - od).astype(F32)) < EPSILON
        if test == DepthTest.NotEqual:
            return np.abs((nd - od).astype(F32)) >= EPSILON
        return np.ones(np.shape(nd), bool)              # Disabled, Always


# =============================================================================================== the restatement: a scene's lines
@dataclass
class Line:
    p0: tuple                       # float32 screen points
    p1: tuple
    d0: np.float32                  # depths[0], depths[1] of the TRIANGLE
    d1: np.float32
    a0: np.float32                  # colour alpha and clip.w of outputs[0], outputs[1]
    a1: np.float32
    w0: np.float32
    w1: np.float32
    interp: bool
    draw: int
    triangle: int                   # submitted triangle of the batch
    fan: int                        # fan triangle of its clipped polygon
    edge: int


def _vertex_outputs(lib, draw):
    v = np.ascontiguousarray(draw.vertices)
    m, vw, p = (np.ascontiguousarray(a, dtype=F32).reshape(-1) for a in (draw.model, draw.view, draw.projection))
    out = (ob.OVertexOutput * v.shape[0])()
    for i in range(v.shape[0]):
        lib.oswr_vertex_shader(v.ctypes.data + i * v.dtype.itemsize, m.ctypes.data, vw.ctypes.data, p.ctypes.data, int(draw.program), C.byref(out[i]))
    return out


def scene_lines(scene, lib=None) -> List[Line]:
    """Every DrawLine call of the scene in the reference's order.  The vertex stage and the near clipper are the oracle's own
    (oswr_vertex_shader, oswr_clip_triangle: tested in tests/test_geometry_edges_host.py); DrawTriangle's mapping to the screen
    (Rasterizer.cs:362-399), the culling (:411-417) and the three calls (:419-425) are restated here."""
    lib = lib or ob.load()
    W, H = scene.width, scene.height
    lines, tri_no = [], 0
    with np.errstate(all="ignore"):
        for di, d in enumerate(scene.draws):
            vo = _vertex_outputs(lib, d)
            idx = d.indices.astype(np.int64).reshape(-1, 3)
            for tri in idx:
                v = (ob.OVertexOutput * 3)(*[vo[int(k)] for k in tri])
                behind = [v[k].clip[3] <= 0 for k in range(3)]
                polys = []
                if all(behind):
                    pass
                elif any(behind):
                    poly = (ob.OVertexOutput * 4)()
                    n = lib.oswr_clip_triangle(F32(scene.near_clip), v, poly)
                    polys = [(poly[0], poly[k], poly[k + 1]) for k in range(1, n - 1)] if n >= 3 else []
                else:
                    polys = [(v[0], v[1], v[2])]
                for fan, (v0, v1, v2) in enumerate(polys):
                    o = (v2, v1, v0)                                                            # :367
                    sx, sy, dz, ok = [], [], [], True
                    for k in range(3):
                        cl = [F32(c) for c in o[k].clip]
                        inv_w = F32(1.0) / cl[3]
                        nx, ny, nz = F32(cl[0] * inv_w), F32(cl[1] * inv_w), F32(cl[2] * inv_w)
                        if not (np.isfinite(nx) and np.isfinite(ny) and np.isfinite(nz)):
                            ok = False
                            break
                        sx.append(F32(F32(F32(nx * F32(0.5)) + F32(0.5)) * F32(W)))
                        sy.append(F32(F32(F32(1.0) - F32(F32(ny * F32(0.5)) + F32(0.5))) * F32(H)))
                        dz.append(F32(F32(nz + F32(1.0)) * F32(0.5)))
                    if not ok or any(F32(x.clip[3]) == 0 for x in o):
                        continue
                    area = F32(F32(F32(sx[2] - sx[0]) * F32(sy[1] - sy[0])) - F32(F32(sy[2] - sy[0]) * F32(sx[1] - sx[0])))   # :562-563
                    if area == 0:
                        continue
                    front = bool(area < 0)
                    if (d.cull == CullMode.Back and not front) or (d.cull == CullMode.Front and front):
                        continue
                    for e in range(3):
                        i0, i1 = e, (e + 1) % 3
                        lines.append(Line((sx[i0], sy[i0]), (sx[i1], sy[i1]), dz[0], dz[1], F32(o[0].color[3]), F32(o[1].color[3]),
                                          F32(o[0].clip[3]), F32(o[1].clip[3]), bool(o[0].interpolate), di, tri_no, fan, e))
                tri_no += 1
    return lines


@dataclass
class Restated:
    depth: np.ndarray               # (H, W) float32: the depth buffer after the frame
    hits: np.ndarray                # (H, W) tested fragments per pixel
    written: np.ndarray             # (H, W) written fragments per pixel
    frags: dict                     # per fragment, in the reference's order: line, x, y, t, depth, den, alpha, shaded, written
    lines: List[Line]
    boxes: list                     # per line (minX, maxX, minY, maxY) or None where DrawLine returns at once
    tile_pairs: int                 # tiles of all boxes: what binning keeps in wireframe
    t_nan_in_box: int               # pixels of a box whose t came out NaN

    @property
    def lit(self):
        return self.hits > 0

    def counters(self):
        return {"fragments_tested": int(self.hits.sum()), "fragments_shaded": int(self.frags["shaded"].sum()),
                "fragments_written": int(self.frags["written"].sum())}


def restate(scene, threshold=0.25, fused=False, floor_bbox=False, clamp_drops_nan=False, lines=None) -> Restated:
    """The scene's wireframe frame -- lit pixels, depth words, the counters -- from the restatement alone.  Fragments of a line
    are listed tile by tile (row-major), inside a tile row by row, as DrawLine walks them."""
    W, H = scene.width, scene.height
    lines = scene_lines(scene) if lines is None else lines
    depth = np.full((H, W), FLOAT_MIN, F32)
    hits, wr = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    cols = {k: [] for k in ("line", "x", "y", "t", "depth", "den", "alpha", "shaded", "written")}
    boxes, pairs, t_nan = [], 0, 0
    for li, ln in enumerate(lines):
        d = scene.draws[ln.draw]
        x0, x1, y0, y1 = line_bbox(ln.p0, ln.p1, W, H, floor_bbox)
        if x0 > x1 or y0 > y1:
            boxes.append(None)
            continue
        boxes.append((x0, x1, y0, y1))
        pairs += (x1 // TILE - x0 // TILE + 1) * (y1 // TILE - y0 // TILE + 1)
        ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        lit, t, _ = line_test(ln.p0, ln.p1, xs, ys, threshold, fused, clamp_drops_nan)
        t_nan += int(np.isnan(t).sum())
        ys, xs, t = ys[lit], xs[lit], t[lit]
        order = np.lexsort((xs, ys, xs // TILE, ys // TILE))
        ys, xs, t = ys[order], xs[order], t[order]
        dep, den = line_depth(ln.d0, ln.d1, t)
        alpha = line_alpha(ln.a0, ln.a1, ln.w0, ln.w1, t, ln.interp)
        shaded = depth_func(d.depth_test, dep, depth[ys, xs])
        written = shaded & (alpha != 0)
        np.add.at(hits, (ys, xs), 1)
        np.add.at(wr, (ys[written], xs[written]), 1)
        if d.depth_test != DepthTest.Disabled:
            depth[ys[written], xs[written]] = dep[written]
        for k, v in (("line", np.full(t.shape, li)), ("x", xs), ("y", ys), ("t", t), ("depth", dep), ("den", den), ("alpha", alpha),
                     ("shaded", shaded), ("written", written)):
            cols[k].append(v)
    frags = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in cols.items()}
    return Restated(depth, hits, wr, frags, lines, boxes, pairs, t_nan)


def tile_stream(r: Restated, tx, ty):
    """The pixels (y * 16 + x inside the tile) of tile (tx, ty)'s fragment stream in list order."""
    f = r.frags
    m = (f["x"] // TILE == tx) & (f["y"] // TILE == ty)
    return ((f["y"][m] % TILE) * TILE + f["x"][m] % TILE).astype(np.int64), f["line"][m].astype(np.int64)


def tile_list(r: Restated, tx, ty):
    """Tile (tx, ty)'s list of pairs in submission order: (line, fragments of the line in the tile)."""
    out = []
    f = r.frags
    in_tile = (f["x"] // TILE == tx) & (f["y"] // TILE == ty)
    for li, b in enumerate(r.boxes):
        if b is not None and b[0] // TILE <= tx <= b[1] // TILE and b[2] // TILE <= ty <= b[3] // TILE:
            out.append((li, int((in_tile & (f["line"] == li)).sum())))
    return out
