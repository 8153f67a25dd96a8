"""Mip chains (include/swr.h) restated in numpy, and the program texts of tests/test_mipmap_host.py and
tests/test_gpu_mipmaps.py.

The downsample is integer arithmetic; the lod works on the bits of a float32; sample_level / sample_lod are float32, operation for
operation, over post_texture_cases.numpy_nearest and the bilinear footprint of depth_texture_cases; the gradient stands beside
program_probe_cases.fs_in_reference and shares its Weights.  Nothing here has a tolerance: the GPU tests compare words."""
from __future__ import annotations

import functools

import numpy as np

import depth_texture_cases as D
import post_cases as P
import post_texture_cases as X
import program_probe_cases as PC
import shade_edge_scenes as S
import vertex_probe_cases as VC

F32 = np.float32
INV255 = X.INV255
ONES = np.ones(4, dtype=F32)
MAX_LEVELS = 32

# (w, h): the smallest shapes that reach every branch
SHAPES = [(1, 1),        # L = 1
          (2, 2),        # the smallest with a second level
          (5, 7),        # odd sides: 5 x 7 -> 2 x 3 -> 1 x 1
          (12, 20),      # not square, even sides; sides multiples of 4: two levels in one launch
          (1, 16), (16, 1),      # a side that reaches 1 early: the clamp bites
          (33, 17),      # odd sides that are no power of two
          (64, 64),      # a full power-of-two chain
          (68, 8)]       # a block-linear level 0 under the bilinear filter
SAMPLE_SHAPES = [(5, 7), (12, 20), (68, 8), (1, 16)]

# the rounding, by hand: four bytes of a 2 x 2 block -> the byte of the next level
KNOWN_BLOCKS = [((0, 0, 0, 1), 0), ((0, 0, 1, 1), 1), ((0, 1, 1, 1), 1), ((255, 255, 255, 254), 255), ((255, 255, 254, 254), 255),
                ((255, 255, 255, 255), 255)]


# ---- the level table -------------------------------------------------------------------------------------------------------------
def full_levels(w, h):
    """L = 1 + floor(log2(max(w, h)))"""
    return int(max(w, h)).bit_length()


def level_size(w, h, level):
    return max(1, w >> level), max(1, h >> level)


def offsets(w, h):
    """offset[l], l >= 1: level l's first texel in the tail, in texels; offset[0] = 0"""
    off, at = [0], 0
    for l in range(1, full_levels(w, h)):
        off.append(at)
        wl, hl = level_size(w, h, l)
        at += wl * hl
    return off


# ---- the downsample, in integers -------------------------------------------------------------------------------------------------
def downsample(level):
    """(h, w, 4) uint8 -> (max(1, h >> 1), max(1, w >> 1), 4) uint8: (p(x0, y0) + p(x1, y0) + p(x0, y1) + p(x1, y1) + 2) >> 2 per byte,
    x1 = min(2x + 1, w - 1), y1 = min(2y + 1, h - 1).  An odd side >= 3 drops its last column or row."""
    t = np.asarray(level, dtype=np.uint8).astype(np.int64)
    h, w = t.shape[:2]
    dw, dh = max(1, w >> 1), max(1, h >> 1)
    x0, y0 = 2 * np.arange(dw), 2 * np.arange(dh)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    s = t[y0][:, x0] + t[y0][:, x1] + t[y1][:, x0] + t[y1][:, x1] + 2
    return (s >> 2).astype(np.uint8)


def chain(texels):
    """[level 0, .., level L - 1]; level l + 1 is made from level l's ROUNDED bytes"""
    levels = [np.ascontiguousarray(texels, dtype=np.uint8)]
    for _ in range(1, full_levels(levels[0].shape[1], levels[0].shape[0])):
        levels.append(downsample(levels[-1]))
    return levels


@functools.lru_cache(maxsize=None)
def texture(size, seed=0):
    """(h, w, 4) uint8, read-only: seeded random bytes, and where they fit the KNOWN_BLOCKS planted as 2 x 2 blocks (one per channel
    rotation) so that every rounding case is in every big enough texture."""
    w, h = size
    t = np.random.default_rng(9000 + 131 * w + h + seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    for i, (block, _) in enumerate(KNOWN_BLOCKS):
        x, y = 2 * i, 2 * (i % max(1, h // 2))
        if x + 1 < w and y + 1 < h:
            for c in range(4):
                t[y:y + 2, x:x + 2, c] = np.roll(np.array(block, dtype=np.uint8), c).reshape(2, 2)
    t.setflags(write=False)
    return t


def checkerboard(n=64):
    """n x n, one-texel checks of 0 and 255 in R, G, B, alpha 255: every level >= 1 is 128 (127.5 rounds half up)."""
    y, x = np.mgrid[0:n, 0:n]
    t = np.empty((n, n, 4), dtype=np.uint8)
    t[..., :3] = (((x + y) & 1) * 255)[..., None]
    t[..., 3] = 255
    return t


# ---- the lod, on bits ------------------------------------------------------------------------------------------------------------
def lod(w, h, grads, levels):
    """texture_slot_lod: grads (..., 4) = (dudx, dvdx, dudy, dvdy) float32 -> float32.  levels 0: an unbound slot, 0."""
    g = np.asarray(grads, dtype=F32)
    if levels == 0:
        return np.zeros(g.shape[:-1], dtype=F32)
    wf, hf = F32(w), F32(h)
    with np.errstate(all="ignore"):
        ax, ay = (g[..., 0] * wf).astype(F32), (g[..., 1] * hf).astype(F32)
        bx, by = (g[..., 2] * wf).astype(F32), (g[..., 3] * hf).astype(F32)
        rx = ((ax * ax).astype(F32) + (ay * ay).astype(F32)).astype(F32)
        ry = ((bx * bx).astype(F32) + (by * by).astype(F32)).astype(F32)
        r2 = np.where((ry > rx) | np.isnan(ry), ry, rx).astype(F32)       # the larger; a NaN from either side
        rho = np.sqrt(r2).astype(F32)                                      # correctly rounded on both sides
        big = rho > F32(1.0)                                               # false for NaN
    bits = np.ascontiguousarray(np.where(big, rho, F32(2.0)).astype(F32)).view(np.uint32)
    e = (bits >> np.uint32(23)).astype(np.int64) - 127
    m = ((bits & np.uint32(0x007fffff)) | np.uint32(0x3f800000)).view(F32)
    out = (e.astype(F32) + (m - F32(1.0)).astype(F32)).astype(F32)
    top = F32(levels - 1)
    out = np.where(out > top, top, out)
    return np.where(big, out, F32(0.0)).astype(F32)


# ---- sample_level, sample_lod ----------------------------------------------------------------------------------------------------
def bilinear(texels, uv):
    """swr::texture_sample_bilinear in float32, operation for operation, over depth_texture_cases.footprint"""
    t = np.asarray(texels, dtype=np.uint8)
    h, w = t.shape[:2]
    ix0, ix1, iy0, iy1, fx, fy = D.footprint(w, h, uv)
    one = F32(1.0)
    fx, fy = fx[..., None], fy[..., None]
    c00, c10 = (t[iy0, ix0].astype(F32) * INV255).astype(F32), (t[iy0, ix1].astype(F32) * INV255).astype(F32)
    c01, c11 = (t[iy1, ix0].astype(F32) * INV255).astype(F32), (t[iy1, ix1].astype(F32) * INV255).astype(F32)
    top = ((c00 * (one - fx)).astype(F32) + (c10 * fx).astype(F32)).astype(F32)
    bot = ((c01 * (one - fx)).astype(F32) + (c11 * fx).astype(F32)).astype(F32)
    return ((top * (one - fy)).astype(F32) + (bot * fy).astype(F32)).astype(F32)


def sample_level(levels, filtered, level, uv, have=None):
    """texture_slot_sample_level: levels = chain(texels) (None: unbound), have = the levels the texture HAS (1 without a chain)."""
    uv = np.asarray(uv, dtype=F32)
    if levels is None:
        return np.broadcast_to(ONES, uv.shape[:-1] + (4,)).copy()
    have = len(levels) if have is None else have
    level = np.broadcast_to(np.clip(np.asarray(level, dtype=np.int64), 0, have - 1), uv.shape[:-1])
    out = np.zeros(uv.shape[:-1] + (4,), dtype=F32)
    for l in np.unique(level):
        sel = level == l
        out[sel] = bilinear(levels[l], uv[sel]) if filtered else X.numpy_nearest(levels[l], uv[sel])
    return out


def sample_lod(levels, filtered, uv, lod_, have=None):
    """texture_slot_sample_lod: NaN or negative -> 0, above the top -> the top; l0 = (int)lod, f = lod - l0; c0 (1 - f) + c1 f."""
    uv = np.asarray(uv, dtype=F32)
    if levels is None:
        return np.broadcast_to(ONES, uv.shape[:-1] + (4,)).copy()
    have = len(levels) if have is None else have
    top = F32(have - 1)
    l = np.broadcast_to(np.asarray(lod_, dtype=F32), uv.shape[:-1]).copy()
    with np.errstate(invalid="ignore"):
        l = np.where(l > 0, l, F32(0.0)).astype(F32)
        l = np.where(l > top, top, l).astype(F32)
    l0 = l.astype(np.int64)
    f = (l - l0.astype(F32)).astype(F32)[..., None]
    c0 = sample_level(levels, filtered, l0, uv, have)
    c1 = sample_level(levels, filtered, np.minimum(l0 + 1, have - 1), uv, have)
    mixed = ((c0 * (F32(1.0) - f)).astype(F32) + (c1 * f).astype(F32)).astype(F32)
    return np.where(f == 0, c0, mixed).astype(F32)


def lookup_uvs(w, h, seed=0):
    """texel centres, texel corners, wraps and negatives of a w x h level 0, and a few random ones"""
    cx, cy = (np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h
    kx, ky = np.arange(w + 1) / w, np.arange(h + 1) / h
    pts = [(u, v) for u in cx[:6] for v in cy[:6]] + [(u, v) for u in kx[:5] for v in ky[:5]]
    pts += [(u + 1.0, v - 2.0) for u in cx[:3] for v in cy[:3]] + [(-u, -v) for u in kx[1:4] for v in cy[:3]]
    rnd = np.random.default_rng(50 + seed).uniform(-2.0, 3.0, (24, 2))
    return np.concatenate([np.array(pts, dtype=F32), rnd.astype(F32)])


def lods_for(levels):
    return np.array([np.nan, -1.0, 0.0, 0.25, 0.5, 1.0, 1.75, levels - 1, levels, np.inf], dtype=F32)


def gradient_ladder(w, h, levels):
    """zeros; rho exactly 1, 2, 4 and 2^(L - 1), axis-aligned (r2 exact); values between; anisotropic pairs in both orders; subnormals;
    an overflow to +Inf; a NaN in each position"""
    g = [(0, 0, 0, 0)]
    for rho in (1.0, 2.0, 4.0, float(2 ** (levels - 1))):
        g += [(rho / w, 0, 0, 0), (0, 0, 0, rho / h), (0, rho / h, 0, 0), (0, 0, rho / w, 0)]
    for rho in (0.5, 1.0000001, 1.5, 2.9, 3.999, 5.3, 100.0, 1e6):
        g += [(rho / w, 0, 0, 0.1 / h), (0.3 / w, 0.2 / h, rho * 0.6 / w, rho * 0.8 / h)]
    g += [(3.0 / w, 0, 0, 7.0 / h), (7.0 / w, 0, 0, 3.0 / h), (1e-42, 0, 0, 1e-44), (1e-40, 1e-41, 0, 0), (3e38, 3e38, 0, 0), (1e30, 0, 0, -1e30)]
    nan = float("nan")
    g += [(nan, 0, 0, 0), (0, nan, 0, 0), (0, 0, nan, 0), (0, 0, 0, nan), (nan, 0, 8.0 / w, 0), (8.0 / w, 0, 0, nan)]
    return np.array(g, dtype=F32)


# ---- the gradient ----------------------------------------------------------------------------------------------------------------
def tex_coord_grad(tri, rect, dtype=F32):
    """in.tex_coord_grad over the covered samples of (tri, rect): (n, 4) = (du/dx, dv/dx, du/dy, dv/dy).  float32: the restatement, in
    the operation order of interpolate_fs_in (csrc/swr_program.hip.h), from the weights the raster stage hands over.  float64: the
    same closed form from the same float32 vertices, with the barycentrics of the sample's position in float64."""
    T = dtype
    t, o = tri.tri, tri.out
    with np.errstate(all="ignore"):
        k = S.Weights(t, rect, o["clip"][:, 3])
        sx, sy = np.asarray(t.sx, dtype=F32).astype(T), np.asarray(t.sy, dtype=F32).astype(T)
        cw = o["clip"][:, 3].astype(T)
        u, v = o["uv"][:, 0].astype(T), o["uv"][:, 1].astype(T)
        area = (sx[2] - sx[0]) * (sy[1] - sy[0]) - (sy[2] - sy[0]) * (sx[1] - sx[0])
        ia = T(1.0) / area
        gx = [(sy[1] - sy[2]) * ia, (sy[2] - sy[0]) * ia, (sy[0] - sy[1]) * ia]
        gy = [(sx[2] - sx[1]) * ia, (sx[0] - sx[2]) * ia, (sx[1] - sx[0]) * ia]
        if T is F32:
            w, tu, tv = k.w, k.persp(*o["uv"][:, 0]), k.persp(*o["uv"][:, 1])
        else:
            sX, eX, sY, eY = rect
            xs, ys = np.meshgrid(np.arange(sX, eX + 1, dtype=T), np.arange(sY, eY + 1, dtype=T))
            x, y = xs[k.inside], ys[k.inside]
            r = [(gx[i] * (x - sx[(i + 1) % 3]) + gy[i] * (y - sy[(i + 1) % 3])) / cw[i] for i in range(3)]
            w = T(1.0) / ((r[0] + r[1]) + r[2])
            tu, tv = ((u[0] * r[0] + u[1] * r[1]) + u[2] * r[2]) * w, ((v[0] * r[0] + v[1] * r[1]) + v[2] * r[2]) * w
        out = []
        for g in (gx, gy):
            q = [g[i] / cw[i] for i in range(3)]
            d = (q[0] + q[1]) + q[2]
            nu = (u[0] * q[0] + u[1] * q[1]) + u[2] * q[2]
            nv = (v[0] * q[0] + v[1] * q[1]) + v[2] * q[2]
            out += [(nu - tu * d) * w, (nv - tv * d) * w]
    return np.stack([np.asarray(c, dtype=T) for c in out], axis=1)


def depth_slope(tri, rect):
    """|D'| / |D| per pixel step, the larger of x and y, over the covered samples: what the finite-difference bound rests on"""
    t, o = tri.tri, tri.out
    sx, sy = np.asarray(t.sx, dtype=np.float64), np.asarray(t.sy, dtype=np.float64)
    cw = o["clip"][:, 3].astype(np.float64)
    area = (sx[2] - sx[0]) * (sy[1] - sy[0]) - (sy[2] - sy[0]) * (sx[1] - sx[0])
    gx = [(sy[1] - sy[2]) / area, (sy[2] - sy[0]) / area, (sy[0] - sy[1]) / area]
    gy = [(sx[2] - sx[1]) / area, (sx[0] - sx[2]) / area, (sx[1] - sx[0]) / area]
    with np.errstate(all="ignore"):
        inside = t.cover(rect)[0]
    sX, eX, sY, eY = rect
    xs, ys = np.meshgrid(np.arange(sX, eX + 1, dtype=np.float64), np.arange(sY, eY + 1, dtype=np.float64))
    x, y = xs[inside], ys[inside]
    D = sum((gx[i] * (x - sx[(i + 1) % 3]) + gy[i] * (y - sy[(i + 1) % 3])) / cw[i] for i in range(3))
    dx, dy = sum(gx[i] / cw[i] for i in range(3)), sum(gy[i] / cw[i] for i in range(3))
    return np.maximum(np.abs(dx), np.abs(dy)) / np.abs(D)


def tex_coord_at(tri, x, y):
    """tex_coord of `tri`'s plane at the real pixel position (x, y), in float64: the function the gradient differentiates"""
    t, o = tri.tri, tri.out
    sx, sy = np.asarray(t.sx, dtype=np.float64), np.asarray(t.sy, dtype=np.float64)
    cw, uv = o["clip"][:, 3].astype(np.float64), o["uv"].astype(np.float64)
    area = (sx[2] - sx[0]) * (sy[1] - sy[0]) - (sy[2] - sy[0]) * (sx[1] - sx[0])
    b = [((sy[(i + 1) % 3] - sy[(i + 2) % 3]) * (x - sx[(i + 1) % 3]) + (sx[(i + 2) % 3] - sx[(i + 1) % 3]) * (y - sy[(i + 1) % 3])) / area
         for i in range(3)]
    r = [b[i] / cw[i] for i in range(3)]
    den = r[0] + r[1] + r[2]
    return np.stack([(uv[0, c] * r[0] + uv[1, c] * r[1] + uv[2, c] * r[2]) / den for c in range(2)], axis=-1)


def grad_planes(scene, tris=None):
    """{"grad.x" .. "grad.w": (H, W) float32 plane} of in.tex_coord_grad, beside program_probe_cases.expected_planes"""
    planes = {n: np.zeros((scene.height, scene.width), dtype=F32) for n in GRAD_NAMES}
    for t in (PC.probe_tris(scene) if tris is None else tris):
        for rect in t.rects():
            with np.errstate(all="ignore"):
                inside = t.tri.cover(rect)[0]
            g = tex_coord_grad(t, rect)
            sX, eX, sY, eY = rect
            for i, n in enumerate(GRAD_NAMES):
                planes[n][sY:eY + 1, sX:eX + 1][inside] = g[:, i]
    return planes


GRAD_NAMES = ("grad.x", "grad.y", "grad.z", "grad.w")

# ---- the program texts -----------------------------------------------------------------------------------------------------------
GRAD_XYZ = PC.HEAD + "    return make_float4(in.tex_coord_grad.x, in.tex_coord_grad.y, in.tex_coord_grad.z, 1.0f);\n}\n"
GRAD_WXY = PC.HEAD + "    return make_float4(in.tex_coord_grad.w, in.tex_coord_grad.x, in.tex_coord_grad.y, 1.0f);\n}\n"
SLOT, PER_PIXEL = 8, 99.0
# (lod, levels, sample.x, 1) of slot constants[8] (99: chosen per pixel), through the gradient
CHAIN_PROBE = PC.HEAD + f"""    const int s = env.constants[{SLOT}] == {PER_PIXEL!r}f ? (env.x + env.y) % 5 : (int)env.constants[{SLOT}];
    return make_float4(swr_lod(env, s, in.tex_coord_grad), (float)swr_texture_levels(env, s),
                       swr_sample_grad(env, s, in.tex_coord, in.tex_coord_grad).x, 1.0f);
}}
"""
# the recipe of INTEGRATION.md: Renderer.FragmentShader's texture fetch through the chain
RECIPE = PC.HEAD + """    const float4 t = swr_sample_grad(env, 0, in.tex_coord, in.tex_coord_grad);
    return make_float4(t.x, t.y, t.z, 1.0f);
}
"""
PLAIN = PC.HEAD + """    const float4 t = swr_sample(env, 0, in.tex_coord);
    return make_float4(t.x, t.y, t.z, 1.0f);
}
"""
# slot 1 at lod constants[0], at the pixel's own uv: the order test
LOD_CONSTANT = PC.HEAD + """    return swr_sample_lod(env, 1, in.tex_coord, env.constants[0]);
}
"""
LEVEL_CONSTANT = PC.HEAD + """    const float4 t = swr_sample_level(env, 1, in.tex_coord, (int)env.constants[0]);
    return make_float4(t.x, t.y, (float)swr_texture_levels(env, 1), 1.0f);
}
"""
POST_PROBE = P.HEAD + X.UV + """    const float4 a = swr_post_sample_lod(env, 0, make_float2(u, v), env.constants[5]);
    const float4 b = swr_post_sample_level(env, 0, make_float2(u, v), (int)env.constants[6]);
    return make_float4(a.x, b.y, (float)swr_post_texture_levels(env, 1) + swr_post_lod(env, 0, make_float4(env.constants[7], 0.0f, 0.0f, 0.0f)), a.w);
}
"""
# the vertex half: slot 1 at the vertex's uv and level constants[0] into data4; the fragment half is program_probe_cases.PROBE_ALL
VERTEX_PROBE = (VC.VS_HEAD + VC.CLIP_RENDERER +
                "    const float4 t = swr_sample_level(env, 1, in.uv, (int)env.constants[0]);\n"
                "    out.data4 = make_float4(t.x, t.y, (float)swr_texture_levels(env, 1), swr_sample_lod(env, 1, in.uv, env.constants[1]).z);\n}\n")
FRAGMENT_TEXTS = {"GRAD_XYZ": GRAD_XYZ, "GRAD_WXY": GRAD_WXY, "CHAIN_PROBE": CHAIN_PROBE, "RECIPE": RECIPE, "PLAIN": PLAIN,
                  "LOD_CONSTANT": LOD_CONSTANT, "LEVEL_CONSTANT": LEVEL_CONSTANT}
POST_TEXTS = {"POST_PROBE": POST_PROBE}
