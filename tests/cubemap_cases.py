"""Cube maps (include/swr.h, csrc/swr_device.h) restated in numpy float32, operation for operation, the case
pools, and the program texts of tests/test_cubemap_host.py and tests/test_gpu_cubemaps.py.

A cube of side n is the (6 n, n) atlas: face f (0..5 = +X, -X, +Y, -Y, +Z, -Z) in rows [f n, (f + 1) n).  Nothing here has a
tolerance: the GPU tests compare 32-bit words.  The wrong twins at the end each restate one plausible mistake; the host tests name a
case every one of them fails."""
from __future__ import annotations

import functools

import numpy as np

import depth_texture_cases as D
import mipmap_cases as M
import post_cases as P
import program_probe_cases as PC
import vertex_probe_cases as VC

F32 = np.float32
INV255 = M.INV255
ONES = np.ones(4, dtype=F32)
MINVALUE = D.MINVALUE
FLT_MAX = np.finfo(F32).max

SIDES = [1, 2, 3, 4, 5, 8, 16]              # 4, 8, 16: the block-linear copy under the bilinear filter; 2, 8, 16: chains
CHAIN_SIDES = [4, 8, 16]


# ---- the lookup ------------------------------------------------------------------------------------------------------------------
def cube_face(dirs, mirrored=False, strict=False, negative_zero=False):
    """texture_cube_face: dirs (..., 3) float32 -> (face int32 (...), st float32 (..., 2)).  The keyword arguments are the wrong
    twins: GL's table (sc of the X and Z majors negated), `>` for `>=` in the selection, -0 sent to the negative face (which shows at
    the origin alone: a major component is never a zero)."""
    d = np.asarray(dirs, dtype=F32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    with np.errstate(all="ignore"):
        bad = ~((ax <= FLT_MAX) & (ay <= FLT_MAX) & (az <= FLT_MAX)) | ((ax == 0) & (ay == 0) & (az == 0))
        if strict:
            xm = (ax > ay) & (ax > az)
            ym = ~xm & (ay > az)
        else:
            xm = (ax >= ay) & (ax >= az)
            ym = ~xm & (ay >= az)
        neg = (lambda v: np.signbit(v)) if negative_zero else (lambda v: v < 0)
        nx, ny, nz = neg(x), neg(y), neg(z)
        ma = np.where(xm, ax, np.where(ym, ay, az))
        face = np.where(xm, np.where(nx, 1, 0), np.where(ym, np.where(ny, 3, 2), np.where(nz, 5, 4))).astype(np.int32)
        sc = np.where(xm, np.where(nx, -z, z), np.where(ym, x, np.where(nz, x, -x))).astype(F32)
        tc = np.where(xm, -y, np.where(ym, np.where(ny, z, -z), -y)).astype(F32)
        if mirrored:
            sc = np.where(ym, sc, -sc).astype(F32)
        ma = np.where(bad, F32(1.0), ma).astype(F32)
        s = (((sc / ma).astype(F32) + F32(1.0)).astype(F32) * F32(0.5)).astype(F32)
        t = (((tc / ma).astype(F32) + F32(1.0)).astype(F32) * F32(0.5)).astype(F32)
    origin = (ax == 0) & (ay == 0) & (az == 0)
    face = np.where(bad, np.where(origin & np.signbit(x), 1, 0) if negative_zero else 0, face).astype(np.int32)
    st = np.stack([np.where(bad, F32(0.5), s), np.where(bad, F32(0.5), t)], axis=-1).astype(F32)
    return face, st


def nearest_xy(n, st):
    """(min((int)(s n), n - 1), min((int)(t n), n - 1))"""
    x = np.minimum((st[..., 0] * F32(n)).astype(F32).astype(np.int64), n - 1)
    y = np.minimum((st[..., 1] * F32(n)).astype(F32).astype(np.int64), n - 1)
    return x, y


def footprint(n, st, wrap=False):
    """X = s n - 0.5, x0 = floor(X), fx = X - x0; taps x0 and x0 + 1 clamped to [0, n - 1] (wrap: the wrong twin)."""
    X = ((st[..., 0] * F32(n)).astype(F32) - F32(0.5)).astype(F32)
    Y = ((st[..., 1] * F32(n)).astype(F32) - F32(0.5)).astype(F32)
    x0f, y0f = np.floor(X).astype(F32), np.floor(Y).astype(F32)
    fx, fy = (X - x0f).astype(F32), (Y - y0f).astype(F32)
    ix, iy = x0f.astype(np.int64), y0f.astype(np.int64)
    if wrap:
        return ix % n, (ix + 1) % n, iy % n, (iy + 1) % n, fx, fy
    return np.clip(ix, 0, n - 1), np.clip(ix + 1, 0, n - 1), np.clip(iy, 0, n - 1), np.clip(iy + 1, 0, n - 1), fx, fy


def is_cube(atlas):
    return atlas is not None and atlas.shape[1] >= 1 and atlas.shape[0] == 6 * atlas.shape[1]


def level_sample(atlas, filtered, dirs, wrap=False, **twin):
    """the slot's filter inside one level: atlas (6 n, n, 4) uint8 -> (..., 4) float32"""
    n = atlas.shape[1]
    face, st = cube_face(dirs, **twin)
    row = face.astype(np.int64) * n
    if not filtered:
        x, y = nearest_xy(n, st)
        return (atlas[row + y, x].astype(F32) * INV255).astype(F32)
    x0, x1, y0, y1, fx, fy = footprint(n, st, wrap)
    one = F32(1.0)
    fx, fy = fx[..., None], fy[..., None]
    c00, c10 = (atlas[row + y0, x0].astype(F32) * INV255).astype(F32), (atlas[row + y0, x1].astype(F32) * INV255).astype(F32)
    c01, c11 = (atlas[row + y1, x0].astype(F32) * INV255).astype(F32), (atlas[row + y1, x1].astype(F32) * INV255).astype(F32)
    top = ((c00 * (one - fx)).astype(F32) + (c10 * fx).astype(F32)).astype(F32)
    bot = ((c01 * (one - fx)).astype(F32) + (c11 * fx).astype(F32)).astype(F32)
    return ((top * (one - fy)).astype(F32) + (bot * fy).astype(F32)).astype(F32)


def sample_cube(atlas, filtered, dirs, **twin):
    """texture_slot_sample_cube; (1, 1, 1, 1) from a slot that is not a cube (atlas None or not n x 6 n)"""
    dirs = np.asarray(dirs, dtype=F32)
    if not is_cube(atlas):
        return np.broadcast_to(ONES, dirs.shape[:-1] + (4,)).copy()
    return level_sample(atlas, filtered, dirs, **twin)


def cube_texel(atlas, face, x, y):
    if not is_cube(atlas):
        return np.broadcast_to(ONES, np.shape(face) + (4,)).copy()
    n = atlas.shape[1]
    return (atlas[np.clip(face, 0, 5) * n + np.clip(y, 0, n - 1), np.clip(x, 0, n - 1)].astype(F32) * INV255).astype(F32)


def cube_size(atlas):
    return atlas.shape[1] if is_cube(atlas) else 0


def chain(atlas):
    """a cube's chain: the first 1 + log2(n) levels of the atlas's chain, each the (6 n_l, n_l, 4) atlas of n_l = n >> l"""
    n = atlas.shape[1]
    assert n & (n - 1) == 0
    levels = [np.ascontiguousarray(atlas, dtype=np.uint8)]
    while levels[-1].shape[1] > 1:
        levels.append(M.downsample(levels[-1]))
    return levels


def sample_cube_level(levels, filtered, level, dirs):
    """texture_slot_sample_cube_level: levels = the levels the texture HAS ([atlas] without a chain)"""
    dirs = np.asarray(dirs, dtype=F32)
    level = np.broadcast_to(np.clip(np.asarray(level, dtype=np.int64), 0, len(levels) - 1), dirs.shape[:-1])
    out = np.zeros(dirs.shape[:-1] + (4,), dtype=F32)
    for l in np.unique(level):
        sel = level == l
        out[sel] = level_sample(levels[l], filtered, dirs[sel])
    return out


def sample_cube_lod(levels, filtered, dirs, lod):
    """texture_slot_sample_cube_lod: mipmap_cases.sample_lod's blend over sample_cube_level"""
    dirs = np.asarray(dirs, dtype=F32)
    top = F32(len(levels) - 1)
    l = np.broadcast_to(np.asarray(lod, dtype=F32), dirs.shape[:-1]).copy()
    with np.errstate(invalid="ignore"):
        l = np.where(l > 0, l, F32(0.0)).astype(F32)
        l = np.where(l > top, top, l).astype(F32)
    l0 = l.astype(np.int64)
    f = (l - l0.astype(F32)).astype(F32)[..., None]
    c0 = sample_cube_level(levels, filtered, l0, dirs)
    c1 = sample_cube_level(levels, filtered, np.minimum(l0 + 1, len(levels) - 1), dirs)
    mixed = ((c0 * (F32(1.0) - f)).astype(F32) + (c1 * f).astype(F32)).astype(F32)
    return np.where(f == 0, c0, mixed).astype(F32)


def depth_sample(words, dirs):
    """texture_slot_cube_depth_sample: words (6 n, n) float32; always nearest; float.MinValue when not a cube"""
    dirs = np.asarray(dirs, dtype=F32)
    if not is_cube(words):
        return np.full(dirs.shape[:-1], MINVALUE, dtype=F32)
    n = words.shape[1]
    face, st = cube_face(dirs)
    x, y = nearest_xy(n, st)
    return words[face.astype(np.int64) * n + y, x]


def shadow_cube(words, filtered, dirs, ref):
    """texture_slot_shadow_cube: depth_texture_cases.shadow's comparisons and lerps over the clamped footprint; 1 when not a cube"""
    dirs = np.asarray(dirs, dtype=F32)
    if not is_cube(words):
        return np.ones(dirs.shape[:-1], dtype=F32)
    if not filtered:
        return D.passes(ref, depth_sample(words, dirs))
    n = words.shape[1]
    face, st = cube_face(dirs)
    row = face.astype(np.int64) * n
    x0, x1, y0, y1, fx, fy = footprint(n, st)
    c00, c10 = D.passes(ref, words[row + y0, x0]), D.passes(ref, words[row + y0, x1])
    c01, c11 = D.passes(ref, words[row + y1, x0]), D.passes(ref, words[row + y1, x1])
    top = (c00 + ((c10 - c00).astype(F32) * fx).astype(F32)).astype(F32)
    bot = (c01 + ((c11 - c01).astype(F32) * fx).astype(F32)).astype(F32)
    return (top + ((bot - top).astype(F32) * fy).astype(F32)).astype(F32)


# ---- the pools -------------------------------------------------------------------------------------------------------------------
def lattice():
    """the 26 vectors of {-1, 0, 1}^3 without the origin: every tie of the selection order, the edges and the corners"""
    g = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=F32)
    assert len(g) == 26
    return g


def degenerate():
    """the origin with both zero signs, a NaN in each component, +-Inf in each component"""
    nan, inf = F32(np.nan), F32(np.inf)
    out = [(0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.0)]
    for k in range(3):
        for v in (nan, inf, -inf):
            d = [0.25, -0.5, 0.75]
            d[k] = v
            out.append(tuple(d))
    out += [(nan, nan, nan), (inf, inf, -inf)]
    return np.array(out, dtype=F32)


def boundaries(n):
    """directions with sc / ma = 2 k / n - 1 exactly (power-of-two n): texel boundaries, and s = 1; on every face, both axes"""
    q = (np.arange(n + 1, dtype=F32) * F32(2.0) / F32(n) - F32(1.0)).astype(F32)
    out = []
    for a in q:
        for b in (q[0], q[n // 2], q[-1], F32(0.3)):
            out += [(1, a, b), (-1, b, a), (a, 1, b), (b, -1, a), (a, b, 1), (b, a, -1)]
    return np.array(out, dtype=F32)


@functools.lru_cache(maxsize=None)
def directions(n=0):
    """the whole pool, (count, 3) float32, read-only"""
    g = lattice()
    zero = np.where(g == 0, F32(-0.0), g).astype(F32)
    rnd = np.random.default_rng(2700).normal(size=(512, 3)).astype(F32)
    parts = [g, zero, (g * F32(2.0 ** -140)).astype(F32), (g * F32(2.0 ** 120)).astype(F32), degenerate(), rnd]
    if n >= 2 and n & (n - 1) == 0:
        parts.append(boundaries(n))
    d = np.ascontiguousarray(np.concatenate(parts))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def colour_faces(n, seed=0):
    """(6, n, n, 4) uint8, read-only: seeded random bytes; the red byte of texel (0, 0) of face f is 40 f"""
    t = np.random.default_rng(2800 + 17 * n + seed).integers(0, 256, (6, n, n, 4), dtype=np.uint8)
    t[:, 0, 0, 0] = np.arange(6) * 40
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def depth_faces(n, seed=0, finite=False):
    """(6, n, n) float32, read-only: depth_texture_cases' pool plane (the special words included), or its finite one"""
    p = (D.finite_plane if finite else D.depth_pool_plane)(6 * n, n, 40 + n + seed).reshape(6, n, n)
    return p


def atlas(faces):
    """(6, n, n, ...) -> (6 n, n, ...)"""
    f = np.asarray(faces)
    return np.ascontiguousarray(f.reshape((6 * f.shape[1], f.shape[2]) + f.shape[3:]))


def refs_for(words, dirs, seed=0):
    """one ref per direction, dealt from the word the nearest lookup reads and its neighbours one ulp up and down (finite words), and
    from depth_texture_cases' pool"""
    d = depth_sample(words, dirs)
    rng = np.random.default_rng(2900 + seed)
    pick = rng.integers(0, 4, d.shape)
    with np.errstate(all="ignore"):
        up, down = np.nextafter(d, F32(np.inf)), np.nextafter(d, F32(-np.inf))
    pooled = D.lookup_refs(d.size, seed).reshape(d.shape)
    return np.where(pick == 0, d, np.where(pick == 1, up, np.where(pick == 2, down, pooled))).astype(F32)


def lods_for(levels):
    return np.array([np.nan, -1.0, 0.0, 0.25, 0.5, 1.0, 1.75, levels - 1, levels - 0.5, levels, np.inf], dtype=F32)


# ---- the face cameras ------------------------------------------------------------------------------------------------------------
def texel_of_direction_f64(face, d, n):
    """An independent float64 formulation: the direction through hostmath.cube_face_view's camera (at the origin) and the 90 degree
    perspective, then the reference's screen mapping (Rasterizer.cs:383-386) onto an n x n frame.  -> (x, y, w) float64"""
    from softwarerenderer_amd import hostmath as hm
    view = hm.cube_face_view(face, (0.0, 0.0, 0.0)).astype(np.float64)
    proj = hm.create_perspective_fov(np.pi / 2, 1.0, 0.1, 100.0).astype(np.float64)
    proj[0, 0] = proj[1, 1] = 1.0                                  # (1 / tan(pi / 4) in float32 is one ulp off)
    clip = np.concatenate([np.asarray(d, dtype=np.float64), [1.0]]) @ view @ proj
    ndc = clip[:3] / clip[3]
    return (ndc[0] / 2 + 0.5) * n, (1 - (ndc[1] / 2 + 0.5)) * n, clip[3]


# ---- the program texts -----------------------------------------------------------------------------------------------------------
# Pixel i = y * PROBE_W + x of a PROBE_W x PROBE_H frame reads direction constants[4 i .. 4 i + 2] and ref (or lod, or level)
# constants[4 i + 3]; constants[60] selects what is written.  Slot 1: a colour cube, slot 2: a depth cube, slot 3: whatever the test binds
PROBE_W, PROBE_H, MODE = 5, 3, 60
PROBE_PIXELS = PROBE_W * PROBE_H


def _probe_body(env, px, py, prefix, colour, depth, other):
    return f"""    const int i = {py} * {PROBE_W} + {px};
    const float3 d = make_float3(env.constants[4 * i], env.constants[4 * i + 1], env.constants[4 * i + 2]);
    const float r = env.constants[4 * i + 3];
    const int mode = (int)env.constants[{MODE}];
    if (mode == 0) {{ const float4 c = {prefix}sample_cube(env, {colour}, d); return make_float4(c.x, c.y, c.z, 1.0f); }}
    if (mode == 1) return make_float4({prefix}sample_cube(env, {colour}, d).w, {prefix}shadow_cube(env, {depth}, d, r), {prefix}sample_cube_depth(env, {depth}, d), 1.0f);
    if (mode == 2) return make_float4({prefix}sample_cube(env, {other}, d).x + {prefix}sample_cube_lod(env, {other}, d, 1.0f).w + {prefix}sample_cube_level(env, {other}, d, 1).y,
                                      {prefix}shadow_cube(env, {other}, d, r) + {prefix}cube_texel(env, {other}, 2, 1, 1).z,
                                      (float){prefix}cube_size(env, {other}) + ({prefix}sample_cube_depth(env, {other}, d) == -3.402823466e+38f ? 0.0f : 100.0f), 1.0f);
    if (mode == 3) {{ const float4 c = {prefix}sample_cube_lod(env, {colour}, d, r); return make_float4(c.x, c.y, c.w, 1.0f); }}
    int face; float2 uv;
    {prefix}cube_face(d, &face, &uv);
    return make_float4({prefix}sample_cube_level(env, {colour}, d, (int)r).z, (float)(face + 8 * {prefix}cube_size(env, {colour})) + uv.x,
                       {prefix}cube_texel(env, {colour}, face, (int)(uv.x * 4.0f) - 1, (int)(uv.y * 4.0f) + 1).y, 1.0f);
}}
"""


FRAGMENT_PROBE = PC.HEAD + _probe_body("env", "env.x", "env.y", "swr_", 1, 2, 3)
POST_PROBE = P.HEAD + _probe_body("env", "in.x", "in.y", "swr_post_", 0, 1, 2)
NOT_A_CUBE = np.array([3.0, 2.0, 0.0], dtype=F32)          # mode 2 on an unbound slot or on one that is not n x 6 n
# the vertex half: the vertex's normal is the direction, its uv.y the ref; the fragment half is program_probe_cases.PROBE_ALL
VERTEX_PROBE = (VC.VS_HEAD + VC.CLIP_RENDERER +
                "    const float3 d = in.normal;\n"
                "    const float4 c = swr_sample_cube(env, 1, d);\n"
                "    out.data4 = make_float4(c.x, swr_shadow_cube(env, 2, d, in.uv.y), swr_sample_cube_depth(env, 2, d), c.w + (float)swr_cube_size(env, 3));\n}\n")


def probe_twin(k, colour, depth, other):
    """the probe over its PROBE_PIXELS pixels: (PROBE_H, PROBE_W, 3) float32.  colour = (levels, filtered), depth = (words, filtered),
    other = None or an atlas that is not a cube"""
    k = np.asarray(k, dtype=F32)
    d = np.ascontiguousarray(k[:4 * PROBE_PIXELS].reshape(PROBE_PIXELS, 4))
    dirs, r = d[:, :3], d[:, 3]
    mode = int(k[MODE])
    levels, cf = colour
    words, df = depth
    if mode == 0:
        out = sample_cube(levels[0], cf, dirs)[:, :3]
    elif mode == 1:
        out = np.stack([sample_cube(levels[0], cf, dirs)[:, 3], shadow_cube(words, df, dirs, r), depth_sample(words, dirs)], axis=1)
    elif mode == 2:
        assert not is_cube(other)
        out = np.broadcast_to(NOT_A_CUBE, (PROBE_PIXELS, 3))
    elif mode == 3:
        out = sample_cube_lod(levels, cf, dirs, r)[:, [0, 1, 3]]
    else:
        n = cube_size(levels[0])
        face, st = cube_face(dirs)
        with np.errstate(invalid="ignore"):
            lv = sample_cube_level(levels, cf, r.astype(np.int64), dirs)[:, 2]
        tx = (st[:, 0] * F32(4.0)).astype(F32).astype(np.int64) - 1
        ty = (st[:, 1] * F32(4.0)).astype(F32).astype(np.int64) + 1
        out = np.stack([lv, ((face + 8 * n).astype(F32) + st[:, 0]).astype(F32), cube_texel(levels[0], face.astype(np.int64), tx, ty)[:, 1]], axis=1)
    return np.ascontiguousarray(np.asarray(out, dtype=F32).reshape(PROBE_H, PROBE_W, 3))


def probe_constants(dirs, last, mode):
    k = np.zeros(64, dtype=F32)
    n = min(len(dirs), PROBE_PIXELS)
    k[:4 * n].reshape(n, 4)[:, :3] = dirs[:n]
    k[:4 * n].reshape(n, 4)[:, 3] = np.broadcast_to(np.asarray(last, dtype=F32), (len(dirs),))[:n]
    k[MODE] = mode
    return k


# The point-light recipe of INTEGRATION.md.  constants[0..2]: the light's position; [3]: far / (near - far) of the faces' common
# perspective; [4]: near * that; [5]: the bias; [6..8] the lit colour, [9..11] the shadowed one.  The world position travels in data4.
SHADOW_VERTEX = (VC.VS_HEAD +
                 "    const float4 world = swr_transform(make_float4(in.position.x, in.position.y, in.position.z, 1.0f), env.model, env);\n"
                 "    out.clip_position = swr_transform(swr_transform(world, env.view, env), env.projection, env);\n"
                 "    out.data4 = world;\n"
                 "    out.color = in.color;\n}\n")
SHADOW_FRAGMENT = PC.HEAD + """    const float3 d = make_float3(in.data4.x - env.constants[0], in.data4.y - env.constants[1], in.data4.z - env.constants[2]);
    const float ma = swr_max(swr_max(fabsf(d.x), fabsf(d.y)), fabsf(d.z));        // the view depth in the face the lookup selects
    // that face's camera maps a point at view depth ma to clip.z = (near - ma) far / (near - far) and clip.w = ma; Rasterizer.cs:388
    // gives (ndc.z + 1) / 2 per vertex and the raster stage stores it under barycentrics that add up to -1: larger is nearer
    const float ndc_z = (env.constants[4] - ma * env.constants[3]) / ma;
    const float ref = -((ndc_z + 1.0f) * 0.5f) + env.constants[5];
    const float s = swr_shadow_cube(env, 1, d, ref);
    const float* lit = env.constants + 6;
    const float* dark = env.constants + 9;
    return make_float4(dark[0] + (lit[0] - dark[0]) * s, dark[1] + (lit[1] - dark[1]) * s, dark[2] + (lit[2] - dark[2]) * s, 1.0f);
}
"""
# the skybox / reflection recipe: the world normal in data4.xyz, the world position in color, the eye in constants[0..2]
REFLECT_VERTEX = (VC.VS_HEAD +
                  "    const float4 world = swr_transform(make_float4(in.position.x, in.position.y, in.position.z, 1.0f), env.model, env);\n"
                  "    out.clip_position = swr_transform(swr_transform(world, env.view, env), env.projection, env);\n"
                  "    out.data4 = make_float4(in.normal.x, in.normal.y, in.normal.z, 0.0f);\n"
                  "    out.color = world;                    // the world position, in a varying this program does not otherwise need\n}\n")
REFLECT_FRAGMENT = PC.HEAD + """    const float3 n = make_float3(in.data4.x, in.data4.y, in.data4.z);
    const float3 v = make_float3(in.color.x - env.constants[0], in.color.y - env.constants[1], in.color.z - env.constants[2]);
    const float k = 2.0f * swr_dot3(v, n) / swr_dot3(n, n);
    return swr_sample_cube(env, 1, make_float3(v.x - k * n.x, v.y - k * n.y, v.z - k * n.z));      // reflect(v, n)
}
"""
FRAGMENT_TEXTS = {"FRAGMENT_PROBE": (None, FRAGMENT_PROBE), "VERTEX_PROBE": (VERTEX_PROBE, PC.PROBE_ALL),
                  "SHADOW": (SHADOW_VERTEX, SHADOW_FRAGMENT), "REFLECT": (REFLECT_VERTEX, REFLECT_FRAGMENT)}
POST_TEXTS = {"POST_PROBE": POST_PROBE}

NEW_EXPORTS = ("swr_texture_create_cube", "swr_texture_create_cube_depth", "swr_texture_is_cube", "swr_texture_update_face_from_frame",
               "swr_texture_update_face_from_depth", "swr_texture_update_face_from_post", "swr_texture_readback_face", "swr_cube_face_view",
               "swr_texture_cube_face", "swr_texture_sample_cube", "swr_texture_sample_cube_depth")
