"""Depth textures restated in numpy float32 (include/swr.h, csrc/swr_deliver.hip.h, csrc/swr_device.h): the
reduction of a depth plane into a texture, the three lookups, the planes and the program texts their tests run on.  Not a test module:
tests/test_depth_texture_host.py and tests/test_gpu_depth_texture.py import it.

A depth texture here is an (h, w) float32 array; `slots` is a sequence of four entries, None or (depth (h, w) float32, bilinear): what
a draw or a present captured.  Every result is one of the input's own words or an exact small float, so every comparison is made on
uint32 views: NaN payloads and the signs of zeros count."""
import functools

import numpy as np

import post_cases as P
import post_texture_cases as X
import program_probe_cases as PC
import program_texture_cases as PT
import vertex_probe_cases as VC
from render_to_texture_cases import BLOCKED_SHAPES, GPU_SHAPES, blocked_permutation, size_rule_holds, source_size, texel_centres  # noqa: F401

F32 = np.float32
MAX, MIN, FIRST = 0, 1, 2                         # SWR_DEPTH_REDUCE_*
REDUCTIONS = (MAX, MIN, FIRST)
RGBA8, DEPTH32F = 0, 1                            # SWR_TEXTURE_FORMAT_*
MINVALUE = F32(-3.40282347e+38)                   # float.MinValue: the cleared depth
SLOTS = 4
NO_SLOTS = (None, None, None, None)


def words(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def from_words(w):
    return np.asarray(w, dtype=np.uint32).view(F32)


# ---- the reduction ---------------------------------------------------------------------------------------------------------------
def pick(a, b, mode):
    """The select of one tree node; the result is a or b, bit for bit.  A comparison with a NaN is false: a NaN on the left stays,
    one on the right is never taken; +0 and -0 compare equal: the left one stays."""
    with np.errstate(invalid="ignore"):
        if mode == MAX:
            return np.where(b > a, b, a)
        if mode == MIN:
            return np.where(b < a, b, a)
    assert mode == FIRST
    return a


def tree(values, mode):
    """The balanced pairwise tree over 1, 2, 4 or 8 values, in order: pick(pick(v0, v1), pick(v2, v3)), ..."""
    if len(values) == 1:
        return values[0]
    half = len(values) // 2
    return pick(tree(values[:half], mode), tree(values[half:], mode), mode)


def reduce(plane, kx, ky, mode):
    """THE RESTATEMENT: plane (h * ky, w * kx) float32 -> (h, w) float32.  In each of the block's ky rows the tree over its kx adjacent
    words, left to right; then the same tree over the ky row results, top to bottom."""
    p = np.ascontiguousarray(plane, dtype=F32)
    assert p.ndim == 2 and p.shape[0] % ky == 0 and p.shape[1] % kx == 0
    rows = [tree([p[r::ky, c::kx] for c in range(kx)], mode) for r in range(ky)]
    return np.ascontiguousarray(tree(rows, mode), dtype=F32)


# ---- the lookups -----------------------------------------------------------------------------------------------------------------
def f2i(f):
    """(int)float as .NET 9 converts: truncating, saturating, NaN -> 0 (swr::f2i)."""
    f = np.asarray(f, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.where(np.isnan(f), 0.0, f))
    return np.clip(t, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def nearest_xy(w, h, uv):
    """The texel Texture.Sample's addressing picks (Texture.cs:43-54; swr::texture_nearest_index): u - (int)u, plus 1 where negative,
    times the size, truncated, modulo the size."""
    uv = np.asarray(uv, dtype=F32)
    out = []
    for c, n in ((uv[..., 0], w), (uv[..., 1], h)):
        with np.errstate(invalid="ignore", over="ignore"):
            f = (c - f2i(c).astype(F32)).astype(F32)
            f = np.where(f < 0, (f + F32(1.0)).astype(F32), f)
            out.append(f2i((f * F32(n)).astype(F32)) % n)
    return out[0], out[1]


def footprint(w, h, uv):
    """The 2 x 2 footprint and the fractions of the bilinear filter (swr::texture_sample_bilinear): x = u w - 0.5, its floor, the
    fraction, the wrapped indices.  Returns ix0, ix1, iy0, iy1, fx, fy."""
    uv = np.asarray(uv, dtype=F32)
    x = ((uv[..., 0] * F32(w)).astype(F32) - F32(0.5)).astype(F32)
    y = ((uv[..., 1] * F32(h)).astype(F32) - F32(0.5)).astype(F32)
    x0, y0 = np.floor(x).astype(F32), np.floor(y).astype(F32)
    fx, fy = (x - x0).astype(F32), (y - y0).astype(F32)
    ix0, iy0 = f2i(x0) % w, f2i(y0) % h
    return ix0, (ix0 + 1) % w, iy0, (iy0 + 1) % h, fx, fy


def _bound(slots, slot):
    return 0 <= slot < SLOTS and slots[slot] is not None


def depth_texel(slots, slot, x, y):
    """swr_texel_depth: the word of texel (x, y), x clamped to [0, w - 1], y to [0, h - 1]; float.MinValue without a texture."""
    if not _bound(slots, slot):
        return np.full(np.shape(x), MINVALUE, dtype=F32)
    t = slots[slot][0]
    return t[np.clip(y, 0, t.shape[0] - 1), np.clip(x, 0, t.shape[1] - 1)]


def depth_sample(slots, slot, uv):
    """swr_sample_depth: the word of the nearest lookup's texel, whatever the filter; float.MinValue without a texture."""
    if not _bound(slots, slot):
        return np.full(np.shape(uv)[:-1], MINVALUE, dtype=F32)
    t = slots[slot][0]
    x, y = nearest_xy(t.shape[1], t.shape[0], uv)
    return t[y, x]


def passes(ref, d):
    """The default test, LessEqual: new >= old (Rasterizer.cs:545); false for NaN.  1.0 or 0.0."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(ref, dtype=F32) >= d).astype(F32)


def shadow(slots, slot, uv, ref):
    """swr_shadow: one texel under the nearest filter; under the bilinear one the four results of the footprint as lerps,
    top = c00 + (c10 - c00) fx, bot = c01 + (c11 - c01) fx, r = top + (bot - top) fy, every operation rounded to float32.  1 without
    a texture."""
    if not _bound(slots, slot):
        return np.ones(np.shape(uv)[:-1], dtype=F32)
    t, bilinear = slots[slot]
    if not bilinear:
        return passes(ref, depth_sample(slots, slot, uv))
    ix0, ix1, iy0, iy1, fx, fy = footprint(t.shape[1], t.shape[0], uv)
    c00, c10, c01, c11 = passes(ref, t[iy0, ix0]), passes(ref, t[iy0, ix1]), passes(ref, t[iy1, ix0]), passes(ref, t[iy1, ix1])
    with np.errstate(invalid="ignore"):
        top = (c00 + ((c10 - c00).astype(F32) * fx).astype(F32)).astype(F32)
        bot = (c01 + ((c11 - c01).astype(F32) * fx).astype(F32)).astype(F32)
        return (top + ((bot - top).astype(F32) * fy).astype(F32)).astype(F32)


# ---- the planes ------------------------------------------------------------------------------------------------------------------
NAN_A, NAN_B, NAN_SIGNALLING = 0x7fc00001, 0xffc12345, 0x7f800001


def pool():
    """The special depth words: float.MinValue, +-0, +-Inf, three NaN payloads (one signalling: a max or min instruction would quiet
    it), subnormals, and neighbours under nextafter of values the planes and the probes' refs hold."""
    v = [0xff7fffff, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, NAN_A, NAN_B, NAN_SIGNALLING, 0x00000001, 0x80000123, 0x007fffff]
    out = list(from_words(v))
    for c in (0.125, 0.25, 0.5, 0.75, 1.0):
        out += [F32(c), np.nextafter(F32(c), F32(2.0)), np.nextafter(F32(c), F32(-1.0))]
    return np.array(out, dtype=F32)


@functools.lru_cache(maxsize=None)
def depth_pool_plane(rows, width, seed):
    """(rows, width) float32, read-only: uniform values in [0, 1]; four words in ten dealt from the pool; runs of equal words (ties
    between neighbours: the left one must win); then constant over one 8 x 8 block in four, so that the specials survive every factor
    pair."""
    rng = np.random.default_rng(9000 + seed)
    p = rng.uniform(0.0, 1.0, rows * width).astype(F32)
    values = pool()
    dealt = rng.permutation(rows * width)[: max(rows * width * 4 // 10, 1)]
    p[dealt] = values[rng.permutation(len(dealt)) % len(values)]
    p = p.reshape(rows, width)
    for _ in range(max(rows * width // 64, 1)):                       # runs of 2 .. 5 equal words
        y, x, n = rng.integers(0, rows), rng.integers(0, width), rng.integers(2, 6)
        p[y, x:x + n] = p[y, x]
    for by in range((rows + 7) // 8):
        for bx in range((width + 7) // 8):
            if rng.random() < 0.25:
                p[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = p[by * 8, bx * 8]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def finite_plane(rows, width, seed):
    """(rows, width) float32, read-only: multiples of 1 / 64 in [0, 1] (ties with the probes' refs), for values that go through the
    interpolator."""
    p = (np.random.default_rng(9500 + seed).integers(0, 65, (rows, width)).astype(F32) * F32(1.0 / 64.0)).astype(F32)
    p.setflags(write=False)
    return p


def lookup_uvs(w, h, seed=0):
    """uvs for a w x h texture, (n, 2) float32: every texel's centre; every texel's corner (a tie of the bilinear footprint, fx = fy =
    0.5 .. and the nearest lookup's edge); wraps and negatives; random ones over [-2, 3]."""
    centres = texel_centres(w, h).reshape(-1, 2)
    y, x = np.mgrid[0:h + 1, 0:w + 1]
    corners = np.stack([x / w, y / h], axis=-1).astype(F32).reshape(-1, 2)
    rng = np.random.default_rng(9700 + seed)
    far = rng.uniform(-2.0, 3.0, (256, 2)).astype(F32)
    edge = np.array([(0.0, 0.0), (-0.0, 1.0), (1.0, 1.0), (-1.0, -1.0), (-0.25, 1.75), (2.5, -1.5), (0.999999, 1e-7), (-1e-7, 0.5)], dtype=F32)
    return np.ascontiguousarray(np.concatenate([centres, corners, (centres - F32(1.0)).astype(F32), (corners + F32(1.0)).astype(F32), far, edge]))


def lookup_refs(n, seed=0):
    """n refs dealt from the pool and from multiples of 1 / 8: equal to stored words often enough."""
    rng = np.random.default_rng(9800 + seed)
    values = np.concatenate([pool(), (np.arange(9) * 0.125).astype(F32)])
    return values[rng.integers(0, len(values), n)]


# ---- the program texts: four in all ----------------------------------------------------------------------------------------------------
# constants of the two pixel probes: [0..3] the uv scale and shift (pixel_uv), [4], [5] the texel walk's periods (fragment) or shift
# (post), [61] the slot or PER_PIXEL.  ref = (x & 7) / 8: an exact product, 0 .. 0.875
SLOT, PER_PIXEL = PT.SLOT, PT.PER_PIXEL

# 1. the fragment probe: (swr_shadow, swr_sample_depth, swr_texel_depth, 1) raw into the frame
FRAGMENT_PROBE = PC.HEAD + PT.UV + f"""    const int slot = env.constants[{SLOT}] == {PER_PIXEL!r}f ? (env.x + env.y) % 5 : (int)env.constants[{SLOT}];
    const float2 uv = make_float2(u, v);
    const float ref = (float)(env.x & 7) * 0.125f;
    return make_float4(swr_shadow(env, slot, uv, ref), swr_sample_depth(env, slot, uv),
                       swr_texel_depth(env, slot, env.x % (int)env.constants[4] - 2, env.y % (int)env.constants[5] - 2), 1.0f);
}}
"""

# 2. the vertex-plus-fragment probe: the same three at the vertex's uv into data4, slot 1 (shadow, sample) and slot 0 (texel);
#    the fragment half is program_probe_cases.PROBE_ALL, which returns data4 as it arrives
VERTEX_PROBE = (VC.VS_HEAD + VC.CLIP_RENDERER +
                "    out.data4 = make_float4(swr_shadow(env, 1, in.uv, in.uv.y), swr_sample_depth(env, 1, in.uv),\n"
                "                            swr_texel_depth(env, 0, (int)(in.uv.x * 16.0f) - 2, (int)(in.uv.y * 24.0f) - 2), 1.0f);\n}\n")
VERTEX_GROUPS = [g for g in PC.FS_IN_GROUPS if any(n.split(".")[0] == "data4" for n in PC.group_names(g))]

# 3. the post probe; constants[6] != 0: the frame's own depth word instead, as swr_post_depth reads it
POST_PROBE = P.HEAD + X.UV + f"""    if (env.constants[6] != 0.0f) return make_float4(swr_post_depth(env, in.x, in.y), 0.0f, 0.0f, 1.0f);
    const int slot = env.constants[{SLOT}] == {PER_PIXEL!r}f ? (in.x + in.y) % 5 : (int)env.constants[{SLOT}];
    const float2 uv = make_float2(u, v);
    const float ref = (float)(in.x & 7) * 0.125f;
    return make_float4(swr_post_shadow(env, slot, uv, ref), swr_post_sample_depth(env, slot, uv),
                       swr_post_texel_depth(env, slot, in.x + (int)env.constants[4], in.y + (int)env.constants[5]), 1.0f);
}}
"""

# 4. the shadow recipe of the porting guide.  constants[0..15]: the light's view * projection, row-major;
#    constants[16]: the bias; constants[17..19] the lit colour, [20..22] the shadowed one
SHADOW_VERTEX = (VC.VS_HEAD +
                 "    const float4 world = swr_transform(make_float4(in.position.x, in.position.y, in.position.z, 1.0f), env.model, env);\n"
                 "    out.clip_position = swr_transform(swr_transform(world, env.view, env), env.projection, env);\n"
                 "    out.data4 = swr_transform(world, env.constants, env);          // the light's clip position\n"
                 "    out.color = in.color;\n}\n")
SHADOW_FRAGMENT = PC.HEAD + """    const float3 ndc = make_float3(in.data4.x / in.data4.w, in.data4.y / in.data4.w, in.data4.z / in.data4.w);
    const float2 uv = make_float2(ndc.x * 0.5f + 0.5f, 1.0f - (ndc.y * 0.5f + 0.5f));      // Rasterizer.cs:383-386: texel and pixel coincide
    // :388 gives (z + 1) / 2 per vertex, and the raster stage stores its sum under barycentrics that add up to -1 (:498-502): the
    // stored depth of this point, as the light saw it, is -((z + 1) / 2) -- larger is nearer -- and the bias lifts it off its own texel
    const float ref = -((ndc.z + 1.0f) * 0.5f) + env.constants[16];
    const float s = swr_shadow(env, 1, uv, ref);
    const float* lit = env.constants + 17;
    const float* dark = env.constants + 20;
    return make_float4(dark[0] + (lit[0] - dark[0]) * s, dark[1] + (lit[1] - dark[1]) * s, dark[2] + (lit[2] - dark[2]) * s, 1.0f);
}
"""

TEXTS = {"FRAGMENT_PROBE": (None, FRAGMENT_PROBE), "VERTEX_PROBE": (VERTEX_PROBE, PC.PROBE_ALL), "SHADOW": (SHADOW_VERTEX, SHADOW_FRAGMENT)}


# ---- the twins -------------------------------------------------------------------------------------------------------------------
def _per_slot(k, n, fn):
    """fn(slot, mask) -> (count, 3) words, for the one slot of constants[61] or, under PER_PIXEL, for slot (x + y) % 5 of each pixel."""
    if k[SLOT] != F32(PER_PIXEL):
        return fn(int(k[SLOT]), slice(None))
    out = np.zeros((len(n), 3), dtype=F32)
    for s in range(5):
        m = n % 5 == s
        if m.any():
            out[m] = fn(s, m)
    return out


def fragment_probe_twin(k, slots, xs, ys):
    """FRAGMENT_PROBE at the pixels (xs, ys): (n, 3) float32."""
    uv = PT.pixel_uv(k, xs, ys)
    ref = ((xs & 7).astype(F32) * F32(0.125)).astype(F32)
    tx, ty = xs % int(k[4]) - 2, ys % int(k[5]) - 2
    return _per_slot(k, xs + ys, lambda s, m: np.stack([shadow(slots, s, uv[m], ref[m]), depth_sample(slots, s, uv[m]),
                                                        depth_texel(slots, s, tx[m], ty[m])], axis=-1))


def post_probe_twin(rows, w, k, slots):
    """POST_PROBE over a rows x w result: (rows, w, 3) float32."""
    ys, xs = (a.reshape(-1) for a in np.mgrid[0:rows, 0:w])
    uv = X.pixel_uv(rows, w, k).reshape(-1, 2)
    ref = ((xs & 7).astype(F32) * F32(0.125)).astype(F32)
    tx, ty = xs + int(k[4]), ys + int(k[5])
    out = _per_slot(k, xs + ys, lambda s, m: np.stack([shadow(slots, s, uv[m], ref[m]), depth_sample(slots, s, uv[m]),
                                                       depth_texel(slots, s, tx[m], ty[m])], axis=-1))
    return np.ascontiguousarray(out.reshape(rows, w, 3))


def vertex_probe_stage(d, flags, slots):
    """VERTEX_PROBE restated per vertex: the outputs program_probe_cases.probe_tris(scene, vertex_stage=...) takes."""
    V, n = d.vertices, d.vertices.shape[0]
    o = VC._empty(n)
    for i in range(n):
        o["clip"][i] = VC.renderer_clip(d, i, flags)
    uv = V["uv"].astype(F32)
    tx = np.trunc((uv[:, 0] * F32(16.0)).astype(F32)).astype(np.int64) - 2
    ty = np.trunc((uv[:, 1] * F32(24.0)).astype(F32)).astype(np.int64) - 2
    o["data4"][:, 0] = shadow(slots, 1, uv, uv[:, 1])
    o["data4"][:, 1] = depth_sample(slots, 1, uv)
    o["data4"][:, 2] = depth_texel(slots, 0, tx, ty)
    o["data4"][:, 3] = 1.0
    return o
