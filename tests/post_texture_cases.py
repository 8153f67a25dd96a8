"""Post programs with texture slots, and a pass's result into a texture, restated in numpy float32 (include/swr.h,
csrc/swr_post.hip.h): the test programs as the texts handed to swr_post_create, their twins, the wrong twins the
GPU tests' inputs must tell apart, and the textures.  Not a test module: tests/test_post_texture_host.py and
tests/test_gpu_post_texture.py import it.  Built on post_cases (planes, shapes, delivery), render_to_texture_cases and present8_cases.

A twin maps (resolved (rows, w, 4), constants[64], slots) to the program's (rows, w, 4) float32 result, w included: a present delivers
x, y, z (post_cases.deliver), swr_texture_update_from_post the bytes of `texels`.  `slots` is a sequence of four entries, None or
(texels (h, w, 4) uint8, bilinear): what the present captured when it was called.  Sampler expectations are the oracle's
(oswr_texture_sample, oswr_texture_sample_bilinear), fed uv computed here with the program's own single IEEE operations; the numpy
sampler below exists for the wrong twins, and a host test holds it to the oracle."""
import functools

import numpy as np

import post_cases as P
import present8_cases as K
import render_to_texture_cases as T

F32 = np.float32
HEAD = P.HEAD
SLOTS = 4
ONES = np.ones(4, dtype=F32)
INV255 = F32(1.0) / F32(255.0)
NO_SLOTS = (None, None, None, None)

# uv of the pixel's centre scaled and shifted by constants[0..3]: each a product rounded to float32, then a sum
UV = """    const float u = ((float)in.x + 0.5f) * env.constants[0] + env.constants[2];
    const float v = ((float)in.y + 0.5f) * env.constants[1] + env.constants[3];
"""

# slot 0 at that uv; constants[4] != 0 delivers the channels reversed, so that alpha reaches a three-channel present
SAMPLE = HEAD + UV + """    const float4 s = swr_post_sample(env, 0, make_float2(u, v));
    if (env.constants[4] != 0.0f) return make_float4(s.w, s.z, s.y, s.x);
    return s;
}
"""

# the four slots at once, weights 1/2, 1/4, 1/8, 1/16 (exact products), summed left to right
FOUR = """__device__ float mix4(float a, float b, float c, float d) { return ((a * 0.5f + b * 0.25f) + c * 0.125f) + d * 0.0625f; }
""" + HEAD + UV + """    const float2 uv = make_float2(u, v);
    const float4 a = swr_post_sample(env, 0, uv), b = swr_post_sample(env, 1, uv), c = swr_post_sample(env, 2, uv), d = swr_post_sample(env, 3, uv);
    return make_float4(mix4(a.x, b.x, c.x, d.x), mix4(a.y, b.y, c.y, d.y), mix4(a.z, b.z, c.z, d.z), mix4(a.w, b.w, c.w, d.w));
}
"""

# a slot that varies by lane, slot 4 (no texture: ones) among them
DYNAMIC = HEAD + UV + """    return swr_post_sample(env, (in.x + in.y) % 5, make_float2(u, v));
}
"""

# the texel at the pixel shifted by (constants[0], constants[1]), clamped by the helper
TEXEL = HEAD + """    return swr_post_texel(env, 0, in.x + (int)env.constants[0], in.y + (int)env.constants[1]);
}
"""

# sizes of slots 0, 1 and 3; slots 4 and -1 measure (0, 0); w = the bound slots as bits, slots 4 and -1 asked as well
SIZES = HEAD + """    const int2 a = swr_post_texture_size(env, 0), b = swr_post_texture_size(env, 1), c = swr_post_texture_size(env, 3);
    const int2 d = swr_post_texture_size(env, 4), e = swr_post_texture_size(env, -1);
    int bits = 0;
#pragma unroll
    for (int k = -1; k < 5; ++k) bits |= swr_post_has_texture(env, k) ? 1 << (k + 1) : 0;
    return make_float4((float)(a.x * 256 + a.y), (float)(b.x * 256 + b.y), (float)(c.x * 256 + c.y) + (float)(d.x + d.y + e.x + e.y) * 0.5f,
                       (float)bits * 0.015625f);
}
"""

# (l + 2 c + r) / 4 over the frame's row; the product by 2 and by 1/4 are exact, the two sums are rounded; all four channels
BLUR_H = HEAD + """    const float4 l = swr_post_fetch(env, in.x - 1, in.y), c = in.color, r = swr_post_fetch(env, in.x + 1, in.y);
    return make_float4(((l.x + c.x * 2.0f) + r.x) * 0.25f, ((l.y + c.y * 2.0f) + r.y) * 0.25f, ((l.z + c.z * 2.0f) + r.z) * 0.25f,
                       ((l.w + c.w * 2.0f) + r.w) * 0.25f);
}
"""

# the same weights down slot 0's column, texel for texel (the frame is not read)
BLUR_V = HEAD + """    const float4 l = swr_post_texel(env, 0, in.x, in.y - 1), c = swr_post_texel(env, 0, in.x, in.y), r = swr_post_texel(env, 0, in.x, in.y + 1);
    return make_float4(((l.x + c.x * 2.0f) + r.x) * 0.25f, ((l.y + c.y * 2.0f) + r.y) * 0.25f, ((l.z + c.z * 2.0f) + r.z) * 0.25f,
                       ((l.w + c.w * 2.0f) + r.w) * 0.25f);
}
"""

# half the frame plus half of last frame's image in slot 0 (exact products, one rounded sum)
ACCUM = HEAD + """    const float4 t = swr_post_texel(env, 0, in.x, in.y);
    return make_float4(in.color.x * 0.5f + t.x * 0.5f, in.color.y * 0.5f + t.y * 0.5f, in.color.z * 0.5f + t.z * 0.5f, in.color.w * 0.5f + t.w * 0.5f);
}
"""

# the frame's colour under slot 0's image where that is opaque: a crosshair or a health bar
OVERLAY = HEAD + UV + """    const float4 o = swr_post_sample(env, 0, make_float2(u, v));
    return make_float4(swr_lerp(in.color.x, o.x, o.w), swr_lerp(in.color.y, o.y, o.w), swr_lerp(in.color.z, o.z, o.w), 1.0f);
}
"""

TEXTS = {"SAMPLE": SAMPLE, "FOUR": FOUR, "DYNAMIC": DYNAMIC, "TEXEL": TEXEL, "SIZES": SIZES, "BLUR_H": BLUR_H, "BLUR_V": BLUR_V,
         "ACCUM": ACCUM, "OVERLAY": OVERLAY}

# the fragment contract does not gain the helper
FRAGMENT_WITH_POST_SAMPLE = """__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {
    return swr_post_sample(env, 0, in.tex_coord);
}
"""


# ---- the textures ---------------------------------------------------------------------------------------------------------------
TEXTURE_SIZES = [(8, 8), (5, 3), (1, 1)]          # (w, h): a block-linear copy under the filter; none (not multiples of 4); one texel


@functools.lru_cache(maxsize=None)
def texture(size, seed=0):
    """(h, w, 4) uint8, read-only: every byte random, alpha too, so that no two texels and no two textures agree by accident."""
    w, h = size
    t = np.random.default_rng(7000 + 100 * w + h + seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    t.setflags(write=False)
    return t


def uv_constants(out_size, lo=-2.0, hi=3.0, reverse=False):
    """constants[0..4] that spread the pixels' centres over about [lo, hi] in u and v."""
    w, rows = out_size
    span = F32(hi) - F32(lo)
    return P.constants64([span / F32(w), span / F32(rows), lo, lo, 1.0 if reverse else 0.0])


def pixel_uv(rows, w, k):
    """The program's own operations: ((float)x + 0.5f) * k[0] + k[2] -- a rounded product, then a rounded sum."""
    y, x = np.mgrid[0:rows, 0:w]
    u = ((x.astype(F32) + F32(0.5)) * k[0]).astype(F32) + k[2]
    v = ((y.astype(F32) + F32(0.5)) * k[1]).astype(F32) + k[3]
    return np.stack([u.astype(F32), v.astype(F32)], axis=-1)


# ---- the samplers ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import binding
    return binding.load()


def oracle_sample(texels, bilinear, uv):
    """The oracle's sampler, one call per uv: (..., 2) float32 -> (..., 4) float32."""
    lib = _oracle()
    fn = lib.oswr_texture_sample_bilinear if bilinear else lib.oswr_texture_sample
    t = np.ascontiguousarray(texels, dtype=np.uint8)
    h, w = t.shape[:2]
    flat = np.ascontiguousarray(uv, dtype=F32).reshape(-1, 2)
    out = np.zeros((flat.shape[0], 4), dtype=F32)
    for i in range(flat.shape[0]):
        fn(t.ctypes.data, w, h, flat[i].ctypes.data, out[i].ctypes.data)
    return out.reshape(np.shape(uv)[:-1] + (4,))


def numpy_nearest(texels, uv, clamp=False, divide=False):
    """Texture.Sample (Texture.cs:43-63) in numpy float32: u - trunc(u), plus 1 where negative, times the size, truncated, modulo the
    size; each byte times the float 1 / 255.  clamp / divide: THE WRONG TWINS' samplers -- uv clamped to the edge instead of wrapped;
    the byte divided by 255."""
    t = np.asarray(texels, dtype=np.uint8)
    h, w = t.shape[:2]
    uv = np.asarray(uv, dtype=F32)
    idx = []
    for c, n in ((uv[..., 0], w), (uv[..., 1], h)):
        if clamp:
            i = np.clip(np.floor((c * F32(n)).astype(F32)), 0, n - 1).astype(np.int64)
        else:
            f = (c - np.trunc(c)).astype(F32)
            f = np.where(f < 0, (f + F32(1.0)).astype(F32), f)
            i = np.trunc((f * F32(n)).astype(F32)).astype(np.int64) % n
        idx.append(i)
    b = t[idx[1], idx[0]].astype(F32)
    return (b / F32(255.0)).astype(F32) if divide else (b * INV255).astype(F32)


def sample(slots, slot, uv, sampler=None):
    """swr_post_sample: an unbound slot and a slot outside 0 .. 3 read ones."""
    if not 0 <= slot < SLOTS or slots[slot] is None:
        return np.broadcast_to(ONES, np.shape(uv)[:-1] + (4,)).copy()
    texels, bilinear = slots[slot]
    if sampler is not None and not bilinear:
        return sampler(texels, uv)
    return oracle_sample(texels, bilinear, uv)


def texel(slots, slot, x, y, divide=False):
    """swr_post_texel: x clamped to [0, w - 1], y to [0, h - 1]; byte times the float 1 / 255; ones without a texture."""
    if not 0 <= slot < SLOTS or slots[slot] is None:
        return np.broadcast_to(ONES, np.shape(x) + (4,)).copy()
    t = np.asarray(slots[slot][0], dtype=np.uint8)
    b = t[np.clip(y, 0, t.shape[0] - 1), np.clip(x, 0, t.shape[1] - 1)].astype(F32)
    return (b / F32(255.0)).astype(F32) if divide else (b * INV255).astype(F32)


def size(slots, slot):
    if not 0 <= slot < SLOTS or slots[slot] is None:
        return 0, 0
    return slots[slot][0].shape[1], slots[slot][0].shape[0]


# ---- the twins ------------------------------------------------------------------------------------------------------------------
def sample_twin(res, k, slots, sampler=None):
    s = sample(slots, 0, pixel_uv(res.shape[0], res.shape[1], k), sampler)
    return s[..., ::-1].copy() if k[4] != 0 else s


def _mix4(a, b, c, d):
    x = ((a * F32(0.5)).astype(F32) + (b * F32(0.25)).astype(F32)).astype(F32)
    x = (x + (c * F32(0.125)).astype(F32)).astype(F32)
    return (x + (d * F32(0.0625)).astype(F32)).astype(F32)


def four_twin(res, k, slots, order=(0, 1, 2, 3)):
    uv = pixel_uv(res.shape[0], res.shape[1], k)
    return _mix4(*[sample(slots, s, uv) for s in order])


def four_slots_swapped(res, k, slots):
    """WRONG TWIN: slots 0 and 1 exchanged."""
    return four_twin(res, k, slots, order=(1, 0, 2, 3))


def dynamic_twin(res, k, slots):
    rows, w = res.shape[:2]
    uv = pixel_uv(rows, w, k)
    y, x = np.mgrid[0:rows, 0:w]
    out = np.zeros((rows, w, 4), dtype=F32)
    for s in range(5):
        m = (x + y) % 5 == s
        if m.any():
            out[m] = sample(slots, s, uv[m])
    return out


def texel_twin(res, k, slots, divide=False):
    y, x = np.mgrid[0:res.shape[0], 0:res.shape[1]]
    return texel(slots, 0, x + int(k[0]), y + int(k[1]), divide)


def sizes_twin(res, k, slots):
    (aw, ah), (bw, bh), (cw, ch) = size(slots, 0), size(slots, 1), size(slots, 3)
    bits = sum(1 << (s + 1) for s in range(SLOTS) if slots[s] is not None)
    px = np.array([aw * 256 + ah, bw * 256 + bh, cw * 256 + ch, bits * 0.015625], dtype=F32)
    return np.broadcast_to(px, res.shape[:2] + (4,)).copy()


def _blur3(l, c, r):
    with np.errstate(all="ignore"):
        s = (l + (c * F32(2.0)).astype(F32)).astype(F32)
        return ((s + r).astype(F32) * F32(0.25)).astype(F32)


def blur_h_twin(res, k, slots):
    return _blur3(P._tap(res, -1, 0), res, P._tap(res, 1, 0))


def blur_v_twin(res, k, slots):
    y, x = np.mgrid[0:res.shape[0], 0:res.shape[1]]
    return _blur3(texel(slots, 0, x, y - 1), texel(slots, 0, x, y), texel(slots, 0, x, y + 1))


def accum_twin(res, k, slots):
    y, x = np.mgrid[0:res.shape[0], 0:res.shape[1]]
    with np.errstate(all="ignore"):
        return ((res * F32(0.5)).astype(F32) + (texel(slots, 0, x, y) * F32(0.5)).astype(F32)).astype(F32)


def identity_twin(res, k, slots):
    return res.copy()


TWINS = {"SAMPLE": sample_twin, "FOUR": four_twin, "DYNAMIC": dynamic_twin, "TEXEL": texel_twin, "SIZES": sizes_twin,
         "BLUR_H": blur_h_twin, "BLUR_V": blur_v_twin, "ACCUM": accum_twin, "IDENTITY": identity_twin}


def result(name, color, kx, ky, constants=(), slots=NO_SLOTS, twin=None):
    """The program's (rows, w, 4) result on the frame `color` resolved by (kx, ky)."""
    return np.ascontiguousarray((twin or TWINS[name])(P.resolve_rgba(color, kx, ky), P.constants64(constants), slots), dtype=F32)


def expected(name, color, kx, ky, fmt=P.RGB32F, constants=(), slots=NO_SLOTS, twin=None):
    """What a present of the program delivers."""
    return P.deliver(result(name, color, kx, ky, constants, slots, twin)[..., :3], fmt)


def texels(result4, keep_alpha=False):
    """swr_texture_update_from_post: R, G, B quantise8 of x, y, z; A 255, or quantise8(w) with keep_alpha."""
    q = K.quantise(result4)
    if not keep_alpha:
        q[..., 3] = 255
    return np.ascontiguousarray(q)


def texels_alpha_from_frame(result4, color, kx, ky):
    """WRONG TWIN of the KEEP mode: alpha is the frame's (swr_texture_update_from_frame's), not the result's w."""
    q = texels(result4)
    q[..., 3] = T.alpha_bytes(color, kx, ky)
    return q


def blur_chain(color, kx, ky):
    """Two passes with an 8-bit intermediate: BLUR_H of the frame into texture A (alpha kept), BLUR_V of A into T (opaque)."""
    a = texels(result("BLUR_H", color, kx, ky), keep_alpha=True)
    rows, w = a.shape[:2]
    t = texels(blur_v_twin(np.zeros((rows, w, 4), dtype=F32), P.constants64(), ((a, False), None, None, None)))
    return a, t


def accumulate(frames):
    """Ping-pong over frames of one size: texture n % 2 = ACCUM(frame n, texture (n + 1) % 2), both zeros at first, alpha kept.
    Returns the two textures after the last frame."""
    rows, w = frames[0].shape[:2]
    tex = [np.zeros((rows, w, 4), dtype=np.uint8), np.zeros((rows, w, 4), dtype=np.uint8)]
    for n, f in enumerate(frames):
        tex[n % 2] = texels(result("ACCUM", f, 1, 1, slots=((tex[(n + 1) % 2], False), None, None, None)), keep_alpha=True)
    return tex
