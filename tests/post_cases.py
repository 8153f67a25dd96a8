"""Post-process programs restated in numpy float32 (include/swr.h, csrc/swr_post.hip.h): each test program as the
text handed to swr_post_create together with its twin, the wrong twins the test planes must tell apart, and the planes and shapes.
Not a test module: tests/test_post_host.py and tests/test_gpu_post.py import it.

A program sees the RESOLVED frame: R, G, B of resolve_cases.resolve and the frame's alpha through the same tree and scale; depth is
the word of the top-left sample of the pixel's kx x ky block.  A twin maps (resolved (rows, w, 4), depth (rows * ky, w * kx), kx, ky,
constants[64]) to the program's (rows, w, 3) float32 result; the 8-bit formats put present8_cases.quantise behind it.  numpy's float32
`+`, `-`, `*`, `/` are IEEE single operations (nothing fuses), which is all the twins use."""
import functools

import numpy as np

import present8_cases as K
import render_to_texture_cases as T
import resolve_cases as R

RGB32F, RGB8, RGBX8 = 0, 3, 4                     # SWR_POST_*
FORMATS = (RGB32F, RGB8, RGBX8)
# output (width, rows): at, below and above the 64 x 4 block of threads, and two blocks and a tail in x and y
OUT_SIZES = [(1, 1), (63, 3), (64, 4), (65, 5), (130, 9)]
FACTORS = [(1, 1), (2, 1), (1, 2), (4, 2), (8, 8)]
F32 = np.float32

HEAD = "__device__ float4 swr_post(const swr_post_in& in, const swr_post_env& env) {\n"

IDENTITY = HEAD + "    return in.color;\n}\n"

# c * k + b per channel: k = constants[0..2], b = constants[3..5]; the product is rounded, then the sum
TINT = HEAD + """    const float r = in.color.x * env.constants[0];
    const float g = in.color.y * env.constants[1];
    const float b = in.color.z * env.constants[2];
    return make_float4(r + env.constants[3], g + env.constants[4], b + env.constants[5], 1.0f);
}
"""

# the same curve through the shared swr_lerp: lerp(b, k, c) = b * (1 - c) + k * c, fused or not with the library's numerics model
TINT_LERP = HEAD + """    return make_float4(swr_lerp(env.constants[3], env.constants[0], in.color.x), swr_lerp(env.constants[4], env.constants[1], in.color.y),
                       swr_lerp(env.constants[5], env.constants[2], in.color.z), 1.0f);
}
"""

COORDS = HEAD + """    const float r = (float)in.x / (float)env.width;
    const float g = (float)in.y / (float)env.height;
    const float b = (float)(env.kx * 16 + env.ky) * 0.0078125f + (float)(in.y * env.width + in.x);
    return make_float4(r, g, b, 0.0f);
}
"""

# nine taps, one running sum in row-major order starting from the first tap, times the float 1 / 9
BOX3 = HEAD + """    float4 s = swr_post_fetch(env, in.x - 1, in.y - 1);
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        const float4 t = swr_post_fetch(env, in.x + k % 3 - 1, in.y + k / 3 - 1);
        s = make_float4(s.x + t.x, s.y + t.y, s.z + t.z, s.w + t.w);
    }
    const float ninth = 1.0f / 9.0f;
    return make_float4(s.x * ninth, s.y * ninth, s.z * ninth, s.w * ninth);
}
"""

EDGE = HEAD + """    const float d = swr_post_depth(env, in.x, in.y);
    return make_float4(d - swr_post_depth(env, in.x + 1, in.y), d - swr_post_depth(env, in.x, in.y + 1), d, 1.0f);
}
"""

# NaN, +Inf, -Inf, -0, a subnormal, two exact ties of c * 255 (0.5 -> 0 and 126.5 -> 126), one below 1: dealt by pixel index, a
# different one per channel; every ninth pixel keeps its colour
SPECIAL_WORDS = [0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x00001234, 0x3b008081, 0x3efdfdfe, 0x3f7fffff]
SPECIALS = HEAD + """    const unsigned int words[8] = { 0x7fc00000u, 0x7f800000u, 0xff800000u, 0x80000000u, 0x00001234u, 0x3b008081u, 0x3efdfdfeu, 0x3f7fffffu };
    const int i = in.y * env.width + in.x;
    if (i % 9 == 8) return in.color;
    unsigned int r = 0u, g = 0u, b = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (i % 9 == k) r = words[k];
        if ((i + 3) % 8 == k) g = words[k];
        if ((i + 5) % 8 == k) b = words[k];
    }
    return make_float4(__uint_as_float(r), __uint_as_float(g), __uint_as_float(b), 0.0f);
}
"""

TEXTS = {"IDENTITY": IDENTITY, "TINT": TINT, "COORDS": COORDS, "BOX3": BOX3, "EDGE": EDGE, "SPECIALS": SPECIALS}

SYNTAX_ERROR = TINT.replace("    const float b = in.color.z * env.constants[2];", "    const float b = in.color.z * ;")
SYNTAX_ERROR_LINE = SYNTAX_ERROR.splitlines().index("    const float b = in.color.z * ;") + 1       # line 4 of the text
NO_ENTRY = "__device__ float4 shade(const swr_post_in& in) { return in.color; }\n"

TINT_CONSTANTS = np.array([1.1, 0.9, 0.7, 0.05, -0.02, 0.1], dtype=F32)


def constants64(values=()):
    k = np.zeros(64, dtype=F32)
    v = np.asarray(values, dtype=F32).reshape(-1)
    k[:v.size] = v
    return k


def resolve_rgba(color, kx, ky):
    """What a program sees: (rows, W, 4) -> (rows / ky, W / kx, 4); alpha rides through the three-channel restatement in R's place."""
    color = np.asarray(color, dtype=F32)
    rgb = R.resolve(color, kx, ky)
    a = R.resolve(np.repeat(color[..., 3:4], 3, axis=2), kx, ky)[..., :1]
    return np.ascontiguousarray(np.concatenate([rgb, a], axis=2))


# ---- the twins ------------------------------------------------------------------------------------------------------------------
def identity(res, depth, kx, ky, k):
    return res[..., :3].copy()


def tint(res, depth, kx, ky, k):
    with np.errstate(all="ignore"):
        prod = (res[..., :3] * k[0:3]).astype(F32)
        return (prod + k[3:6]).astype(F32)


def tint_fused(res, depth, kx, ky, k):
    """WRONG TWIN: fma(c, k, b), the product not rounded to float32 (evaluated in float64, where a float32 product is exact; the sum's
    own rounding there is far below a float32 ulp -- a wrong twin only has to differ from the right one, which a test asserts)."""
    with np.errstate(all="ignore"):
        return (res[..., :3].astype(np.float64) * k[0:3].astype(np.float64) + k[3:6].astype(np.float64)).astype(F32)


def tint_lerp(res, depth, kx, ky, k):
    """TINT_LERP under an unfused library: x = b * (1 - c); y = k * c; x + y."""
    c = res[..., :3]
    with np.errstate(all="ignore"):
        x = (k[3:6] * (F32(1.0) - c).astype(F32)).astype(F32)
        y = (k[0:3] * c).astype(F32)
        return (x + y).astype(F32)


def tint_lerp_fused(res, depth, kx, ky, k):
    """TINT_LERP under a SWR_NUMERICS_FMA library: fma(b, 1 - c, k * c), exactly (rationals), NaN and Inf by IEEE in float64."""
    from fractions import Fraction
    c = res[..., :3]
    with np.errstate(all="ignore"):
        one_minus = (F32(1.0) - c).astype(F32)
        y = (k[0:3] * c).astype(F32)
        b = np.broadcast_to(k[3:6], c.shape)
        approx = (b.astype(np.float64) * one_minus.astype(np.float64) + y.astype(np.float64))
    out = approx.astype(F32)
    fin = np.isfinite(one_minus) & np.isfinite(y)
    for idx in np.argwhere(fin):
        i = tuple(idx)
        exact = Fraction(float(b[i])) * Fraction(float(one_minus[i])) + Fraction(float(y[i]))
        out[i] = round_fraction_to_f32(exact, out[i])
    return out


def round_fraction_to_f32(q, guess):
    """The float32 nearest to the rational q (ties to even), found among `guess` and its neighbours."""
    from fractions import Fraction
    if q == 0 or not np.isfinite(guess):
        return guess                                       # (an exact zero's sign and an overflow are float64's: the same rules)
    cand = [np.nextafter(F32(guess), F32(-np.inf)), F32(guess), np.nextafter(F32(guess), F32(np.inf))]
    cand = [c for c in cand if np.isfinite(c)]
    best = min(cand, key=lambda c: (abs(Fraction(float(c)) - q), int(np.array([c], dtype=F32).view(np.uint32)[0]) & 1))
    return F32(best)


def coords(res, depth, kx, ky, k):
    rows, w = res.shape[:2]
    y, x = np.mgrid[0:rows, 0:w]
    r = x.astype(F32) / F32(w)
    g = y.astype(F32) / F32(rows)
    b = (F32(kx * 16 + ky) * F32(0.0078125)).astype(F32) + (y * w + x).astype(F32)
    return np.stack([r, g, b.astype(F32)], axis=-1).astype(F32)


def _tap(res, dx, dy, wrap=False):
    rows, w = res.shape[:2]
    y, x = np.arange(rows) + dy, np.arange(w) + dx
    if wrap:
        y, x = y % rows, x % w
    else:
        y, x = np.clip(y, 0, rows - 1), np.clip(x, 0, w - 1)
    return res[y][:, x]


def box3(res, depth, kx, ky, k, wrap=False, column_first=False):
    order = [(j // 3 - 1, j % 3 - 1) for j in range(9)] if column_first else [(j % 3 - 1, j // 3 - 1) for j in range(9)]
    with np.errstate(all="ignore"):
        s = _tap(res, *order[0], wrap=wrap)
        for dx, dy in order[1:]:
            s = (s + _tap(res, dx, dy, wrap=wrap)).astype(F32)
        return (s * (F32(1.0) / F32(9.0))).astype(F32)[..., :3]


def box3_wrap(res, depth, kx, ky, k):
    """WRONG TWIN: taps wrap around the frame instead of clamping to it."""
    return box3(res, depth, kx, ky, k, wrap=True)


def box3_column_first(res, depth, kx, ky, k):
    """WRONG TWIN: the running sum goes down the columns."""
    return box3(res, depth, kx, ky, k, column_first=True)


def _depth_tap(depth, kx, ky, dx, dy, last=False):
    rows, w = depth.shape[0] // ky, depth.shape[1] // kx
    y, x = np.clip(np.arange(rows) + dy, 0, rows - 1), np.clip(np.arange(w) + dx, 0, w - 1)
    oy, ox = (ky - 1, kx - 1) if last else (0, 0)
    return depth[y * ky + oy][:, x * kx + ox]


def edge(res, depth, kx, ky, k, last=False):
    with np.errstate(all="ignore"):
        d = _depth_tap(depth, kx, ky, 0, 0, last)
        return np.stack([d - _depth_tap(depth, kx, ky, 1, 0, last), d - _depth_tap(depth, kx, ky, 0, 1, last), d], axis=-1).astype(F32)


def edge_last_sample(res, depth, kx, ky, k):
    """WRONG TWIN: the block's bottom-right sample instead of its top-left one."""
    return edge(res, depth, kx, ky, k, last=True)


def specials(res, depth, kx, ky, k):
    rows, w = res.shape[:2]
    words = np.array(SPECIAL_WORDS, dtype=np.uint32).view(F32)
    i = (np.arange(rows)[:, None] * w + np.arange(w)[None, :])
    out = np.stack([words[i % 9 % 8], words[(i + 3) % 8], words[(i + 5) % 8]], axis=-1).astype(F32)
    keep = i % 9 == 8
    out[keep] = res[..., :3][keep]
    return out


TWINS = {"IDENTITY": identity, "TINT": tint, "COORDS": coords, "BOX3": box3, "EDGE": edge, "SPECIALS": specials}
WRONG_TWINS = {"BOX3 wraps": ("BOX3", box3_wrap), "BOX3 column first": ("BOX3", box3_column_first), "TINT fused": ("TINT", tint_fused),
               "EDGE last sample": ("EDGE", edge_last_sample)}
CONSTANTS = {"TINT": TINT_CONSTANTS}


def deliver(rgb, fmt):
    """A twin's floats in the present's format: as they are, or quantised (and a fourth byte of 255)."""
    if fmt == RGB32F:
        return np.ascontiguousarray(rgb, dtype=F32)
    q = K.quantise(rgb)
    if fmt == RGBX8:
        q = np.concatenate([q, np.full(q.shape[:2] + (1,), 255, dtype=np.uint8)], axis=2)
    return np.ascontiguousarray(q)


def expected(name, color, depth, kx, ky, fmt=RGB32F, constants=None, twin=None):
    k = constants64(CONSTANTS.get(name, ()) if constants is None else constants)
    return deliver((twin or TWINS[name])(resolve_rgba(color, kx, ky), np.asarray(depth, dtype=F32), kx, ky, k), fmt)


# ---- the planes -----------------------------------------------------------------------------------------------------------------
def frame_size(out_size, factors):
    return out_size[0] * factors[0], out_size[1] * factors[1]


def color_plane(width, height, seed, kind="special"):
    """(height, width, 4): resolve_cases.special_plane (magnitudes, signs, subnormals, Inf, NaN, cancelling neighbours) or
    render_to_texture_cases.pool_plane (values around the quantiser's ties, in alpha too)."""
    return R.special_plane(height, width, seed) if kind == "special" else T.pool_plane(height, width, seed)


def plane_kind(name, fmt=RGB32F):
    """IDENTITY's floats run on the special plane, where the resolve's tree meets cancellation, overflow and NaN.  Every program whose
    own arithmetic is under test, and everything that goes through the quantiser, runs on the pool plane: under the larger factors the
    special plane's 64-sample averages are NaN or Inf nearly everywhere, which no wrong twin could be told from the right one on."""
    return "special" if name == "IDENTITY" and fmt == RGB32F else "pool"


@functools.lru_cache(maxsize=None)
def planes(out_size, factors, kind):
    """The frame a case uploads: (colour (h, w, 4), depth (h, w)), read-only and shared between the tests that need them."""
    w, h = frame_size(out_size, factors)
    color, depth = color_plane(w, h, 1000 * factors[0] + 100 * factors[1] + w + h, kind), depth_plane(w, h, w + h)
    color.setflags(write=False); depth.setflags(write=False)
    return color, depth


def depth_plane(width, height, seed):
    """(height, width) float32: depths in (0, 1) in runs, a quarter of the pixels float.MinValue (cleared), every sample of a block
    different from its neighbours so that the block's first and last samples never agree by accident."""
    rng = np.random.default_rng(seed + 101)
    d = rng.uniform(0.0, 1.0, (height, width)).astype(F32)
    d[rng.random((height, width)) < 0.25] = np.finfo(F32).min
    return d
