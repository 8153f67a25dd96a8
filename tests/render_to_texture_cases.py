"""Render to texture restated in numpy (include/swr.h, csrc/swr_deliver.hip.h), the planes and shapes its tests run
on.  Not a test module: tests/test_render_to_texture_host.py and tests/test_gpu_render_to_texture.py import it.

Texel (x, y) of a w x h texture updated from a frame of w * kx by h * ky pixels: R, G, B are the bytes of the 8-bit present at 4 bytes
per pixel (present8_cases.present8: resolve_cases.resolve, then the quantiser); A is 255, or with keep_alpha the frame's alpha channel
through the same resolve and the same quantiser.  Nothing here has arithmetic of its own."""
import numpy as np

import present8_cases as K
import resolve_cases as R

PAIRS = R.PAIRS
ALPHA_OPAQUE, ALPHA_KEEP = 0, 1

# the GPU tests' shapes, texture (w, h) x factors (kx, ky): one block's corner; a full 64-wide block plus a 4-texel tail and a second
# block row; odd sides (no block-linear copy possible) over two blocks in x and y; each factor alone at its widest; the most rows per
# thread; three blocks in x and y under the largest factors
GPU_SHAPES = [((4, 4), (1, 1)), ((68, 8), (1, 1)), ((67, 5), (2, 2)), ((64, 4), (4, 1)), ((8, 16), (1, 8)), ((132, 12), (8, 8))]
BLOCKED_SHAPES = [((68, 8), (1, 1)), ((132, 12), (8, 8))]


def source_size(tex_size, factors):
    """THE SIZE RULE: the frame a (w, h) texture is updated from under (kx, ky) measures (w * kx, h * ky)."""
    return tex_size[0] * factors[0], tex_size[1] * factors[1]


def size_rule_holds(tex_size, factors, frame_size):
    return factors[0] in R.FACTORS and factors[1] in R.FACTORS and source_size(tex_size, factors) == tuple(frame_size)


def alpha_bytes(color, kx, ky):
    """The frame's alpha through the three-channel restatement: the channel rides in R's place."""
    a = np.repeat(np.asarray(color, dtype=np.float32)[..., 3:4], 3, axis=2)
    return K.quantise(R.resolve(a, kx, ky))[..., 0]


def texels(color, kx, ky, keep_alpha=False):
    """THE RESTATEMENT: color (h * ky, w * kx, 4) float32 -> (h, w, 4) uint8."""
    out = K.present8(color, kx, ky, 4).copy()
    if keep_alpha:
        out[..., 3] = alpha_bytes(color, kx, ky)
    return np.ascontiguousarray(out)


def blocked_offset(w, x, y):
    """Texel index of (x, y) in the block-linear copy of a texture w wide: 4 x 4-texel blocks of 64 B, blocks row-major
    (bilinear_texel_offset<true>, csrc/swr_device.h)."""
    return (((y >> 2) * (w >> 2) + (x >> 2)) << 4) + ((y & 3) << 2) + (x & 3)


def blocked_permutation(w, h):
    """flat block-linear index of every row-major texel, shape (h, w); w and h multiples of 4."""
    assert w % 4 == 0 and h % 4 == 0
    y, x = np.mgrid[0:h, 0:w]
    return blocked_offset(w, x, y)


def pool_plane(rows, width, seed):
    """(rows, width, 4) float32: present8_cases.tie_plane, and alpha drawn the same way -- 60 % of it dealt from the pool (every exact
    tie at +-1 ulp, k / 255, +-0, subnormals, negatives, values above 1, +-Inf, NaN, nextafter(1, 0)), the rest uniform over
    [-0.25, 1.25], then constant over one 8 x 8 block in four, so that ties and specials survive every factor pair."""
    p = K.tie_plane(rows, width, seed)
    rng = np.random.default_rng(seed + 7919)
    a = rng.uniform(-0.25, 1.25, rows * width).astype(np.float32)
    values = K.pool()
    slots = rng.permutation(rows * width)
    slots = slots[: max(len(slots) * 6 // 10, 1)]
    a[slots] = values[rng.permutation(len(slots)) % len(values)]
    a = a.reshape(rows, width)
    for by in range((rows + 7) // 8):
        for bx in range((width + 7) // 8):
            if rng.random() < 0.25:
                a[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = a[by * 8, bx * 8]
    p[..., 3] = a
    return p


def texel_centres(w, h):
    """uv of every texel's centre, (h, w, 2) float32: Texture.Sample's nearest index of it is the texel itself."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x + 0.5) / w, (y + 0.5) / h], axis=-1).astype(np.float32)
