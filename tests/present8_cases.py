"""The 8-bit present's quantiser restated in numpy float32 (include/swr.h, csrc/swr_deliver.hip.h), the planes the present8 tests run
it on, and the mutants its known answers must reject.  Not a test module: tests/test_present8_host.py and tests/test_gpu_present8.py
import it.

The input per output pixel is what the float payload delivers: resolve_cases.resolve (the flatten under (1, 1)).  Per channel c:
NaN -> 0; c <= 0 -> 0; c >= 1 -> 255; otherwise uint8(rint(float32(c * 255))), ties to even.  numpy's float32 `*` is one IEEE single
multiply and np.rint rounds half to even, which is all the definition uses."""
import numpy as np

import resolve_cases as R

PAIRS = R.PAIRS
F255 = np.float32(255.0)


def _gate(c, mid_value):
    """The definition's cases around a rounding rule: mid_value holds the rule's result where 0 < c < 1 (anything elsewhere)."""
    mid = (c > 0) & (c < 1)                                           # False for NaN
    out = np.where(mid, mid_value, np.where(c >= 1, 255.0, 0.0))
    return out.astype(np.uint8)


def _product(c, scale=F255):
    c = np.asarray(c, dtype=np.float32)
    safe = np.where((c > 0) & (c < 1), c, np.float32(0.5)).astype(np.float32)       # keeps NaN and Inf out of the arithmetic
    return c, (safe * scale).astype(np.float32)


def quantise(rgb):
    """THE RESTATEMENT: float32 array -> uint8 array of the same shape."""
    c, prod = _product(rgb)
    return _gate(c, np.rint(prod))


def quantise_half_up(rgb):
    """MUTANT: ties away from zero, floor(x + 0.5) (evaluated exactly)."""
    c, prod = _product(rgb)
    return _gate(c, np.floor(prod.astype(np.float64) + 0.5))


def quantise_truncate(rgb):
    """MUTANT: (uint8)(c * 255)."""
    c, prod = _product(rgb)
    return _gate(c, np.floor(prod))


def quantise_times_256(rgb):
    """MUTANT: min(255, floor(c * 256))."""
    c, prod = _product(rgb, np.float32(256.0))
    return _gate(c, np.minimum(np.floor(prod), 255.0))


def quantise_clamp_after_round(rgb):
    """MUTANT: round first, then clamp as r < 0 ? 0 : (r < 255 ? r : 255) -- every comparison with NaN is false, so NaN passes the
    lower clamp and leaves as 255."""
    c = np.asarray(rgb, dtype=np.float32)
    with np.errstate(all="ignore"):
        r = np.rint((c * F255).astype(np.float32))
        r = np.where(r < 0, np.float32(0), np.where(r < 255, r, np.float32(255)))
    return r.astype(np.uint8)


MUTANTS = {"half_up": quantise_half_up, "truncate": quantise_truncate, "times_256": quantise_times_256,
           "clamp_after_round": quantise_clamp_after_round}


def present8(color, kx, ky, bpp, quantise_fn=quantise, **resolve_kw):
    """color: (rows, W, >= 3) float32 -> (rows / ky, W / kx, bpp) uint8; the fourth byte of bpp = 4 is 255."""
    assert bpp in (3, 4)
    q = quantise_fn(R.resolve(color, kx, ky, **resolve_kw))
    if bpp == 4:
        q = np.concatenate([q, np.full(q.shape[:2] + (1,), 255, dtype=np.uint8)], axis=2)
    return np.ascontiguousarray(q)


def word(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


ONE_BELOW = np.nextafter(np.float32(1.0), np.float32(0.0))
# the definition's known answers: (input, result); the first five are exact ties of c * 255 in float32
KNOWN = [(word(0x3b008081), 0), (word(0x3bc0c0c1), 2), (word(0x3efdfdfe), 126), (word(0x3f000000), 128), (word(0x3f7f7f7f), 254),
         (ONE_BELOW, 255), (np.float32(1e-45), 0)]
# the named known answers, one per mutant: each is missed by its mutant and by no other
KNOWN_TIES_TO_EVEN = [(word(0x3b008081), 0), (word(0x3efdfdfe), 126)]             # half-up: 1 and 127
KNOWN_NEAREST = [(word(0x3f000000), 128), (ONE_BELOW, 255)]                       # truncate: 127 and 254
KNOWN_SCALE_255 = [(np.float32(0.75), 191)]                                       # 191.25; times 256: 192
KNOWN_NAN = [(np.float32(np.nan), 0)]                                             # clamp after round: 255
# resolve, then quantise: the stage-order case of resolve_cases gives 0.5 -> 127.5 -> 128; columns first gives 0 -> 0
KNOWN_COMBINED = (R.KNOWN_STAGE_ORDER[0], R.KNOWN_STAGE_ORDER[1], 128)


def answers(fn, cases):
    return [int(fn(np.array([x], dtype=np.float32))[0]) for x, _ in cases]


def expected(cases):
    return [want for _, want in cases]


def tie_inputs():
    """Every float32 c with float32(c * 255) == k + 0.5 exactly, k in 0..254, found within a few ulps of float32((k + 0.5) / 255):
    {k: [inputs]}.  Every k has at least one."""
    out = {}
    for k in range(255):
        centre = np.array([np.float32((k + 0.5) / 255.0)], dtype=np.float32).view(np.uint32)[0]
        cand = (np.arange(-8, 9, dtype=np.int64) + int(centre)).astype(np.uint32).view(np.float32)
        hit = cand[(cand * F255).astype(np.float32) == np.float32(k + 0.5)]
        assert hit.size, k
        out[k] = hit
    return out


def ulp_neighbours(x):
    x = np.asarray(x, dtype=np.float32)
    return np.concatenate([np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))])


def pool():
    """The values a tie_plane deals out besides its uniform fill."""
    ties = ulp_neighbours(np.concatenate(list(tie_inputs().values())))
    k = np.arange(256)
    levels = np.concatenate([(k / 255.0).astype(np.float32), k.astype(np.float32) * np.float32(1.0 / 255.0)])
    sub = np.array([1, 0x1234, 0x7fffff, 0x80000001, 0x807fffff], dtype=np.uint32).view(np.float32)
    specials = np.concatenate([sub, np.array([0.0, -0.0, -1e-30, -0.5, -3.0, 1.0, 1.0000001, 1.5, 256.0, 3e38, -3e38, np.inf, -np.inf,
                                              np.nan, ONE_BELOW, 1e-45, 1.17549435e-38], dtype=np.float32)])
    return np.concatenate([ties, levels, np.tile(specials, 8)]).astype(np.float32)


def tie_plane(rows, width, seed):
    """(rows, width, 4) float32.  Every channel is drawn from the pool -- all exact-tie inputs, each also at +-1 ulp; k / 255 and
    float32(k) * float32(1 / 255); +-0, subnormals, negatives, values above 1, +-Inf, NaN, nextafter(1, 0) -- or from a uniform fill
    over [-0.25, 1.25].  The pool is dealt over up to 60 % of the R, G, B channels in a seeded order.  Then one 8 x 8 block in four
    (rows and width are multiples of 8 in the tests) is made constant per channel: the average of 2^n equal values is that value,
    so ties and specials reach the quantiser under every factor pair, not only under (1, 1).  Alpha carries values of its own."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.25, 1.25, (rows, width, 4)).astype(np.float32)
    values = pool()
    slots = rng.permutation(rows * width * 3)
    slots = slots[: max(len(slots) * 6 // 10, 1)]
    rgb = p[..., :3].reshape(-1).copy()
    rgb[slots] = values[rng.permutation(len(slots)) % len(values)]
    p[..., :3] = rgb.reshape(rows, width, 3)
    p[..., 3] = np.where(rng.random((rows, width)) < 0.1, np.float32(np.nan), p[..., 3] * np.float32(7.0))
    for by in range(rows // 8):
        for bx in range(width // 8):
            if rng.random() < 0.25:
                p[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8, :3] = p[by * 8, bx * 8, :3]
    return p
