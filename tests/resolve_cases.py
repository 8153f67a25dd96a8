"""The supersampled present's arithmetic restated in numpy float32 (include/swr.h, csrc/swr_deliver.hip.h), and the planes the
resolve tests run it on.  Not a test module: tests/test_resolve_host.py and tests/test_gpu_resolve.py import it.

Per output pixel and channel R, G, B: the kx samples of each source row summed as a balanced pairwise tree left to right, the ky row
sums by the same tree top to bottom, times float32(1 / (kx * ky)).  numpy's float32 `+` and `*` are IEEE single operations (nothing
fuses, denormals are kept), which is all the definition uses."""
import numpy as np

FACTORS = (1, 2, 4, 8)
PAIRS = [(kx, ky) for kx in FACTORS for ky in FACTORS]


def tree_sum(parts):
    """Balanced pairwise tree over 1, 2, 4 or 8 float32 arrays, in order: ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7))."""
    parts = list(parts)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
    return parts[0]


def sequential_sum(parts):
    """MUTANT: left-to-right running sum, ((p0+p1)+p2)+p3 ..."""
    parts = list(parts)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc


def resolve(color, kx, ky, sum_fn=tree_sum, vertical_first=False):
    """color: (rows, W, >= 3) float32 with rows % ky == 0 and W % kx == 0 -> (rows / ky, W / kx, 3) float32.
    sum_fn / vertical_first select the mutants that the known-answer tests must reject."""
    c = np.ascontiguousarray(np.asarray(color, dtype=np.float32)[..., :3])
    rows, w, _ = c.shape
    assert rows % ky == 0 and w % kx == 0
    c = c.reshape(rows // ky, ky, w // kx, kx, 3)
    with np.errstate(all="ignore"):
        if vertical_first:
            v = sum_fn([c[:, r] for r in range(ky)])                  # (R, OW, kx, 3)
            s = sum_fn([v[:, :, i] for i in range(kx)])
        else:
            h = sum_fn([c[:, :, :, i] for i in range(kx)])            # (R, ky, OW, 3)
            s = sum_fn([h[:, r] for r in range(ky)])
        return (s * np.float32(1.0 / (kx * ky))).astype(np.float32)


def resolve_sequential(color, kx, ky):
    return resolve(color, kx, ky, sum_fn=sequential_sum)


def resolve_vertical_first(color, kx, ky):
    return resolve(color, kx, ky, vertical_first=True)


# the two known answers of the definition: (input plane rows x W of one channel, (kx, ky), expected value)
KNOWN_TREE_ORDER = (np.array([[1e8, 1.0, -1e8, 1.0]], dtype=np.float32), (4, 1), 0.0)         # left to right: 0.25
KNOWN_STAGE_ORDER = (np.array([[1e8, -1e8], [1.0, 1.0]], dtype=np.float32), (2, 2), 0.5)      # vertical first: 0.0


def known_answer(fn, case):
    """fn's value for a known-answer case (the channel plane replicated into R, G, B, another value in alpha)."""
    plane, (kx, ky), _ = case
    color = np.repeat(plane[:, :, None], 4, axis=2).astype(np.float32)
    color[..., 3] = 7.0
    out = fn(color, kx, ky)
    assert out.shape == (1, 1, 3) and out[0, 0, 0] == out[0, 0, 1] == out[0, 0, 2]
    return float(out[0, 0, 0])


def special_plane(rows, width, seed):
    """(rows, width, 4) float32: seeded values across magnitudes and signs, +-0, subnormals, +-Inf, NaN, neighbours that cancel
    (exactly, nearly, and as Inf - Inf), and sums that overflow.  Alpha carries values of its own: the resolve must drop them."""
    rng = np.random.default_rng(seed)
    n = rows * width * 4
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    v = (sign * rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-40, 41, n))).astype(np.float32)
    kind = rng.random(n)
    big = (sign * rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(120, 128, n))).astype(np.float32)        # sums overflow to +-Inf
    tiny = (sign * rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-130, -124, n))).astype(np.float32)    # averages fall below FLT_MIN
    sub = rng.integers(1, 0x800000, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)
    v = np.where(kind < 0.06, big, v)
    v = np.where((kind >= 0.06) & (kind < 0.12), tiny, v)
    v = np.where((kind >= 0.12) & (kind < 0.17), sub.view(np.float32), v)
    v = np.where((kind >= 0.17) & (kind < 0.20), np.float32(0.0) * sign.astype(np.float32), v)               # +0 and -0
    v = np.where((kind >= 0.20) & (kind < 0.22), (sign * np.inf).astype(np.float32), v)
    v = np.where((kind >= 0.22) & (kind < 0.23), np.float32(np.nan), v)
    p = v.astype(np.float32).reshape(rows, width, 4)
    # neighbours that cancel, horizontally and vertically (only where the neighbour exists)
    for _ in range(max(4, rows * width // 24)):
        y, x, ch = int(rng.integers(0, rows)), int(rng.integers(0, width)), int(rng.integers(0, 3))
        how = int(rng.integers(0, 3))
        a = p[y, x, ch] if np.isfinite(p[y, x, ch]) else np.float32(3.0)
        other = {0: -a, 1: np.nextafter(-a, np.float32(0.0)), 2: np.float32(-np.inf)}[how]
        if how == 2:
            a = np.float32(np.inf)
        p[y, x, ch] = a
        if rng.random() < 0.5 and x + 1 < width:
            p[y, x + 1, ch] = other
        elif y + 1 < rows:
            p[y + 1, x, ch] = other
    return p


def assert_same_words(got, want, what=""):
    """Word for word on uint32 views; NaN positions are compared as NaN (a NaN's payload is unspecified)."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions differ", int((gn != wn).sum()))
    g, w = np.where(gn, np.float32(0), got).view(np.uint32), np.where(wn, np.float32(0), want).view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, f"{len(bad)} words differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}")
