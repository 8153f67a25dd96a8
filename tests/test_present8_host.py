"""8-bit present, host side (no GPU): the numpy restatement of the quantiser gives the definition's known answers (include/swr.h,
csrc/swr_deliver.hip.h), each plausible wrong quantiser misses exactly the known answer named for it, the bytes round-trip through
k / 255, the generator delivers what the GPU test relies on, and the Python wrappers' shapes and argument checks."""
import types

import numpy as np
import pytest

import present8_cases as K
from softwarerenderer_amd import _native
from softwarerenderer_amd.rasterizer import MainWindow

NEW_EXPORTS = ("swr_present8_size", "swr_readback_rgb8", "swr_present_rgb8_async", "swr_resolve_rgb8_device", "swr_resolve_rgb8_device_async")


def check_ties_go_to_even(fn):
    """0x3b008081 * 255 is exactly 0.5 and 0x3efdfdfe * 255 exactly 126.5 in float32: 0 and 126; half-up gives 1 and 127."""
    assert K.answers(fn, K.KNOWN_TIES_TO_EVEN) == K.expected(K.KNOWN_TIES_TO_EVEN) == [0, 126]


def check_rounds_to_nearest(fn):
    """0.5 * 255 = 127.5 -> 128 and nextafter(1, 0) * 255 = 254.99998 -> 255; truncation gives 127 and 254."""
    assert K.answers(fn, K.KNOWN_NEAREST) == K.expected(K.KNOWN_NEAREST) == [128, 255]


def check_scale_is_255(fn):
    """0.75 * 255 = 191.25 -> 191; floor(0.75 * 256) = 192."""
    assert K.answers(fn, K.KNOWN_SCALE_255) == K.expected(K.KNOWN_SCALE_255) == [191]


def check_nan_is_zero(fn):
    """NaN -> 0; rounding first and clamping with r < 0 ? 0 : (r < 255 ? r : 255) lets it out as 255."""
    assert K.answers(fn, K.KNOWN_NAN) == K.expected(K.KNOWN_NAN) == [0]


CHECKS = {"half_up": check_ties_go_to_even, "truncate": check_rounds_to_nearest, "times_256": check_scale_is_255,
          "clamp_after_round": check_nan_is_zero}


def test_known_answers_of_the_definition():
    assert K.answers(K.quantise, K.KNOWN) == K.expected(K.KNOWN) == [0, 2, 126, 128, 254, 255, 0]
    # the first five really are ties of the float32 product
    prod = (np.array([x for x, _ in K.KNOWN[:5]], dtype=np.float32) * np.float32(255.0)).astype(np.float32)
    assert prod.tolist() == [0.5, 1.5, 126.5, 127.5, 254.5]
    for check in CHECKS.values():
        check(K.quantise)


def test_the_special_values():
    x = np.array([np.nan, 0.0, -0.0, -1e-30, -3.0, -np.inf, 1.0, 1.0000001, 256.0, 3e38, np.inf, 1e-45, 1.17549435e-38], dtype=np.float32)
    assert K.quantise(x).tolist() == [0, 0, 0, 0, 0, 0, 255, 255, 255, 255, 255, 0, 0]
    assert K.quantise(x).dtype == np.uint8 and K.quantise(x.reshape(13, 1)).shape == (13, 1)


@pytest.mark.parametrize("name", sorted(K.MUTANTS))
def test_each_mutant_fails_exactly_its_known_answer(name):
    for other, check in CHECKS.items():
        if other == name:
            with pytest.raises(AssertionError):
                check(K.MUTANTS[name])
        else:
            check(K.MUTANTS[name])
    # half-up is the one mutant the issue's table pins: word 0x3b008081 gives 1
    if name == "half_up":
        assert K.answers(K.quantise_half_up, K.KNOWN_TIES_TO_EVEN[:1]) == [1]


def test_every_level_round_trips():
    """quantise(float32(k) / 255) == k, and for the other way of writing the level too: under round-to-nearest an UnsignedByte upload
    of these bytes into a float texture, drawn with Nearest, displays the byte that was uploaded."""
    k = np.arange(256)
    assert np.array_equal(K.quantise(k.astype(np.float32) / np.float32(255.0)), k)
    assert np.array_equal(K.quantise((k / 255.0).astype(np.float32)), k)
    assert np.array_equal(K.quantise(k.astype(np.float32) * np.float32(1.0 / 255.0)), k)


def test_every_level_has_an_exact_tie_and_ties_go_to_even():
    ties = K.tie_inputs()
    assert sorted(ties) == list(range(255))
    for k, xs in ties.items():
        even = k if k % 2 == 0 else k + 1
        assert K.quantise(xs).tolist() == [even] * len(xs), k
        assert K.quantise_half_up(xs).tolist() == [k + 1] * len(xs), k
        assert K.quantise_truncate(xs).tolist() == [k] * len(xs), k


def test_resolve_then_quantise():
    """[[1e8, -1e8], [1, 1]] at (2, 2): rows first resolves to 0.5, 127.5 -> 128; columns first resolves to 0 -> 0."""
    plane, (kx, ky), want = K.KNOWN_COMBINED
    color = np.repeat(plane[:, :, None], 4, axis=2).astype(np.float32)
    color[..., 3] = 7.0
    assert want == 128
    for bpp in (3, 4):
        got = K.present8(color, kx, ky, bpp)
        assert got.shape == (1, 1, bpp) and got.dtype == np.uint8
        assert got[0, 0].tolist() == [128, 128, 128, 255][:bpp]
        assert K.present8(color, kx, ky, bpp, vertical_first=True)[0, 0].tolist() == [0, 0, 0, 255][:bpp]
    # under (1, 1) the payload is the flatten: alpha never reaches it
    assert K.present8(color, 1, 1, 4)[..., 3].tolist() == [[255, 255], [255, 255]]
    assert np.array_equal(K.present8(color, 1, 1, 3), K.quantise(color[..., :3]))


def test_the_tie_plane_delivers_what_the_gpu_test_relies_on():
    p = K.tie_plane(72, 136, seed=136)
    assert p.shape == (72, 136, 4) and p.dtype == np.float32
    rgb = p[..., :3]
    words = set(rgb.view(np.uint32).reshape(-1).tolist())
    ties = np.concatenate(list(K.tie_inputs().values()))
    assert all(int(w) in words for w in K.ulp_neighbours(ties).view(np.uint32))             # every tie, and its two neighbours
    k = np.arange(256)
    assert all(int(w) in words for w in (k / 255.0).astype(np.float32).view(np.uint32))
    assert np.isnan(rgb).any() and np.isposinf(rgb).any() and np.isneginf(rgb).any()
    assert ((rgb != 0) & (np.abs(rgb) < np.float32(1.17549435e-38))).any()                   # subnormals
    assert (rgb.view(np.uint32) == 0x80000000).any() and (rgb.view(np.uint32) == 0).any()    # -0 and +0
    assert (rgb == K.ONE_BELOW).any() and (rgb > 1).any() and (rgb < 0).any()
    # constant 8 x 8 blocks carry ties through every resolve: at (8, 8) some outputs are exact ties still
    r = K.R.resolve(p, 8, 8)
    prod = (np.where((r > 0) & (r < 1), r, np.float32(0.25)) * np.float32(255.0)).astype(np.float32)
    assert (prod - np.floor(prod) == 0.5).any()
    # the mutants are all visible on the plane itself
    want = K.present8(p, 1, 1, 3)
    for name, fn in K.MUTANTS.items():
        assert not np.array_equal(K.present8(p, 1, 1, 3, quantise_fn=fn), want), name
    small = K.tie_plane(24, 40, seed=40)
    assert small.shape == (24, 40, 4) and np.isnan(small[..., :3]).any()
    assert np.array_equal(K.tie_plane(24, 40, seed=40).view(np.uint32), small.view(np.uint32))          # seeded


class _FakeDevice:
    """Stands in for a Device: every native call succeeds and is recorded, so the wrappers' shapes and argument checks run without
    a GPU."""
    _ctx = None

    def __init__(self):
        self.calls = []

        def rec(name):
            def f(*a):
                self.calls.append((name, a))
                return 0
            return f
        ok = lambda *a: 0
        self._lib = types.SimpleNamespace(swr_resize=ok, swr_set_band=ok, swr_set_band_interleaved=ok, swr_bind_framebuffer=ok,
                                          **{n: rec(n) for n in NEW_EXPORTS})

    def _ck(self, rc):
        assert rc == 0


def test_present8_size_arithmetic():
    w = MainWindow(_FakeDevice(), 136, 72)
    assert w.Present8Size() == (72, 136, 3)
    assert w.Present8Size(8, 2, 4) == (36, 17, 4)
    w.SetBand(4, 1)                                         # the partial last tile row alone
    assert w.Present8Size(8, 8, 3) == (1, 17, 3)
    w.SetBand(-1, -1)
    for bad in (0, 1, 2, 5, 12, -3):
        with pytest.raises(ValueError):
            w.Present8Size(1, 1, bad)
    with pytest.raises(ValueError):
        w.Present8Size(3, 1, 3)
    w.Resize(36, 72)
    with pytest.raises(ValueError):
        w.Present8Size(8, 1, 3)                             # 36 is no multiple of 8
    w.Resize(0, 0)
    assert w.Present8Size(8, 8, 4) == (0, 0, 4)


def test_wrapper_shapes_and_argument_checks():
    dev = _FakeDevice()
    w = MainWindow(dev, 40, 24)
    out = w.ColorBuffer8()
    assert out.shape == (24, 40, 3) and out.dtype == np.uint8
    assert dev.calls[-1] == ("swr_readback_rgb8", (None, 1, 1, 3, out.ctypes.data))
    out = w.ColorBuffer8(8, 4, channels=4)
    assert out.shape == (6, 5, 4) and dev.calls[-1][1][1:4] == (8, 4, 4)
    mine = np.zeros((12, 20, 4), dtype=np.uint8)
    assert w.ColorBuffer8(2, 2, 4, out=mine) is mine
    n = len(dev.calls)
    for bad in (np.zeros((12, 20, 3), dtype=np.uint8), np.zeros((12, 20, 4), dtype=np.float32), np.zeros((12, 40, 4), dtype=np.uint8)[:, ::2]):
        with pytest.raises(ValueError):
            w.ColorBuffer8(2, 2, 4, out=bad)
    with pytest.raises(ValueError):
        w.ColorBuffer8(1, 1, channels=2)
    # Present8Async takes the format from the array
    t = w.Present8Async(mine, 2, 2)
    assert isinstance(t, int) and dev.calls[-1][0] == "swr_present_rgb8_async" and dev.calls[-1][1][1:4] == (2, 2, 4)
    w.Present8Async(np.zeros((24, 40, 3), dtype=np.uint8))
    assert dev.calls[-1][1][1:4] == (1, 1, 3)
    n = len(dev.calls)
    for bad in (np.zeros((24, 40, 2), dtype=np.uint8), np.zeros((24, 40), dtype=np.uint8), np.zeros((24, 40, 3), dtype=np.float32),
                np.zeros((12, 20, 3), dtype=np.uint8)):
        with pytest.raises(ValueError):
            w.Present8Async(bad)
    with pytest.raises(ValueError):
        w.Present8Async(mine, 2, 3)
    assert len(dev.calls) == n                              # nothing refused reached the library
    w.Quantise8To(4096, 4, 2, 3)
    assert dev.calls[-1][0] == "swr_resolve_rgb8_device" and dev.calls[-1][1][1:4] == (4, 2, 3) and dev.calls[-1][1][4].value == 4096
    w.Quantise8ToAsync(4096, channels=4)
    assert dev.calls[-1][0] == "swr_resolve_rgb8_device_async" and dev.calls[-1][1][1:4] == (1, 1, 4)
    # a zero-size window delivers an empty array without a native call
    w.Resize(0, 0)
    n = len(dev.calls)
    assert w.ColorBuffer8(4, 4, 4).shape == (0, 0, 4) and len(dev.calls) == n


def test_the_binding_declares_the_present8_entry_points():
    for name in NEW_EXPORTS:
        assert name in _native.EXPORTS, name
    for name in ("Present8Size", "ColorBuffer8", "Present8Async", "Quantise8To", "Quantise8ToAsync"):
        assert callable(getattr(MainWindow, name, None)), name
