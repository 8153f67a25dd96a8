"""Render to texture, host side: the numpy restatement of tests/render_to_texture_cases.py against the
restatements it is built from, the block-linear permutation, the C# surface and the size rule of the GPU tests' shapes.  No GPU."""
import os
import re

import numpy as np
import pytest

import present8_cases as K
import render_to_texture_cases as T
import resolve_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plane():
    p = T.pool_plane(32, 48, 19)
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("kx,ky", T.PAIRS)
def test_alpha_opaque_is_the_eight_bit_present_at_four_bytes(plane, kx, ky):
    got = T.texels(plane, kx, ky)
    assert got.dtype == np.uint8 and got.shape == (32 // ky, 48 // kx, 4)
    assert np.array_equal(got, K.present8(plane, kx, ky, bpp=4))
    assert np.all(got[..., 3] == 255)


@pytest.mark.parametrize("kx,ky", T.PAIRS)
def test_alpha_kept_leaves_rgb_alone_and_resolves_alpha_like_a_colour_channel(plane, kx, ky):
    opaque, kept = T.texels(plane, kx, ky), T.texels(plane, kx, ky, keep_alpha=True)
    assert np.array_equal(kept[..., :3], opaque[..., :3])
    # the same plane with alpha moved into R: the three-channel restatement's R is the kept A
    moved = plane.copy()
    moved[..., 0] = plane[..., 3]
    assert np.array_equal(kept[..., 3], K.present8(moved, kx, ky, bpp=3)[..., 0])
    assert len(np.unique(kept[..., 3])) > 8                           # alpha is not a constant in disguise


def test_alpha_follows_the_pool_of_the_eight_bit_present():
    """Ties, NaN, +-0, +-Inf, subnormals and one ulp below 1 in ALPHA give what the quantiser's known answers give in colour."""
    pool = K.pool()
    side = int(np.ceil(np.sqrt(pool.size)))
    a = np.resize(pool, side * side).reshape(side, side)
    color = np.full((side, side, 4), 0.5, dtype=np.float32)
    color[..., 3] = a
    got = T.texels(color, 1, 1, keep_alpha=True)
    assert np.array_equal(got[..., 3], K.quantise(a))
    assert np.all(got[..., :3] == 128)                                # 0.5 * 255 = 127.5: the tie goes to even
    for cases in (K.KNOWN, K.KNOWN_TIES_TO_EVEN, K.KNOWN_NEAREST, K.KNOWN_SCALE_255, K.KNOWN_NAN):
        for value, want in cases:
            for kx, ky in ((1, 1), (2, 2), (8, 4)):                   # the average of 2^n equal values is that value
                c = np.zeros((ky, kx, 4), dtype=np.float32)
                c[..., 3] = value
                assert T.texels(c, kx, ky, keep_alpha=True)[0, 0].tolist() == [0, 0, 0, want], (value, kx, ky)
                assert T.texels(c, kx, ky)[0, 0].tolist() == [0, 0, 0, 255]
    specials = {np.float32(np.inf): 255, np.float32(-np.inf): 0, np.float32(-0.0): 0, np.float32(0.0): 0, K.ONE_BELOW: 255,
                np.float32(1.0): 255, np.float32(-3.0): 0}
    for value, want in specials.items():
        c = np.zeros((1, 1, 4), dtype=np.float32)
        c[..., 3] = value
        assert int(T.texels(c, 1, 1, keep_alpha=True)[0, 0, 3]) == want, value


def test_alpha_goes_through_the_same_tree_in_the_same_stage_order():
    for case in (R.KNOWN_TREE_ORDER, R.KNOWN_STAGE_ORDER):
        chan, (kx, ky), want = case
        c = np.zeros(chan.shape + (4,), dtype=np.float32)
        c[..., 3] = chan
        assert int(T.texels(c, kx, ky, keep_alpha=True)[0, 0, 3]) == int(K.quantise(np.array([want], dtype=np.float32))[0])
    # the stage-order case separates the two orders after the quantiser as well: 0.5 -> 128, columns first 0 -> 0
    chan, (kx, ky), byte = K.KNOWN_COMBINED
    c = np.zeros(chan.shape + (4,), dtype=np.float32)
    c[..., 3] = chan
    assert int(T.texels(c, kx, ky, keep_alpha=True)[0, 0, 3]) == byte == 128


@pytest.mark.parametrize("w,h", [(4, 4), (8, 4), (64, 12)])
def test_the_block_linear_permutation_is_a_bijection(w, h):
    perm = T.blocked_permutation(w, h)
    assert perm.shape == (h, w)
    assert np.array_equal(np.sort(perm.reshape(-1)), np.arange(w * h))
    # a 4 x 4 block is 16 consecutive texels (one 64-byte line), blocks row-major
    for by in range(h // 4):
        for bx in range(w // 4):
            block = perm[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4].reshape(-1)
            assert np.array_equal(block, (by * (w // 4) + bx) * 16 + np.arange(16))


def test_the_csharp_texture_declares_the_three_calls():
    cs = open(os.path.join(ROOT, "csharp", "RasterizerNative.cs")).read()
    body = cs[cs.index("class TextureNative : IDisposable"):]
    assert re.search(r"public static TextureNative CreateTarget\(int width, int height\)", body)
    assert re.search(r"public void UpdateFrom\(int kx = 1, int ky = 1, bool keepAlpha = false", body)
    assert re.search(r"public byte\[\] Read\(\)", body)
    for fn in ("swr_texture_create_target", "swr_texture_update_from_frame", "swr_texture_readback"):
        assert body.count("Native." + fn) == 1, fn
    hpp = open(os.path.join(ROOT, "softwarerenderer_amd", "cpp", "Rasterizer.hpp")).read()
    for name in ("static Texture Target(", "void UpdateFrom(const MainWindow& window, int kx = 1, int ky = 1, bool keepAlpha = false)", "Read() const"):
        assert name in hpp, name


def test_every_gpu_shape_satisfies_the_size_rule():
    assert len(T.GPU_SHAPES) == 6
    for tex, factors in T.GPU_SHAPES:
        frame = T.source_size(tex, factors)
        assert T.size_rule_holds(tex, factors, frame)
        assert not T.size_rule_holds(tex, factors, (frame[0] + 1, frame[1])) and not T.size_rule_holds(tex, (3, 1), frame)
        assert 0 < frame[0] <= 65535 and 0 < frame[1] <= 65535 and tex[0] * tex[1] < 1 << 30
        # the restatement accepts exactly that frame
        assert T.texels(np.zeros((frame[1], frame[0], 4), dtype=np.float32), *factors).shape == (tex[1], tex[0], 4)
    for tex, factors in T.BLOCKED_SHAPES:
        assert (tex, factors) in T.GPU_SHAPES and tex[0] % 4 == 0 and tex[1] % 4 == 0
    assert any(tex[0] % 4 or tex[1] % 4 for tex, _ in T.GPU_SHAPES)   # and one shape that can have no block-linear copy
