"""Supersampled present, host side (no GPU): the numpy restatement of the resolve arithmetic has the tree order and the stage order
the definition fixes (include/swr.h, csrc/swr_deliver.hip.h) -- known answers that the plausible wrong orders miss --, the payload's
size arithmetic of MainWindow.ResolvedSize, and the new entry points' names."""
import types

import numpy as np
import pytest

import resolve_cases as K
from softwarerenderer_amd import _native
from softwarerenderer_amd.rasterizer import MainWindow

NEW_EXPORTS = ("swr_resolved_size", "swr_readback_rgb_resolved", "swr_present_rgb_resolved_async", "swr_resolve_rgb_device",
               "swr_resolve_rgb_device_async")


def check_tree_order(fn):
    """[1e8, 1, -1e8, 1] at (4, 1): (1e8 + 1) + (-1e8 + 1) = 1e8 + -1e8 = 0 in float32; left to right gives ((1e8 + 1) - 1e8) + 1 = 1,
    i.e. 0.25 after the scale."""
    assert K.known_answer(fn, K.KNOWN_TREE_ORDER) == K.KNOWN_TREE_ORDER[2] == 0.0


def check_stage_order(fn):
    """[[1e8, -1e8], [1, 1]] at (2, 2): rows first gives (1e8 - 1e8) + (1 + 1) = 2 -> 0.5; columns first gives (1e8 + 1) + (-1e8 + 1) = 0."""
    assert K.known_answer(fn, K.KNOWN_STAGE_ORDER) == K.KNOWN_STAGE_ORDER[2] == 0.5


def test_known_answer_for_the_tree_order():
    check_tree_order(K.resolve)


def test_known_answer_for_the_stage_order():
    check_stage_order(K.resolve)


def test_the_known_answers_reject_the_mutants():
    """A sequential sum and a vertical-first resolve are the two ways to get the definition wrong without noticing on smooth data."""
    with pytest.raises(AssertionError):
        check_tree_order(K.resolve_sequential)
    assert K.known_answer(K.resolve_sequential, K.KNOWN_TREE_ORDER) == 0.25
    with pytest.raises(AssertionError):
        check_stage_order(K.resolve_vertical_first)
    assert K.known_answer(K.resolve_vertical_first, K.KNOWN_STAGE_ORDER) == 0.0
    # each mutant is caught by ITS test: the other order is still right in it
    check_stage_order(K.resolve_sequential)
    check_tree_order(K.resolve_vertical_first)


def test_restatement_basics():
    """(1, 1) is the flatten; an 8 x 8 block of ones averages to one; alpha never reaches the result; the scale is a power of two."""
    p = K.special_plane(16, 24, seed=1)
    K.assert_same_words(K.resolve(p, 1, 1), p[..., :3])
    ones = np.ones((8, 8, 4), dtype=np.float32)
    assert np.array_equal(K.resolve(ones, 8, 8), np.ones((1, 1, 3), dtype=np.float32))
    q = p.copy(); q[..., 3] = np.nan
    for kx, ky in K.PAIRS:
        K.assert_same_words(K.resolve(q, kx, ky), K.resolve(p, kx, ky), (kx, ky))
        assert K.resolve(p, kx, ky).shape == (16 // ky, 24 // kx, 3)
    # the generator delivers what the GPU test relies on
    big = K.special_plane(24, 40, seed=2)[..., :3]
    assert np.isnan(big).any() and np.isposinf(big).any() and np.isneginf(big).any()
    assert ((big != 0) & (np.abs(big) < np.float32(1.17549435e-38))).any()                   # subnormals
    assert (big.view(np.uint32) == 0x80000000).any() and (big.view(np.uint32) == 0).any()    # -0 and +0
    r = K.resolve(big, 2, 2)
    assert np.isnan(r).sum() > np.isnan(big).sum() // 4                                      # Inf - Inf made new NaNs


class _NoDevice:
    """Stands in for a Device where only MainWindow's host-side arithmetic is exercised: every native call succeeds."""
    _ctx = None

    def __init__(self):
        ok = lambda *a: 0
        self._lib = types.SimpleNamespace(swr_resize=ok, swr_set_band=ok, swr_set_band_interleaved=ok, swr_bind_framebuffer=ok)

    def _ck(self, rc):
        assert rc == 0


def test_resolved_size_arithmetic():
    w = MainWindow(_NoDevice(), 136, 72)                    # 5 tile rows, the last one holds 8 pixel rows
    assert w.ResolvedSize(1, 1) == (72, 136)
    assert w.ResolvedSize(8, 2) == (36, 17)
    assert w.ResolvedSize(2, 8) == (9, 68)
    w.SetBand(3, 2)                                         # tile rows 3 and 4: 16 + 8 pixel rows
    assert w.band_pixel_rows() == (48, 24)
    assert w.ResolvedSize(4, 8) == (3, 34) and w.ResolvedSize(1, 4) == (6, 136)
    w.SetBand(4, 1)                                         # the partial last tile row alone
    assert w.ResolvedSize(8, 8) == (1, 17)
    w.SetBandInterleaved(1, 2, 1)                           # stripes 1 and 3: 32 rows; rank 0 holds stripes 0, 2 and 4: 16 + 16 + 8
    assert w.ResolvedSize(2, 8) == (4, 68)
    w.SetBandInterleaved(0, 2, 1)
    assert w.ResolvedSize(2, 8) == (5, 68)
    w.SetBand(-1, -1)
    for bad in (0, 3, 16, -2):
        with pytest.raises(ValueError):
            w.ResolvedSize(bad, 1)
        with pytest.raises(ValueError):
            w.ResolvedSize(1, bad)
    w.Resize(36, 72)
    with pytest.raises(ValueError):
        w.ResolvedSize(8, 1)                                # 36 is no multiple of 8
    assert w.ResolvedSize(4, 8) == (9, 9)
    w.Resize(136, 20)
    with pytest.raises(ValueError):
        w.ResolvedSize(1, 8)
    w.Resize(0, 0)
    assert w.ResolvedSize(8, 8) == (0, 0)                   # a zero-size target resolves to nothing under any factors


def test_the_binding_declares_the_resolve_entry_points():
    for name in NEW_EXPORTS:
        assert name in _native.EXPORTS, name
    for name in ("ResolvedSize", "ResolvedColorBuffer", "PresentResolvedAsync", "ResolveTo", "ResolveToAsync"):
        assert callable(getattr(MainWindow, name, None)), name
