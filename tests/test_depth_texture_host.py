"""Depth textures without a GPU (include/swr.h): the numpy restatement of tests/depth_texture_cases.py against
independent formulations and hand-written known answers, its lookups against the nearest sampler's index and the oracle's bilinear
footprint, the four program texts through the run-time compile step, the new names in all four bindings, and the kernels' resource
usage from the compiler's remarks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import depth_texture_cases as D
import post_texture_cases as X
import resolve_cases as R
from softwarerenderer_amd import _native as N
from test_post_host import HIPCC, ROOT, validate

F32 = np.float32
NAN = D.from_words([D.NAN_A])[0]
ENTRY_POINTS = ("swr_texture_create_depth", "swr_texture_update_from_depth", "swr_texture_readback_depth", "swr_texture_sample_depth",
                "swr_texture_format")


def same_words(got, want, what=""):
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(D.words(got) != D.words(want))
    assert bad.size == 0, (what, f"{len(bad)} words differ, first at {tuple(bad[0])}")


# ---- the reduction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", D.REDUCTIONS)
def test_under_one_by_one_every_reduction_copies_the_plane(mode):
    p = D.depth_pool_plane(24, 40, 1)
    assert np.isnan(p).any() and (D.words(p) == 0x80000000).any()
    same_words(D.reduce(p, 1, 1, mode), p)


@pytest.mark.parametrize("kx,ky", R.PAIRS)
def test_on_finite_planes_max_and_min_are_the_blocks_extremes_and_first_the_top_left_word(kx, ky):
    """An independent formulation: np.max / np.min over the block axis; no NaN and one sign of zero, where the tree order cannot show."""
    rng = np.random.default_rng(kx * 10 + ky)
    p = rng.uniform(0.0, 1.0, (8 * ky, 12 * kx)).astype(F32)
    p[rng.integers(0, p.shape[0], 40), rng.integers(0, p.shape[1], 40)] = D.MINVALUE
    blocks = p.reshape(8, ky, 12, kx)
    same_words(D.reduce(p, kx, ky, D.MAX), blocks.max(axis=(1, 3)), "max")
    same_words(D.reduce(p, kx, ky, D.MIN), blocks.min(axis=(1, 3)), "min")
    same_words(D.reduce(p, kx, ky, D.FIRST), p[::ky, ::kx], "first")
    q = D.depth_pool_plane(8 * ky, 12 * kx, 2)
    same_words(D.reduce(q, kx, ky, D.FIRST), q[::ky, ::kx], "first, specials")


def one_block(values, kx, ky, mode):
    return D.words(D.reduce(np.array(values, dtype=F32).reshape(ky, kx), kx, ky, mode))[0, 0]


def test_known_answers_pin_the_tree_order():
    """A NaN wins exactly where it is the left operand of every select above it: position 0 always; position 2 of four beats
    position 3 only."""
    w = lambda f: D.words(np.array([f], dtype=F32))[0]
    for mode, best in ((D.MAX, 4.0), (D.MIN, 1.0)):
        for shape in ((2, 2), (4, 1), (1, 4)):
            kx, ky = shape
            # the tree over four leaves l0..l3 (row-major for 2 x 2): pick(pick(l0, l1), pick(l2, l3))
            assert one_block([NAN, 2.0, 3.0, 4.0 if mode == D.MAX else 1.0], kx, ky, mode) == D.NAN_A, (mode, shape, 0)
            # a NaN at l1 is never taken by the first pick: the rest decides
            assert one_block([2.0, NAN, 3.0, best], kx, ky, mode) == w(best), (mode, shape, 1)
            # a NaN at l2 takes its pair, and is then the RIGHT operand of the root: not taken
            assert one_block([2.0, 3.0, NAN, best], kx, ky, mode) == w(3.0 if mode == D.MAX else 2.0), (mode, shape, 2)
            assert one_block([2.0, 3.0, best, NAN], kx, ky, mode) == w(best), (mode, shape, 3)
        # +0 and -0 compare equal: the left one stays, in both orders, across a row and across two rows
        for kx, ky in ((2, 1), (1, 2)):
            assert one_block([0.0, -0.0], kx, ky, mode) == 0x00000000
            assert one_block([-0.0, 0.0], kx, ky, mode) == 0x80000000
    # a sequential left-to-right fold would answer differently: fold(max) over (2, 3, NaN, 1) ends at max(NaN, 1) = NaN's pair
    assert one_block([2.0, 3.0, NAN, 1.0], 4, 1, D.MAX) == w(3.0)
    assert one_block([NAN, 2.0, 3.0, 4.0], 4, 1, D.FIRST) == D.NAN_A and one_block([2.0, NAN, NAN, NAN], 2, 2, D.FIRST) == w(2.0)
    # eight in a row: ((l0 l1)(l2 l3))((l4 l5)(l6 l7)); a NaN at l4 takes its half and loses at the root
    assert one_block([1.0, 2.0, 3.0, 4.0, NAN, 9.0, 9.0, 9.0], 8, 1, D.MAX) == w(4.0)
    assert one_block([NAN, 2.0, 3.0, 4.0, 5.0, 9.0, 9.0, 9.0], 8, 1, D.MAX) == D.NAN_A


def test_the_result_is_always_one_of_the_blocks_own_words():
    p = D.depth_pool_plane(64, 64, 3)
    for kx, ky in R.PAIRS:
        blocks = D.words(p).reshape(64 // ky, ky, 64 // kx, kx).transpose(0, 2, 1, 3).reshape(64 // ky, 64 // kx, kx * ky)
        for mode in D.REDUCTIONS:
            r = D.words(D.reduce(p, kx, ky, mode))
            assert (blocks == r[..., None]).any(axis=-1).all(), (kx, ky, mode)
    assert not np.array_equal(D.words(D.reduce(p, 2, 2, D.MAX)), D.words(D.reduce(p, 2, 2, D.MIN)))


# ---- the lookups -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(8, 8), (5, 3), (1, 1), (12, 20)])
def test_the_nearest_lookup_addresses_as_the_colour_sampler_does(size):
    """An index-coded RGBA8 texture through post_texture_cases.numpy_nearest (which a host test holds to the oracle) names the texel."""
    w, h = size
    coded = np.zeros((h, w, 4), dtype=np.uint8)
    coded[..., 0], coded[..., 1] = np.mgrid[0:h, 0:w][1], np.mgrid[0:h, 0:w][0]
    uv = D.lookup_uvs(w, h)
    got = np.rint(X.numpy_nearest(coded, uv) * 255.0).astype(np.int64)
    x, y = D.nearest_xy(w, h, uv)
    assert np.array_equal(x, got[:, 0]) and np.array_equal(y, got[:, 1])
    depth = np.arange(w * h, dtype=F32).reshape(h, w)
    same_words(D.depth_sample(((depth, False), None, None, None), 0, uv), depth[y, x])
    same_words(D.depth_sample(((depth, True), None, None, None), 0, uv), depth[y, x], "the filter does not change the word")


@pytest.mark.parametrize("size", [(8, 8), (5, 3), (2, 1)])
def test_the_bilinear_footprint_is_the_oracles(oracle_lib, size):
    """A texture with R = 255 at exactly one texel samples non-zero, through the oracle's bilinear colour sampler, exactly where that
    texel is in the restated footprint with a non-zero weight."""
    w, h = size
    uv = D.lookup_uvs(w, h, seed=1)
    ix0, ix1, iy0, iy1, fx, fy = D.footprint(w, h, uv)
    one = F32(1.0)
    for tx, ty in ((0, 0), (w - 1, h - 1), (w // 2, h // 2)):
        t = np.zeros((h, w, 4), dtype=np.uint8)
        t[ty, tx, 0] = 255
        lit = X.oracle_sample(t, True, uv)[:, 0] != 0
        weight = np.zeros(len(uv), dtype=np.float64)
        for ix, iy, wx, wy in ((ix0, iy0, one - fx, one - fy), (ix1, iy0, fx, one - fy), (ix0, iy1, one - fx, fy), (ix1, iy1, fx, fy)):
            weight += np.where((ix == tx) & (iy == ty), wx.astype(np.float64) * wy.astype(np.float64), 0.0)
        assert np.array_equal(lit, weight != 0), (size, tx, ty, np.argwhere(lit != (weight != 0))[:4])
        assert lit.any() and not lit.all() or w * h <= 2


def test_shadow_is_exactly_zero_or_one_on_constant_maps_and_within_the_unit_interval_always():
    rng = np.random.default_rng(5)
    uv = np.concatenate([rng.uniform(-2.0, 3.0, (4000, 2)).astype(F32), D.lookup_uvs(8, 4)])
    const = np.full((4, 8), 0.5, dtype=F32)
    for bilinear in (False, True):
        slots = ((const, bilinear), None, None, None)
        assert (D.words(D.shadow(slots, 0, uv, F32(0.5))) == 0x3f800000).all()            # ref >= d: the tie passes
        assert (D.words(D.shadow(slots, 0, uv, np.nextafter(F32(0.5), F32(0.0)))) == 0).all()
        assert (D.words(D.shadow(slots, 0, uv, NAN)) == 0).all()                           # false for NaN
        pool = (D.depth_pool_plane(4, 8, 4), bilinear)
        s = D.shadow((pool, None, None, None), 0, uv, D.lookup_refs(len(uv)))
        assert ((s >= 0) & (s <= 1)).all()
        if bilinear:
            assert ((s > 0) & (s < 1)).any(), "no footprint straddles an edge: the blend is not exercised"
        else:
            assert np.isin(s, (0.0, 1.0)).all()
    # unbound and out of range: lit, and nothing drawn
    for slot in (1, -1, 4):
        assert (D.shadow(slots, slot, uv, F32(-1.0)) == 1).all() and (D.depth_sample(slots, slot, uv) == D.MINVALUE).all()
        assert (D.depth_texel(slots, slot, np.arange(3), np.arange(3)) == D.MINVALUE).all()
    t = np.arange(32, dtype=F32).reshape(4, 8)
    same_words(D.depth_texel(((t, True), None, None, None), 0, np.array([-5, 0, 7, 9]), np.array([2, -1, 4, 3])), [16.0, 0.0, 31.0, 31.0])


# ---- shapes, programs, bindings --------------------------------------------------------------------------------------------------
def test_every_gpu_shape_obeys_the_size_rule():
    for tex_size, factors in D.GPU_SHAPES + D.BLOCKED_SHAPES:
        assert D.size_rule_holds(tex_size, factors, D.source_size(tex_size, factors))
    for (w, h), _ in D.BLOCKED_SHAPES:
        assert w % 4 == 0 and h % 4 == 0
        assert sorted(D.blocked_permutation(w, h).reshape(-1)) == list(range(w * h))


def test_the_four_program_texts_compile():
    lib = N.load()
    log = ctypes.create_string_buffer(1 << 14)
    for name, (vertex, fragment) in D.TEXTS.items():
        if vertex is None:
            rc = lib.swr_program_validate(fragment.encode(), log, len(log))
        else:
            rc = lib.swr_program_validate_vf(vertex.encode(), fragment.encode(), log, len(log))
        assert rc == N.SWR_OK, (name, log.value.decode())
    rc, text = validate(lib, D.POST_PROBE)
    assert rc == N.SWR_OK, text
    # neither contract gains the other's names
    assert lib.swr_program_validate(D.FRAGMENT_PROBE.replace("swr_shadow(", "swr_post_shadow(").encode(), log, len(log)) == N.SWR_ERR_INVALID_ARG
    assert validate(lib, D.POST_PROBE.replace("swr_post_shadow(", "swr_shadow("))[0] == N.SWR_ERR_INVALID_ARG


def test_the_new_names_are_in_all_four_surfaces():
    lib, raw = N.load(), ctypes.CDLL(N.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "swr.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "RasterizerNative.cs")).read()
    hpp = open(os.path.join(ROOT, "softwarerenderer_amd", "cpp", "Rasterizer.hpp")).read()
    for name in ENTRY_POINTS:
        assert name in N.EXPORTS and hasattr(raw, name) and getattr(lib, name).argtypes is not None, name
        assert re.search(r"\bint\s+%s\(" % name, header), name
        assert re.search(r"extern int %s\(IntPtr ctx" % name, cs), name
        assert name + "(" in hpp, name
    assert "#define SWR_ABI_VERSION 3" in header
    assert "SWR_TEXTURE_FORMAT_RGBA8 = 0, SWR_TEXTURE_FORMAT_DEPTH32F = 1" in header
    assert "SWR_DEPTH_REDUCE_MAX = 0, SWR_DEPTH_REDUCE_MIN = 1, SWR_DEPTH_REDUCE_FIRST = 2" in header
    assert (N.SWR_TEXTURE_FORMAT_RGBA8, N.SWR_TEXTURE_FORMAT_DEPTH32F) == (D.RGBA8, D.DEPTH32F) == (0, 1)
    assert (N.SWR_DEPTH_REDUCE_MAX, N.SWR_DEPTH_REDUCE_MIN, N.SWR_DEPTH_REDUCE_FIRST) == D.REDUCTIONS
    from softwarerenderer_amd import DepthReduce, Texture
    assert tuple(int(m) for m in DepthReduce) == D.REDUCTIONS
    for method in ("Depth", "UpdateFromDepth", "ReadDepth", "SampleDepth", "Format"):
        assert hasattr(Texture, method), method
    tex = cs[cs.index("class TextureNative"):]
    for method in ("public static TextureNative CreateDepth(", "public void UpdateFromDepth(", "public float[] ReadDepth("):
        assert method in tex, method
    for method in ("static Texture Depth(", "void UpdateFromDepth(", "ReadDepth()", "SampleDepth(", "int Format()"):
        assert method in hpp, method
    for helper in ("swr_texel_depth", "swr_sample_depth", "swr_shadow", "swr_post_texel_depth", "swr_post_sample_depth", "swr_post_shadow"):
        assert helper in header, helper


# ---- the kernels as compiled -----------------------------------------------------------------------------------------------------
def test_the_kernels_use_no_lds_and_no_scratch():
    """k_depth_to_texture, all 32 instantiations, and k_texture_sample_depth from the compiler's resource remarks."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    csrc = os.path.join(ROOT, "softwarerenderer_amd", "csrc")
    mk = subprocess.run(["make", "-s", "-C", csrc, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in mk if f != "-shared" and not f.startswith("-Wl,")]
    err = subprocess.run([HIPCC] + flags + ["-I" + os.path.join(ROOT, "softwarerenderer_amd", "build"), "-Rpass-analysis=kernel-resource-usage",
                                            "--cuda-device-only", "-c", "swr_api.hip", "-o", os.devnull],
                         cwd=csrc, capture_output=True, text=True, check=True).stderr
    usage, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            usage[cur] = {}
            continue
        m = re.search(r"remark: +(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            usage[cur][m.group(1).split(" ")[0]] = int(m.group(2))
    mine = {k: v for k, v in usage.items() if "k_depth_to_texture" in k}
    assert len(mine) == 32, sorted(mine)
    mine.update({k: v for k, v in usage.items() if "k_texture_sample_depth" in k})
    assert len(mine) == 33
    for k, v in mine.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["LDS"] == 0, (k, v)
