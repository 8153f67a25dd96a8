"""Mip chains without a GPU (include/swr.h): the numpy restatements of tests/mipmap_cases.py against hand-written
known answers and independent formulations, the float32 gradient against float64, the program texts through the run-time compile
step, the new names in every binding, and the new kernels' resource usage from the compiler's remarks."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import mipmap_cases as M
import program_probe_cases as PC
from softwarerenderer_amd import _native as N
from test_post_host import HIPCC, ROOT, validate

F32 = np.float32
ENTRY_POINTS = ("swr_texture_generate_mipmaps", "swr_texture_levels", "swr_texture_level_size", "swr_texture_readback_level",
                "swr_texture_sample_lod", "swr_texture_lod")
# The float32 gradient against the float64 evaluation of the same closed form, over the scenes cells, clipped and wide.  Measured, as
# the largest component's error over the largest component of the fragment's gradient: cells 8.3e-7, wide 3.8e-7, clipped 3.04e-5 (the
# clipper's triangles reach the near plane, where N' - u D' cancels).  The bound is four times the largest, for other seeds.
GRAD_MEASURED = 3.04e-5
GRAD_BOUND = 4 * GRAD_MEASURED
# Central differences of the float64 tex_coord with a step of H pixels.  tex_coord = N / D with N and D linear in the pixel, so its
# third derivative is 6 (D' / D)^2 times its first and the truncation error, H^2 / 6 times the third derivative, is H^2 (D' / D)^2
# relative to the gradient; the rounding error of the difference is taken as 64 ulp(max(|uv|, 1)) / (2 H) -- tex_coord_at is some
# thirty float64 operations, and its barycentrics cancel positions of up to 144 pixels.  Both are computed per fragment (the scenes'
# largest D' / D is 8.5 per pixel, in `clipped`) and doubled: with H = 1e-4 that is below 2e-6 everywhere.
FD_STEP = 1e-4


# ---- the downsample --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,want", M.KNOWN_BLOCKS)
def test_known_answers_pin_the_rounding(block, want):
    for order in (block, block[::-1], block[1:] + block[:1]):
        t = np.zeros((2, 2, 4), dtype=np.uint8)
        t[..., 2] = np.array(order, dtype=np.uint8).reshape(2, 2)
        out = M.downsample(t)
        assert out.shape == (1, 1, 4) and out[0, 0, 2] == want and (out[0, 0, [0, 1, 3]] == 0).all()


def test_a_constant_texture_is_constant_at_every_level():
    for w, h in M.SHAPES:
        for value in (0, 1, 127, 254, 255):
            t = np.full((h, w, 4), value, dtype=np.uint8)
            t[..., 1] = 255 - value
            for l, level in enumerate(M.chain(t)):
                assert (level[..., 0] == value).all() and (level[..., 1] == 255 - value).all(), (w, h, value, l)


def test_level_sizes_and_offsets_of_every_shape():
    want = {(1, 1): [(1, 1)], (2, 2): [(2, 2), (1, 1)], (5, 7): [(5, 7), (2, 3), (1, 1)],
            (12, 20): [(12, 20), (6, 10), (3, 5), (1, 2), (1, 1)], (1, 16): [(1, 16), (1, 8), (1, 4), (1, 2), (1, 1)],
            (16, 1): [(16, 1), (8, 1), (4, 1), (2, 1), (1, 1)], (33, 17): [(33, 17), (16, 8), (8, 4), (4, 2), (2, 1), (1, 1)],
            (64, 64): [(64 >> l, 64 >> l) for l in range(7)], (68, 8): [(68, 8), (34, 4), (17, 2), (8, 1), (4, 1), (2, 1), (1, 1)]}
    assert sorted(want) == sorted(M.SHAPES)
    for (w, h), sizes in want.items():
        L = M.full_levels(w, h)
        assert L == len(sizes) == 1 + int(math.floor(math.log2(max(w, h)))) <= M.MAX_LEVELS
        assert [M.level_size(w, h, l) for l in range(L)] == sizes
        off = M.offsets(w, h)
        assert off[0] == 0 and off[1:] == [sum(a * b for a, b in sizes[1:l]) for l in range(1, L)]
        levels = M.chain(M.texture((w, h)))
        assert [(t.shape[1], t.shape[0]) for t in levels] == sizes
        if (w, h) != (1, 1):
            assert L >= 2                          # (no test may skip a case "because levels is 1")


def test_a_one_wide_texture_averages_pairs_with_the_duplicated_tap():
    t = M.texture((1, 16))
    a = t[:, 0, :].astype(np.int64)
    want = (2 * a[0::2] + 2 * a[1::2] + 2) >> 2
    assert np.array_equal(M.downsample(t)[:, 0, :], want)
    t = M.texture((16, 1))
    a = t[0].astype(np.int64)
    assert np.array_equal(M.downsample(t)[0], (2 * a[0::2] + 2 * a[1::2] + 2) >> 2)


def test_an_odd_side_drops_its_last_column_or_row():
    t = M.texture((5, 7)).copy()
    before = M.downsample(t)
    t[:, 4] ^= 0xff
    t[6, :] ^= 0xff
    assert np.array_equal(M.downsample(t), before)
    t[0, 0] ^= 0xff
    assert not np.array_equal(M.downsample(t), before)


def test_the_planted_blocks_are_in_the_textures_and_round_as_written():
    t = M.texture((64, 64))
    lvl1 = M.downsample(t)
    for i, (block, want) in enumerate(M.KNOWN_BLOCKS):
        assert tuple(t[2 * i:2 * i + 2, 2 * i:2 * i + 2, 0].reshape(-1)) == block
        assert (lvl1[i, i] == want).all(), (block, lvl1[i, i])
    assert (M.chain(M.checkerboard(64))[-1] == (128, 128, 128, 255)).all()


# ---- the lod ---------------------------------------------------------------------------------------------------------------------
def lod_of_rho(rho, levels=40):
    """through the restatement with w = h = 1: rho = |dudx|"""
    g = np.zeros(np.shape(rho) + (4,), dtype=F32)
    g[..., 0] = rho
    return M.lod(1, 1, g, levels)


def test_lod_is_the_integer_at_powers_of_two():
    k = np.arange(0, 39)
    assert np.array_equal(lod_of_rho(np.exp2(k).astype(F32)), k.astype(F32))


def test_lod_is_within_the_stated_band_of_log2_and_monotone():
    rho = np.unique(np.concatenate([np.geomspace(1.0, 2.0 ** 30, 20001), 1.0 + np.geomspace(1e-7, 1.0, 500)]).astype(F32))
    got = lod_of_rho(rho).astype(np.float64)
    ref = np.log2(rho.astype(np.float64))
    assert (got <= ref + 1e-12).all() and (got >= ref - 0.0861).all()
    assert (ref - got).max() > 0.086                      # (the band is tight: the maximum is at m = 1 / ln 2)
    assert (np.diff(got) >= 0).all()


def test_lod_is_zero_at_or_below_one_and_for_every_nan_position():
    small = np.array([0.0, -0.0, 1e-45, 1e-38, 0.5, np.nextafter(F32(1.0), F32(0.0)), 1.0, -1.0], dtype=F32)
    assert (lod_of_rho(small).view(np.uint32) == 0).all()
    nan = float("nan")
    for pos in range(4):
        g = np.array([8.0, 8.0, 8.0, 8.0], dtype=F32)
        g[pos] = nan
        assert M.lod(4, 4, g, 5).view(np.uint32) == 0, pos
    assert M.lod(4, 4, np.array([3e38, 3e38, 0, 0], dtype=F32), 3) == 2.0          # overflow to +Inf: the top level
    assert M.lod(4, 4, np.array([8.0, 0, 0, 0], dtype=F32), 0) == 0.0              # an unbound slot
    for w, h, L in ((12, 20, 5), (68, 8, 7)):
        got = M.lod(w, h, M.gradient_ladder(w, h, L), L)
        assert ((got >= 0) & (got <= L - 1)).all() and (got == L - 1).any() and (got == 0).any() and ((got > 0) & (got < 1)).any()


def test_sample_lod_meets_its_definition_at_the_ends():
    t = M.texture((12, 20))
    levels = M.chain(t)
    uv = M.lookup_uvs(12, 20)
    for filtered in (False, True):
        lvl = lambda l: M.sample_level(levels, filtered, l, uv)
        same = lambda a, b: np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))
        assert same(M.sample_lod(levels, filtered, uv, F32("nan")), lvl(0)) and same(M.sample_lod(levels, filtered, uv, F32(-1)), lvl(0))
        assert same(M.sample_lod(levels, filtered, uv, F32(2.0)), lvl(2))
        assert same(M.sample_lod(levels, filtered, uv, F32("inf")), lvl(4)) and same(M.sample_lod(levels, filtered, uv, F32(5)), lvl(4))
        mid = M.sample_lod(levels, filtered, uv, F32(1.5))
        lo, hi = np.minimum(lvl(1), lvl(2)), np.maximum(lvl(1), lvl(2))
        assert ((mid >= lo - 1e-6) & (mid <= hi + 1e-6)).all() and not same(mid, lvl(1))
        # without a chain every lod is level 0
        assert same(M.sample_lod(levels, filtered, uv, F32(3.0), have=1), lvl(0))
    assert (M.sample_lod(None, False, uv, F32(1.0)) == 1).all()


# ---- the gradient ----------------------------------------------------------------------------------------------------------------
SCENES = {"cells": PC.cells, "clipped": PC.clipped, "wide": PC.wide}


def relative_error(got, ref):
    """per fragment: the largest component's error over the largest component of the reference"""
    scale = np.abs(ref).max(axis=1)
    return np.where(scale > 0, np.abs(got.astype(np.float64) - ref).max(axis=1) / np.where(scale > 0, scale, 1.0), 0.0)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_float32_gradient_meets_float64(name):
    scene = SCENES[name]()
    worst, worst_fd, n, h = 0.0, 0.0, 0, FD_STEP
    for t in PC.probe_tris(scene):
        for rect in t.rects():
            g32, g64 = M.tex_coord_grad(t, rect), M.tex_coord_grad(t, rect, np.float64)
            assert g32.dtype == F32 and g32.shape == g64.shape and g32.shape[1] == 4
            worst = max(worst, float(relative_error(g32, g64).max(initial=0.0)))
            # central differences of the float64 tex_coord at the covered pixels
            with np.errstate(all="ignore"):
                inside = t.tri.cover(rect)[0]
            sX, eX, sY, eY = rect
            xs, ys = np.meshgrid(np.arange(sX, eX + 1, dtype=np.float64), np.arange(sY, eY + 1, dtype=np.float64))
            x, y = xs[inside], ys[inside]
            ddx = (M.tex_coord_at(t, x + h, y) - M.tex_coord_at(t, x - h, y)) / (2 * h)
            ddy = (M.tex_coord_at(t, x, y + h) - M.tex_coord_at(t, x, y - h)) / (2 * h)
            fd = np.stack([ddx[:, 0], ddx[:, 1], ddy[:, 0], ddy[:, 1]], axis=1)
            at = M.tex_coord_at(t, x, y)
            scale = np.abs(g64).max(axis=1)
            allowed = 2 * ((h * M.depth_slope(t, rect)) ** 2 + 64 * np.spacing(np.maximum(np.abs(at).max(axis=1), 1.0)) / (2 * h) / np.where(scale > 0, scale, 1.0))
            err = relative_error(fd, g64)
            assert (err <= allowed).all(), (name, t.index, float(err.max()), float(allowed.min()))
            assert allowed.max() < 2e-6
            worst_fd = max(worst_fd, float(err.max(initial=0.0)))
            # tex_coord_at is the function fs_in_reference interpolates
            r = PC.fs_in_reference(scene, t.draw, t, rect)
            assert np.allclose(at[:, 0], r["tex_coord.x"], rtol=0, atol=2e-4) and np.allclose(at[:, 1], r["tex_coord.y"], rtol=0, atol=2e-4)
            n += len(x)
    print(f"{name}: {n} fragments, float32 against float64 {worst:.3e} (bound {GRAD_BOUND:.3e}), float64 against central differences {worst_fd:.3e}")
    assert n > 0 and worst <= GRAD_BOUND


# ---- programs, bindings ----------------------------------------------------------------------------------------------------------
def test_every_program_text_compiles_and_the_contracts_stay_apart():
    lib = N.load()
    log = ctypes.create_string_buffer(1 << 14)
    for name, text in M.FRAGMENT_TEXTS.items():
        assert lib.swr_program_validate(text.encode(), log, len(log)) == N.SWR_OK, (name, log.value.decode())
    assert lib.swr_program_validate_vf(M.VERTEX_PROBE.encode(), PC.PROBE_ALL.encode(), log, len(log)) == N.SWR_OK, log.value.decode()
    for name, text in M.POST_TEXTS.items():
        rc, msg = validate(lib, text)
        assert rc == N.SWR_OK, (name, msg)
    # the post contract does not gain tex_coord_grad, the fragment contract does not gain the swr_post_* names
    assert validate(lib, M.POST_PROBE.replace("env.constants[7]", "in.tex_coord_grad.x"))[0] == N.SWR_ERR_INVALID_ARG
    assert lib.swr_program_validate(M.LOD_CONSTANT.replace("swr_sample_lod(", "swr_post_sample_lod(").encode(), log, len(log)) == N.SWR_ERR_INVALID_ARG


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
    from softwarerenderer_amd import Texture
    for method in ("GenerateMipmaps", "Levels", "LevelSize", "ReadLevel", "SampleLod", "Lod"):
        assert hasattr(Texture, method), method
    tex = cs[cs.index("class TextureNative"):]
    for method in ("public void GenerateMipmaps(", "public int Levels", "public byte[] ReadLevel("):
        assert method in tex, method
    for method in ("void GenerateMipmaps(", "int Levels()", "LevelSize(", "ReadLevel(", "SampleLod(", "float Lod("):
        assert method in hpp, method
    for helper in ("swr_sample_level", "swr_sample_lod", "swr_lod", "swr_sample_grad", "tex_coord_grad", "swr_post_texture_levels",
                   "swr_post_sample_level", "swr_post_sample_lod", "swr_post_lod"):
        assert helper in header, helper
    # the pins the header's layout answers to
    device = open(os.path.join(ROOT, "softwarerenderer_amd", "csrc", "swr_device.h")).read()
    assert "struct TextureSlot { const uint8_t* texels; int w, h; };" in device and "sizeof(TextureHeader) == 144" in device


# ---- the kernels as compiled -----------------------------------------------------------------------------------------------------
def test_the_kernels_use_no_lds_and_no_scratch():
    """k_mip_downsample's two instantiations, the two batch kernels and the header's launch from the compiler's resource remarks."""
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
    mine = {k: v for k, v in usage.items() if "k_mip_downsample" in k}
    assert len(mine) == 2, sorted(mine)
    for other in ("k_texture_sample_lod", "k_texture_lod", "k_texture_header"):
        found = {k: v for k, v in usage.items() if other in k}
        assert len(found) == 1, (other, sorted(found))
        mine.update(found)
    for k, v in mine.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["LDS"] == 0, (k, v)
