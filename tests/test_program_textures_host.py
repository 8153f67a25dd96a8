"""User programs with texture slots, without a GPU: the contract compiles (swr_program_validate needs neither a context nor a device),
the three mirrors declare the entry point, the header states the rules, and the twins of tests/program_texture_cases.py tell right
from wrong on the inputs the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest

import program_texture_cases as T
from softwarerenderer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return N.load()


def validate(lib, fragment, vertex=None):
    log = ctypes.create_string_buffer(1 << 16)
    if vertex is None:
        rc = lib.swr_program_validate(fragment.encode(), log, len(log))
    else:
        rc = lib.swr_program_validate_vf(vertex.encode(), fragment.encode(), log, len(log))
    return rc, log.value.decode(errors="replace")


@pytest.mark.parametrize("name", list(T.ONE_HELPER))
def test_each_slot_helper_compiles_in_each_half(lib, name):
    vertex, fragment = T.ONE_HELPER[name]
    rc, log = validate(lib, fragment, vertex)
    assert rc == N.SWR_OK, log


@pytest.mark.parametrize("name", ["FOUR", "PROBE", "PLAIN", "LIGHTMAP"])
def test_the_gpu_tests_fragment_texts_compile(lib, name):
    rc, log = validate(lib, T.TEXTS[name])
    assert rc == N.SWR_OK, log


def test_the_gpu_tests_vertex_text_compiles(lib):
    import program_probe_cases as PC
    rc, log = validate(lib, PC.PROBE_ALL, T.VERTEX)
    assert rc == N.SWR_OK, log


def test_a_slot_is_an_int_not_a_texture(lib):
    """The helpers take the env and a slot number; there is no way to name a texture's memory."""
    rc, log = validate(lib, T.HEAD + "    return swr_sample(env, env.tex, in.tex_coord);\n}\n")
    assert rc == N.SWR_ERR_INVALID_ARG and "fragment.hip:" in log, log


def test_the_one_argument_helpers_stay(lib):
    rc, log = validate(lib, T.HEAD + "    return swr_has_texture(env) ? swr_sample(env, in.tex_coord) : swr_sample(env, 0, in.tex_coord);\n}\n")
    assert rc == N.SWR_OK, log


def test_entry_point_is_declared_by_header_ctypes_cpp_and_csharp(lib):
    header = open(os.path.join(ROOT, "include", "swr.h")).read()
    assert "#define SWR_ABI_VERSION 3" in header and "#define SWR_PROGRAM_TEXTURES 4" in header
    assert re.search(r"int\s+swr_program_set_texture\(swr_context\* ctx, int program_id, int slot, const swr_texture\* tex", header)
    assert N.SWR_PROGRAM_TEXTURES == T.SLOTS == 4
    assert "swr_program_set_texture" in N.EXPORTS and hasattr(lib, "swr_program_set_texture")
    cs = open(os.path.join(ROOT, "csharp", "RasterizerNative.cs")).read()
    assert "swr_program_set_texture(IntPtr ctx, int programId, int slot, IntPtr texture)" in cs
    assert "public static void SetTexture(Shaders.FragmentShader method, int slot, TextureNative? texture)" in cs
    hpp = open(os.path.join(ROOT, "softwarerenderer_amd", "cpp", "Rasterizer.hpp")).read()
    assert "SetProgramTexture(int id, int slot, const Texture* texture)" in hpp and "textures[SWR_PROGRAM_TEXTURES - 1]" in hpp


def test_header_states_capture_order_and_errors():
    header = open(os.path.join(ROOT, "include", "swr.h")).read()
    text = " ".join(header.split())
    for phrase in ("when it is RECORDED", "later swr_program_set_texture and swr_texture_set_filter calls do not change recorded draws",
                   "sample the old texels", "a slot outside 1 .. 3", "an id below SWR_PROG_USER_BASE"):
        assert phrase in text.replace("* ", ""), phrase


def test_the_user_block_is_76_words_with_one_definition_of_its_stride():
    csrc = os.path.join(ROOT, "softwarerenderer_amd", "csrc")
    dev = open(os.path.join(csrc, "swr_device.h")).read()
    assert "#define SWR_USER_BLOCK_WORDS (SWR_USER_CONSTANTS + 4 * (SWR_PROGRAM_TEXTURES - 1))" in dev and "#define SWR_USER_CONSTANTS 64" in dev
    assert "struct TextureSlot { const uint8_t* texels; int w, h; };" in dev
    # the stride's three users go through it
    assert "SWR_USER_BLOCK_WORDS * draw" in open(os.path.join(csrc, "swr_raster_c.hip.h")).read()
    assert "SWR_USER_BLOCK_WORDS * bm.draw" in open(os.path.join(csrc, "swr_geometry.hip.h")).read()
    flush = open(os.path.join(csrc, "swr_flush.h")).read()
    assert "nd * sizeof(UserBlock)" in flush and "64u * " not in flush
    for f in ("swr_raster_c.hip.h", "swr_geometry.hip.h"):
        assert not re.search(r"user_consts \+ 64u", open(os.path.join(csrc, f)).read()), f
    # one home for the descriptor: the post prelude no longer has a type of its own
    assert "struct PostTexture" not in open(os.path.join(csrc, "swr_post.hip.h")).read()


def test_python_mirror_takes_three_textures():
    from softwarerenderer_amd.rasterizer import CustomProgram, Shaders
    p = Shaders.Custom(T.PLAIN, textures=(None, None))
    assert isinstance(p, CustomProgram) and p.textures == (None, None)
    with pytest.raises(ValueError):
        CustomProgram(T.PLAIN, textures=(None,) * 4)


# ---- the twins tell right from wrong on the GPU tests' inputs
def _pixels(W=144, H=80):
    ys, xs = np.mgrid[0:H, 0:W]
    return xs.reshape(-1), ys.reshape(-1)


@pytest.mark.parametrize("bilinear", [False, True])
def test_four_slots_twin_differs_from_all_slot0_and_from_a_swap(bilinear):
    xs, ys = _pixels()
    slots = T.slots_of(("12x20", "8x8", "5x3", "1x1"), bilinear)
    k = T.constants(144, 80)
    right = T.four_twin(k, slots, xs, ys)
    assert (right.view(np.uint32) != T.four_all_slot0(k, slots, xs, ys).view(np.uint32)).any()
    swapped = (slots[0], slots[2], slots[1], slots[3])
    assert (right.view(np.uint32) != T.four_twin(k, swapped, xs, ys).view(np.uint32)).any()
    assert len(np.unique(right[:, 0])) > 50          # many different texels


def test_probe_twin_unbound_and_out_of_range_slots_read_ones_and_measure_zero():
    xs, ys = _pixels(32, 16)
    slots = T.slots_of(("12x20", None, "5x3", None))
    for slot in (1, 3, -1, 4, 1000):
        for mode in (T.SAMPLE, T.TEXEL):
            assert (T.probe_twin(T.constants(32, 16, mode=mode, slot=slot), slots, xs, ys) == 1.0).all()
        assert (T.probe_twin(T.constants(32, 16, mode=T.SIZE, slot=slot), slots, xs, ys) == 0.0).all()
    sz = T.probe_twin(T.constants(32, 16, mode=T.SIZE, slot=2), slots, xs, ys)
    assert (sz == np.array([5, 3, 1, 5 * 256 + 3], dtype=F32)).all()
    # the per-pixel slot visits all five, the unbound ones among them
    dyn = T.probe_twin(T.constants(32, 16, slot=T.PER_PIXEL), slots, xs, ys)
    assert ((dyn == 1.0).all(axis=1) == np.isin((xs + ys) % 5, (1, 3, 4))).all()


def test_texel_walk_reaches_both_sides_of_the_clamp():
    k = T.constants(144, 80, mode=T.TEXEL, texel_span=(16, 24))
    xs, ys = _pixels()
    tx, ty = xs % int(k[4]) - 2, ys % int(k[5]) - 2
    assert (tx.min(), tx.max(), ty.min(), ty.max()) == (-2, 13, -2, 21)          # 12 x 20: -2 .. w + 1, -2 .. h + 1
