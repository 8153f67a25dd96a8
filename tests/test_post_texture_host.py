"""Post programs with textures, without a GPU (include/swr.h, csrc/swr_post.hip.h): the run-time compile step, the
entry points of the binding and of the C# file, the twins of tests/post_texture_cases.py on hand-computed planes, the wrong twins on
the GPU tests' inputs, and the kernels' resource usage from the compiler's remarks -- the two texel instantiations included."""
import ctypes
import os
import re

import numpy as np
import pytest

import post_cases as P
import post_texture_cases as X
import present8_cases as K
from softwarerenderer_amd import _native as N
from test_post_host import HIPCC, ROOT, _remarks, validate

F32 = np.float32
ENTRY_POINTS = ("swr_post_set_texture", "swr_texture_update_from_post")
INSTANTIATIONS = (0, 3, 4, 16, 17)                # the three present formats; SWR_POST_TEXELS_OPAQUE, SWR_POST_TEXELS_KEEP


@pytest.fixture(scope="module")
def lib():
    return N.load()


@pytest.mark.parametrize("name", sorted(X.TEXTS))
def test_validate_accepts_every_new_program(lib, name):
    rc, log = validate(lib, X.TEXTS[name])
    assert rc == N.SWR_OK, log


@pytest.mark.parametrize("name", sorted(P.TEXTS))
def test_validate_still_accepts_the_programs_without_textures(lib, name):
    rc, log = validate(lib, P.TEXTS[name])
    assert rc == N.SWR_OK, log


def test_the_fragment_contract_does_not_gain_the_helper(lib):
    log = ctypes.create_string_buffer(1 << 14)
    assert lib.swr_program_validate(X.FRAGMENT_WITH_POST_SAMPLE.encode(), log, len(log)) == N.SWR_ERR_INVALID_ARG
    assert b"swr_post_sample" in log.value, log.value
    assert lib.swr_program_validate(X.FRAGMENT_WITH_POST_SAMPLE.replace("swr_post_sample(env, 0, ", "swr_sample(env, ").encode(), log, len(log)) == N.SWR_OK


def test_entry_points_are_exported_bound_and_declared():
    lib = N.load()
    raw = ctypes.CDLL(N.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "swr.h")).read()
    for name in ENTRY_POINTS:
        assert name in N.EXPORTS and hasattr(raw, name) and getattr(lib, name).argtypes is not None, name
        assert re.search(r"\bint\s+%s\(" % name, header), name
    assert len(lib.swr_post_set_texture.argtypes) == 4 and len(lib.swr_texture_update_from_post.argtypes) == 7
    assert "#define SWR_ABI_VERSION 3" in header and "#define SWR_POST_TEXTURES 4" in header
    assert N.SWR_POST_TEXTURES == X.SLOTS == 4
    assert "There are no textures in a post program" not in header
    for helper in ("swr_post_has_texture", "swr_post_sample", "swr_post_texel", "swr_post_texture_size"):
        assert helper in header, helper


def test_the_csharp_file_declares_both_calls():
    cs = open(os.path.join(ROOT, "csharp", "RasterizerNative.cs")).read()
    assert re.search(r"extern int swr_post_set_texture\(IntPtr ctx, int postId, int slot, IntPtr texture\);", cs)
    assert re.search(r"extern int swr_texture_update_from_post\(IntPtr ctx, IntPtr texture, IntPtr sourceCtx, int postId, int kx, int ky, int alphaMode\);", cs)
    post = cs[cs.index("class PostProgramNative"):cs.index("class TextureNative")]
    assert "public void SetTexture(int slot, TextureNative? texture)" in post and "Native.swr_post_set_texture(" in post
    tex = cs[cs.index("class TextureNative"):]
    assert "public void UpdateFromPost(PostProgramNative post" in tex and "Native.swr_texture_update_from_post(" in tex


# ---- the twins on hand-computed 3 x 3 planes, with a 2 x 2 and a 4 x 4 texture ---------------------------------------------------
RES = np.zeros((3, 3, 4), dtype=F32)
T2 = np.arange(16, dtype=np.uint8).reshape(2, 2, 4) * 10 + 5            # texel (x, y): bytes 80 y + 40 x + 5 + (0, 10, 20, 30)
T4 = (np.arange(64, dtype=np.uint8).reshape(4, 4, 4) * 3 + 1).astype(np.uint8)


def unpack(t):
    return t.astype(F32) * X.INV255


def test_sample_wraps_at_negative_uv_and_at_one_and_above():
    # u = (x + 0.5) * 0.5 - 0.75 = -0.5, 0, 0.5: the texel columns 1 (wrapped), 0, 1; v = (y + 0.5) * 0.5 + 0.75 = 1, 1.5, 2: rows 0, 1, 0
    k = P.constants64([0.5, 0.5, -0.75, 0.75, 0])
    assert X.pixel_uv(3, 3, k)[0, :, 0].tolist() == [-0.5, 0.0, 0.5] and X.pixel_uv(3, 3, k)[:, 0, 1].tolist() == [1.0, 1.5, 2.0]
    slots = ((T2, False), None, None, None)
    for sampler in (None, X.numpy_nearest):                            # the oracle, and the restatement the wrong twins vary
        out = X.sample_twin(RES, k, slots, sampler)
        for y, ty in enumerate([0, 1, 0]):
            for x, tx in enumerate([1, 0, 1]):
                assert out[y, x].tolist() == unpack(T2[ty, tx]).tolist(), (sampler, x, y)
    # the wrong twin clamps: u = -0.5 reads column 0, v = 1.5 and 2 read row 1
    wrong = X.sample_twin(RES, k, slots, lambda t, uv: X.numpy_nearest(t, uv, clamp=True))
    assert wrong[0, 0].tolist() == unpack(T2[1, 0]).tolist() and wrong[2, 2].tolist() == unpack(T2[1, 1]).tolist()
    # constants[4]: the channels reversed
    assert X.sample_twin(RES, P.constants64([0.5, 0.5, -0.75, 0.75, 1]), slots)[1, 1].tolist() == unpack(T2[1, 0])[::-1].tolist()


def test_the_multiply_by_the_float_1_over_255_is_not_the_division():
    # 15 * (1f / 255f) and 15 / 255f are different floats (Texture.cs:57-62 multiplies); 126 of the 256 bytes tell the two apart
    assert F32(15) * X.INV255 != F32(15) / F32(255)
    slots = ((T2, False), None, None, None)
    k = P.constants64([0.5, 0.5, -0.75, 0.75, 0])
    right = X.sample_twin(RES, k, slots)
    assert right[0, 1, 1] == F32(15) * X.INV255                        # texel (0, 0), G: byte 15
    assert X.sample_twin(RES, k, slots, lambda t, uv: X.numpy_nearest(t, uv, divide=True))[0, 1, 1] == F32(15) / F32(255)
    assert X.texel_twin(RES, P.constants64([0, 0]), slots)[0, 0, 1] == F32(15) * X.INV255
    assert X.texel_twin(RES, P.constants64([0, 0]), slots, divide=True)[0, 0, 1] == F32(15) / F32(255)


def test_bilinear_known_answer_halfway_between_four_texels():
    # uv = (0.5, 0.5) on 2 x 2: x = 0.5 * 2 - 0.5 = 0.5: halfway between columns 0 and 1, and rows 0 and 1
    t = np.zeros((2, 2, 4), dtype=np.uint8)
    t[0, 0], t[0, 1], t[1, 0], t[1, 1] = 0, 255, 255, 255
    out = X.sample(((t, True), None, None, None), 0, np.array([[0.5, 0.5]], dtype=F32))
    assert out[0].tolist() == [0.75] * 4
    assert X.sample(((t, False), None, None, None), 0, np.array([[0.5, 0.5]], dtype=F32))[0].tolist() == [1.0] * 4      # nearest: texel (1, 1)


def test_texel_clamps_to_the_texture():
    slots = ((T4, False), None, None, None)
    out = X.texel_twin(RES, P.constants64([-2, 2]), slots)             # pixel (x, y) reads texel (x - 2, y + 2)
    assert out[0, 0].tolist() == unpack(T4[2, 0]).tolist()             # x = -2 -> 0
    assert out[2, 2].tolist() == unpack(T4[3, 0]).tolist()             # y = 4 -> 3
    out = X.texel_twin(RES, P.constants64([3, -3]), slots)
    assert out[0, 2].tolist() == unpack(T4[0, 3]).tolist()             # x = 5 -> 3, y = -3 -> 0
    assert out[2, 0].tolist() == unpack(T4[0, 3]).tolist()             # x = 3, y = -1 -> 0


def test_an_unbound_slot_and_slot_4_read_ones_and_measure_nothing():
    k = P.constants64([0.5, 0.5, -0.75, 0.75, 0])
    assert np.array_equal(X.sample_twin(RES, k, X.NO_SLOTS), np.ones((3, 3, 4), dtype=F32))
    assert np.array_equal(X.texel_twin(RES, k, X.NO_SLOTS), np.ones((3, 3, 4), dtype=F32))
    slots = ((T2, False), (T4, False), (T2, False), (T4, False))
    out = X.dynamic_twin(RES, k, slots)
    assert out[2, 2].tolist() == [1.0] * 4 and out[0, 2].tolist() != [1.0] * 4     # (2 + 2) % 5 = 4: no such slot; slot 2 is bound
    assert X.sample(slots, -1, np.zeros((1, 2), dtype=F32)).tolist() == [[1.0] * 4]
    # FOUR with two slots bound: (a / 2 + 1 / 4) + c / 8 + 1 / 16, here with a = c = 0
    zero = np.zeros((2, 2, 4), dtype=np.uint8)
    assert X.four_twin(RES, k, ((zero, False), None, (zero, False), None))[1, 1].tolist() == [0.3125] * 4
    assert X.four_twin(RES, k, (None, (zero, False), None, (zero, False)))[1, 1].tolist() == [0.625] * 4
    # sizes: (w * 256 + h) of slots 0, 1, 3; bits of the bound slots / 64, slot k at bit k + 1
    s = X.sizes_twin(RES, k, ((T2, False), None, None, (np.zeros((3, 5, 4), dtype=np.uint8), True)))
    assert s[1, 2].tolist() == [2 * 256 + 2, 0.0, 5 * 256 + 3, (2 + 16) / 64]


def test_alpha_comes_from_w_through_the_quantiser_with_its_ties():
    w = np.array([K.word(0x3b008081), K.word(0x3efdfdfe), K.ONE_BELOW, np.nan, -0.0, 2.0, 0.5, K.word(0x3bc0c0c1), 1.0], dtype=F32)
    r = np.zeros((3, 3, 4), dtype=F32)
    r[..., 3] = w.reshape(3, 3)
    r[..., 0] = 0.5
    keep = X.texels(r, keep_alpha=True)
    assert keep[..., 3].reshape(-1).tolist() == [0, 126, 255, 0, 0, 255, 128, 2, 255]         # ties to even: 0.5 -> 0, 126.5 -> 126
    assert np.all(X.texels(r)[..., 3] == 255) and np.all(keep[..., 0] == 128) and np.all(keep[..., 1] == 0)
    frame = np.zeros((3, 3, 4), dtype=F32)
    frame[..., 3] = 1.0
    assert np.all(X.texels_alpha_from_frame(r, frame, 1, 1)[..., 3] == 255)


def test_blur_chain_and_accumulation_known_answers():
    c = np.zeros((3, 3, 4), dtype=F32)
    c[1, 1] = 1.0                                                      # one white pixel
    a, t = X.blur_chain(c, 1, 1)
    assert a[1, :, 0].tolist() == [64, 128, 64] and a[0].max() == 0    # (0 + 0 + 1) / 4 = 0.25 -> 63.75 -> 64; 2 / 4 -> 127.5 -> 128
    assert a[1, 1, 3] == 128                                           # alpha kept in the intermediate
    # down the middle column: texels 0, 128, 0 -> (0 + 2 * 128 / 255 + 0) / 4 -> 64; above: (0 + 0 + 128 / 255) / 4 -> 32
    assert t[:, 1, 0].tolist() == [32, 64, 32] and np.all(t[..., 3] == 255)
    # the top row clamps: texel (x, -1) is texel (x, 0)
    col = np.zeros((3, 1, 4), dtype=np.uint8)
    col[0] = 255
    assert X.blur_v_twin(np.zeros((3, 1, 4), dtype=F32), P.constants64(), ((col, False), None, None, None))[:, 0, 0].tolist() == [0.75, 0.25, 0.0]
    # accumulation: 1 -> 128 (0.5 -> 127.5 -> 128); 0 -> half of 128 / 255 -> 64; 0 -> half of 64 / 255 -> 32
    one, zero = np.ones((3, 3, 4), dtype=F32), np.zeros((3, 3, 4), dtype=F32)
    tex = X.accumulate([one, zero, zero])
    assert np.all(tex[1] == 64) and np.all(tex[0] == 32)


# ---- the GPU tests' inputs tell every wrong twin from the right one --------------------------------------------------------------
SIZES_WITH_NEIGHBOURS = [s for s in P.OUT_SIZES if s != (1, 1)]        # one pixel sits at uv (0.5, 0.5) and has no neighbour


@pytest.mark.parametrize("tex_size", [(8, 8), (5, 3)])
def test_the_gpu_inputs_tell_the_wrong_samplers_from_the_right_one(tex_size):
    t = X.texture(tex_size)
    for out_size in SIZES_WITH_NEIGHBOURS:
        k = X.uv_constants(out_size)
        res = np.zeros((out_size[1], out_size[0], 4), dtype=F32)
        uv = X.pixel_uv(out_size[1], out_size[0], k)
        assert uv.min() < -1.5 and uv.max() > 2.5                       # the span the issue asks for
        right = X.sample_twin(res, k, ((t, False), None, None, None))
        assert np.array_equal(right.view(np.uint32), X.numpy_nearest(t, uv).view(np.uint32))        # the restatement is the oracle's
        for what, wrong in (("clamp", dict(clamp=True)), ("divide", dict(divide=True))):
            other = X.sample_twin(res, k, ((t, False), None, None, None), lambda tt, u: X.numpy_nearest(tt, u, **wrong))
            assert not np.array_equal(right.view(np.uint32), other.view(np.uint32)), (what, out_size)
        # the filter read at bind time (nearest then) instead of at the call (bilinear by then)
        at_call = X.sample_twin(res, k, ((t, True), None, None, None))
        assert not np.array_equal(right.view(np.uint32), at_call.view(np.uint32)), ("filter", out_size)
        assert not np.array_equal(X.texel_twin(res, P.constants64([-2, -1]), ((t, False),) + X.NO_SLOTS[1:]).view(np.uint32),
                                  X.texel_twin(res, P.constants64([-2, -1]), ((t, False),) + X.NO_SLOTS[1:], divide=True).view(np.uint32))


def test_the_gpu_inputs_tell_swapped_slots_apart():
    slots = ((X.texture((8, 8)), False), (X.texture((5, 3)), False), (X.texture((1, 1)), False), None)
    for out_size in P.OUT_SIZES:
        k = X.uv_constants(out_size)
        res = np.zeros((out_size[1], out_size[0], 4), dtype=F32)
        assert not np.array_equal(X.four_twin(res, k, slots), X.four_slots_swapped(res, k, slots)), out_size


def test_the_gpu_planes_tell_alpha_from_w_from_alpha_from_the_frame():
    for out_size in SIZES_WITH_NEIGHBOURS:
        for factors in P.FACTORS:
            color, _ = P.planes(out_size, factors, "pool")
            r = X.result("BLUR_H", color, *factors)
            assert not np.array_equal(X.texels(r, keep_alpha=True), X.texels_alpha_from_frame(r, color, *factors)), (out_size, factors)


# ---- resource usage of the kernels, from the compiler's remarks ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(X.TEXTS))
def test_k_post_with_textures_uses_no_lds_no_scratch_and_eight_waves(tmp_path, name):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    inst = "".join(f"template __global__ void swr::k_post<{f}>(const float4*, const float*, void*, uint32_t, uint32_t, int, int, const swr::PostConstants);\n"
                   for f in INSTANTIATIONS)
    usage = _remarks(tmp_path, name, '#include "swr_post.hip.h"\n#line 1 "post.hip"\n' + X.TEXTS[name] + "\n" + inst, ["-DSWR_RTC_POST=1"])
    for f in INSTANTIATIONS:
        v = usage[f"swr::k_post<{f}>"]
        print(name, f, v)
        assert v["LDS"] == 0 and v["ScratchSize"] == 0, (name, f, v)
        assert v["VGPRs"] + v.get("AGPRs", 0) <= 64, (name, f, v)      # eight waves per SIMD, the filter's four taps and a lane-varying slot included


@pytest.mark.parametrize("name", ["IDENTITY", "BOX3"])
def test_the_texel_instantiations_of_programs_without_textures(tmp_path, name):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    inst = "".join(f"template __global__ void swr::k_post<{f}>(const float4*, const float*, void*, uint32_t, uint32_t, int, int, const swr::PostConstants);\n"
                   for f in (16, 17))
    usage = _remarks(tmp_path, name, '#include "swr_post.hip.h"\n#line 1 "post.hip"\n' + P.TEXTS[name] + "\n" + inst, ["-DSWR_RTC_POST=1"])
    for f in (16, 17):
        v = usage[f"swr::k_post<{f}>"]
        assert v["LDS"] == 0 and v["ScratchSize"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 64, (name, f, v)
