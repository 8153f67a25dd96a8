"""Post-process programs without a GPU (include/swr.h, csrc/swr_post.hip.h): the run-time compile step alone
(swr_post_validate needs neither a context nor a device), the entry points and constants of the binding, the twins of
tests/post_cases.py on hand-computed planes, the wrong twins on the GPU tests' planes, and the kernels' resource usage from the
compiler's remarks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import post_cases as P
from softwarerenderer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softwarerenderer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
F32 = np.float32

ENTRY_POINTS = ("swr_post_create", "swr_post_destroy", "swr_post_set_constants", "swr_post_validate", "swr_post_size",
                "swr_readback_post", "swr_present_post_async", "swr_post_device", "swr_post_device_async")


@pytest.fixture(scope="module")
def lib():
    return N.load()


def validate(lib, src, size=1 << 16):
    log = ctypes.create_string_buffer(size)
    rc = lib.swr_post_validate(src.encode(), log, len(log))
    return rc, log.value.decode(errors="replace")


@pytest.mark.parametrize("name", sorted(P.TEXTS) + ["TINT_LERP"])
def test_validate_accepts_every_test_program(lib, name):
    rc, log = validate(lib, P.TINT_LERP if name == "TINT_LERP" else P.TEXTS[name])
    assert rc == N.SWR_OK, log


def test_validate_rejects_a_syntax_error_with_the_callers_line(lib):
    rc, log = validate(lib, P.SYNTAX_ERROR)
    assert rc == N.SWR_ERR_INVALID_ARG
    assert f"post.hip:{P.SYNTAX_ERROR_LINE}:" in log, log


def test_validate_rejects_a_text_without_swr_post(lib):
    rc, log = validate(lib, P.NO_ENTRY)
    assert rc == N.SWR_ERR_INVALID_ARG
    assert "swr_post" in log, log


def test_validate_truncates_the_log_to_the_buffer(lib):
    buf = ctypes.create_string_buffer(b"\xa5" * 32, 32)
    assert lib.swr_post_validate(b"float4 swr_post( this is not C++", buf, 16) == N.SWR_ERR_INVALID_ARG
    assert 0 < len(buf.value) <= 15
    assert buf.raw[16:] == b"\xa5" * 16                               # nothing past the 16 bytes it was given
    assert lib.swr_post_validate(None, buf, 16) == N.SWR_ERR_INVALID_ARG
    assert lib.swr_post_validate(P.IDENTITY.encode(), None, 0) == N.SWR_OK


def test_a_text_is_compiled_against_the_contract_of_the_entry_it_was_handed_to(lib):
    """A post program sees the post contract alone (no swr_fs_in), a fragment program the fragment contract alone (no swr_post_in)."""
    fragment = "__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) { return in.color; }\n"
    both = "#ifdef SWR_RTC_POST\n" + P.IDENTITY + "#else\n" + fragment + "#endif\n"
    log = ctypes.create_string_buffer(1 << 14)
    assert lib.swr_post_validate(both.encode(), log, len(log)) == N.SWR_OK, log.value
    assert lib.swr_program_validate(both.encode(), log, len(log)) == N.SWR_OK, log.value
    assert lib.swr_post_validate((fragment + P.IDENTITY).encode(), log, len(log)) == N.SWR_ERR_INVALID_ARG and b"swr_fs_in" in log.value
    assert lib.swr_program_validate((P.IDENTITY + fragment).encode(), log, len(log)) == N.SWR_ERR_INVALID_ARG and b"swr_post_in" in log.value


def test_entry_points_are_exported_and_bound(lib):
    raw = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in N.EXPORTS and hasattr(raw, name) and getattr(lib, name).argtypes is not None, name
    header = open(os.path.join(ROOT, "include", "swr.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\(" % name, header), name


def test_enum_values():
    header = open(os.path.join(ROOT, "include", "swr.h")).read()
    for name, value in (("SWR_POST_RGB32F", 0), ("SWR_POST_RGB8", 3), ("SWR_POST_RGBX8", 4)):
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
        assert getattr(N, name) == value
    assert (P.RGB32F, P.RGB8, P.RGBX8) == (N.SWR_POST_RGB32F, N.SWR_POST_RGB8, N.SWR_POST_RGBX8)
    assert "#define SWR_ABI_VERSION 3" in header


# ---- the twins on hand-computed 3 x 3 planes -------------------------------------------------------------------------------------
def plane3(values, alpha=7.0):
    """(3, 3, 4): `values` in R, twice that in G, minus that in B."""
    v = np.asarray(values, dtype=F32).reshape(3, 3)
    return np.stack([v, v * F32(2), -v, np.full((3, 3), alpha, dtype=F32)], axis=-1)


ZERO_DEPTH = np.zeros((3, 3), dtype=F32)
K0 = P.constants64()


def test_identity_and_resolve_rgba_known_answers():
    p = plane3(np.arange(9))
    res = P.resolve_rgba(p, 1, 1)
    assert np.array_equal(res, p)
    assert np.array_equal(P.identity(res, ZERO_DEPTH, 1, 1, K0), p[..., :3])
    # a 2 x 2 block of 1, 2, 3, 4 (alpha 8, 8, 8, 0) averages to 2.5 (alpha 6)
    blk = np.zeros((2, 2, 4), dtype=F32)
    blk[..., :3] = np.array([[1, 2], [3, 4]], dtype=F32)[..., None]
    blk[..., 3] = [[8, 8], [8, 0]]
    assert P.resolve_rgba(blk, 2, 2).tolist() == [[[2.5, 2.5, 2.5, 6.0]]]


def test_tint_rounds_the_product_before_the_sum():
    # c * k = (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11; minus (1 + 2^-11) leaves 0 -- fused, the 2^-24 survives
    c = F32(1.0 + 2.0 ** -12)
    k = P.constants64([c, 1, 1, -(1.0 + 2.0 ** -11), 0, 0])
    p = plane3(np.full(9, c))
    assert P.tint(p, ZERO_DEPTH, 1, 1, k)[0, 0, 0] == 0.0
    assert P.tint_fused(p, ZERO_DEPTH, 1, 1, k)[0, 0, 0] == F32(2.0 ** -24)
    # and the plain case: 2 * 0.5 + 0.25
    assert P.tint(plane3(np.full(9, 2.0)), ZERO_DEPTH, 1, 1, P.constants64([0.5, 0, 0, 0.25, 0, 0]))[1, 1].tolist() == [1.25, 0.0, 0.0]


def test_tint_lerp_twins_known_answers():
    # lerp(b, k, c) with c = 0.25: b * 0.75 + k * 0.25
    k = P.constants64([8, 0, 0, 4, 0, 0])
    p = plane3(np.full(9, 0.25))
    assert P.tint_lerp(p, ZERO_DEPTH, 1, 1, k)[0, 0, 0] == 5.0 and P.tint_lerp_fused(p, ZERO_DEPTH, 1, 1, k)[0, 0, 0] == 5.0
    # b * (1 - c) = (1 + 2^-12)(1 + 2^-12) again, y = k * c = -(1 + 2^-11): unfused 0, fused 2^-24
    c = F32(-(2.0 ** -12))
    a = F32(1.0 + 2.0 ** -12)
    k = P.constants64([F32(1.0 + 2.0 ** -11) / (-c), 0, 0, a, 0, 0])
    assert k[0] * c == F32(-(1.0 + 2.0 ** -11))
    p = plane3(np.full(9, c))
    assert P.tint_lerp(p, ZERO_DEPTH, 1, 1, k)[0, 0, 0] == 0.0
    assert P.tint_lerp_fused(p, ZERO_DEPTH, 1, 1, k)[0, 0, 0] == F32(2.0 ** -24)


def test_coords_known_answers():
    res = np.zeros((3, 3, 4), dtype=F32)
    out = P.coords(res, ZERO_DEPTH, 4, 2, K0)
    assert out[2, 1].tolist() == [float(F32(1) / F32(3)), float(F32(2) / F32(3)), (4 * 16 + 2) / 128 + 7.0]
    assert out[0, 0].tolist() == [0.0, 0.0, 66 / 128]


def test_box3_known_answers_clamp_and_order():
    ninth = F32(1.0) / F32(9.0)
    p = plane3(np.arange(1, 10))                                       # 1 2 3 / 4 5 6 / 7 8 9
    out = P.box3(p, ZERO_DEPTH, 1, 1, K0)
    assert out[1, 1, 0] == F32(45) * ninth                             # the centre sees all nine
    assert out[0, 0, 0] == F32(1 + 1 + 2 + 1 + 1 + 2 + 4 + 4 + 5) * ninth       # the corner: clamped taps repeat the edge
    assert P.box3_wrap(p, ZERO_DEPTH, 1, 1, K0)[0, 0, 0] == F32(45) * ninth     # wrapped, every pixel sees all nine
    # order: the row-major running sum loses the 1 behind 1e8 (1e8 + 1 == 1e8 in float32), the column-major one cancels first
    q = plane3([1e8, 1.0, 0.0, -1e8, 0.0, 0.0, 0.0, 0.0, 0.0])
    assert P.box3(q, ZERO_DEPTH, 1, 1, K0)[1, 1, 0] == 0.0
    assert P.box3_column_first(q, ZERO_DEPTH, 1, 1, K0)[1, 1, 0] == ninth


def test_edge_known_answers_first_sample_and_clamp():
    d = np.arange(36, dtype=F32).reshape(6, 6)                         # 3 x 3 output pixels of 2 x 2 samples
    res = np.zeros((3, 3, 4), dtype=F32)
    out = P.edge(res, d, 2, 2, K0)
    assert out[0, 0].tolist() == [-2.0, -12.0, 0.0]                    # d[0, 0] - d[0, 2], d[0, 0] - d[2, 0], d[0, 0]
    assert out[2, 2].tolist() == [0.0, 0.0, 28.0]                      # the last pixel's neighbours are itself: d[4, 4]
    assert P.edge_last_sample(res, d, 2, 2, K0)[0, 0].tolist() == [-2.0, -12.0, 7.0]      # d[1, 1]
    cleared = np.full((3, 3), np.finfo(F32).min, dtype=F32)
    assert P.edge(res, cleared, 1, 1, K0)[1, 1].tolist() == [0.0, 0.0, float(np.finfo(F32).min)]


def test_specials_known_answers():
    res = plane3(np.arange(9))
    out = P.specials(res, ZERO_DEPTH, 1, 1, K0)
    w = np.array(P.SPECIAL_WORDS, dtype=np.uint32).view(F32)
    assert np.isnan(out[0, 0, 0]) and out[0, 0, 1] == w[3] and np.signbit(out[0, 0, 1]) and out[0, 0, 2] == w[5]
    assert out[0, 1, 0] == np.inf and out[0, 2, 0] == -np.inf
    assert out[2, 2].tolist() == res[2, 2, :3].tolist()                # pixel 8 keeps its colour
    q = P.deliver(out, P.RGBX8)
    assert q[0, 0].tolist() == [0, 0, 0, 255] and q[0, 1, 0] == 255 and q[2, 0, 0] == 126        # NaN, -0, a tie; +Inf; the other tie
    assert q[2, 1, 0] == 255                                           # nextafter(1, 0) * 255 rounds up


@pytest.mark.parametrize("which", sorted(P.WRONG_TWINS))
def test_the_gpu_planes_tell_every_wrong_twin_from_the_right_one(which):
    """On every plane the GPU test compares a program on (two pixels or more), the wrong twin gives other words than the right one:
    a plane that could not tell them apart would let the kernel pass with the wrong arithmetic."""
    name, wrong = P.WRONG_TWINS[which]
    for out_size in P.OUT_SIZES:
        for factors in P.FACTORS:
            if out_size == (1, 1) or (which == "EDGE last sample" and factors == (1, 1)):
                continue                                               # one pixel has no neighbours; a block of one sample has no last
            color, depth = P.planes(out_size, factors, P.plane_kind(name))
            right = P.expected(name, color, depth, *factors)
            other = P.expected(name, color, depth, *factors, twin=wrong)
            same = (right.view(np.uint32) == other.view(np.uint32)) | (np.isnan(right) & np.isnan(other))
            assert not same.all(), (which, out_size, factors)


# ---- resource usage of the kernels, from the compiler's remarks ------------------------------------------------------------------
def _remarks(tmp_path, name, source, defines=()):
    mk = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    flags = [f for f in mk if f != "-shared" and not f.startswith("-Wl,")]
    src = tmp_path / (name + ".hip")
    src.write_text(source)
    err = subprocess.run([HIPCC] + flags + list(defines) + ["-I" + CSRC, "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / (name + ".o"))],
                         capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().replace("void ", "")
            cur = re.sub(r"\(.*", "", cur)
            out[cur] = {}
            continue
        m = re.search(r"remark: +(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            out[cur][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


@pytest.mark.parametrize("name", ["IDENTITY", "BOX3"])
def test_k_post_uses_no_lds_and_no_scratch(tmp_path, name):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    inst = "".join(f"template __global__ void swr::k_post<{f}>(const float4*, const float*, void*, uint32_t, uint32_t, int, int, const swr::PostConstants);\n"
                   for f in P.FORMATS)
    usage = _remarks(tmp_path, name, '#include "swr_post.hip.h"\n#line 1 "post.hip"\n' + P.TEXTS[name] + "\n" + inst, ["-DSWR_RTC_POST=1"])
    for f in P.FORMATS:
        v = usage[f"swr::k_post<{f}>"]
        assert v["LDS"] == 0 and v["ScratchSize"] == 0, (name, f, v)
        assert v["VGPRs"] + v.get("AGPRs", 0) <= 64, (name, f, v)      # eight waves per SIMD: the kernel is bound by memory, not registers


def test_k_resolve_rgba_uses_no_lds_and_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    pairs = [(1, 2), (2, 1), (2, 2), (4, 2), (8, 8)]
    inst = "".join(f"template __global__ void swr::k_resolve_rgba<{kx}, {ky}>(const float4*, float4*, uint32_t, uint32_t);\n" for kx, ky in pairs)
    usage = _remarks(tmp_path, "resolve_rgba", '#include "swr_post.hip.h"\n' + inst)
    for kx, ky in pairs:
        v = usage[f"swr::k_resolve_rgba<{kx}, {ky}>"]
        assert v["LDS"] == 0 and v["ScratchSize"] == 0, (kx, ky, v)
