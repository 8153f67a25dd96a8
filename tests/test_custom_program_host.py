"""User fragment programs: the run-time compile step alone (swr_program_validate needs neither a context nor a GPU).

The library compiles the program for gfx950 with hiprtc, which it opens with dlopen; the CPU suite checks that the contract's
prelude, the embedded kernel headers and the user's text compile together, and that errors come back with the compiler's log."""
import ctypes

import pytest

from softwarerenderer_amd import _native as N

# Renderer.FragmentShader (Renderer.cs:848-860) against the contract of include/swr.h
DUST2 = r"""
__device__ float4 swr_fragment(const swr_fs_in& in, const swr_fs_env& env) {
    const swr_uniforms& u = env.uniforms;
    const float3 to_light = make_float3(-u.light_direction[0], -u.light_direction[1], -u.light_direction[2]);
    const float diffuse = swr_max(0.25f, swr_dot3(in.world_normal, to_light));
    const float4 tc = swr_sample(env, in.tex_coord);
    const float4 base = make_float4(in.color.x * tc.x, in.color.y * tc.y, in.color.z * tc.z, in.color.w * tc.w);
    float fog = swr_clamp((u.fog_end - in.clip_position.z) / (u.fog_end - u.fog_start), 0.0f, 1.0f);
    fog = fog * fog * (3.0f - 2.0f * fog);
    const float s = 0.1f + 0.9f * diffuse;
    return make_float4(swr_lerp(u.fog_color[0], base.x * s * u.light_color[0], fog),
                       swr_lerp(u.fog_color[1], base.y * s * u.light_color[1], fog),
                       swr_lerp(u.fog_color[2], base.z * s * u.light_color[2], fog), base.w);
}
"""


@pytest.fixture(scope="module")
def lib():
    return N.load()


def validate(lib, src):
    log = ctypes.create_string_buffer(1 << 16)
    rc = lib.swr_program_validate(src.encode(), log, len(log))
    return rc, log.value.decode(errors="replace")


def test_validate_accepts_the_dust2_restatement(lib):
    rc, log = validate(lib, DUST2)
    assert rc == N.SWR_OK, log


def test_validate_rejects_a_syntax_error_with_its_line(lib):
    src = DUST2.replace("fog = fog * fog * (3.0f - 2.0f * fog);", "fog = fog * fog * (3.0f - 2.0f * fog)\n    fog +;")
    line = src.splitlines().index("    fog +;") + 1
    rc, log = validate(lib, src)
    assert rc == N.SWR_ERR_INVALID_ARG
    assert f"fragment.hip:{line - 1}:" in log or f"fragment.hip:{line}:" in log, log


def test_validate_rejects_a_source_without_swr_fragment(lib):
    rc, log = validate(lib, "__device__ float4 shade(const swr_fs_in& in) { return in.color; }\n")
    assert rc == N.SWR_ERR_INVALID_ARG
    assert "swr_fragment" in log, log


def test_validate_truncates_the_log_to_the_buffer(lib):
    buf = ctypes.create_string_buffer(16)
    assert lib.swr_program_validate(b"this is not C++", buf, 16) == N.SWR_ERR_INVALID_ARG
    assert 0 < len(buf.value) <= 15


def test_user_program_entry_points_are_exported(lib):
    for name in ("swr_program_create", "swr_program_destroy", "swr_program_set_constants", "swr_program_validate"):
        assert name in N.EXPORTS and hasattr(lib, name)
